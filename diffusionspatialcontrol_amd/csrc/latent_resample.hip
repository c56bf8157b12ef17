// The step between the two passes of a hires request (dsc_latent_resample_noise): the final latent rows of the base pass are
// enlarged to the target latent size and the start noise of the second pass is added, in one launch - what the reference does
// with F.interpolate on an fp32 copy (modules/model_k_diffusion.py:1179-1191), `.to(fp16)`, and img2img's
// `latents + noise * sqrt(sigma_0^2 + 1)` (:647).  All six interpolate modes arrive as separable tap tables (four source indices
// and weights per output coordinate and axis, modules/latent_resample.py), so the kernel does not know the mode.
//
// At most 4 x 256 x 256 outputs: memory- and launch-bound.  One thread per destination piece - 8 halfs stored as one 16-byte
// vector when every row piece is whole and aligned (W % 8 == 0 and dst, noise 16-byte aligned), else one half - with the 16
// source samples of each output read through the cache (the source row set is a few KB).  fp32 accumulation in a fixed order -
// per source row the four taps of x (a product, then three fmas), then the four rows along y the same way: the order of torch's
// own CPU kernels, so that with the tables' weights the fp32 value is torch's - then one fp16 rounding of the resampled value,
// one of the scaled noise, one of their sum: the roundings of the torch expressions on fp16 tensors.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

typedef int i4_t __attribute__((ext_vector_type(4)));

template <int P>
__global__ __launch_bounds__(256) void latent_resample_kernel(const half_t* __restrict__ src, const half_t* __restrict__ noise,
                                                              half_t* __restrict__ dst, int rows, int h, int w, int H, int W,
                                                              const i4_t* __restrict__ idx_y, const f4x_t* __restrict__ w_y,
                                                              const i4_t* __restrict__ idx_x, const f4x_t* __restrict__ w_x, float s) {
    const int ppr = W / P;                                       // pieces per destination row (P == 8 only when W % 8 == 0)
    const int piece = blockIdx.x * 256 + threadIdx.x;
    if (piece >= rows * ppr) return;
    const int row = piece / ppr, px = piece - row * ppr;         // row = (image * C + channel) * H + y
    const int nc = row / H, y = row - nc * H;
    const half_t* sp = src + (long long)nc * h * w;
    const i4_t iy = idx_y[y];
    const f4x_t wy = w_y[y];
    const half_t* rp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rp[i] = sp + min(max(iy[i], 0), h - 1) * w;      // never outside the source plane
    const long long o0 = (long long)row * W + px * P;
    half_t res[P];
#pragma unroll
    for (int e = 0; e < P; ++e) {
        const int x = px * P + e;
        const i4_t ix = idx_x[x];
        const f4x_t wx = w_x[x];
        int xi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xi[j] = min(max(ix[j], 0), w - 1);
        // torch's order (UpSampleKernel.cpp: along x inside each source row, then along y), every step after a row's / the
        // column's first product one fma; the table's tap order is the evaluation order
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float t = (float)rp[i][xi[0]] * wx[0];
#pragma unroll
            for (int j = 1; j < 4; ++j) t = fmaf((float)rp[i][xi[j]], wx[j], t);
            acc = i == 0 ? t * wy[0] : fmaf(t, wy[i], acc);
        }
        // the fp32 rounding of the sum is part of the contract (torch rounds to fp32, then `.to(fp16)`): keep the compiler from
        // folding the last fma and the conversion into one single-rounding v_fma_mixlo_f16 (seen in the 2-byte-store variant)
        asm volatile("" : "+v"(acc));
        res[e] = (half_t)acc;
    }
    if (noise) {
        half_t nz[P];
        if (P == 8) {
            const h8_t nv = *reinterpret_cast<const h8_t*>(noise + o0);
#pragma unroll
            for (int e = 0; e < P; ++e) nz[e] = nv[e];
        } else {
            nz[0] = noise[o0];
        }
#pragma unroll
        for (int e = 0; e < P; ++e) {
            const half_t scaled = (half_t)((float)nz[e] * s);                      // fp16 tensor * fp16 scalar
            res[e] = (half_t)((float)res[e] + (float)scaled);                      // fp16 tensor + fp16 tensor
        }
    }
    if (P == 8) {
        h8_t ov;
#pragma unroll
        for (int e = 0; e < P; ++e) ov[e] = res[e];
        *reinterpret_cast<h8_t*>(dst + o0) = ov;
    } else {
        dst[o0] = res[0];
    }
}

}  // namespace

extern "C" int dsc_latent_resample_noise(const void* src, const void* noise, void* dst, int n, int C, int h, int w, int H, int W,
                                         const int* idx_y, const float* w_y, const int* idx_x, const float* w_x,
                                         float noise_scale_f16_value, void* stream) {
    if (!src || !dst || dst == src || !idx_y || !w_y || !idx_x || !w_x) return DSC_ERR_BAD_ARG;
    if (n < 1 || C < 1 || h < 1 || w < 1 || H < h || W < w) return DSC_ERR_BAD_ARG;
    const long long rows = (long long)n * C * H;
    if (rows * W >= (1ll << 31) || (long long)n * C * h * w >= (1ll << 31)) return DSC_ERR_UNSUPPORTED;
    const uintptr_t tabs = reinterpret_cast<uintptr_t>(idx_y) | reinterpret_cast<uintptr_t>(w_y) |
                           reinterpret_cast<uintptr_t>(idx_x) | reinterpret_cast<uintptr_t>(w_x);
    if (tabs & 15) return DSC_ERR_UNSUPPORTED;                    // one 16-byte row of four taps per coordinate
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(noise) | reinterpret_cast<uintptr_t>(dst)) & 1)
        return DSC_ERR_UNSUPPORTED;
    // 16-byte stores where every destination row piece is whole and aligned: rows start at multiples of W halfs from dst
    const bool wide = W % 8 == 0 && !((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(noise)) & 15);
    const long long pieces = rows * (wide ? W / 8 : W);
    const dim3 grid((unsigned)((pieces + 255) / 256)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const half_t* sp = static_cast<const half_t*>(src); const half_t* np = static_cast<const half_t*>(noise);
    half_t* dp = static_cast<half_t*>(dst);
    const i4_t* iy = reinterpret_cast<const i4_t*>(idx_y); const f4x_t* wy = reinterpret_cast<const f4x_t*>(w_y);
    const i4_t* ix = reinterpret_cast<const i4_t*>(idx_x); const f4x_t* wx = reinterpret_cast<const f4x_t*>(w_x);
    if (wide)
        DSC_LAUNCH(latent_resample_kernel<8>, grid, block, 0, st, sp, np, dp, (int)rows, h, w, H, W, iy, wy, ix, wx, noise_scale_f16_value);
    else
        DSC_LAUNCH(latent_resample_kernel<1>, grid, block, 0, st, sp, np, dp, (int)rows, h, w, H, W, iy, wy, ix, wx, noise_scale_f16_value);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
