// The first steps of a served pixel input, the reverse direction of image_finish.hip: two launches around the VAE encoder's
// captured graph on the encode lane of the continuous batcher (modules/serving/encode_lane.py).
//
// dsc_image_prepare: up to 16 request images become what `vae.encode` and the sampler step read, in one launch - what the
// reference does with VaeImageProcessor.preprocess (modules/model_k_diffusion.py:1447-1449, :1480-1482: bytes / 255, `2 x - 1`,
// channel-major float32; masks binarised at 0.5), `init_image * (mask < 0.5)` (:1480-1482's masked image), the conversion to the
// VAE's fp16 and `F.interpolate(mask, size=(h, w))` (:1253-1257, default nearest: pixel (8 i, 8 j)).  Per element:
//     uint8 image:    v = 2.0f * (float(b) / 255.0f) - 1.0f     (an IEEE division; 2 q is exact, so the fma the compiler may form
//                                                                 of `2 q - 1` rounds as the product and the difference do)
//     float32 image:  v = x
//     image out:      fp16(v)
//     mask:           m = b >= 128  (uint8)   /   m = x >= 0.5f  (float32; a NaN compares false: 0)
//     masked out:     fp16(v * (m ? 0.0f : 1.0f))                (the literal fp32 product: -0.0 under a negative v)
//     latent mask:    fp16(m) of pixel (8 i, 8 j), written `rep` times
// Memory-bound and small (0.75 MB in, 1.5 MB out per 512x512 uint8 image): no LDS.  Both sides are multiples of 8, so H * W is
// a multiple of 64 and one lane owns 16 consecutive pixels of the dense plane: 48 interleaved bytes at a 16-byte-aligned address
// as three 16-byte loads, split into three planes in registers (or 64 bytes per channel plane as four 16-byte loads of float32),
// and per channel 32 bytes out as two 16-byte stores.  Each half of the 16 starts at a multiple of 8, inside one image row at a
// column that is a multiple of 8: when its row is one too, its first pixel is a latent-mask sample, which the same lane stores.
// The rows ride in the kernel arguments, like the step records of sampler.hip; a row that asks for nothing forms no address.
//
// dsc_latent_start_rows: after the encode, every row of it in one launch - DiagonalGaussianDistribution.sample times the scaling
// factor (:1234-1246, _encode_vae_image) and the start latent of its kind (:647 img2img; :1306-1362 prepare_latents_inpating),
// with an fp16 rounding wherever the torch chain has a tensor:
//     lv  = clamp(logvar, -30, 20)                 (fp16: both bounds are fp16 values)
//     std = fp16(expf(float(fp16(0.5f * lv))))     (torch evaluates a half exp in fp32 and rounds once)
//     lat = fp16(scaling * float(fp16(mean + fp16(std * eps))))
//     DSC_START_ADD:    start = fp16(lat + fp16(noise * coef))      (img2img: coef = fp16 sqrt(sigma_0^2 + 1); inpainting below
//                                                                     strength 1: coef = sigma_0)
//     DSC_START_SCALE:  start = fp16(noise * coef)                  (inpainting at strength 1: coef = fp32(sqrt(sigma_0^2 + 1)))
//     DSC_START_NONE:   no start latent                             (the masked image of a 9-channel request)
// `keep` (optional) receives lat: r.known["image"] of 4-channel inpainting, rows 1..4 of r.extra for a masked-image row.
// `keep_noise` (optional) receives the noise row as it is.  A conversion to fp16 between a product and a sum does NOT keep the
// compiler from fusing them: the product of two halfs is exact in fp32, so it narrows `fp16(float(a) * float(b))` to a half
// multiply, the sum likewise, and contracts the pair into one half fma - one rounding where torch has two (measured: 2 % of the
// latents off by an ulp over every logvar).  pin_f32 (sampler.hip's as_f32) materialises each product in fp32.
// One lane owns 8 consecutive halfs of a row's 4 h w: 16-byte loads and stores when 4 h w is a multiple of 8 and every pointer is
// 16-byte aligned, element by element with a bound check otherwise (h w odd, or 2 mod 4).
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

typedef unsigned u4_t __attribute__((ext_vector_type(4)));

struct PrepareArgs {
    dsc_image_prepare_row rows[DSC_IMAGE_PREPARE_MAX_ROWS];
};

struct StartArgs {
    dsc_latent_start_row rows[DSC_IMAGE_PREPARE_MAX_ROWS];
};

__device__ __forceinline__ float byte_value(unsigned b) { return 2.0f * ((float)b / 255.0f) - 1.0f; }

__global__ __launch_bounds__(256) void image_prepare_kernel(int plane_pieces, int W, const PrepareArgs a) {
    const dsc_image_prepare_row& r = a.rows[blockIdx.y];               // (uniform: scalar loads of the kernel arguments)
    const bool want_img = r.out_image != nullptr, want_masked = r.out_masked != nullptr, want_lm = r.out_mask != nullptr;
    if (!want_img && !want_masked && !want_lm) return;
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= plane_pieces) return;
    const long long px = at * 16;                                      // first of this lane's 16 pixels of the dense plane
    const long long plane = (long long)plane_pieces * 16;              // H * W
    float v[3][16];
    if (want_img || want_masked) {
        if (r.image_kind == DSC_PIXELS_U8) {
            const u4_t* src = reinterpret_cast<const u4_t*>(static_cast<const unsigned char*>(r.image) + px * 3);
            unsigned wd[12];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const u4_t q = src[k];
#pragma unroll
                for (int j = 0; j < 4; ++j) wd[4 * k + j] = q[j];
            }
#pragma unroll
            for (int e = 0; e < 16; ++e)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int byte = 3 * e + c;
                    v[c][e] = byte_value((wd[byte / 4] >> (8 * (byte % 4))) & 0xffu);
                }
        } else {
            const float* src = static_cast<const float*>(r.image) + px;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const f4x_t q = *reinterpret_cast<const f4x_t*>(src + c * plane + 4 * k);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[c][4 * k + j] = q[j];
                }
        }
    }
    bool m[16];
    if (want_masked || want_lm) {
        if (r.mask_kind == DSC_PIXELS_U8) {
            const u4_t q = *reinterpret_cast<const u4_t*>(static_cast<const unsigned char*>(r.mask) + px);
#pragma unroll
            for (int e = 0; e < 16; ++e) m[e] = ((q[e / 4] >> (8 * (e % 4))) & 0xffu) >= 128u;
        } else {
            const float* src = static_cast<const float*>(r.mask) + px;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f4x_t q = *reinterpret_cast<const f4x_t*>(src + 4 * k);
#pragma unroll
                for (int j = 0; j < 4; ++j) m[4 * k + j] = q[j] >= 0.5f;
            }
        }
    }
    if (want_img) {
        half_t* dst = static_cast<half_t*>(r.out_image) + px;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                h8_t o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (half_t)v[c][8 * k + e];
                *reinterpret_cast<h8_t*>(dst + c * plane + 8 * k) = o;
            }
    }
    if (want_masked) {
        half_t* dst = static_cast<half_t*>(r.out_masked) + px;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                h8_t o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (half_t)(v[c][8 * k + e] * (m[8 * k + e] ? 0.0f : 1.0f));
                *reinterpret_cast<h8_t*>(dst + c * plane + 8 * k) = o;
            }
    }
    if (want_lm) {
        const int w8 = W / 8;
        const long long lplane = plane / 64;                           // (H / 8) * (W / 8)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long long p = px + 8 * k;                            // a multiple of 8: column x is one too
            const long long y = p / W;
            if (y % 8 == 0) {
                const long long x = p - y * W;
                half_t* dst = static_cast<half_t*>(r.out_mask) + (y / 8) * w8 + x / 8;
                const half_t val = m[8 * k] ? (half_t)1.0f : (half_t)0.0f;
                for (int q = 0; q < r.mask_rep; ++q) dst[q * lplane] = val;
            }
        }
    }
}

// an fp32 value the compiler must materialise: the product stays an fp32 multiply with a rounding of its own
__device__ __forceinline__ float pin_f32(float v) {
    __asm__ volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ half_t latent_value(half_t mean, half_t logvar, half_t eps, float scaling) {
    half_t lv = logvar < (half_t)-30.0f ? (half_t)-30.0f : logvar;     // torch.clamp(logvar, -30.0, 20.0)
    lv = lv > (half_t)20.0f ? (half_t)20.0f : lv;
    const half_t halved = (half_t)pin_f32(0.5f * (float)lv);
    const half_t std = (half_t)expf((float)halved);
    const half_t se = (half_t)pin_f32((float)std * (float)eps);
    const half_t z = (half_t)((float)mean + (float)se);
    return (half_t)pin_f32(scaling * (float)z);
}

__device__ __forceinline__ half_t start_value(int kind, half_t lat, half_t noise, float coef) {
    const half_t scaled = (half_t)pin_f32((float)noise * coef);
    return kind == DSC_START_ADD ? (half_t)((float)lat + (float)scaled) : scaled;
}

template <bool kVec>
__global__ __launch_bounds__(256) void latent_start_kernel(const half_t* __restrict__ moments, int row_elems, const StartArgs a) {
    const dsc_latent_start_row& r = a.rows[blockIdx.y];
    if (r.kind == DSC_START_IDLE) return;
    const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (e0 >= row_elems) return;
    const half_t* mean = moments + (long long)r.moments_row * 2 * row_elems + e0;
    const half_t* logvar = mean + row_elems;
    const half_t* eps = static_cast<const half_t*>(r.eps) + e0;
    const half_t* noise = r.noise ? static_cast<const half_t*>(r.noise) + e0 : nullptr;
    half_t* start = r.kind != DSC_START_NONE ? static_cast<half_t*>(r.start) + e0 : nullptr;
    half_t* keep = r.keep ? static_cast<half_t*>(r.keep) + e0 : nullptr;
    half_t* keep_noise = r.keep_noise ? static_cast<half_t*>(r.keep_noise) + e0 : nullptr;
    if (kVec) {
        const h8_t mu = *reinterpret_cast<const h8_t*>(mean), lv = *reinterpret_cast<const h8_t*>(logvar);
        const h8_t ep = *reinterpret_cast<const h8_t*>(eps);
        h8_t nz = {};
        if (noise) nz = *reinterpret_cast<const h8_t*>(noise);
        h8_t lat, st;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            lat[e] = latent_value(mu[e], lv[e], ep[e], r.scaling);
            st[e] = start_value(r.kind, lat[e], nz[e], r.coef);
        }
        if (start) *reinterpret_cast<h8_t*>(start) = st;
        if (keep) *reinterpret_cast<h8_t*>(keep) = lat;
        if (keep_noise) *reinterpret_cast<h8_t*>(keep_noise) = nz;
    } else {
        const int left = (int)(row_elems - e0 < 8 ? row_elems - e0 : 8);
        for (int e = 0; e < left; ++e) {
            const half_t lat = latent_value(mean[e], logvar[e], eps[e], r.scaling);
            const half_t nz = noise ? noise[e] : (half_t)0.0f;
            if (start) start[e] = start_value(r.kind, lat, nz, r.coef);
            if (keep) keep[e] = lat;
            if (keep_noise) keep_noise[e] = nz;
        }
    }
}

bool pixels_kind(int k) { return k == DSC_PIXELS_U8 || k == DSC_PIXELS_F32; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int dsc_image_prepare(const dsc_image_prepare_row* rows, int n, int H, int W, void* stream) {
    if (!rows || n < 1 || n > DSC_IMAGE_PREPARE_MAX_ROWS || H < 1 || W < 1) return DSC_ERR_BAD_ARG;
    bool any = false;
    for (int j = 0; j < n; ++j) {
        const dsc_image_prepare_row& r = rows[j];
        const bool img = r.out_image || r.out_masked, msk = r.out_masked || r.out_mask;
        if (img && (!r.image || !pixels_kind(r.image_kind))) return DSC_ERR_BAD_ARG;
        if (msk && (!r.mask || !pixels_kind(r.mask_kind))) return DSC_ERR_BAD_ARG;
        if (r.out_mask && r.mask_rep != 1 && r.mask_rep != 4) return DSC_ERR_BAD_ARG;
        if (r.out_image && r.out_image == r.out_masked) return DSC_ERR_BAD_ARG;
        any = any || img || msk;
    }
    if (H % 8 != 0 || W % 8 != 0) return DSC_ERR_UNSUPPORTED;
    const long long plane_pieces = (long long)H * W / 16;
    if (plane_pieces >= (1ll << 31) - 256) return DSC_ERR_UNSUPPORTED;
    PrepareArgs a = {};
    for (int j = 0; j < n; ++j) {
        const dsc_image_prepare_row& r = rows[j];
        const bool img = r.out_image || r.out_masked, msk = r.out_masked || r.out_mask;
        // every vector access is 16 bytes at a multiple of 16 bytes from its base; the latent mask is written half by half
        if (img && !aligned16(r.image)) return DSC_ERR_UNSUPPORTED;
        if (msk && !aligned16(r.mask)) return DSC_ERR_UNSUPPORTED;
        if (!aligned16(r.out_image) || !aligned16(r.out_masked)) return DSC_ERR_UNSUPPORTED;
        if (reinterpret_cast<uintptr_t>(r.out_mask) & 1) return DSC_ERR_UNSUPPORTED;
        a.rows[j] = r;
    }
    if (!any) return DSC_OK;                                           // nobody asked for anything: no launch
    const dim3 grid((unsigned)((plane_pieces + 255) / 256), (unsigned)n), block(256);
    DSC_LAUNCH(image_prepare_kernel, grid, block, 0, static_cast<hipStream_t>(stream), (int)plane_pieces, W, a);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_latent_start_rows(const void* moments, int m, const dsc_latent_start_row* rows, int n, int h, int w,
                                     void* stream) {
    if (!moments || !rows || m < 1 || n < 1 || n > DSC_IMAGE_PREPARE_MAX_ROWS || h < 1 || w < 1) return DSC_ERR_BAD_ARG;
    const long long row_elems = 4ll * h * w;
    if (row_elems >= (1ll << 30)) return DSC_ERR_UNSUPPORTED;
    bool any = false, vec = row_elems % 8 == 0 && aligned16(moments);
    StartArgs a = {};
    for (int j = 0; j < n; ++j) {
        const dsc_latent_start_row& r = rows[j];
        if (r.kind == DSC_START_IDLE) continue;
        if (r.kind != DSC_START_ADD && r.kind != DSC_START_SCALE && r.kind != DSC_START_NONE) return DSC_ERR_BAD_ARG;
        if (r.moments_row < 0 || r.moments_row >= m || !r.eps) return DSC_ERR_BAD_ARG;
        if (r.kind != DSC_START_NONE && (!r.noise || !r.start)) return DSC_ERR_BAD_ARG;
        if (r.kind == DSC_START_NONE && !r.keep) return DSC_ERR_BAD_ARG;          // (a row that would write nothing)
        if (r.keep_noise && !r.noise) return DSC_ERR_BAD_ARG;
        if (r.start && (r.start == r.keep || r.start == r.keep_noise)) return DSC_ERR_BAD_ARG;
        if (r.keep && r.keep == r.keep_noise) return DSC_ERR_BAD_ARG;
        const void* ptrs[] = {r.eps, r.noise, r.start, r.keep, r.keep_noise};
        for (const void* p : ptrs) {
            if (reinterpret_cast<uintptr_t>(p) & 1) return DSC_ERR_UNSUPPORTED;
            vec = vec && aligned16(p);
        }
        a.rows[j] = r;
        any = true;
    }
    if (reinterpret_cast<uintptr_t>(moments) & 1) return DSC_ERR_UNSUPPORTED;
    if (!any) return DSC_OK;
    const long long pieces = (row_elems + 7) / 8;
    const dim3 grid((unsigned)((pieces + 255) / 256), (unsigned)n), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const half_t* mp = static_cast<const half_t*>(moments);
    if (vec)
        DSC_LAUNCH(latent_start_kernel<true>, grid, block, 0, st, mp, (int)row_elems, a);
    else
        DSC_LAUNCH(latent_start_kernel<false>, grid, block, 0, st, mp, (int)row_elems, a);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
