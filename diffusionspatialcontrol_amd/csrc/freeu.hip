// FreeU (arXiv 2309.11497) on one up-block ResNet's inputs, per batch row, in one launch (dsc_freeu_rows_f16): what diffusers'
// `apply_freeu` does before the ResNet concatenates `hidden` with the skip tensor (the reference UNet enables it through
// modules/u_net_condition_modify.py:835-865 `enable_freeu` / `disable_freeu`, its up blocks built with `resolution_idx`, :445):
//     hidden[r][:, :C_h/2] *= b[r]                           fp16( fp32( fp32(x) * b ) )
//     skip[r] = fourier_filter(skip[r], threshold 1, s[r])   fftn, fftshift, the centre 2x2 block times s, and back
// with (s, b) read per batch row from DEVICE memory, so that one captured launch serves rows with and without FreeU.
//
// The filter touches the frequencies {0, -1} x {0, -1} only, so it is no FFT: per image and channel, with th = 2 pi h / H and
// tw = 2 pi w / W, seven sums
//     S0 = sum x             Ach = sum x cos th    Ash = sum x sin th    Acw = sum x cos tw    Asw = sum x sin tw
//     Ac2 = sum x cos(th+tw) As2 = sum x sin(th+tw)
// and one streaming pass
//     out = x + (s - 1) / (H W) * [S0 + Ach cos th + Ash sin th + Acw cos tw + Asw sin tw + Ac2 cos(th+tw) + As2 sin(th+tw)]
// (a side of 2, where -1 and +1 are one frequency, included: at 2x2 this is s * x.  A side of 1 is refused: diffusers' slice
// covers something else there.)
//
// One workgroup owns ALL H * W pixels of kVecs 8-channel vectors of one batch row: 256 lanes = kSlices pixel slices x kVecs
// vectors, a lane walking pixels slice, slice + kSlices, ...  Sums: per lane in that fixed order, then a butterfly over the 16
// slices of a wave, then the four waves' partials through LDS added in wave order - no atomics, the same bits every run.
// The sums, the cos / sin values and the formula are fp64, rounded once at the end: with the paper's s2 = 0.2 the result
// x - 0.8 * (low frequencies) crosses zero, and there fp32 sums of a stream with a DC offset of 5 were up to 9 fp16 ulps off
// (measured; 0.1 % of the elements), while the kernel is latency-bound either way (GroupNorm's statistics are fp64 for the
// same reason).
// A barrier separates the summing pass from the writing pass, and no other workgroup reads these channels: in place is safe.  The
// second read of the slab (64 bytes x H x W per workgroup) is served by the caches.  cos / sin of th and tw are built once per
// workgroup (H + W sincospi calls) in LDS.
// The workgroups behind the skip tensor's scale the hidden tensor's first half, as gated_add.hip streams its rows.
// The batch row is the grid's second dimension: a row's (s, b) are wave-uniform loads and "s == 1" / "b == 1" uniform branches
// taken before anything else is loaded - such a row is neither read nor written and may hold anything.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

constexpr int kVecs = 4;                       // 8-channel vectors per workgroup: 64 contiguous bytes per pixel
constexpr int kSlices = 256 / kVecs;           // pixel slices per workgroup
constexpr int kSums = 7;
constexpr int kMaxSide = DSC_FREEU_MAX_SIDE;   // the cos / sin tables in LDS
constexpr int kHiddenBlocks = 64;              // workgroups per batch row that scale the hidden half, at most

__global__ __launch_bounds__(256) void freeu_rows_kernel(h8_t* hidden, int C_h, h8_t* skip, int C_s, int H, int W,
                                                         const float* params, int stage, int skip_blocks) {
    __shared__ double tab_ch[kMaxSide], tab_sh[kMaxSide], tab_cw[kMaxSide], tab_sw[kMaxSide];
    __shared__ double part[4][kVecs][kSums * 8];
    const int r = blockIdx.y, t = threadIdx.x;
    const int HW = H * W;

    if ((int)blockIdx.x >= skip_blocks) {        // ---- hidden[r][:, :C_h/2] *= b
        const float b = params[4 * r + 2 + stage];
        if (b == 1.f) return;
        const int hv = C_h / 16, cv = C_h / 8;   // vectors of a pixel's first half / of a whole pixel
        h8_t* row = hidden + (long long)r * HW * cv;
        const long long total = (long long)HW * hv;
        const int stride = ((int)gridDim.x - skip_blocks) * 256;
        for (long long i = ((int)blockIdx.x - skip_blocks) * 256 + t; i < total; i += stride) {
            const long long p = i / hv, v = i - p * hv;
            h8_t* at = row + p * cv + v;
            const h8_t xv = *at;
            h8_t ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float acc = (float)xv[e] * b;
                // the product rounded to fp32 and THEN to fp16 is the contract (torch's fp16 `x * b` on the CPU, `(x.float() *
                // b).half()` anywhere): keep the multiply and the conversion two instructions, as gated_add.hip does - fused into
                // one mixed-precision instruction the product would be rounded once, which differs in about one element of 60
                asm volatile("" : "+v"(acc));
                ov[e] = (half_t)acc;
            }
            *at = ov;
        }
        return;
    }

    // ---- skip[r] = fourier_filter(skip[r], 1, s)
    const float s = params[4 * r + stage];
    if (s == 1.f) return;
    for (int i = t; i < H + W; i += 256) {
        double sn, cs;
        if (i < H) { sincospi(2.0 * (double)i / (double)H, &sn, &cs); tab_ch[i] = cs; tab_sh[i] = sn; }
        else { sincospi(2.0 * (double)(i - H) / (double)W, &sn, &cs); tab_cw[i - H] = cs; tab_sw[i - H] = sn; }
    }
    __syncthreads();

    const int nvec = C_s / 8;
    const int v = t % kVecs, slice = t / kVecs;
    const int vec = blockIdx.x * kVecs + v;
    const bool live = vec < nvec;                // (the last workgroup of a row when nvec % kVecs != 0)
    h8_t* base = skip + (long long)r * HW * nvec + (live ? vec : 0);

    double acc[kSums][8];
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.0;
    if (live) {
        for (int p = slice; p < HW; p += kSlices) {
            const int h = p / W, w = p - h * W;
            const double ch = tab_ch[h], sh = tab_sh[h], cw = tab_cw[w], sw = tab_sw[w];
            const double c2 = ch * cw - sh * sw, s2 = sh * cw + ch * sw;
            const h8_t xv = base[(long long)p * nvec];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double x = (double)(float)xv[e];
                acc[0][e] += x;
                acc[1][e] = fma(x, ch, acc[1][e]);
                acc[2][e] = fma(x, sh, acc[2][e]);
                acc[3][e] = fma(x, cw, acc[3][e]);
                acc[4][e] = fma(x, sw, acc[4][e]);
                acc[5][e] = fma(x, c2, acc[5][e]);
                acc[6][e] = fma(x, s2, acc[6][e]);
            }
        }
    }
    // the 16 slices of a wave (lanes v, v + 4, ..., v + 60): a butterfly, every lane ends with the wave's sum
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            double a = acc[k][e];
#pragma unroll
            for (int o = kVecs; o < DSC_WAVE; o <<= 1) a += __shfl_xor(a, o, DSC_WAVE);
            acc[k][e] = a;
        }
    const int wave = t / DSC_WAVE, lane = t % DSC_WAVE;
    if (lane < kVecs) {
#pragma unroll
        for (int k = 0; k < kSums; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) part[wave][lane][k * 8 + e] = acc[k][e];
    }
    __syncthreads();                             // every lane's reads of the slab are done before this barrier; the writes come after it
    if (!live) return;
    const double f = ((double)s - 1.0) / (double)HW;
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            acc[k][e] = ((part[0][v][k * 8 + e] + part[1][v][k * 8 + e]) + part[2][v][k * 8 + e]) + part[3][v][k * 8 + e];
    for (int p = slice; p < HW; p += kSlices) {
        const int h = p / W, w = p - h * W;
        const double ch = tab_ch[h], sh = tab_sh[h], cw = tab_cw[w], sw = tab_sw[w];
        const double c2 = ch * cw - sh * sw, s2 = sh * cw + ch * sw;
        h8_t* at = base + (long long)p * nvec;
        const h8_t xv = *at;
        h8_t ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            double low = acc[0][e];
            low = fma(acc[1][e], ch, low);
            low = fma(acc[2][e], sh, low);
            low = fma(acc[3][e], cw, low);
            low = fma(acc[4][e], sw, low);
            low = fma(acc[5][e], c2, low);
            low = fma(acc[6][e], s2, low);
            ov[e] = (half_t)fma(f, low, (double)(float)xv[e]);
        }
        *at = ov;
    }
}

bool overlap(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

}  // namespace

extern "C" int dsc_freeu_rows_f16(void* hidden, int C_h, void* skip, int C_s, int B, int H, int W, const float* params, int stage,
                                  void* stream) {
    if (!hidden || !skip || !params) return DSC_ERR_BAD_ARG;
    if (B < 1 || H < 2 || W < 2 || C_h < 1 || C_s < 1 || (stage != 0 && stage != 1)) return DSC_ERR_BAD_ARG;
    if (H > kMaxSide || W > kMaxSide) return DSC_ERR_UNSUPPORTED;        // (so H * W * C / 8 of one row stays far inside an int)
    if (C_s % 8 != 0 || C_h % 16 != 0 || C_h > (1 << 20) || C_s > (1 << 20)) return DSC_ERR_UNSUPPORTED;
    if (B > 65535) return DSC_ERR_UNSUPPORTED;                             // the batch row is gridDim.y
    const uintptr_t ha = reinterpret_cast<uintptr_t>(hidden), sa = reinterpret_cast<uintptr_t>(skip);
    const uintptr_t pa = reinterpret_cast<uintptr_t>(params);
    if (((ha | sa) & 15) || (pa & 3)) return DSC_ERR_UNSUPPORTED;
    const uintptr_t px = (uintptr_t)B * (uintptr_t)H * (uintptr_t)W;
    const uintptr_t h_bytes = px * (uintptr_t)C_h * 2, s_bytes = px * (uintptr_t)C_s * 2, p_bytes = (uintptr_t)B * 16;
    if (overlap(ha, h_bytes, sa, s_bytes) || overlap(ha, h_bytes, pa, p_bytes) || overlap(sa, s_bytes, pa, p_bytes))
        return DSC_ERR_BAD_ARG;
    const int skip_blocks = (C_s / 8 + kVecs - 1) / kVecs;
    const long long hid_pieces = (long long)H * W * (C_h / 16);
    const long long want = (hid_pieces + 255) / 256;
    const int hid_blocks = (int)(want < kHiddenBlocks ? want : kHiddenBlocks);
    const dim3 grid((unsigned)(skip_blocks + hid_blocks), (unsigned)B), block(256);
    DSC_LAUNCH(freeu_rows_kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<h8_t*>(hidden), C_h,
               static_cast<h8_t*>(skip), C_s, H, W, params, stage, skip_blocks);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
