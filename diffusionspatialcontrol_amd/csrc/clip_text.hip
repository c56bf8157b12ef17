// The two kernels the CLIP text encoder needs beside the GEMM and the LayerNorm (modules/clip_text.py): causal self-attention
// over one text chunk (dsc_causal_attn_f16) and the feed-forward activation between fc1 and fc2 (dsc_act_f16).
//
// dsc_causal_attn_f16:  out[b, i, h, :] = softmax_{j <= i}(scale * q[b, i, h, :] . k[b, j, h, :]) . v[b, j, h, :]
// CLIP attention is 77 tokens of 64 channels over 12 - 20 heads: nothing like the thousands of queries dsc_self_attn_fwd is tiled
// for.  One workgroup per (b, h), five waves, wave w owns the 16 queries [16 w, 16 w + 16):
//   stage       K of the head -> LDS [80][64] (rows padded to 72 halfs), V -> LDS transposed [64][80] (rows padded to 88), both as
//               16-byte global reads; rows >= S are ZEROS, never read from memory (a NaN behind the operand must not meet p = 0)
//   S^T = K Q^T v_mfma_f32_16x16x32_f16, two steps per 16-key tile (d = 64); lane (r = lane & 15, g = lane >> 4) holds
//               K[16 kt + r][32 s + 8 g ..+8] (one 16-byte LDS read) and Q[16 w + r][32 s + 8 g ..+8] (one 16-byte global read); the
//               accumulator holds keys 16 kt + 4 g + i (i < 4) of query r.  Key tiles kt > w lie wholly above the diagonal: skipped.
//   softmax     key t of query l counts when t <= l (index mask; l < S implies t < S).  Maximum and sum over the lane's <= 20
//               values, then xor-shuffles 16 and 32; fp32.  The sum is of the fp16-ROUNDED probabilities the next product reads,
//               so the weights of a row add up to one whatever the rounding did, and a row with one key is exactly 1 * v.
//   O^T = V^T P^T v_mfma_f32_16x16x16_f16: its B operand (k = 4 g + i, column r) IS the accumulator layout above - probabilities go
//               from registers to registers.  Row 4 g' + i of call u is channel 32 m + 8 g' + 4 u + i (csrc/ip_xattn.hip's
//               permutation), so lane (r, g) ends up with the 8 consecutive channels 32 m + 8 g ..+8 of query r: one 16-byte store.
//               The A operand is one 8-byte LDS read of V^T.
// Rows >= S of a padded tile are computed on zeros and never stored.  No workspace, no atomics, one fixed summation order.
//
// dsc_act_f16: x <- act(x) in place, 8 halfs per thread, fp32 arithmetic with the correctly rounded division and the device
// library's expf / erff / erfcf (the fast v_exp / v_rcp forms of dsc_common.h are for epilogues where 2e-7 does not matter; here
// the result is compared value by value with the fp64 formula).  The negative half of the erf GELU uses erfc: 1 + erf(z)
// cancels there, and x * Phi(x) below x = -4 is a handful of fp16 subnormal steps.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

constexpr int kCaD = 64;          // head dim
constexpr int kCaSMax = 80;       // five 16-row MFMA tiles
constexpr int kCaWaves = 5;
constexpr int kCaKP = 72;         // LDS row stride of K (halfs): 144 B, keeps 16-byte pieces aligned
constexpr int kCaVP = 88;         // LDS row stride of V^T (halfs): 176 B, keeps 8-byte pieces aligned

struct CaParams {
    const half_t* q; const half_t* k; const half_t* v; half_t* out;
    int H, S;
    float scale_log2e;
    long long qsb, qss, qsh, ksb, kss, ksh, vsb, vss, vsh, osb, oss, osh;
};

__global__ __launch_bounds__(64 * kCaWaves) void causal_attn_kernel(CaParams p) {
    __shared__ __attribute__((aligned(16))) half_t Ks[kCaSMax * kCaKP];
    __shared__ __attribute__((aligned(16))) half_t Vt[kCaD * kCaVP];
    const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int S = p.S, n_tiles = (S + 15) >> 4;
    const h8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // this lane's query row: requested ahead of the staging loads
    const int l = 16 * wave + r;
    const bool ok = l < S;
    h8_t qf[2];
    {
        const half_t* qp = p.q + b * p.qsb + l * p.qss + h * p.qsh;
#pragma unroll
        for (int s = 0; s < 2; ++s) qf[s] = ok ? *reinterpret_cast<const h8_t*>(qp + 32 * s + 8 * g) : zero8;
    }

    const half_t* kb = p.k + b * p.ksb + h * p.ksh;
    const half_t* vb = p.v + b * p.vsb + h * p.vsh;
    for (int i = tid; i < n_tiles * 16 * 8; i += 64 * kCaWaves) {        // rows [0, 16 n_tiles) <= 80, 8 pieces of 8 halfs each
        const int row = i >> 3, c8 = (i & 7) * 8;
        h8_t kk = zero8, vv = zero8;
        if (row < S) {
            kk = *reinterpret_cast<const h8_t*>(kb + row * p.kss + c8);
            vv = *reinterpret_cast<const h8_t*>(vb + row * p.vss + c8);
        }
        *reinterpret_cast<h8_t*>(Ks + row * kCaKP + c8) = kk;
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(c8 + j) * kCaVP + row] = vv[j];
    }
    __syncthreads();
    if (wave >= n_tiles) return;                                          // wave-uniform, after the only barrier

    f4x_t acc[kCaWaves];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < kCaWaves; ++kt) {
        acc[kt] = f4x_t{0.f, 0.f, 0.f, 0.f};
        if (kt <= wave) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const h8_t kf = *reinterpret_cast<const h8_t*>(Ks + (16 * kt + r) * kCaKP + 32 * s + 8 * g);
                acc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[s], acc[kt], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float x = (16 * kt + 4 * g + i <= l) ? acc[kt][i] * p.scale_log2e : -INFINITY;
                acc[kt][i] = x;
                mx = fmaxf(mx, x);
            }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                               // key 0 counts for every query: mx is a score
    h4_t pf[kCaWaves];
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < kCaWaves; ++kt) {
        pf[kt] = h4_t{0, 0, 0, 0};
        if (kt <= wave) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pf[kt][i] = (half_t)__builtin_amdgcn_exp2f(acc[kt][i] - mx);   // exp2(-inf) = 0
                sum += (float)pf[kt][i];
            }
        }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;                                          // sum >= 1: the maximum's own term

    half_t* op = p.out + b * p.osb + l * p.oss + h * p.osh;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        f4x_t o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
        const int c = 32 * m + 8 * (r >> 2) + (r & 3);
#pragma unroll
        for (int kt = 0; kt < kCaWaves; ++kt) {
            if (kt <= wave) {
                const h4_t v0 = *reinterpret_cast<const h4_t*>(Vt + c * kCaVP + 16 * kt + 4 * g);
                const h4_t v1 = *reinterpret_cast<const h4_t*>(Vt + (c + 4) * kCaVP + 16 * kt + 4 * g);
                o0 = __builtin_amdgcn_mfma_f32_16x16x16f16(v0, pf[kt], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_16x16x16f16(v1, pf[kt], o1, 0, 0, 0);
            }
        }
        if (ok) {
            h8_t res;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                res[i] = (half_t)(o0[i] * inv);
                res[4 + i] = (half_t)(o1[i] * inv);
            }
            *reinterpret_cast<h8_t*>(op + 32 * m + 8 * g) = res;
        }
    }
}

__device__ __forceinline__ float quick_gelu_f(float x) {
#pragma clang fp contract(off)
    const float t = 1.702f * x;
    return x * (1.f / (1.f + expf(-t)));
}

__device__ __forceinline__ float erf_gelu_f(float x) {
#pragma clang fp contract(off)
    const float z = x * 0.70710678118654752f;
    const float hx = 0.5f * x;
    return x >= 0.f ? hx * (1.f + erff(z)) : hx * erfcf(-z);             // a NaN takes the second arm and stays a NaN
}

template <int KIND>
__global__ __launch_bounds__(256) void act_kernel(half_t* x, long long n8) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    h8_t* px = reinterpret_cast<h8_t*>(x) + i;
    const h8_t a = *px;
    h8_t y;
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = (half_t)(KIND == DSC_ACT_QUICK_GELU ? quick_gelu_f((float)a[j]) : erf_gelu_f((float)a[j]));
    *px = y;
}

bool ca_aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
bool ca_strides_ok(const int64_t s[3]) { return s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0; }

}  // namespace

extern "C" int dsc_causal_attn_f16(const void* q, const void* k, const void* v, void* out, int B, int H, int S, int d,
                                   const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                                   const int64_t o_strides[3], float scale, int dtype, void* stream) {
    if (!q || !k || !v || !out || !q_strides || !k_strides || !v_strides || !o_strides) return DSC_ERR_BAD_ARG;
    if (B <= 0 || H <= 0 || S <= 0 || d <= 0) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || d != DSC_CAUSAL_ATTN_HEAD_DIM || S > DSC_CAUSAL_ATTN_MAX_TOKENS) return DSC_ERR_UNSUPPORTED;
    if (!ca_aligned16(q) || !ca_aligned16(k) || !ca_aligned16(v) || !ca_aligned16(out) || !ca_strides_ok(q_strides) ||
        !ca_strides_ok(k_strides) || !ca_strides_ok(v_strides) || !ca_strides_ok(o_strides))
        return DSC_ERR_UNSUPPORTED;
    if ((long long)B * H > 0x7fffffffll) return DSC_ERR_UNSUPPORTED;
    static_assert(DSC_CAUSAL_ATTN_HEAD_DIM == kCaD && DSC_CAUSAL_ATTN_MAX_TOKENS == kCaSMax, "header and kernel limits");
    CaParams p{};
    p.q = static_cast<const half_t*>(q); p.k = static_cast<const half_t*>(k);
    p.v = static_cast<const half_t*>(v); p.out = static_cast<half_t*>(out);
    p.H = H; p.S = S;
    p.scale_log2e = (scale > 0.f ? scale : 1.0f / sqrtf((float)d)) * 1.4426950408889634f;
    p.qsb = q_strides[0]; p.qss = q_strides[1]; p.qsh = q_strides[2];
    p.ksb = k_strides[0]; p.kss = k_strides[1]; p.ksh = k_strides[2];
    p.vsb = v_strides[0]; p.vss = v_strides[1]; p.vsh = v_strides[2];
    p.osb = o_strides[0]; p.oss = o_strides[1]; p.osh = o_strides[2];
    DSC_LAUNCH(causal_attn_kernel, dim3((unsigned)(B * H)), dim3(64 * kCaWaves), 0, static_cast<hipStream_t>(stream), p);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_act_f16(void* x, int64_t n, int kind, int dtype, void* stream) {
    if (!x || n <= 0) return DSC_ERR_BAD_ARG;
    if (kind != DSC_ACT_QUICK_GELU && kind != DSC_ACT_GELU_ERF) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || n % 8 != 0 || !ca_aligned16(x)) return DSC_ERR_UNSUPPORTED;
    const long long n8 = n / 8, blocks = (n8 + 255) / 256;
    if (blocks > 0x7fffffffll) return DSC_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    half_t* px = static_cast<half_t*>(x);
    if (kind == DSC_ACT_QUICK_GELU) DSC_LAUNCH(act_kernel<DSC_ACT_QUICK_GELU>, dim3((unsigned)blocks), dim3(256), 0, st, px, n8);
    else DSC_LAUNCH(act_kernel<DSC_ACT_GELU_ERF>, dim3((unsigned)blocks), dim3(256), 0, st, px, n8);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
