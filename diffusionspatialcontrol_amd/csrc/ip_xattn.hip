// The IP-Adapter term of a cross-attention layer, accumulated in place with one scale per batch row (dsc_ip_xattn_add_f16):
//     io[b, l, h, :] = fp16( float(io[b, l, h, :]) + row_scale[b] * sum_t softmax_t(s * q[b, l, h, :] . k_ip[b, t, h, :]) v_ip[b, t, h, :] )
// - what the reference's two IP-Adapter processors do per adapter after the text branch (modules/attention_modify.py:365-385 and
// :659-685: attention of the layer's queries over the adapter's 4 / 16 image tokens, `hidden_states + scale * ...`), with the
// per-processor Python float `scale` replaced by a DEVICE vector with one entry per batch row: rows of different requests of a
// continuous batch carry different scales (or none), and a captured step stays valid when they change.  to_k_ip / to_v_ip of the
// tokens (:368-369 / :662-663) are inputs: they do not change during a generation.
//
// Design: MFMA, no LDS.  One wave owns 16 queries of one (b, h); the tokens (T <= 16) are one MFMA tile:
//   S^T[t, l] = K Q^T   v_mfma_f32_16x16x32_f16, ceil(d / 32) steps.  Lane (r = lane & 15, g = lane >> 4) holds K[t = r][32 s + 8 g ..+8]
//                       and Q[l = r][32 s + 8 g ..+8]: both are ONE 16-byte global load per step (channels >= d and tokens >= T: zeros)
//   softmax over t      the accumulator holds t = 4 g + i (i < 4) of query r: 4 values in the lane, then two xor-shuffles (16, 32)
//   O^T[c, l] = V^T P^T v_mfma_f32_16x16x16_f16: its B operand (k = 4 g + i, column r) IS the accumulator layout above, so the
//                       probabilities go from registers to registers.  Two MFMAs per 32 channels, with the rows of the A operand
//                       permuted (row 4 g + i of call u is channel 32 m + 8 g + 4 u + i) so that lane (r, g) ends up with the 8
//                       CONSECUTIVE channels 32 m + 8 g ..+8 of query r: io is read and written in 16-byte pieces by the one
//                       lane that owns them.  Unnormalised probabilities (<= 1) round to fp16; 1 / sum and row_scale are applied
//                       in fp32 to the fp32 accumulator; one fp16 rounding at the store.
// The K and V operands (<= 20 + 20 registers) are loaded once per wave and reused over its query tiles.  Arithmetic: per (row,
// head) the kernel moves 6 d bytes for 4 T d flops - at most ~11 flop/B - so it is bound by the q / io traffic; on the VALU the
// same work costs 2 T d fp32 FMAs per 16-byte piece plus a cross-lane reduction over d / 8 lanes (5, 10, 20: no power of two)
// or T LDS reads of k / v per query (10 x the global bytes at T = 16, the LDS : HBM ratio of the part); the MFMA form needs neither.
//
// The masked entry (dsc_ip_xattn_add_masked_f16) is the same body with MASKED = true: one fp16 weight per query, the IP-Adapter
// region mask after the reference's down-sampling (modules/attention_modify.py:371-385 and :676-685: the adapter's output times
// the mask, then `scale *` and the add), folded into the per-query fp32 coefficient as (row_scale[b] * w[b, l]) / sum - with
// w == 1 that is row_scale[b] / sum bit for bit.  Lane (r, g) reads the half of its query, w[b, 16 tile + r]; a ballot over
// w != 0 decides per wave whether the tile is worked on at all (a region mask is exactly zero over most of the image: no q
// load, no io load, no store), and a query whose weight is zero in a mixed tile is not stored (its q may hold anything).  The
// weight of a wave's first tile is requested before its K / V operands and the weight of tile i + 1 before the q / io loads of
// tile i: from the second tile on the ballot waits for nothing; on the first the chain is row_scale -> weight -> q / io, one
// load deeper than unmasked (the weights of a row with scale 0 are not read, and a skipped tile's q / io are not requested).
//
// row_scale[b] == 0: every workgroup of row b returns after that one (scalar, workgroup-uniform) load, before it reads k_ip / v_ip / q
// or touches io.  b is grid coordinate z.  No allocation, no synchronisation, no atomics, one fixed summation order.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

template <int NK, bool MASKED>                                       // NK = ceil(d / 32); MASKED: one weight per query (qw)
__global__ __launch_bounds__(256) void ip_xattn_add_kernel(const half_t* __restrict__ q, long long qs_b, long long qs_l, long long qs_h,
                                                           const half_t* __restrict__ k_ip, const half_t* __restrict__ v_ip,
                                                           long long kvs_b, const float* __restrict__ row_scale, half_t* __restrict__ io,
                                                           const half_t* __restrict__ qw, long long ws_b,
                                                           int L, int H, int d, int T, float scale_log2e, int tiles_per_wave) {
    const int b = blockIdx.z, h = blockIdx.y;
    const float rs = row_scale[b];
    if (rs == 0.f) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int n_tiles = (L + 15) >> 4;
    const int tile0 = (blockIdx.x * 4 + wave) * tiles_per_wave;
    const half_t* wb = MASKED ? qw + b * ws_b : nullptr;
    half_t w_next = (half_t)0;
    if constexpr (MASKED) {
        if (tile0 * 16 + r < L) w_next = wb[tile0 * 16 + r];          // ahead of the K / V loads: back by the time they are
    }
    const long long tok = (long long)H * d;                           // elements between two tokens / two queries of io
    const half_t* kb = k_ip + b * kvs_b + h * d;
    const half_t* vb = v_ip + b * kvs_b + h * d;
    const h8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    h8_t kf[NK];
    h4_t vf[NK][2];
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        const int dd = 32 * s + 8 * g;
        kf[s] = (r < T && dd < d) ? *reinterpret_cast<const h8_t*>(kb + r * tok + dd) : zero8;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int dv = 32 * s + 8 * (r >> 2) + 4 * u + (r & 3);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = 4 * g + i;
                vf[s][u][i] = (t < T && dv < d) ? vb[t * tok + dv] : (half_t)0;
            }
        }
    }
    for (int it = 0; it < tiles_per_wave; ++it) {
        const int tile = tile0 + it;
        if (tile >= n_tiles) break;                                   // wave-uniform
        const int l = tile * 16 + r;
        const bool ok = l < L;
        float w = 1.f;
        if constexpr (MASKED) {
            w = (float)w_next;
            w_next = (half_t)0;
            const int ln = l + 16;                                    // the next tile's weight: in flight under this tile's work
            if (it + 1 < tiles_per_wave && ln < L) w_next = wb[ln];
            if (__ballot(w != 0.f) == 0ull) continue;                 // wave-uniform: nothing of this tile is read or written
        }
        const half_t* qp = q + b * qs_b + l * qs_l + h * qs_h;
        half_t* op = io + ((long long)b * L + l) * tok + (long long)h * d;
        // every load of the tile is issued here: the io pieces do not wait for the scores (one memory latency per tile, not two)
        h8_t qf[NK], cur[NK];
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            const int dd = 32 * s + 8 * g;
            qf[s] = (ok && dd < d) ? *reinterpret_cast<const h8_t*>(qp + dd) : zero8;
        }
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            const int dd = 32 * s + 8 * g;
            cur[s] = (ok && dd < d) ? *reinterpret_cast<const h8_t*>(op + dd) : zero8;
        }
        f4x_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NK; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[s], qf[s], acc, 0, 0, 0);
        float x[4], mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[i] = (4 * g + i < T) ? acc[i] * scale_log2e : -INFINITY;
            mx = fmaxf(mx, x[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                       // T >= 1: token 0 is never masked, mx is a score
        float sum = 0.f;
        h4_t pf;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float p = (4 * g + i < T) ? __builtin_amdgcn_exp2f(x[i] - mx) : 0.f;
            sum += p;
            pf[i] = (half_t)p;
        }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float coef = MASKED ? (rs * w) / sum : rs / sum;
        const bool st = ok && (!MASKED || w != 0.f);
#pragma unroll
        for (int m = 0; m < NK; ++m) {
            const f4x_t z = {0.f, 0.f, 0.f, 0.f};
            const f4x_t o0 = __builtin_amdgcn_mfma_f32_16x16x16f16(vf[m][0], pf, z, 0, 0, 0);
            const f4x_t o1 = __builtin_amdgcn_mfma_f32_16x16x16f16(vf[m][1], pf, z, 0, 0, 0);
            const int dd = 32 * m + 8 * g;
            if (st && dd < d) {
                h8_t res;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    res[i] = (half_t)fmaf(coef, o0[i], (float)cur[m][i]);
                    res[4 + i] = (half_t)fmaf(coef, o1[i], (float)cur[m][4 + i]);
                }
                *reinterpret_cast<h8_t*>(op + dd) = res;
            }
        }
    }
}

}  // namespace

// both entries: q_weight == nullptr is the unmasked one (the masked entry has refused a null weight before it comes here)
static int ip_xattn_add(const void* q, long long q_stride_b, long long q_stride_l, long long q_stride_h, const void* k_ip,
                        const void* v_ip, long long kv_stride_b, const float* row_scale, void* io, const void* q_weight,
                        long long w_stride_b, int B, int L, int H, int d, int T, float softmax_scale, void* stream) {
    if (!q || !k_ip || !v_ip || !row_scale || !io || io == q || io == k_ip || io == v_ip) return DSC_ERR_BAD_ARG;
    if (B < 1 || L < 1 || H < 1 || d < 1 || T < 1 || q_stride_b < 0 || q_stride_l < 1 || q_stride_h < 1) return DSC_ERR_BAD_ARG;
    if (kv_stride_b < (long long)T * H * d) return DSC_ERR_BAD_ARG;                      // rows of k_ip / v_ip must not overlap
    if (d % 8 != 0 || d < 8 || d > 160 || T > DSC_IP_MAX_TOKENS) return DSC_ERR_UNSUPPORTED;
    if (B > 65535 || H > 65535 || (long long)B * L * H * d >= (1ll << 40)) return DSC_ERR_UNSUPPORTED;
    if ((q_stride_b | q_stride_l | q_stride_h | kv_stride_b) & 7) return DSC_ERR_UNSUPPORTED;      // 16-byte pieces of q / k_ip
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_ip) | reinterpret_cast<uintptr_t>(v_ip) |
         reinterpret_cast<uintptr_t>(io)) & 15) return DSC_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(row_scale) & 3) return DSC_ERR_UNSUPPORTED;
    const int n_tiles = (L + 15) / 16;
    // a wave is one dependent chain per tile (loads -> MFMA -> softmax -> MFMA -> store): one tile per wave, for the most waves in
    // flight, until the grid is many rounds of the chip deep (64 x 64 latents and up) - there four tiles share the K / V operand loads
    const int tpw = n_tiles >= 256 ? 4 : 1;
    const dim3 grid((unsigned)((n_tiles + 4 * tpw - 1) / (4 * tpw)), (unsigned)H, (unsigned)B), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const half_t* qp = static_cast<const half_t*>(q);
    const half_t* kp = static_cast<const half_t*>(k_ip);
    const half_t* vp = static_cast<const half_t*>(v_ip);
    half_t* op = static_cast<half_t*>(io);
    const half_t* wp = static_cast<const half_t*>(q_weight);
    const float sl = softmax_scale * 1.4426950408889634f;
#define DSC_IP_LAUNCH_M(NK, M) DSC_LAUNCH((ip_xattn_add_kernel<NK, M>), grid, block, 0, st, qp, q_stride_b, q_stride_l, q_stride_h, \
                                          kp, vp, kv_stride_b, row_scale, op, wp, w_stride_b, L, H, d, T, sl, tpw)
#define DSC_IP_LAUNCH(NK) do { if (wp) DSC_IP_LAUNCH_M(NK, true); else DSC_IP_LAUNCH_M(NK, false); } while (0)
    switch ((d + 31) / 32) {
        case 1: DSC_IP_LAUNCH(1); break;
        case 2: DSC_IP_LAUNCH(2); break;
        case 3: DSC_IP_LAUNCH(3); break;
        case 4: DSC_IP_LAUNCH(4); break;
        default: DSC_IP_LAUNCH(5); break;
    }
#undef DSC_IP_LAUNCH
#undef DSC_IP_LAUNCH_M
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_ip_xattn_add_f16(const void* q, long long q_stride_b, long long q_stride_l, long long q_stride_h,
                                    const void* k_ip, const void* v_ip, long long kv_stride_b, const float* row_scale, void* io,
                                    int B, int L, int H, int d, int T, float softmax_scale, void* stream) {
    return ip_xattn_add(q, q_stride_b, q_stride_l, q_stride_h, k_ip, v_ip, kv_stride_b, row_scale, io, nullptr, 0, B, L, H, d, T,
                        softmax_scale, stream);
}

extern "C" int dsc_ip_xattn_add_masked_f16(const void* q, long long q_stride_b, long long q_stride_l, long long q_stride_h,
                                           const void* k_ip, const void* v_ip, long long kv_stride_b, const float* row_scale,
                                           void* io, const void* q_weight, long long w_stride_b, int B, int L, int H, int d, int T,
                                           float softmax_scale, void* stream) {
    if (!q_weight || q_weight == io || w_stride_b < L) return DSC_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(q_weight) & 1) return DSC_ERR_UNSUPPORTED;
    return ip_xattn_add(q, q_stride_b, q_stride_l, q_stride_h, k_ip, v_ip, kv_stride_b, row_scale, io, q_weight, w_stride_b, B, L, H,
                        d, T, softmax_scale, stream);
}
