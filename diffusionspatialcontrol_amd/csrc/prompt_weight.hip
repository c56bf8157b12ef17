// Prompt emphasis on the text lane of the continuous batcher (dsc_prompt_weight_rows_f16): the tail of
// FrozenCLIPEmbedderWithCustomWordsBase.process_tokens (reference modules/prompt_parser.py:196-221), the hstack over chunks and
// the cast of encode_prompt_automatic1111, for up to 16 (request, chunk) groups in one launch.  Per group, with z the encoder's
// fp16 output for the chunk's [negative, positive] rows (N = 2 T C elements) and m the fp32 multiplier of every token:
//     before = fp16(sum z / N)                   the sum in fp64
//     p      = fp32(z) * m                       every product rounded to fp32
//     after  = fp32(sum p / N)                   the sum in fp64
//     ratio  = fp32(before) / after              an IEEE fp32 division; no guard: after == 0 gives inf / NaN as the eager chain does
//     out    = fp16(fp32(p * ratio))             two roundings
// Both means run over BOTH rows of the group (the eager chain takes `z.mean()` of the [2, T, C] tensor).
//
// One workgroup of 1024 lanes owns a group's sums: lane t walks the 8-half vectors t, t + 1024, ... of the 2 T C / 8 the two rows
// hold (row 0 first), adding element by element into two fp64 accumulators; a butterfly over each wave, then the sixteen waves'
// partials through LDS added in wave order by every lane.  No atomics, and the order is a property of the workgroup, not of the
// grid: gridDim.x workgroups per group each redo the sums (the second and later readers are served by the caches) and store one
// contiguous slice of the vectors, so the bits do not depend on how many there are.
// The product and the scaling are pinned in fp32 registers (freeu.hip, gated_add.hip): fused into one mixed-precision
// multiply-convert the scaled value would be rounded once where the contract has two roundings.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / DSC_WAVE;
constexpr int kAhead = 4;                      // vectors a lane loads before it adds them

struct WeightArgs {
    dsc_prompt_weight_group g[DSC_PROMPT_WEIGHT_MAX_GROUPS];
};

int g_slices = 0;                              // dsc_debug_set_prompt_weight_slices: 0 = the launch rule below

__device__ __forceinline__ float pin_f32(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

__global__ __launch_bounds__(kThreads) void prompt_weight_kernel(const h8_t* __restrict__ z, int T, int cv, long long ldo,
                                                                 const WeightArgs a) {
    __shared__ double part[2][kWaves];
    const dsc_prompt_weight_group& g = a.g[blockIdx.y];              // (uniform: scalar loads of the kernel arguments)
    if (!g.out[0]) return;
    const int t = threadIdx.x;
    const int per_row = T * cv, total = 2 * per_row;
    const h8_t* zr[2] = {z + (long long)g.z_row[0] * per_row, z + (long long)g.z_row[1] * per_row};
    const float* mult = static_cast<const float*>(g.mult);

    // (kAhead loads in flight per lane: the additions below keep the order v = t, t + 1024, ... whatever kAhead is)
    double s0 = 0.0, s1 = 0.0;
    for (int v0 = t; v0 < total; v0 += kAhead * kThreads) {
        h8_t xv[kAhead];
        float m[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int v = v0 + u * kThreads;
            if (v < total) {
                const int row = v >= per_row, w = v - row * per_row;
                m[u] = mult[row * T + w / cv];
                xv[u] = zr[row][w];
            }
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            if (v0 + u * kThreads < total) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float x = (float)xv[u][e];
                    s0 += (double)x;
                    s1 += (double)pin_f32(x * m[u]);
                }
            }
        }
    }
    s0 = wave_sum_f64(s0);
    s1 = wave_sum_f64(s1);
    if (t % DSC_WAVE == 0) {
        part[0][t / DSC_WAVE] = s0;
        part[1][t / DSC_WAVE] = s1;
    }
    __syncthreads();
    s0 = s1 = 0.0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        s0 += part[0][k];
        s1 += part[1][k];
    }
    const double count = 8.0 * (double)total;
    const half_t before = (half_t)(s0 / count);
    const float after = (float)(s1 / count);
    const float ratio = (float)before / after;

    const int chunk = (total + (int)gridDim.x - 1) / (int)gridDim.x;
    const int lo = (int)blockIdx.x * chunk, hi = lo + chunk < total ? lo + chunk : total;
    half_t* out[2] = {static_cast<half_t*>(g.out[0]), static_cast<half_t*>(g.out[1])};
    for (int v = lo + t; v < hi; v += kThreads) {
        const int row = v >= per_row, w = v - row * per_row, tok = w / cv, c = w - tok * cv;
        const float m = mult[row * T + tok];
        const h8_t xv = zr[row][w];
        h8_t ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float p = pin_f32((float)xv[e] * m);
            ov[e] = (half_t)pin_f32(p * ratio);
        }
        *reinterpret_cast<h8_t*>(out[row] + (long long)tok * ldo + 8 * c) = ov;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool overlap(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

}  // namespace

extern "C" void dsc_debug_set_prompt_weight_slices(int slices) { g_slices = slices > 0 ? slices : 0; }

extern "C" int dsc_prompt_weight_rows_f16(const void* z, int m, int T, int C, const dsc_prompt_weight_group* groups, int n,
                                          long long ldo, void* stream) {
    if (!z || !groups || m < 1 || T < 1 || C < 1 || n < 1 || n > DSC_PROMPT_WEIGHT_MAX_GROUPS || ldo < C) return DSC_ERR_BAD_ARG;
    const uintptr_t za = reinterpret_cast<uintptr_t>(z);
    const uintptr_t z_bytes = (uintptr_t)m * (uintptr_t)T * (uintptr_t)C * 2;
    const uintptr_t o_bytes = ((uintptr_t)(T - 1) * (uintptr_t)ldo + (uintptr_t)C) * 2, m_bytes = (uintptr_t)T * 8;
    bool any = false;
    for (int j = 0; j < n; ++j) {
        const dsc_prompt_weight_group& g = groups[j];
        if (!g.out[0] && !g.out[1]) continue;
        if (!g.out[0] || !g.out[1] || !g.mult) return DSC_ERR_BAD_ARG;
        if (g.z_row[0] < 0 || g.z_row[0] >= m || g.z_row[1] < 0 || g.z_row[1] >= m) return DSC_ERR_BAD_ARG;
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(g.out[0]), o1 = reinterpret_cast<uintptr_t>(g.out[1]);
        const uintptr_t ma = reinterpret_cast<uintptr_t>(g.mult);
        if (overlap(o0, o_bytes, o1, o_bytes) && (ldo == C || o0 == o1)) return DSC_ERR_BAD_ARG;
        if (overlap(o0, o_bytes, za, z_bytes) || overlap(o1, o_bytes, za, z_bytes)) return DSC_ERR_BAD_ARG;
        if (overlap(o0, o_bytes, ma, m_bytes) || overlap(o1, o_bytes, ma, m_bytes)) return DSC_ERR_BAD_ARG;
        any = true;
    }
    if (C % 8 != 0 || ldo % 8 != 0 || !aligned16(z)) return DSC_ERR_UNSUPPORTED;
    if ((long long)T * C >= (1ll << 30) || (long long)m * T * C >= (1ll << 40)) return DSC_ERR_UNSUPPORTED;
    WeightArgs a = {};
    for (int j = 0; j < n; ++j) {
        const dsc_prompt_weight_group& g = groups[j];
        if (!g.out[0]) continue;
        if (!aligned16(g.out[0]) || !aligned16(g.out[1]) || (reinterpret_cast<uintptr_t>(g.mult) & 3)) return DSC_ERR_UNSUPPORTED;
        a.g[j] = g;
    }
    if (!any) return DSC_OK;                                           // every group is idle: no launch
    // launch rule: slices of at least one vector per lane, at most 8 workgroups per group (tools/mb_prompt_weight.py)
    const long long total = 2ll * T * (C / 8);
    long long slices = (total + kThreads - 1) / kThreads;
    slices = g_slices ? (g_slices > 64 ? 64 : g_slices) : (slices > 8 ? 8 : slices);
    const dim3 grid((unsigned)slices, (unsigned)n), block(kThreads);
    DSC_LAUNCH(prompt_weight_kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const h8_t*>(z), T, C / 8,
               ldo, a);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
