// LoRA merge over a table of weights in one launch (dsc_lora_merge_f16; modules/lora.py).  Per job, one nn.Linear or 1x1-conv
// weight [N, K] with its adapters concatenated along the rank (R = 32 * segments, each adapter zero-padded to whole segments):
//     dst[n, k] = fp16( fp32(base[n, k]) + sum_seg gain[seg] * ( sum_{r in seg} up[n, r] * down[r, k] ) )
// which is the reference's `W += alpha * mm(up.float(), down.float())` from a pristine copy: the fp32 product sum of a segment is
// one v_mfma_f32_16x16x32_f16 from a zero accumulator, the gain multiplies that fp32 sum (its own rounding, no fma), segments are
// added in ascending order, base is added last and the result is rounded once.  A segment whose gain is 0 is skipped, not
// multiplied: NaN / inf in its up / down rows never reach an accumulator.
//
// Tiles of 64 rows x 64 columns, 256 lanes; a workgroup finds its job by bisection over the jobs' first-tile numbers (tile0, the
// prefix sum dsc_lora_merge_plan writes).  down[:, k0 .. k0 + 64) goes to LDS transposed ([64][R], rows padded by 8 halfs), columns
// >= K as zeros.  Wave w owns rows n0 + 16 w ..+16.  The product is taken transposed, D^T = down^T up^T: the A operand of lane
// (c = lane & 15, g = lane >> 4) is one 16-byte LDS read of down^T[k(c)][32 s + 8 g ..+8], the B operand one 16-byte global read of
// up[n0 + 16 w + c][32 s + 8 g ..+8], and the accumulator holds 4 consecutive k of row n = c.  With A row m standing for column
// 32 kt + 8 (m >> 2) + 4 u + (m & 3) (csrc/clip_text.hip's permutation) the two calls u = 0, 1 leave lane (c, g) with the 8
// consecutive columns 32 kt + 8 g ..+8 of its row: one 16-byte read of base, one 16-byte store to dst.  Rows >= N are computed on
// zeros and never stored.  No workspace, no atomics; the order of every sum is a property of the tile alone, so the bits do not
// depend on the grid or on the other jobs of the launch.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

constexpr int kTN = 64, kTK = 64;                     // tile: rows (4 waves x 16), columns
constexpr int kDP = DSC_LORA_MAX_RANK + 8;            // LDS row stride of down^T (halfs): 528 B, keeps 16-byte pieces aligned

__device__ __forceinline__ float add_scaled(float total, float gain, float sum) {
#pragma clang fp contract(off)
    const float p = gain * sum;                       // the reference's alpha * mm(...): rounded before it is added
    return total + p;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const dsc_lora_job* __restrict__ jobs, int n_jobs) {
    __shared__ __attribute__((aligned(16))) half_t Dt[kTK * kDP];
    const int bid = blockIdx.x;
    int lo = 0, hi = n_jobs - 1;                      // the last job whose first tile is <= bid (uniform: scalar loads)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].tile0 <= bid) lo = mid;
        else hi = mid - 1;
    }
    const dsc_lora_job& job = jobs[lo];
    const int N = job.N, K = job.K, R = job.R, nseg = R / DSC_LORA_SEGMENT;
    const int t = bid - job.tile0, ntk = (K + kTK - 1) / kTK;
    const int tn = t / ntk, n0 = tn * kTN, k0 = (t - tn * ntk) * kTK;
    const half_t* base = static_cast<const half_t*>(job.base);
    const half_t* up = static_cast<const half_t*>(job.up);
    const half_t* down = static_cast<const half_t*>(job.down);
    half_t* dst = static_cast<half_t*>(job.dst);
    const float* gain = job.gain;
    const long long ldd = job.ld_dst;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const h8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    const int n = n0 + 16 * wave + c;
    const bool okn = n < N;
    h8_t bv[2];
    bool okk[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {                  // this lane's base pieces: requested ahead of the staging loads
        const int k = k0 + 32 * kt + 8 * g;
        okk[kt] = okn && k < K;                       // K % 8 == 0: a piece lies wholly inside or outside the row
        bv[kt] = okk[kt] ? *reinterpret_cast<const h8_t*>(base + (long long)n * K + k) : zero8;
    }

    for (int i = tid; i < R * 8; i += 256) {          // down[r][k0 + c8 ..+8] -> Dt[c8 + j][r]
        const int r = i >> 3, c8 = (i & 7) * 8;
        const h8_t v = k0 + c8 < K ? *reinterpret_cast<const h8_t*>(down + (long long)r * K + k0 + c8) : zero8;
#pragma unroll
        for (int j = 0; j < 8; ++j) Dt[(c8 + j) * kDP + r] = v[j];
    }
    __syncthreads();
    if (n0 + 16 * wave >= N) return;                  // wave-uniform, after the only barrier

    f4x_t tot[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int u = 0; u < 2; ++u) tot[kt][u] = f4x_t{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nseg; ++s) {
        const float gs = gain[s];
        if (gs == 0.f) continue;                      // uniform; the segment's operands are not read at all
        const h8_t b = okn ? *reinterpret_cast<const h8_t*>(up + (long long)n * R + 32 * s + 8 * g) : zero8;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int kl = 32 * kt + 8 * (c >> 2) + 4 * u + (c & 3);
                const h8_t a = *reinterpret_cast<const h8_t*>(Dt + kl * kDP + 32 * s + 8 * g);
                const f4x_t p = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, f4x_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) tot[kt][u][i] = add_scaled(tot[kt][u][i], gs, p[i]);
            }
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        if (!okk[kt]) continue;
        h8_t res;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            res[i] = (half_t)((float)bv[kt][i] + tot[kt][0][i]);
            res[4 + i] = (half_t)((float)bv[kt][4 + i] + tot[kt][1][i]);
        }
        *reinterpret_cast<h8_t*>(dst + (long long)n * ldd + k0 + 32 * kt + 8 * g) = res;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool overlap(uintptr_t a, uintptr_t a_bytes, const void* b, uintptr_t b_bytes) {
    const uintptr_t bb = reinterpret_cast<uintptr_t>(b);
    return a < bb + b_bytes && bb < a + a_bytes;
}

// one job against the limits of include/dsc_hip.h -> DSC_OK or the status both entries return for it
int check_job(const dsc_lora_job& j) {
    if (!j.base || !j.dst || !j.up || !j.down || !j.gain) return DSC_ERR_BAD_ARG;
    if (j.N < 1 || j.K < 1 || j.R < 1 || j.ld_dst < j.K) return DSC_ERR_BAD_ARG;
    if (j.K % 8 != 0 || j.ld_dst % 8 != 0 || j.R % DSC_LORA_SEGMENT != 0 || j.R > DSC_LORA_MAX_RANK) return DSC_ERR_UNSUPPORTED;
    if (!aligned16(j.base) || !aligned16(j.dst) || !aligned16(j.up) || !aligned16(j.down) ||
        (reinterpret_cast<uintptr_t>(j.gain) & 3))
        return DSC_ERR_UNSUPPORTED;
    const uintptr_t N = (uintptr_t)j.N, K = (uintptr_t)j.K, R = (uintptr_t)j.R;
    const uintptr_t d = reinterpret_cast<uintptr_t>(j.dst), d_bytes = ((N - 1) * (uintptr_t)j.ld_dst + K) * 2;
    if (overlap(d, d_bytes, j.base, N * K * 2) || overlap(d, d_bytes, j.up, N * R * 2) || overlap(d, d_bytes, j.down, R * K * 2) ||
        overlap(d, d_bytes, j.gain, R / DSC_LORA_SEGMENT * 4))
        return DSC_ERR_BAD_ARG;
    return DSC_OK;
}

long long job_tiles(const dsc_lora_job& j) { return (long long)((j.N + kTN - 1) / kTN) * ((j.K + kTK - 1) / kTK); }

}  // namespace

extern "C" long long dsc_lora_merge_plan(dsc_lora_job* jobs, int n_jobs) {
    if (!jobs || n_jobs < 1) return DSC_ERR_BAD_ARG;
    long long total = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const int rc = check_job(jobs[i]);
        if (rc != DSC_OK) return rc;
        jobs[i].tile0 = (int)total;
        total += job_tiles(jobs[i]);
        if (total > 0x7fffffffll) return DSC_ERR_UNSUPPORTED;
    }
    return total;
}

extern "C" int dsc_lora_merge_f16(const dsc_lora_job* jobs, const void* jobs_dev, int n_jobs, int dtype, void* stream) {
    if (!jobs || !jobs_dev || n_jobs < 1) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || (reinterpret_cast<uintptr_t>(jobs_dev) & 7)) return DSC_ERR_UNSUPPORTED;
    long long total = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const int rc = check_job(jobs[i]);
        if (rc != DSC_OK) return rc;
        if (jobs[i].tile0 != (int)total) return DSC_ERR_BAD_ARG;          // not the table dsc_lora_merge_plan numbered
        total += job_tiles(jobs[i]);
        if (total > 0x7fffffffll) return DSC_ERR_UNSUPPORTED;
    }
    static_assert(DSC_LORA_SEGMENT == 32, "one v_mfma_f32_16x16x32_f16 per segment");
    DSC_LAUNCH(lora_merge_kernel, dim3((unsigned)total), dim3(256), 0, static_cast<hipStream_t>(stream),
               static_cast<const dsc_lora_job*>(jobs_dev), n_jobs);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
