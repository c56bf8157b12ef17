// The ControlNet residual add of the continuous batcher's captured step (dsc_scatter_add_rows_f16): lane row j of a compact
// ControlNet batch lands in batch row dst[j] of a UNet skip tensor (or of the mid block's output), in place:
//     t = fp16( gate[0][j] * feat[0][j][e] )
//     t = fp16( t + fp16( gate[a][j] * feat[a][j][e] ) )          for every further net a whose gate is not 0
//     x[dst[j]][e] = fp16( x[dst[j]][e] + t )
// - what the reference does in three places: ControlNetModel.forward (`d * conditioning_scale`), MultiControlNetModel.forward
// (`a + b` over the nets) and the UNet (`s + r`, modules/u_net_condition_modify.py:1236-1245).  Every product and sum is an fp32
// operation rounded to fp32 and THEN to fp16, on its own - the bits of torch's fp16 `feat * g`, `a + b` and `s + r` at every
// tensor of 2048 elements and more, i.e. at every residual of a real model.  (Below that torch's multiply launches another kernel
// variant, in which the compiler has folded the conversion into the multiply - v_fma_mixlo_f16, ONE rounding of the exact
// product - and about 4 % of the products differ by an ulp; this kernel does not follow torch's tensor-length rule.)  "This lane
// serves that batch row at this scale" is device data (gate fp32 [nets][lane_rows], dst int32 [lane_rows]), so one captured
// launch follows the batch's membership.
//
// Streaming and HBM-bound, the shape of add_rows_gated_kernel: 16-byte loads and stores, 8 halfs per lane, no LDS, no atomics.
// The lane row is the grid's second dimension, so dst, the gates and the skip test are wave-uniform: a workgroup whose lane is
// idle (dst < 0, or every gate 0) returns before it has loaded anything from x or feat.  The nets whose gate is 0 are not read
// either: the chain starts at the first open net.  The grid is capped at ~2048 workgroups and strides over the rest of a row.
// Active lane rows must name DISTINCT destination rows (the caller's invariant: two lanes on one row would race).
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

constexpr int kScatterBlocks = 2048;         // whole grid, all lane rows together
constexpr int kScatterMaxNets = 8;

// an fp32 operation's result, rounded to fp16 as an instruction of its own: the empty asm keeps the compiler from contracting
// the operation and the conversion (or two steps of the chain) into one single-rounding mixed-precision fma, as gated_add.hip does
__device__ __forceinline__ half_t round_own(float v) {
    asm volatile("" : "+v"(v));
    return (half_t)v;
}

__global__ __launch_bounds__(256) void scatter_add_rows_kernel(h8_t* x, const h8_t* feat, const float* gate, const int* dst,
                                                               int x_rows, int lane_rows, int nets, long long pieces) {
    const int j = blockIdx.y;
    const int d = dst[j];
    if (d < 0 || d >= x_rows) return;                            // an idle lane (a row past x is never written either)
    int a0 = 0;
    while (a0 < nets && gate[(long long)a0 * lane_rows + j] == 0.f) ++a0;
    if (a0 == nets) return;                                      // every gate closed: nothing read, nothing written
    const float g0 = gate[(long long)a0 * lane_rows + j];
    h8_t* xr = x + (long long)d * pieces;
    const h8_t* f0 = feat + ((long long)a0 * lane_rows + j) * pieces;
    const long long stride = (long long)gridDim.x * 256;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pieces; p += stride) {
        const h8_t xv = xr[p];
        h8_t fv = f0[p];
        half_t t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = round_own(g0 * (float)fv[e]);
        for (int a = a0 + 1; a < nets; ++a) {
            const float g = gate[(long long)a * lane_rows + j];  // (wave-uniform, like the branch)
            if (g == 0.f) continue;
            fv = feat[((long long)a * lane_rows + j) * pieces + p];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const half_t s = round_own(g * (float)fv[e]);
                t[e] = round_own((float)t[e] + (float)s);
            }
        }
        h8_t ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) ov[e] = round_own((float)xv[e] + (float)t[e]);
        xr[p] = ov;
    }
}

}  // namespace

extern "C" int dsc_scatter_add_rows_f16(void* x, const void* feat, const void* gate, const void* dst, int x_rows, int lane_rows,
                                        int nets, long long row_elems, void* stream) {
    if (!x || !feat || !gate || !dst) return DSC_ERR_BAD_ARG;
    if (x_rows < 1 || lane_rows < 1 || nets < 1 || row_elems < 1 || nets > kScatterMaxNets) return DSC_ERR_BAD_ARG;
    if (row_elems >= (1ll << 40)) return DSC_ERR_UNSUPPORTED;
    if (lane_rows > 65535) return DSC_ERR_UNSUPPORTED;           // the lane row is gridDim.y
    // x and feat below 2^60 bytes each, so that the byte counts of the overlap tests cannot wrap
    if (row_elems > (1ll << 59) / x_rows || row_elems > (1ll << 59) / ((long long)nets * lane_rows)) return DSC_ERR_UNSUPPORTED;
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), fa = reinterpret_cast<uintptr_t>(feat);
    const uintptr_t ga = reinterpret_cast<uintptr_t>(gate), da = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t x_bytes = (uintptr_t)x_rows * (uintptr_t)row_elems * 2;
    const uintptr_t f_bytes = (uintptr_t)nets * (uintptr_t)lane_rows * (uintptr_t)row_elems * 2;
    // x is written while the other three are read: it lies apart from all of them
    if (xa < fa + f_bytes && fa < xa + x_bytes) return DSC_ERR_BAD_ARG;
    if (xa < ga + (uintptr_t)nets * (uintptr_t)lane_rows * 4 && ga < xa + x_bytes) return DSC_ERR_BAD_ARG;
    if (xa < da + (uintptr_t)lane_rows * 4 && da < xa + x_bytes) return DSC_ERR_BAD_ARG;
    if (row_elems % 8 != 0 || ((xa | fa) & 15) || ((ga | da) & 3)) return DSC_ERR_UNSUPPORTED;
    const long long pieces = row_elems / 8;
    const long long want = (pieces + 255) / 256;
    const long long cap = kScatterBlocks / lane_rows > 0 ? kScatterBlocks / lane_rows : 1;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)lane_rows), block(256);
    DSC_LAUNCH(scatter_add_rows_kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<h8_t*>(x),
               static_cast<const h8_t*>(feat), static_cast<const float*>(gate), static_cast<const int*>(dst), x_rows, lane_rows, nets,
               pieces);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
