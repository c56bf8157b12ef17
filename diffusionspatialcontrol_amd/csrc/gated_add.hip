// The T2I-Adapter residual add of the continuous batcher's captured step (dsc_add_rows_gated_f16): per batch row
//     out[r][e] = fp16( x[r][e] + gate[r] * feat[r % feat_rows][e] )
// - what the reference's down blocks do with `down_intrablock_additional_residuals` (modules/u_net_condition_modify.py:1194-1230,
// `sample += down_intrablock_additional_residuals.pop(0)`), with "is there a residual for this row, at this step" turned from
// Python control flow into one fp32 gate per batch row in DEVICE memory: a captured launch serves rows with and without a control
// image, inside and outside their `adapter_conditioning_factor` window.
//
// Streaming and HBM-bound: 16-byte loads and stores, 8 halfs per lane, no LDS, no atomics.  The batch row is the grid's second
// dimension, so the gate is one wave-uniform scalar load and "gate == 0" one uniform branch: in place such a workgroup returns
// before it has loaded anything (its x row stays as it is and its feature row may hold anything), out of place it copies its
// piece of x.  The grid is capped at ~2048 workgroups and strides over the rest of a row.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

constexpr int kGatedAddBlocks = 2048;        // whole grid, all rows together

// (no __restrict__: out may be x)
template <bool kInPlace>
__global__ __launch_bounds__(256) void add_rows_gated_kernel(const h8_t* x, const h8_t* feat, const float* gate, h8_t* out,
                                                             int feat_rows, long long pieces) {
    const int r = blockIdx.y;
    const float g = gate[r];
    if (kInPlace && g == 0.f) return;
    const h8_t* xr = x + (long long)r * pieces;
    h8_t* orow = out + (long long)r * pieces;
    const long long stride = (long long)gridDim.x * 256;
    long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g == 0.f) {                                              // out of place: the row bit for bit, the feature row unread
        for (; p < pieces; p += stride) orow[p] = xr[p];
        return;
    }
    const h8_t* fr = feat + (long long)(r % feat_rows) * pieces;
    for (; p < pieces; p += stride) {
        const h8_t xv = xr[p], fv = fr[p];
        h8_t ov;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float acc = fmaf(g, (float)fv[e], (float)xv[e]);
            // the fp32 rounding of the fma is part of the contract (with gate 1 torch's fp16 `x + feat`: an fp32 sum, then
            // `.to(fp16)`): keep the fma and the conversion two instructions, as dsc_latent_resample_noise does
            asm volatile("" : "+v"(acc));
            ov[e] = (half_t)acc;
        }
        orow[p] = ov;
    }
}

}  // namespace

extern "C" int dsc_add_rows_gated_f16(const void* x, const void* feat, const void* gate, void* out, int rows, int feat_rows,
                                      long long row_elems, void* stream) {
    if (!x || !feat || !gate || !out) return DSC_ERR_BAD_ARG;
    if (rows < 1 || feat_rows < 1 || row_elems < 1 || rows % feat_rows != 0) return DSC_ERR_BAD_ARG;
    if (row_elems >= (1ll << 40)) return DSC_ERR_UNSUPPORTED;
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), fa = reinterpret_cast<uintptr_t>(feat), oa = reinterpret_cast<uintptr_t>(out);
    const uintptr_t ga = reinterpret_cast<uintptr_t>(gate);
    const uintptr_t x_bytes = (uintptr_t)rows * (uintptr_t)row_elems * 2, f_bytes = (uintptr_t)feat_rows * (uintptr_t)row_elems * 2;
    // out is x itself (in place: every lane reads the piece it writes) or apart from it; never inside the features or the gates
    if (oa != xa && oa < xa + x_bytes && xa < oa + x_bytes) return DSC_ERR_BAD_ARG;
    if (oa < fa + f_bytes && fa < oa + x_bytes) return DSC_ERR_BAD_ARG;
    if (oa < ga + (uintptr_t)rows * 4 && ga < oa + x_bytes) return DSC_ERR_BAD_ARG;
    if (row_elems % 8 != 0 || ((xa | fa | oa) & 15) || (ga & 3)) return DSC_ERR_UNSUPPORTED;
    if (rows > 65535) return DSC_ERR_UNSUPPORTED;                // the batch row is gridDim.y
    const long long pieces = row_elems / 8;
    const long long want = (pieces + 255) / 256;
    const long long cap = kGatedAddBlocks / rows > 0 ? kGatedAddBlocks / rows : 1;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)rows), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const h8_t* xp = static_cast<const h8_t*>(x);
    const h8_t* fp = static_cast<const h8_t*>(feat);
    const float* gp = static_cast<const float*>(gate);
    h8_t* op = static_cast<h8_t*>(out);
    if (oa == xa)
        DSC_LAUNCH(add_rows_gated_kernel<true>, grid, block, 0, st, xp, fp, gp, op, feat_rows, pieces);
    else
        DSC_LAUNCH(add_rows_gated_kernel<false>, grid, block, 0, st, xp, fp, gp, op, feat_rows, pieces);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
