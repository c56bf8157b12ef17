// The last step of a served image (dsc_image_finish): the decoder's fp16 channel-major output becomes what the caller receives,
// an interleaved [n, H, W, 3] uint8 or float32 image, in one launch - what the reference does with `(image / 2 + 0.5).clamp(0, 1)`
// on the fp16 tensor, `.cpu().permute(0, 2, 3, 1).float()` (modules/model_k_diffusion.py:291-299, decode_latents) and, for PIL
// output, `(x * 255).round().astype("uint8")` on the host (numpy_to_pil, reached from :533-539).
//
// Per element, the roundings of those fp16 tensor expressions one by one:
//     h = fp16( float(fp16( float(x) * 0.5f )) + 0.5f ),  clamped to [0, 1]           (NaN -> 0: outside the contract)
//     float32 output: float(h);   uint8 output: (uint8) rintf( float(h) * 255.0f )
// h has at most 11 significant bits, so the fp32 product with 255 is exact, and its only tie (h = 0.5 -> 127.5) goes to the even
// 128 under rintf as under numpy's round.
//
// Memory-bound and small (1.5 MB in, 0.75 MB out per 512x512 uint8 image): no LDS.  Both sides are multiples of 8, so one lane
// owns 8 consecutive pixels of a row: three 16-byte loads (one per channel plane) and, interleaved, 24 output bytes at an
// 8-byte-aligned address as three 8-byte stores (uint8) or 96 bytes at a 16-byte-aligned address as six 16-byte stores (float32).
// A lane past the last piece returns before it has formed an address.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

typedef unsigned u2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ half_t finish_value(half_t x) {
    const half_t halved = (half_t)((float)x * 0.5f);                 // fp16 tensor / 2
    const half_t h = (half_t)((float)halved + 0.5f);                 // fp16 tensor + 0.5
    const half_t lo = h > (half_t)0.f ? h : (half_t)0.f;             // (a NaN compares false: 0)
    return lo < (half_t)1.f ? lo : (half_t)1.f;
}

template <int kKind>
__global__ __launch_bounds__(256) void image_finish_kernel(const half_t* __restrict__ img, void* __restrict__ out, long long pieces,
                                                           int plane_pieces) {
    const long long piece = (long long)blockIdx.x * 256 + threadIdx.x;
    if (piece >= pieces) return;
    const long long image = piece / plane_pieces;
    const long long px = (piece - image * plane_pieces) * 8;          // first of this lane's 8 pixels inside its image
    const long long plane = (long long)plane_pieces * 8;              // H * W
    const half_t* src = img + image * 3 * plane + px;
    h8_t ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ch[c] = *reinterpret_cast<const h8_t*>(src + c * plane);
    const long long o0 = (image * plane + px) * 3;                    // element index of the first output value
    if (kKind == DSC_IMAGE_U8) {
        unsigned char v[24];
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * e + c] = (unsigned char)rintf((float)finish_value(ch[c][e]) * 255.0f);
        u2_t* dst = reinterpret_cast<u2_t*>(static_cast<unsigned char*>(out) + o0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u2_t w;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                w[j] = (unsigned)v[8 * k + 4 * j] | ((unsigned)v[8 * k + 4 * j + 1] << 8) | ((unsigned)v[8 * k + 4 * j + 2] << 16) |
                       ((unsigned)v[8 * k + 4 * j + 3] << 24);
            dst[k] = w;
        }
    } else {
        float v[24];
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * e + c] = (float)finish_value(ch[c][e]);
        f4x_t* dst = reinterpret_cast<f4x_t*>(static_cast<float*>(out) + o0);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const f4x_t w = {v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
            dst[k] = w;
        }
    }
}

}  // namespace

extern "C" int dsc_image_finish(const void* img, void* out, int n, int H, int W, int out_kind, void* stream) {
    if (!img || !out || img == out) return DSC_ERR_BAD_ARG;
    if (n < 1 || H < 1 || W < 1) return DSC_ERR_BAD_ARG;
    if (out_kind != DSC_IMAGE_U8 && out_kind != DSC_IMAGE_F32) return DSC_ERR_BAD_ARG;
    if (H % 8 != 0 || W % 8 != 0) return DSC_ERR_UNSUPPORTED;
    const long long plane_pieces = (long long)H * W / 8;
    const long long pieces = (long long)n * plane_pieces;
    if (plane_pieces >= (1ll << 31) || (pieces + 255) / 256 >= (1ll << 31)) return DSC_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(img) & 15) return DSC_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(out) & (out_kind == DSC_IMAGE_U8 ? 7 : 15)) return DSC_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((pieces + 255) / 256)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const half_t* ip = static_cast<const half_t*>(img);
    if (out_kind == DSC_IMAGE_U8)
        DSC_LAUNCH(image_finish_kernel<DSC_IMAGE_U8>, grid, block, 0, st, ip, out, pieces, (int)plane_pieces);
    else
        DSC_LAUNCH(image_finish_kernel<DSC_IMAGE_F32>, grid, block, 0, st, ip, out, pieces, (int)plane_pieces);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
