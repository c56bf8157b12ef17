// Live previews of running requests (dsc_latent_preview): up to 16 fp16 latent rows [C, h, w] - the denoised estimate every
// per-row step entry leaves in `old` - become approximate RGB thumbnails, uint8 [n, h * up, w * up, 3], in one launch: a C x 3
// linear map with a bias, `/ 2 + 0.5`, clamp, round to bytes, nearest-neighbour enlargement by up in {1, 2, 4, 8}.
//
// Per latent pixel and colour, all fp32, every product and every sum rounded on its own (pin_f32 keeps the compiler from
// contracting `v + k * z` into an fma, as sampler.hip's as_f32 does for its rounding points):
//     v = bias;  for c in 0..C-1:  v = v + k[c] * float(z[c])
//     y = v * 0.5f + 0.5f;   y = y > 0 ? y : 0;   y = y < 1 ? y : 1           (a NaN compares false: 0)
//     byte = (uint8) rintf(y * 255.0f)
// so a numpy float32 restatement gives the same bits (latent_preview.py).
//
// Launch-bound and tiny (32 KB in per SD1.5 row; 12 KB out at up = 1, 768 KB at up = 8): no LDS, no workspace.  One lane owns 8
// consecutive pixels of ONE OUTPUT ROW: 24 contiguous bytes at an 8-byte-aligned address as three 8-byte stores (the layout of
// image_finish.hip).  The up output rows that share a latent row are written by up different lanes, each of which RECOMPUTES the
// 8 / up latent pixels (at most 8 * 3 * C multiply-adds): the loads hit the cache line the first lane fetched, and one SD1.5 row
// at up = 8 is 128 workgroups of three stores per lane instead of 16 workgroups of 24 stores per lane on a chip of 256 CUs.
// Per channel the lane loads its 8 / up latent pixels in one piece: 16, 8, 4 or 2 bytes (the entry checks the alignment the
// piece needs).  The row indices and the coefficients ride in the kernel arguments, like the step records of sampler.hip: the
// caller's arrays are read on the host at the call.  A lane past the last piece returns before it has formed an address.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

typedef unsigned u2_t __attribute__((ext_vector_type(2)));

struct PreviewArgs {
    int rows[DSC_PREVIEW_MAX_ROWS];
    float k[DSC_PREVIEW_MAX_CHANNELS][3];
    float bias[3];
};

// an fp32 value the compiler must materialise (sampler.hip's as_f32): the product and the sum below stay two roundings
__device__ __forceinline__ float pin_f32(float v) {
    __asm__ volatile("" : "+v"(v));
    return v;
}

template <int P> struct piece_sel;                                   // the load of P latent pixels of one channel
template <> struct piece_sel<8> { typedef h8_t type; };
template <> struct piece_sel<4> { typedef h4_t type; };
template <> struct piece_sel<2> { typedef h2_t type; };

template <int P>
__device__ __forceinline__ void load_piece(const half_t* p, float (&z)[P]) {
    const typename piece_sel<P>::type v = *reinterpret_cast<const typename piece_sel<P>::type*>(p);
#pragma unroll
    for (int e = 0; e < P; ++e) z[e] = (float)v[e];
}
template <>
__device__ __forceinline__ void load_piece<1>(const half_t* p, float (&z)[1]) { z[0] = (float)*p; }

template <int UP>
__global__ __launch_bounds__(256) void latent_preview_kernel(const half_t* __restrict__ lat, long long row_stride, int C, int h, int w,
                                                             unsigned char* __restrict__ out, int pieces, FastDiv row_pieces,
                                                             const PreviewArgs a) {
    constexpr int P = 8 / UP;                                        // latent pixels under this lane's 8 output pixels
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;  // inside thumbnail j = blockIdx.y (uniform: scalar loads)
    if (at >= pieces) return;
    const int piece = (int)at;
    const int j = blockIdx.y;
    const int oy = fdiv(piece, row_pieces);                          // output row
    const int p = piece - oy * row_pieces.d;                         // piece inside the output row
    const int y = oy / UP;                                           // latent row
    const long long plane = (long long)h * w;
    const half_t* src = lat + (long long)a.rows[j] * row_stride + (long long)y * w + (long long)p * P;
    float v[P][3];
#pragma unroll
    for (int e = 0; e < P; ++e)
#pragma unroll
        for (int q = 0; q < 3; ++q) v[e][q] = a.bias[q];
#pragma unroll
    for (int c = 0; c < DSC_PREVIEW_MAX_CHANNELS; ++c) {
        if (c < C) {                                                 // (uniform: C is a launch constant)
            float z[P];
            load_piece<P>(src + c * plane, z);
#pragma unroll
            for (int e = 0; e < P; ++e)
#pragma unroll
                for (int q = 0; q < 3; ++q) v[e][q] = pin_f32(v[e][q] + pin_f32(a.k[c][q] * z[e]));
        }
    }
    unsigned char b[P][3];
#pragma unroll
    for (int e = 0; e < P; ++e)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float yv = pin_f32(pin_f32(v[e][q] * 0.5f) + 0.5f);
            yv = yv > 0.f ? yv : 0.f;
            yv = yv < 1.f ? yv : 1.f;
            b[e][q] = (unsigned char)rintf(yv * 255.0f);
        }
    // output pixel i of the 8 shows latent pixel i / UP: bytes 3 i + q
    u2_t* dst = reinterpret_cast<u2_t*>(out + ((long long)j * pieces + piece) * 24);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u2_t wv;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            unsigned word = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int byte = 8 * k + 4 * d + s;
                word |= (unsigned)b[(byte / 3) / UP][byte % 3] << (8 * s);
            }
            wv[d] = word;
        }
        dst[k] = wv;
    }
}

}  // namespace

extern "C" int dsc_latent_preview(const void* lat, long long row_stride, const int* rows, int n, int C, int h, int w,
                                  const float* coef, int up, void* out, void* stream) {
    if (!lat || !rows || !coef || !out) return DSC_ERR_BAD_ARG;
    if (n < 1 || C < 1 || h < 1 || w < 1) return DSC_ERR_BAD_ARG;
    if (n > DSC_PREVIEW_MAX_ROWS || C > DSC_PREVIEW_MAX_CHANNELS) return DSC_ERR_BAD_ARG;
    if (up != 1 && up != 2 && up != 4 && up != 8) return DSC_ERR_BAD_ARG;
    for (int j = 0; j < n; ++j)
        if (rows[j] < 0) return DSC_ERR_BAD_ARG;
    if (((long long)w * up) % 8 != 0) return DSC_ERR_UNSUPPORTED;
    // the piece of 8 / up halfs a lane loads per channel starts at rows[j] * row_stride + c * h * w + y * w + p * (8 / up): w is
    // a multiple of 8 / up here, so every piece is aligned when the base and the row stride are
    const int piece_halfs = 8 / up;
    if (reinterpret_cast<uintptr_t>(lat) % (2 * piece_halfs) != 0 || row_stride % piece_halfs != 0) return DSC_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(out) & 7) return DSC_ERR_UNSUPPORTED;
    const long long row_pieces = (long long)w * up / 8;
    const long long pieces = (long long)h * up * row_pieces;         // per thumbnail; the thumbnail is the grid's y
    if (pieces >= (1ll << 31)) return DSC_ERR_UNSUPPORTED;
    PreviewArgs a = {};
    for (int j = 0; j < n; ++j) a.rows[j] = rows[j];
    for (int c = 0; c < C; ++c)
        for (int q = 0; q < 3; ++q) a.k[c][q] = coef[3 * c + q];
    for (int q = 0; q < 3; ++q) a.bias[q] = coef[3 * C + q];
    const dim3 grid((unsigned)((pieces + 255) / 256), (unsigned)n), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const half_t* lp = static_cast<const half_t*>(lat);
    unsigned char* op = static_cast<unsigned char*>(out);
    const int np = (int)pieces;
    const FastDiv rp = make_fastdiv(row_pieces, pieces);
    switch (up) {
        case 1: DSC_LAUNCH(latent_preview_kernel<1>, grid, block, 0, st, lp, row_stride, C, h, w, op, np, rp, a); break;
        case 2: DSC_LAUNCH(latent_preview_kernel<2>, grid, block, 0, st, lp, row_stride, C, h, w, op, np, rp, a); break;
        case 4: DSC_LAUNCH(latent_preview_kernel<4>, grid, block, 0, st, lp, row_stride, C, h, w, op, np, rp, a); break;
        default: DSC_LAUNCH(latent_preview_kernel<8>, grid, block, 0, st, lp, row_stride, C, h, w, op, np, rp, a); break;
    }
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
