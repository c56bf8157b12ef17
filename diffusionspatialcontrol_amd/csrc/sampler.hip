// Fused sampler-step kernels (include/dsc_hip.h: dsc_prepare_unet_input, dsc_cfg_dpmpp2m_step, dsc_dpmpp2m_update).
// Pure HBM-bound elementwise work on [n_img, 4, h, w] latents (32 KB per 512x512 image): the point is launch
// count - one launch per step instead of ~10 - and keeping sigma / t on the device for the captured UNet graph.
#include "dsc_common.h"
#include "dsc_hip.h"

namespace {

__device__ __forceinline__ void unpack8(const h8_t v, float (&f)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
}
__device__ __forceinline__ h8_t pack8(const float (&f)[8]) {
    h8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (half_t)f[j];
    return v;
}

// V halfs per access: 8 (16 bytes) where a latent row holds a multiple of 8 halfs, else 4 - rows of 4 h w halfs with h w odd (the
// 19 x 19 latents of a 152 x 152 image) are only 8-byte aligned.  The arithmetic per element is the same: equal bits.
template <int V> struct hv_sel;
template <> struct hv_sel<8> { typedef h8_t type; };
template <> struct hv_sel<4> { typedef h4_t type; };
template <int V> using hv_t = typename hv_sel<V>::type;
template <int V>
__device__ __forceinline__ void unpackv(const hv_t<V> v, float (&f)[V]) {
#pragma unroll
    for (int j = 0; j < V; ++j) f[j] = (float)v[j];
}
template <int V>
__device__ __forceinline__ hv_t<V> packv(const float (&f)[V]) {
    hv_t<V> v;
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = (half_t)f[j];
    return v;
}

// the step's row of a per-generation table (the time-embedding projections of every ResNet block for this step's timestep,
// computed for all steps before the loop) copied to every row of the static buffer the captured UNet step reads
__device__ __forceinline__ void copy_row(const half_t* src, half_t* dst, int halfs, int copies) {
    if (!src) return;
    const int v8 = halfs / 8;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < (long long)v8 * copies; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / v8), c = (int)(i - (long long)r * v8);
        *reinterpret_cast<h8_t*>(dst + (long long)r * halfs + c * 8) = *reinterpret_cast<const h8_t*>(src + c * 8);
    }
}

template <int V>
__global__ __launch_bounds__(256) void prepare_kernel(const half_t* x, float c_in, float t, float sigma, half_t* x_in,
                                                      float* t_buf, float* sigma_buf, int n_img, int chw,
                                                      const half_t* row_src, half_t* row_dst, int row_halfs, int row_copies) {
    copy_row(row_src, row_dst, row_halfs, row_copies);
    const long long n8 = (long long)n_img * chw / V;
    const long long half_elems = (long long)n_img * chw;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        float f[V];
        unpackv<V>(*reinterpret_cast<const hv_t<V>*>(x + i * V), f);
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] *= c_in;
        const hv_t<V> o = packv<V>(f);
        *reinterpret_cast<hv_t<V>*>(x_in + i * V) = o;
        *reinterpret_cast<hv_t<V>*>(x_in + half_elems + i * V) = o;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < 2 * n_img) t_buf[threadIdx.x] = t;
        for (int i = threadIdx.x + 256; i < 2 * n_img; i += 256) t_buf[i] = t;
        if (threadIdx.x == 0) sigma_buf[0] = sigma;
    }
}

template <int V>
__global__ __launch_bounds__(256) void step_kernel(half_t* x, const half_t* eps, half_t* old, float sigma, float g,
                                                   float a, float b, float c, float c_in_next, float t_next,
                                                   float sigma_next, half_t* x_in, float* t_buf, float* sigma_buf,
                                                   int n_img, int chw,
                                                   const half_t* row_src, half_t* row_dst, int row_halfs, int row_copies) {
    copy_row(row_src, row_dst, row_halfs, row_copies);
    const long long half_elems = (long long)n_img * chw;
    const long long n8 = half_elems / V;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        float xv[V], eu[V], ec[V], ov[V], dn[V], xn[V], xi[V];
        unpackv<V>(*reinterpret_cast<const hv_t<V>*>(x + i * V), xv);
        unpackv<V>(*reinterpret_cast<const hv_t<V>*>(eps + i * V), eu);
        unpackv<V>(*reinterpret_cast<const hv_t<V>*>(eps + half_elems + i * V), ec);
        unpackv<V>(*reinterpret_cast<const hv_t<V>*>(old + i * V), ov);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float e = eu[j] + g * (ec[j] - eu[j]);          // model_k_diffusion.py:1162-1166 (affine in eps)
            dn[j] = (float)(half_t)(xv[j] - sigma * e);           // external_k_diffusion.py:114, stored as fp16
            xn[j] = (float)(half_t)(a * xv[j] + b * dn[j] + c * ov[j]);
            xi[j] = xn[j] * c_in_next;
        }
        *reinterpret_cast<hv_t<V>*>(old + i * V) = packv<V>(dn);
        *reinterpret_cast<hv_t<V>*>(x + i * V) = packv<V>(xn);
        const hv_t<V> o = packv<V>(xi);
        *reinterpret_cast<hv_t<V>*>(x_in + i * V) = o;
        *reinterpret_cast<hv_t<V>*>(x_in + half_elems + i * V) = o;
    }
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < 2 * n_img; i += 256) t_buf[i] = t_next;
        if (threadIdx.x == 0) sigma_buf[0] = sigma_next;
    }
}

template <int V>
__global__ __launch_bounds__(256) void update_kernel(const half_t* x, const half_t* den, const half_t* old, float a,
                                                     float b, float c, half_t* out, long long n8) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        float xv[V], dv[V], ov[V], r[V];
        unpackv<V>(*reinterpret_cast<const hv_t<V>*>(x + i * V), xv);
        unpackv<V>(*reinterpret_cast<const hv_t<V>*>(den + i * V), dv);
        if (old) unpackv<V>(*reinterpret_cast<const hv_t<V>*>(old + i * V), ov);
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = a * xv[j] + b * dv[j] + (old ? c * ov[j] : 0.f);
        *reinterpret_cast<hv_t<V>*>(out + i * V) = packv<V>(r);
    }
}

// an fp32 value the compiler must materialise: keeps `(half)(fp32 expression)` two roundings (fp32 result, then fp16), as in
// step_kernel / prepare_kernel, instead of a mixed-precision fma that rounds the exact result to fp16 once (1 ulp apart)
__device__ __forceinline__ float as_f32(float v) {
    __asm__ volatile("" : "+v"(v));
    return v;
}

// ---- what the per-row kernels below share (slot i = blockIdx.y; T: the workgroup size, 256 for the first three)
// the slot's time-embedding row -> both of its CFG rows of the destination bucket
template <int T = 256>
__device__ __forceinline__ void rows_copy_temb(const void* temb_row, half_t* tadd, int tadd_halfs, int n_dst, int i) {
    if (!temb_row) return;
    const int t8 = tadd_halfs / 8;
    for (int j = blockIdx.x * T + threadIdx.x; j < 2 * t8; j += gridDim.x * T) {
        const int h = j >= t8, c = j - h * t8;
        *reinterpret_cast<h8_t*>(tadd + ((long long)(h ? n_dst + i : i) * tadd_halfs) + c * 8) =
            reinterpret_cast<const h8_t*>(temb_row)[c];
    }
}
// JOIN: prepare_kernel's line for a freshly loaded start latent (a request's first model call: never blended), old row zeroed;
// IDLE: zero input rows
template <int T = 256, int V = 8>
__device__ __forceinline__ void rows_join_or_idle(bool join, float c_in, const half_t* xr, half_t* orow, half_t* xi_u, half_t* xi_c,
                                                  long long v8) {
    for (long long k = blockIdx.x * (long long)T + threadIdx.x; k < v8; k += (long long)gridDim.x * T) {
        hv_t<V> o;
        if (join) {
            float f[V];
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(xr + k * V), f);
#pragma unroll
            for (int j = 0; j < V; ++j) f[j] = as_f32(f[j] * c_in);
            o = packv<V>(f);
            *reinterpret_cast<hv_t<V>*>(orow + k * V) = hv_t<V>{};
        } else {
            o = hv_t<V>{};
        }
        *reinterpret_cast<hv_t<V>*>(xi_u + k * V) = o;
        *reinterpret_cast<hv_t<V>*>(xi_c + k * V) = o;
    }
}
// t of both CFG rows and the sigma of the slot's std group
__device__ __forceinline__ void rows_write_scalars(float* t_buf, float* sigma_groups, int n_dst, int i, float t_next, float sigma) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        t_buf[i] = t_next;
        t_buf[n_dst + i] = t_next;
        sigma_groups[i] = sigma;
    }
}

// dsc_cfg_linear_step_rows_cat: the channels a 9-channel inpainting UNet reads beside the latent (reference
// model_k_diffusion.py:1617-1619), scaled like the latent by the coming step's c_in; zeros for an IDLE slot or one without a row
template <int T = 256>
__device__ __forceinline__ void rows_cat_extra(const void* extra, bool idle, float c_in, half_t* xe_u, half_t* xe_c, int e8) {
    const half_t* ex = idle ? nullptr : static_cast<const half_t*>(extra);      // per slot: uniform per workgroup
    for (int k = blockIdx.x * T + threadIdx.x; k < e8; k += gridDim.x * T) {
        h8_t o{};
        if (ex) {
            float f[8];
            unpack8(*reinterpret_cast<const h8_t*>(ex + k * 8), f);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = as_f32(f[j] * c_in);
            o = pack8(f);
        }
        *reinterpret_cast<h8_t*>(xe_u + k * 8) = o;
        *reinterpret_cast<h8_t*>(xe_c + k * 8) = o;
    }
}

// dsc_cfg_dpmpp2m_step_rows: the records ride in the kernel arguments (kernarg segment, read through scalar loads: the slot is
// blockIdx.y, uniform per workgroup)
struct RowSteps { dsc_row_step r[DSC_ROW_STEP_MAX_SLOTS]; };

template <int V>
__global__ __launch_bounds__(256) void step_rows_kernel(half_t* x, const half_t* eps, half_t* old, int n_src, half_t* x_in,
                                                        float* t_buf, float* sigma_groups, half_t* tadd, int tadd_halfs,
                                                        int n_dst, int chw, const RowSteps rs) {
    const int i = blockIdx.y;
    const dsc_row_step& r = rs.r[i];
    const bool dst = i < n_dst;
    const long long v8 = chw / V;
    if (dst) rows_copy_temb(r.temb_row, tadd, tadd_halfs, n_dst, i);
    half_t* xi_u = x_in + (long long)i * chw;
    half_t* xi_c = x_in + (long long)(n_dst + i) * chw;
    if (r.mode == DSC_ROW_STEP) {
        const float sigma = r.sigma, g = r.guidance, a = r.a, b = r.b, c = r.c, c_in_next = r.c_in_next;
        half_t* xr = x + (long long)i * chw;
        half_t* orow = old + (long long)i * chw;
        const half_t* eur = eps + (long long)i * chw;
        const half_t* ecr = eps + (long long)(n_src + i) * chw;
        for (long long k = blockIdx.x * 256ll + threadIdx.x; k < v8; k += (long long)gridDim.x * 256) {
            float xv[V], eu[V], ec[V], ov[V], dn[V], xn[V], xi[V];
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(xr + k * V), xv);
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(eur + k * V), eu);
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(ecr + k * V), ec);
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(orow + k * V), ov);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                // step_kernel's arithmetic with the fused multiply-adds it compiles to, spelled out (the contraction of a
                // plain expression depends on the surrounding code, and the per-row step must give the same bits):
                // e = fma(g, ec - eu, eu), D = fma(-sigma, e, x), x' = fma(c, old, fma(a, x, b * D))
                const float e = as_f32(__builtin_fmaf(g, ec[j] - eu[j], eu[j]));
                dn[j] = (float)(half_t)as_f32(__builtin_fmaf(-sigma, e, xv[j]));
                const float bd = as_f32(b * dn[j]);
                xn[j] = (float)(half_t)as_f32(__builtin_fmaf(c, ov[j], as_f32(__builtin_fmaf(a, xv[j], bd))));
                xi[j] = as_f32(xn[j] * c_in_next);
            }
            *reinterpret_cast<hv_t<V>*>(orow + k * V) = packv<V>(dn);
            *reinterpret_cast<hv_t<V>*>(xr + k * V) = packv<V>(xn);
            if (dst) {
                const hv_t<V> o = packv<V>(xi);
                *reinterpret_cast<hv_t<V>*>(xi_u + k * V) = o;
                *reinterpret_cast<hv_t<V>*>(xi_c + k * V) = o;
            }
        }
    } else if (dst) {
        rows_join_or_idle<256, V>(r.mode == DSC_ROW_JOIN, r.c_in_next, x + (long long)i * chw, old + (long long)i * chw, xi_u, xi_c, v8);
    }
    if (dst) rows_write_scalars(t_buf, sigma_groups, n_dst, i, r.t_next, r.mode == DSC_ROW_IDLE ? 1.0f : r.sigma_next);
}

// dsc_cfg_dpmpp2m_step_rows_known: step_rows_kernel plus, per slot, the known region of an inpainting request blended into the
// model input (what the eager hook of `inpaiting` did per model call, reference model_k_diffusion.py:1599-1612).  A slot whose
// record has no image runs step_rows_kernel's arithmetic unchanged (same bits); JOIN / IDLE slots never look at the record.
struct RowKnowns { dsc_row_known r[DSC_ROW_STEP_MAX_SLOTS]; };

template <int V>
__global__ __launch_bounds__(256) void step_rows_known_kernel(half_t* x, const half_t* eps, half_t* old, int n_src, half_t* x_in,
                                                              float* t_buf, float* sigma_groups, half_t* tadd, int tadd_halfs,
                                                              int n_dst, int chw, const RowSteps rs, const RowKnowns ks) {
    const int i = blockIdx.y;
    const dsc_row_step& r = rs.r[i];
    const dsc_row_known& kr = ks.r[i];
    const bool dst = i < n_dst;
    const long long v8 = chw / V;
    if (dst) rows_copy_temb(r.temb_row, tadd, tadd_halfs, n_dst, i);
    half_t* xi_u = x_in + (long long)i * chw;
    half_t* xi_c = x_in + (long long)(n_dst + i) * chw;
    if (r.mode == DSC_ROW_STEP) {
        const float sigma = r.sigma, g = r.guidance, a = r.a, b = r.b, c = r.c, c_in_next = r.c_in_next;
        const float sigma_next = r.sigma_next;
        const half_t* img = static_cast<const half_t*>(kr.image);
        const half_t* nse = static_cast<const half_t*>(kr.noise);
        const half_t* msk = static_cast<const half_t*>(kr.mask);
        const bool now = img && kr.blend_now, next = img && kr.blend_next && dst;
        half_t* xr = x + (long long)i * chw;
        half_t* orow = old + (long long)i * chw;
        const half_t* eur = eps + (long long)i * chw;
        const half_t* ecr = eps + (long long)(n_src + i) * chw;
        for (long long k = blockIdx.x * 256ll + threadIdx.x; k < v8; k += (long long)gridDim.x * 256) {
            float xv[V], eu[V], ec[V], ov[V], dn[V], xn[V], xi[V], im[V], nz[V], mk[V];
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(xr + k * V), xv);
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(eur + k * V), eu);
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(ecr + k * V), ec);
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(orow + k * V), ov);
            if (now || next) {
                unpackv<V>(*reinterpret_cast<const hv_t<V>*>(img + k * V), im);
                unpackv<V>(*reinterpret_cast<const hv_t<V>*>(nse + k * V), nz);
                unpackv<V>(*reinterpret_cast<const hv_t<V>*>(msk + k * V), mk);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                // step_rows_kernel's lines; the model input xh replaces x in D only - the sampler's own state stays unblended
                const float e = as_f32(__builtin_fmaf(g, ec[j] - eu[j], eu[j]));
                float xh = xv[j];
                if (now) {
                    const float kn = as_f32(__builtin_fmaf(sigma, nz[j], im[j]));          // known region at this sigma
                    xh = as_f32(__builtin_fmaf(mk[j], xv[j], as_f32((1.0f - mk[j]) * kn)));
                }
                dn[j] = (float)(half_t)as_f32(__builtin_fmaf(-sigma, e, xh));
                const float bd = as_f32(b * dn[j]);
                xn[j] = (float)(half_t)as_f32(__builtin_fmaf(c, ov[j], as_f32(__builtin_fmaf(a, xv[j], bd))));
                float xo = xn[j];
                if (next) {
                    const float kn = as_f32(__builtin_fmaf(sigma_next, nz[j], im[j]));     // ... and at the coming one
                    xo = as_f32(__builtin_fmaf(mk[j], xn[j], as_f32((1.0f - mk[j]) * kn)));
                }
                xi[j] = as_f32(xo * c_in_next);
            }
            *reinterpret_cast<hv_t<V>*>(orow + k * V) = packv<V>(dn);
            *reinterpret_cast<hv_t<V>*>(xr + k * V) = packv<V>(xn);
            if (dst) {
                const hv_t<V> o = packv<V>(xi);
                *reinterpret_cast<hv_t<V>*>(xi_u + k * V) = o;
                *reinterpret_cast<hv_t<V>*>(xi_c + k * V) = o;
            }
        }
    } else if (dst) {
        rows_join_or_idle<256, V>(r.mode == DSC_ROW_JOIN, r.c_in_next, x + (long long)i * chw, old + (long long)i * chw, xi_u, xi_c, v8);
    }
    if (dst) rows_write_scalars(t_buf, sigma_groups, n_dst, i, r.t_next, r.mode == DSC_ROW_IDLE ? 1.0f : r.sigma_next);
}

// dsc_cfg_linear_step_rows: step_rows_kernel with the denoised estimate affine in (x, model output) - D = c_skip x + c_out m, eps- or
// v-prediction - and an optional per-slot noise row: x' = a x + b D + c D_old + s xi, the one-model-call-per-step samplers of
// modules/sampling.py (sample_euler, sample_euler_ancestral, sample_dpmpp_2m, sample_dpmpp_2m_sde, sample_lcm of
// samplers_extra_k_diffusion.py) with their scalars computed on the host (sampling.linear_step_coefficients).  A slot with
// c_skip = 1, c_out = -sigma and no noise row runs step_rows_kernel's arithmetic (same bits); JOIN / IDLE slots are its lines.
struct RowLinears { dsc_row_linear r[DSC_ROW_STEP_MAX_SLOTS]; };
// CAT (dsc_cfg_linear_step_rows_cat): an x_in row is chw + extra_halfs halfs long and ends with the slot's extra channels
struct RowExtras { dsc_row_extra r[DSC_ROW_STEP_MAX_SLOTS]; };

template <bool CAT>
__device__ __forceinline__ void linear_rows_body(half_t* x, const half_t* eps, half_t* old, int n_src, half_t* x_in,
                                                 float* t_buf, float* sigma_groups, half_t* tadd, int tadd_halfs,
                                                 int n_dst, int chw, const RowLinears& rs, int extra_halfs, const RowExtras* es) {
    const int i = blockIdx.y;
    const dsc_row_linear& r = rs.r[i];
    const bool dst = i < n_dst;
    const long long v8 = chw / 8;
    if (dst) rows_copy_temb(r.temb_row, tadd, tadd_halfs, n_dst, i);
    const long long xs = CAT ? (long long)chw + extra_halfs : chw;         // halfs per x_in row
    half_t* xi_u = x_in + (long long)i * xs;
    half_t* xi_c = x_in + (long long)(n_dst + i) * xs;
    if (CAT && dst) rows_cat_extra(es->r[i].extra, r.mode == DSC_ROW_IDLE, r.c_in_next, xi_u + chw, xi_c + chw, extra_halfs / 8);
    if (r.mode == DSC_ROW_STEP) {
        const float g = r.guidance, a = r.a, b = r.b, c = r.c, c_in_next = r.c_in_next;
        const float c_skip = r.c_skip, c_out = r.c_out, s = r.s;
        const half_t* nse = static_cast<const half_t*>(r.noise);            // per slot: the branch below is uniform per workgroup
        half_t* xr = x + (long long)i * chw;
        half_t* orow = old + (long long)i * chw;
        const half_t* eur = eps + (long long)i * chw;
        const half_t* ecr = eps + (long long)(n_src + i) * chw;
        for (long long k = blockIdx.x * 256ll + threadIdx.x; k < v8; k += (long long)gridDim.x * 256) {
            float xv[8], eu[8], ec[8], ov[8], dn[8], xn[8], xi[8], nz[8];
            unpack8(*reinterpret_cast<const h8_t*>(xr + k * 8), xv);
            unpack8(*reinterpret_cast<const h8_t*>(eur + k * 8), eu);
            unpack8(*reinterpret_cast<const h8_t*>(ecr + k * 8), ec);
            unpack8(*reinterpret_cast<const h8_t*>(orow + k * 8), ov);
            if (nse) unpack8(*reinterpret_cast<const h8_t*>(nse + k * 8), nz);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // e = fma(g, ec - eu, eu), D = fma(c_out, e, c_skip * x), x' = fma(s, xi, fma(c, old, fma(a, x, b * D)))
                const float e = as_f32(__builtin_fmaf(g, ec[j] - eu[j], eu[j]));
                const float sx = as_f32(c_skip * xv[j]);
                dn[j] = (float)(half_t)as_f32(__builtin_fmaf(c_out, e, sx));
                const float bd = as_f32(b * dn[j]);
                float xo = as_f32(__builtin_fmaf(c, ov[j], as_f32(__builtin_fmaf(a, xv[j], bd))));
                if (nse) xo = as_f32(__builtin_fmaf(s, nz[j], xo));
                xn[j] = (float)(half_t)xo;
                xi[j] = as_f32(xn[j] * c_in_next);
            }
            *reinterpret_cast<h8_t*>(orow + k * 8) = pack8(dn);
            *reinterpret_cast<h8_t*>(xr + k * 8) = pack8(xn);
            if (dst) {
                const h8_t o = pack8(xi);
                *reinterpret_cast<h8_t*>(xi_u + k * 8) = o;
                *reinterpret_cast<h8_t*>(xi_c + k * 8) = o;
            }
        }
    } else if (dst) {
        rows_join_or_idle(r.mode == DSC_ROW_JOIN, r.c_in_next, x + (long long)i * chw, old + (long long)i * chw, xi_u, xi_c, v8);
    }
    if (dst) rows_write_scalars(t_buf, sigma_groups, n_dst, i, r.t_next, r.mode == DSC_ROW_IDLE ? 1.0f : r.sigma_next);
}

__global__ __launch_bounds__(256) void linear_rows_kernel(half_t* x, const half_t* eps, half_t* old, int n_src, half_t* x_in,
                                                          float* t_buf, float* sigma_groups, half_t* tadd, int tadd_halfs,
                                                          int n_dst, int chw, const RowLinears rs) {
    linear_rows_body<false>(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, chw, rs, 0, nullptr);
}
__global__ __launch_bounds__(256) void linear_rows_cat_kernel(half_t* x, const half_t* eps, half_t* old, int n_src, half_t* x_in,
                                                              float* t_buf, float* sigma_groups, half_t* tadd, int tadd_halfs,
                                                              int n_dst, int chw, const RowLinears rs, int extra_halfs,
                                                              const RowExtras es) {
    linear_rows_body<true>(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, chw, rs, extra_halfs, &es);
}

// dsc_cfg_linear_step_rows_rescale: linear_rows_kernel with the guidance rescale of arXiv 2305.08891 sec. 3.4 per slot, applied
// - as the reference does - to the denoised estimate: D' = K D, K = phi sqrt(SSD(D_c) / SSD(D)) + (1 - phi), the two sums of
// squared deviations taken over the slot's whole row.  x is updated in place, so a slot with phi > 0 belongs to ONE workgroup
// (blockIdx.x == 0; the slot's other workgroups leave once the embedding row is copied): it reads x / m_u / m_c for the four
// sums, meets at the workgroup barrier of the across-wave sum - after which no thread reads the old x of an element it does
// not own - and then updates the row, every thread the elements it alone reads and writes.  Slots with phi == 0 and JOIN /
// IDLE slots keep linear_rows_kernel's striding over gridDim.x and its bits.  No atomics, nothing crosses workgroups.
// The sums have one fixed order: per thread over k = tid, tid + T, ... (8 halfs in order each), a 6-stage xor butterfly in the
// wave (32, 16, .. 1: every lane ends with the same value), then waves 0 .. T/64 - 1 in order out of LDS.
#ifndef DSC_RESCALE_THREADS
#define DSC_RESCALE_THREADS 1024
#endif
struct RowRescales { float phi[DSC_ROW_STEP_MAX_SLOTS]; };

template <int T, bool CAT>
__device__ __forceinline__ void linear_rows_rescale_body(half_t* x, const half_t* eps, half_t* old, int n_src, half_t* x_in,
                                                         float* t_buf, float* sigma_groups, half_t* tadd, int tadd_halfs,
                                                         int n_dst, int chw, const RowLinears& rs, const RowRescales& ps,
                                                         int extra_halfs, const RowExtras* es) {
    static_assert(T % 64 == 0 && T <= 1024, "whole waves");
    __shared__ double red[T / 64][4];
    const int i = blockIdx.y;
    const dsc_row_linear& r = rs.r[i];
    const bool dst = i < n_dst;
    const long long v8 = chw / 8;
    if (dst) rows_copy_temb<T>(r.temb_row, tadd, tadd_halfs, n_dst, i);
    const long long xs = CAT ? (long long)chw + extra_halfs : chw;         // halfs per x_in row
    half_t* xi_u = x_in + (long long)i * xs;
    half_t* xi_c = x_in + (long long)(n_dst + i) * xs;
    // (before an owned slot's other workgroups leave: the extra channels stride over the whole grid)
    if (CAT && dst) rows_cat_extra<T>(es->r[i].extra, r.mode == DSC_ROW_IDLE, r.c_in_next, xi_u + chw, xi_c + chw, extra_halfs / 8);
    if (r.mode == DSC_ROW_STEP) {
        const float phi = ps.phi[i];
        const bool owned = phi > 0.0f;                                      // per slot: uniform per workgroup
        if (owned && blockIdx.x != 0) return;
        const float g = r.guidance, a = r.a, b = r.b, c = r.c, c_in_next = r.c_in_next;
        const float c_skip = r.c_skip, c_out = r.c_out, s = r.s;
        const half_t* nse = static_cast<const half_t*>(r.noise);
        half_t* xr = x + (long long)i * chw;
        half_t* orow = old + (long long)i * chw;
        const half_t* eur = eps + (long long)i * chw;
        const half_t* ecr = eps + (long long)(n_src + i) * chw;
        float K = 1.0f;
        if (owned) {
            double sc = 0.0, qc = 0.0, sg = 0.0, qg = 0.0;                   // sum Dc, sum Dc^2, sum Dg, sum Dg^2
            for (long long k = threadIdx.x; k < v8; k += T) {
                float xv[8], eu[8], ec[8];
                unpack8(*reinterpret_cast<const h8_t*>(xr + k * 8), xv);
                unpack8(*reinterpret_cast<const h8_t*>(eur + k * 8), eu);
                unpack8(*reinterpret_cast<const h8_t*>(ecr + k * 8), ec);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float e = as_f32(__builtin_fmaf(g, ec[j] - eu[j], eu[j]));
                    const float sx = as_f32(c_skip * xv[j]);
                    const double dc = (double)as_f32(__builtin_fmaf(c_out, ec[j], sx));
                    const double dg = (double)as_f32(__builtin_fmaf(c_out, e, sx));
                    sc += dc;
                    qc = __builtin_fma(dc, dc, qc);
                    sg += dg;
                    qg = __builtin_fma(dg, dg, qg);
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                sc += __shfl_xor(sc, m);
                qc += __shfl_xor(qc, m);
                sg += __shfl_xor(sg, m);
                qg += __shfl_xor(qg, m);
            }
            if ((threadIdx.x & 63) == 0) {
                double* w = red[threadIdx.x >> 6];
                w[0] = sc, w[1] = qc, w[2] = sg, w[3] = qg;
            }
            __syncthreads();                                                // also: every read of the old x row is done
            sc = qc = sg = qg = 0.0;
            for (int w = 0; w < T / 64; ++w) {
                sc += red[w][0];
                qc += red[w][1];
                sg += red[w][2];
                qg += red[w][3];
            }
            const double n = (double)chw;
            const double ssd_c = qc - sc * sc / n, ssd_g = qg - sg * sg / n;   // (the n - 1 of both stds cancels)
            K = (float)((double)phi * __builtin_sqrt(ssd_c / ssd_g) + (1.0 - (double)phi));
        }
        const long long k0 = owned ? threadIdx.x : blockIdx.x * (long long)T + threadIdx.x;
        const long long dk = owned ? T : (long long)gridDim.x * T;
        for (long long k = k0; k < v8; k += dk) {
            float xv[8], eu[8], ec[8], ov[8], dn[8], xn[8], xi[8], nz[8];
            unpack8(*reinterpret_cast<const h8_t*>(xr + k * 8), xv);
            unpack8(*reinterpret_cast<const h8_t*>(eur + k * 8), eu);
            unpack8(*reinterpret_cast<const h8_t*>(ecr + k * 8), ec);
            unpack8(*reinterpret_cast<const h8_t*>(orow + k * 8), ov);
            if (nse) unpack8(*reinterpret_cast<const h8_t*>(nse + k * 8), nz);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // linear_rows_kernel's lines, D scaled by K before its fp16 rounding in an owned slot
                const float e = as_f32(__builtin_fmaf(g, ec[j] - eu[j], eu[j]));
                const float sx = as_f32(c_skip * xv[j]);
                float dg = as_f32(__builtin_fmaf(c_out, e, sx));
                if (owned) dg = as_f32(K * dg);
                dn[j] = (float)(half_t)dg;
                const float bd = as_f32(b * dn[j]);
                float xo = as_f32(__builtin_fmaf(c, ov[j], as_f32(__builtin_fmaf(a, xv[j], bd))));
                if (nse) xo = as_f32(__builtin_fmaf(s, nz[j], xo));
                xn[j] = (float)(half_t)xo;
                xi[j] = as_f32(xn[j] * c_in_next);
            }
            *reinterpret_cast<h8_t*>(orow + k * 8) = pack8(dn);
            *reinterpret_cast<h8_t*>(xr + k * 8) = pack8(xn);
            if (dst) {
                const h8_t o = pack8(xi);
                *reinterpret_cast<h8_t*>(xi_u + k * 8) = o;
                *reinterpret_cast<h8_t*>(xi_c + k * 8) = o;
            }
        }
    } else if (dst) {
        rows_join_or_idle<T>(r.mode == DSC_ROW_JOIN, r.c_in_next, x + (long long)i * chw, old + (long long)i * chw, xi_u, xi_c, v8);
    }
    if (dst) rows_write_scalars(t_buf, sigma_groups, n_dst, i, r.t_next, r.mode == DSC_ROW_IDLE ? 1.0f : r.sigma_next);
}

template <int T>
__global__ __launch_bounds__(T) void linear_rows_rescale_kernel(half_t* x, const half_t* eps, half_t* old, int n_src, half_t* x_in,
                                                                float* t_buf, float* sigma_groups, half_t* tadd, int tadd_halfs,
                                                                int n_dst, int chw, const RowLinears rs, const RowRescales ps) {
    linear_rows_rescale_body<T, false>(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, chw, rs, ps, 0, nullptr);
}
template <int T>
__global__ __launch_bounds__(T) void linear_rows_rescale_cat_kernel(half_t* x, const half_t* eps, half_t* old, int n_src,
                                                                    half_t* x_in, float* t_buf, float* sigma_groups, half_t* tadd,
                                                                    int tadd_halfs, int n_dst, int chw, const RowLinears rs,
                                                                    const RowRescales ps, int extra_halfs, const RowExtras es) {
    linear_rows_rescale_body<T, true>(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, chw, rs, ps,
                                      extra_halfs, &es);
}

int grid_for(long long n8) {
    long long g = (n8 + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}
bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

namespace {
int row_args_status(const void* row_src, const void* row_dst, int row_halfs, int row_copies) {
    if (!row_src) return DSC_OK;
    if (!row_dst || row_halfs <= 0 || row_copies <= 0) return DSC_ERR_BAD_ARG;
    if (row_halfs % 8 != 0 || !al16(row_src) || !al16(row_dst)) return DSC_ERR_UNSUPPORTED;
    return DSC_OK;
}
// one record of the per-row entries: STEP needs the model output and a source row, JOIN a destination row; an aligned embedding row
int row_record_status(int mode, int i, int n_src, int n_dst, const void* eps, const void* temb_row, bool* any_row) {
    if (mode == DSC_ROW_STEP) {
        if (!eps || i >= n_src) return DSC_ERR_BAD_ARG;
    } else if (mode == DSC_ROW_JOIN) {
        if (i >= n_dst) return DSC_ERR_BAD_ARG;
    } else if (mode != DSC_ROW_IDLE) {
        return DSC_ERR_BAD_ARG;
    }
    if (temb_row) {
        if (!al16(temb_row)) return DSC_ERR_UNSUPPORTED;
        *any_row = true;
    }
    return DSC_OK;
}
}  // namespace

extern "C" int dsc_prepare_unet_input(const void* x, float c_in, float t, float sigma, void* x_in, float* t_buf,
                                      float* sigma_buf, int n_img, int chw, int dtype,
                                      const void* row_src, void* row_dst, int row_halfs, int row_copies, void* stream) {
    if (!x || !x_in || !t_buf || !sigma_buf || n_img <= 0 || chw <= 0) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || chw % 4 != 0 || !al16(x) || !al16(x_in)) return DSC_ERR_UNSUPPORTED;
    if (const int rs = row_args_status(row_src, row_dst, row_halfs, row_copies)) return rs;
    const int V = chw % 8 == 0 ? 8 : 4;               // (4: latent rows of 4 h w halfs with h w odd)
    const long long n8 = (long long)n_img * chw / V;
#define DSC_PREPARE(VV) DSC_LAUNCH(prepare_kernel<VV>, dim3(grid_for(n8)), dim3(256), 0, static_cast<hipStream_t>(stream), \
                       static_cast<const half_t*>(x), c_in, t, sigma, static_cast<half_t*>(x_in), t_buf, sigma_buf, \
                       n_img, chw, static_cast<const half_t*>(row_src), static_cast<half_t*>(row_dst), row_halfs, row_copies)
    if (V == 8) DSC_PREPARE(8); else DSC_PREPARE(4);
#undef DSC_PREPARE
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_cfg_dpmpp2m_step(void* x, const void* eps, void* old, float sigma, float guidance, float a, float b,
                                    float c, float c_in_next, float t_next, float sigma_next, void* x_in, float* t_buf,
                                    float* sigma_buf, int n_img, int chw, int dtype,
                                    const void* row_src, void* row_dst, int row_halfs, int row_copies, void* stream) {
    if (!x || !eps || !old || !x_in || !t_buf || !sigma_buf || n_img <= 0 || chw <= 0) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || chw % 4 != 0 || !al16(x) || !al16(eps) || !al16(old) || !al16(x_in)) return DSC_ERR_UNSUPPORTED;
    if (const int rs = row_args_status(row_src, row_dst, row_halfs, row_copies)) return rs;
    const int V = chw % 8 == 0 ? 8 : 4;
    const long long n8 = (long long)n_img * chw / V;
#define DSC_STEP(VV) DSC_LAUNCH(step_kernel<VV>, dim3(grid_for(n8)), dim3(256), 0, static_cast<hipStream_t>(stream), \
                       static_cast<half_t*>(x), static_cast<const half_t*>(eps), static_cast<half_t*>(old), sigma, \
                       guidance, a, b, c, c_in_next, t_next, sigma_next, static_cast<half_t*>(x_in), t_buf, sigma_buf, \
                       n_img, chw, static_cast<const half_t*>(row_src), static_cast<half_t*>(row_dst), row_halfs, row_copies)
    if (V == 8) DSC_STEP(8); else DSC_STEP(4);
#undef DSC_STEP
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_dpmpp2m_update(const void* x, const void* denoised, const void* old, float a, float b, float c,
                                  void* out, int64_t n, int dtype, void* stream) {
    if (!x || !denoised || !out || n <= 0 || (!old && c != 0.f)) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || n % 4 != 0 || !al16(x) || !al16(denoised) || !al16(out) || (old && !al16(old)))
        return DSC_ERR_UNSUPPORTED;
#define DSC_UPDATE(VV) DSC_LAUNCH(update_kernel<VV>, dim3(grid_for(n / VV)), dim3(256), 0, static_cast<hipStream_t>(stream), \
                       static_cast<const half_t*>(x), static_cast<const half_t*>(denoised), \
                       static_cast<const half_t*>(old), a, b, c, static_cast<half_t*>(out), (long long)(n / VV))
    if (n % 8 == 0) DSC_UPDATE(8); else DSC_UPDATE(4);
#undef DSC_UPDATE
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_cfg_dpmpp2m_step_rows(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                         float* sigma_groups, void* tadd, int tadd_halfs, int n_dst, const dsc_row_step* rows,
                                         int n_slots, int chw, int dtype, void* stream) {
    if (!x || !old || !x_in || !t_buf || !sigma_groups || !rows || n_src < 0 || n_dst <= 0 || chw <= 0) return DSC_ERR_BAD_ARG;
    if (n_slots < n_dst || n_slots > DSC_ROW_STEP_MAX_SLOTS) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || chw % 4 != 0 || !al16(x) || !al16(old) || !al16(x_in) || (eps && !al16(eps))) return DSC_ERR_UNSUPPORTED;
    RowSteps rs{};
    bool any_row = false;
    for (int i = 0; i < n_slots; ++i) {
        const dsc_row_step& r = rows[i];
        if (const int st = row_record_status(r.mode, i, n_src, n_dst, eps, r.temb_row, &any_row)) return st;
        rs.r[i] = r;
    }
    if (any_row) {
        if (!tadd || tadd_halfs <= 0) return DSC_ERR_BAD_ARG;
        if (tadd_halfs % 8 != 0 || !al16(tadd)) return DSC_ERR_UNSUPPORTED;
    }
    const int V = chw % 8 == 0 ? 8 : 4;
    const long long v8 = chw / V;
    long long gx = (v8 + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
#define DSC_STEP_ROWS(VV) DSC_LAUNCH(step_rows_kernel<VV>, dim3((unsigned)gx, (unsigned)n_slots), dim3(256), 0, static_cast<hipStream_t>(stream), \
               static_cast<half_t*>(x), static_cast<const half_t*>(eps), static_cast<half_t*>(old), n_src, \
               static_cast<half_t*>(x_in), t_buf, sigma_groups, static_cast<half_t*>(tadd), tadd_halfs, n_dst, chw, rs)
    if (V == 8) DSC_STEP_ROWS(8); else DSC_STEP_ROWS(4);
#undef DSC_STEP_ROWS
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_cfg_dpmpp2m_step_rows_known(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                               float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                                               const dsc_row_step* rows, const dsc_row_known* known, int n_slots, int chw,
                                               int dtype, void* stream) {
    if (!x || !old || !x_in || !t_buf || !sigma_groups || !rows || !known || n_src < 0 || n_dst <= 0 || chw <= 0)
        return DSC_ERR_BAD_ARG;
    if (n_slots < n_dst || n_slots > DSC_ROW_STEP_MAX_SLOTS) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || chw % 4 != 0 || !al16(x) || !al16(old) || !al16(x_in) || (eps && !al16(eps))) return DSC_ERR_UNSUPPORTED;
    RowSteps rs{};
    RowKnowns ks{};
    bool any_row = false;
    for (int i = 0; i < n_slots; ++i) {
        const dsc_row_step& r = rows[i];
        if (r.mode == DSC_ROW_STEP) {
            if (!eps || i >= n_src) return DSC_ERR_BAD_ARG;
            const dsc_row_known& k = known[i];
            const int set = (k.image != nullptr) + (k.noise != nullptr) + (k.mask != nullptr);
            if (set != 0 && set != 3) return DSC_ERR_BAD_ARG;
            if (set && (!al16(k.image) || !al16(k.noise) || !al16(k.mask))) return DSC_ERR_UNSUPPORTED;
            ks.r[i] = k;
        }
        if (const int st = row_record_status(r.mode, i, n_src, n_dst, eps, r.temb_row, &any_row)) return st;
        rs.r[i] = r;
    }
    if (any_row) {
        if (!tadd || tadd_halfs <= 0) return DSC_ERR_BAD_ARG;
        if (tadd_halfs % 8 != 0 || !al16(tadd)) return DSC_ERR_UNSUPPORTED;
    }
    const int V = chw % 8 == 0 ? 8 : 4;
    const long long v8 = chw / V;
    long long gx = (v8 + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
#define DSC_STEP_KNOWN(VV) DSC_LAUNCH(step_rows_known_kernel<VV>, dim3((unsigned)gx, (unsigned)n_slots), dim3(256), 0, static_cast<hipStream_t>(stream), \
               static_cast<half_t*>(x), static_cast<const half_t*>(eps), static_cast<half_t*>(old), n_src, \
               static_cast<half_t*>(x_in), t_buf, sigma_groups, static_cast<half_t*>(tadd), tadd_halfs, n_dst, chw, rs, ks)
    if (V == 8) DSC_STEP_KNOWN(8); else DSC_STEP_KNOWN(4);
#undef DSC_STEP_KNOWN
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_cfg_linear_step_rows(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                        float* sigma_groups, void* tadd, int tadd_halfs, int n_dst, const dsc_row_linear* rows,
                                        int n_slots, int chw, int dtype, void* stream) {
    if (!x || !old || !x_in || !t_buf || !sigma_groups || !rows || n_src < 0 || n_dst <= 0 || chw <= 0) return DSC_ERR_BAD_ARG;
    if (n_slots < n_dst || n_slots > DSC_ROW_STEP_MAX_SLOTS) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || chw % 8 != 0 || !al16(x) || !al16(old) || !al16(x_in) || (eps && !al16(eps))) return DSC_ERR_UNSUPPORTED;
    RowLinears rs{};
    bool any_row = false;
    for (int i = 0; i < n_slots; ++i) {
        const dsc_row_linear& r = rows[i];
        if (const int st = row_record_status(r.mode, i, n_src, n_dst, eps, r.temb_row, &any_row)) return st;
        if (r.mode == DSC_ROW_STEP && r.noise && !al16(r.noise)) return DSC_ERR_UNSUPPORTED;
        rs.r[i] = r;
    }
    if (any_row) {
        if (!tadd || tadd_halfs <= 0) return DSC_ERR_BAD_ARG;
        if (tadd_halfs % 8 != 0 || !al16(tadd)) return DSC_ERR_UNSUPPORTED;
    }
    const long long v8 = chw / 8;
    long long gx = (v8 + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    DSC_LAUNCH(linear_rows_kernel, dim3((unsigned)gx, (unsigned)n_slots), dim3(256), 0, static_cast<hipStream_t>(stream),
               static_cast<half_t*>(x), static_cast<const half_t*>(eps), static_cast<half_t*>(old), n_src,
               static_cast<half_t*>(x_in), t_buf, sigma_groups, static_cast<half_t*>(tadd), tadd_halfs, n_dst, chw, rs);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_cfg_linear_step_rows_rescale(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                                float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                                                const dsc_row_linear* rows, const float* rescale, int n_slots, int chw, int dtype,
                                                void* stream) {
    if (!x || !old || !x_in || !t_buf || !sigma_groups || !rows || !rescale || n_src < 0 || n_dst <= 0 || chw <= 0)
        return DSC_ERR_BAD_ARG;
    if (n_slots < n_dst || n_slots > DSC_ROW_STEP_MAX_SLOTS) return DSC_ERR_BAD_ARG;
    if (dtype != DSC_F16 || chw % 8 != 0 || !al16(x) || !al16(old) || !al16(x_in) || (eps && !al16(eps))) return DSC_ERR_UNSUPPORTED;
    RowLinears rs{};
    RowRescales ps{};
    bool any_row = false;
    for (int i = 0; i < n_slots; ++i) {
        const dsc_row_linear& r = rows[i];
        if (const int st = row_record_status(r.mode, i, n_src, n_dst, eps, r.temb_row, &any_row)) return st;
        if (r.mode == DSC_ROW_STEP) {
            if (r.noise && !al16(r.noise)) return DSC_ERR_UNSUPPORTED;
            if (!(rescale[i] >= 0.0f && rescale[i] <= 1.0f)) return DSC_ERR_BAD_ARG;      // (NaN lands here too)
            ps.phi[i] = rescale[i];
        }
        rs.r[i] = r;
    }
    if (any_row) {
        if (!tadd || tadd_halfs <= 0) return DSC_ERR_BAD_ARG;
        if (tadd_halfs % 8 != 0 || !al16(tadd)) return DSC_ERR_UNSUPPORTED;
    }
    constexpr int T = DSC_RESCALE_THREADS;
    const long long v8 = chw / 8;
    long long gx = (v8 + T - 1) / T;
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    DSC_LAUNCH(linear_rows_rescale_kernel<T>, dim3((unsigned)gx, (unsigned)n_slots), dim3(T), 0, static_cast<hipStream_t>(stream),
               static_cast<half_t*>(x), static_cast<const half_t*>(eps), static_cast<half_t*>(old), n_src,
               static_cast<half_t*>(x_in), t_buf, sigma_groups, static_cast<half_t*>(tadd), tadd_halfs, n_dst, chw, rs, ps);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}

extern "C" int dsc_cfg_linear_step_rows_cat(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                            float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                                            const dsc_row_linear* rows, const float* rescale, const dsc_row_extra* extras,
                                            int extra_halfs, int n_slots, int chw, int dtype, void* stream) {
    if (!x || !old || !x_in || !t_buf || !sigma_groups || !rows || !extras || n_src < 0 || n_dst <= 0 || chw <= 0)
        return DSC_ERR_BAD_ARG;
    if (n_slots < n_dst || n_slots > DSC_ROW_STEP_MAX_SLOTS) return DSC_ERR_BAD_ARG;
    if (extra_halfs <= 0 || extra_halfs % 8 != 0 || chw % 8 != 0) return DSC_ERR_BAD_ARG;     // 16-byte rows of chw + extra_halfs
    if (dtype != DSC_F16 || !al16(x) || !al16(old) || !al16(x_in) || (eps && !al16(eps))) return DSC_ERR_UNSUPPORTED;
    RowLinears rs{};
    RowRescales ps{};
    RowExtras es{};
    bool any_row = false, any_phi = false;
    for (int i = 0; i < n_slots; ++i) {
        const dsc_row_linear& r = rows[i];
        if (const int st = row_record_status(r.mode, i, n_src, n_dst, eps, r.temb_row, &any_row)) return st;
        if (r.mode == DSC_ROW_STEP) {
            if (r.noise && !al16(r.noise)) return DSC_ERR_UNSUPPORTED;
            if (rescale) {
                if (!(rescale[i] >= 0.0f && rescale[i] <= 1.0f)) return DSC_ERR_BAD_ARG;      // (NaN lands here too)
                ps.phi[i] = rescale[i];
                any_phi |= rescale[i] > 0.0f;
            }
        }
        if (extras[i].extra && !al16(extras[i].extra)) return DSC_ERR_BAD_ARG;
        rs.r[i] = r;
        es.r[i] = extras[i];
    }
    if (any_row) {
        if (!tadd || tadd_halfs <= 0) return DSC_ERR_BAD_ARG;
        if (tadd_halfs % 8 != 0 || !al16(tadd)) return DSC_ERR_UNSUPPORTED;
    }
    // the grids of the two entries this one shares its arithmetic with (the extra channels stride over the same grid)
    const long long v8 = chw / 8;
    if (!any_phi) {
        long long gx = (v8 + 255) / 256;
        gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
        DSC_LAUNCH(linear_rows_cat_kernel, dim3((unsigned)gx, (unsigned)n_slots), dim3(256), 0, static_cast<hipStream_t>(stream),
                   static_cast<half_t*>(x), static_cast<const half_t*>(eps), static_cast<half_t*>(old), n_src,
                   static_cast<half_t*>(x_in), t_buf, sigma_groups, static_cast<half_t*>(tadd), tadd_halfs, n_dst, chw, rs,
                   extra_halfs, es);
    } else {
        constexpr int T = DSC_RESCALE_THREADS;
        long long gx = (v8 + T - 1) / T;
        gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
        DSC_LAUNCH(linear_rows_rescale_cat_kernel<T>, dim3((unsigned)gx, (unsigned)n_slots), dim3(T), 0,
                   static_cast<hipStream_t>(stream), static_cast<half_t*>(x), static_cast<const half_t*>(eps),
                   static_cast<half_t*>(old), n_src, static_cast<half_t*>(x_in), t_buf, sigma_groups, static_cast<half_t*>(tadd),
                   tadd_halfs, n_dst, chw, rs, ps, extra_halfs, es);
    }
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
}
