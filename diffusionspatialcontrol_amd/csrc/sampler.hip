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

// ---- the helpers of the per-row step below (slot i = blockIdx.y; T: the workgroup size)
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

// ---- the per-row step: ONE body behind the six dsc_cfg_*_step_rows* entries.  What every kernel takes, by value in the kernel
// arguments (kernarg segment, read through scalar loads: the slot is blockIdx.y, uniform per workgroup): the buffers and one
// dsc_row_linear per slot - the dsc_cfg_dpmpp2m_* entries fill c_skip = 1, c_out = -sigma, noise = NULL on the host.
struct RowArgs {
    half_t* x; const half_t* eps; half_t* old; int n_src; half_t* x_in; float* t_buf; float* sigma_groups; half_t* tadd;
    int tadd_halfs, n_dst, chw;
    dsc_row_linear r[DSC_ROW_STEP_MAX_SLOTS];
};
// the optional parts, each passed only to the kernels compiled with its flag:
// KNOWN (dsc_cfg_dpmpp2m_step_rows_known): the known region of an inpainting request blended into the model input (what the eager
// hook of `inpaiting` did per model call, reference model_k_diffusion.py:1599-1612); a slot without an image is unblended
struct RowKnowns { dsc_row_known r[DSC_ROW_STEP_MAX_SLOTS]; };
// RESCALE (dsc_cfg_linear_step_rows_rescale): the guidance rescale of arXiv 2305.08891 sec. 3.4 per slot, applied - as the
// reference does - to the denoised estimate: D' = K D, K = phi sqrt(SSD(D_c) / SSD(D)) + (1 - phi), the two sums of squared
// deviations taken over the slot's whole row.  x is updated in place, so a slot with phi > 0 belongs to ONE workgroup
// (blockIdx.x == 0; the slot's other workgroups leave once the embedding row and the extra channels are copied): it reads
// x / m_u / m_c for the four sums, meets at the workgroup barrier of the across-wave sum - after which no thread reads the old x
// of an element it does not own - and then updates the row, every thread the elements it alone reads and writes.  Slots with
// phi == 0 and JOIN / IDLE slots stride over gridDim.x like everyone else.  No atomics, nothing crosses workgroups.
// The sums have one fixed order: per thread over k = tid, tid + T, ... (8 halfs in order each), a 6-stage xor butterfly in the
// wave (32, 16, .. 1: every lane ends with the same value), then waves 0 .. T/64 - 1 in order out of LDS.
#ifndef DSC_RESCALE_THREADS
#define DSC_RESCALE_THREADS 1024
#endif
struct RowRescales { float phi[DSC_ROW_STEP_MAX_SLOTS]; };
// CAT (dsc_cfg_linear_step_rows_cat): an x_in row is chw + halfs halfs long and ends with the slot's extra channels
struct RowExtras { int halfs; dsc_row_extra r[DSC_ROW_STEP_MAX_SLOTS]; };
// STAGED (dsc_cfg_staged_step_rows): the two-call samplers (modules/sampling.py call_plan).  A slot's step is two transitions:
// PREDICT writes the intermediate point into the slot's row of `mid` and leaves x alone; CORRECT - the model ran on mid - takes
// D (and the rescale's sums) from mid and adds m * mid to the update of x.  A FULL slot is the linear step: mid is not touched.
struct RowStages { half_t* mid; dsc_row_stage r[DSC_ROW_STEP_MAX_SLOTS]; };

// T threads, V halfs per access.  A flag that is off compiles its part out; LINEAR off: the record is a DPM++ 2M one, c_skip == 1
// and no noise row by construction (x for 1 x: the same bits, one multiply and a row of registers less).  Per element of a STEP
// slot, all fp32:
//   e = fma(g, m_c - m_u, m_u), D = fp16([K] fma(c_out, e, c_skip xh)), x' = fp16([fma(s, noise,] fma(c, old, fma(a, x, b D))[)]),
//   x_in = fp16(xh' c_in_next) - xh, xh': x, x' with the known region blended in (KNOWN), else x, x' themselves.
// STAGED, PREDICT: x' = fp16([fma(s, noise,] fma(a, x, b D)[)]) goes to mid and into x_in, x stays; CORRECT: xh = mid and
//   x' = fp16([fma(s, noise,] fma(m, mid, fma(c, old, fma(a, x, b D)))[)]).
// These are step_kernel's lines with the fused multiply-adds it compiles to spelled out, every intermediate pinned to fp32 by
// as_f32 (the contraction of a plain expression depends on the surrounding code, and every instantiation must give the same bits).
template <int T, int V, bool LINEAR, bool KNOWN, bool RESCALE, bool CAT, bool STAGED = false>
__device__ __forceinline__ void rows_body(const RowArgs& p, const RowKnowns* ks, const RowRescales* ps, const RowExtras* es,
                                          const RowStages* ss = nullptr) {
    static_assert(T % 64 == 0 && T <= 1024, "whole waves");
    static_assert(!STAGED || (LINEAR && !KNOWN && !CAT && V == 8), "the staged entry is the linear one, without KNOWN and CAT");
    static_assert(!(KNOWN && RESCALE), "the row sums read x: they would have to read the blended model input");
    static_assert(V == 8 || !(RESCALE || CAT), "8-byte rows: the sums and the extra channels move 8 halfs");
    const int i = blockIdx.y, n_dst = p.n_dst, chw = p.chw;
    const dsc_row_linear& r = p.r[i];
    const int mode = r.mode;
    const bool dst = i < n_dst;
    const long long nv = chw / V;
    if (dst) rows_copy_temb<T>(r.temb_row, p.tadd, p.tadd_halfs, n_dst, i);
    const long long xs = CAT ? (long long)chw + es->halfs : chw;           // halfs per x_in row
    half_t* xi_u = p.x_in + (long long)i * xs;
    half_t* xi_c = p.x_in + (long long)(n_dst + i) * xs;
    half_t* xr = p.x + (long long)i * chw;
    half_t* orow = p.old + (long long)i * chw;
    // (before an owned slot's other workgroups leave: the extra channels stride over the whole grid)
    if constexpr (CAT) if (dst) rows_cat_extra<T>(es->r[i].extra, mode == DSC_ROW_IDLE, r.c_in_next, xi_u + chw, xi_c + chw, es->halfs / 8);
    if (mode == DSC_ROW_STEP) {
        bool owned = false;                                                 // per slot: uniform per workgroup, like every branch below
        if constexpr (RESCALE) {
            owned = ps->phi[i] > 0.0f;
            if (owned && blockIdx.x != 0) return;
        }
        const float g = r.guidance, a = r.a, b = r.b, c = r.c, c_in_next = r.c_in_next;
        const float c_skip = r.c_skip, c_out = r.c_out, s = r.s, sigma = r.sigma, sigma_next = r.sigma_next;   // (KNOWN's)
        const half_t* nse = LINEAR ? static_cast<const half_t*>(r.noise) : nullptr;
        const half_t* eur = p.eps + (long long)i * chw;
        const half_t* ecr = p.eps + (long long)(p.n_src + i) * chw;
        const auto combine = [&](float mu, float mc) { return as_f32(__builtin_fmaf(g, mc - mu, mu)); };
        const auto skip = [&](float v) { return LINEAR ? as_f32(c_skip * v) : v; };
        const auto estimate = [&](float m, float sx) { return as_f32(__builtin_fmaf(c_out, m, sx)); };      // D in fp32
        // (STAGED) the row the model call saw: mid in CORRECT, else x
        bool predict = false, correct = false;
        float sm = 0.0f;
        const half_t* srow = xr;
        half_t* midr = nullptr;
        if constexpr (STAGED) {
            predict = ss->r[i].stage == DSC_ROW_STAGE_PREDICT, correct = ss->r[i].stage == DSC_ROW_STAGE_CORRECT;
            sm = ss->r[i].m;
            midr = ss->mid + (long long)i * chw;
            if (correct) srow = midr;
        }
        const half_t *img = nullptr, *knz = nullptr, *msk = nullptr;
        bool now = false, next = false;
        if constexpr (KNOWN) {
            const dsc_row_known& kr = ks->r[i];
            img = static_cast<const half_t*>(kr.image), knz = static_cast<const half_t*>(kr.noise), msk = static_cast<const half_t*>(kr.mask);
            now = img && kr.blend_now, next = img && kr.blend_next && dst;
        }
        // v with the known region at noise level sg in the place of what the mask keeps
        const auto blend = [](float v, float sg, float im, float nz, float mk) {
            const float kn = as_f32(__builtin_fmaf(sg, nz, im));
            return as_f32(__builtin_fmaf(mk, v, as_f32((1.0f - mk) * kn)));
        };
        float K = 1.0f;
        if constexpr (RESCALE) if (owned) {
            __shared__ double red[T / 64][4];
            double sc = 0.0, qc = 0.0, sg = 0.0, qg = 0.0;                   // sum Dc, sum Dc^2, sum Dg, sum Dg^2
            for (long long k = threadIdx.x; k < nv; k += T) {
                float xv[V], eu[V], ec[V];
                unpackv<V>(*reinterpret_cast<const hv_t<V>*>((STAGED ? srow : xr) + k * V), xv);
                unpackv<V>(*reinterpret_cast<const hv_t<V>*>(eur + k * V), eu);
                unpackv<V>(*reinterpret_cast<const hv_t<V>*>(ecr + k * V), ec);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float e = combine(eu[j], ec[j]);
                    const float sx = skip(xv[j]);
                    const double dc = (double)estimate(ec[j], sx);
                    const double dg = (double)estimate(e, sx);
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
            const float phi = ps->phi[i];
            K = (float)((double)phi * __builtin_sqrt(ssd_c / ssd_g) + (1.0 - (double)phi));
        }
        // an owned slot's row is this workgroup's alone; any other strides over the slot's workgroups
        for (long long k = owned ? threadIdx.x : blockIdx.x * (long long)T + threadIdx.x; k < nv;
             k += owned ? T : (long long)gridDim.x * T) {
            float xv[V], eu[V], ec[V], ov[V], dn[V], xn[V], xi[V], nz[V], im[V], kz[V], mk[V], mv[V];
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(xr + k * V), xv);
            if constexpr (STAGED) if (correct) unpackv<V>(*reinterpret_cast<const hv_t<V>*>(midr + k * V), mv);
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(eur + k * V), eu);
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(ecr + k * V), ec);
            unpackv<V>(*reinterpret_cast<const hv_t<V>*>(orow + k * V), ov);
            if (nse) unpackv<V>(*reinterpret_cast<const hv_t<V>*>(nse + k * V), nz);
            if constexpr (KNOWN) if (now || next) {
                unpackv<V>(*reinterpret_cast<const hv_t<V>*>(img + k * V), im);
                unpackv<V>(*reinterpret_cast<const hv_t<V>*>(knz + k * V), kz);
                unpackv<V>(*reinterpret_cast<const hv_t<V>*>(msk + k * V), mk);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float e = combine(eu[j], ec[j]);
                float xh = xv[j];                                           // the model input replaces x in D only - the
                if constexpr (KNOWN) if (now) xh = blend(xv[j], sigma, im[j], kz[j], mk[j]);   // sampler's own state stays unblended
                if constexpr (STAGED) if (correct) xh = mv[j];
                float d = estimate(e, skip(xh));
                if constexpr (RESCALE) if (owned) d = as_f32(K * d);        // before D's fp16 rounding
                dn[j] = (float)(half_t)d;
                const float bd = as_f32(b * dn[j]);
                float xo = as_f32(__builtin_fmaf(a, xv[j], bd));
                if (!(STAGED && predict)) xo = as_f32(__builtin_fmaf(c, ov[j], xo));
                if constexpr (STAGED) if (correct) xo = as_f32(__builtin_fmaf(sm, mv[j], xo));
                if (nse) xo = as_f32(__builtin_fmaf(s, nz[j], xo));
                xn[j] = (float)(half_t)xo;
                float xm = xn[j];
                if constexpr (KNOWN) if (next) xm = blend(xn[j], sigma_next, im[j], kz[j], mk[j]);
                xi[j] = as_f32(xm * c_in_next);
            }
            *reinterpret_cast<hv_t<V>*>(orow + k * V) = packv<V>(dn);
            *reinterpret_cast<hv_t<V>*>((STAGED && predict ? midr : xr) + k * V) = packv<V>(xn);
            if (dst) {
                const hv_t<V> o = packv<V>(xi);
                *reinterpret_cast<hv_t<V>*>(xi_u + k * V) = o;
                *reinterpret_cast<hv_t<V>*>(xi_c + k * V) = o;
            }
        }
    } else if (dst) {
        rows_join_or_idle<T, V>(mode == DSC_ROW_JOIN, r.c_in_next, xr, orow, xi_u, xi_c, nv);
    }
    if (dst) rows_write_scalars(p.t_buf, p.sigma_groups, n_dst, i, r.t_next, mode == DSC_ROW_IDLE ? 1.0f : r.sigma_next);
}

template <int V>
__global__ __launch_bounds__(256) void step_rows_kernel(const RowArgs p) {
    rows_body<256, V, false, false, false, false>(p, nullptr, nullptr, nullptr);
}
template <int V>
__global__ __launch_bounds__(256) void step_rows_known_kernel(const RowArgs p, const RowKnowns ks) {
    rows_body<256, V, false, true, false, false>(p, &ks, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void linear_rows_kernel(const RowArgs p) {
    rows_body<256, 8, true, false, false, false>(p, nullptr, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void linear_rows_cat_kernel(const RowArgs p, const RowExtras es) {
    rows_body<256, 8, true, false, false, true>(p, nullptr, nullptr, &es);
}
template <int T>
__global__ __launch_bounds__(T) void linear_rows_rescale_kernel(const RowArgs p, const RowRescales ps) {
    rows_body<T, 8, true, false, true, false>(p, nullptr, &ps, nullptr);
}
template <int T>
__global__ __launch_bounds__(T) void linear_rows_rescale_cat_kernel(const RowArgs p, const RowRescales ps, const RowExtras es) {
    rows_body<T, 8, true, false, true, true>(p, nullptr, &ps, &es);
}
__global__ __launch_bounds__(256) void staged_rows_kernel(const RowArgs p, const RowStages ss) {
    rows_body<256, 8, true, false, false, false, true>(p, nullptr, nullptr, nullptr, &ss);
}
template <int T>
__global__ __launch_bounds__(T) void staged_rows_rescale_kernel(const RowArgs p, const RowRescales ps, const RowStages ss) {
    rows_body<T, 8, true, false, true, false, true>(p, nullptr, &ps, nullptr, &ss);
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

// ---- the host side of the per-row entries: one check, one grid rule, one launch
struct RowLaunch { RowArgs a; RowKnowns ks; RowRescales ps; RowExtras es; RowStages ss; bool any_phi; };

// What the six entries check, in the order of their status paragraphs (include/dsc_hip.h); fills the by-value structs.  Records:
// `steps` (the dsc_cfg_dpmpp2m_* entries: chw % 4 == 0, D = x - sigma e written as a dsc_row_linear) or `linears` (chw % 8 == 0).
// need_known / need_rescale / need_extras: the entry has that argument and refuses NULL; rescale is also read where it is merely
// given (dsc_cfg_linear_step_rows_cat's may be NULL).  need_stages (dsc_cfg_staged_step_rows): `stages` is refused when NULL, and a
// STEP slot's stage is read: one of the three, and PREDICT / CORRECT need the 16-byte aligned `mid`.
int rows_check(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf, float* sigma_groups, void* tadd,
               int tadd_halfs, int n_dst, const dsc_row_step* steps, const dsc_row_linear* linears, int n_slots, int chw, int dtype,
               bool need_known, const dsc_row_known* known, bool need_rescale, const float* rescale,
               bool need_extras, const dsc_row_extra* extras, int extra_halfs, RowLaunch* L,
               bool need_stages = false, const dsc_row_stage* stages = nullptr, void* mid = nullptr) {
    if (!x || !old || !x_in || !t_buf || !sigma_groups || !(steps || linears) || (need_known && !known) ||
        (need_rescale && !rescale) || (need_extras && !extras) || (need_stages && !stages) || n_src < 0 || n_dst <= 0 || chw <= 0)
        return DSC_ERR_BAD_ARG;
    if (n_slots < n_dst || n_slots > DSC_ROW_STEP_MAX_SLOTS) return DSC_ERR_BAD_ARG;
    if (extras && (extra_halfs <= 0 || extra_halfs % 8 != 0 || chw % 8 != 0)) return DSC_ERR_BAD_ARG;  // 16-byte rows of chw + extra_halfs
    if (dtype != DSC_F16 || chw % (steps ? 4 : 8) != 0 || !al16(x) || !al16(old) || !al16(x_in) || (eps && !al16(eps)))
        return DSC_ERR_UNSUPPORTED;
    *L = RowLaunch{};
    L->a = RowArgs{static_cast<half_t*>(x), static_cast<const half_t*>(eps), static_cast<half_t*>(old), n_src, static_cast<half_t*>(x_in),
                   t_buf, sigma_groups, static_cast<half_t*>(tadd), tadd_halfs, n_dst, chw, {}};
    L->es.halfs = extra_halfs;
    L->ss.mid = static_cast<half_t*>(mid);
    bool any_row = false;
    for (int i = 0; i < n_slots; ++i) {
        dsc_row_linear r;
        if (steps) {
            const dsc_row_step& q = steps[i];
            r = dsc_row_linear{q.mode, q.sigma, q.guidance, q.a, q.b, q.c, q.c_in_next, q.t_next, q.sigma_next,
                               /* c_skip, c_out, s */ 1.0f, -q.sigma, 0.0f, q.temb_row, /* noise */ nullptr};
        } else {
            r = linears[i];
        }
        const bool step = r.mode == DSC_ROW_STEP;
        if (known && step) {
            if (!eps || i >= n_src) return DSC_ERR_BAD_ARG;                 // (row_record_status' line, ahead of the record's own)
            const dsc_row_known& k = known[i];
            const int set = (k.image != nullptr) + (k.noise != nullptr) + (k.mask != nullptr);
            if (set != 0 && set != 3) return DSC_ERR_BAD_ARG;
            if (set && (!al16(k.image) || !al16(k.noise) || !al16(k.mask))) return DSC_ERR_UNSUPPORTED;
            L->ks.r[i] = k;
        }
        if (const int st = row_record_status(r.mode, i, n_src, n_dst, eps, r.temb_row, &any_row)) return st;
        if (step && r.noise && !al16(r.noise)) return DSC_ERR_UNSUPPORTED;
        if (step && rescale) {
            if (!(rescale[i] >= 0.0f && rescale[i] <= 1.0f)) return DSC_ERR_BAD_ARG;      // (NaN lands here too)
            L->ps.phi[i] = rescale[i];
            L->any_phi |= rescale[i] > 0.0f;
        }
        if (stages && step) {
            const int stage = stages[i].stage;
            if (stage != DSC_ROW_STAGE_FULL && stage != DSC_ROW_STAGE_PREDICT && stage != DSC_ROW_STAGE_CORRECT) return DSC_ERR_BAD_ARG;
            if (stage != DSC_ROW_STAGE_FULL) {
                if (!mid) return DSC_ERR_BAD_ARG;
                if (!al16(mid)) return DSC_ERR_UNSUPPORTED;
            }
            L->ss.r[i] = stages[i];
        }
        if (extras) {
            if (extras[i].extra && !al16(extras[i].extra)) return DSC_ERR_BAD_ARG;
            L->es.r[i] = extras[i];
        }
        L->a.r[i] = r;
    }
    if (any_row) {
        if (!tadd || tadd_halfs <= 0) return DSC_ERR_BAD_ARG;
        if (tadd_halfs % 8 != 0 || !al16(tadd)) return DSC_ERR_UNSUPPORTED;
    }
    return DSC_OK;
}

// workgroups per slot: a row's vectors over T threads, at most 256 (the rest is strided)
unsigned rows_grid(long long vectors, int T) {
    const long long g = (vectors + T - 1) / T;
    return (unsigned)(g < 1 ? 1 : (g > 256 ? 256 : g));
}
template <int T, int V, typename... Parts>
int rows_launch(void (*kernel)(RowArgs, Parts...), const RowArgs& a, int n_slots, void* stream, const Parts&... parts) {
    DSC_LAUNCH(kernel, dim3(rows_grid(a.chw / V, T), (unsigned)n_slots), dim3(T), 0, static_cast<hipStream_t>(stream), a, parts...);
    return hipGetLastError() == hipSuccess ? DSC_OK : DSC_ERR_LAUNCH;
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
    RowLaunch L;
    if (const int st = rows_check(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, rows, nullptr, n_slots, chw,
                                  dtype, false, nullptr, false, nullptr, false, nullptr, 0, &L)) return st;
    return chw % 8 == 0 ? rows_launch<256, 8>(step_rows_kernel<8>, L.a, n_slots, stream)
                        : rows_launch<256, 4>(step_rows_kernel<4>, L.a, n_slots, stream);
}

extern "C" int dsc_cfg_dpmpp2m_step_rows_known(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                               float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                                               const dsc_row_step* rows, const dsc_row_known* known, int n_slots, int chw,
                                               int dtype, void* stream) {
    RowLaunch L;
    if (const int st = rows_check(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, rows, nullptr, n_slots, chw,
                                  dtype, true, known, false, nullptr, false, nullptr, 0, &L)) return st;
    return chw % 8 == 0 ? rows_launch<256, 8>(step_rows_known_kernel<8>, L.a, n_slots, stream, L.ks)
                        : rows_launch<256, 4>(step_rows_known_kernel<4>, L.a, n_slots, stream, L.ks);
}

extern "C" int dsc_cfg_linear_step_rows(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                        float* sigma_groups, void* tadd, int tadd_halfs, int n_dst, const dsc_row_linear* rows,
                                        int n_slots, int chw, int dtype, void* stream) {
    RowLaunch L;
    if (const int st = rows_check(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, nullptr, rows, n_slots, chw,
                                  dtype, false, nullptr, false, nullptr, false, nullptr, 0, &L)) return st;
    return rows_launch<256, 8>(linear_rows_kernel, L.a, n_slots, stream);
}

extern "C" int dsc_cfg_linear_step_rows_rescale(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                                float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                                                const dsc_row_linear* rows, const float* rescale, int n_slots, int chw, int dtype,
                                                void* stream) {
    RowLaunch L;
    if (const int st = rows_check(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, nullptr, rows, n_slots, chw,
                                  dtype, false, nullptr, true, rescale, false, nullptr, 0, &L)) return st;
    return rows_launch<DSC_RESCALE_THREADS, 8>(linear_rows_rescale_kernel<DSC_RESCALE_THREADS>, L.a, n_slots, stream, L.ps);
}

// the grid and the kernel of the entry this one shares its arithmetic with (the extra channels stride over the same grid)
extern "C" int dsc_cfg_linear_step_rows_cat(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                            float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                                            const dsc_row_linear* rows, const float* rescale, const dsc_row_extra* extras,
                                            int extra_halfs, int n_slots, int chw, int dtype, void* stream) {
    RowLaunch L;
    if (const int st = rows_check(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, nullptr, rows, n_slots, chw,
                                  dtype, false, nullptr, false, rescale, true, extras, extra_halfs, &L)) return st;
    return L.any_phi ? rows_launch<DSC_RESCALE_THREADS, 8>(linear_rows_rescale_cat_kernel<DSC_RESCALE_THREADS>, L.a, n_slots, stream, L.ps, L.es)
                     : rows_launch<256, 8>(linear_rows_cat_kernel, L.a, n_slots, stream, L.es);
}

// the kernels of the two linear entries this one shares its arithmetic with, each with the STAGED flag: without a phi > 0 the 256-thread
// grid of dsc_cfg_linear_step_rows, with one the single-workgroup sums of dsc_cfg_linear_step_rows_rescale
extern "C" int dsc_cfg_staged_step_rows(void* x, void* mid, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                        float* sigma_groups, void* tadd, int tadd_halfs, int n_dst, const dsc_row_linear* rows,
                                        const dsc_row_stage* stages, const float* rescale, int n_slots, int chw, int dtype,
                                        void* stream) {
    RowLaunch L;
    if (const int st = rows_check(x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, tadd_halfs, n_dst, nullptr, rows, n_slots, chw,
                                  dtype, false, nullptr, false, rescale, false, nullptr, 0, &L, true, stages, mid)) return st;
    return L.any_phi ? rows_launch<DSC_RESCALE_THREADS, 8>(staged_rows_rescale_kernel<DSC_RESCALE_THREADS>, L.a, n_slots, stream, L.ps, L.ss)
                     : rows_launch<256, 8>(staged_rows_kernel, L.a, n_slots, stream, L.ss);
}
