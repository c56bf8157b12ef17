/*
 * dsc_hip.h - C ABI of libdsc_hip.so: the MI355X (gfx950) hot path of the spatially-controlled denoising
 * step of duongve13112002/DiffusionSpatialControl.
 *
 * Conventions (last row):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says host;
 *   - the caller owns every buffer, including the workspace; nothing is allocated or freed inside;
 *   - every entry is asynchronous on the `stream` it is given (a hipStream_t passed as void*), re-entrant for
 *     distinct streams/workspaces, and safe to capture into a hipGraph (no sync, no malloc, no memcpy);
 *   - the return value is a status: DSC_OK (0) or a negative DSC_ERR_* code; no exception crosses the ABI;
 *   - strides are in ELEMENTS; the innermost (head-dim / channel) stride is always 1;
 *   - a destination with a row / pixel stride (ldo, ldq, ld_probs, o_strides) is written inside [rows] x [row length] only, at any
 *     stride: the ld - row length elements between rows, and everything before the first and behind the last row, are never
 *     touched, whatever tile overhangs the last row; dense destinations (partial sums, statistics, head-major K / V,
 *     channel-major images) are written inside their stated shape only;
 *   - a strided operand (ldx, ldr, ld_scores, add_ld, ...) is read inside [rows] x [row length] only;
 *   - a *_workspace_bytes() answer is exact: the entry touches those bytes of `workspace` and no others, at the alignment it
 *     states; fewer bytes are refused with DSC_ERR_WORKSPACE before any launch (tests/test_guard_bands_gpu.py holds every
 *     entry of the UNet step to these four).
 *
 * Each entry replaces torch-op sequences issued by the reference's Python; the reference has no FFI of its
 * own (it is pure Python), so the "interface each one replaces" is the Python function cited beside it.
 * Paths below are relative to /root/reference/source/.
 */
#ifndef DSC_HIP_H
#define DSC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSC_OK                0
#define DSC_ERR_BAD_ARG      -1   /* null pointer, non-positive size, Bw does not divide Bc*H, ...        */
#define DSC_ERR_UNSUPPORTED  -2   /* head dim / dtype / alignment outside what the kernels are built for */
#define DSC_ERR_WORKSPACE    -3   /* workspace missing or smaller than the *_workspace_bytes() answer    */
#define DSC_ERR_LAUNCH       -4   /* hipLaunchKernel returned an error (hipGetLastError is left set)     */

/* dtype tags */
#define DSC_F16 0
/* flags for dsc_region_xattn_fwd */
#define DSC_FLAG_REF_FP16_ROUNDING 1u  /* round where the reference's fp16 tensors round: scores
                                          (attention_modify.py:90), std (0-dim fp16), the in-place bias add (:97)
                                          and the softmax output (:101) */
#define DSC_FLAG_REUSE_STATS       4u  /* measurement aid: skip the statistics launch and reuse the partial sums the
                                          previous identical call left in `workspace` (times the forward kernel alone) */
#define DSC_FLAG_ROWS_PADDED     256u  /* dsc_region_xattn_fwd_packed only: `region_rows` is [n_rows][100] fp32 (row stride 100
                                          floats = the kernel's LDS table, zeros beyond column S, 16-byte aligned) instead
                                          of [n_rows][S]: the table goes to LDS as a flat 16-byte copy.  S <= 96 only. */
#define DSC_FLAG_BIAS_IS_FINAL     2u  /* `region` already holds the additive bias (a custom weight_func was
                                          evaluated by the caller): add it as is, skip the statistics pass */
#define DSC_FLAG_SIGMA_PER_GROUP 512u  /* dsc_region_xattn_fwd / _fwd_packed: `sigma_dev` points to n_std_groups floats and
                                          batch row b uses sigma_dev[b % n_std_groups] (the row's std group; a continuous
                                          batch of requests at different sigmas).  Needs sigma_dev. */

/* ABI version of this header; bumped on any signature change. */
int dsc_abi_version(void);
/* Static string naming the code-object target the library was built for ("gfx950"). */
const char* dsc_target_arch(void);
/* Diagnostic builds only: a 2-KiB device buffer that receives in-kernel clock stamps of workgroup 0 when a
 * call carries debug flag 32 (tools/mb_xattn.py); NULL (default) disables it.  No output tensor is ever touched. */
void dsc_debug_set_stamp_buffer(void* device_buffer_2KiB);
/* Tuning aid: force a tiling variant of the flash self-attention kernel (0 = automatic choice, 1 = one query tile per
 * wave, 2 = two query tiles per wave where the head dim allows it). */
void dsc_debug_set_self_attn_variant(int variant);
/* Diagnostic: 6 x u64 per-segment cycle sums of workgroup 0 / wave 0 of the flash self-attention kernel (NULL = off). */
void dsc_debug_set_self_attn_stamps(void* device_buffer_64B);
void dsc_debug_set_gemm_stamps(void* device_buffer);   /* 8 x int64 per workgroup of the next gemm_tn_f16 launches (tools/stamps_gemm.py) */
void dsc_debug_set_self_attn_stamp_wave(int wave);    /* which wave of workgroup 0 writes them (default 0) */
/* Human-readable text for a status code. */
const char* dsc_status_string(int status);

/*
 * Region-biased cross-attention forward - replaces modules/attention_modify.py:74-103
 * `scaled_dot_product_attention_regionstate` with weight_func = `w * sigma * qk.std()` (app.py:1004), i.e.
 * rows 2-10 of SURVEY.md 2b, and (with region == NULL) the plain cross-attention SDPA call at :483-485.
 *
 *   out[b,l,h,:] = softmax_s( scale*q[b,l,h,:].k[b,s,h,:] + region[bw(b,h),l,s] * sigma * std_g ) . v[b,s,h,:]
 *
 *   q, out : Bc x L x H x d   addressed as base + b*sb + l*sl + h*sh + i   (q_strides / o_strides = {sb, sl, sh})
 *   k, v   : Bc x S x H x d   addressed as base + b*sb + s*ss + h*sh + i   (k_strides / v_strides = {sb, ss, sh})
 *            so both the processor's [Bc, L, H*d] projection outputs (sl = H*d, sh = d) and a transposed
 *            [Bc, H, L, d] tensor (sh = L*d, sl = d) are consumed in place, and `out` is written directly in the
 *            [Bc, L, H*d] layout `to_out[0]` reads (attention_modify.py:487).
 *   region : fp32 dense [Bw, L, S], Bw divides Bc*H; flattened score row bh = b*H + h takes table row
 *            bh / (Bc*H/Bw)  (torch.repeat_interleave at :96-99).  NULL = no bias (std pass skipped).
 *   std_g  : unbiased (N-1) standard deviation of scale*q.k^T over std group g = b % n_std_groups, all heads,
 *            all L x S scores of the group's rows (:93-95: ONE global std when n_std_groups == 1).
 *   sigma  : `sigma_dev` (device fp32 scalar) if non-NULL, else `sigma_host`.  A device scalar lets a captured
 *            graph be replayed for every step without a host sync (the reference syncs, model_k_diffusion.py:1115).
 *   scale  : <= 0 means 1/sqrt(d)  (attention_modify.py:77; attn.scale is ignored there).
 *
 * Requirements: dtype DSC_F16; d % 8 == 0 and d <= 160; S <= 96; all strides % 8 == 0; pointers 16-byte aligned.
 * Workspace: dsc_region_xattn_workspace_bytes(); contents need no initialisation and carry nothing across calls.
 */
size_t dsc_region_xattn_workspace_bytes(int Bc, int H, int L, int S, int d, int n_std_groups);

int dsc_region_xattn_fwd(const void* q, const void* k, const void* v, void* out,
                         const float* region,
                         int Bc, int H, int L, int S, int d, int Bw, int n_std_groups,
                         const int64_t q_strides[3], const int64_t k_strides[3],
                         const int64_t v_strides[3], const int64_t o_strides[3],
                         float sigma_host, const float* sigma_dev, float scale,
                         int dtype, unsigned flags,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * Statistics only: writes std_out[g] (fp32, n_std_groups values) = the std the call above would use.
 * Exposes `qk.std()` of app.py:1004 so that a caller-supplied weight_func that is not the default one can be
 * evaluated on the host side without materialising the scores more than once.
 */
int dsc_region_xattn_std(const void* q, const void* k,
                         int Bc, int H, int L, int S, int d, int n_std_groups,
                         const int64_t q_strides[3], const int64_t k_strides[3], float scale,
                         int dtype, unsigned flags, float* std_out,
                         void* workspace, size_t workspace_bytes, void* stream);
/*
 * The same with an additive attention mask inside the statistics - reference attention_modify.py:85-95 adds `attn_mask`
 * (float) to the scaled scores BEFORE weight_func sees them, so the std is over scale * q.k^T + mask; likewise
 * `get_attention_scores(attn, query, key, attention_mask)` (:39-70, baddbmm with beta = 1) on the AttnProcessor path
 * (:144,166).  mask: fp32, element (b * H + h, l, s) at mask[bh * mask_strides[0] + l * mask_strides[1] + s]; a stride of 0
 * broadcasts that dimension (an [L, S] mask: strides {0, S}; a [B*H, 1, S] one: {S, 0}).  NULL = dsc_region_xattn_std.
 */
int dsc_region_xattn_std_masked(const void* q, const void* k,
                                int Bc, int H, int L, int S, int d, int n_std_groups,
                                const int64_t q_strides[3], const int64_t k_strides[3], float scale,
                                int dtype, unsigned flags, const float* mask, const int64_t mask_strides[2],
                                float* std_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Prepared-operand path of the region cross-attention (the one the pipeline uses).
 *
 * dsc_xattn_kv_pack: the text keys / values of a cross-attention layer are step-invariant (the reference re-projects
 * them in every layer at every step, attention_modify.py:465-466); they are packed once per generation into the
 * register image the MFMAs consume (zero-padded K fragments, V^T fragments in the chained product's k order).
 * `packed` holds dsc_xattn_kv_pack_bytes() bytes, 16-byte aligned; k / v addressed as in dsc_region_xattn_fwd.
 *
 * dsc_region_xattn_fwd_packed: same result as dsc_region_xattn_fwd, with
 *   packed_kv   : the image written by dsc_xattn_kv_pack for the same (Bc, H, S, d);
 *   region_ids  : uint16 [Bw, L] - index of each table row into region_rows, or NULL for no bias;
 *   region_rows : fp32 [n_rows, S] - the DISTINCT rows of the dense table (n_rows <= 32; the reference's tables have
 *                 at most 2^regions distinct rows, encode_region_map_function.py:49-69).
 * The forward kernel DMAs the image into LDS (global_load_lds) and folds sigma * std into an LDS bias table once per
 * workgroup.  Flags: DSC_FLAG_REF_FP16_ROUNDING, DSC_FLAG_REUSE_STATS.  Workspace as dsc_region_xattn_workspace_bytes().
 * S <= 96: one image per (b, h).  96 < S <= 384 (prompts of several 77-token chunks, encoder_prompt_modify.py:691-812): one
 * image per (b, h, 96-key chunk); the statistics run over all chunks, the forward pass walks them with an online softmax;
 * fp32 scores only (DSC_FLAG_REF_FP16_ROUNDING -> DSC_ERR_UNSUPPORTED).
 */
size_t dsc_xattn_kv_pack_bytes(int Bc, int H, int S, int d);
int dsc_xattn_kv_pack(const void* k, const void* v, void* packed, int Bc, int H, int S, int d,
                      const int64_t k_strides[3], const int64_t v_strides[3], int dtype, void* stream);
int dsc_region_xattn_fwd_packed(const void* q, const void* packed_kv, void* out,
                                const uint16_t* region_ids, const float* region_rows, int n_rows,
                                int Bc, int H, int L, int S, int d, int Bw, int n_std_groups,
                                const int64_t q_strides[3], const int64_t o_strides[3],
                                float sigma_host, const float* sigma_dev, float scale,
                                int dtype, unsigned flags,
                                void* workspace, size_t workspace_bytes, void* stream);

/*
 * Flash self-attention forward - replaces `F.scaled_dot_product_attention(query, key, value)` on the self-attention
 * branch of the processors (modules/attention_modify.py:483-485) and `attn.get_attention_scores` + bmm (:187-188).
 *   out[b,l,h,:] = softmax_s(scale * q[b,l,h,:].k[b,s,h,:]) . v[b,s,h,:]     (no mask, no dropout)
 * Same addressing as dsc_region_xattn_fwd: q/out [Bc, L, H, d] and k/v [Bc, S, H, d] through {sb, sl|ss, sh} element
 * strides, so the three operands can be strided views of ONE fused [Bc, L, 3*H*d] QKV projection.  The L x S scores
 * are never written to memory (online softmax over 64-key tiles).  fp16, d % 8 == 0, d <= 160, strides % 8 == 0.
 * scale <= 0 means 1/sqrt(d).  No workspace.
 */
int dsc_self_attn_fwd(const void* q, const void* k, const void* v, void* out,
                      int Bc, int H, int L, int S, int d,
                      const int64_t q_strides[3], const int64_t k_strides[3],
                      const int64_t v_strides[3], const int64_t o_strides[3],
                      float scale, int dtype, void* stream);

/*
 * Fused sampler step for the k-diffusion DPM++ 2M loop with classifier-free guidance - replaces, per step,
 * `torch.cat([x]*2)` + `input * c_in` (model_k_diffusion.py:1097, external_k_diffusion.py:111),
 * `input + eps * c_out` (:114), the CFG combine (model_k_diffusion.py:1162-1166) and the 3-5 elementwise launches
 * of k_diffusion.sampling.sample_dpmpp_2m (un-vendored), by ONE launch:
 *
 *   D      = x - sigma * (eps_u + guidance * (eps_c - eps_u))          eps = [eps_u(n_img rows); eps_c(n_img rows)]
 *   x      = a * x + b * D + c * old ;   old = D                       (in place; fp32 math, one fp16 rounding each)
 *   x_in   = [x; x] * c_in_next ;  t_buf[0 .. 2 n_img) = t_next ;  sigma_buf[0] = sigma_next
 *
 * x, old: fp16 [n_img, chw]; eps, x_in: fp16 [2 n_img, chw]; t_buf fp32 [2 n_img]; sigma_buf fp32 [1].
 * dsc_prepare_unet_input does only the last line (before the first step).  chw % 4 == 0 (8-byte accesses unless chw % 8 == 0:
 * 4 h w halfs with h w odd, the 19 x 19 latents of a 152 x 152 image), 16-byte aligned pointers.
 */
/* row_src (optional, NULL = none): row_halfs fp16 values copied to each of the row_copies rows of row_dst in the same launch -
 * the pipeline keeps the per-ResNet time-embedding projections of ALL steps in a table computed once per schedule (they depend on
 * the timestep only, reference u_net_condition_modify.py:1040-1060 + diffusers ResnetBlock2D.time_emb_proj) and hands the
 * coming step's row to the static buffer the captured UNet step reads: three launches per step fewer.  row_halfs % 8 == 0. */
int dsc_prepare_unet_input(const void* x, float c_in, float t, float sigma,
                           void* x_in, float* t_buf, float* sigma_buf, int n_img, int chw, int dtype,
                           const void* row_src, void* row_dst, int row_halfs, int row_copies, void* stream);
int dsc_cfg_dpmpp2m_step(void* x, const void* eps, void* old, float sigma, float guidance,
                         float a, float b, float c, float c_in_next, float t_next, float sigma_next,
                         void* x_in, float* t_buf, float* sigma_buf, int n_img, int chw, int dtype,
                         const void* row_src, void* row_dst, int row_halfs, int row_copies, void* stream);
/*
 * Per-request variant of dsc_cfg_dpmpp2m_step for continuous batching: request slot i is latent row i of x / old, rows
 * {i, n_src + i} of eps (the bucket that just ran, [u_0..u_{n_src-1}, c_0..c_{n_src-1}]) and rows {i, n_dst + i} of x_in,
 * t_buf and tadd (the bucket that runs next); sigma_groups[i] is its std group's sigma.  One record per slot, passed BY VALUE
 * in the kernel arguments (at most DSC_ROW_STEP_MAX_SLOTS, 48 bytes each), so the host may reuse its record array at once.
 *   DSC_ROW_STEP: the arithmetic and fp16 rounding points of dsc_cfg_dpmpp2m_step with this slot's scalars (i < n_src);
 *                 the next-step values are those of the coming step (for a request that has just finished: any finite ones)
 *   DSC_ROW_JOIN: x[i] already holds the start latent: x_in rows = x[i] * c_in_next, old[i] = 0 (dsc_prepare_unet_input's line)
 *   DSC_ROW_IDLE: padding: x_in rows = 0, sigma_groups[i] = 1
 * Every slot i < n_dst writes t_next into t_buf rows {i, n_dst + i}, its sigma (sigma_next; 1 for IDLE) into sigma_groups[i]
 * and, when temb_row != NULL, copies temb_row (tadd_halfs fp16) into tadd rows {i, n_dst + i}.  Slots i >= n_dst write no
 * destination row (only STEP or IDLE there).  n_slots >= n_dst records.  chw % 4 == 0 (as above; dsc_cfg_dpmpp2m_step_rows_known
 * too - dsc_cfg_linear_step_rows and its rescale form keep chw % 8 == 0), tadd_halfs % 8 == 0, 16-byte aligned.
 */
#define DSC_ROW_STEP 0
#define DSC_ROW_JOIN 1
#define DSC_ROW_IDLE 2
#define DSC_ROW_STEP_MAX_SLOTS 16
typedef struct {
    int   mode;                                    /* DSC_ROW_STEP, DSC_ROW_JOIN, DSC_ROW_IDLE */
    float sigma, guidance, a, b, c;                /* this step (STEP) */
    float c_in_next, t_next, sigma_next;           /* what the coming UNet step reads */
    const void* temb_row;                          /* fp16 time-embedding row for the coming step, or NULL */
} dsc_row_step;
int dsc_cfg_dpmpp2m_step_rows(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf, float* sigma_groups,
                              void* tadd, int tadd_halfs, int n_dst, const dsc_row_step* rows /* host */, int n_slots,
                              int chw, int dtype, void* stream);
/*
 * dsc_cfg_dpmpp2m_step_rows with a known region per slot: the 4-channel inpainting branch re-imposes the known part of the image
 * on the model input before every model call after a request's first (reference model_k_diffusion.py:1599-1612,
 * `((1 - mask) * (alpha_t * image + sigma_t * noise) + mask * x / rate) * rate`, rate = sqrt(sigma^2 + 1), i.e.
 * alpha_t * rate = 1 and sigma_t * rate = sigma) - five or six eager elementwise launches and a host read of sigma per model
 * call there.  One more record per slot, also passed by value (32 bytes each).  For a DSC_ROW_STEP slot with image != NULL,
 * all fp32, fp16 rounding where marked:
 *   kn(s) = fma(s, noise, image)                                   the known region at noise level s
 *   xh    = blend_now ? fma(mask, x, (1 - mask) * kn(sigma)) : x   the input the model call of this step saw
 *   D     = fp16(fma(-sigma, e, xh))                               e = CFG combine as in dsc_cfg_dpmpp2m_step_rows; old = D
 *   x'    = fp16(fma(c, old, fma(a, x, b * D)))                    x: the sampler's own, unblended state
 *   xh'   = blend_next ? fma(mask, x', (1 - mask) * kn(sigma_next)) : x'
 *   x_in rows {i, n_dst + i} = fp16(xh' * c_in_next)
 * A STEP slot with image == NULL computes dsc_cfg_dpmpp2m_step_rows' bits; JOIN (a request's first model call is not blended)
 * and IDLE slots ignore their record.  image / noise / mask: all three set or all NULL, fp16 [chw], 16-byte aligned.
 */
typedef struct {
    const void* image;      /* fp16 [chw] image latents of this slot, or NULL: slot has no known region */
    const void* noise;      /* fp16 [chw] the request's noise */
    const void* mask;       /* fp16 [chw] 1 = repaint, 0 = keep (already broadcast over the channels) */
    int blend_now;          /* the x of THIS step's model call was blended (request step index >= 1) */
    int blend_next;         /* blend the input of the coming model call */
} dsc_row_known;
int dsc_cfg_dpmpp2m_step_rows_known(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                    float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                                    const dsc_row_step* rows /* host */, const dsc_row_known* known /* host */, int n_slots,
                                    int chw, int dtype, void* stream);
/*
 * dsc_cfg_dpmpp2m_step_rows generalised to the one-model-call-per-step samplers and to v-prediction: per slot, host scalars
 * (modules/sampling.py linear_step_coefficients) select the update of sample_euler (a = sigma'/sigma, b = 1 - a),
 * sample_euler_ancestral (the same to sigma_down, s = s_noise * sigma_up), sample_dpmpp_2m (s = 0), sample_dpmpp_2m_sde
 * (midpoint / heun; s = sigma' sqrt(-expm1(-2 eta h)) s_noise) and sample_lcm (a = 0, b = 1, s = sigma'), and (c_skip, c_out)
 * the parameterisation: eps-prediction c_skip = 1, c_out = -sigma; v-prediction CompVisVDenoiser.get_scalings.  Same launch
 * contract as dsc_cfg_dpmpp2m_step_rows (slot = row, STEP / JOIN / IDLE, separate source and destination buckets, t_buf / tadd /
 * sigma_groups written per slot); one 64-byte record per slot passed by value.  For a DSC_ROW_STEP slot, all fp32, every
 * intermediate rounded to fp32 before the next operation, fp16 rounding where marked:
 *   e  = fma(guidance, m_c - m_u, m_u)                                the model output (eps or v) rows {i, n_src + i}
 *   D  = fp16(fma(c_out, e, c_skip * x))                              old = D
 *   x' = fp16(noise ? fma(s, noise, fma(c, old, fma(a, x, b * D))) : fma(c, old, fma(a, x, b * D)))
 *   x_in rows {i, n_dst + i} = fp16(x' * c_in_next)
 * With c_skip = 1, c_out = -sigma and noise == NULL these are dsc_cfg_dpmpp2m_step_rows' bits.  JOIN / IDLE as there.
 * noise: this step's unit noise row of the slot, fp16 [chw], 16-byte aligned, or NULL (no noise term; s is ignored).
 * The inpainting known-region blend stays with dsc_cfg_dpmpp2m_step_rows_known.
 */
typedef struct {
    int   mode;                                    /* DSC_ROW_STEP, DSC_ROW_JOIN, DSC_ROW_IDLE */
    float sigma, guidance, a, b, c;                /* this step (STEP); sigma is informative: D reads c_skip / c_out */
    float c_in_next, t_next, sigma_next;           /* what the coming UNet step reads */
    float c_skip, c_out, s;                        /* D = c_skip x + c_out e; s scales the noise row */
    const void* temb_row;                          /* fp16 time-embedding row for the coming step, or NULL */
    const void* noise;                             /* fp16 [chw] unit noise of this step, or NULL */
} dsc_row_linear;
int dsc_cfg_linear_step_rows(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf, float* sigma_groups,
                             void* tadd, int tadd_halfs, int n_dst, const dsc_row_linear* rows /* host */, int n_slots,
                             int chw, int dtype, void* stream);
/*
 * dsc_cfg_linear_step_rows with the guidance rescale of arXiv 2305.08891 sec. 3.4 per slot (`guidance_rescale`, phi).  The
 * k-diffusion pipelines of the reference rescale what their model call returns, which is the DENOISED estimate and not eps
 * (reference model_k_diffusion.py:71-82 applied at :781 / :1168 / :1694; modules/model_k_diffusion.py rescale_noise_cfg), and so
 * does this entry.  rescale: one phi per slot on the host, read at the call like the records (0 = off).  For a DSC_ROW_STEP
 * slot with phi > 0, all fp32 with every intermediate rounded to fp32 unless marked:
 *   e   = fma(guidance, m_c - m_u, m_u)      sx = c_skip * x
 *   Dc  = fma(c_out, m_c, sx)                Dg = fma(c_out, e, sx)                 (fp32, not yet rounded to fp16)
 *   the sums of Dc, Dc^2, Dg, Dg^2 over the slot's whole row (n = chw elements) in fp64, in one fixed order
 *   SSD(v) = sum v^2 - (sum v)^2 / n         K = (float)(phi * sqrt(SSD(Dc) / SSD(Dg)) + (1 - phi))     (fp64 until the cast)
 *   D   = fp16(K * Dg)                       old = D
 *   x', x_in rows exactly as dsc_cfg_linear_step_rows from here on (noise row included)
 * (std(Dc) / std(Dg) of the reference: both run over the same n, the unbiased n - 1 cancels.)  SSD(Dg) == 0 - a constant
 * guided estimate - is NOT guarded: K is inf or NaN there, as the reference's division is.  Two launches on the same inputs
 * give the same bits.  A STEP slot with phi == 0 and every JOIN / IDLE slot compute dsc_cfg_linear_step_rows' bits, and t_buf /
 * sigma_groups / tadd are written as there.  Status: what dsc_cfg_linear_step_rows checks; rescale == NULL, or a phi outside
 * [0, 1] (NaN included) in a STEP slot: DSC_ERR_BAD_ARG.  The known-region blend of inpainting is not part of this entry.
 */
int dsc_cfg_linear_step_rows_rescale(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                     float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                                     const dsc_row_linear* rows /* host */, const float* rescale /* host, n_slots */, int n_slots,
                                     int chw, int dtype, void* stream);
/*
 * dsc_cfg_linear_step_rows for a UNet that reads more channels than the latent has: the 9-channel inpainting checkpoints take
 * `[latents | mask | masked-image latents]` (reference model_k_diffusion.py:1617-1619), and the denoiser's c_in scales all nine
 * (external_k_diffusion.py:94-97).  Same launch contract as dsc_cfg_linear_step_rows, with two differences: a row of x_in is
 * chw + extra_halfs halfs long (slot i owns rows {i, n_dst + i} at that stride; x, old, eps and noise rows stay chw), and there
 * is one more record per slot, passed by value (8 bytes each): the slot's step-invariant extra channels.
 *   x_in row [0, chw)                  : exactly what dsc_cfg_linear_step_rows / _rescale write there
 *   x_in row [chw, chw + extra_halfs)  : STEP / JOIN: fp16((float)extra[k] * c_in_next), fp32 with one rounding, the same value in
 *                                        both rows; zeros where extra == NULL.  IDLE: zeros (the whole row is).
 * Slots i >= n_dst write no destination row.  rescale: one phi per slot on the host, or NULL (no slot rescales).  With NULL or
 * every STEP slot's phi == 0 this is ONE launch whose x, old, t_buf, sigma_groups, tadd and x_in[:, :chw] are
 * dsc_cfg_linear_step_rows' bits; with some phi > 0 it is one launch with dsc_cfg_linear_step_rows_rescale's bits and its
 * fixed-order sums.  Plain vector stores, no atomics, nothing crosses workgroups.
 * Status: what dsc_cfg_linear_step_rows checks (and, with rescale != NULL, the phi range of the rescale entry); extras == NULL,
 * extra_halfs <= 0, extra_halfs % 8 != 0, chw % 8 != 0 or a non-NULL extra that is not 16-byte aligned: DSC_ERR_BAD_ARG.  All
 * checks run before the launch: nothing is written on failure.
 */
typedef struct {
    const void* extra;      /* fp16 [extra_halfs] extra input channels of this slot (unscaled), or NULL: zeros */
} dsc_row_extra;
int dsc_cfg_linear_step_rows_cat(void* x, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                                 float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                                 const dsc_row_linear* rows /* host */, const float* rescale /* host, n_slots, or NULL */,
                                 const dsc_row_extra* extras /* host, n_slots */, int extra_halfs, int n_slots,
                                 int chw, int dtype, void* stream);
/*
 * dsc_cfg_linear_step_rows for the samplers that make TWO model calls per step (modules/sampling.py TWO_CALL_FAMILY: sample_heun,
 * sample_dpm_2, sample_dpm_2_ancestral, sample_dpmpp_2s_ancestral, sample_dpmpp_sde; host scalars: call_plan).  Their step is two
 * consecutive transitions of the per-row step: the first leaves x alone and writes the intermediate point the second model call
 * runs on, the second reads that point back as a third state row.  Same launch contract as dsc_cfg_linear_step_rows, with one more
 * state buffer - mid: fp16 [slots, chw], 16-byte aligned, the row stride of x - and one more record per slot, passed by value
 * (8 bytes each; with the 64-byte dsc_row_linear and the phi that is 16 x (64 + 8 + 4) bytes plus the buffers, far below the 4 KB
 * of kernel arguments).  For a DSC_ROW_STEP slot, all fp32, every intermediate rounded to fp32 before the next operation, fp16
 * rounding where marked; [K]: the rescale factor of a slot with phi > 0, as in dsc_cfg_linear_step_rows_rescale:
 *   e = fma(guidance, m_c - m_u, m_u)
 *   DSC_ROW_STAGE_FULL:    exactly dsc_cfg_linear_step_rows (with phi > 0: _rescale); mid is neither read nor written
 *   DSC_ROW_STAGE_PREDICT: D  = fp16([K] fma(c_out, e, c_skip * x))                        old = D
 *                          xm = fp16(noise ? fma(s, noise, fma(a, x, b * D)) : fma(a, x, b * D))
 *                          mid = xm; x is NOT written; x_in rows {i, n_dst + i} = fp16(xm * c_in_next)
 *   DSC_ROW_STAGE_CORRECT: xm = mid; D = fp16([K] fma(c_out, e, c_skip * xm))   (the model saw xm: D and the rescale's sums read
 *                          mid, not x)
 *                          t3 = fma(m, xm, fma(c, old, fma(a, x, b * D)));  x' = fp16(noise ? fma(s, noise, t3) : t3)
 *                          x = x'; old = D; x_in rows {i, n_dst + i} = fp16(x' * c_in_next)
 * JOIN / IDLE slots, t_buf, sigma_groups, tadd and slots i >= n_dst are dsc_cfg_linear_step_rows'.  rescale: NULL or one phi per
 * slot, dsc_cfg_linear_step_rows_cat's meaning: with some phi > 0 the launch has the rescale entry's single-workgroup fixed-order
 * fp64 sums (over mid in CORRECT), so a linear-family slot with a rescale and a two-call slot share one launch.  No KNOWN and no
 * CAT form.  Plain vector stores, no atomics, nothing crosses workgroups.
 * Status: what dsc_cfg_linear_step_rows checks (chw % 8 != 0: DSC_ERR_UNSUPPORTED) and the phi range; stages == NULL, a STEP slot
 * whose stage is none of the three, or mid == NULL while a STEP slot is PREDICT / CORRECT: DSC_ERR_BAD_ARG; a misaligned mid there:
 * DSC_ERR_UNSUPPORTED.  All checks run before the launch: nothing is written on failure.
 */
#define DSC_ROW_STAGE_FULL 0
#define DSC_ROW_STAGE_PREDICT 1
#define DSC_ROW_STAGE_CORRECT 2
typedef struct {
    int   stage;            /* DSC_ROW_STAGE_FULL, _PREDICT, _CORRECT (read for STEP slots) */
    float m;                /* CORRECT: the weight of mid in x' */
} dsc_row_stage;
int dsc_cfg_staged_step_rows(void* x, void* mid, const void* eps, void* old, int n_src, void* x_in, float* t_buf,
                             float* sigma_groups, void* tadd, int tadd_halfs, int n_dst,
                             const dsc_row_linear* rows /* host */, const dsc_row_stage* stages /* host, n_slots */,
                             const float* rescale /* host, n_slots, or NULL */, int n_slots, int chw, int dtype, void* stream);
/* out = a*x + b*denoised + c*old  (old may be NULL when c == 0): the sampler update alone, for callers that keep
 * the reference's `sampler(model_fn, x, sigmas=...)` control flow.  n elements, n % 4 == 0 (8-byte accesses unless n % 8 == 0). */
int dsc_dpmpp2m_update(const void* x, const void* denoised, const void* old, float a, float b, float c,
                       void* out, int64_t n, int dtype, void* stream);

/*
 * GroupNorm (+ optional SiLU) over NCHW fp16 - replaces `GroupNorm(32, eps)` -> `SiLU` pairs of the UNet
 * (u_net_condition_modify.py:465-470,1304-1306 and diffusers ResnetBlock2D / Transformer2DModel norms; SURVEY.md 2b
 * row 12).  y[b,c,:,:] = act((x - mean_bg) * rstd_bg * gamma[c] + beta[c]), statistics in fp32/fp64 over the
 * (C/groups) * hw elements of group g of row b (biased variance, as torch).  Two launches (partial sums, apply);
 * workspace from dsc_groupnorm_workspace_bytes() (8-byte aligned; exactly those bytes are touched), no initialisation needed.
 * gamma/beta fp16 [C].
 * Requirements: C % groups == 0, 16-byte aligned x / y (hw % 8 != 0 takes a scalar-load path).
 */
size_t dsc_groupnorm_workspace_bytes(int B, int C, int hw, int groups);
int dsc_groupnorm_silu(const void* x, void* y, const void* gamma, const void* beta,
                       int B, int C, int hw, int groups, float eps, int apply_silu, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * GroupNorm (+ optional SiLU) over channels-last (NHWC) fp16 - the layout the UNet keeps its activations in so that
 * MIOpen's NHWC implicit-GEMM convolutions and the transformer's token-major GEMMs need no transposes.
 *   x, y  : [B, hw, C] (= a channels_last [B, C, h, w] tensor), C % 8 == 0, C/8 <= 512
 *   add   : optional fp16 [B, C] added to x before the statistics and the normalisation - fuses the ResNet block's
 *           `hidden + time_emb_proj(silu(temb))[:, :, None, None]` (diffusers ResnetBlock2D) into the norm that follows
 *   y[b,p,c] = act(((x[b,p,c] + add[b,c]) - mean_bg) * rstd_bg * gamma[c] + beta[c])
 * Every access is a coalesced 16-byte vector; two launches (per-chunk partial sums, apply); bit-reproducible.
 * Workspace: dsc_groupnorm_nhwc_workspace_bytes(), 8-byte aligned, no initialisation needed.  It is sized by the apply pass's row
 * chunks; the statistics pass writes at most as many chunk rows (fewer in the slab form), the apply pass reads only what was written,
 * and nothing outside the returned bytes is touched in any launch form of dsc_debug_set_gn_mode.  y is written inside [B, hw, C] only.
 */
size_t dsc_groupnorm_nhwc_workspace_bytes(int B, int C, int hw, int groups);
/* diagnostics: 0 = choose the kernel from the shape, 2 = never a single-launch kernel (statistics + apply), 3 = also allow the
 * 1024-thread single-launch kernel (measured slower; kept for tools/mb_gn.py), 4 = 2 in the old three-launch form (fine row
 * chunks, separate finalize launch); 10 / 11 = statistics workgroups without / with channel slabs (default 11) */
void dsc_debug_set_gn_mode(int mode);
int dsc_groupnorm_silu_nhwc(const void* x, void* y, const void* gamma, const void* beta,
                            const void* add, int64_t add_row_stride,   /* elements between rows of `add` (>= C) */
                            int B, int C, int hw, int groups, float eps, int apply_silu, int dtype,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The same over the channel concatenation [x1 | x2] that the caller never materialised - the up blocks'
 * `torch.cat([hidden_states, res_hidden_states], dim=1)` in front of every ResNet block (diffusers UpBlock2D /
 * CrossAttnUpBlock2D, reached from reference u_net_condition_modify.py:1274-1302): x1 [B, hw, C1], x2 [B, hw, C - C1],
 * C1 % 8 == 0.  The pass that reads the two sources for the statistics also writes the concatenation to `cat`
 * [B, hw, C] (the block's 1x1 shortcut reads it), so the separate concatenation kernel and one read of the tensor go away.
 * y as above.  cat must not alias x1, x2 or y.  Same workspace as dsc_groupnorm_silu_nhwc for (B, C, hw, groups). */
int dsc_groupnorm_silu_nhwc_cat(const void* x1, const void* x2, int C1, void* cat, void* y, const void* gamma,
                                const void* beta, const void* add, int64_t add_row_stride, int B, int C, int hw,
                                int groups, float eps, int apply_silu, int dtype, void* workspace, size_t workspace_bytes,
                                void* stream);

/* out[r, c] = a[r, c] + b[r, c] + bias[c] over fp16 [rows, C] (channels-last residual add with the convolution's
 * bias folded in: the ResNet block's `x + conv2(h)` where conv2 ran without its bias).  bias may be NULL. C % 8 == 0. */
int dsc_add_bias_residual(const void* a, const void* b, const void* bias, void* out, int64_t rows, int C,
                          int dtype, void* stream);

/*
 * Token-major fp16 linear with fused epilogues - replaces `F.linear` (+ the separate residual add / GEGLU kernels) for
 * the UNet's `to_q/to_k/to_v/to_out`, feed-forward and 1x1 projection layers (diffusers BasicTransformerBlock /
 * Transformer2DModel / ResnetBlock2D shortcut):
 *   geglu == 0:  out[m, n] = sum_k x[m,k] w[n,k] (+ bias[n]) (+ residual[m,n]),            out is [M, N]
 *   geglu == 1:  out[m, j] = (acc[m,j] + bias[j]) * gelu(acc[m,N/2+j] + bias[N/2+j]),      out is [M, N/2]
 * x [M, K] with row stride ldx, w [N, K] contiguous (torch Linear layout), residual / out with row strides ldr / ldo.
 * Requirements: fp16, K % 64 == 0, N % 64 == 0, strides % 8 == 0, 16-byte aligned pointers; geglu needs bias, no residual.
 * A residual of FEWER rows than M - the residual stream of layers that ran once per image in front of the first cross-attention,
 * added to a result that has a row per classifier-free-guidance branch (the reference repeats nothing there: its batch is
 * already doubled) - is passed as  ldr = row stride | (R << 32)  with R = its row count: row m adds residual row m % R.
 * R % 128 == 0, M % R == 0; same encoding in dsc_linear_ln_f16 and dsc_linear_gn_f16.  High bits 0: a residual of M rows.
 * Rows >= M of the last row tile (and the workgroups that pad an XCD-ordered grid) load clamped rows and store nothing: out is
 * written inside [M] x [N] (GEGLU: [M] x [N/2]) at any ldo >= the row length, x and the residual are read inside [M] x [K] and
 * [M or R] x [N] at any ldx / ldr.
 */
int dsc_linear_f16(const void* x, const void* w, const void* bias, const void* residual, void* out,
                   int64_t M, int N, int K, int64_t ldx, int64_t ldr, int64_t ldo, int geglu, int dtype, void* stream);

/*
 * 3x3 / stride 1 / pad 1 convolution over channels-last fp16 - replaces `F.conv2d` (MIOpen) for the ResnetBlock2D
 * conv1/conv2 and the Upsample2D conv of the UNet that reference source/modules/u_net_condition_modify.py assembles
 * from diffusers blocks:
 *   out[b,y,x,n] = sum_{dy,dx,c} x[b,y+dy-1,x+dx-1,c] * w[n,dy,dx,c]  (+ bias[n]) (+ residual[b,y,x,n]),  zero padding
 * x [B,H,W,Cin] with pixel stride ldx, w [Cout,3,3,Cin] contiguous (a torch conv weight in channels_last memory
 * format), residual / out [B,H,W,Cout] with pixel strides ldr / ldo.  fp32 accumulation, one fp16 rounding.
 * resample == DSC_CONV_UPSAMPLE2X: x is [B,H/2,W/2,Cin] and the convolution reads it through a nearest-neighbour 2x
 * upsampling (diffusers Upsample2D = F.interpolate(scale_factor=2, mode="nearest") + conv) without materialising the image.
 * resample == DSC_CONV_UPSAMPLE_CEIL: x is [B,(H+1)/2,(W+1)/2,Cin] and is read through F.interpolate(x, size=(H, W),
 * mode="nearest") - the upsampling to the size of the skip tensor the result is concatenated with (the reference UNet's
 * `upsample_size`, u_net_condition_modify.py:1114-1123, 1281-1300), which lets latents whose sides are not multiples of 8 through
 * the UNet.  Each side is 2s or 2s-1 of its source side s, and for both torch's source index is dst >> 1: exactly,
 * floor(dst * s / (2s-1)) = floor(dst/2 + dst / (2 (2s-1))) and the second term is below 1/2 for dst <= 2s-2; torch computes the
 * index in fp32, and tests/test_any_size_host.py compares it with the shift for every s in 1..1099.  So the gather is the 2x
 * one with another source extent, and for even H, W the result has the bytes of DSC_CONV_UPSAMPLE2X.
 * resample == DSC_CONV_STRIDE2: only the even pixels are stored, out is [B,(H+1)/2,(W+1)/2,Cout] - the stride-2 / pad-1 convolution
 * of diffusers Downsample2D (3 per UNet step), odd sides included (their last pixel is an even one).  The taps still run at H x W (4x the necessary MFMA work); it is nevertheless
 * faster than MIOpen's stride-2 kernels here (24-27 us vs 31-37 us) and, unlike their atomic split-K, bit-reproducible.
 * out_nchw != 0: out is [B,Cout,H,W] (channel-major; the UNet's 4-channel conv_out hands its result back in the sampler's
 * layout); such a launch is never split, whatever `splits` says (the split's reduce launch stores pixel-major).  Cout need not be a multiple of 64: a ragged last channel tile reads zero weight rows through the buffer bounds.
 * splits: number of input-channel ranges accumulated by separate workgroups (0 = chosen from the shape); splits > 1
 * needs `workspace` (dsc_conv3x3_workspace_bytes) and sums the partials in range order: bit-reproducible.
 * Supported (dsc_conv3x3_supported): Cin % 64 == 0, strides % 8 == 0 (when Cout % 8 == 0), 16-byte aligned pointers; any
 * H, W >= 1 (sides that are not multiples of the 8 x 16 / 8 x 8 pixel tile - 12 x 12, the lowest level of a 768 x 768 generation -
 * cost the overhang's MFMAs, nothing else); anything else returns DSC_ERR_UNSUPPORTED and the caller keeps the library convolution.
 * Overhanging pixels and the channel padding of a ragged last tile are never stored: out is written inside [stored pixels] x [Cout]
 * at any ldo >= Cout (channel-major: inside [B, Cout, H W]), x and the residual are read inside [pixels] x [Cin] / [Cout] at any ldx /
 * ldr.  Cout % 8 != 0 takes any ldo / ldr >= Cout (the rows are then 8-byte aligned at best, as with ldo = Cout).
 * dsc_conv3x3_workspace_bytes() takes no resample code: it sizes the partial sums by the H x W pixels the taps run over, which covers
 * the fewer pixels a stride-2 launch stores; a launch touches at most those bytes, and its reduce pass reads only what the split pass wrote.
 */
/* the resample codes (0: none of them); ops.py mirrors them as CONV_*, tests/test_conv_dispatch_host.py compares the two */
#define DSC_CONV_UPSAMPLE2X 1
#define DSC_CONV_STRIDE2 2
#define DSC_CONV_STRIDE2_PAD_BR 3   /* stride 2 with zero padding on the bottom / right only (F.pad (0,1,0,1) + stride-2 conv of
                                     * the AutoencoderKL encoder's Downsample2D): the ODD pixels of the stride-1 / pad-1 taps;
                                     * even H, W only (image sides are multiples of 8) */
#define DSC_CONV_UPSAMPLE_CEIL 4
int dsc_conv3x3_supported(int B, int H, int W, int Cin, int Cout);
/* diagnostics: 8 x int64 per workgroup (start / loop start / loop end / end in 100 MHz ticks, the three segment lengths in
 * shader clocks, XCC and HW ids) of every following dsc_conv3x3_nhwc_f16 call go to `device_buffer`; NULL switches it off */
void dsc_debug_set_conv_stamps(void* device_buffer);
/* diagnostics: 3 / 9 = force the weight-tile ring depth, 0 = by grid size and tuning profile; 200 + n = the split-count
 * model's per-step time for grids of <= 256 workgroups (n / 100 us); 300 / 301 = pixel tiles / channel blocks fastest
 * within an XCD (default: by shape); 400 / 401 / 402 = the nine-stage kernels without DMA-only loader waves / by rule / always;
 * 500 + n = the same per-step time for dsc_conv3x3_up2x_nhwc_f16's grids of <= 256 workgroups (n / 100 us) */
void dsc_debug_set_conv_ring(int stages);
size_t dsc_conv3x3_workspace_bytes(int B, int H, int W, int Cin, int Cout, int splits);
int dsc_conv3x3_nhwc_f16(const void* x, const void* w, const void* bias, const void* residual, void* out,
                         int B, int H, int W, int Cin, int Cout, int64_t ldx, int64_t ldr, int64_t ldo,
                         int resample, int out_nchw, int splits, int dtype, void* workspace, size_t workspace_bytes,
                         void* stream);

/*
 * The same Upsample2D pair - `F.interpolate(x, scale_factor=2.0, mode="nearest")` followed by the 3x3 / pad-1 `conv`
 * (diffusers Upsample2D.forward, reached from reference u_net_condition_modify.py:1281-1300 with no `upsample_size`) - as FOUR
 * 2x2 convolutions of the SOURCE image, one per output phase: a nearest-neighbour doubling hands the same source pixel to up to
 * three taps per axis, so
 *   out[b, 2i+py, 2j+px, n] = sum_{a,b in {0,1}} sum_c K[2py+px][n][2a+b][c] * x[b, i+py+a-1, j+px+b-1, c]  (+ bias[n]),  x = 0 outside
 *   K[2py+px][n][2a+b][c]   = sum_{dy in R(py,a)} sum_{dx in R(px,b)} w[n][dy][dx][c],   R(0,0)={0} R(0,1)={1,2} R(1,0)={0,1} R(1,1)={2}
 * - 4 taps per 64-channel slice instead of 9.  For the exact 2x target the zero padding of the doubled image and of the source
 * coincide; the skip-sized targets 2s-1 of DSC_CONV_UPSAMPLE_CEIL do NOT (their last row / column has a tap on padding whose twin
 * is inside) and stay with dsc_conv3x3_nhwc_f16.
 * dsc_conv3x3_up2x_pack_f16: w [Cout,3,3,Cin] -> packed [4,Cout,4,Cin] fp16; the 1, 2 or 4 weights are added in fp32, dy ascending
 * then dx ascending, and rounded ONCE - so results differ from dsc_conv3x3_nhwc_f16(DSC_CONV_UPSAMPLE2X) by that rounding of the
 * weights.  Depends on the weight only: pack once per weight, not per call.  Cin % 64 == 0.
 * dsc_conv3x3_up2x_nhwc_f16: x [B,h,w,Cin] with pixel stride ldx, out [B,2h,2w,Cout] with pixel stride ldo; Cin % 64 == 0,
 * Cout % 64 == 0, strides % 8 == 0, 16-byte aligned pointers, any h, w >= 1 (dsc_conv3x3_up2x_supported).  splits / workspace
 * as for dsc_conv3x3_nhwc_f16 (dsc_conv3x3_up2x_workspace_bytes; the partial sums are indexed by output pixel).  The tuning
 * profile and dsc_debug_set_conv_ring's ring / loader settings select nothing here: one kernel per tile width, equal bytes.
 */
int dsc_conv3x3_up2x_pack_f16(const void* w, void* packed, int Cin, int Cout, void* stream);
int dsc_conv3x3_up2x_supported(int B, int h, int w, int Cin, int Cout);
size_t dsc_conv3x3_up2x_workspace_bytes(int B, int h, int w, int Cin, int Cout, int splits);
int dsc_conv3x3_up2x_nhwc_f16(const void* x, const void* w_packed, const void* bias, void* out, int B, int h, int w,
                              int Cin, int Cout, int splits, void* workspace, size_t workspace_bytes, int64_t ldx,
                              int64_t ldo, int dtype, void* stream);

/*
 * dsc_linear_f16 with a LayerNorm folded in on either side - removes the `nn.LayerNorm` launches of diffusers'
 * BasicTransformerBlock (norm1/norm2/norm3) between the token-major GEMMs of a block:
 *   ln_out != NULL  (producer): also writes, per output row and 64-column block, the (sum, sum of squares) of the fp16
 *                   output row segment to ln_out[M][N/64][2] (fp32) - the statistics of the residual stream s = out.
 *   ln_in  != NULL  (consumer): x is the UN-normalised s [M, K = C], w = W diag(gamma) (fp16), bias = beta.W^T + b,
 *                   ln_cvec[n] = sum_k w[n,k] (fp32); per row mu, rstd come from ln_in[M][ln_nb][2] (summed in block order) and
 *                   out[m,n] = rstd_m (acc[m,n] - mu_m cvec[n]) + bias[n]      ( = LayerNorm(s)[m,:] . W[n,:] + b[n] )
 * geglu may be combined with ln_in, not with ln_out.  Same shape limits as dsc_linear_f16.
 */
int dsc_linear_ln_f16(const void* x, const void* w, const void* bias, const void* residual, void* out,
                      int64_t M, int N, int K, int64_t ldx, int64_t ldr, int64_t ldo, int geglu,
                      const float* ln_in, int ln_nb, const float* ln_cvec, float ln_eps, float* ln_out,
                      int dtype, void* stream);
/*
 * The self-attention branch's fused q / k / v projection (reference attention_modify.py:458-474: `attn.to_q / to_k / to_v` on
 * the same hidden states, then `.view(batch, -1, heads, head_dim).transpose(1, 2)`) as ONE GEMM over w = [Wq; Wk; Wv]
 * ([3C, K]) whose epilogue already performs the head split for K and V: columns [0, C) -> q_out [M, C] (row stride ldq),
 * columns [C, 3C) -> kv_out [2][M / seq_len][heads][seq_len][C / heads] (fp16, 16-byte aligned) - each head's keys / values
 * contiguous, the layout dsc_self_attn_fwd's 64-key LDS-DMA tiles want (contiguous 1-KiB pieces instead of C/heads-element
 * row segments 3C elements apart).  Same LayerNorm-folding arguments as dsc_linear_ln_f16 (ln_in NULL = plain GEMM).
 * Needs C % 64 == 0, (C / heads) % 8 == 0, K % 64 == 0, M % seq_len == 0.
 */
/* diagnostics: launch variant of dsc_linear_f16 / _ln_f16 / _qkv_f16, one decimal field each (0 = the measured rule):
 *   v % 10            K-tile ring depth (2 or 3 stages)
 *   v / 10 % 1000     tile height (64 or 128 token rows)                          e.g. 643 = 64-row tiles, 3 stages
 *   v / 10000 % 10    DMA-only loader waves: 4 = for every tile, 9 = never
 *   v / 100000 % 10   128-column tiles: 1 = never, 2 = wherever N is a multiple of 128
 *   v / 1000000 % 10  workgroup order: 1 = plain blockIdx, 2 = XCD-aware for every shape
 *   v / 10000000 % 10 1 = non-temporal stores of the GEGLU output (measured: no effect)
 *   v < 0             -v = the grid (workgroups) a plain GEMM must keep to take 128-column tiles (default 512: the throughput
 *                     tier - 8 images per generation, coalesced requests; no batch-1 launch qualifies)
 * Every variant gives equal bytes (tests/test_unet_pipeline_gpu.py::test_linear_kernel_tilings_agree_bit_for_bit). */
void dsc_debug_set_gemm_stages(int stages);
int dsc_linear_qkv_f16(const void* x, const void* w, const void* bias, void* q_out, void* kv_out,
                       int64_t M, int C, int K, int64_t ldx, int64_t ldq, int heads, int seq_len,
                       const float* ln_in, int ln_nb, const float* ln_cvec, float ln_eps, int dtype, void* stream);

/*
 * 3x3 / pad 1 convolution with few input channels (<= 16) - the UNet's `conv_in` (4 -> 320; reference
 * u_net_condition_modify.py:352-356,1187): x [B,Cin,H,W] channel-major fp16 (the sampler's latent layout),
 * w_t [9*Cin, Cout] = weight.reshape(Cout, Cin*9).t() (k = (ci*3 + dy)*3 + dx), out [B,H,W,Cout] channels-last, bias fused.
 * Cout % 8 == 0, Cout <= 512; any H, W >= 1 (a workgroup computes 8 pixels of a row; the last one of a ragged row stores fewer).
 */
int dsc_conv3x3_fewcin_f16(const void* x_nchw, const void* w_t, const void* bias, void* out_nhwc,
                           int B, int Cin, int H, int W, int Cout, int dtype, void* stream);

/*
 * out = x . w^T (+ bias) (+ residual) as ONE hipBLASLt launch (bias epilogue + beta = 1 with C = residual) - the plain
 * library GEMM for the token-major linears dsc_linear_f16 does not cover (few rows, long K); replaces `F.linear` + the
 * separate residual add of diffusers' FeedForward / Transformer2DModel.proj_out / ResnetBlock2D.conv_shortcut.
 * Same operand conventions as dsc_linear_f16; K, N and the strides multiples of 8.  The first call for a shape queries
 * the heuristic (and creates the handle / a 32 MiB workspace): run it once outside a graph capture.
 */
int dsc_linear_lt_f16(const void* x, const void* w, const void* bias, const void* residual, void* out,
                      int64_t M, int N, int K, int64_t ldx, int64_t ldr, int64_t ldo, int dtype, void* stream);
/* 1 when this build of the library contains the hipBLASLt path above (built with DSC_WITH_HIPBLASLT=1), 0 for the default
 * build, which neither contains nor links hipBLASLt: dsc_linear_lt_f16 then returns DSC_ERR_UNSUPPORTED for every shape and
 * the caller's own GEMM (dsc_linear_f16 / dsc_linear_splitk_f16) runs it - what the pipeline does by default since round 3. */
int dsc_has_library_gemm(void);
/* Generation slot of the calling host thread (0..3, default 0): which of the library-GEMM workspaces dsc_linear_lt_f16 hands
 * to hipBLASLt (its stream-K kernels keep partial tiles there).  A pipeline that keeps two generations in flight on two
 * streams drives each from its own thread / slot, so that neither the eager GEMMs nor the ones baked into the two captured
 * step graphs share a workspace.  Thread-local; returns DSC_ERR_BAD_ARG outside 0..3. */
int dsc_set_workspace_slot(int slot);
/*
 * Tuning profile of the launch rules, process-wide, read when a kernel is LAUNCHED (so a captured graph keeps the profile it
 * was captured under):
 *   DSC_TUNE_LATENCY     one generation at a time owns the chip (default): kernels may take a whole CU each - the 3x3
 *                        convolution's nine-stage weight ring for grids of <= 256 workgroups (all of a CU's LDS), the GEMM's
 *                        four extra DMA-only loader waves for its 64-row tiles.  +1.5 % images/s one at a time.
 *   DSC_TUNE_THROUGHPUT  several generations share the chip on their own streams: the three-stage ring / four-wave forms,
 *                        which leave room for the other stream's workgroups on the same CU.  +3 % images/s with two generations
 *                        in flight against the latency rules (7 interleaved runs each on one box: 10.81 vs 10.46).
 * This library's OWN kernels give equal bytes under the two (tests/...::test_conv3x3_and_gemm_profiles_give_equal_bytes); a GEMM
 * that is left to hipBLASLt (dsc_linear_lt_f16) may run another library algorithm under DSC_TUNE_THROUGHPUT, and two library
 * algorithms need not add in the same order: those results agree to rounding, not to the bit.
 * Returns DSC_ERR_BAD_ARG for any other value.
 */
#define DSC_TUNE_LATENCY 0
#define DSC_TUNE_THROUGHPUT 1
int dsc_set_tuning_profile(int profile);
int dsc_get_tuning_profile(void);
/* Diagnostic: out[0] = shapes planned so far, out[1] = library candidate algorithms the heuristic offered, out[2] = how
 * many of those need a workspace (stream-K / split-K kernels whose workgroups wait on each other's partial tiles) and were
 * therefore NOT eligible: dsc_linear_lt_f16 only ever runs workspace-free algorithms, which finish under any residency. */
void dsc_linear_lt_stats(long long out[3]);

/*
 * Few-row linear (M <= 8) for the time-embedding path: y[m,n] = act(sum_k x[m,k] w[n,k] + bias[n]) - `Timesteps` +
 * `TimestepEmbedding.linear_1/linear_2` (reference u_net_condition_modify.py:554-560, 1040-1060) and the per-ResNet
 * `time_emb_proj(silu(temb))` projections.  x [M,K] fp16 (row stride ldx) or, with DSC_ROWS_SINUSOID_IN, fp32 t[M] from which
 * the sinusoidal embedding [cos | sin] of width K is generated on the fly; DSC_ROWS_SILU_OUT applies SiLU to the result.
 */
#define DSC_ROWS_SINUSOID_IN 1
#define DSC_ROWS_SILU_OUT 2
int dsc_linear_rows_f16(const void* x, const void* w, const void* bias, void* out, int M, int N, int K,
                        int64_t ldx, int64_t ldo, int flags, int dtype, void* stream);

/*
 * (residual add +) LayerNorm over the last dimension - replaces the `x = attn(...) + x` elementwise add and the
 * `nn.LayerNorm` that follows it in diffusers' BasicTransformerBlock (norm1/norm2/norm3, eps 1e-5):
 *   s[r, :]  = x[r, :] + a[r, :]            (a == NULL: s = x)         -> written to `sum_out` when non-NULL (fp16)
 *   y[r, :]  = (s - mean_r) * rstd_r * gamma + beta                     statistics in fp32 on the fp16-rounded s
 * rows x C fp16, contiguous rows; C % 8 == 0, C <= 4096.  One wave per row, 16-byte accesses, one launch.
 */
int dsc_add_layernorm(const void* x, const void* a, const void* gamma, const void* beta, void* sum_out, void* y,
                      int64_t rows, int C, float eps, int dtype, void* stream);

/* GEGLU of the transformer feed-forward (diffusers GEGLU): y[r, j] = x[r, j] * gelu(x[r, n + j]), exact erf gelu.
 * x fp16 [rows, 2n] contiguous, y fp16 [rows, n]; n % 8 == 0. */
int dsc_geglu(const void* x, void* y, int64_t rows, int n, int dtype, void* stream);

/*
 * GroupNorm statistics from the PRODUCER's epilogue - the GroupNorms of the UNet's ResNet / transformer blocks
 * (modules/u_net_condition_modify.py:465-470,1304-1306 and the diffusers blocks it builds) at the 64x64 / 32x32 levels were a
 * statistics launch + an apply launch each, and the statistics launch re-read a tensor that the convolution / GEMM in front of it
 * had just written.  These entries let that producer emit the statistics:
 *   dsc_conv3x3_gn_nhwc_f16  = dsc_conv3x3_nhwc_f16 (no split, channels-last output) + `add`: an optional per-IMAGE bias row
 *                              add[b][c] (fp16, row stride add_ld: the ResNet block's time-embedding projection, which
 *                              diffusers adds between conv1 and norm2) + the partial sums of the fp16 tensor it stores;
 *   dsc_linear_gn_f16        = dsc_linear_f16 (bias / residual epilogue) whose rows are the pixels of images of
 *                              `rows_per_image` rows + the same partial sums (1x1 convolutions: proj_out, conv_shortcut);
 *   dsc_groupnorm_apply_nhwc = the whole GroupNorm (+ SiLU) in ONE launch given those partial sums.
 * gn_part is fp32 [B][rows][groups][2][2] with rows = dsc_*_gn_rows(...) pixel tiles per image (0 = shape not covered: 16-wide
 * convolution tiles without split-K, Cout % 64 == 0, groups of <= 64 channels, <= 128 tiles per image); slot [g][1] holds the
 * part of a group that lies beyond a 64-channel tile boundary.  Fixed summation orders: bit-reproducible.  No workgroup waits
 * for another - the partial sums cross the kernel boundary.  Nothing outside that shape is written; every slot the consumer reads
 * is ([g][0] of every group, [g][1] of the groups that cross a boundary), a [g][1] no group needs is left as it was.  A shape
 * dsc_*_gn_rows() answers 0 for is refused with DSC_ERR_UNSUPPORTED before any launch.
 */
int dsc_conv3x3_gn_rows(int B, int H, int W, int Cin, int Cout, int groups, int resample);
int dsc_conv3x3_gn_nhwc_f16(const void* x, const void* w, const void* bias, const void* add, int64_t add_ld,
                            const void* residual, void* out, int B, int H, int W, int Cin, int Cout, int64_t ldx,
                            int64_t ldr, int64_t ldo, int resample, float* gn_part, int groups, int dtype, void* stream);
int dsc_linear_gn_rows(int64_t M, int N, int K, int rows_per_image, int groups);
int dsc_linear_gn_f16(const void* x, const void* w, const void* bias, const void* residual, void* out,
                      int64_t M, int N, int K, int64_t ldx, int64_t ldr, int64_t ldo, int rows_per_image,
                      float* gn_part, int groups, int dtype, void* stream);
int dsc_groupnorm_apply_nhwc(const void* x, void* y, const void* gamma, const void* beta, const float* gn_part,
                             int part_rows, int B, int C, int hw, int groups, float eps, int apply_silu, int dtype,
                             void* stream);

/*
 * Split-K form of dsc_linear_f16 for few-row, long-K projections - out = x . w^T (+ bias) (+ residual) - the feed-forward
 * output projections (`ff.net.2`, K = 4C) and the 1x1 `conv_shortcut`s on concatenated skips (K = 1920 / 2560) of the 16x16 and
 * 8x8 UNet levels that modules/u_net_condition_modify.py builds from diffusers blocks (M = 128 / 512 token rows at batch 1).
 * Those GEMMs are bound by how many bytes of cold WEIGHTS are in flight, so the K tiles are dealt over `splits` workgroups per
 * output tile (splits <= 0: chosen from the shape), each writes its raw fp32 tile to `workspace` ([splits][M][N] fp32,
 * dsc_linear_splitk_workspace_bytes; 16-byte aligned) and a second launch adds the splits IN ORDER, then bias and residual, with
 * one fp16 rounding: bit-reproducible, no atomics, no workgroup waits on another.  Same operand constraints as dsc_linear_f16
 * (K % 64 == 0, N % 64 == 0, 16-byte aligned rows); splits == 1 after clamping runs dsc_linear_f16 itself.
 * dsc_linear_splitk_workspace_bytes() is the [splits][M][N] fp32 of the split count actually run (uneven last split included;
 * 0: no split, no workspace); exactly those bytes are written, every one of them, and then read.  out, x and the residual as in
 * dsc_linear_f16, at any ldo / ldx / ldr.
 */
size_t dsc_linear_splitk_workspace_bytes(int64_t M, int N, int K, int splits);
int dsc_linear_splitk_f16(const void* x, const void* w, const void* bias, const void* residual, void* out,
                          int64_t M, int N, int K, int64_t ldx, int64_t ldr, int64_t ldo, int splits,
                          void* workspace, size_t workspace_bytes, int dtype, void* stream);

/*
 * Row softmax of materialised fp16 scores: probs[r, :] = softmax(scale * scores[r, :]), fp32 arithmetic, one fp16 rounding.
 * The middle step of the VAE decoder's / encoder's single 512-channel attention head (diffusers AutoencoderKL mid-block
 * `Attention`, reached from modules/model_k_diffusion.py:291-299 `decode_latents` and :600-606 `vae.encode`): too wide for
 * the flash kernel's registers, so it runs scores = q.k^T (dsc_linear_f16) -> this -> out = probs.v (dsc_linear_f16).
 * rows x n fp16, row strides ld_* in elements (% 8 == 0); n % 8 == 0, n <= 16384.  One workgroup per row, one launch.
 * Reads scores[r][0 .. n) and writes probs[r][0 .. n) only, at any ld_scores / ld_probs >= n.
 */
int dsc_softmax_rows_f16(const void* scores, void* probs, int64_t rows, int n, int64_t ld_scores, int64_t ld_probs,
                         float scale, int dtype, void* stream);

/*
 * The step between the two passes of a hires request: enlarge the final latent rows of the base pass and add the start noise of
 * the second pass, one launch.  Replaces modules/model_k_diffusion.py:1179-1191 (`F.interpolate(latents.float(), size, mode
 * [, antialias]).to(fp16)`) and :647 (`latents + noise * (sigma_0 ** 2 + 1) ** 0.5` on fp16 tensors) of the reference.
 * src [n, C, h, w], noise (NULL: resample only) and dst [n, C, H, W]: fp16, contiguous, H >= h, W >= w; dst must not be src.
 * idx_* / w_* are the separable tap tables of the mode (modules/latent_resample.py): [H, 4] / [W, 4], int32 source indices
 * (clamped into the plane by the kernel) and fp32 weights, 16-byte aligned; unused taps carry weight 0.  Per output element
 *     r   = fp16( sum_i w_y[y, i] * ( sum_j w_x[x, j] * float(src[c, idx_y[y, i], idx_x[x, j]]) ) )   fp32, each sum in tap
 *           order: the first product, then one fma per further tap (the order of torch's CPU kernels)
 *     out = fp16( float(r) + float(fp16( float(noise) * s )) )                                      s = noise_scale_f16_value
 * with s the fp16-rounded sqrt(sigma_0^2 + 1) passed as a float.  16-byte stores when W % 8 == 0 and dst / noise are 16-byte
 * aligned, 2-byte stores otherwise (chosen per launch).  No allocation, no synchronisation: safe under graph capture.
 * DSC_ERR_BAD_ARG: null src / dst / table, n, C, h, w < 1, H < h, W < w, dst == src.  DSC_ERR_UNSUPPORTED: misaligned tables,
 * 2^31 elements or more.
 */
int dsc_latent_resample_noise(const void* src, const void* noise, void* dst, int n, int C, int h, int w, int H, int W,
                              const int* idx_y, const float* w_y, const int* idx_x, const float* w_x,
                              float noise_scale_f16_value, void* stream);

/*
 * The IP-Adapter term of one cross-attention layer, accumulated in place with one scale per batch row, one launch per adapter.
 * Replaces, per adapter, modules/attention_modify.py:370-374 + :385 (IPAdapterAttnProcessor) and :664-674 + :685
 * (IPAdapterAttnProcessor2_0) of the reference: attention of the layer's queries over the adapter's image tokens and
 * `hidden_states + scale * current_ip_hidden_states`, with the processor's Python float `scale` replaced by a device vector:
 *     io[b, l, h, :] = fp16( float(io[b, l, h, :]) +
 *                            row_scale[b] * sum_t softmax_t(softmax_scale * q[b, l, h, :] . k_ip[b, t, h, :]) * v_ip[b, t, h, :] )
 * q [B, L, H, d] fp16 with its strides in elements (innermost 1; q_stride_b may be 0: the shared classifier-free-guidance
 * prefix), k_ip / v_ip [B, T, H, d] fp16, each batch row contiguous and kv_stride_b >= T * H * d elements from the next (views
 * into one buffer per batch row; to_k_ip / to_v_ip of the tokens, :368-369 / :662-663: computed once per generation by the
 * caller), io [B, L, H * d] fp16 contiguous: the text branch's output on entry.  Products of fp16 values
 * accumulate in fp32, the softmax subtracts the row maximum, its unnormalised weights (<= 1) round to fp16 for the second
 * product, 1 / sum and row_scale are applied in fp32, one fp16 rounding at the store.
 * row_scale [B] fp32 is read from DEVICE memory (never by value): a captured launch stays valid when a row's scale changes.
 * row_scale[b] == 0: the workgroups of row b (b is a grid coordinate) return after that one uniform load - k_ip / v_ip / q of
 * the row are not read (they may hold anything) and io is not touched.
 * d % 8 == 0, 8 <= d <= 160; 1 <= T <= DSC_IP_MAX_TOKENS; any L >= 1.  16-byte loads and stores of q / k_ip / io: pointers
 * 16-byte aligned, strides % 8 == 0.  No workspace, no allocation, no synchronisation, no atomics (every io element is read
 * and written by the one lane that owns it), one fixed summation order: deterministic and safe under graph capture.
 * DSC_ERR_BAD_ARG: null pointer, non-positive size or stride (q_stride_b < 0, kv_stride_b < T * H * d), io aliasing an input.  DSC_ERR_UNSUPPORTED:
 * d, T or alignment outside the above, B or H > 65535.
 */
#define DSC_IP_MAX_TOKENS 16
int dsc_ip_xattn_add_f16(const void* q, long long q_stride_b, long long q_stride_l, long long q_stride_h,
                         const void* k_ip, const void* v_ip, long long kv_stride_b, const float* row_scale, void* io,
                         int B, int L, int H, int d, int T, float softmax_scale, void* stream);

/*
 * dsc_ip_xattn_add_f16 with one weight per query: the IP-Adapter region mask (`ip_adapter_masks`) of the reference, which both
 * IP-Adapter processors down-sample to one value per query, convert to the query dtype and multiply into the adapter's attention
 * output before `scale *` and the add (modules/attention_modify.py:371-385 / :676-685):
 *     io[b, l, h, :] = fp16( float(io[b, l, h, :]) + ((row_scale[b] * float(q_weight[b, l])) / sum) * (V^T P^T)[.., l] )
 * q_weight [B, L] fp16, unit inner stride, w_stride_b >= L elements between batch rows, read from DEVICE memory like row_scale
 * (a captured launch stays valid when a mask changes).  Weights are not clamped (bicubic down-sampling overshoots: they may be
 * negative or above 1).  The coefficient is formed in that order: a weight of 1.0 gives the bits of dsc_ip_xattn_add_f16.  Same
 * kernel body as the unmasked entry (a compile-time flag), same launch geometry, arguments and limits.
 * A query whose weight is 0 is NOT stored: its io bits stay as they were, whatever q holds there.  A 16-query tile (queries
 * 16 t .. 16 t + 15 of one (b, h)) whose weights are all 0 issues no q load, no io load and no store: the decision is one
 * wave-uniform ballot over the 16 halfs w[b, 16 t ..], requested ahead of the tile's q / io loads (a tile ahead inside a wave
 * that walks several), so tiles that are not skipped do not wait on it.  row_scale[b] == 0 still returns before anything else
 * of row b is read, its weights included.
 * DSC_ERR_BAD_ARG also for: null q_weight, q_weight == io, w_stride_b < L.  DSC_ERR_UNSUPPORTED also for: q_weight not 2-byte
 * aligned.  No workspace, no LDS, no allocation, no atomics, one fixed summation order.
 */
int dsc_ip_xattn_add_masked_f16(const void* q, long long q_stride_b, long long q_stride_l, long long q_stride_h,
                                const void* k_ip, const void* v_ip, long long kv_stride_b, const float* row_scale, void* io,
                                const void* q_weight, long long w_stride_b, int B, int L, int H, int d, int T, float softmax_scale,
                                void* stream);

/*
 * A residual added to a batch of feature rows with one gate per batch row: the T2I-Adapter hook of the continuous batcher's
 * captured step.  Replaces modules/u_net_condition_modify.py:1194-1230 of the reference (`sample +=
 * down_intrablock_additional_residuals.pop(0)` inside the down blocks), with "this row has a residual at this step" a device
 * value, not Python control flow:
 *     out[r][e] = fp16( float(x[r][e]) + gate[r] * float(feat[r % feat_rows][e]) )        r < rows, e < row_elems
 * x, out: fp16, `rows` dense rows of row_elems halfs (a channels-last [B, C, h, w] tensor: row_elems = h * w * C).  feat: fp16,
 * feat_rows rows of the same length, rows % feat_rows == 0 (one row per slot: batch rows i and n + i, the classifier-free-guidance
 * pair, read row i).  gate [rows] fp32 is read from DEVICE memory (never by value): a captured launch sees the values of the
 * moment it replays.  One fp32 fma and one fp16 rounding of its fp32 result per element: gate[r] == 1 gives the bits of torch's
 * fp16 `x + feat`.  gate[r] == 0: the feature row is not read (it may hold anything); with out == x (in place, allowed) the
 * workgroups of row r return after that one uniform load and the row is neither loaded nor stored; with out != x the row is
 * copied bit for bit.  The batch row is a grid coordinate (rows <= 65535).
 * row_elems % 8 == 0; x, feat, out 16-byte aligned, gate 4-byte aligned: 16-byte loads and stores.  No workspace, no LDS, no
 * allocation, no synchronisation, no atomics, every element written by the one lane that owns it: deterministic and safe under
 * graph capture.
 * DSC_ERR_BAD_ARG: null pointer, rows / feat_rows / row_elems < 1, rows % feat_rows != 0, out overlapping x other than out == x,
 * out overlapping feat or gate.  DSC_ERR_UNSUPPORTED: row_elems % 8 != 0, alignment, rows > 65535.
 */
int dsc_add_rows_gated_f16(const void* x, const void* feat, const void* gate, void* out, int rows, int feat_rows,
                           long long row_elems, void* stream);

/*
 * FreeU (arXiv 2309.11497) on the two inputs of one up-block ResNet, per batch row, in place, in one launch.  Replaces what
 * modules/u_net_condition_modify.py:835-865 of the reference (`enable_freeu` / `disable_freeu`, the up blocks built with
 * `resolution_idx`, :445) switches on: diffusers' `apply_freeu` and `fourier_filter(x, threshold=1, scale)` (fftn, fftshift, a
 * mask multiply, ifftshift, ifftn, .real, a cast) in front of every ResNet of up blocks 0 and 1, with "this row has FreeU" a
 * device value, not Python control flow:
 *     hidden[r][p][c] = fp16( float(hidden[r][p][c]) * b[r] )                       c < C_h / 2
 *     skip[r][p][c]   = fp16( x + (s[r] - 1) / (H W) * [ S0 + Ach cos th + Ash sin th + Acw cos tw + Asw sin tw
 *                                                        + Ac2 cos(th + tw) + As2 sin(th + tw) ] )
 * with th = 2 pi h / H, tw = 2 pi w / W of pixel p = (h, w), x = float(skip[r][p][c]) and the seven sums over the H * W pixels
 * of (r, c): S0 = sum x, Ach / Ash = sum x cos th / sin th, Acw / Asw = sum x cos tw / sin tw, Ac2 / As2 = sum x cos(th + tw) /
 * sin(th + tw) - the scaling of the frequencies {0, -1} x {0, -1}, which is all the filter does at threshold 1.
 * hidden [B, H, W, C_h] and skip [B, H, W, C_s]: fp16, channels-last, dense, both updated IN PLACE.  params [B][4] fp32 =
 * (s1, s2, b1, b2) per batch row, read from DEVICE memory (never by value): a captured launch sees the values of the moment it
 * replays.  stage 0 (up block 0) reads s = params[r][0], b = params[r][2]; stage 1 reads s = params[r][1], b = params[r][3].
 * b[r] == 1: the hidden row is neither read nor written; s[r] == 1: the skip row is neither read nor written (such rows may
 * hold anything).  The batch row is a grid coordinate (B <= 65535).
 * Hidden: one fp32 product, rounded to fp32 and then to fp16, per element: `fp16(fp32(x) * b)`, the bits of torch's fp16 `x * b`
 * on the CPU and of `(x.float() * b).half()` anywhere.  Skip: fp64 sums in a fixed order (per lane, a wave butterfly, the waves
 * through LDS), the formula in fp64, one rounding to fp16 (with s2 = 0.2 the result crosses zero, where fp32 sums were up to 9 fp16
 * ulps off); one workgroup owns all pixels of its channels, with a barrier between its reads and its writes.  No workspace, no allocation, no synchronisation, no atomics:
 * deterministic and safe under graph capture.
 * DSC_ERR_BAD_ARG: null pointer, B < 1, H < 2 or W < 2 (diffusers' slice means something else on a side of 1), C_h / C_s < 1,
 * stage not 0 / 1, any overlap among hidden, skip and params.  DSC_ERR_UNSUPPORTED: C_s % 8 != 0, C_h % 16 != 0, C_h or C_s above
 * 2^20, hidden / skip not 16-byte or params not 4-byte aligned, B > 65535, H or W above DSC_FREEU_MAX_SIDE (the cos / sin tables
 * live in LDS; it also keeps a row's H * W inside an int).
 */
#define DSC_FREEU_MAX_SIDE 512
int dsc_freeu_rows_f16(void* hidden, int C_h, void* skip, int C_s, int B, int H, int W, const float* params, int stage,
                       void* stream);

/*
 * Residuals of a compact ControlNet batch ("lanes") added into the batch rows they belong to: the ControlNet hook of the
 * continuous batcher's captured step.  Replaces, in one launch per skip tensor, ControlNetModel.forward's
 * `d * conditioning_scale`, MultiControlNetModel.forward's sum over the nets and modules/u_net_condition_modify.py:1236-1245 of
 * the reference (`s + r`), with "lane row j serves batch row dst[j] at this scale" device values, not Python control flow.
 * In place on x, for lane row j < lane_rows with dst[j] >= 0 and at least one gate[a][j] != 0, for e < row_elems:
 *     t = fp16( gate[a0][j] * float(feat[a0][j][e]) )                          a0 the first net with gate[a0][j] != 0
 *     t = fp16( float(t) + float(fp16( gate[a][j] * float(feat[a][j][e]) )) )  for each a > a0 with gate[a][j] != 0, in order
 *     x[dst[j]][e] = fp16( float(x[dst[j]][e]) + float(t) )
 * - every product and every sum an fp32 operation, rounded to fp32 and then to fp16 on its own (torch's fp16 `feat * g`,
 * `a + b`, `s + r`); no step is contracted with its neighbour into a single-rounding mixed-precision fma.  With nets == 1 the
 * bits of torch's fp16 `x[d] + feat[j] * g` for a python float g at tensors of 2048 elements and more (below that torch's own
 * multiply launches a kernel variant that rounds the exact product once, and differs from its large-tensor self by an ulp in
 * about 4 % of the elements; this entry rounds the same way at every size).
 * x: fp16, x_rows dense rows of row_elems halfs (a channels-last [X, C, h, w] tensor: row_elems = h * w * C; a token-major
 * [X, L, C] tensor: L * C).  feat: fp16 [nets][lane_rows][row_elems], dense.  gate: fp32 [nets][lane_rows], dst: int32
 * [lane_rows], both read from DEVICE memory (never by value): a captured launch sees the values of the moment it replays.
 * A lane row with dst[j] < 0 (or >= x_rows), or with every gate 0, reads and writes nothing: its feature rows may hold anything
 * and its would-be destination keeps its bits.  A net whose gate is 0 is not read for that lane row.
 * THE CALLER'S INVARIANT, which the kernel cannot check: the destination rows of active lane rows are distinct (two lanes on
 * one row would race).  Rows of x that no active lane names are neither loaded nor stored.
 * The lane row is a grid coordinate (lane_rows <= 65535); nets <= 8.  row_elems % 8 == 0; x, feat 16-byte aligned, gate, dst
 * 4-byte aligned: 16-byte loads and stores.  No workspace, no LDS, no allocation, no synchronisation, no atomics, every element
 * written by the one lane that owns it: deterministic and safe under graph capture.
 * DSC_ERR_BAD_ARG: null pointer, x_rows / lane_rows / nets / row_elems < 1, nets > 8, x overlapping feat, gate or dst.
 * DSC_ERR_UNSUPPORTED: row_elems % 8 != 0, alignment, lane_rows > 65535, x or feat of 2^60 bytes and more.
 */
int dsc_scatter_add_rows_f16(void* x, const void* feat, const void* gate, const void* dst, int x_rows, int lane_rows, int nets,
                             long long row_elems, void* stream);

/*
 * The decoder's output turned into the image a caller receives, in one launch: the decode lane of the continuous batcher.
 * Replaces the tail of modules/model_k_diffusion.py:291-299 of the reference (`decode_latents`: `(image / 2 + 0.5).clamp(0, 1)` on
 * the fp16 tensor, `.cpu().permute(0, 2, 3, 1).float().numpy()`) and, for DSC_IMAGE_U8, `numpy_to_pil`'s
 * `(images * 255).round().astype("uint8")`, reached from :533-539 (`latent_to_image`).
 * img: fp16 [n, 3, H, W], dense and channel-major (what AutoencoderKLDecoder.decode returns).  out: [n, H, W, 3], dense, uint8
 * (DSC_IMAGE_U8) or float32 (DSC_IMAGE_F32).  Per element, every rounding of the reference chain on its own:
 *     h = fp16( float(fp16( float(x) * 0.5f )) + 0.5f ), clamped to [0, 1]
 *     DSC_IMAGE_F32: float(h)          DSC_IMAGE_U8: (uint8) rintf( float(h) * 255.0f )
 * (the product is exact in fp32 - h has at most 11 significant bits - and its only tie, h = 0.5, goes to 128): bit for bit the
 * torch / numpy chain for every fp16 input that is not a NaN.  +-inf clamp like any other value.  NaN inputs are OUTSIDE the
 * contract: 0 is written for them (the reference would propagate the NaN / cast it with an undefined result).
 * H % 8 == 0 and W % 8 == 0 (every image of this project; one lane owns 8 consecutive pixels of a row: three 16-byte loads, 24
 * contiguous output bytes as 8-byte stores or 96 as 16-byte stores).  img 16-byte aligned; out 8-byte (U8) / 16-byte (F32) aligned.
 * No workspace, no LDS, no allocation, no synchronisation, no atomics, every element written by the one lane that owns it and
 * nothing behind the last one: deterministic and safe under graph capture.
 * DSC_ERR_BAD_ARG (before any GPU call): null pointer, out == img, n / H / W < 1, an unknown out_kind.  DSC_ERR_UNSUPPORTED: a side
 * that is no multiple of 8, alignment, 2^31 pieces of 8 pixels and more per image.
 */
#define DSC_IMAGE_U8  0
#define DSC_IMAGE_F32 1
int dsc_image_finish(const void* img, void* out, int n, int H, int W, int out_kind, void* stream);

/*
 * Live previews of running requests: up to 16 latent rows become approximate RGB thumbnails in one launch - the preview path of
 * the continuous batcher (modules/serving/preview_lane.py), which reads the denoised estimate every per-row step entry above
 * leaves in `old`.  Replaces, per preview, the eager chain index / matmul with a [C, 3] matrix / `/ 2 + 0.5` / clamp / `* 255` /
 * round / cast / permute / nearest upsample and its blocking copy.
 * lat: fp16; row rows[j] starts at lat + rows[j] * row_stride halfs and is dense [C, h, w].  rows (n ints) and coef (C * 3 + 3
 * floats: k[c][rgb] row-major, then bias[rgb]) are HOST arrays, read at the call and passed to the kernel by value, as the step
 * records are: the caller may reuse both at once.  out: uint8 [n, h * up, w * up, 3], dense; up in {1, 2, 4, 8}, nearest
 * neighbour (every latent pixel becomes an up x up block).  Per latent pixel and colour, all fp32, every product and every sum
 * rounded to fp32 on its own (no contraction into an fma):
 *     v = bias;  for c in 0..C-1:  v = v + k[c] * float(z[c])                  (channel order, left to right)
 *     y = v * 0.5f + 0.5f;   y = y > 0 ? y : 0;   y = y < 1 ? y : 1            (a NaN compares false: 0)
 *     byte = (uint8) rintf(y * 255.0f)
 * - bit for bit what a numpy float32 restatement gives (ops.latent_preview_numpy).  Non-finite inputs are OUTSIDE the contract:
 * a byte is written for them and nothing else happens.  A row index is not checked against the buffer (its size is not known
 * here): rows[j] must name a row of lat.
 * One lane owns 8 consecutive pixels of one output row (24 contiguous bytes, three 8-byte stores) and loads, per channel, the
 * 8 / up latent pixels under them in one piece of 16, 8, 4 or 2 bytes; the up output rows of a latent row are written by up lanes
 * that each recompute it.  n <= DSC_PREVIEW_MAX_ROWS (the thumbnail is a grid coordinate), C <= DSC_PREVIEW_MAX_CHANNELS.
 * No workspace, no LDS, no allocation, no synchronisation, no atomics, every byte written by the one lane that owns it and nothing
 * behind the last one: deterministic and safe beside captured graphs.
 * DSC_ERR_BAD_ARG (before any GPU call): null pointer; n / C / h / w < 1; n > 16; C > 8; up not in {1, 2, 4, 8}; a negative row
 * index.  DSC_ERR_UNSUPPORTED: (w * up) % 8 != 0 (any w runs with up = 8); lat not aligned to, or row_stride no multiple of, the
 * piece of 8 / up halfs; out not 8-byte aligned; 2^31 pieces of 8 pixels and more per thumbnail.
 */
#define DSC_PREVIEW_MAX_ROWS     16
#define DSC_PREVIEW_MAX_CHANNELS 8
int dsc_latent_preview(const void* lat, long long row_stride, const int* rows, int n, int C, int h, int w, const float* coef,
                       int up, void* out, void* stream);

/*
 * Pixel inputs of served requests, the reverse direction of dsc_image_finish: the two launches around the VAE encoder's captured
 * graph on the encode lane of the continuous batcher (modules/serving/encode_lane.py).
 *
 * dsc_image_prepare: up to DSC_IMAGE_PREPARE_MAX_ROWS request images become what `vae.encode` and the sampler step read, in one
 * launch.  Replaces, per request, the reference's VaeImageProcessor.preprocess at its call sites
 * modules/model_k_diffusion.py:1447-1449 (the image: bytes / 255, `2 x - 1`, channel-major float32) and :1480-1482 (the mask,
 * binarised at 0.5, and the masked image `init_image * (mask < 0.5)`), the conversion to the VAE's fp16 inside
 * `_encode_vae_image` (:1234-1246) and `F.interpolate(mask, size=(h, w))` (:1253-1257; default nearest: pixel (8 i, 8 j)).
 * rows: a HOST array of n records, read at the call and passed to the kernel by value (the caller may reuse it at once).  Per row:
 *     image      uint8 [H, W, 3] (DSC_PIXELS_U8: the bytes of a PIL image) or float32 [3, H, W] in [-1, 1] (DSC_PIXELS_F32), dense
 *     mask       uint8 [H, W] or float32 [H, W], dense; NULL when the row has none
 *     out_image  fp16 [3, H, W]: fp16(v), v = 2.0f * (float(b) / 255.0f) - 1.0f (an IEEE division) / v = x;  NULL: not wanted
 *     out_masked fp16 [3, H, W]: fp16(v * (m ? 0.0f : 1.0f)), the literal fp32 product (-0.0 under a negative v);  NULL: not wanted
 *     out_mask   fp16 [mask_rep, H / 8, W / 8]: fp16(m) of pixel (8 i, 8 j), mask_rep (1 or 4) times;  NULL: not wanted
 * with m = b >= 128 (uint8) / x >= 0.5f (float32; a NaN compares false).  Bit for bit the torch chain for every input.  A row
 * whose three destinations are NULL is neither read nor written; with no destination in any row nothing is launched.
 * H % 8 == 0 and W % 8 == 0: one lane owns 16 consecutive pixels of the dense plane - 48 interleaved bytes as three 16-byte loads
 * split into planes in registers (four 16-byte loads per float32 plane), two 16-byte stores per channel; the lane whose 8-pixel
 * half starts a latent cell stores its mask sample.  image, mask, out_image, out_masked 16-byte aligned; out_mask 2-byte.
 * No workspace, no LDS, no allocation, no synchronisation, no atomics, every element written by the one lane that owns it and
 * nothing behind the last one: deterministic and safe beside captured graphs.
 * DSC_ERR_BAD_ARG (before any GPU call): rows NULL; n < 1 or > 16; H / W < 1; a wanted destination without its source; an
 * unknown kind; mask_rep not 1 or 4; out_image == out_masked.  DSC_ERR_UNSUPPORTED: a side that is no multiple of 8, alignment,
 * 2^31 pieces of 16 pixels and more.
 *
 * dsc_latent_start_rows: after the encode, every row of it in one launch.  Replaces DiagonalGaussianDistribution.sample and
 * `_encode_vae_image`'s product (:1234-1246), img2img's start latent (:647) and prepare_latents_inpating's branches (:1306-1362),
 * with an fp16 rounding wherever that chain holds an fp16 tensor:
 *     lv  = clamp(logvar, -30, 20);   std = fp16(expf(float(fp16(0.5f * lv))))
 *     lat = fp16(scaling * float(fp16(mean + fp16(std * eps))))
 *     DSC_START_ADD:   start = fp16(lat + fp16(noise * coef))    (img2img: coef = fp16 sqrt(sigma_0^2 + 1); inpainting below
 *                                                                  strength 1: coef = sigma_0, both fp16 values)
 *     DSC_START_SCALE: start = fp16(noise * coef)                (inpainting at strength 1 / with given latents:
 *                                                                  coef = fp32(sqrt(sigma_0^2 + 1)) of the python float)
 *     DSC_START_NONE:  no start latent                           (the masked image of a 9-channel request)
 * moments: fp16 [m, 8, h, w] dense (`vae.encode(x).latent_dist.parameters`: mean | logvar).  rows: a HOST array of n records, by
 * value as above.  Per row: kind (DSC_START_IDLE: neither read nor written), moments_row in [0, m), eps (the posterior draw) and
 * noise, fp16 [4, h, w]; start fp16 [4, h, w]; keep (optional) receives lat - r.known["image"] of 4-channel inpainting, rows 1..4
 * of r.extra for a masked-image row; keep_noise (optional) receives the noise row as it is.
 * One lane owns 8 consecutive halfs of a row's 4 h w: 16-byte loads and stores when 4 h w % 8 == 0 and every pointer is 16-byte
 * aligned, otherwise element by element with a bound check (any h, w; pointers 2-byte aligned).
 * No workspace, no LDS, no allocation, no synchronisation, no atomics: deterministic and safe beside captured graphs.
 * DSC_ERR_BAD_ARG: NULL moments / rows; m / n / h / w < 1; n > 16; an unknown kind; moments_row outside [0, m); NULL eps; a start
 * kind without noise or start; DSC_START_NONE without keep; keep_noise without noise; two destinations of a row that are one.
 * DSC_ERR_UNSUPPORTED: an odd pointer; 2^30 halfs and more per row.
 */
#define DSC_IMAGE_PREPARE_MAX_ROWS 16
#define DSC_PIXELS_U8  0
#define DSC_PIXELS_F32 1
typedef struct {
    const void* image;
    const void* mask;
    int image_kind;
    int mask_kind;
    void* out_image;
    void* out_masked;
    void* out_mask;
    int mask_rep;
} dsc_image_prepare_row;
int dsc_image_prepare(const dsc_image_prepare_row* rows, int n, int H, int W, void* stream);

#define DSC_START_IDLE  0
#define DSC_START_ADD   1
#define DSC_START_SCALE 2
#define DSC_START_NONE  3
typedef struct {
    int kind;
    int moments_row;
    const void* eps;
    const void* noise;
    float scaling;
    float coef;
    void* start;
    void* keep;
    void* keep_noise;
} dsc_latent_start_row;
int dsc_latent_start_rows(const void* moments, int m, const dsc_latent_start_row* rows, int n, int h, int w, void* stream);

/*
 * The CLIP text encoder's two own kernels (modules/clip_text.py; the encoder the reference loads from transformers and calls
 * from modules/encoder_prompt_modify.py and modules/prompt_parser.py).  Its GEMMs and LayerNorms are dsc_linear_f16 and
 * dsc_add_layernorm.
 *
 * dsc_causal_attn_f16: causal self-attention over one text chunk,
 *   out[b,i,h,:] = softmax_{j<=i}(scale * q[b,i,h,:].k[b,j,h,:]) . v[b,j,h,:]        (transformers CLIPAttention with the causal mask)
 * Addressing as dsc_self_attn_fwd: q / k / v / out are [B, S, H, d] through {sb, ss, sh} element strides, so q, k and v may be
 * views of one fused [B, S, 3 H d] projection and out a view of a wider buffer.  scale <= 0 means 1/sqrt(d).
 * One workgroup per (b, h) keeps the head's K and V in LDS; scores stay in MFMA accumulators; maximum and sum in fp32 over the
 * whole row; probabilities round to fp16 for the second product and are normalised by the sum of the ROUNDED values (a row with
 * one key is exactly v).  Rows >= S of any operand are never read, rows >= S of out never written.  No workspace.
 * Limits - stated here once, mirrored by ops.causal_attn_takes: fp16, d == DSC_CAUSAL_ATTN_HEAD_DIM (CLIP-L, OpenCLIP-H and bigG),
 * 1 <= S <= DSC_CAUSAL_ATTN_MAX_TOKENS (five 16-row MFMA tiles), strides % 8 == 0, 16-byte aligned pointers, B * H < 2^31:
 * otherwise DSC_ERR_UNSUPPORTED.  A null pointer or a non-positive B / H / S / d: DSC_ERR_BAD_ARG.  All checks before the launch.
 */
#define DSC_CAUSAL_ATTN_HEAD_DIM   64
#define DSC_CAUSAL_ATTN_MAX_TOKENS 80
int dsc_causal_attn_f16(const void* q, const void* k, const void* v, void* out, int B, int H, int S, int d,
                        const int64_t q_strides[3], const int64_t k_strides[3],
                        const int64_t v_strides[3], const int64_t o_strides[3],
                        float scale, int dtype, void* stream);
/*
 * dsc_act_f16: x <- act(x) in place over a contiguous fp16 buffer of n elements (between fc1 and fc2 of the encoder's MLP); fp32
 * arithmetic, one fp16 rounding, 16-byte accesses.
 *   DSC_ACT_QUICK_GELU: x * sigmoid(1.702 x)                 (hidden_act "quick_gelu": SD1.5's CLIP-L)
 *   DSC_ACT_GELU_ERF:   x/2 (1 + erf(x / sqrt 2))            (hidden_act "gelu": the OpenCLIP encoders of SD2 and SDXL)
 * NaN and +-inf come out as the fp32 formula gives them (-inf -> NaN in both).  n % 8 == 0, 16-byte aligned x, fp16, fewer than
 * 2^31 workgroups of 2048 elements: otherwise DSC_ERR_UNSUPPORTED.  NULL x, n <= 0 or an unknown kind: DSC_ERR_BAD_ARG.
 */
#define DSC_ACT_QUICK_GELU 0
#define DSC_ACT_GELU_ERF   1
int dsc_act_f16(void* x, int64_t n, int kind, int dtype, void* stream);

/*
 * dsc_prompt_weight_rows_f16: prompt emphasis after the text encoder on the text lane of the continuous batcher
 * (modules/serving/text_lane.py), for up to DSC_PROMPT_WEIGHT_MAX_GROUPS (request, chunk) groups in one launch.  Replaces the tail
 * of FrozenCLIPEmbedderWithCustomWordsBase.process_tokens (reference modules/prompt_parser.py:196-221: `z * multipliers` with the
 * tensor mean restored), the hstack over chunks in its forward and the cast of encode_prompt_automatic1111.  Per group, with
 * N = 2 T C the elements of its two rows of z and m the fp32 multiplier of a token:
 *     before = fp16(sum z / N);   p = fp32(z) * m, every product rounded to fp32;   after = fp32(sum p / N)
 *     ratio  = fp32(before) / after   (an IEEE fp32 division);   out = fp16(fp32(p * ratio))
 * Both sums are fp64 sums over BOTH rows in a fixed order, each divided by N in fp64 and rounded once.  No guard on after == 0:
 * inf and NaN follow IEEE, as in the eager chain (all-zero multipliers give NaN everywhere).  The product, the scaling and the
 * conversion to fp16 are three separate roundings.
 * z: fp16 [m, T, C] dense (the encoder's output).  groups: a HOST array of n records, read at the call and passed to the kernel by
 * value (the caller may reuse it at once).  Per group: z_row[2], its negative and positive row of z, each in [0, m), in any order
 * and not necessarily adjacent; mult, DEVICE fp32 [2][T]; out[2], fp16 [T, C] destinations with row stride ldo (elements) - chunk
 * k's place inside a request's negative / positive [S, C] row.  A group whose two destinations are NULL is neither read nor
 * written; with no live group nothing is launched.
 * C % 8 == 0, ldo % 8 == 0, z and every destination 16-byte aligned, mult 4-byte aligned, any T >= 1.  No workspace, no atomics, no
 * allocation; deterministic, and the bits do not depend on the grid: every workgroup of a group redoes the group's sums in the
 * order its 1024 lanes define and stores one slice.  Safe beside captured graphs.
 * DSC_ERR_BAD_ARG (before any GPU call): NULL z / groups; m, T, C < 1; n < 1 or > 16; ldo < C; a group with one NULL destination,
 * a NULL mult, a z_row outside [0, m), out[0] == out[1] (or two dense destinations that overlap), a destination that overlaps z
 * or the group's mult.  DSC_ERR_UNSUPPORTED: C % 8 or ldo % 8, alignment, 2^30 elements and more per row of z.
 * dsc_debug_set_prompt_weight_slices: workgroups per group for A/B runs (tools/mb_prompt_weight.py); 0 = the launch rule.
 */
#define DSC_PROMPT_WEIGHT_MAX_GROUPS 16
typedef struct {
    int z_row[2];
    const void* mult;
    void* out[2];
} dsc_prompt_weight_group;
int dsc_prompt_weight_rows_f16(const void* z, int m, int T, int C, const dsc_prompt_weight_group* groups, int n, long long ldo,
                               void* stream);
void dsc_debug_set_prompt_weight_slices(int slices);

/*
 * dsc_lora_merge_f16: LoRA adapters merged into a table of weights in one launch (modules/lora.py; the reference merges in
 * load_lora_control_pipeline, app.py:532-597, with four to five eager launches per layer).  Per job, one nn.Linear or 1x1-conv
 * weight [N, K] (a [N, K, 1, 1] weight has the same bytes):
 *     dst[n,k] = fp16( fp32(base[n,k]) + sum_seg gain[seg] * ( sum_{r in seg} up[n,r] * down[r,k] ) )
 * base: fp16 [N, K] dense, the pristine copy, never written.  dst: fp16 [N, K] with row stride ld_dst (elements), the live
 * parameter.  up: fp16 [N, R] dense, down: fp16 [R, K] dense: all adapters of the job concatenated along the rank, each padded
 * with zero columns / rows to a multiple of DSC_LORA_SEGMENT.  A segment is DSC_LORA_SEGMENT consecutive rank columns of one
 * adapter; gain: DEVICE fp32 [R / DSC_LORA_SEGMENT], read by the kernel (a rescale uploads gains and launches again).
 * Arithmetic: a segment's sum is one v_mfma_f32_16x16x32_f16 from a zero accumulator; the gain multiplies that fp32 sum (a
 * rounding of its own); segments are added in ascending order in fp32; base is added last; one rounding to fp16, to nearest
 * even.  A segment whose gain is 0 is skipped - its up / down values are not read, NaN and inf included - so all gains 0 gives
 * dst == base bit for bit.  The order is fixed per 64 x 64 tile: the bits do not depend on the grid or on the other jobs.
 * dsc_lora_merge_plan(jobs, n) checks a HOST table and writes each job's tile0 (the prefix sum of tile counts a workgroup
 * bisects to find its job) -> the launch's tile count (> 0), or a negative status.  dsc_lora_merge_f16 takes that host table
 * (checked again, nothing else is read from it) and a DEVICE copy of the same bytes, which is what the kernel reads.
 * Limits - stated here once, mirrored by ops.lora_merge_takes: fp16; K % 8 == 0 and ld_dst % 8 == 0 (16-byte rows); any N >= 1
 * (the last row tile is masked); R % DSC_LORA_SEGMENT == 0, R <= DSC_LORA_MAX_RANK; base / dst / up / down 16-byte aligned, gain
 * 4-byte, the device table 8-byte; fewer than 2^31 tiles: otherwise DSC_ERR_UNSUPPORTED.
 * DSC_ERR_BAD_ARG: NULL tables, n < 1, a NULL pointer in a job, N / K / R < 1, ld_dst < K, dst overlapping the job's base, up,
 * down or gain, a tile0 that is not the plan's.  All checks run on the host before the launch.  No workspace, no atomics, no
 * allocation, no synchronisation.
 */
#define DSC_LORA_SEGMENT  32
#define DSC_LORA_MAX_RANK 256
typedef struct {
    const void* base;
    void* dst;
    const void* up;
    const void* down;
    const float* gain;
    int N, K, R;
    int tile0;
    long long ld_dst;
} dsc_lora_job;
long long dsc_lora_merge_plan(dsc_lora_job* jobs, int n_jobs);
int dsc_lora_merge_f16(const dsc_lora_job* jobs, const void* jobs_dev, int n_jobs, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSC_HIP_H */
