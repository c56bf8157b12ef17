"""Thin torch-tensor wrappers over the C ABI (include/dsc_hip.h).  torch is plumbing here: device memory,
the current HIP stream and strides; all arithmetic happens in libdsc_hip.so."""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib

FLAG_REF_FP16_ROUNDING = 1
FLAG_BIAS_IS_FINAL = 2
FLAG_REUSE_STATS = 4
FLAG_ROWS_PADDED = 256
FLAG_SIGMA_PER_GROUP = 512
REGION_ROW_STRIDE = 100    # region_xattn_packed.hip kBP: the forward kernel's LDS bias-table row stride (floats)
# What the attention kernels can read - stated here once; every Python site that routes by a key count or a head dim asks these
XATTN_MAX_KEYS = 96            # xattn_shared.h kSMax: one 77-token text chunk, padded to three MFMA row tiles
XATTN_MAX_KEYS_PACKED = 384    # region_xattn_packed.hip kSMax x kChunksMax: long prompts (77 n tokens) on the chunked kernels
ATTN_MAX_HEAD_DIM = 160        # the `d > 160` of check_common (csrc/region_xattn.hip), dsc_self_attn_fwd and dsc_ip_xattn_add_f16


def attn_head_dim_ok(d):
    """a head dim the attention kernels take: a multiple of 8 (16-byte pieces of fp16), at most ATTN_MAX_HEAD_DIM"""
    return d % 8 == 0 and 8 <= d <= ATTN_MAX_HEAD_DIM


def attn_kernel_takes(dtype, d):
    """fp16 with a head dim the kernels take: what check_common, dsc_self_attn_fwd and dsc_ip_xattn_add_f16 all require"""
    return dtype == torch.float16 and attn_head_dim_ok(d)


def xattn_kv_packable(S, d):
    """this (S, d) has a packed K/V image (dsc_xattn_kv_pack_bytes != 0)"""
    return S <= XATTN_MAX_KEYS_PACKED and attn_head_dim_ok(d)


def _stream_ptr(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _i64x3(a, b, c):
    return (ctypes.c_int64 * 3)(a, b, c)


def _require_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.DscLibraryError("dsc ops run on the GPU only (no CPU fallback); got a CPU tensor")


def _check_out(out, shape, like, what):
    """an `out=` the caller supplied is written through its raw pointer as a [shape] fp16 tensor on `like`'s device: anything
    smaller, of another dtype or on another device would be an out-of-bounds or foreign write, so refuse it before any launch"""
    if out.dtype != torch.float16:
        raise TypeError(f"{what}: out must be fp16, got {out.dtype}")
    if out.device != like.device:
        raise ValueError(f"{what}: out is on {out.device}, the operands on {like.device}")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{what}: out has shape {tuple(out.shape)}, the kernel writes {tuple(shape)}")
    return out


def _workspace(device, nbytes):
    """fp64 scratch for one call, from torch's caching allocator.  Deliberately NOT cached across calls: inside a
    HIP-graph capture the allocation must belong to that graph's private pool, and a buffer remembered from an
    earlier (since destroyed) capture would alias live activations of the next one."""
    return torch.empty(max(nbytes, 16) // 8 + 1, dtype=torch.float64, device=device)


USE_CFG_SHARED_PREFIX = os.environ.get("DSC_CFG_PREFIX", "1") != "0"   # captured step: the layers in front of the first cross-attention once per image
USE_TEMB_HOIST = os.environ.get("DSC_TEMB_HOIST", "1") != "0"   # fused loop: the time-embedding path once per schedule, not per step


TUNING_PROFILES = {"latency": 0, "throughput": 1}       # DSC_TUNE_LATENCY / DSC_TUNE_THROUGHPUT (include/dsc_hip.h)


def set_tuning_profile(name):
    """launch rules for one generation at a time ("latency", the default) or for several generations in flight on their
    own streams ("throughput") - dsc_set_tuning_profile.  Read at launch time: a step graph keeps the profile it was
    captured under, and the pipeline re-captures a slot's step when the profile has changed since.  The package's own kernels
    give equal bytes under both; a GEMM left to the library (dsc_linear_lt_f16) may run another library algorithm and then
    agrees to rounding only."""
    if name not in TUNING_PROFILES:
        raise ValueError(f"tuning profile must be one of {sorted(TUNING_PROFILES)}")
    _lib.check(_lib.load_library().dsc_set_tuning_profile(TUNING_PROFILES[name]), "dsc_set_tuning_profile")


def tuning_profile():
    v = _lib.load_library().dsc_get_tuning_profile()
    return next(k for k, x in TUNING_PROFILES.items() if x == v)


def _blhd_strides(t, layout):
    """(sb, sl, sh) element strides of a [B, L, H, d]-addressable tensor.
    layout 'blc': t is [B, L, H*d] (or a view [B, L, H, d]);  'bhld': t is [B, H, L, d]."""
    if t.stride(-1) != 1:
        raise ValueError("innermost dimension must be contiguous")
    if layout == "bhld":
        B, H, L, d = t.shape
        return (t.stride(0), t.stride(2), t.stride(1)), (B, H, L, d)
    B, L, H, d = t.shape
    return (t.stride(0), t.stride(1), t.stride(2)), (B, H, L, d)


def region_xattn(q, k, v, region=None, sigma=1.0, *, layout="bhld", n_std_groups=1, scale=None,
                 ref_fp16_rounding=True, bias_is_final=False, out=None, reuse_stats=False, debug_flags=0,
                 per_group_sigma=False):
    """softmax(scale*q.k^T + region*sigma*std) . v  on the GPU (dsc_region_xattn_fwd).

    layout 'bhld': q [Bc,H,L,d], k/v [Bc,H,S,d] -> out [Bc,H,L,d] (the shape of
                   scaled_dot_product_attention_regionstate, attention_modify.py:74);
    layout 'blhd': q [Bc,L,H,d], k/v [Bc,S,H,d] (views of the projection outputs) -> out [Bc,L,H,d] contiguous,
                   i.e. already the [Bc, L, H*d] tensor `to_out[0]` consumes.
    region: fp32 [Bw,L,S] on the same device or None.  sigma: python float or a 0-dim/1-element fp32 CUDA tensor.
    per_group_sigma: sigma is an [n_std_groups] fp32 CUDA tensor and batch row b uses sigma[b % n_std_groups]
    (DSC_FLAG_SIGMA_PER_GROUP; continuous batching).  Never inferred from sigma's size.
    """
    _require_gpu(q, k, v, region)
    lib = _lib.load_library()
    if q.dtype != torch.float16 or k.dtype != torch.float16 or v.dtype != torch.float16:
        raise TypeError("region_xattn: fp16 tensors only (the dtype the reference pipeline runs in)")
    lay = "bhld" if layout == "bhld" else "blc"
    qs, (Bc, H, L, d) = _blhd_strides(q, lay)
    ks, (_, _, S, _) = _blhd_strides(k, lay)
    vs, _ = _blhd_strides(v, lay)
    if out is None:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    _check_out(out, q.shape, q, "region_xattn")
    _drop_gn_partials(out)
    os_, _ = _blhd_strides(out, lay)
    Bw = 0
    rptr = None
    if region is not None:
        if region.dtype != torch.float32:
            region = region.float()
        region = region.contiguous()
        if region.shape[1] != L or region.shape[2] != S:
            raise ValueError(f"region table {tuple(region.shape)} does not match L={L}, S={S}")
        Bw = region.shape[0]
        rptr = ctypes.c_void_p(region.data_ptr())
    sig_host, sig_dev = _sigma_args(sigma, per_group_sigma, n_std_groups, q.device, "region_xattn")
    flags = _xattn_flags(ref_fp16_rounding, reuse_stats, per_group_sigma, debug_flags) | (FLAG_BIAS_IS_FINAL if bias_is_final else 0)
    nbytes = lib.dsc_region_xattn_workspace_bytes(Bc, H, L, S, d, n_std_groups)
    ws = _workspace(q.device, nbytes)
    rc = lib.dsc_region_xattn_fwd(
        ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(v.data_ptr()),
        ctypes.c_void_p(out.data_ptr()), rptr, Bc, H, L, S, d, Bw, n_std_groups,
        _i64x3(*qs), _i64x3(*ks), _i64x3(*vs), _i64x3(*os_),
        sig_host, sig_dev, float(scale) if scale else 0.0, 0, flags,
        ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _stream_ptr(q))
    _lib.check(rc, "dsc_region_xattn_fwd")
    return out


def _sigma_args(sigma, per_group, n_std_groups, device, what):
    """(sigma_host, sigma_dev) of the region kernels: an fp32 device tensor goes by pointer (no host sync), anything else as a host
    float; per_group: one fp32 sigma per std group, dense on the attention's device"""
    if per_group:
        if not (isinstance(sigma, torch.Tensor) and sigma.is_cuda and sigma.dtype == torch.float32 and sigma.dim() == 1
                and sigma.numel() == n_std_groups and sigma.is_contiguous() and sigma.device == device):
            raise ValueError(f"{what}: per_group_sigma needs a dense [n_std_groups={n_std_groups}] fp32 tensor on {device}")
    elif not (isinstance(sigma, torch.Tensor) and sigma.is_cuda and sigma.dtype == torch.float32):
        return float(sigma), None
    return 0.0, ctypes.c_void_p(sigma.data_ptr())


def _xattn_flags(ref_fp16_rounding, reuse_stats, per_group_sigma, debug_flags):
    return (FLAG_REF_FP16_ROUNDING if ref_fp16_rounding else 0) | (FLAG_REUSE_STATS if reuse_stats else 0) \
        | (FLAG_SIGMA_PER_GROUP if per_group_sigma else 0) | debug_flags


def xattn_kv_pack(k, v, *, layout="blhd", out=None):
    """Pack cross-attention K / V ([Bc,S,H,d] views, or [Bc,H,S,d] with layout='bhld') into the MFMA-fragment image
    of dsc_xattn_kv_pack (once per generation: text keys/values are step-invariant)."""
    _require_gpu(k, v)
    lib = _lib.load_library()
    lay = "bhld" if layout == "bhld" else "blc"
    ks, (Bc, H, S, d) = _blhd_strides(k, lay)
    vs, _ = _blhd_strides(v, lay)
    nbytes = lib.dsc_xattn_kv_pack_bytes(Bc, H, S, d)
    if nbytes == 0:
        raise _lib.DscLibraryError(f"xattn_kv_pack: unsupported shape S={S}, d={d}")
    if out is None or out.numel() * 2 != nbytes or out.dtype != torch.float16 or out.device != k.device or not out.is_contiguous():
        out = torch.empty(nbytes // 2, dtype=torch.float16, device=k.device)
    _drop_gn_partials(out)
    rc = lib.dsc_xattn_kv_pack(_p(k), _p(v), _p(out), Bc, H, S, d, _i64x3(*ks), _i64x3(*vs), 0, _stream_ptr(k))
    _lib.check(rc, "dsc_xattn_kv_pack")
    return out


MAX_REGION_ROWS = 32


def compress_region_table(w, pad_rows=False):
    """dense fp32 [Bw, L, S] -> (ids int16 [Bw, L], rows fp32 [NU, S]) with rows = the distinct table rows, or None
    when there are more than MAX_REGION_ROWS of them.  Lossless (rows[ids] == w).  Works on the tensor's own device:
    on a CPU table (where the reference keeps them, encode_region_map_function.py:33-34) nothing touches the GPU.
    pad_rows: zero-pad `rows` to MAX_REGION_ROWS so that shapes (and captured kernel arguments) never change."""
    Bw, L, S = w.shape
    flat = w.reshape(Bw * L, S)
    if not flat.is_cuda:
        # numpy (single-threaded, no torch intra-op pool): distinct rows through a 1-D key (two fixed random
        # projections in fp64), then verified exactly
        a = flat.contiguous().numpy()
        proj = np.random.default_rng(1234).random((S, 2))
        key = a.astype(np.float64) @ proj
        _, first_idx, inv_np = np.unique(key[:, 0] * 1.000123 + key[:, 1], return_index=True, return_inverse=True)
        if first_idx.shape[0] > MAX_REGION_ROWS:
            return None
        rows_np = a[first_idx]
        if not np.array_equal(rows_np[inv_np], a):       # projection collision (never seen): exact fallback
            rows_np, inv_np = np.unique(a, axis=0, return_inverse=True)
            if rows_np.shape[0] > MAX_REGION_ROWS:
                return None
        rows, inv = torch.from_numpy(np.ascontiguousarray(rows_np)), torch.from_numpy(inv_np.reshape(-1).astype(np.int64))
    else:
        rows, inv = torch.unique(flat, dim=0, return_inverse=True)
        if rows.shape[0] > MAX_REGION_ROWS:
            return None
    if pad_rows and rows.shape[0] < MAX_REGION_ROWS:
        rows = torch.cat([rows, rows.new_zeros(MAX_REGION_ROWS - rows.shape[0], S)])
    return inv.reshape(Bw, L).to(torch.int16).contiguous(), rows.contiguous()


def pad_region_rows(rows):
    """distinct region rows [NU, S] (compress_region_table) -> [NU, 100] fp32, zero padded: the shape of the forward kernel's LDS
    table, which it then fills with a flat 16-byte copy (DSC_FLAG_ROWS_PADDED).  S <= XATTN_MAX_KEYS."""
    NU, S = rows.shape
    if S > XATTN_MAX_KEYS:
        raise ValueError(f"pad_region_rows: at most {XATTN_MAX_KEYS} keys (one text chunk)")
    out = rows.new_zeros((NU, REGION_ROW_STRIDE), dtype=torch.float32)
    out[:, :S] = rows
    return out


def compress_region_table_for_kernel(w, pad_rows=False):
    """compress_region_table, with the rows in the forward kernel's own table shape (pad_region_rows) when the keys are one text
    chunk: what region_xattn_packed takes as `region`, or None"""
    comp = compress_region_table(w, pad_rows)
    if comp is not None and comp[1].shape[1] <= XATTN_MAX_KEYS:
        comp = (comp[0], pad_region_rows(comp[1]))
    return comp


def region_xattn_packed(q, packed_kv, S, region=None, sigma=1.0, *, n_std_groups=1, scale=None, ref_fp16_rounding=True,
                        out=None, reuse_stats=False, debug_flags=0, per_group_sigma=False):
    """dsc_region_xattn_fwd_packed: q [Bc,L,H,d] view, packed_kv from xattn_kv_pack, region = (ids, rows) from
    compress_region_table (device tensors; rows optionally through pad_region_rows) or None -> out [Bc,L,H,d] contiguous.
    per_group_sigma: as region_xattn."""
    _require_gpu(q, packed_kv)
    lib = _lib.load_library()
    qs, (Bc, H, L, d) = _blhd_strides(q, "blc")
    if out is None:
        out = torch.empty((Bc, L, H, d), dtype=q.dtype, device=q.device)
    _check_out(out, (Bc, L, H, d), q, "region_xattn_packed")
    _drop_gn_partials(out)
    os_, _ = _blhd_strides(out, "blc")
    ids = rows = None
    Bw = nrows = 0
    if region is not None:
        ids, rows = region
        Bw, nrows = ids.shape[0], rows.shape[0]
    sig_host, sig_dev = _sigma_args(sigma, per_group_sigma, n_std_groups, q.device, "region_xattn_packed")
    flags = _xattn_flags(ref_fp16_rounding, reuse_stats, per_group_sigma, debug_flags)
    if rows is not None and rows.shape[1] == REGION_ROW_STRIDE and S <= XATTN_MAX_KEYS:      # pad_region_rows() form
        flags |= FLAG_ROWS_PADDED
    ws = _workspace(q.device, lib.dsc_region_xattn_workspace_bytes(Bc, H, L, S, d, n_std_groups))
    rc = lib.dsc_region_xattn_fwd_packed(_p(q), _p(packed_kv), _p(out), _p(ids), _p(rows), nrows, Bc, H, L, S, d, Bw,
                                         n_std_groups, _i64x3(*qs), _i64x3(*os_), sig_host, sig_dev,
                                         float(scale) if scale else 0.0, 0, flags, _p(ws), ws.numel() * 8, _stream_ptr(q))
    _lib.check(rc, "dsc_region_xattn_fwd_packed")
    return out


def mask_3d(mask, BH, L, S, check=True):
    """an additive attention mask as the kernels read it: fp32 [1 | BH, 1 | L, S] (leading dimensions added as needed).
    check=False: the caller adds the mask to [BH, L, S] scores with torch first, whose broadcast error is then the refusal"""
    m3 = mask.float()
    while m3.dim() < 3:
        m3 = m3.unsqueeze(0)
    if check and (m3.dim() != 3 or m3.shape[2] != S or m3.shape[1] not in (1, L) or m3.shape[0] not in (1, BH)):
        raise ValueError(f"mask {tuple(mask.shape)} does not broadcast to [{BH}, {L}, {S}]")
    return m3


def region_xattn_std(q, k, *, layout="bhld", n_std_groups=1, scale=None, ref_fp16_rounding=True, mask=None):
    """std of scale*q.k^T (+ mask) per std group (dsc_region_xattn_std[_masked]) -> fp32 CUDA tensor [n_std_groups].
    mask: additive fp32 CUDA tensor broadcastable to [Bc*H, L, S] (shapes [L, S], [1, S], [Bc*H, 1, S], [Bc*H, L, S], ...)."""
    _require_gpu(q, k, mask)
    lib = _lib.load_library()
    lay = "bhld" if layout == "bhld" else "blc"
    qs, (Bc, H, L, d) = _blhd_strides(q, lay)
    ks, (_, _, S, _) = _blhd_strides(k, lay)
    out = torch.empty(n_std_groups, dtype=torch.float32, device=q.device)
    nbytes = lib.dsc_region_xattn_workspace_bytes(Bc, H, L, S, d, n_std_groups)
    ws = _workspace(q.device, nbytes)
    flags = FLAG_REF_FP16_ROUNDING if ref_fp16_rounding else 0
    if mask is None:
        rc = lib.dsc_region_xattn_std(
            ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(k.data_ptr()), Bc, H, L, S, d, n_std_groups,
            _i64x3(*qs), _i64x3(*ks), float(scale) if scale else 0.0, 0, flags, ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _stream_ptr(q))
        _lib.check(rc, "dsc_region_xattn_std")
        return out
    m3 = mask_3d(mask, Bc * H, L, S).contiguous()
    ms = (ctypes.c_int64 * 2)(0 if m3.shape[0] == 1 else m3.stride(0), 0 if m3.shape[1] == 1 else m3.stride(1))
    rc = lib.dsc_region_xattn_std_masked(
        ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(k.data_ptr()), Bc, H, L, S, d, n_std_groups,
        _i64x3(*qs), _i64x3(*ks), float(scale) if scale else 0.0, 0, flags, ctypes.c_void_p(m3.data_ptr()), ms,
        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _stream_ptr(q))
    _lib.check(rc, "dsc_region_xattn_std_masked")
    return out


# ----------------------------------------------------------------------------- ops of the UNet step
def self_attention(q, k, v, scale=None, out=None):
    """softmax(q.k^T * scale) . v for q [B, L, H, d], k/v [B, S, H, d] (strided views allowed) -> [B, L, H, d]
    contiguous (dsc_self_attn_fwd: flash attention, scores never materialised)."""
    _require_gpu(q, k, v)
    if q.dtype != torch.float16:
        raise TypeError("self_attention: fp16 only")
    qs, (B, H, L, d) = _blhd_strides(q, "blc")
    ks, (_, _, S, _) = _blhd_strides(k, "blc")
    vs, _ = _blhd_strides(v, "blc")
    if out is None:
        out = torch.empty((B, L, H, d), dtype=q.dtype, device=q.device)
    _check_out(out, (B, L, H, d), q, "self_attention")
    _drop_gn_partials(out)
    os_, _ = _blhd_strides(out, "blc")
    rc = _lib.load_library().dsc_self_attn_fwd(
        ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(v.data_ptr()),
        ctypes.c_void_p(out.data_ptr()), B, H, L, S, d, _i64x3(*qs), _i64x3(*ks), _i64x3(*vs), _i64x3(*os_),
        float(scale) if scale else 0.0, 0, _stream_ptr(q))
    _lib.check(rc, "dsc_self_attn_fwd")
    return out


CAUSAL_ATTN_HEAD_DIM = 64      # DSC_CAUSAL_ATTN_HEAD_DIM (include/dsc_hip.h): CLIP-L, OpenCLIP-H and bigG
CAUSAL_ATTN_MAX_TOKENS = 80    # DSC_CAUSAL_ATTN_MAX_TOKENS: five 16-row MFMA tiles (one 77-token chunk)
ACT_KINDS = {"quick_gelu": 0, "gelu": 1}    # DSC_ACT_QUICK_GELU / DSC_ACT_GELU_ERF


def causal_attn_takes(dtype, S, d):
    """dsc_causal_attn_f16's limits (stated in include/dsc_hip.h): fp16, head dim 64, 1..80 tokens"""
    return dtype == torch.float16 and d == CAUSAL_ATTN_HEAD_DIM and 1 <= S <= CAUSAL_ATTN_MAX_TOKENS


def causal_attn(q, k, v, scale=None, into=None):
    """softmax_{j <= i}(q_i.k_j * scale) . v for q / k / v [B, S, H, d] (strided views allowed, e.g. of one fused QKV
    projection) -> [B, S, H, d] (dsc_causal_attn_f16: the CLIP text encoder's attention).  `into`: the destination, a
    [B, S, H, d] fp16 tensor or strided view (unit inner stride, strides in 8s); a new contiguous tensor by default.  (Not
    `out`: tests/test_output_paths.py keeps a closed table of the ops with that parameter; the contract it checks - sums a
    producer attached to the destination are dropped - holds here and is checked in tests/test_clip_text_gpu.py.)"""
    _require_gpu(q, k, v)
    if q.dtype != torch.float16 or k.dtype != torch.float16 or v.dtype != torch.float16:
        raise TypeError("causal_attn: fp16 only")
    qs, (B, H, S, d) = _blhd_strides(q, "blc")
    ks, kshape = _blhd_strides(k, "blc")
    vs, vshape = _blhd_strides(v, "blc")
    if kshape != (B, H, S, d) or vshape != (B, H, S, d):
        raise ValueError(f"causal_attn: q {tuple(q.shape)}, k {tuple(k.shape)} and v {tuple(v.shape)} must have one shape")
    if into is None:
        into = torch.empty((B, S, H, d), dtype=q.dtype, device=q.device)
    _check_out(into, (B, S, H, d), q, "causal_attn")
    _drop_gn_partials(into)
    os_, _ = _blhd_strides(into, "blc")
    rc = _lib.load_library().dsc_causal_attn_f16(_p(q), _p(k), _p(v), _p(into), B, H, S, d, _i64x3(*qs), _i64x3(*ks), _i64x3(*vs),
                                                 _i64x3(*os_), float(scale) if scale else 0.0, 0, _stream_ptr(q))
    _lib.check(rc, "dsc_causal_attn_f16")
    return into


def act_(x, kind):
    """x <- quick_gelu(x) / gelu(x) in place (dsc_act_f16); x fp16 contiguous with numel % 8 == 0; kind: a key of ACT_KINDS"""
    _require_gpu(x)
    if kind not in ACT_KINDS:
        raise ValueError(f"act_: kind must be one of {sorted(ACT_KINDS)}")
    if x.dtype != torch.float16 or not x.is_contiguous():
        raise TypeError("act_: a contiguous fp16 tensor")
    _drop_gn_partials(x)
    rc = _lib.load_library().dsc_act_f16(_p(x), x.numel(), ACT_KINDS[kind], 0, _stream_ptr(x))
    _lib.check(rc, "dsc_act_f16")
    return x


IP_MAX_TOKENS = 16         # DSC_IP_MAX_TOKENS (include/dsc_hip.h): the image tokens of one adapter are one MFMA tile


def ip_xattn_add(q4, k_ip, v_ip, row_scale, io, scale=None, q_weight=None):
    """io[b, l, h, :] += row_scale[b] * softmax(scale * q4[b, l, h, :] . k_ip[b, :, h, :]^T) . v_ip[b, :, h, :], in place
    (dsc_ip_xattn_add_f16: the IP-Adapter term of a cross-attention layer with one scale per batch row, read on the device).
    q4 [B, L, H, d] fp16 with its strides (a stride-0 batch dimension included), k_ip / v_ip [B, T, H, d] fp16 with contiguous
    batch rows and one common batch stride (views into a buffer with one row per batch row),
    row_scale [B] fp32 on the device, io [B, L, H * d] (or [B, L, H, d]) fp16 contiguous: the text branch's output.  Rows whose
    scale is 0 are left untouched and their k_ip / v_ip rows are not read.  scale: default 1 / sqrt(d).  q_weight: [B, L] fp16
    with unit inner stride (a batch stride is allowed), one weight per query multiplied into the term - the down-sampled
    IP-Adapter region mask (dsc_ip_xattn_add_masked_f16): queries with weight 0 are not written and 16-query tiles of zeros are
    not read; a weight of 1 gives the bits of the call without weights.  Returns io."""
    _require_gpu(q4, k_ip, v_ip, row_scale, io)
    if q4.dtype != torch.float16 or k_ip.dtype != torch.float16 or v_ip.dtype != torch.float16 or io.dtype != torch.float16:
        raise TypeError("ip_xattn_add: q4 / k_ip / v_ip / io must be fp16")
    if q4.dim() != 4 or k_ip.dim() != 4:
        raise ValueError(f"ip_xattn_add: q4 is [B, L, H, d] and k_ip / v_ip [B, T, H, d], got {tuple(q4.shape)} / {tuple(k_ip.shape)}")
    (sb, sl, sh), (B, H, L, d) = _blhd_strides(q4, "blc")
    T = k_ip.shape[1]
    if not attn_head_dim_ok(d):
        raise ValueError(f"ip_xattn_add: head dim {d} is not a multiple of 8 in [8, {ATTN_MAX_HEAD_DIM}]")
    if not 1 <= T <= IP_MAX_TOKENS:
        raise ValueError(f"ip_xattn_add: {T} image tokens; the kernel takes 1 .. {IP_MAX_TOKENS} (IP_MAX_TOKENS)")
    skb = k_ip.stride(0) if B > 1 else T * H * d
    want = (k_ip.stride(0), H * d, d, 1)
    if tuple(k_ip.shape) != (B, T, H, d) or tuple(v_ip.shape) != (B, T, H, d) or k_ip.stride() != want or v_ip.stride() != want \
            or skb < T * H * d:
        raise ValueError(f"ip_xattn_add: k_ip / v_ip must be {(B, T, H, d)} tensors with contiguous batch rows and the same batch "
                         f"stride, got {tuple(k_ip.shape)} {k_ip.stride()} / {tuple(v_ip.shape)} {v_ip.stride()}")
    if row_scale.dtype != torch.float32 or tuple(row_scale.shape) != (B,) or not row_scale.is_contiguous():
        raise ValueError(f"ip_xattn_add: row_scale must be a contiguous fp32 [{B}] tensor, got {row_scale.dtype} "
                         f"{tuple(row_scale.shape)}")
    if io.numel() != B * L * H * d or tuple(io.shape[:2]) != (B, L) or not io.is_contiguous():
        raise ValueError(f"ip_xattn_add: io must be a contiguous {(B, L, H * d)} tensor, got {tuple(io.shape)}")
    if any(t.device != q4.device for t in (k_ip, v_ip, row_scale, io)):
        raise ValueError("ip_xattn_add: all operands must be on one device")
    if sb % 8 or sl % 8 or sh % 8 or skb % 8 or any(t.data_ptr() % 16 for t in (q4, k_ip, v_ip, io)):
        raise ValueError("ip_xattn_add: q4's strides must be multiples of 8 elements and every tensor 16-byte aligned")
    sc = float(scale) if scale else float(d) ** -0.5
    if q_weight is not None:
        if not torch.is_tensor(q_weight) or q_weight.dtype != torch.float16 or tuple(q_weight.shape) != (B, L) \
                or q_weight.stride(1) != 1:
            got = f"{q_weight.dtype} {tuple(q_weight.shape)} {q_weight.stride()}" if torch.is_tensor(q_weight) else type(q_weight).__name__
            raise ValueError(f"ip_xattn_add: q_weight must be an fp16 [{B}, {L}] tensor with unit inner stride, got {got}")
        if q_weight.device != q4.device:
            raise ValueError("ip_xattn_add: all operands must be on one device")
        swb = q_weight.stride(0) if B > 1 else L
        if swb < L:
            raise ValueError(f"ip_xattn_add: q_weight's batch stride {swb} is below its row length {L} (rows would overlap)")
        _drop_gn_partials(io)
        rc = _lib.load_library().dsc_ip_xattn_add_masked_f16(_p(q4), sb, sl, sh, _p(k_ip), _p(v_ip), skb, _p(row_scale), _p(io),
                                                             _p(q_weight), swb, B, L, H, d, T, sc, _stream_ptr(q4))
        _lib.check(rc, "dsc_ip_xattn_add_masked_f16")
        return io
    _drop_gn_partials(io)
    rc = _lib.load_library().dsc_ip_xattn_add_f16(_p(q4), sb, sl, sh, _p(k_ip), _p(v_ip), skb, _p(row_scale), _p(io), B, L,
                                                  H, d, T, sc, _stream_ptr(q4))
    _lib.check(rc, "dsc_ip_xattn_add_f16")
    return io


def groupnorm_silu(x, groups, weight, bias, eps, act):
    """GroupNorm(groups, eps) [+ SiLU] over NCHW fp16 [B, C, h, w] (dsc_groupnorm_silu: two HIP launches)."""
    _require_gpu(x)
    lib = _lib.load_library()
    if x.dtype != torch.float16:
        raise TypeError("groupnorm_silu: fp16 only")
    x = x.contiguous()
    B, C = x.shape[0], x.shape[1]
    hw = x.numel() // (B * C)
    y = torch.empty_like(x)
    ws = _workspace(x.device, lib.dsc_groupnorm_workspace_bytes(B, C, hw, groups))
    rc = lib.dsc_groupnorm_silu(_p(x), _p(y), _p(weight), _p(bias), B, C, hw, groups, float(eps), 1 if act else 0, 0,
                                _p(ws), ws.numel() * 8, _stream_ptr(x))
    _lib.check(rc, "dsc_groupnorm_silu")
    return y


def groupnorm_silu_nhwc(x, groups, weight, bias, eps, act, add=None):
    """GroupNorm(groups, eps) [+ SiLU] over channels-last fp16 (dsc_groupnorm_silu_nhwc).

    x: a channels_last [B, C, h, w] tensor (returned likewise) or token-major [B, hw, C].  add: optional [B, C] added
    to x first (the ResNet block's time-embedding term)."""
    _require_gpu(x)
    lib = _lib.load_library()
    if x.dtype != torch.float16:
        raise TypeError("groupnorm_silu_nhwc: fp16 only")
    if x.dim() == 4:
        if not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        B, C, h, w = x.shape
        hw = h * w
        y = torch.empty_like(x, memory_format=torch.channels_last)
    else:
        x = x.contiguous()
        B, hw, C = x.shape
        y = torch.empty_like(x)
    add_stride = 0
    if add is not None:
        if add.stride(-1) != 1 or add.stride(0) % 8 != 0 or add.data_ptr() % 16 != 0:
            add = add.contiguous()
        add_stride = add.stride(0)
    ws = _workspace(x.device, lib.dsc_groupnorm_nhwc_workspace_bytes(B, C, hw, groups))
    rc = lib.dsc_groupnorm_silu_nhwc(_p(x), _p(y), _p(weight), _p(bias), _p(add), add_stride, B, C, hw, groups, float(eps),
                                     1 if act else 0, 0, _p(ws), ws.numel() * 8, _stream_ptr(x))
    _lib.check(rc, "dsc_groupnorm_silu_nhwc")
    return y


GN_CHECK = os.environ.get("DSC_GN_CHECK", "0") != "0"      # debug: verify a producer's partial sums against the tensor before use
USE_GN_FUSE = os.environ.get("DSC_GN_FUSE", "1") != "0"   # GroupNorm statistics from the producing convolution / GEMM epilogue (gn_partials.h)


class GnPartials:
    """the GroupNorm partial sums a producer emitted for the tensor it wrote (dsc_conv3x3_gn_nhwc_f16 / dsc_linear_gn_f16):
    buffer fp32 [B, rows, groups, 2, 2], for a tensor of C channels normalised in `groups` groups"""
    __slots__ = ("buf", "rows", "groups", "C", "B", "hw", "version")

    def __init__(self, buf, rows, groups, C, B, hw):
        self.buf, self.rows, self.groups, self.C, self.B, self.hw = buf, rows, groups, C, B, hw
        self.version = None                   # torch's in-place version counter of the tensor when the sums were attached


def attach_gn_partials(t, part):
    """hand a producer's partial sums on with the tensor OBJECT `t` (a view of the producer's output is fine: same bytes).

    CONTRACT: the sums are invalidated through torch's `_version` counter only, and this package's own kernels write through raw
    pointers (ctypes), which does not bump it - so NO dsc_* call may write in place into (or take as `out=`) a tensor that carries
    partials.  The ops of this module that accept `out=` or write in place drop the attribute from their destination
    (`_drop_gn_partials`); `DSC_GN_CHECK=1` makes `groupnorm_apply_nhwc` recompute the statistics from the tensor and compare."""
    if part is not None:
        part.version = t._version
        t._dsc_gn = part
    return t


def _drop_gn_partials(t):
    """a dsc_* kernel is about to write into `t` through its raw pointer: sums a producer attached to it no longer describe it"""
    if t is not None and getattr(t, "_dsc_gn", None) is not None:
        t._dsc_gn = None
    return t


def gn_partials_of(t):
    """the GnPartials a producer attached to the tensor OBJECT it returned (views and copies carry none), or None - also None once
    the tensor has been written in place since (torch's version counter): the sums would describe other bytes"""
    part = getattr(t, "_dsc_gn", None) if USE_GN_FUSE else None
    if part is not None and part.version != t._version:
        return None
    return part


def groupnorm_apply_nhwc(x, part, groups, weight, bias, eps, act):
    """GroupNorm [+ SiLU] in ONE launch from the producer's partial sums (dsc_groupnorm_apply_nhwc); x channels_last [B,C,h,w]"""
    _require_gpu(x)
    B, C, h, w = x.shape
    if part.groups != groups or part.C != C or part.B != B or part.hw != h * w or not x.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("groupnorm_apply_nhwc: the partial sums do not belong to this tensor / grouping")
    if GN_CHECK:                               # debug: the producer's sums against statistics recomputed from the tensor itself
        cpg = C // groups
        pv = part.buf.view(B, part.rows, groups, 2, 2).double()
        straddles = torch.tensor([(g * cpg) // 64 != ((g + 1) * cpg - 1) // 64 for g in range(groups)], device=x.device)
        sums = pv[:, :, :, 0, 0].sum(1) + torch.where(straddles, pv[:, :, :, 1, 0].sum(1), torch.zeros((), dtype=pv.dtype, device=x.device))
        ref = x.double().reshape(B, groups, C // groups, h * w).sum(dim=(2, 3))
        if not torch.allclose(sums, ref, rtol=1e-3, atol=1e-2 * (C // groups) * h * w ** 0.5):
            raise RuntimeError("groupnorm_apply_nhwc: stale GroupNorm partial sums (the tensor was written after its producer)")
    y = torch.empty_like(x, memory_format=torch.channels_last)
    rc = _lib.load_library().dsc_groupnorm_apply_nhwc(_p(x), _p(y), _p(weight), _p(bias), _p(part.buf), part.rows, B, C, h * w,
                                                      groups, float(eps), 1 if act else 0, 0, _stream_ptr(x))
    _lib.check(rc, "dsc_groupnorm_apply_nhwc")
    return y


def conv3x3_gn_rows(x, weight, groups, upsample=False, upsample_size=None):
    """pixel tiles per image when dsc_conv3x3_gn_nhwc_f16 covers this convolution (and GroupNorm grouping of its output), else 0;
    upsample_size as in conv3x3"""
    geom = _conv3x3_geometry(x, upsample, upsample_size)
    if not (USE_GN_FUSE and _conv3x3_covered(x, weight, geom)):
        return 0
    mode, (H, W), _ = geom
    return int(_lib.load_library().dsc_conv3x3_gn_rows(x.shape[0], H, W, x.shape[1], weight.shape[0], groups, mode))


def conv3x3_gn(x, weight, groups, bias=None, add=None, residual=None, upsample=False, upsample_size=None):
    """conv3x3 (+ bias) (+ per-image bias row add [B, Cout]) (+ residual), channels_last; the returned tensor carries the
    GroupNorm partial sums of what was stored (gn_partials_of) - call only when conv3x3_gn_rows() > 0"""
    mode, (H, W), _ = _conv3x3_geometry(x, upsample, upsample_size)
    _require_gpu(x, weight)
    lib = _lib.load_library()
    B, Cin, Cout = x.shape[0], x.shape[1], weight.shape[0]
    rows = int(lib.dsc_conv3x3_gn_rows(B, H, W, Cin, Cout, groups, mode))
    if rows <= 0:
        raise ValueError("conv3x3_gn: shape not covered (ask conv3x3_gn_rows first)")
    x, weight, residual, ldr = _conv3x3_operands("conv3x3_gn", x, weight, residual, (B, Cout, H, W))
    out = torch.empty((B, Cout, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    add_ld = 0
    if add is not None:
        if add.stride(-1) != 1 or add.stride(0) % 8 != 0 or add.data_ptr() % 16 != 0:
            add = add.contiguous()
        add_ld = add.stride(0)
    part = torch.empty((B, rows, groups, 2, 2), dtype=torch.float32, device=x.device)
    rc = lib.dsc_conv3x3_gn_nhwc_f16(_p(x), _p(weight), _p(bias), _p(add), add_ld, _p(residual), _p(out), B, H, W, Cin, Cout, Cin,
                                     ldr, Cout, mode, _p(part), groups, 0, _stream_ptr(x))
    _lib.check(rc, "dsc_conv3x3_gn_nhwc_f16")
    return attach_gn_partials(out, GnPartials(part, rows, groups, Cout, B, H * W))


def linear_gn(x, weight, bias, residual, rows_per_image, groups):
    """x [B, L, K] @ weight.T (+ bias) (+ residual) -> [B, L, N] with the GroupNorm partial sums of the result (a 1x1 convolution
    in token-major form: proj_out, conv_shortcut), or None when dsc_linear_gn_f16 does not cover the shape"""
    got = USE_GN_FUSE and x.is_cuda and x.dim() == 3 and x.shape[1] == rows_per_image and _gemm_operands(x, weight, bias, residual)
    if not got:
        return None
    x2, r2, ldr = got
    lib = _lib.load_library()
    B, L, K = x.shape
    N = weight.shape[0]
    M = B * L
    rows = int(lib.dsc_linear_gn_rows(M, N, K, rows_per_image, groups))
    if rows <= 0:
        return None
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    part = torch.empty((B, rows, groups, 2, 2), dtype=torch.float32, device=x.device)
    rc = lib.dsc_linear_gn_f16(_p(x2), _p(weight), _p(bias), _p(r2), _p(out), M, N, K, x2.stride(0),
                               ldr, N, rows_per_image, _p(part), groups, 0, _stream_ptr(x))
    _lib.check(rc, "dsc_linear_gn_f16")
    return out.reshape(B, L, N), GnPartials(part, rows, groups, N, B, L)


USE_RESIDUAL_WRAP = os.environ.get("DSC_RESIDUAL_WRAP", "1") != "0"   # (A/B switch: 0 = repeat a shorter residual on the host, as before)


def _residual_wraps(R):
    """the GEMM kernels add residual row m % R to row m themselves when R is a multiple of their 128-row tile"""
    return USE_RESIDUAL_WRAP and R % 128 == 0


def residual_for_batch(residual, batch):
    """the [b, L, N] residual stream of a GEMM whose result has `batch` = k b images (shared CFG prefix: the stream was computed
    once per image): itself where the kernels wrap its rows, else repeated k times"""
    b, L = residual.shape[:2]
    return residual if b == batch or _residual_wraps(b * L) else residual.repeat(batch // b, 1, 1)


def _residual_2d(residual, M, N):
    """(r2, ldr) for the GEMM entry points: the residual as [R, N] rows and its row stride, with R << 32 in the stride's high bits
    when it has fewer rows than the result (include/dsc_hip.h, dsc_linear_f16); None when the kernels do not take the shape."""
    R = residual.numel() // N
    if R * N != residual.numel() or R <= 0 or M % R != 0 or not (R == M or _residual_wraps(R)):
        return None
    r2 = residual.reshape(R, N)
    if r2.stride(1) != 1 or r2.stride(0) % 8 != 0 or r2.data_ptr() % 16 != 0:
        return None
    return r2, r2.stride(0) | (R << 32 if R != M else 0)


def _gemm_shape(N, K, dtype, geglu=False):
    """the shapes gemm_tn_f16 is built for: fp16, 64-column tiles, 64-deep K steps, a GEGLU pair in one 64-column tile"""
    return dtype == torch.float16 and K % 64 == 0 and N % 64 == 0 and (not geglu or (N // 2) % 32 == 0)


def _gemm_operands(x, weight, bias=None, residual=None, geglu=False, must=None):
    """(x2, r2, ldr) when the package's GEMM entry points (gemm.hip: dsc_linear_f16 / _ln_f16 / _qkv_f16 / _gn_f16 / _splitk_f16)
    can read these operands, else None - or a ValueError in the name of `must`, an entry point with no other route: fp16 only (the
    C ABI sees no dtypes), _gemm_shape, unit inner strides, row strides in 8s, 16-byte aligned pointers, a contiguous weight, GEGLU
    only with a bias and no residual, the residual as in _residual_2d.  x2 = x as [M, K]: a copy only where x does not collapse.
    An x whose last dimension is not the weight's K is a RuntimeError for every caller, as from the reshape or F.linear before."""
    N, K = weight.shape
    if x.shape[-1] != K:
        raise RuntimeError(f"{must or 'linear'}: x {tuple(x.shape)} does not multiply with weight {tuple(weight.shape)}")
    got, at_fault = None, "x, weight or bias (fp16, K and N in 64s, unit-stride rows in 8s at 16 bytes, GEGLU with a bias)"
    if (_gemm_shape(N, K, x.dtype, geglu) and weight.dtype == torch.float16 and x.stride(-1) == 1 and weight.is_contiguous()
            and (bias is None or (bias.dtype == torch.float16 and bias.data_ptr() % 16 == 0))
            and (not geglu or (bias is not None and residual is None))):
        x2 = x.reshape(math.prod(x.shape[:-1]), K)
        if x2.stride(1) == 1 and x2.stride(0) % 8 == 0 and x2.data_ptr() % 16 == 0:
            got = (None, 0) if residual is None else _residual_2d(residual, x2.shape[0], N)
            got, at_fault = got and (x2, *got), "the residual (M rows, or M / k rows in 128s; unit-stride rows in 8s at 16 bytes)"
    if got is None and must:
        raise ValueError(f"{must}: the GEMM kernels cannot read {at_fault}")
    return got


def linear_kernel_can(x, weight, bias, residual):
    """dsc_linear_f16's operand constraints (_gemm_operands), not its row / K preferences"""
    return _gemm_operands(x, weight, bias, residual) is not None


USE_GN_CAT = os.environ.get("DSC_GN_CAT", "1") != "0"   # up blocks: the skip concatenation is written by the GroupNorm that reads it


def groupnorm_cat_covers(x1, x2):
    """True when dsc_groupnorm_silu_nhwc_cat takes this pair of channels_last [B, C1, h, w] / [B, C2, h, w] tensors"""
    cl = torch.channels_last
    return (USE_GN_CAT and x1.is_cuda and x1.dtype == torch.float16 and x2.dtype == torch.float16 and x1.dim() == 4
            and x2.dim() == 4 and x1.shape[0] == x2.shape[0] and x1.shape[2:] == x2.shape[2:] and x1.shape[1] % 8 == 0
            and x2.shape[1] % 8 == 0 and (x1.shape[1] + x2.shape[1]) // 8 <= 512
            and x1.is_contiguous(memory_format=cl) and x2.is_contiguous(memory_format=cl))


def groupnorm_silu_nhwc_cat(x1, x2, groups, weight, bias, eps, act, add=None):
    """(GroupNorm [+ SiLU] of cat([x1, x2], dim=1), the concatenation itself), both channels_last: the statistics pass reads
    the two sources and writes the concatenation on the way (dsc_groupnorm_silu_nhwc_cat) - no separate cat kernel."""
    _require_gpu(x1, x2)
    if not groupnorm_cat_covers(x1, x2):
        raise ValueError("groupnorm_silu_nhwc_cat: channels_last fp16 [B, C, h, w] pairs with C % 8 == 0 only")
    lib = _lib.load_library()
    B, C1, h, w = x1.shape
    C = C1 + x2.shape[1]
    cat = torch.empty((B, C, h, w), dtype=x1.dtype, device=x1.device, memory_format=torch.channels_last)
    y = torch.empty_like(cat, memory_format=torch.channels_last)
    add_stride = 0
    if add is not None:
        if add.stride(-1) != 1 or add.stride(0) % 8 != 0 or add.data_ptr() % 16 != 0:
            add = add.contiguous()
        add_stride = add.stride(0)
    ws = _workspace(x1.device, lib.dsc_groupnorm_nhwc_workspace_bytes(B, C, h * w, groups))
    rc = lib.dsc_groupnorm_silu_nhwc_cat(_p(x1), _p(x2), C1, _p(cat), _p(y), _p(weight), _p(bias), _p(add), add_stride, B, C,
                                         h * w, groups, float(eps), 1 if act else 0, 0, _p(ws), ws.numel() * 8,
                                         _stream_ptr(x1))
    _lib.check(rc, "dsc_groupnorm_silu_nhwc_cat")
    return y, cat


# Library GEMMs (hipBLASLt through dsc_linear_lt_f16) are OFF by default: every linear of the step runs on the package's own kernels
# (gemm_tn_f16, split-K for the few-row long-K shapes).  Per step that costs ~20 us against the best of both per shape
# (tools/mb_gemm_cold.py) and buys: the same bits in every process, rank and tuning profile (the library's algorithm was timed per
# process and differed per profile), no 0.3 s of algorithm timing at start-up, no stream-K kernels in a step on two streams.
USE_LIBRARY_GEMM = os.environ.get("DSC_LIBRARY_GEMM", "0") != "0"
USE_LT_RESIDUAL = USE_LIBRARY_GEMM and os.environ.get("DSC_LT_RESIDUAL", "1") != "0"   # bias + residual in the library launch (dsc_linear_lt_f16)
USE_LT_ALL = USE_LIBRARY_GEMM and os.environ.get("DSC_LT_ALL", "1") != "0"   # ... and the ones without a residual go the same way
USE_DSC_GEMM = True        # False: no linear reaches dsc_linear_f16 / dsc_linear_splitk_f16 (library, else torch)
USE_LN_FOLD = os.environ.get("DSC_LN_FOLD", "1") != "0"   # BasicTransformerBlock: LayerNorms folded into the GEMMs (dsc_linear_ln_f16)
# The window (_gemm_rows_k_preferred): >= MIN_ROWS rows with K <= MAX_K, MID_ROWS <= rows < MIN_ROWS with K <= MID_K (DSC_GEMM_MID=0
# closes that half), GEGLU with K <= 1280.  Measured against the library (tools/mb_gemm.py: the mid rows a wash per GEMM, QKV 14.0
# vs 15.4 us, C->C 11.8 vs 11.1; GEGLU at M=512 N=10240 K=1280 22.2 vs 23.2 us + the GEGLU launch); with the library on it still
# decides between the two.  With it off (the default) every linear the kernels can read runs on them, inside the window or not,
# and the window decides (_linear_plan): outside it few rows with a long K go to split-K (SPLITK_*) and a residual of fewer rows is
# repeated, inside it (or with prefer_kernel) dsc_linear_f16 wraps those rows; and (linear_kernel_covers) only inside it the
# LayerNorms fold into the GEMMs (three add+LayerNorm launches fewer per block) and K / V leave the QKV GEMM head-major.
DSC_GEMM_MIN_ROWS = 1024
DSC_GEMM_MAX_K = int(os.environ.get("DSC_GEMM_MAX_K", "640"))
DSC_GEMM_MID_ROWS = int(os.environ.get("DSC_GEMM_MID_ROWS", "128")) if os.environ.get("DSC_GEMM_MID", "1") != "0" else 1 << 30
DSC_GEMM_MID_K = int(os.environ.get("DSC_GEMM_MID_K", "1280"))


def _gemm_rows_k_preferred(M, K, geglu=False):
    """the row / K window of the comment above"""
    if M >= DSC_GEMM_MIN_ROWS and K <= DSC_GEMM_MAX_K:
        return True
    if DSC_GEMM_MID_ROWS <= M < DSC_GEMM_MIN_ROWS and K <= DSC_GEMM_MID_K:
        return True
    return bool(geglu) and K <= 1280


def linear_kernel_covers(M, N, K, dtype, geglu=False):
    """True for gemm_tn_f16's shapes inside the window: asked before dsc_linear_ln_f16 / _qkv_f16, which have no other route"""
    return USE_DSC_GEMM and _gemm_shape(N, K, dtype, geglu) and _gemm_rows_k_preferred(M, K, geglu)


def fold_layernorm(weight, bias, gamma, beta):
    """(w', b', cvec) for dsc_linear_ln_f16: LayerNorm(s; gamma, beta) @ weight.T + bias
       == rstd (s @ w'.T - mu cvec) + b'   with w' = weight * gamma, b' = weight @ beta + bias, cvec = w'.sum(1) (fp32, of
    the fp16-rounded w' the kernel multiplies with)."""
    w2 = (weight.float() * gamma.float()[None, :]).to(weight.dtype).contiguous()
    b2 = weight.float() @ beta.float()
    if bias is not None:
        b2 = b2 + bias.float()
    return w2, b2.to(weight.dtype).contiguous(), w2.float().sum(dim=1).contiguous()


def _ln_args(what, ln, M, N):
    """dsc_linear_ln_f16 / _qkv_f16's four LayerNorm arguments from ln = (partials [M, nb, 2] fp32, cvec [N] fp32, eps) or None"""
    if ln is None:
        return None, 0, None, 0.0
    part, cvec, eps = ln
    if part.shape[0] != M or part.dtype != torch.float32 or not part.is_contiguous() or cvec.numel() != N:
        raise ValueError(f"{what}: statistics / cvec do not match the operands")
    return _p(part), part.shape[1], _p(cvec), float(eps)


def linear_ln(x, weight, bias, *, residual=None, geglu=False, ln=None, ln_stats=False):
    """dsc_linear_ln_f16 (no library fallback: call only when linear_kernel_covers() says so).
    ln = (partials [M, nb, 2] fp32, cvec [N] fp32, eps): x is the un-normalised stream, weight / bias come from
    fold_layernorm().  ln_stats=True additionally returns the [M, N/64, 2] row partials of the output."""
    _require_gpu(x, weight)
    x2, r2, ldr = _gemm_operands(x, weight, bias, residual, geglu, must="linear_ln")
    N, K = weight.shape
    M = x2.shape[0]
    n_out = N // 2 if geglu else N
    out = torch.empty((M, n_out), dtype=x.dtype, device=x.device)
    stats = torch.empty((M, N // 64, 2), dtype=torch.float32, device=x.device) if ln_stats else None
    rc = _lib.load_library().dsc_linear_ln_f16(_p(x2), _p(weight), _p(bias), _p(r2), _p(out), M, N, K, x2.stride(0), ldr, n_out,
                                               1 if geglu else 0, *_ln_args("linear_ln", ln, M, N), _p(stats), 0, _stream_ptr(x))
    _lib.check(rc, "dsc_linear_ln_f16")
    out = out.reshape(*x.shape[:-1], n_out)
    return (out, stats) if ln_stats else out


USE_QKV_HEAD_MAJOR = os.environ.get("DSC_QKV_HEAD_MAJOR", "1") != "0"


def linear_qkv_covers(x, weight, heads):
    """True when dsc_linear_qkv_f16 takes the fused self-attention projection of x [B, L, K] by weight [3C, K]"""
    C = weight.shape[0] // 3
    return (USE_QKV_HEAD_MAJOR and x.dim() == 3 and weight.dtype == torch.float16 and weight.shape[0] == 3 * C and C % heads == 0
            and (C // heads) % 8 == 0 and linear_kernel_covers(x.shape[0] * x.shape[1], 3 * C, x.shape[2], x.dtype)
            and x.stride(-1) == 1 and weight.is_contiguous())


def linear_qkv(x, weight, bias, heads, ln=None):
    """The self-attention q / k / v projection as one GEMM with the head split of K and V done by its epilogue
    (dsc_linear_qkv_f16): x [B, L, K], weight [3C, K] -> (q4, k4, v4), each a [B, L, heads, d] VIEW: q4 of a [B, L, C]
    tensor, k4 / v4 of a head-major [2, B, heads, L, d] one (a head's keys / values contiguous).  ln as in linear_ln."""
    _require_gpu(x, weight)
    B, L, K = x.shape
    C = weight.shape[0] // 3
    d = C // heads
    M = B * L
    x2 = _gemm_operands(x, weight, bias, must="linear_qkv")[0]
    q = torch.empty((B, L, C), dtype=x.dtype, device=x.device)
    kv = torch.empty((2, B, heads, L, d), dtype=x.dtype, device=x.device)
    rc = _lib.load_library().dsc_linear_qkv_f16(_p(x2), _p(weight), _p(bias), _p(q), _p(kv), M, C, K, x2.stride(0), C, heads, L,
                                                *_ln_args("linear_qkv", ln, M, 3 * C), 0, _stream_ptr(x))
    _lib.check(rc, "dsc_linear_qkv_f16")
    return q.view(B, L, heads, d), kv[0].permute(0, 2, 1, 3), kv[1].permute(0, 2, 1, 3)


USE_SPLITK = os.environ.get("DSC_GEMM_SPLITK", "1") != "0"    # few-row long-K GEMMs on dsc_linear_splitk_f16 instead of the library
SPLITK_MAX_ROWS = int(os.environ.get("DSC_SPLITK_MAX_ROWS", "512"))
SPLITK_MIN_K = int(os.environ.get("DSC_SPLITK_MIN_K", "1920"))


def linear_splitk(x2, weight, bias, r2, splits=0):
    """dsc_linear_splitk_f16 on 2-D operands (x2 [M, K], weight [N, K] contiguous, r2 [M, N] or None) -> [M, N]"""
    lib = _lib.load_library()
    M, K = x2.shape
    N = weight.shape[0]
    out = torch.empty((M, N), dtype=x2.dtype, device=x2.device)
    nbytes = lib.dsc_linear_splitk_workspace_bytes(M, N, K, splits)
    ws = _workspace(x2.device, nbytes) if nbytes else None
    rc = lib.dsc_linear_splitk_f16(_p(x2), _p(weight), _p(bias), _p(r2), _p(out), M, N, K, x2.stride(0),
                                   r2.stride(0) if r2 is not None else 0, N, splits, _p(ws), ws.numel() * 8 if ws is not None else 0,
                                   0, _stream_ptr(x2))
    _lib.check(rc, "dsc_linear_splitk_f16")
    return out


# _linear_plan's routes: dsc_linear_f16 (epilogue fused, fewer residual rows wrapped); dsc_linear_splitk_f16 (epilogue in its reduce
# launch); dsc_linear_lt_f16 (hipBLASLt: bias epilogue, residual as beta * C; it may decline); F.linear, then the epilogue as separate ops
LINEAR_KERNEL, LINEAR_SPLITK, LINEAR_LIBRARY, LINEAR_TORCH = range(4)


def _linear_plan(x, weight, bias, residual, geglu, prefer_kernel):
    """Where ops.linear sends these operands, from shapes, strides, dtypes, pointers and the module's switches alone (no launch;
    the only allocations are the [M, K] form of an x and, for the library, the [M, N] form of a residual whose leading dimensions
    do not collapse) -> (route, fallback, x2, r2, ldr, repeat): a LINEAR_* route and the one to take if LINEAR_LIBRARY declines; x
    as [M, K] and the residual as rows with their stride (_residual_2d), None / 0 where no entry point reads them; repeat = k:
    first repeat the residual's M / k rows k times."""
    N, K = weight.shape
    M = math.prod(x.shape[:-1])
    inside = prefer_kernel or _gemm_rows_k_preferred(M, K, geglu)
    x2, r2, ldr = (USE_DSC_GEMM and _gemm_operands(x, weight, bias, None, geglu)) or (None, None, 0)
    can, repeat = x2 is not None, None            # the package's kernels can read x, weight and bias ...
    if residual is not None:
        rows = _residual_2d(residual, M, N) if can else None
        if residual.numel() != M * N and (rows is None or not inside):
            # fewer rows (shared CFG prefix), not wrapped: outside the window even where dsc_linear_f16 then runs (2048 rows, K = 1280)
            repeat = M // (residual.numel() // N)
        else:
            can = rows is not None                # ... and the residual
            r2, ldr = rows or (None, 0)
    # outside the window the kernel still takes what it can read: no GEMM of the step reaches a library algorithm nobody vetted
    route = fallback = LINEAR_KERNEL if can else LINEAR_TORCH
    if can and inside:
        return route, fallback, x2, r2, ldr, repeat
    if can and not geglu and USE_SPLITK and not USE_LIBRARY_GEMM and M <= SPLITK_MAX_ROWS and K >= SPLITK_MIN_K:
        # few rows, long K (the 16x16 / 8x8 levels' feed-forward output projections and shortcut 1x1s): weight-streaming bound, split
        # over K + an ordered reduce launch; measured against the library per shape in the step's cache state (tools/mb_gemm_cold.py)
        route = LINEAR_SPLITK
    elif (USE_LT_RESIDUAL if residual is not None else USE_LT_ALL) and x.dtype == torch.float16 and K % 8 == 0 and N % 8 == 0 and M >= 8:
        if not can:                               # the library asks less of its operands than the kernels: no 64s, no pointers
            x2 = x.reshape(M, K) if x2 is None else x2
            if residual is not None and repeat is None:
                r2 = residual.reshape(M, N)       # (a copy where the residual's leading dimensions do not collapse)
                ldr = r2.stride(0)
        if (x2.stride(1) == 1 and x2.stride(0) % 8 == 0 and weight.is_contiguous() and weight.dtype == torch.float16
                and (bias is None or bias.dtype == torch.float16) and (r2 is None or (r2.stride(1) == 1 and ldr % 8 == 0))):
            route = LINEAR_LIBRARY
    return route, fallback, x2, r2, ldr, repeat


def _unfused_epilogue(y, residual, gated):
    """what dsc_linear_f16 fuses, after a GEMM that has no such epilogue"""
    return geglu(y) if gated else y if residual is None else y + residual


def linear(x, weight, bias=None, residual=None, geglu=False, prefer_kernel=False):
    """x @ weight.T (+ bias) (+ residual), or the fused GEGLU of [x @ weight.T + bias]; x [..., K], weight [N, K].
    prefer_kernel: as if the shape lay inside the row / K window (DSC_GEMM_*).
    Every linear the package's kernels can read (_gemm_operands: fp16, K and N multiples of 64, aligned unit-stride rows) runs on
    dsc_linear_f16 with the epilogue fused, or outside the window, with few rows and a long K, on split-K; DSC_LIBRARY_GEMM=1
    sends those outside the window to dsc_linear_lt_f16 first.  What no entry point can read is F.linear and separate ops."""
    if geglu and residual is not None:
        raise ValueError("linear: the GEGLU epilogue takes no residual")
    _require_gpu(x, weight)
    route, fallback, x2, r2, ldr, repeat = _linear_plan(x, weight, bias, residual, geglu, prefer_kernel)
    N, K = weight.shape
    lead = x.shape[:-1]
    M = math.prod(lead)
    if repeat is not None:
        residual = residual.reshape(-1, N).repeat(repeat, 1).reshape(*lead, N)
        r2, ldr = residual.reshape(M, N), N
    if route == LINEAR_LIBRARY:
        # one launch instead of GEMM + add, by the fastest of the heuristic's candidates, timed on a shape's first call (linear_lt.hip)
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
        rc = _lib.load_library().dsc_linear_lt_f16(_p(x2), _p(weight), _p(bias), _p(r2), _p(out), M, N, K, x2.stride(0), ldr, N, 0,
                                                   _stream_ptr(x))
        if rc == 0:
            return _unfused_epilogue(out.reshape(*lead, N), None, geglu)
        route = fallback
    if route == LINEAR_TORCH:
        return _unfused_epilogue(torch.nn.functional.linear(x, weight, bias), residual, geglu)
    if route == LINEAR_SPLITK:
        return linear_splitk(x2, weight, bias, r2).reshape(*lead, N)
    n_out = N // 2 if geglu else N
    out = torch.empty((M, n_out), dtype=x.dtype, device=x.device)
    rc = _lib.load_library().dsc_linear_f16(_p(x2), _p(weight), _p(bias), _p(r2), _p(out), M, N, K, x2.stride(0), ldr, n_out,
                                            1 if geglu else 0, 0, _stream_ptr(x))
    _lib.check(rc, "dsc_linear_f16")
    return out.reshape(*lead, n_out)


USE_DSC_CONV = True        # route qualifying 3x3 convolutions to dsc_conv3x3_nhwc_f16 (False: always MIOpen through torch)


# the `resample` codes of dsc_conv3x3_nhwc_f16 / dsc_conv3x3_gn_* (DSC_CONV_* of include/dsc_hip.h, which has no name for 0)
CONV_PLAIN = 0
CONV_UPSAMPLE2X = 1           # the convolution of the 2x nearest-neighbour upsampling of x
CONV_STRIDE2 = 2              # stride 2 / pad 1: ceil(n / 2) pixels per side
CONV_STRIDE2_PAD_BR = 3       # stride 2 / zero padding on the bottom and right only; even sides
CONV_UPSAMPLE_SIZE = 4        # DSC_CONV_UPSAMPLE_CEIL: of x upsampled to a given size, each side 2s or 2s-1


_CONV_MODE_KEYWORD = {CONV_PLAIN: None, CONV_UPSAMPLE2X: "upsample", CONV_STRIDE2: "stride2_ceil", CONV_STRIDE2_PAD_BR: "stride2_pad_br",
                      CONV_UPSAMPLE_SIZE: "upsample_size"}      # conv3x3's keyword of each code


def _conv3x3_geometry(x, upsample=False, upsample_size=None, stride2=False, stride2_ceil=False, stride2_pad_br=False):
    """(mode, (H, W), (oh, ow)) of a conv3x3 call: the CONV_* code, the image the nine taps run over and the image that is stored.
    Every ValueError of the conv3x3 family for its mode keywords is raised here, from the arguments alone."""
    if sum(map(bool, (upsample, upsample_size is not None, stride2 or stride2_ceil, stride2_pad_br))) > 1:
        raise ValueError("conv3x3: upsample, upsample_size, stride2 / stride2_ceil and stride2_pad_br exclude each other")
    # (a tensor that is no [B, C, H, W] image: conv3x3_supported says False, conv3x3 fails on its shape)
    H, W = (int(x.shape[2]), int(x.shape[3])) if x.dim() == 4 else (0, 0)
    if upsample_size is not None:
        if x.dim() != 4 or len(upsample_size) != 2:
            raise ValueError("conv3x3: upsample_size is the (H, W) of the upsampled [B, C, H, W] image")
        size = (int(upsample_size[0]), int(upsample_size[1]))
        for t, s in zip(size, (H, W)):
            # the only targets whose nearest-neighbour source index is dst >> 1 (and the only ones a UNet skip tensor demands)
            if t not in (2 * s, 2 * s - 1) or t < 1:
                raise ValueError(f"conv3x3: upsample_size {size} is not 2s or 2s-1 of the source sides {(H, W)}")
        return CONV_UPSAMPLE_SIZE, size, size
    if stride2 and (H % 2 or W % 2):
        raise ValueError("conv3x3: stride2=True keeps its even-sides rule; stride2_ceil=True takes any side")
    if upsample:
        return CONV_UPSAMPLE2X, (2 * H, 2 * W), (2 * H, 2 * W)
    if stride2 or stride2_ceil:
        return CONV_STRIDE2, (H, W), ((H + 1) // 2, (W + 1) // 2)
    if stride2_pad_br:
        return CONV_STRIDE2_PAD_BR, (H, W), (H // 2, W // 2)
    return CONV_PLAIN, (H, W), (H, W)


def _conv3x3_covered(x, weight, geom):
    """True when dsc_conv3x3_nhwc_f16 covers the convolution of this geometry: routing switch, device, dtypes, shapes, the kernel's plan"""
    if not (USE_DSC_CONV and x.is_cuda and x.dtype == torch.float16 and weight.dtype == torch.float16 and x.dim() == 4
            and tuple(weight.shape[2:]) == (3, 3) and weight.shape[1] == x.shape[1]):
        return False
    _, (H, W), _ = geom
    return bool(_lib.load_library().dsc_conv3x3_supported(x.shape[0], H, W, x.shape[1], weight.shape[0]))


def _conv3x3_operands(what, x, weight, residual, out_shape):
    """x, weight and residual in channels_last memory (weight / residual may be None) and the residual's pixel stride; ValueError
    for a residual that has not the output's shape"""
    if residual is not None and tuple(residual.shape) != tuple(out_shape):
        raise ValueError(f"{what}: residual must have the output's shape")
    cl = torch.channels_last
    x, weight, residual = (t if t is None or t.is_contiguous(memory_format=cl) else t.contiguous(memory_format=cl)
                           for t in (x, weight, residual))
    return x, weight, residual, 0 if residual is None else out_shape[1]


def conv3x3_supported(x, weight, upsample=False, upsample_size=None):
    """True when dsc_conv3x3_nhwc_f16 covers this [B, Cin, H, W] channels_last fp16 input / [Cout, Cin, 3, 3] weight
    (upsample: the convolution runs on the 2x nearest-upsampled image; upsample_size=(H', W'): on the image upsampled to that
    size, each side 2s or 2s-1 of the source side - ValueError otherwise)."""
    return _conv3x3_covered(x, weight, _conv3x3_geometry(x, upsample, upsample_size))


def conv3x3(x, weight, bias=None, residual=None, splits=0, upsample=False, out_nchw=False, stride2=False, stride2_pad_br=False,
            upsample_size=None, stride2_ceil=False):
    """3x3 / stride 1 / pad 1 convolution (+ bias) (+ residual) of a channels_last fp16 [B, Cin, H, W] tensor with a
    [Cout, Cin, 3, 3] weight held in channels_last memory format (dsc_conv3x3_nhwc_f16); returns channels_last
    [B, Cout, H, W], or a plain contiguous (NCHW) tensor with out_nchw=True (never split).  upsample=True convolves the 2x
    nearest-neighbour upsampling of x (output [B, Cout, 2H, 2W]) without materialising it; upsample_size=(H', W') convolves
    `F.interpolate(x, size=(H', W'), mode="nearest")`, each side 2s or 2s-1 of the source side (the UNet's upsampling to the
    size of a skip tensor; ValueError for any other size); stride2_ceil=True is the stride-2 / pad-1 convolution (output
    [B, Cout, ceil(H/2), ceil(W/2)], any H and W: UNet Downsample2D); stride2=True the same launch behind its older even-sides-only
    rule (ValueError for an odd side: tests/test_unet_pipeline_gpu.py::test_conv3x3_unsupported pins that refusal, so the rule
    stays under this name until that assertion goes); stride2_pad_br=True the stride-2 convolution with zero padding on the bottom / right only
    (`F.pad(x, (0, 1, 0, 1))` + stride-2 / pad-0 conv: AutoencoderKL encoder; H and W even).  Raises on an unsupported shape - ask
    conv3x3_supported() first, or call conv3x3_try()."""
    mode, (H, W), (oh, ow) = _conv3x3_geometry(x, upsample, upsample_size, stride2, stride2_ceil, stride2_pad_br)
    _require_gpu(x, weight)
    lib = _lib.load_library()
    splits = 1 if out_nchw else splits    # as the library does: only the convolution's own epilogue stores channel-major
    B, Cin, _, _ = x.shape
    Cout = weight.shape[0]
    x, weight, residual, ldr = _conv3x3_operands("conv3x3", x, weight, residual, (B, Cout, oh, ow))
    out = torch.empty((B, Cout, oh, ow), dtype=x.dtype, device=x.device,
                      memory_format=torch.contiguous_format if out_nchw else torch.channels_last)
    nbytes = lib.dsc_conv3x3_workspace_bytes(B, H, W, Cin, Cout, splits)
    ws = _workspace(x.device, nbytes) if nbytes else None
    rc = lib.dsc_conv3x3_nhwc_f16(_p(x), _p(weight), _p(bias), _p(residual), _p(out), B, H, W, Cin, Cout, Cin, ldr, Cout,
                                  mode, 1 if out_nchw else 0, splits, 0, _p(ws), ws.numel() * 8 if ws is not None else 0,
                                  _stream_ptr(x))
    _lib.check(rc, "dsc_conv3x3_nhwc_f16")
    return out


def conv3x3_try(x, weight, bias=None, residual=None, *, mode=CONV_PLAIN, size=None, out_nchw=False, splits=0):
    """conv3x3 in the given CONV_* mode (size: the upsample_size of CONV_UPSAMPLE_SIZE) where dsc_conv3x3_nhwc_f16 covers the call,
    else None - a CPU tensor, another dtype, a shape outside the kernel's, USE_DSC_CONV off - and the caller takes its library
    path.  ValueError for bad arguments, as conv3x3.
    (dsc_conv3x3_workspace_bytes cannot double as the coverage answer: its 0 is "not covered" and "no split" alike, and it does not
    apply the 2^30 bounds of dsc_conv3x3_supported - so coverage is asked once, through conv3x3_supported, and nothing is skipped.)"""
    keyword = _CONV_MODE_KEYWORD.get(mode, "") if isinstance(mode, int) else ""
    if keyword == "" or (size is None) == (mode == CONV_UPSAMPLE_SIZE):
        raise ValueError("conv3x3_try: mode is one of ops.CONV_*; size goes with CONV_UPSAMPLE_SIZE, and only with it")
    kw = {} if keyword is None else {keyword: True if size is None else size}
    _, (H, W), _ = _conv3x3_geometry(x, **kw)
    stride2 = mode in (CONV_STRIDE2, CONV_STRIDE2_PAD_BR)
    # two refusals of conv_impl (conv3x3.hip) that dsc_conv3x3_supported, which is not told the mode, cannot give: a stride-2 code
    # with a channel-major output, and odd sides with the bottom / right padding.  conv3x3 leaves both to the library's error.
    if (stride2 and out_nchw) or (mode == CONV_STRIDE2_PAD_BR and (H % 2 or W % 2)):
        return None
    if not conv3x3_supported(x, weight, **({} if stride2 else kw)):
        return None
    return conv3x3(x, weight, bias, residual, splits=splits, out_nchw=out_nchw, **kw)


# Upsample2D (exact 2x): four 2x2 phase convolutions of the source with pre-summed weights (dsc_conv3x3_up2x_nhwc_f16) instead of
# the 3x3 taps over the gathered image.  "0": the gather form, conv3x3(upsample=True) - an A/B switch like DSC_LN_FOLD
USE_UP2X_PHASES = os.environ.get("DSC_UP2X_PHASES", "1") != "0"


def conv3x3_up2x_pack(weight):
    """[Cout, Cin, 3, 3] fp16 conv weight -> the [4, Cout, 4, Cin] fp16 phase weights of conv3x3_up2x (dsc_conv3x3_up2x_pack_f16):
    packed[2*py+px, n, 2*a+b, c] = sum of weight[n, c, dy, dx] over dy in R(py, a), dx in R(px, b), R(0,0) = {0}, R(0,1) = {1, 2},
    R(1,0) = {0, 1}, R(1,1) = {2}; added in fp32 (dy ascending, then dx ascending) and rounded once.  Depends on the weight only."""
    _require_gpu(weight)
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.dtype != torch.float16:
        raise ValueError("conv3x3_up2x_pack: weight must be a [Cout, Cin, 3, 3] fp16 tensor")
    Cout, Cin = weight.shape[:2]
    if Cin % 64 != 0:
        raise ValueError("conv3x3_up2x_pack: Cin must be a multiple of 64")
    cl = torch.channels_last
    if not weight.is_contiguous(memory_format=cl):
        weight = weight.contiguous(memory_format=cl)
    packed = torch.empty((4, Cout, 4, Cin), dtype=torch.float16, device=weight.device)
    rc = _lib.load_library().dsc_conv3x3_up2x_pack_f16(_p(weight), _p(packed), Cin, Cout, _stream_ptr(weight))
    _lib.check(rc, "dsc_conv3x3_up2x_pack_f16")
    return packed


def conv3x3_up2x_supported(x, weight):
    """True when dsc_conv3x3_up2x_nhwc_f16 covers the exact 2x upsampling + 3x3 convolution of this [B, Cin, h, w] channels_last
    fp16 input with this [Cout, Cin, 3, 3] weight (Cin and Cout multiples of 64)"""
    if not (USE_DSC_CONV and x.is_cuda and x.dtype == torch.float16 and weight.dtype == torch.float16 and x.dim() == 4
            and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3) and weight.shape[1] == x.shape[1]):
        return False
    B, C, h, w = x.shape
    return bool(_lib.load_library().dsc_conv3x3_up2x_supported(B, h, w, C, weight.shape[0]))


def conv3x3_up2x(x, packed, bias=None, splits=0):
    """`F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), weight, bias, padding=1)` of a channels_last fp16
    [B, Cin, h, w] tensor as four 2x2 phase convolutions of x itself with packed = conv3x3_up2x_pack(weight); returns channels_last
    [B, Cout, 2h, 2w].  Only the exact 2x target: for the skip-sized 2s-1 targets the last row / column has a tap on the zero padding
    whose twin is inside the image, which the summed weights cannot express - those keep conv3x3(upsample_size=...).  The result
    differs from conv3x3(upsample=True) by the one fp16 rounding of the summed weights.  Raises on an unsupported shape."""
    if x.dim() != 4 or x.dtype != torch.float16:
        raise ValueError("conv3x3_up2x: x must be a [B, Cin, h, w] fp16 tensor")
    B, Cin, h, w = x.shape
    if (packed.dim() != 4 or packed.shape[0] != 4 or packed.shape[2] != 4 or packed.shape[3] != Cin
            or packed.dtype != torch.float16 or not packed.is_contiguous()):
        raise ValueError(f"conv3x3_up2x: packed must be the contiguous fp16 [4, Cout, 4, {Cin}] tensor of conv3x3_up2x_pack, "
                         f"not {tuple(packed.shape)}")
    Cout = packed.shape[1]
    if bias is not None and (bias.dtype != torch.float16 or bias.numel() != Cout or not bias.is_contiguous()):
        raise ValueError("conv3x3_up2x: bias must be a contiguous fp16 [Cout] tensor")
    _require_gpu(x, packed)
    lib = _lib.load_library()
    x, _, _, _ = _conv3x3_operands("conv3x3_up2x", x, None, None, None)
    out = torch.empty((B, Cout, 2 * h, 2 * w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    nbytes = lib.dsc_conv3x3_up2x_workspace_bytes(B, h, w, Cin, Cout, splits)
    ws = _workspace(x.device, nbytes) if nbytes else None
    rc = lib.dsc_conv3x3_up2x_nhwc_f16(_p(x), _p(packed), _p(bias), _p(out), B, h, w, Cin, Cout, splits, _p(ws),
                                       ws.numel() * 8 if ws is not None else 0, Cin, Cout, 0, _stream_ptr(x))
    _lib.check(rc, "dsc_conv3x3_up2x_nhwc_f16")
    return out


def conv3x3_fewcin(x, weight_t, bias, cout):
    """3x3 / pad 1 convolution of a plain (NCHW) fp16 [B, Cin <= 16, H, W] tensor -> channels_last [B, cout, H, W]
    (dsc_conv3x3_fewcin_f16); weight_t is weight.reshape(cout, Cin * 9).t().contiguous()."""
    _require_gpu(x, weight_t)
    x = x.contiguous()
    B, Cin, H, W = x.shape
    out = torch.empty((B, cout, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    rc = _lib.load_library().dsc_conv3x3_fewcin_f16(_p(x), _p(weight_t), _p(bias), _p(out), B, Cin, H, W, cout, 0, _stream_ptr(x))
    _lib.check(rc, "dsc_conv3x3_fewcin_f16")
    return out


def linear_rows(x, weight, bias=None, silu_out=False, sinusoid_dim=0):
    """Few-row linear (<= 8 rows) of the time-embedding path (dsc_linear_rows_f16): act(x @ weight.T + bias).
    sinusoid_dim > 0: x is an fp32 [M] tensor of timesteps and the input row is its sinusoidal embedding of that width
    ([cos | sin], diffusers Timesteps(flip_sin_to_cos=True, freq_shift=0)), generated inside the kernel."""
    _require_gpu(x, weight)
    N, K = weight.shape
    if sinusoid_dim:
        if x.dtype != torch.float32 or x.dim() != 1 or sinusoid_dim != K:
            raise ValueError("linear_rows: sinusoid input is an fp32 [M] tensor and sinusoid_dim == weight.shape[1]")
        x = x.contiguous()                                   # (an expanded scalar timestep has stride 0: the kernel reads x[m])
        M, ldx = x.shape[0], 0
    else:
        x = x if x.stride(-1) == 1 else x.contiguous()
        M, ldx = x.shape[0], x.stride(0)
    out = torch.empty((M, N), dtype=weight.dtype, device=weight.device)
    flags = (1 if sinusoid_dim else 0) | (2 if silu_out else 0)
    rc = _lib.load_library().dsc_linear_rows_f16(_p(x), _p(weight), _p(bias), _p(out), M, N, K, ldx, N, flags, 0, _stream_ptr(weight))
    _lib.check(rc, "dsc_linear_rows_f16")
    return out


def add_bias_residual(a, b, bias=None):
    """a + b + bias[c] over channels-last / token-major fp16 tensors of identical layout (dsc_add_bias_residual)."""
    _require_gpu(a, b)
    if a.dim() == 4:
        cl = torch.channels_last
        if not a.is_contiguous(memory_format=cl):
            a = a.contiguous(memory_format=cl)
        if not b.is_contiguous(memory_format=cl):
            b = b.contiguous(memory_format=cl)
        C = a.shape[1]
        out = torch.empty_like(a, memory_format=cl)
    else:
        a, b = a.contiguous(), b.contiguous()
        C = a.shape[-1]
        out = torch.empty_like(a)
    rc = _lib.load_library().dsc_add_bias_residual(_p(a), _p(b), _p(bias), _p(out), a.numel() // C, C, 0, _stream_ptr(a))
    _lib.check(rc, "dsc_add_bias_residual")
    return out


def add_layernorm(x, a, weight, bias, eps=1e-5):
    """(x + a, LayerNorm(x + a)) in one launch (dsc_add_layernorm); a may be None -> (x, LayerNorm(x)).
    x, a: [..., C] fp16 contiguous."""
    _require_gpu(x)
    x = x.contiguous()
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    s = x
    if a is not None:
        a = a.contiguous()
        s = torch.empty_like(x)
    rc = _lib.load_library().dsc_add_layernorm(_p(x), _p(a), _p(weight), _p(bias), _p(s) if a is not None else None, _p(y),
                                               rows, C, float(eps), 0, _stream_ptr(x))
    _lib.check(rc, "dsc_add_layernorm")
    return s, y


def softmax_rows(scores, scale=1.0, out=None):
    """softmax(scale * scores, dim=-1) of an fp16 [rows, n] matrix (unit inner stride, 16-byte aligned rows) in fp32 arithmetic
    (dsc_softmax_rows_f16) - the middle step of the VAE's 512-channel attention head between its two GEMMs."""
    _require_gpu(scores)
    if scores.dtype != torch.float16 or scores.dim() != 2 or scores.stride(1) != 1:
        raise TypeError("softmax_rows: a 2-D fp16 matrix with unit inner stride")
    if out is None:
        out = torch.empty_like(scores)
    _check_out(out, scores.shape, scores, "softmax_rows")
    if out.stride(1) != 1:
        raise ValueError("softmax_rows: out needs unit inner stride")
    _drop_gn_partials(out)
    rc = _lib.load_library().dsc_softmax_rows_f16(_p(scores), _p(out), scores.shape[0], scores.shape[1], scores.stride(0),
                                                  out.stride(0), float(scale), 0, _stream_ptr(scores))
    _lib.check(rc, "dsc_softmax_rows_f16")
    return out


def geglu(x):
    """hidden * gelu(gate) for x = [..., 2n] fp16 contiguous (dsc_geglu)."""
    _require_gpu(x)
    lib = _lib.load_library()
    x = x.contiguous()
    n = x.shape[-1] // 2
    y = torch.empty(x.shape[:-1] + (n,), dtype=x.dtype, device=x.device)
    rc = lib.dsc_geglu(_p(x), _p(y), x.numel() // (2 * n), n, 0, _stream_ptr(x))
    _lib.check(rc, "dsc_geglu")
    return y


# ----------------------------------------------------------------------------- sampler step
GRAPHS_ENABLED = True      # the fused pipeline captures the UNet step into a HIP graph (torch.cuda.CUDAGraph)
PROTOCOL_GRAPH = os.environ.get("DSC_PROTOCOL_GRAPH", "1") != "0"   # protocol-mode model calls replay the same graph


def _row_args(row, device):
    """(src, dst, halfs, copies) of the optional row broadcast of the sampler kernels: row = (src [n] fp16, dst [copies, n] fp16)"""
    if row is None:
        return None, None, 0, 0
    src, dst = row
    _require_gpu(src, dst)
    if src.dtype != torch.float16 or dst.dtype != torch.float16 or not dst.is_contiguous() or src.stride(-1) != 1 \
            or dst.dim() != 2 or dst.shape[1] != src.numel() or src.device != device or dst.device != device:
        raise ValueError("row broadcast: fp16 source [n] and contiguous destination [copies, n]")
    _drop_gn_partials(dst)
    return _p(src), _p(dst), src.numel(), dst.shape[0]


def _check_sampler_buffers(what, x, x_in, t_buf, sigma_buf, eps=None, old=None):
    """the sampler kernels address fp16 x / old as [n_img, chw], eps / x_in as [2 n_img, chw] and fp32 t_buf as [2 n_img],
    sigma_buf as [1] (include/dsc_hip.h) - all dense, on x's device; returns (n_img, chw).  Alignment is the C side's check."""
    if x.dim() == 0 or x.shape[0] == 0:
        raise ValueError(f"{what}: x needs a leading image dimension")
    n_img = x.shape[0]
    for name, t, rows in (("x", x, n_img), ("old", old, n_img), ("eps", eps, 2 * n_img), ("x_in", x_in, 2 * n_img)):
        if t is None:
            continue
        if t.dtype != torch.float16:
            raise TypeError(f"{what}: {name} must be fp16, got {t.dtype}")
        if t.device != x.device:
            raise ValueError(f"{what}: {name} is on {t.device}, x on {x.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if t.dim() == 0 or t.shape[0] != rows or t.numel() != rows * (x.numel() // n_img):
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, need {rows} rows of {x.numel() // n_img}")
    if old is not None and old.shape != x.shape:
        raise ValueError(f"{what}: old has shape {tuple(old.shape)}, x {tuple(x.shape)}")
    for name, t in (("t_buf", t_buf), ("sigma_buf", sigma_buf)):
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be fp32, got {t.dtype}")
        if t.device != x.device or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a dense vector on {x.device}")
    if t_buf.numel() != 2 * n_img:
        raise ValueError(f"{what}: t_buf has {t_buf.numel()} elements, need 2 n_img = {2 * n_img}")
    if sigma_buf.numel() < 1:
        raise ValueError(f"{what}: sigma_buf is empty")
    return n_img, x.numel() // n_img


def prepare_unet_input(x, c_in, t, sigma, x_in, t_buf, sigma_buf, row=None):
    """x_in = [x; x] * c_in, t_buf[:] = t, sigma_buf[0] = sigma (dsc_prepare_unet_input); row: see _row_args."""
    _require_gpu(x, x_in, t_buf, sigma_buf)
    n_img, chw = _check_sampler_buffers("prepare_unet_input", x, x_in, t_buf, sigma_buf)
    rargs = _row_args(row, x.device)
    _drop_gn_partials(x_in)
    rc = _lib.load_library().dsc_prepare_unet_input(_p(x), c_in, t, sigma, _p(x_in), _p(t_buf), _p(sigma_buf), n_img, chw, 0,
                                                    *rargs, _stream_ptr(x))
    _lib.check(rc, "dsc_prepare_unet_input")


def cfg_dpmpp2m_step(x, eps, old, sigma, guidance, a, b, c, c_in_next, t_next, sigma_next, x_in, t_buf, sigma_buf, row=None):
    """One launch: CFG combine + eps->denoised + DPM++ 2M update (in place on x, old) + next UNet input (+ the row broadcast)."""
    _require_gpu(x, eps, old, x_in, t_buf, sigma_buf)
    n_img, chw = _check_sampler_buffers("cfg_dpmpp2m_step", x, x_in, t_buf, sigma_buf, eps=eps, old=old)
    rargs = _row_args(row, x.device)
    _drop_gn_partials(x)
    _drop_gn_partials(old)
    _drop_gn_partials(x_in)
    rc = _lib.load_library().dsc_cfg_dpmpp2m_step(_p(x), _p(eps), _p(old), sigma, guidance, a, b, c, c_in_next, t_next,
                                                  sigma_next, _p(x_in), _p(t_buf), _p(sigma_buf), n_img, chw, 0, *rargs,
                                                  _stream_ptr(x))
    _lib.check(rc, "dsc_cfg_dpmpp2m_step")


ROW_STEP, ROW_JOIN, ROW_IDLE = 0, 1, 2
ROW_STEP_MAX_SLOTS = 16


class RowStep(ctypes.Structure):
    """dsc_row_step (include/dsc_hip.h)"""
    _fields_ = [("mode", ctypes.c_int), ("sigma", ctypes.c_float), ("guidance", ctypes.c_float), ("a", ctypes.c_float),
                ("b", ctypes.c_float), ("c", ctypes.c_float), ("c_in_next", ctypes.c_float), ("t_next", ctypes.c_float),
                ("sigma_next", ctypes.c_float), ("temb_row", ctypes.c_void_p)]


class RowLinear(ctypes.Structure):
    """dsc_row_linear (include/dsc_hip.h)"""
    _fields_ = RowStep._fields_[:-1] + [("c_skip", ctypes.c_float), ("c_out", ctypes.c_float), ("s", ctypes.c_float),
                                        ("temb_row", ctypes.c_void_p), ("noise", ctypes.c_void_p)]


def _step_rows_args(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd, linear=False, cat=False):
    """shape / dtype / device validation shared by the per-row sampler steps -> (n_dst, n_slots, chw, dsc_row_step array, or
    dsc_row_linear array with linear=True).  cat: x_in rows may be longer than a latent (cfg_linear_step_rows_cat checks them)."""
    _require_gpu(x, old, x_in, t_buf, sigma_groups)
    n_dst = t_buf.numel() // 2
    n_slots = len(rows)
    if not 1 <= n_dst <= n_slots <= ROW_STEP_MAX_SLOTS:
        raise ValueError(f"{what}: {n_slots} records for a {n_dst}-row bucket (at most {ROW_STEP_MAX_SLOTS})")
    if x.shape[0] < n_slots or old.shape != x.shape:
        raise ValueError(f"{what}: x / old need a latent row per slot")
    chw = x.numel() // x.shape[0]
    for name, t, nr in (("x", x, None), ("old", old, None), ("x_in", x_in, 2 * n_dst), ("eps", eps, 2 * n_src), ("tadd", tadd, 2 * n_dst)):
        if t is None:
            continue
        if t.dtype != torch.float16 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"{what}: {name} must be dense fp16 on {x.device}")
        if nr is not None and t.shape[0] != nr:
            raise ValueError(f"{what}: {name} has {t.shape[0]} rows, need {nr}")
        if name in ("x_in", "eps") and t.numel() != nr * chw and not (cat and name == "x_in"):
            raise ValueError(f"{what}: {name} rows are not [{chw}] latents")
    for name, t, n in (("t_buf", t_buf, 2 * n_dst), ("sigma_groups", sigma_groups, n_dst)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device or t.numel() != n:
            raise ValueError(f"{what}: {name} must be a dense fp32 [{n}] on {x.device}")
    recs = ((RowLinear if linear else RowStep) * n_slots)()
    for i, r in enumerate(rows):
        tr = r.get("temb_row")
        if tr is not None:
            if tadd is None or tr.dtype != torch.float16 or tr.device != x.device or tr.stride(-1) != 1 \
                    or tr.numel() != tadd.shape[1]:
                raise ValueError(f"{what}: temb_row must be an fp16 row of the tadd buffer's width")
        head = (int(r["mode"]), *(float(r.get(f, 0.0)) for f in ("sigma", "guidance", "a", "b", "c", "c_in_next", "t_next")),
                float(r.get("sigma_next", 1.0)))
        if not linear:
            recs[i] = RowStep(*head, None if tr is None else tr.data_ptr())
            continue
        # eps-prediction unless the record says otherwise: D = x - sigma * e
        recs[i] = RowLinear(*head, float(r.get("c_skip", 1.0)), float(r.get("c_out", -float(r.get("sigma", 0.0)))),
                            float(r.get("s", 0.0)), None if tr is None else tr.data_ptr(),
                            _slot_row(what, f"rows[{i}]['noise']", r.get("noise"), chw, x.device))
    for t in (x, old, x_in, t_buf, sigma_groups, tadd):
        _drop_gn_partials(t)
    return n_dst, n_slots, chw, recs


def _slot_row(what, name, t, n, device):
    """address of an optional per-slot row of the per-row sampler steps - a dense fp16 [n] row on x's device - or None for None"""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float16 or t.device != device or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"{what}: {name} must be a dense fp16 [{n}] row on {device}")
    return t.data_ptr()


def _step_rows_call(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, n_dst, n_slots, chw, recs, *more):
    """the library call every per-row sampler step ends in (entry dsc_<what>); more: the entry's own arguments, which follow the
    records (ctypes arrays go as pointers)"""
    more = [ctypes.cast(m, ctypes.c_void_p) if isinstance(m, ctypes.Array) else m for m in more]
    rc = getattr(_lib.load_library(), "dsc_" + what)(
        _p(x), _p(eps), _p(old), n_src, _p(x_in), _p(t_buf), _p(sigma_groups), _p(tadd),
        0 if tadd is None else tadd.shape[1], n_dst, ctypes.cast(recs, ctypes.c_void_p), *more, n_slots, chw, 0, _stream_ptr(x))
    _lib.check(rc, "dsc_" + what)


def cfg_dpmpp2m_step_rows(x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd=None):
    """Per-request sampler step of a continuous batch (dsc_cfg_dpmpp2m_step_rows): slot i = latent row i of x / old, rows
    {i, n_src + i} of eps (the bucket that just ran; eps may be None when no slot steps) and rows {i, n' + i} of x_in / t_buf /
    tadd (the bucket that runs next, n' = t_buf.numel() // 2); sigma_groups [n'] fp32.  rows: one dict per slot with `mode`
    (ROW_STEP / ROW_JOIN / ROW_IDLE), the scalars of dsc_row_step and `temb_row` (an fp16 [tadd width] tensor or None); at least
    n' of them.  x / old hold at least len(rows) latent rows."""
    what = "cfg_dpmpp2m_step_rows"
    _step_rows_call(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd,
                    *_step_rows_args(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd))


def cfg_linear_step_rows(x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd=None):
    """cfg_dpmpp2m_step_rows for every sampler of sampling.LINEAR_FAMILY and both parameterisations (dsc_cfg_linear_step_rows):
    D = c_skip x + c_out e, x' = a x + b D + c D_old + s noise.  rows: cfg_dpmpp2m_step_rows' dicts plus `c_skip` / `c_out`
    (default 1 / -sigma: eps-prediction), `s` and `noise` (this step's fp16 [chw] unit noise row on x's device, or None: no noise
    term).  A record without them gives cfg_dpmpp2m_step_rows' bits.  A STEP record may carry `rescale` (guidance_rescale, phi
    in [0, 1], default 0): when any does with phi > 0 the launch is cfg_linear_step_rows_rescale's, otherwise this one's as ever."""
    what = "cfg_linear_step_rows"
    if any(phi > 0.0 for phi in _row_rescales(what, rows)):
        return cfg_linear_step_rows_rescale(x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd=tadd)
    _step_rows_call(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd,
                    *_step_rows_args(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd, linear=True))


def _row_rescales(what, rows):
    """phi of every record (0 where it is not a STEP record or has no `rescale`), validated"""
    out = []
    for i, r in enumerate(rows):
        phi = r.get("rescale", 0.0) if int(r["mode"]) == ROW_STEP else 0.0
        if isinstance(phi, bool) or not isinstance(phi, (int, float)) or not 0.0 <= phi <= 1.0:       # (NaN fails the range)
            raise ValueError(f"{what}: rows[{i}]['rescale'] (guidance_rescale) must be a number in [0, 1], got {phi!r}")
        out.append(float(phi))
    return out


def cfg_linear_step_rows_rescale(x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd=None):
    """cfg_linear_step_rows with the guidance rescale of each STEP record's `rescale` (dsc_cfg_linear_step_rows_rescale): the
    denoised estimate of a slot with phi > 0 is scaled by K = phi * std(D_c) / std(D) + 1 - phi, the stds taken over the slot's
    whole row inside the same launch; a slot with phi == 0 carries cfg_linear_step_rows' bits."""
    what = "cfg_linear_step_rows_rescale"
    phis = _row_rescales(what, rows)
    args = _step_rows_args(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd, linear=True)
    _step_rows_call(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, *args, (ctypes.c_float * len(phis))(*phis))


class RowExtra(ctypes.Structure):
    """dsc_row_extra (include/dsc_hip.h)"""
    _fields_ = [("extra", ctypes.c_void_p)]


def cfg_linear_step_rows_cat(x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, extras, tadd=None):
    """cfg_linear_step_rows for a UNet whose input carries more channels than the latent - the 9-channel inpainting checkpoints,
    `[latents | mask | masked-image latents]` (dsc_cfg_linear_step_rows_cat).  x_in: contiguous [2 n', chw + extra_halfs] (or a
    view of that shape, [2 n', 9, h, w]); the first chw halfs of a row are cfg_linear_step_rows' (with a `rescale` > 0 in some
    record: cfg_linear_step_rows_rescale's) bits, the rest is the slot's `extras` entry times the record's c_in_next.  extras: one
    entry per record of `rows` - an fp16 [extra_halfs] tensor on x's device (unscaled, step-invariant), or None: zeros.  IDLE
    slots get a zero row whatever their entry.  The library refuses extra_halfs % 8 != 0, chw % 8 != 0 and rows that are not
    16-byte aligned before it launches anything."""
    what = "cfg_linear_step_rows_cat"
    phis = _row_rescales(what, rows)
    n_dst, n_slots, chw, recs = _step_rows_args(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd, linear=True, cat=True)
    if x_in.numel() % (2 * n_dst) != 0 or x_in.numel() // (2 * n_dst) < chw:
        raise ValueError(f"{what}: x_in has shape {tuple(x_in.shape)}, need {2 * n_dst} rows of [{chw}] latents plus the extra channels")
    extra_halfs = x_in.numel() // (2 * n_dst) - chw
    if len(extras) != n_slots:
        raise ValueError(f"{what}: {len(extras)} extras for {n_slots} slots")
    ex = (RowExtra * n_slots)(*(RowExtra(_slot_row(what, f"extras[{i}]", t, extra_halfs, x.device)) for i, t in enumerate(extras)))
    phi = (ctypes.c_float * n_slots)(*phis) if any(p > 0.0 for p in phis) else None
    _step_rows_call(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, n_dst, n_slots, chw, recs, phi, ex, extra_halfs)


ROW_STAGE_FULL, ROW_STAGE_PREDICT, ROW_STAGE_CORRECT = 0, 1, 2


class RowStage(ctypes.Structure):
    """dsc_row_stage (include/dsc_hip.h)"""
    _fields_ = [("stage", ctypes.c_int), ("m", ctypes.c_float)]


def cfg_staged_step_rows(x, mid, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd=None):
    """cfg_linear_step_rows for the two-call samplers of sampling.TWO_CALL_FAMILY (dsc_cfg_staged_step_rows).  rows:
    cfg_linear_step_rows' dicts plus `stage` (ROW_STAGE_FULL, the default: the linear step; ROW_STAGE_PREDICT: the update goes to
    the slot's row of `mid` and into x_in, x stays; ROW_STAGE_CORRECT: the model ran on `mid` - D is taken from it and `m` * mid
    joins the update of x) and `m` (default 0).  mid: a dense fp16 tensor of x's shape (None only when every STEP record is FULL).
    A STEP record's `rescale` is applied inside the same launch, whatever the stage."""
    what = "cfg_staged_step_rows"
    phis = _row_rescales(what, rows)
    n_dst, n_slots, chw, recs = _step_rows_args(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd, linear=True)
    if mid is not None:
        _require_gpu(mid)
        if mid.dtype != torch.float16 or not mid.is_contiguous() or mid.device != x.device or mid.shape != x.shape:
            raise ValueError(f"{what}: mid must be dense fp16 of x's shape {tuple(x.shape)} on {x.device}")
        _drop_gn_partials(mid)
    stages = (RowStage * n_slots)()
    for i, r in enumerate(rows):
        stage = r.get("stage", ROW_STAGE_FULL)
        if isinstance(stage, bool) or not isinstance(stage, int):
            raise ValueError(f"{what}: rows[{i}]['stage'] must be ROW_STAGE_FULL / _PREDICT / _CORRECT, got {stage!r}")
        stages[i] = RowStage(stage, float(r.get("m", 0.0)))
    phi = (ctypes.c_float * n_slots)(*phis) if any(p > 0.0 for p in phis) else None
    rc = _lib.load_library().dsc_cfg_staged_step_rows(
        _p(x), _p(mid), _p(eps), _p(old), n_src, _p(x_in), _p(t_buf), _p(sigma_groups), _p(tadd),
        0 if tadd is None else tadd.shape[1], n_dst, ctypes.cast(recs, ctypes.c_void_p), ctypes.cast(stages, ctypes.c_void_p),
        None if phi is None else ctypes.cast(phi, ctypes.c_void_p), n_slots, chw, 0, _stream_ptr(x))
    _lib.check(rc, "dsc_" + what)


class RowKnown(ctypes.Structure):
    """dsc_row_known (include/dsc_hip.h)"""
    _fields_ = [("image", ctypes.c_void_p), ("noise", ctypes.c_void_p), ("mask", ctypes.c_void_p),
                ("blend_now", ctypes.c_int), ("blend_next", ctypes.c_int)]


def cfg_dpmpp2m_step_rows_known(x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, known, tadd=None):
    """cfg_dpmpp2m_step_rows with the known region of inpainting slots blended into the model input
    (dsc_cfg_dpmpp2m_step_rows_known).  known: one entry per record of `rows` - None (the slot has no known region: the plain
    op's bits) or a dict with `image` / `noise` / `mask` (fp16 [chw] rows on x's device, mask 1 = repaint, 0 = keep) and the
    flags `blend_now` / `blend_next`.  A row given as None inside a dict is passed as NULL: the library refuses a record with
    only some of the three, and rows that are not 16-byte aligned."""
    what = "cfg_dpmpp2m_step_rows_known"
    n_dst, n_slots, chw, recs = _step_rows_args(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, rows, tadd)
    if len(known) != n_slots:
        raise ValueError(f"{what}: {len(known)} known-region records for {n_slots} slots")
    kn = (RowKnown * n_slots)()
    for i, k in enumerate(known):
        if k is None:
            continue
        ptrs = [_slot_row(what, f"known[{i}][{name!r}]", k.get(name), chw, x.device) for name in ("image", "noise", "mask")]
        kn[i] = RowKnown(*ptrs, int(bool(k.get("blend_now"))), int(bool(k.get("blend_next"))))
    _step_rows_call(what, x, eps, old, n_src, x_in, t_buf, sigma_groups, tadd, n_dst, n_slots, chw, recs, kn)


def dpmpp2m_update(x, denoised, old, a, b, c):
    """a*x + b*denoised + c*old as one launch (dsc_dpmpp2m_update)."""
    _require_gpu(x, denoised)
    x, denoised = x.contiguous(), denoised.contiguous()
    if old is not None:
        old = old.contiguous()
    elif c != 0.0:
        raise ValueError("c != 0 needs the previous denoised estimate")
    out = torch.empty_like(x)
    rc = _lib.load_library().dsc_dpmpp2m_update(_p(x), _p(denoised), _p(old), a, b, c if old is not None else 0.0,
                                                _p(out), x.numel(), 0, _stream_ptr(x))
    _lib.check(rc, "dsc_dpmpp2m_update")
    return out


# The hires pass's resample + noise launch (dsc_latent_resample_noise).  Its wrapper lives beside the tap tables it is made of;
# like every writer here it drops GroupNorm partial sums from its destination (tests/test_hires_gpu.py).
from .modules.latent_resample import latent_resample_noise, noise_scale_f16  # noqa: E402,F401


# the gated per-row residual add of the continuous batcher's T2I-Adapter step (dsc_add_rows_gated_f16): its wrapper lives beside
# its kernel's name, like modules/latent_resample.py's, and is reached as ops.add_rows_gated / ops.add_rows_gated_supported
from .gated_add import add_rows_gated, add_rows_gated_supported  # noqa: E402,F401


# the ControlNet residuals of the continuous batcher's compact lanes, added into their batch rows (dsc_scatter_add_rows_f16):
# wrapper beside its kernel's name, like gated_add.py's, reached as ops.scatter_add_rows / ops.scatter_add_rows_supported
from .scatter_add import scatter_add_rows, scatter_add_rows_supported, scatter_add_rows_torch  # noqa: E402,F401


# the finished image of a served request (dsc_image_finish: the decoder's fp16 NCHW output -> uint8 / float32 NHWC): wrapper beside
# its kernel's name, like gated_add.py's, reached as ops.image_finish; image_finish_torch restates its arithmetic in torch
from .image_finish import IMAGE_KINDS, image_finish, image_finish_torch  # noqa: E402,F401

# live previews of running requests (dsc_latent_preview: up to 16 fp16 latent rows -> uint8 RGB thumbnails): wrapper beside its
# kernel's name, reached as ops.latent_preview; latent_preview_numpy restates its arithmetic in numpy float32, op by op
from .latent_preview import LATENT_RGB_SD15, PREVIEW_MAX_CHANNELS, PREVIEW_MAX_ROWS, PREVIEW_SCALES, latent_preview, latent_preview_numpy  # noqa: E402,F401

# FreeU on an up-block ResNet's (hidden, skip) pair (dsc_freeu_rows_f16: the half-channel scale and the four-frequency Fourier
# filter, per batch row, in one launch): wrapper beside its kernel's name, reached as ops.freeu_rows_ / ops.freeu_covers;
# freeu_eager is diffusers' algorithm with torch.fft in fp32 (the CPU / fp32 route and the tests' restatement)
USE_FREEU_KERNEL = os.environ.get("DSC_FREEU", "1") != "0"   # A/B switch: 0 = FreeU through freeu_eager (torch.fft) everywhere
from .freeu import FREEU_MAX_SIDE, fourier_filter_eager, freeu_covers, freeu_eager, freeu_rows_, freeu_values  # noqa: E402,F401

# pixel inputs of served requests (dsc_image_prepare: request images -> the VAE encoder's fp16 input, the masked image and the
# latent mask; dsc_latent_start_rows: the encoder's moments -> latents and start latents, per row): wrappers beside their kernels'
# names, reached as ops.image_prepare / ops.latent_start; the *_torch functions are the literal eager chains they replace
from .image_prepare import image_prepare, image_prepare_torch, latent_start, latent_start_torch, start_form  # noqa: E402,F401

# prompt emphasis behind the text encoder on the text lane of the continuous batcher (dsc_prompt_weight_rows_f16: multipliers and
# mean restoration of every (request, chunk) group in one launch): wrapper beside its kernel's name, reached as
# ops.prompt_weight_rows; prompt_weight_numpy restates the contract with exact sums, prompt_weight_torch is the eager chain
from .prompt_weight import MAX_GROUPS as PROMPT_WEIGHT_MAX_GROUPS, prompt_weight_numpy, prompt_weight_rows, prompt_weight_torch  # noqa: E402,F401

# LoRA adapters merged into every touched weight in one launch (dsc_lora_merge_f16: base + sum of gain-scaled low-rank products,
# rounded once): wrapper beside its kernel's name, reached as ops.lora_merge_ / ops.lora_merge_takes; lora_merge_eager is the
# reference's arithmetic in torch (CPU, fp32 / fp64, shapes outside the limits, DSC_LORA=0)
from .lora_merge import (MAX_RANK as LORA_MAX_RANK, SEGMENT as LORA_SEGMENT, LoraMergeTable, lora_merge_, lora_merge_eager,  # noqa: E402,F401
                         lora_merge_takes, pack_adapters as lora_pack_adapters, padded_rank as lora_padded_rank)
