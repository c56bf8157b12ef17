"""Attention processors for the MI355X hot path - drop-in counterparts of reference
`source/modules/attention_modify.py`:

  * `scaled_dot_product_attention_regionstate` (:74-103)  -> one fused HIP call (two launches)
  * `AttnProcessor2_0` (:405-503) - the live processor (app.py:479-481)
  * `AttnProcessor` (:106-207)    - same arithmetic through `get_attention_scores` (:39-70); verified
                                    bit-equal to AttnProcessor2_0 in fp32, so both classes share one
                                    implementation here and differ only in which `scale` they honour
Same call signature, same `region_prompt` contract:
    {"region_state": {L: FloatTensor[Bw, L, S]} | non-dict, "sigma": 0-dim tensor, "weight_func": callable}
(plus, from the serving mode, "sigma_per_group": True with "sigma" an [n_std_groups] fp32 device tensor: one sigma per
request of a continuous batch; the fused default-weight_func routes only, others raise NotImplementedError)

What changes underneath:
  * the scores are never materialised: q.k^T, *scale, std(), w*sigma*std, repeat_interleave, +=, softmax, @v run
    inside libdsc_hip.so (diffusionspatialcontrol_amd/csrc/region_xattn.hip);
  * the region table is uploaded ONCE per table object instead of once per call (:481 `.to(query.device)`);
  * `weight_func` is a caller-supplied callable (app.py:1004 builds a fresh lambda per request): it is probed once
    with two tiny tensors; if it behaves as `w * sigma * qk.std()` the fused path runs, otherwise the scores are
    materialised, the callable is evaluated as the reference would, and its result is added by the same kernel.
Which kernel runs a call is decided by `attention_plan` (the facts of the call -> a ROUTE_* constant or the refusal) and run by
`run_attention`; the limits of the kernels are ops.XATTN_MAX_KEYS / XATTN_MAX_KEYS_PACKED / ATTN_MAX_HEAD_DIM (DESIGN.md
"Attention routes" is the table; tests/golden/attention_routes.json pins it on the host).
There is no CPU path: tensors must live on the GPU and libdsc_hip.so must be built.
"""
import math
from collections import OrderedDict
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

USE_PEFT_BACKEND = True


# ----------------------------------------------------------------------------- weight_func dispatch
_PROBES = (
    (torch.tensor([[[0.25, -1.5, 3.0], [0.0, 2.0, -0.5]]]), torch.tensor(1.75),
     torch.tensor([[[0.5, -2.0, 4.0], [1.0, 0.0, -3.0]]])),
    (torch.tensor([[[-0.75, 0.125, 1.0], [4.0, -2.5, 0.0]]]), torch.tensor(0.3125),
     torch.tensor([[[7.0, 1.0, -1.0], [2.5, -4.0, 0.25]]])),
)


class _PerObjectCache:
    """What was derived from an object, keyed by (id, in-place version, *extra): the entry holds the object, so its id cannot be
    reused while the entry lives; the least recently used entry leaves when there are more than `size`."""

    def __init__(self, size):
        self.size, self.entries = size, OrderedDict()

    def get(self, obj, make, *extra):
        key = (id(obj), getattr(obj, "_version", None)) + extra
        hit = self.entries.get(key)
        if hit is not None and hit[0] is obj:
            self.entries.move_to_end(key)
            return hit[1]
        value = make()
        self.entries[key] = (obj, value)
        while len(self.entries) > self.size:
            self.entries.popitem(last=False)
        return value


_WF_CACHE, _TABLE_CACHE, _COMPRESSED_CACHE, _SIGMA_CACHE = _PerObjectCache(32), _PerObjectCache(64), _PerObjectCache(64), _PerObjectCache(8)


def _probe_weight_func(weight_func):
    try:
        for w, s, qk in _PROBES:
            r = weight_func(w, s, qk)
            e = w * s * qk.std()
            if not (torch.is_tensor(r) and r.shape == e.shape and torch.allclose(r.float(), e, rtol=1e-6, atol=0.0)):
                return False
    except Exception:  # noqa: BLE001 - any failure on the probe means "not the default": take the generic path
        return False
    return True


def weight_func_is_default(weight_func):
    """True iff `weight_func(w, sigma, qk)` equals `w * sigma * qk.std()` on two probes."""
    return _WF_CACHE.get(weight_func, lambda: _probe_weight_func(weight_func))


def weight_func_fused(weight_func):
    """None or default-equivalent: the fused kernels compute the bias themselves"""
    return weight_func is None or weight_func_is_default(weight_func)


# ----------------------------------------------------------------------------- region table residency
def resident_table(w, device):
    """fp32 device copy of a region table, made once per (tensor object, version, device)."""
    if w.device == device and w.dtype == torch.float32 and w.is_contiguous():
        return w
    return _TABLE_CACHE.get(w, lambda: w.to(device=device, dtype=torch.float32).contiguous(), str(device))


def compressed_table(w, device):
    """(ids, rows) of ops.compress_region_table_for_kernel for a region table, or None when it has too many distinct rows;
    computed once per (tensor object, version, device) like resident_table."""
    return _COMPRESSED_CACHE.get(w, lambda: ops.compress_region_table_for_kernel(resident_table(w, device)), str(device))


def _sigma_arg(sigma):
    """What ops.region_xattn[_packed] take as sigma without a host sync: a python float, or an fp32 device tensor - a device
    scalar of another dtype is converted once per (tensor object, version)."""
    if not torch.is_tensor(sigma) or not sigma.is_cuda:
        return float(sigma)
    if sigma.dtype == torch.float32:
        return sigma
    return _SIGMA_CACHE.get(sigma, lambda: sigma.detach().float().reshape(1))


# ----------------------------------------------------------------------------- the plan: which route runs an attention call
ROUTE_FLASH = "flash"                      # dsc_self_attn_fwd: self-attention, and long keys without a table
ROUTE_SDPA = "sdpa"                        # the library's scaled_dot_product_attention: what no kernel here can read
ROUTE_PLAIN_KERNEL = "plain-kernel"        # dsc_region_xattn_fwd without a table
ROUTE_PLAIN_PACKED = "plain-packed"        # dsc_region_xattn_fwd_packed without a table
ROUTE_PLAIN_MASK = "plain-mask"            # dsc_region_xattn_fwd, the mask as its final bias
ROUTE_REGION_PACKED = "region-packed"      # dsc_region_xattn_fwd_packed: packed text K/V + (ids, rows) table
ROUTE_REGION_DENSE = "region-dense"        # dsc_region_xattn_fwd with the dense table
ROUTE_REGION_GENERIC = "region-generic"    # scores materialised for a custom weight_func, its result the kernel's final bias
ROUTE_REGION_LONG = "region-long"          # more keys than the kernels hold: the reference's op sequence on the library
ROUTE_REGION_MASKED = "region-masked"      # dsc_region_xattn_std_masked, then mask + bias as the kernel's final bias
ROUTES = (ROUTE_FLASH, ROUTE_SDPA, ROUTE_PLAIN_KERNEL, ROUTE_PLAIN_PACKED, ROUTE_PLAIN_MASK, ROUTE_REGION_PACKED, ROUTE_REGION_DENSE,
          ROUTE_REGION_GENERIC, ROUTE_REGION_LONG, ROUTE_REGION_MASKED)


def attention_plan(*, S, d, dtype, is_self=False, layout="blhd", table=False, mask=False, packed=False, compressed=None,
                   fused_weight_func=True, ref16=False, per_group_sigma=False, short_keys_unchecked=True):
    """The route of one attention call, from its facts alone - decides (or refuses), launches nothing.
    S keys of head dim d in `dtype`; table: a region table applies; mask: an additive mask applies; packed: the text K/V have a
    packed image (ops.xattn_kv_pack); compressed: the table has an (ids, rows) form - True, None = not derived yet (assume it
    has: the caller asks again with False if it turns out to have none), False = none, or the table is a static buffer that must
    be read densely (region_prompt["compressed"] = False); fused_weight_func: weight_func_fused(); ref16: the reference's fp16
    rounding; per_group_sigma: one sigma per std group (serving) - only the fused kernels take it.
    short_keys_unchecked (no table): the sites WITHOUT a mask hand up to XATTN_MAX_KEYS keys to the region kernel whatever the
    dtype and head dim, and what it cannot read is its refusal (TypeError for fp32); the site WITH a mask passes False and
    asks first, because the library route takes the mask at any shape.  The difference is older than this plan and is kept."""
    short = S <= ops.XATTN_MAX_KEYS
    if table:
        if per_group_sigma and mask:
            raise NotImplementedError("per-group sigma: attention masks are not supported")
        if per_group_sigma and not fused_weight_func:
            raise NotImplementedError("per-group sigma: a custom weight_func is not supported")
        if mask:
            if not short:
                raise NotImplementedError(f"attention masks with more than {ops.XATTN_MAX_KEYS} text keys")
            return ROUTE_REGION_MASKED
        can_pack = packed and compressed is not False and layout == "blhd" and fused_weight_func
        if not short:
            # the prepared-operand kernels walk the keys in chunks with an online softmax (fp32 scores, default weight_func,
            # compressible table); anything else runs the reference's op sequence as library kernels
            if can_pack and S <= ops.XATTN_MAX_KEYS_PACKED and not ref16:
                return ROUTE_REGION_PACKED
            if per_group_sigma:
                raise NotImplementedError(f"per-group sigma: {S} text keys need the chunked prepared-operand kernels "
                                          f"(<= {ops.XATTN_MAX_KEYS_PACKED} keys, packed text K/V, compressible table)")
            return ROUTE_REGION_LONG
        if not fused_weight_func:
            return ROUTE_REGION_GENERIC
        return ROUTE_REGION_PACKED if can_pack else ROUTE_REGION_DENSE
    if is_self and not mask:
        return ROUTE_FLASH
    fits = ops.attn_kernel_takes(dtype, d)
    if short and (fits or short_keys_unchecked):
        return ROUTE_PLAIN_MASK if mask else ROUTE_PLAIN_PACKED if packed else ROUTE_PLAIN_KERNEL
    return ROUTE_FLASH if fits and not mask else ROUTE_SDPA


def _scores(q, k, layout, scale):
    """scale * q k^T materialised by the library, [B, H, L, S]: what a custom weight_func is evaluated on (reference :90-95)"""
    qh, kh = (q, k) if layout == "bhld" else (q.transpose(1, 2), k.transpose(1, 2))
    return (qh @ kh.transpose(-2, -1)) * (scale if scale else 1.0 / math.sqrt(q.shape[-1]))


def _region_attention_long(q, k, v, w, sigma, weight_func, fused, layout, n_std_groups, scale):
    """Prompts longer than one 77-token chunk (S = 154, 231, ... from the A1111-style encoder): the fused kernels hold
    at most ops.XATTN_MAX_KEYS keys, so the reference's op sequence (attention_modify.py:90-103) runs as library kernels on
    the GPU - scores materialised once, the std over the std group(s), bias add, softmax, PV."""
    vh = v if layout == "bhld" else v.transpose(1, 2)
    scores = _scores(q, k, layout, scale)
    B, H, L, S = scores.shape
    w_dev = resident_table(w, q.device)
    sig = sigma.float() if (torch.is_tensor(sigma) and sigma.is_cuda) else float(sigma)   # device scalar: no host sync (graphs)
    if not fused:
        bias = torch.broadcast_to(weight_func(w_dev, sigma, scores.reshape(-1, L, S)), w_dev.shape)
    elif n_std_groups == 1:
        bias = w_dev * sig * scores.float().std()
    else:                                                                       # row b belongs to group b % n_std_groups
        g = scores.float().reshape(B // n_std_groups, n_std_groups, -1).transpose(0, 1).reshape(n_std_groups, -1).std(dim=1)
        Bw = w_dev.shape[0]
        rows = (torch.arange(Bw, device=q.device) * (B * H // Bw)) // H         # table row -> batch row (b = bh // H)
        bias = w_dev * sig * g[rows % n_std_groups].reshape(Bw, 1, 1)
    flat = scores.reshape(-1, L, S).float() + torch.repeat_interleave(bias.float(), (B * H) // bias.shape[0], dim=0)
    out = torch.softmax(flat, dim=-1).to(vh.dtype).reshape(B, H, L, S) @ vh
    return out if layout == "bhld" else out.transpose(1, 2).contiguous()


def _region_attention_masked(q, k, v, w, sigma, weight_func, fused, layout, n_std_groups, scale, ref16, mask):
    """The region path with an additive attention mask (reference :85-97 / :144-170): the mask enters the scores BEFORE the
    statistics, so the std comes from dsc_region_xattn_std_masked; mask + w * sigma * std is then the final bias of the
    forward kernel (one dense fp32 [Bc*H, L, S] tensor - this is the rarely-taken path, app.py never passes a mask)."""
    Bc, H, L, _ = q.shape if layout == "bhld" else q.transpose(1, 2).shape
    S = k.shape[2 if layout == "bhld" else 1]
    # a custom weight_func meets a mask of another shape in its own `scores + mask` below (RuntimeError, as the reference's)
    m3 = ops.mask_3d(mask, Bc * H, L, S, check=fused)
    w_dev = resident_table(w, q.device)
    rep = (Bc * H) // w_dev.shape[0]
    if fused:
        std = ops.region_xattn_std(q, k, layout=layout, n_std_groups=n_std_groups, scale=scale, ref_fp16_rounding=ref16, mask=m3)
        sig = sigma.float() if (torch.is_tensor(sigma) and sigma.is_cuda) else float(sigma)
        if ref16:                                                                   # 0-dim fp16 tensors in the fp16 pipeline
            std = std.half().float()
            sig = torch.as_tensor(sig).half().float() if not torch.is_tensor(sig) else sig.half().float()
        grp = (torch.arange(Bc * H, device=q.device) // H) % n_std_groups           # row bh = b * H + h belongs to group b % n
        region = torch.repeat_interleave(w_dev, rep, dim=0) * sig * std[grp].reshape(-1, 1, 1)
    else:
        scores = _scores(q, k, layout, scale).reshape(-1, L, S) + m3.to(q.dtype)
        region = torch.repeat_interleave(torch.broadcast_to(weight_func(w_dev, sigma, scores), w_dev.shape).float(), rep, dim=0)
    bias = (region + m3).contiguous()
    return ops.region_xattn(q, k, v, bias, 1.0, layout=layout, scale=scale, bias_is_final=True, ref_fp16_rounding=ref16)


def _region_attention_generic(q, k, v, w, sigma, weight_func, layout, scale, ref16):
    """a custom weight_func: evaluate it the way the reference does (attention_modify.py:90-95), then let the kernel add its
    result (flag BIAS_IS_FINAL).  Slow path by construction - the scores are materialised once."""
    w_dev = resident_table(w, q.device)
    scores = _scores(q, k, layout, scale)
    bias = weight_func(w_dev, sigma, scores.reshape(-1, scores.shape[-2], scores.shape[-1]))
    bias = torch.broadcast_to(bias, w_dev.shape).float().contiguous()
    return ops.region_xattn(q, k, v, bias, 1.0, layout=layout, scale=scale, bias_is_final=True, ref_fp16_rounding=ref16)


def run_attention(route, q, k, v, *, layout="blhd", scale=None, mask=None, packed_kv=None, table=None, comp=None, sigma=1.0,
                  weight_func=None, fused=True, n_std_groups=1, ref16=False, per_group_sigma=False):
    """Runs the route attention_plan chose.  q / k / v [B, L | S, H, d] ('blhd': views of the projection outputs, the only layout
    of the routes without a table) or [B, H, L | S, d] ('bhld') -> the attention output in q's layout, contiguous.
    mask: additive, [B*H, 1|L, S] without a table, anything ops.mask_3d takes with one; table: the region table, comp its
    (ids, rows); the defaults are a call without a table (sigma 1, one std group, fp32 scores)."""
    if route == ROUTE_FLASH:
        return ops.self_attention(q, k, v, scale=scale)          # [B, L, H, d]; S != L: long keys without a table
    S = k.shape[2 if layout == "bhld" else 1]
    if route in (ROUTE_REGION_PACKED, ROUTE_PLAIN_PACKED):       # prepared operands: packed text K/V (+ row-id region table)
        return ops.region_xattn_packed(q, packed_kv, S, comp, _sigma_arg(sigma), n_std_groups=n_std_groups, scale=scale,
                                       ref_fp16_rounding=ref16, per_group_sigma=per_group_sigma)
    if route in (ROUTE_REGION_DENSE, ROUTE_PLAIN_KERNEL):
        w_dev = None if table is None else resident_table(table, q.device)
        return ops.region_xattn(q, k, v, w_dev, _sigma_arg(sigma), layout=layout, n_std_groups=n_std_groups, scale=scale,
                                ref_fp16_rounding=ref16, per_group_sigma=per_group_sigma)
    if route == ROUTE_REGION_GENERIC:
        return _region_attention_generic(q, k, v, table, sigma, weight_func, layout, scale, ref16)
    if route == ROUTE_REGION_LONG:
        return _region_attention_long(q, k, v, table, sigma, weight_func, fused, layout, n_std_groups, scale)
    if route == ROUTE_REGION_MASKED:
        return _region_attention_masked(q, k, v, table, sigma, weight_func, fused, layout, n_std_groups, scale, ref16, mask)
    B, L, H, _ = q.shape
    if route == ROUTE_PLAIN_MASK:                                # (:483-485 / :182-186) the mask is the forward kernel's final bias
        bias = torch.broadcast_to(mask.float(), (B * H, L, S)).contiguous()
        return ops.region_xattn(q, k, v, bias, 1.0, layout="blhd", scale=scale, bias_is_final=True, ref_fp16_rounding=False)
    if route != ROUTE_SDPA:
        raise ValueError(f"unknown attention route {route!r}")
    m4 = None if mask is None else mask.view(B, H, -1, S).to(q.dtype)
    return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=m4,
                                          scale=scale).transpose(1, 2).contiguous()


def _plain_attention(q4, k4, v4, scale, *, mask3=None, packed_kv=None, is_self=False):
    """Attention without a region table, q4 [B, L, H, d], k4 / v4 [B, S, H, d]: the flash kernel for self-attention; else the
    region kernel (no table, or the mask as its final bias) when the keys fit it, the flash kernel when dtype and head dim fit,
    the library's SDPA otherwise.  Only the call with a mask asks about dtype and head dim before it takes the region kernel
    (attention_plan, short_keys_unchecked)."""
    route = attention_plan(S=k4.shape[1], d=q4.shape[-1], dtype=q4.dtype, is_self=is_self, mask=mask3 is not None,
                           packed=packed_kv is not None, short_keys_unchecked=mask3 is None)
    return run_attention(route, q4, k4, v4, scale=scale, mask=mask3, packed_kv=packed_kv)


def _region_attention(q, k, v, w, sigma, weight_func, layout, n_std_groups, scale=None, ref16=False, packed_kv=None,
                      comp=None, mask=None, per_group_sigma=False):
    """Attention with the region table `w`.  comp: the caller's (ids, rows) of `w`, None = compress `w` here when a route needs it
    (cached per tensor version), False = `w` is a static buffer whose CONTENTS change between replays of a captured step: read it
    densely, derive nothing from its values.
    per_group_sigma: `sigma` is an [n_std_groups] fp32 device tensor, one sigma per std group (continuous batching,
    modules/serving/) - only the fused default-weight_func kernels take it; every other route raises NotImplementedError."""
    fused = weight_func_fused(weight_func)                       # asked once per call
    facts = dict(S=k.shape[2 if layout == "bhld" else 1], d=q.shape[-1], dtype=q.dtype, layout=layout, table=True,
                 mask=mask is not None, packed=packed_kv is not None, fused_weight_func=fused, ref16=ref16,
                 per_group_sigma=per_group_sigma)
    route = attention_plan(compressed=None if comp is None else comp is not False, **facts)
    if route == ROUTE_REGION_PACKED and comp is None:
        comp = compressed_table(w, q.device)
        if comp is None:                                         # more distinct rows than the kernels' table holds
            route = attention_plan(compressed=False, **facts)
    return run_attention(route, q, k, v, layout=layout, scale=scale, mask=mask, packed_kv=packed_kv, table=w, comp=comp, sigma=sigma,
                         weight_func=weight_func, fused=fused, n_std_groups=n_std_groups, ref16=ref16,
                         per_group_sigma=per_group_sigma)


def scaled_dot_product_attention_regionstate(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False,
                                             scale=None, weight_func=None, region_state=None, sigma=None,
                                             n_std_groups=1) -> torch.Tensor:
    """Same signature and result as attention_modify.py:74-103; query [Bc,H,L,d], key/value [Bc,H,S,d].

    attn_mask as the reference treats it (:85-91): a FLOAT mask is added in place into an [L, S] bias (`attn_bias +=
    attn_mask`), so it must broadcast INTO [L, S] - a [B, H, ., S] mask raises the same RuntimeError torch raises there -
    and the std is taken over the masked scores; a BOOL mask only rewrites itself (`attn_mask.masked_fill_(~attn_mask,
    -inf)` on a bool tensor turns every element True) and never reaches the scores - reproduced, not fixed."""
    if is_causal or dropout_p != 0.0:
        raise NotImplementedError("is_causal / dropout are not on the hot path (never used by app.py)")
    mask = None
    if attn_mask is not None:
        if attn_mask.dtype == torch.bool:
            attn_mask.masked_fill_(attn_mask.logical_not(), float("-inf"))          # :86-87, all True afterwards
        else:
            L, S = query.size(-2), key.size(-2)
            mask = torch.zeros(L, S, dtype=query.dtype, device=query.device)
            mask += attn_mask                                                        # :89 (raises unless it broadcasts into [L, S])
    return _region_attention(query, key, value, region_state, sigma, weight_func, "bhld", n_std_groups, scale,
                             ref16=query.dtype == torch.float16, mask=mask)


def get_attention_scores(attn, query, key, attention_mask=None):
    """attention_modify.py:39-70 (used by the generic weight_func path of callers that want raw scores): library baddbmm,
    the mask as its additive input (beta = 1)."""
    if attn.upcast_attention:
        query, key = query.float(), key.float()
    if attention_mask is None:
        base, beta = torch.empty(query.shape[0], query.shape[1], key.shape[1], dtype=query.dtype, device=query.device), 0
    else:
        base, beta = attention_mask, 1
    scores = torch.baddbmm(base, query, key.transpose(-1, -2), beta=beta, alpha=attn.scale)
    if attn.upcast_softmax:
        scores = scores.float()
    return scores.to(query.dtype)


class _RegionProcessor:
    """Shared body of AttnProcessor / AttnProcessor2_0 (reference :106-207 and :414-503)."""

    honours_attn_scale = False
    is_ip_adapter = False

    def __init__(self, n_std_groups: int = 1, ref_fp16_rounding: bool = False):
        # 1 = the reference: ONE std over the whole call (all rows, all heads).  The pipeline sets B when it
        # micro-batches B images in the row layout [u_0..u_{B-1}, c_0..c_{B-1}] so that each image keeps the std
        # group the reference's one-image-per-call k-diffusion path gives it.
        self.n_std_groups = n_std_groups
        # False: scores stay fp32 inside the kernel (the parity target is the reference's CPU fp32 pipeline).
        # True: round where the reference's fp16 GPU tensors round (scores, std, bias add, softmax) - ~15 % slower.
        self.ref_fp16_rounding = ref_fp16_rounding

    def __call__(self, attn, hidden_states: torch.Tensor, encoder_hidden_states=None,
                 attention_mask: Optional[torch.Tensor] = None, temb: Optional[torch.Tensor] = None, scale: float = 1.0,
                 region_prompt=None, ip_adapter_masks=None, _ln_fold=None) -> torch.Tensor:
        # _ln_fold (private, passed only by this package's BasicTransformerBlock to its own stock processors - see
        # u_net_condition_modify.LNFold): hidden_states is the UN-normalised residual stream, the block's LayerNorm is
        # folded into the q / qkv projection, the block's residual add into to_out, and (output, row statistics) is returned
        residual = hidden_states
        n_queries = hidden_states.shape[1]                        # :427 - dim 1 also for 4-D input
        ip_hidden_states = None
        # prepared rows (the continuous batcher's step, see prepared_ip_rows): the text arrives alone - no split, which in its
        # deprecated single-tensor form would cut the last num_tokens[0] text rows off
        ip_rows = prepared_ip_rows(region_prompt) if self.is_ip_adapter and encoder_hidden_states is not None else None
        if self.is_ip_adapter and encoder_hidden_states is not None and ip_rows is None:
            encoder_hidden_states, ip_hidden_states = self._split_ip(encoder_hidden_states)
        if attn.spatial_norm is not None:
            hidden_states = attn.spatial_norm(hidden_states, temb)
        image_shape = hidden_states.shape if hidden_states.ndim == 4 else None
        if image_shape is not None:
            hidden_states = hidden_states.view(image_shape[0], image_shape[1], -1).transpose(1, 2)
        is_self = encoder_hidden_states is None
        mask3 = None
        if attention_mask is not None:
            # reference :144 / :448-452: [B, 1|L, S_mask] -> padded to the key length and repeated per head -> [B*H, 1|L, S]
            kv_len = hidden_states.shape[1] if is_self else encoder_hidden_states.shape[1]
            mask3 = attn.prepare_attention_mask(attention_mask, kv_len, hidden_states.shape[0])
        if attn.group_norm is not None:
            hidden_states = attn.group_norm(hidden_states.transpose(1, 2)).transpose(1, 2)
        q4, k4, v4, packed_kv = self._project_qkv(attn, hidden_states, encoder_hidden_states, _ln_fold)
        sc = attn.scale if self.honours_attn_scale else None
        out = self._attend(q4, k4, v4, sc, packed_kv, mask3, None if is_self else region_prompt, n_queries, is_self)
        hidden_states = out.reshape(q4.shape[0], q4.shape[1], -1)
        if ip_rows is not None:
            hidden_states = self._ip_rows_branch(q4, hidden_states, ip_rows[self], ip_adapter_masks, sc)
        elif self.is_ip_adapter:
            hidden_states = self._ip_branch(attn, q4, hidden_states, ip_hidden_states, ip_adapter_masks, sc)
        return self._project_out(attn, hidden_states, residual, image_shape, _ln_fold)

    @staticmethod
    def _project_qkv(attn, hidden_states, encoder_hidden_states, _ln_fold):
        """-> q4 [B, L, H, d], k4 / v4 [B, S, H, d] (views) and the packed image of the text K/V, or None"""
        is_self = encoder_hidden_states is None
        H = attn.heads
        fused_qkv = getattr(attn, "qkv_weight", None)
        if is_self and fused_qkv is not None and attn.to_q.bias is None:
            # self-attention: q, k, v from ONE [3C, C] GEMM; the three [B, L, H, d] operands are strided views of it
            wq = fused_qkv()
            w2, b2, ln = _ln_fold.folded(attn, "qkv", wq) if _ln_fold is not None else (wq, None, None)
            if ops.linear_qkv_covers(hidden_states, wq, H):
                # the GEMM's epilogue writes K / V head-major: the flash kernel's key tiles are then contiguous DMA pieces
                return (*ops.linear_qkv(hidden_states, w2, b2, H, ln=ln), None)
            qkv = ops.linear_ln(hidden_states, w2, b2, ln=ln) if ln is not None else ops.linear(hidden_states, wq)
            C = qkv.shape[-1] // 3
            return (*(qkv[..., i * C:(i + 1) * C].unflatten(-1, (H, C // H)) for i in range(3)), None)
        if _ln_fold is not None:
            w2, b2, ln = _ln_fold.folded(attn, "q", attn.to_q.weight, attn.to_q.bias)
            query = ops.linear_ln(hidden_states, w2, b2, ln=ln)
        else:
            query = ops.linear(hidden_states, attn.to_q.weight, attn.to_q.bias) if type(attn.to_q) is nn.Linear \
                else attn.to_q(hidden_states)
        if is_self:
            encoder_hidden_states = hidden_states
        elif attn.norm_cross:
            encoder_hidden_states = attn.norm_encoder_hidden_states(encoder_hidden_states)
        packed_kv = None
        cache = getattr(attn, "kv_cache", None)
        if cache is not None and cache["src"] is not encoder_hidden_states:     # another generation slot's text buffer?
            cache = next((c for c in getattr(attn, "kv_caches", ()) if c["src"] is encoder_hidden_states), None)
        if cache is not None and cache["src"] is encoder_hidden_states:
            key, value = cache["k"], cache["v"]          # text K/V: once per generation, not once per step
            packed_kv = cache.get("packed")
        else:
            key = attn.to_k(encoder_hidden_states)
            value = attn.to_v(encoder_hidden_states)
        if not is_self and key.shape[0] != query.shape[0] and key.shape[0] % query.shape[0] == 0:
            # shared CFG prefix (UNet2DConditionModel.forward): up to the first cross-attention the unconditional and
            # the conditional rows of the batch are the same numbers and were computed once - from here on they differ
            # (one image: a stride-0 batch dimension - the kernels take the query's strides - instead of a 5 MB copy launch)
            query = query.expand(key.shape[0], -1, -1) if query.shape[0] == 1 else query.repeat(key.shape[0] // query.shape[0], 1, 1)
        B, L, C = query.shape
        S = key.shape[1]
        return query.view(B, L, H, C // H), key.view(B, S, H, C // H), value.view(B, S, H, C // H), packed_kv

    def _attend(self, q4, k4, v4, sc, packed_kv, mask3, region_prompt, n_queries, is_self):
        """the text (or self-) attention -> [B, L, H, d]: with the region table of the level when the call carries one"""
        if region_prompt is None or not isinstance(region_prompt["region_state"], dict):
            return _plain_attention(q4, k4, v4, sc, mask3=mask3, packed_kv=packed_kv, is_self=is_self)
        w = region_prompt["region_state"][n_queries]                    # KeyError when L is not a level (:481)
        pre = region_prompt.get("compressed")                           # the pipeline's static (ids, rows) buffers
        comp = pre.get(n_queries) if isinstance(pre, dict) else (False if pre is False else None)
        if mask3 is not None and not self.honours_attn_scale:
            # AttnProcessor2_0 hands the [B, H, ., S] view of the mask to scaled_dot_product_attention_regionstate, whose
            # in-place `attn_bias += attn_mask` into an [L, S] tensor torch refuses for any 4-D mask (:89): the
            # reference raises here - so does this (same exception type)
            B, L, H, _ = q4.shape
            S = k4.shape[1]
            torch.zeros(L, S, dtype=q4.dtype, device=q4.device).add_(mask3.view(B, H, -1, S))
        return _region_attention(q4, k4, v4, w, region_prompt["sigma"], region_prompt["weight_func"], "blhd",
                                 region_prompt.get("n_std_groups", self.n_std_groups), sc, ref16=self.ref_fp16_rounding,
                                 packed_kv=packed_kv, comp=comp, mask=mask3,
                                 per_group_sigma=bool(region_prompt.get("sigma_per_group", False)))

    @staticmethod
    def _project_out(attn, hidden_states, residual, image_shape, _ln_fold):
        to_out = attn.to_out[0]
        if _ln_fold is not None:
            # the block's `x = attn(norm(x)) + x` add and the next LayerNorm's row statistics ride in this GEMM's epilogue
            res = ops.residual_for_batch(_ln_fold.residual, hidden_states.shape[0])    # shared CFG prefix: computed once per image
            return ops.linear_ln(hidden_states, to_out.weight, to_out.bias, residual=res, ln_stats=True)
        hidden_states = ops.linear(hidden_states, to_out.weight, to_out.bias) if type(to_out) is nn.Linear \
            else to_out(hidden_states)
        hidden_states = attn.to_out[1](hidden_states)
        if image_shape is not None:
            hidden_states = hidden_states.transpose(-1, -2).reshape(image_shape)
        if attn.residual_connection:
            hidden_states = hidden_states + residual
        if attn.rescale_output_factor != 1.0:
            hidden_states = hidden_states / attn.rescale_output_factor
        return hidden_states


def prepared_ip_rows(region_prompt):
    """The prepared IP-Adapter rows a call carries, or None: region_prompt["ip_rows"] = {processor: [(k_ip, v_ip, row_scale), ...
    one per adapter]} with k_ip / v_ip [B, T, H * d] fp16 (to_k_ip / to_v_ip of the adapter's image tokens of every batch row,
    computed once per request; a batch stride is allowed) and row_scale [B] fp32 on the device (0: the row has no image prompt).
    A fourth element is the adapter's region mask as one weight per query: a [B, L] fp16 buffer for the layer's query count, or
    a {L: buffer} dict resolved by the layer's L (`ip_adapter_masks` down-sampled once per request; ones: no mask).
    The continuous batcher's captured step passes them (modules/serving/): the buffers are static, their contents change
    between replays.  Every other caller hands the image tokens over as the reference does, as (text, [tokens])."""
    if not isinstance(region_prompt, dict):
        return None
    return region_prompt.get("ip_rows")


class AttnProcessor2_0(_RegionProcessor):
    r"""Counterpart of reference `AttnProcessor2_0` (:405-503): scale is 1/sqrt(head_dim) on every branch."""
    honours_attn_scale = False


class AttnProcessor(_RegionProcessor, nn.Module):
    r"""Counterpart of reference `AttnProcessor` (:106-207): scores use `attn.scale` (:57-63)."""
    honours_attn_scale = True

    def __init__(self, n_std_groups: int = 1, ref_fp16_rounding: bool = False):
        nn.Module.__init__(self)
        _RegionProcessor.__init__(self, n_std_groups, ref_fp16_rounding)

    def forward(self, *a, **k):
        return _RegionProcessor.__call__(self, *a, **k)

    __call__ = _RegionProcessor.__call__


# ----------------------------------------------------------------------------- IP-Adapter
class IPAdapterMaskProcessor:
    """`downsample` of diffusers 0.27.2 `IPAdapterMaskProcessor` (imported at reference attention_modify.py:25, called at
    :373-376 and :672-675).  diffusers is not part of the reference tree nor of this image: restated from the published
    algorithm, PARITY UNPINNED (oracle/region_attention.py `ip_mask_downsample` is the same restatement)."""

    @staticmethod
    def downsample(mask: torch.Tensor, batch_size: int, num_queries: int, value_embed_dim: int):
        o_h, o_w = mask.shape[1], mask.shape[2]
        ratio = o_w / o_h
        mask_h = int(math.sqrt(num_queries / ratio))
        mask_h = int(mask_h) + int((num_queries % int(mask_h)) != 0)
        mask_w = num_queries // mask_h
        m = F.interpolate(mask.unsqueeze(0), size=(mask_h, mask_w), mode="bicubic").squeeze(0)
        if m.shape[0] < batch_size:
            m = m.repeat(batch_size, 1, 1)
        m = m.view(m.shape[0], -1)
        area = mask_h * mask_w
        if area < num_queries:
            m = F.pad(m, (0, num_queries - m.shape[1]), value=0.0)
        if area > num_queries:
            m = m[:, :num_queries]
        return m.view(m.shape[0], m.shape[1], 1).repeat(1, 1, value_embed_dim)


class _IPAdapterProcessor(_RegionProcessor, nn.Module):
    """Shared body of the two IP-Adapter processors (reference :208-404 and :506-700): the text branch is the region
    cross-attention of `_RegionProcessor`; every adapter adds `scale_i * softmax(q k_ip^T) v_ip` (optionally times a
    down-sampled mask) of the SAME queries before the output projection.  Constructor arguments, attribute names and
    the `to_k_ip` / `to_v_ip` ModuleLists (hence the state-dict keys `_load_ip_adapter_weights` fills) are the
    reference's.  The image-token attention (4 / 16 tokens per adapter) runs on the generic HIP kernel without a table."""

    is_ip_adapter = True

    def __init__(self, hidden_size, cross_attention_dim=None, num_tokens=(4,), scale=1.0, n_std_groups: int = 1,
                 ref_fp16_rounding: bool = False):
        nn.Module.__init__(self)
        _RegionProcessor.__init__(self, n_std_groups, ref_fp16_rounding)
        self.hidden_size = hidden_size
        self.cross_attention_dim = cross_attention_dim
        if not isinstance(num_tokens, (tuple, list)):
            num_tokens = [num_tokens]
        self.num_tokens = num_tokens
        if not isinstance(scale, list):
            scale = [scale] * len(num_tokens)
        if len(scale) != len(num_tokens):
            raise ValueError("`scale` should be a list of integers with the same length as `num_tokens`.")
        self.scale = scale
        self.to_k_ip = nn.ModuleList([nn.Linear(cross_attention_dim, hidden_size, bias=False) for _ in num_tokens])
        self.to_v_ip = nn.ModuleList([nn.Linear(cross_attention_dim, hidden_size, bias=False) for _ in num_tokens])

    def _split_ip(self, encoder_hidden_states):
        if isinstance(encoder_hidden_states, tuple):
            return encoder_hidden_states
        # deprecated single-tensor form (:568-577): the last num_tokens[0] rows are the (single) adapter's image tokens
        end_pos = encoder_hidden_states.shape[1] - self.num_tokens[0]
        return encoder_hidden_states[:, :end_pos, :], [encoder_hidden_states[:, end_pos:, :]]

    def _ip_branch(self, attn, q4, hidden_states, ip_hidden_states, ip_adapter_masks, sc):
        if ip_adapter_masks is not None:
            if not isinstance(ip_adapter_masks, torch.Tensor) or ip_adapter_masks.ndim != 4:
                raise ValueError(" ip_adapter_mask should be a tensor with shape [num_ip_adapter, 1, height, width]."
                                 " Please use `IPAdapterMaskProcessor` to preprocess your mask")
            if len(ip_adapter_masks) != len(self.scale):
                raise ValueError(f"Number of ip_adapter_masks ({len(ip_adapter_masks)}) must match number of IP-Adapters "
                                 f"({len(self.scale)})")
        else:
            ip_adapter_masks = [None] * len(self.scale)
        if ip_hidden_states is None:                 # self-attention call: the reference would fail on an unbound name
            return hidden_states
        B, L, H, d = q4.shape
        for cur, scale, to_k_ip, to_v_ip, mask in zip(ip_hidden_states, self.scale, self.to_k_ip, self.to_v_ip, ip_adapter_masks):
            T = cur.shape[1]
            k4 = to_k_ip(cur).view(B, T, H, d)
            v4 = to_v_ip(cur).view(B, T, H, d)
            o = _plain_attention(q4, k4, v4, sc).reshape(B, L, H * d)    # 257-token variants (Full / Plus): the flash kernel
            if mask is not None:
                md = IPAdapterMaskProcessor.downsample(mask, B, o.shape[1], o.shape[2])
                o = o * md.to(dtype=o.dtype, device=o.device)
            hidden_states = hidden_states + scale * o
        return hidden_states

    def _ip_rows_branch(self, q4, hidden_states, rows, ip_adapter_masks, sc):
        """the static route of the continuous batcher: one launch per adapter adds row_scale[b] * softmax(q k_ip^T) v_ip to the text
        branch's output in place (dsc_ip_xattn_add_f16) - instead of _ip_branch's two GEMMs, attention, multiply and add with
        a scale baked in as a Python float.  Rows with a fourth element carry the region mask as per-query weights
        (dsc_ip_xattn_add_masked_f16) - instead of _ip_branch's interpolate, repeat and multiply per layer and step"""
        if ip_adapter_masks is not None:
            raise ValueError("`ip_adapter_masks` are not supported with prepared IP-Adapter rows (the continuous batcher hands masks "
                             "over inside the rows, as per-query weights)")
        if len(rows) != len(self.num_tokens):
            raise ValueError(f"prepared IP-Adapter rows for {len(rows)} adapters, the processor holds {len(self.num_tokens)}")
        B, L, H, d = q4.shape
        for k_ip, v_ip, row_scale, *rest in rows:
            qw = rest[0] if rest else None
            if isinstance(qw, dict):
                qw = qw[L]
            ops.ip_xattn_add(q4, k_ip.unflatten(-1, (H, d)), v_ip.unflatten(-1, (H, d)), row_scale, hidden_states, scale=sc,
                             q_weight=qw)
        return hidden_states

    def forward(self, *a, **k):
        return _RegionProcessor.__call__(self, *a, **k)

    __call__ = _RegionProcessor.__call__


class IPAdapterAttnProcessor2_0(_IPAdapterProcessor):
    r"""Counterpart of reference `IPAdapterAttnProcessor2_0` (:506-700): scale 1/sqrt(head_dim) on every branch."""
    honours_attn_scale = False


class IPAdapterAttnProcessor(_IPAdapterProcessor):
    r"""Counterpart of reference `IPAdapterAttnProcessor` (:208-404): scores use `attn.scale` (:57-63)."""
    honours_attn_scale = True
