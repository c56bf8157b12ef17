"""ops.freeu_rows_ / ops.freeu_covers / ops.freeu_eager: FreeU (arXiv 2309.11497) on the two inputs of an up-block ResNet.
`freeu_rows_` wraps dsc_freeu_rows_f16 (csrc/freeu.hip): one launch, in place, (s1, s2, b1, b2) per batch row read from device
memory - the form a captured step uses (UNet2DConditionModel.forward(freeu_rows=...), modules/serving/).  `freeu_eager` is the
literal algorithm of diffusers' `apply_freeu` / `fourier_filter` with torch.fft, always in fp32: the route of CPU, fp32 and
non-channels-last tensors, and the restatement the tests compare the kernel against."""
import torch

from . import _lib

FREEU_MAX_SIDE = 512                     # DSC_FREEU_MAX_SIDE (include/dsc_hip.h)


def _ops():
    from . import ops                    # (ops re-exports this module's functions: resolved at call time)
    return ops


def _pair_ok(hidden, skip):
    """None, or why dsc_freeu_rows_f16 does not take this (hidden, skip) pair"""
    if not (torch.is_tensor(hidden) and torch.is_tensor(skip)):
        return "hidden and skip must be tensors"
    if not (hidden.is_cuda and skip.is_cuda and hidden.device == skip.device):
        return "hidden and skip must be on one GPU"
    if hidden.dtype != torch.float16 or skip.dtype != torch.float16:
        return f"hidden and skip must be fp16, got {hidden.dtype} / {skip.dtype}"
    if hidden.dim() != 4 or skip.dim() != 4 or hidden.shape[0] != skip.shape[0] or hidden.shape[2:] != skip.shape[2:]:
        return f"hidden {tuple(hidden.shape)} and skip {tuple(skip.shape)} must be [B, C, H, W] with the same B, H, W"
    B, C_h, H, W = (int(v) for v in hidden.shape)
    C_s = int(skip.shape[1])
    if B < 1 or B > 65535:
        return f"{B} batch rows; the kernel takes 1 to 65535"
    if H < 2 or W < 2 or H > FREEU_MAX_SIDE or W > FREEU_MAX_SIDE:
        return f"sides {H} x {W}; the kernel takes 2 to {FREEU_MAX_SIDE} (diffusers' slice means something else on a side of 1)"
    if C_h % 16 or C_s % 8:
        return f"{C_h} hidden channels must be a multiple of 16 and {C_s} skip channels a multiple of 8 (16-byte pieces)"
    if not (hidden.is_contiguous(memory_format=torch.channels_last) and skip.is_contiguous(memory_format=torch.channels_last)):
        return f"hidden and skip must be channels-last and dense, got strides {hidden.stride()} / {skip.stride()}"
    if hidden.data_ptr() % 16 or skip.data_ptr() % 16:
        return "hidden and skip must be 16-byte aligned"
    return None


def freeu_covers(hidden, skip):
    """whether freeu_rows_ takes this pair (dsc_freeu_rows_f16: fp16 channels-last [B, C, H, W] on one GPU with the same B, H, W,
    sides 2 to 512, C_h % 16 == 0, C_s % 8 == 0, 16-byte aligned) and the kernel route is switched on (ops.USE_FREEU_KERNEL, the
    environment's DSC_FREEU)"""
    return _ops().USE_FREEU_KERNEL and _pair_ok(hidden, skip) is None


def freeu_rows_(hidden, skip, params, stage):
    """FreeU on (hidden, skip), both updated IN PLACE by one launch (dsc_freeu_rows_f16) and returned: per batch row r
    `hidden[r, :C_h/2] *= b` (`fp16(fp32(x) * b)`: torch's fp16 `x * b` as the CPU computes it, bit for bit) and `skip[r] =
    fourier_filter(skip[r], threshold=1, scale=s)` (seven fp64 sums per channel and one pass, rounded once).  params fp32 [B, 4]
    on the device = (s1, s2, b1, b2) per row, read by the kernel (a captured launch sees the values of the moment it replays);
    stage 0 (up block 0) uses (s1, b1), stage 1 (s2, b2).
    A row with b == 1 / s == 1 has its hidden / skip row neither read nor written.  Everything is checked before the launch."""
    ops = _ops()
    if not all(torch.is_tensor(t) for t in (hidden, skip, params)):
        raise TypeError("freeu_rows_: hidden, skip and params must be tensors")
    ops._require_gpu(hidden, skip, params)
    why = _pair_ok(hidden, skip)
    if why is None and params.device != hidden.device:
        why = "params must be on the operands' GPU"
    if why is not None:
        raise (TypeError if "fp16" in why else ValueError)(f"freeu_rows_: {why}")
    B, C_h, H, W = (int(v) for v in hidden.shape)
    C_s = int(skip.shape[1])
    if params.dtype != torch.float32 or tuple(params.shape) != (B, 4) or not params.is_contiguous():
        raise ValueError(f"freeu_rows_: params must be a contiguous fp32 [{B}, 4] tensor (s1, s2, b1, b2 per batch row), got "
                         f"{params.dtype} {tuple(params.shape)}")
    if stage not in (0, 1):
        raise ValueError(f"freeu_rows_: stage must be 0 (up block 0: s1, b1) or 1 (up block 1: s2, b2), got {stage!r}")

    def overlap(a, a_bytes, b, b_bytes):
        return a.data_ptr() < b.data_ptr() + b_bytes and b.data_ptr() < a.data_ptr() + a_bytes

    hb, sb = hidden.numel() * 2, skip.numel() * 2
    if overlap(hidden, hb, skip, sb) or overlap(hidden, hb, params, 16 * B) or overlap(skip, sb, params, 16 * B):
        raise ValueError("freeu_rows_: hidden, skip and params must not overlap")
    ops._drop_gn_partials(hidden)            # group sums a producer attached describe the values before this launch
    ops._drop_gn_partials(skip)
    rc = _lib.load_library().dsc_freeu_rows_f16(ops._p(hidden), C_h, ops._p(skip), C_s, B, H, W, ops._p(params), int(stage),
                                                ops._stream_ptr(hidden))
    _lib.check(rc, "dsc_freeu_rows_f16")
    return hidden, skip


def _per_row(v, B, like, name):
    """a float or B numbers -> an fp32 [B, 1, 1, 1] tensor on like's device"""
    t = torch.as_tensor(v, dtype=torch.float32).to(like.device).reshape(-1)
    if t.numel() == 1:
        t = t.expand(B)
    if t.numel() != B:
        raise ValueError(f"freeu_eager: {name} must be one number or one per batch row ({B}), got {t.numel()}")
    return t.reshape(B, 1, 1, 1)


def fourier_filter_eager(x, scale):
    """diffusers' `fourier_filter(x, threshold=1, scale)` on x [B, C, H, W], computed in fp32 whatever x's dtype (diffusers runs
    power-of-two sides in x's own dtype): fftn over (H, W), fftshift, the block [H//2-1 : H//2+1, W//2-1 : W//2+1] times scale
    (one number or one per batch row), ifftshift, ifftn, .real -> fp32"""
    B, _, H, W = x.shape
    if H < 2 or W < 2:
        raise ValueError(f"freeu: sides {H} x {W}; a side of 1 is refused (diffusers' slice means something else there)")
    freq = torch.fft.fftshift(torch.fft.fftn(x.float(), dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, 1, H, W), dtype=torch.float32, device=x.device)
    crow, ccol = H // 2, W // 2
    mask[..., crow - 1:crow + 1, ccol - 1:ccol + 1] = _per_row(scale, B, x, "s")
    freq = torch.fft.ifftshift(freq * mask, dim=(-2, -1))
    return torch.fft.ifftn(freq, dim=(-2, -1)).real


def freeu_eager(hidden, skip, s, b):
    """(hidden', skip'), NEW tensors of the operands' dtypes: diffusers' `apply_freeu` for one up-block ResNet, literally -
    `hidden[:, :C/2] * b` (in hidden's dtype, as torch multiplies) and `fourier_filter(skip, 1, s)` with torch.fft in fp32, cast
    back.  s, b: one number each, or one per batch row (a tensor may live on the operands' device: nothing is synchronised).  A
    row with s == 1 keeps its skip values exactly, as on the kernel route."""
    B, C = hidden.shape[0], hidden.shape[1]
    half = C // 2
    bt = _per_row(b, B, hidden, "b")
    out_h = hidden.clone(memory_format=torch.preserve_format)
    out_h[:, :half] = (hidden[:, :half].float() * bt).to(hidden.dtype)      # fp16: the fp32 product rounded once, as `x * b`
    out_s = torch.empty_like(skip, memory_format=torch.preserve_format)
    # a row with s == 1 keeps its values exactly, as on the kernel route (the transform there and back is the identity only to
    # rounding); out_s keeps skip's layout
    out_s.copy_(torch.where(_per_row(s, B, skip, "s") == 1.0, skip.float(), fourier_filter_eager(skip, s)))
    return out_h, out_s


def freeu_values(v):
    """(s1, s2, b1, b2) as four finite floats from a 4-sequence or a dict with those names; ValueError otherwise"""
    import math
    if isinstance(v, dict):
        if set(v) != {"s1", "s2", "b1", "b2"}:
            raise ValueError(f"freeu: a dict must have exactly the keys s1, s2, b1, b2, got {sorted(v)}")
        v = (v["s1"], v["s2"], v["b1"], v["b2"])
    try:
        vals = tuple(float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"freeu: expected four numbers (s1, s2, b1, b2), got {v!r}") from None
    if len(vals) != 4 or any(isinstance(x, bool) for x in v) or not all(math.isfinite(x) for x in vals):
        raise ValueError(f"freeu: expected four finite numbers (s1, s2, b1, b2), got {v!r}")
    return vals
