"""ops.add_rows_gated / ops.add_rows_gated_supported: the wrapper of dsc_add_rows_gated_f16 (csrc/gated_add.hip), the residual
added with one gate per batch row that the continuous batcher's captured step uses for T2I-Adapter features
(modules/serving/, UNet2DConditionModel.forward(down_intrablock_gated=...))."""
import torch

from . import _lib


def _ops():
    from . import ops                    # (ops re-exports this module's functions: resolved at call time)
    return ops


def _dense_rows(t):
    """(layout, halfs per row) of a tensor whose batch rows are dense in memory: "nhwc" for a channels-last [B, C, h, w],
    "tokens" for a contiguous [B, ..., C]; None when it is neither"""
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return "nhwc", t[0].numel()
    if t.dim() >= 2 and t.is_contiguous():
        return "tokens", t[0].numel()
    return None


def add_rows_gated_supported(x, feat):
    """whether add_rows_gated takes these operands (dsc_add_rows_gated_f16: fp16 on one GPU, both channels-last or both
    token-major with the same trailing shape, rows of a multiple of 8 halfs, 16-byte aligned, x's rows a multiple of feat's)"""
    if not (torch.is_tensor(x) and torch.is_tensor(feat) and x.is_cuda and feat.is_cuda and x.device == feat.device):
        return False
    if x.dtype != torch.float16 or feat.dtype != torch.float16 or x.dim() < 2 or x.shape[1:] != feat.shape[1:]:
        return False
    lx, lf = _dense_rows(x), _dense_rows(feat)
    if lx is None or lf is None or lx[0] != lf[0]:
        return False
    if x.shape[0] < 1 or feat.shape[0] < 1 or x.shape[0] % feat.shape[0] != 0 or x.shape[0] > 65535:
        return False
    return lx[1] >= 8 and lx[1] % 8 == 0 and x.data_ptr() % 16 == 0 and feat.data_ptr() % 16 == 0


def add_rows_gated(x, feat, gate, out=None):
    """out[r] = x[r] + gate[r] * feat[r % F] per batch row (dsc_add_rows_gated_f16: the T2I-Adapter residual of the continuous
    batcher's step).  x [B, ...] and feat [F, ...] fp16 with the same trailing shape, both channels-last or both token-major
    (dense batch rows), B % F == 0; gate [B] fp32 on the device, read by the kernel (a captured launch sees the values of the
    moment it replays).  One fp32 fma and one rounding: gate 1 gives the bits of `x + feat`.  Rows with gate 0 never read their
    feature row; with out=x (in place) they are not touched at all, otherwise copied.  out: None (a new tensor of x's layout),
    x itself, or a tensor of x's shape and layout that does not overlap it.  Returns out."""
    ops = _ops()
    ops._require_gpu(x, feat, gate)
    if x.dtype != torch.float16 or feat.dtype != torch.float16:
        raise TypeError("add_rows_gated: x / feat must be fp16")
    if x.dim() < 2 or x.shape[1:] != feat.shape[1:]:
        raise ValueError(f"add_rows_gated: x {tuple(x.shape)} and feat {tuple(feat.shape)} must share their trailing shape")
    lx, lf = _dense_rows(x), _dense_rows(feat)
    if lx is None or lf is None or lx[0] != lf[0]:
        raise ValueError(f"add_rows_gated: x and feat must both be channels-last or both token-major with dense batch rows, got "
                         f"strides {x.stride()} / {feat.stride()}")
    B, F_, n = x.shape[0], feat.shape[0], lx[1]
    if F_ < 1 or B % F_ != 0:
        raise ValueError(f"add_rows_gated: x's {B} rows are not a multiple of feat's {F_}")
    if B > 65535:
        raise ValueError(f"add_rows_gated: {B} batch rows; the kernel takes at most 65535")
    if n < 8 or n % 8 != 0:
        raise ValueError(f"add_rows_gated: {n} halfs per row is not a multiple of 8 (16-byte pieces)")
    if not torch.is_tensor(gate) or gate.dtype != torch.float32 or tuple(gate.shape) != (B,) or not gate.is_contiguous():
        got = f"{gate.dtype} {tuple(gate.shape)}" if torch.is_tensor(gate) else type(gate).__name__
        raise ValueError(f"add_rows_gated: gate must be a contiguous fp32 [{B}] tensor, got {got}")
    if out is None:
        out = torch.empty_like(x, memory_format=torch.channels_last if lx[0] == "nhwc" else torch.contiguous_format)
    ops._check_out(out, x.shape, x, "add_rows_gated")
    if _dense_rows(out) is None or _dense_rows(out)[0] != lx[0]:
        raise ValueError(f"add_rows_gated: out must have x's layout, got strides {out.stride()} for {x.stride()}")
    if feat.device != x.device or gate.device != x.device:
        raise ValueError("add_rows_gated: all operands must be on one device")
    if any(t.data_ptr() % 16 for t in (x, feat, out)):
        raise ValueError("add_rows_gated: x / feat / out must be 16-byte aligned")
    nbytes = B * n * 2

    def overlap(a, a_bytes, b, b_bytes):
        return a.data_ptr() < b.data_ptr() + b_bytes and b.data_ptr() < a.data_ptr() + a_bytes

    if out.data_ptr() != x.data_ptr() and overlap(out, nbytes, x, nbytes):
        raise ValueError("add_rows_gated: out overlaps x without being x (in place means the same rows)")
    if overlap(out, nbytes, feat, F_ * n * 2) or overlap(out, nbytes, gate, 4 * B):
        raise ValueError("add_rows_gated: out overlaps feat or gate")
    ops._drop_gn_partials(out)
    rc = _lib.load_library().dsc_add_rows_gated_f16(ops._p(x), ops._p(feat), ops._p(gate), ops._p(out), B, F_, n, ops._stream_ptr(x))
    _lib.check(rc, "dsc_add_rows_gated_f16")
    return out
