"""ops.scatter_add_rows / ops.scatter_add_rows_supported: the wrapper of dsc_scatter_add_rows_f16 (csrc/scatter_add.hip), the
ControlNet residuals of a compact lane batch added into the batch rows they belong to
(UNet2DConditionModel.forward(down_block_scattered=...)); scatter_add_rows_torch is the same chain in torch ops."""
import torch

from . import _lib
from .gated_add import _dense_rows

MAX_NETS = 8                             # kScatterMaxNets (csrc/scatter_add.hip)


def _ops():
    from . import ops                    # (ops re-exports this module's functions: resolved at call time)
    return ops


def _feat_layout(x, feat):
    """(layout, halfs per row) when feat [A, R, ...] holds, per net, R dense rows of x's trailing shape in x's layout and the
    nets lie densely behind one another; None otherwise"""
    lx = _dense_rows(x)
    if lx is None or feat.dim() != x.dim() + 1 or feat.shape[2:] != x.shape[1:] or feat.shape[0] < 1 or feat.shape[1] < 1:
        return None
    lf = _dense_rows(feat[0])
    if lf is None or lf[0] != lx[0] or lf[1] != lx[1]:
        return None
    if feat.shape[0] > 1 and feat.stride(0) != feat.shape[1] * lx[1]:
        return None
    return lx


def scatter_add_rows_supported(x, feat):
    """whether scatter_add_rows takes these operands (dsc_scatter_add_rows_f16: fp16 on one GPU, x [X, ...] channels-last or
    token-major, feat [A, R, ...] of the same trailing shape and layout per net, rows of a multiple of 8 halfs, 16-byte aligned)"""
    if not (torch.is_tensor(x) and torch.is_tensor(feat) and x.is_cuda and feat.is_cuda and x.device == feat.device):
        return False
    if x.dtype != torch.float16 or feat.dtype != torch.float16 or x.dim() < 2:
        return False
    lx = _feat_layout(x, feat)
    if lx is None or feat.shape[0] > MAX_NETS or feat.shape[1] > 65535 or x.shape[0] < 1:
        return False
    return lx[1] >= 8 and lx[1] % 8 == 0 and x.data_ptr() % 16 == 0 and feat.data_ptr() % 16 == 0


def scatter_add_rows(x, feat, gate, dst):
    """In place: x[dst[j]] += sum over nets a of gate[a][j] * feat[a][j], for every lane row j with dst[j] >= 0 and an open gate
    (dsc_scatter_add_rows_f16: the ControlNet residuals of the continuous batcher's step).  x [X, ...] fp16, channels-last or
    token-major (dense batch rows); feat [A, R, ...] fp16, per net R rows of x's trailing shape and layout, the nets dense behind
    one another; gate [A, R] fp32 and dst [R] int32 on the device, read by the kernel (a captured launch sees the values of the
    moment it replays).  Every product and sum is an fp32 operation rounded to fp16 on its own, in the order `t = g0 * f0`,
    `t = t + g_a * f_a` (nets with gate 0 left out), `x + t`: with A == 1 the bits of torch's `x[d] + feat[j] * g` (as torch
    multiplies tensors of 2048 elements and more; its small-tensor kernel rounds the exact product once).  A lane row with
    dst < 0 or every gate 0 reads and writes nothing.
    THE CALLER'S INVARIANT: the destination rows of active lane rows are distinct (the kernel cannot check device data; host code
    that builds `dst` asserts it).  Drops GroupNorm partial sums attached to x.  Returns x."""
    ops = _ops()
    ops._require_gpu(x, feat, gate, dst)
    if x.dtype != torch.float16 or feat.dtype != torch.float16:
        raise TypeError("scatter_add_rows: x / feat must be fp16")
    if x.dim() < 2 or feat.dim() != x.dim() + 1 or feat.shape[2:] != x.shape[1:]:
        raise ValueError(f"scatter_add_rows: feat {tuple(feat.shape)} must be [nets, lane rows] + x's trailing shape "
                         f"{tuple(x.shape[1:])}")
    A, R, X = feat.shape[0], feat.shape[1], x.shape[0]
    if A < 1 or R < 1 or X < 1:
        raise ValueError(f"scatter_add_rows: nets {A}, lane rows {R} and batch rows {X} must all be >= 1")
    if A > MAX_NETS:
        raise ValueError(f"scatter_add_rows: {A} nets; the kernel takes at most {MAX_NETS}")
    if R > 65535:
        raise ValueError(f"scatter_add_rows: {R} lane rows; the kernel takes at most 65535")
    lx = _feat_layout(x, feat)
    if lx is None:
        raise ValueError(f"scatter_add_rows: x and every feat[a] must both be channels-last or both token-major with dense rows, "
                         f"the nets dense behind one another, got strides {x.stride()} / {feat.stride()}")
    n = lx[1]
    if n < 8 or n % 8 != 0:
        raise ValueError(f"scatter_add_rows: {n} halfs per row is not a multiple of 8 (16-byte pieces)")
    if not torch.is_tensor(gate) or gate.dtype != torch.float32 or tuple(gate.shape) != (A, R) or not gate.is_contiguous():
        got = f"{gate.dtype} {tuple(gate.shape)}" if torch.is_tensor(gate) else type(gate).__name__
        raise ValueError(f"scatter_add_rows: gate must be a contiguous fp32 [{A}, {R}] tensor, got {got}")
    if not torch.is_tensor(dst) or dst.dtype != torch.int32 or tuple(dst.shape) != (R,) or not dst.is_contiguous():
        got = f"{dst.dtype} {tuple(dst.shape)}" if torch.is_tensor(dst) else type(dst).__name__
        raise ValueError(f"scatter_add_rows: dst must be a contiguous int32 [{R}] tensor, got {got}")
    if feat.device != x.device or gate.device != x.device or dst.device != x.device:
        raise ValueError("scatter_add_rows: all operands must be on one device")
    if x.data_ptr() % 16 or feat.data_ptr() % 16:
        raise ValueError("scatter_add_rows: x / feat must be 16-byte aligned")
    x_bytes = X * n * 2
    for other, nbytes, name in ((feat, A * R * n * 2, "feat"), (gate, 4 * A * R, "gate"), (dst, 4 * R, "dst")):
        if x.data_ptr() < other.data_ptr() + nbytes and other.data_ptr() < x.data_ptr() + x_bytes:
            raise ValueError(f"scatter_add_rows: x overlaps {name}")
    ops._drop_gn_partials(x)
    rc = _lib.load_library().dsc_scatter_add_rows_f16(ops._p(x), ops._p(feat), ops._p(gate), ops._p(dst), X, R, A, n,
                                                      ops._stream_ptr(x))
    _lib.check(rc, "dsc_scatter_add_rows_f16")
    return x


def scatter_add_rows_torch(x, feat, gate, dst):
    """scatter_add_rows in torch ops, for tensors the kernel does not serve (off the GPU, not fp16): the same chain, every product
    and sum rounded to x's dtype on its own, idle lanes and closed nets left out.  Reads gate and dst on the host.  In place;
    returns x."""
    g, d = gate.detach().cpu().tolist(), dst.detach().cpu().tolist()
    active = [v for j, v in enumerate(d) if v >= 0 and any(g[a][j] != 0 for a in range(len(g)))]
    assert len(set(active)) == len(active), f"scatter_add_rows: active lane rows share a destination row: {d}"
    for j, row in enumerate(d):
        if row < 0 or row >= x.shape[0]:
            continue
        t = None
        for a in range(feat.shape[0]):
            if g[a][j] == 0:
                continue
            s = feat[a, j].to(x.dtype) * g[a][j]
            t = s if t is None else t + s
        if t is not None:
            x[row] = x[row] + t
    return x
