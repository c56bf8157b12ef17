"""ops.prompt_weight_rows: the wrapper of dsc_prompt_weight_rows_f16 (csrc/prompt_weight.hip), the one launch behind the text
encoder's captured graph on the text lane of the continuous batcher (modules/serving/text_lane.py); `prompt_weight_numpy`, the
restatement of its contract with exact sums, and `prompt_weight_torch`, the literal eager chain it replaces, for tests and tools."""
import math

import numpy as np
import torch

from . import _lib

MAX_GROUPS = 16                                  # DSC_PROMPT_WEIGHT_MAX_GROUPS (include/dsc_hip.h)


def _ops():
    from . import ops                    # (ops re-exports this module's functions: resolved at call time)
    return ops


def prompt_weight_torch(z, mult):
    """The eager chain the kernel replaces, on any device: FrozenCLIPEmbedderWithCustomWordsBase.process_tokens' tail for one
    chunk and encode_prompt_automatic1111's cast.  z fp16 [2, T, C] (negative and positive row), mult float32 [2, T] -> fp16
    [2, T, C]"""
    before = z.mean()
    p = z * mult.reshape(mult.shape + (1,)).expand(z.shape)
    return (p * (before / p.mean())).to(z.dtype)


def prompt_weight_numpy(z, mult):
    """The kernel's contract restated (include/dsc_hip.h) with exactly rounded sums (math.fsum): z fp16 [2, T, C] and mult
    float32 [2, T] as numpy arrays -> fp16 [2, T, C].  before = fp16(sum z / N), p = fp32(z) * m rounded to fp32, after =
    fp32(sum p / N), ratio = fp32(before) / after in fp32, out = fp16(fp32(p * ratio)); no guard on after == 0."""
    z, mult = np.asarray(z), np.asarray(mult, dtype=np.float32)
    if z.dtype != np.float16 or z.ndim != 3 or z.shape[0] != 2 or mult.shape != z.shape[:2]:
        raise ValueError(f"prompt_weight_numpy: z fp16 [2, T, C] and mult [2, T], got {z.dtype} {z.shape} and {mult.shape}")
    zf = z.astype(np.float32)
    count = float(zf.size)
    with np.errstate(all="ignore"):
        before = np.float16(math.fsum(zf.ravel().tolist()) / count)
        p = zf * mult[:, :, None]
        after = np.float32(math.fsum(p.ravel().tolist()) / count)
        ratio = np.float32(before) / after
        return (p * ratio).astype(np.float16)


def prompt_weight_rows(z, groups):
    """Up to 16 (request, chunk) groups of the encoder's output -> their weighted, mean-restored fp16 rows, in ONE launch on the
    current stream (dsc_prompt_weight_rows_f16).  z: fp16 [m, T, C] contiguous on the GPU.  groups: a list with, per group, None
    (idle: neither read nor written) or a dict of
        rows   (i, j): the group's negative and positive row of z
        mult   fp32 [2, T] contiguous on z's GPU: one multiplier per token of either row
        out    (negative, positive): two fp16 [T, C] tensors with unit column stride and ONE row stride ldo >= C for every group
               of the call (views of a request's [S, C] rows), 16-byte aligned, ldo % 8 == 0
    C % 8 == 0."""
    ops = _ops()
    ops._require_gpu(z)
    if z.dtype != torch.float16:
        raise TypeError(f"prompt_weight_rows: z must be fp16, got {z.dtype}")
    if z.dim() != 3 or min(z.shape) < 1 or not z.is_contiguous():
        raise ValueError(f"prompt_weight_rows: z must be a contiguous [m, T, C], got {tuple(z.shape)} with strides {z.stride()}")
    if not isinstance(groups, (list, tuple)) or not 1 <= len(groups) <= MAX_GROUPS:
        raise ValueError(f"prompt_weight_rows: groups must be a list of 1 to {MAX_GROUPS} groups, got "
                         f"{len(groups) if isinstance(groups, (list, tuple)) else type(groups).__name__}")
    m, T, C = (int(v) for v in z.shape)
    if C % 8:
        raise ValueError(f"prompt_weight_rows: C = {C} must be a multiple of 8")
    ldo = None
    recs = (_lib.PromptWeightGroup * len(groups))()
    for j, g in enumerate(groups):
        if g is None:
            continue
        unknown = set(g) - {"rows", "mult", "out"}
        if unknown or set(g) != {"rows", "mult", "out"}:
            raise ValueError(f"prompt_weight_rows: group {j} takes `rows`, `mult` and `out`, got {sorted(g)}")
        rows, mult, out = g["rows"], g["mult"], g["out"]
        if len(rows) != 2 or any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < m for i in rows):
            raise ValueError(f"prompt_weight_rows: group {j} reads rows {rows!r} of z, which has {m}")
        if not torch.is_tensor(mult) or mult.dtype != torch.float32 or tuple(mult.shape) != (2, T) or not mult.is_contiguous() \
                or mult.device != z.device:
            raise ValueError(f"prompt_weight_rows: group {j}: mult must be a contiguous fp32 [2, {T}] on {z.device}")
        if len(out) != 2:
            raise ValueError(f"prompt_weight_rows: group {j}: out is a (negative, positive) pair")
        for o in out:
            if not torch.is_tensor(o) or o.dtype != torch.float16 or tuple(o.shape) != (T, C) or o.device != z.device \
                    or o.stride(1) != 1:
                raise ValueError(f"prompt_weight_rows: group {j}: a destination must be fp16 [{T}, {C}] with unit column stride on "
                                 f"{z.device}, got {tuple(o.shape) if torch.is_tensor(o) else type(o).__name__}")
            ld = int(o.stride(0)) if T > 1 else (ldo if ldo is not None else C)
            if ldo is None:
                ldo = ld
            if ld != ldo or ld < C or ld % 8 or o.data_ptr() % 16:
                raise ValueError(f"prompt_weight_rows: group {j}: every destination of a call has one row stride >= C that is a "
                                 f"multiple of 8, and is 16-byte aligned (got stride {ld}, the call's {ldo})")
        if out[0].data_ptr() == out[1].data_ptr():
            raise ValueError(f"prompt_weight_rows: group {j}: both destinations are one tensor")
        rec = recs[j]
        rec.z_row[0], rec.z_row[1] = int(rows[0]), int(rows[1])
        rec.mult = mult.data_ptr()
        rec.out[0], rec.out[1] = out[0].data_ptr(), out[1].data_ptr()
    if ldo is None:
        ldo = C
    _lib.check(_lib.load_library().dsc_prompt_weight_rows_f16(ops._p(z), m, T, C, recs, len(groups), ldo, ops._stream_ptr(z)),
               "dsc_prompt_weight_rows_f16")
