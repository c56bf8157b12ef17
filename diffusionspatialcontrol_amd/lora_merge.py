"""LoRA merge over a table of weights (dsc_lora_merge_f16, csrc/lora_merge.hip): the wrapper beside its kernel's name, reached as
ops.lora_merge_ / ops.LoraMergeTable / ops.lora_merge_takes; lora_merge_eager is the reference's arithmetic in torch
(app.py:583-590: `W += alpha * mm(up.float(), down.float())`), the route of CPU, fp32 / fp64 weights, shapes outside the
kernel's limits and DSC_LORA=0.

A job is (dst, base, up, down): `dst` the live weight, [N, K] with unit inner stride (a strided view is allowed) or a contiguous
1x1-conv weight [N, K, 1, 1]; `base` its pristine fp16 copy; `up` [N, R] and `down` [R, K] the job's adapters concatenated along
the rank, each padded to a multiple of SEGMENT (pack_adapters).  Gains: one fp32 per segment."""
import ctypes
import os

import torch

from . import _lib

SEGMENT = 32            # DSC_LORA_SEGMENT (include/dsc_hip.h): rank columns of one v_mfma_f32_16x16x32_f16
MAX_RANK = 256          # DSC_LORA_MAX_RANK: the padded ranks of all adapters of one weight
USE_LORA_KERNEL = os.environ.get("DSC_LORA", "1") != "0"   # A/B switch: 0 = every merge through lora_merge_eager


def padded_rank(rank):
    return (rank + SEGMENT - 1) // SEGMENT * SEGMENT


def lora_merge_takes(weight, ranks):
    """dsc_lora_merge_f16's limits (stated in include/dsc_hip.h) for one weight and the ranks of its adapters: an fp16 GPU
    Linear / 1x1-conv weight with 16-byte rows, at most MAX_RANK padded rank columns in all"""
    if not (USE_LORA_KERNEL and weight.is_cuda and weight.dtype == torch.float16 and weight.is_contiguous()):
        return False
    if weight.dim() not in (2, 4) or (weight.dim() == 4 and tuple(weight.shape[2:]) != (1, 1)):
        return False
    total = sum(padded_rank(r) for r in ranks)
    return weight.shape[1] % 8 == 0 and weight.data_ptr() % 16 == 0 and 0 < total <= MAX_RANK


def pack_adapters(adapters, N, K, device=None):
    """[(up [N, r], down [r, K]), ...] -> (up_cat fp16 [N, R], down_cat fp16 [R, K], owner): every adapter's rank padded with zero
    columns / rows to a multiple of SEGMENT, owner[s] the index of the adapter segment s belongs to.  fp32 / fp64 tensors are
    rounded to fp16 here."""
    ups, downs, owner = [], [], []
    for i, (up, down) in enumerate(adapters):
        r = up.shape[1]
        if tuple(up.shape) != (N, r) or tuple(down.shape) != (r, K) or r < 1:
            raise ValueError(f"pack_adapters: up {tuple(up.shape)} and down {tuple(down.shape)} do not form a [{N}, {K}] update")
        rp = padded_rank(r)
        u = torch.zeros(N, rp, dtype=torch.float16, device=device if device is not None else up.device)
        d = torch.zeros(rp, K, dtype=torch.float16, device=u.device)
        u[:, :r] = up.to(device=u.device, dtype=torch.float16)
        d[:r] = down.to(device=u.device, dtype=torch.float16)
        ups.append(u)
        downs.append(d)
        owner += [i] * (rp // SEGMENT)
    return torch.cat(ups, dim=1).contiguous(), torch.cat(downs, dim=0).contiguous(), owner


def _dst_2d(dst):
    if dst.dim() == 4:
        if tuple(dst.shape[2:]) != (1, 1) or not dst.is_contiguous():
            raise ValueError(f"lora_merge: a 4-D destination must be a contiguous 1x1-conv weight, got {tuple(dst.shape)}")
        return dst.detach().view(dst.shape[0], dst.shape[1])
    if dst.dim() != 2 or dst.stride(1) != 1:
        raise ValueError(f"lora_merge: the destination must be [N, K] with unit inner stride, got {tuple(dst.shape)}")
    return dst.detach()


class LoraMergeTable:
    """A checked and numbered job table: the host records (dsc_lora_job, tile0 filled by dsc_lora_merge_plan), their device copy
    and the fp32 gain buffer the records point into.  Built once per set of adapters; a rescale writes `gains` and launches."""

    def __init__(self, jobs):
        if not jobs:
            raise ValueError("lora_merge: an empty job table")
        dev = jobs[0][0].device
        self.jobs = [tuple(j) for j in jobs]                          # keeps every operand alive
        self.segments = []
        views = []
        for dst, base, up, down in self.jobs:
            for t in (dst, base, up, down):
                if not t.is_cuda or t.device != dev:
                    raise _lib.DscLibraryError("lora_merge: the kernel route takes GPU tensors of one device (lora_merge_eager "
                                               "is the other route)")
                if t.dtype != torch.float16:
                    raise TypeError("lora_merge: fp16 only")
            d2 = _dst_2d(dst)
            N, K = d2.shape
            R = up.shape[1]
            if tuple(base.shape[:2]) != (N, K) or base.numel() != N * K or tuple(up.shape) != (N, R) or tuple(down.shape) != (R, K):
                raise ValueError(f"lora_merge: dst {tuple(dst.shape)}, base {tuple(base.shape)}, up {tuple(up.shape)} and down "
                                 f"{tuple(down.shape)} do not fit together")
            if not (base.is_contiguous() and up.is_contiguous() and down.is_contiguous()):
                raise ValueError("lora_merge: base, up and down must be contiguous")
            if R % SEGMENT != 0:
                raise ValueError(f"lora_merge: the rank {R} is not padded to a multiple of {SEGMENT} (pack_adapters)")
            views.append(d2)
            self.segments.append(R // SEGMENT)
        self.n_segments = sum(self.segments)
        self.gains = torch.zeros(self.n_segments, dtype=torch.float32, device=dev)
        self.host = (_lib.LoraJob * len(self.jobs))()
        seg0 = 0
        for rec, d2, (dst, base, up, down), nseg in zip(self.host, views, self.jobs, self.segments):
            rec.base, rec.dst, rec.up, rec.down = base.data_ptr(), d2.data_ptr(), up.data_ptr(), down.data_ptr()
            rec.gain = self.gains.data_ptr() + 4 * seg0
            rec.N, rec.K, rec.R, rec.ld_dst = d2.shape[0], d2.shape[1], up.shape[1], d2.stride(0) if d2.shape[0] > 1 else d2.shape[1]
            seg0 += nseg
        self.tiles = _lib.load_library().dsc_lora_merge_plan(self.host, len(self.jobs))
        if self.tiles < 0:
            _lib.check(int(self.tiles), "dsc_lora_merge_plan")
        raw = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8)
        self.device_table = raw.to(dev)


def lora_merge_(jobs, gains):
    """dst <- fp16(base + sum_seg gain[seg] * up[:, seg] @ down[seg]) for every job, in ONE launch (dsc_lora_merge_f16).  `jobs`: a
    LoraMergeTable or a list of (dst, base, up, down); `gains`: one float per segment, job after job, flat or one sequence per
    job.  Afterwards every written tensor's version counter is incremented, so the `_version`-keyed caches (derived weights,
    the time-embedding table's signature, GroupNorm partial sums, CLIPTextModel's fused QKV) rebuild by themselves."""
    table = jobs if isinstance(jobs, LoraMergeTable) else LoraMergeTable(jobs)
    flat = []
    for g in gains:
        flat += [float(v) for v in g] if isinstance(g, (list, tuple)) else [float(g)]
    if len(flat) != table.n_segments:
        raise ValueError(f"lora_merge_: {len(flat)} gains for {table.n_segments} segments")
    table.gains.copy_(torch.tensor(flat, dtype=torch.float32))
    rc = _lib.load_library().dsc_lora_merge_f16(table.host, ctypes.c_void_p(table.device_table.data_ptr()), len(table.jobs), 0,
                                                ctypes.c_void_p(torch.cuda.current_stream(table.gains.device).cuda_stream))
    _lib.check(rc, "dsc_lora_merge_f16")
    for dst, _, _, _ in table.jobs:
        torch.autograd.graph.increment_version(dst)
    return table


def lora_merge_eager(dst, base, adapters):
    """The reference's arithmetic for one weight, from its pristine copy: dst <- cast(base.float() + sum_i gain_i * mm(up_i.float(),
    down_i.float())), adapters = [(up [N, r], down [r, K], gain)] in order (fp64 weights: the same in fp64).  A gain of 0 is
    skipped, as the kernel skips it.  In place, through copy_: the version counter moves by itself."""
    acc_t = torch.float64 if dst.dtype == torch.float64 else torch.float32
    N, K = dst.shape[0], dst.shape[1]
    with torch.no_grad():
        total = None
        for up, down, gain in adapters:
            if float(gain) == 0.0:
                continue
            delta = float(gain) * torch.mm(up.to(device=dst.device, dtype=acc_t).reshape(N, -1),
                                           down.to(device=dst.device, dtype=acc_t).reshape(-1, K))
            total = delta if total is None else total + delta
        w = base.to(acc_t).reshape(N, K)
        if total is not None:
            w = w + total
        dst.copy_(w.reshape(dst.shape).to(dst.dtype))
    return dst
