"""Inputs, case tables and the error bound of the LoRA merge tests (test_lora_host.py shows the bound on the eager fp32 route on
the CPU, test_lora_gpu.py holds dsc_lora_merge_f16 to it).  A plain module: no fixtures."""
import torch

from diffusionspatialcontrol_amd import ops

# the smallest shapes with each edge: one partial tile, partial row and column tiles (64 x 64 tiles), exactly one tile, three
# row tiles by five column tiles with both edges partial; K always a multiple of 8
SHAPES = [(8, 8), (40, 72), (33, 136), (64, 64), (130, 264)]
# one adapter of each rank (below, at and above one 32-column segment; 4 segments), and two adapters: rank 4 beside rank 32
RANK_SETS = [(1,), (4,), (17,), (32,), (128,), (32, 4)]
GAINS = (0.75, -1.25)            # exact in fp32 (the kernel reads fp32 gains); one per adapter
CANCEL_ROWS = 4                  # leading rows whose base is the rounded negative of the update: base + delta cancels


def case(N, K, ranks, seed, cancel=True):
    """(base fp16 [N, K], [(up fp16 [N, r], down fp16 [r, K], gain)]) on the CPU: weight-like magnitudes (base ~ 0.05, factors
    ~ 0.1); with `cancel`, the first rows of base are -delta rounded to fp16, so the sum is a few fp16 ulps of the operands"""
    g = torch.Generator().manual_seed(seed)
    base = (0.05 * torch.randn(N, K, generator=g)).half()
    adapters = []
    for i, r in enumerate(ranks):
        up = (0.1 * torch.randn(N, r, generator=g)).half()
        down = (0.1 * torch.randn(r, K, generator=g)).half()
        adapters.append((up, down, GAINS[i % len(GAINS)]))
    if cancel:
        rows = min(CANCEL_ROWS, N)
        base[:rows] = (-delta64(adapters)[:rows]).half()
    return base, adapters


def delta64(adapters):
    return sum(g * (up.double() @ down.double()) for up, down, g in adapters)


def exact64(base, adapters):
    return base.double() + delta64(adapters)


def padded_rank(adapters):
    return sum(ops.lora_padded_rank(up.shape[1]) for up, _, _ in adapters)


def ulp16(x):
    """the spacing of fp16 at |x| (fp64 in, fp64 out): 2^(e - 10) in the binade 2^e <= |x| < 2^(e + 1), 2^-24 below 2^-14"""
    _, e = torch.frexp(x.abs())
    e = torch.where(x == 0, torch.full_like(e, -100), e - 1).clamp_min(-14)
    return torch.exp2((e - 10).double())


def bound(base, adapters):
    """ulp16(exact) / 2 + (R_pad + 4) * 2^-24 * (|base| + sum |gain| |up| |down|): one fp16 rounding of the exact value plus the
    fp32 accumulation bound over R_pad products, the gain, the segment adds and the base add"""
    mag = base.double().abs() + sum(abs(g) * (up.double().abs() @ down.double().abs()) for up, down, g in adapters)
    return ulp16(exact64(base, adapters)) / 2 + (padded_rank(adapters) + 4) * 2.0 ** -24 * mag


def violations(got, base, adapters):
    """(count of elements outside the bound, largest error in fp16 ulps of the exact value, share of elements that differ from
    fp64 rounded once)"""
    exact = exact64(base, adapters)
    err = (got.double() - exact).abs()
    bad = int((err > bound(base, adapters)).sum())
    share = float((got != exact.to(torch.float16)).float().mean())
    return bad, float((err / ulp16(exact)).max()), share


def exact_case(N, K, ranks, seed):
    """integer and dyadic operands on which every fp32 product sum, gain product and segment sum is exact: up in {-4..4}, down in
    {-4..4} / 4, gains 0.5 and -2, base multiples of 1/8 up to +-64 - only the final rounding to fp16 is inexact (ties included)"""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randint(-512, 513, (N, K), generator=g).double() / 8).half()
    adapters = []
    for i, r in enumerate(ranks):
        up = torch.randint(-4, 5, (N, r), generator=g).half()
        down = (torch.randint(-4, 5, (r, K), generator=g).double() / 4).half()
        adapters.append((up, down, (0.5, -2.0)[i % 2]))
    return base, adapters


def kernel_job(base, adapters, device="cuda", dst=None):
    """((dst, base, up_cat, down_cat), gains per segment) for ops.lora_merge_: the adapters packed as modules/lora.py packs them"""
    N, K = base.shape
    up, down, owner = ops.lora_pack_adapters([(u, d) for u, d, _ in adapters], N, K, device=device)
    if dst is None:
        dst = torch.full((N, K), float("nan"), dtype=torch.float16, device=device)
    return (dst, base.to(device), up, down), [adapters[i][2] for i in owner]
