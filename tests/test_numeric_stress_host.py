"""The helpers of tests/numeric_ref.py checked on the CPU, before a GPU sees the inputs they build: the references against
torch's own fp32 operators, the attention emulation's floor under its caps, the staircase logits bit for bit, and the GroupNorm
inputs fair at every (offset, sigma) - the fp64 result rounded to fp16, i.e. a perfect kernel, sits inside the bound."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import numeric_ref as nr
from oracle import region_attention as ra


def test_ulp16_and_the_fp16_sweep():
    assert nr.ulp16(1.0) == 2.0 ** -10 and nr.ulp16(1.999) == 2.0 ** -10 and nr.ulp16(2.0) == 2.0 ** -9
    assert nr.ulp16(1000.0) == 0.5 and nr.ulp16(-60000.0) == 32.0
    assert nr.ulp16(2.0 ** -14) == 2.0 ** -24 and nr.ulp16(1e-6) == 2.0 ** -24 and nr.ulp16(0.0) == 2.0 ** -24
    a = nr.all_finite_fp16()
    assert a.numel() == 63488 and torch.isfinite(a).all() and a.dtype == torch.float16
    assert a.view(torch.int16).unique().numel() == 63488                       # both zeros included, nothing twice
    f = a.double().numpy()
    with np.errstate(over="ignore"):                                           # (65504 steps to inf; excluded below)
        nxt = np.nextafter(a.numpy(), np.float16(np.inf)).astype(np.float64)
    pos = (f > 0) & (f < 65504)
    assert np.array_equal((nxt - f)[pos], nr.ulp16(f)[pos])                     # spacing towards the next value up


def test_gelu64_against_torch():
    x = nr.all_finite_fp16()
    ref = F.gelu(x.double())
    got = nr.gelu64(x)
    assert torch.all((got - ref).abs() <= 1e-15 * ref.abs() + 1e-300) or (got - ref).abs().max().item() < 1e-12
    tail = torch.tensor([-8.0, -12.0, -30.0])
    assert torch.all(nr.gelu64(tail) <= 0) and nr.gelu64(tail)[0].item() == pytest.approx(-8.0 * 0.5 * math.erfc(8 / math.sqrt(2)), rel=1e-12)
    assert torch.equal(nr.geglu64(torch.tensor([2.0]), torch.tensor([0.5])), 2.0 * nr.gelu64(torch.tensor([0.5])))


def test_norm_references_against_torch_fp32():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 24, 5, 3, generator=g).half()
    add = torch.randn(2, 24, generator=g).half()
    gamma, beta = torch.randn(24, generator=g).half(), torch.randn(24, generator=g).half()
    for act in (False, True):
        ref = F.group_norm(x.float() + add.float()[:, :, None, None], 4, gamma.float(), beta.float(), 1e-5)
        ref = F.silu(ref) if act else ref
        assert (nr.groupnorm64(x, 4, gamma, beta, 1e-5, act, add=add) - ref).abs().max().item() < 2e-5
    rows = torch.randn(7, 64, generator=g).half()
    lg, lb = torch.randn(64, generator=g).half(), torch.randn(64, generator=g).half()
    assert (nr.layernorm64(rows, lg, lb) - F.layer_norm(rows.float(), (64,), lg.float(), lb.float(), 1e-5)).abs().max().item() < 2e-5
    s = (torch.randn(3, 40, generator=g) * 6).half()
    assert (nr.softmax64(s, 0.37) - torch.softmax(s.float() * 0.37, -1)).abs().max().item() < 1e-6


def test_attention_references_against_torch_fp32_and_the_oracle():
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, n, 3, 16, generator=g).half() for n in (9, 13, 13))
    ref = F.scaled_dot_product_attention(q.float().transpose(1, 2), k.float().transpose(1, 2), v.float().transpose(1, 2)).transpose(1, 2)
    assert (nr.attention64(q, k, v) - ref).abs().max().item() < 1e-5
    assert (nr.attention_emulated(q, k, v) - ref).abs().max().item() < 1e-3                 # unit Gaussians: the roundings are small
    w = torch.randn(2, 9, 13, generator=g)
    qh, kh, vh = (t.transpose(1, 2) for t in (q, k, v))
    for ng in (1, 2):
        exp = ra.region_attention(qh, kh, vh, w, 2.0, n_std_groups=ng)
        assert (nr.region_attention64(qh, kh, vh, w, 2.0, n_std_groups=ng) - exp).abs().max().item() < 1e-5
    io = torch.randn(2, 9, 48, generator=g).half()
    wq = torch.rand(2, 9, generator=g).half()
    o = ref.reshape(2, 9, 48).double()
    assert (nr.ip_restated64(q, k, v, io, [0.5, -1.0], wq) - (io.double() + torch.tensor([0.5, -1.0]).view(2, 1, 1) * wq.double().view(2, 9, 1) * o)).abs().max().item() < 1e-5


@pytest.mark.parametrize("gain", nr.ATTN_GAINS)
@pytest.mark.parametrize("B,H,L,S,d,seed", nr.ATTN_CASES + [nr.VARIANT_CASE, nr.ROTATED_BASE])
def test_emulated_attention_floor_stays_under_its_cap(B, H, L, S, d, seed, gain):
    """floor = max |attention_emulated - fp64|: what the kernel's documented roundings alone cost at these logits.  The GPU test
    allows the kernel twice this floor; the cap keeps the floor itself honest (a seed over the cap is replaced, the cap is not)."""
    q, k, v, ref, emu, floor = nr.attention_case(B, H, L, S, d, gain, seed)
    top = nr.max_logit(q, k)
    print(f"B={B} H={H} L={L} S={S} d={d} gain={gain}: max |s| {top:.1f}, floor {floor:.3e} (cap {nr.FLOOR_CAP[gain]:.1e})")
    assert floor <= nr.FLOOR_CAP[gain], floor
    assert top > (12.0 if gain == 2 else 27.0)                 # the logits do reach the range the case is named for
    assert torch.equal(nr.prescaled_q(q).float(), (q.float() * float(nr.kernel_scale_log2e(d))).half().float())


def test_rotated_case_is_the_base_case_laid_out_per_head():
    q, k, v, ref, emu, floor = nr.rotated_case(2)
    bq, bk, bv, bref, bemu, bfloor = nr.attention_case(*nr.ROTATED_BASE[:5], 2, nr.ROTATED_BASE[5])
    B, H = nr.ROTATED_BH
    assert q.shape == (B, 256, H, 40) and k.shape == (B, 200, H, 40) and floor == bfloor
    assert B * H * ((q.shape[1] + 255) // 256) >= 256                           # the launch rule of the rotated-stagger image
    for b, h in ((0, 0), (3, 2), (15, 15)):
        j = (b + h) % 4
        assert torch.equal(q[b, :, h], bq[0, :, j]) and torch.equal(k[b, :, h], bk[0, :, j]) and torch.equal(v[b, :, h], bv[0, :, j])
        assert torch.equal(ref[b, :, h], bref[0, :, j]) and torch.equal(emu[b, :, h], bemu[0, :, j])


@pytest.mark.parametrize("S", [129, 191, 256])
@pytest.mark.parametrize("d", [40, 64])
def test_staircase_logits_are_exact(S, d):
    steps = nr.staircase_patterns(S)
    q, k, v, logits = nr.staircase_qkv(64, S, d, steps)
    c2 = float(nr.kernel_scale_log2e(d, nr.STAIRCASE_SCALE))
    assert abs(c2 - 1.0) <= 2.0 ** -23
    qs = nr.prescaled_q(q, nr.STAIRCASE_SCALE)
    got = torch.einsum("blhd,bshd->bhls", qs.double(), k.double())[0, 0]
    assert torch.equal(got, logits)                                             # bit for bit after the pre-scale
    ntile = (S + 63) // 64
    for p_, row in enumerate(steps):
        for t in range(ntile):
            assert logits[p_, t * 64:min((t + 1) * 64, S)].max().item() == row[t]                   # the tile maximum is the level
    assert logits[0].max().item() == 9.0 * (ntile - 1) and logits[3, :(ntile - 1) * 64].max().item() == 0.0
    assert torch.equal(v[0, :, 0, :].sum(-1), torch.ones(S, dtype=torch.float16))               # V one-hot per key
    # the emulation and fp64 agree on these inputs up to the fp16 rounding of P: nothing else rounds
    ref = nr.attention64(q, k, v, nr.STAIRCASE_SCALE)
    emu = nr.attention_emulated(q, k, v, nr.STAIRCASE_SCALE)
    assert (emu - ref).abs().max().item() < 1e-3 and abs(ref.sum(-1) - 1).max().item() < 1e-12


def test_staircase_refuses_inexact_levels():
    with pytest.raises(AssertionError):
        nr.staircase_qkv(8, 64, 40, [[0.1]])                                   # 0.1 is not an fp16 value


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("offset,sigma", nr.OFFSET_SIGMA)
def test_groupnorm_inputs_are_fair(offset, sigma, with_add):
    """a perfect kernel (fp64, one fp16 rounding of the result) sits inside the GroupNorm bound at every (offset, sigma), so a
    miss on the GPU is the kernel's; and the inputs do have the structure they claim"""
    B, C, h, w, G = 2, 64, 12, 12, 8
    x, add, gamma, beta = nr.offset_groupnorm_inputs(B, C, h, w, G, offset, sigma, seed=3, with_add=with_add)
    xin = x.double() + (add.double()[:, :, None, None] if with_add else 0.0)
    grp = xin.reshape(B, G, -1)
    assert torch.all(grp[:, 0] == 1.0)                                          # the constant group: variance exactly 0
    ratio = (grp.mean(-1).abs() / grp.std(-1).clamp_min(1e-30))[:, 1::2]
    assert ratio.min().item() > 0.8 * offset / sigma and torch.all(grp.mean(-1)[:, 1::4] > 0) and torch.all(grp.mean(-1)[:, 3::4] < 0)
    assert (grp.mean(-1)[:, 2::2].abs() < 3 * sigma).all()
    assert torch.equal(nr.channel_offsets(C, G, offset)[8:16], torch.full((8,), offset))
    for act in (False, True):
        ref = nr.groupnorm64(x, G, gamma, beta, 1e-5, act, add=add)
        mx, mean, bound = nr.gn_errors(ref.half(), ref)
        assert mx < bound and mean < nr.GN_MEAN, (mx, mean, bound)
        ref32 = F.group_norm(xin.float(), G, gamma.float(), beta.float(), 1e-5)
        ref32 = F.silu(ref32) if act else ref32
        assert (ref32.double() - ref).abs().max().item() < 2e-3                # torch's fp32 operator agrees with the fp64 one


@pytest.mark.parametrize("offset,sigma", nr.OFFSET_SIGMA)
def test_layernorm_inputs_are_fair(offset, sigma):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(6, 320, generator=g) * sigma)
    x[::2] += offset
    x[1] -= offset
    x = x.half()
    gamma, beta = (torch.randn(320, generator=g) * 0.3 + 1).half(), (torch.randn(320, generator=g) * 0.2).half()
    ref = nr.layernorm64(x, gamma, beta)
    assert torch.all((ref.half().double() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3)
