"""High-precision CPU references and input builders for the activation-like stress tests (tests/test_numeric_stress_*.py):
channels that sit tens to hundreds of standard deviations from zero, attention logits in the tens, a running maximum that is
placed tile by tile, and every finite fp16 value through GELU.

Everything here is fp64 torch / numpy on the CPU.  `attention_emulated` restates the roundings the header comment of
csrc/self_attn.hip documents (Q times scale * log2 e rounded to fp16, exp2(s - max) rounded to fp16, the row sum taken over the
rounded values) and nothing else of the kernel: no tiles, no lazy maximum, no MFMA summation order."""
import functools
import math

import numpy as np
import torch

LOG2E_F32 = np.float32(1.4426950408889634)
LN2 = math.log(2.0)

# (channel offset, standard deviation) of the GroupNorm / LayerNorm stress inputs.  mean / sigma = 17, 86, 240, 286, 200; the
# first two are the range in which every form, the producer-statistics ones included, is held to the bound; fp16 spacing at 1000
# is 0.5, hence sigma = 5 there.
OFFSET_SIGMA = [(12.0, 0.7), (60.0, 0.7), (60.0, 0.25), (200.0, 0.7), (1000.0, 5.0)]
MODERATE = OFFSET_SIGMA[:2]            # mean / sigma <= ~100
GN_MAX_REL, GN_MEAN = 4e-3, 4e-4       # the suite's GroupNorm bound: max err < 4e-3 * max(1, |ref|max), mean err < 4e-4


# ----------------------------------------------------------------------------- fp16 spacing
def ulp16(x):
    """spacing of fp16 at |x| (numpy array or scalar, any float type): 2^(floor(log2 |x|) - 10) for normal values, the subnormal
    spacing 2^-24 below 2^-14 (and at 0)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(e - 10.0)


def all_finite_fp16():
    """every finite fp16 value once (63 488 of them: both signs of zero, the subnormals, up to +-65504), as an fp16 torch tensor"""
    bits = np.arange(1 << 16, dtype=np.uint16)
    bits = bits[(bits & 0x7C00) != 0x7C00]                       # exponent field all ones: inf / NaN
    return torch.from_numpy(bits.view(np.float16).copy())


# ----------------------------------------------------------------------------- normalisations
def groupnorm64(x, groups, gamma, beta, eps, act, add=None):
    """GroupNorm(+ per-(b, c) add first)(+ SiLU) of x [B, C, ...] in fp64 (biased variance, as torch.nn.functional.group_norm)"""
    B, C = x.shape[0], x.shape[1]
    xd = x.double().reshape(B, C, -1)
    if add is not None:
        xd = xd + add.double().reshape(B, C, 1)
    g = xd.reshape(B, groups, -1)
    mean = g.mean(dim=2, keepdim=True)
    var = ((g - mean) ** 2).mean(dim=2, keepdim=True)
    y = ((g - mean) / torch.sqrt(var + eps)).reshape(B, C, -1)
    y = y * gamma.double().reshape(1, C, 1) + beta.double().reshape(1, C, 1)
    if act:
        y = y * torch.sigmoid(y)
    return y.reshape(x.shape)


def layernorm64(x, gamma, beta, eps=1e-5):
    """LayerNorm over the last dimension in fp64"""
    xd = x.double()
    mean = xd.mean(dim=-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=-1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def offset_groupnorm_inputs(B, C, h, w, groups, offset, sigma, seed, with_add=False):
    """(x fp16 [B, C, h, w], add fp16 [B, C] or None, gamma, beta): x = randn * sigma + offset_c.  Every second group carries the
    offset, alternately +offset and -offset, the others stay around zero; group 0 is exactly constant (x + add == 1 there: variance
    0, rstd = 1 / sqrt(eps)).  The constant group sits in an un-offset group on purpose: GroupNorm as scale and shift per channel,
    y = x * (gamma * rstd) + (beta - mean * gamma * rstd), carries the fp32 rounding of |mean| * rstd = 1000 * 316 there, which is a
    property of that corner (a constant far from zero), not of the statistics this input is after."""
    g = torch.Generator().manual_seed(seed)
    cpg = C // groups
    x = torch.randn(B, C, h, w, generator=g) * sigma
    for gi in range(1, groups, 2):
        x[:, gi * cpg:(gi + 1) * cpg] += offset if gi % 4 == 1 else -offset
    add = None
    if with_add:
        add = torch.randn(B, C, generator=g) * 0.5 * sigma       # (per channel: it widens the group, so it scales with sigma)
        add[:, :cpg] = 0.25
    x[:, :cpg] = 0.75 if with_add else 1.0
    gamma = (torch.randn(C, generator=g) * 0.5 + 1).half()
    beta = (torch.randn(C, generator=g) * 0.3).half()
    return x.half(), (add.half() if with_add else None), gamma, beta


def channel_offsets(C, groups, offset):
    """the per-channel offsets of offset_groupnorm_inputs as a [C] tensor (for producers that add them as a bias)"""
    cpg = C // groups
    o = torch.zeros(C)
    for gi in range(1, groups, 2):
        o[gi * cpg:(gi + 1) * cpg] = offset if gi % 4 == 1 else -offset
    return o


def gn_errors(y, ref):
    """(max err, mean err, max bound) of the suite's GroupNorm check: max err < 4e-3 * max(1, |ref|max), mean err < 4e-4"""
    err = (y.double().cpu() - ref).abs()
    return err.max().item(), err.mean().item(), GN_MAX_REL * max(1.0, ref.abs().max().item())


# ----------------------------------------------------------------------------- attention, softmax, GEGLU
def attention64(q, k, v, scale=None):
    """softmax(scale * q k^T) v in fp64; q [B, L, H, d], k / v [B, S, H, d] -> [B, L, H, d]"""
    d = q.shape[-1]
    sc = 1.0 / math.sqrt(d) if scale is None else float(scale)
    s = torch.einsum("blhd,bshd->bhls", q.double(), k.double()) * sc
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhls,bshd->blhd", p, v.double())


def kernel_scale_log2e(d, scale=None):
    """scale * log2 e as dsc_self_attn_fwd forms it: in fp32, the default scale being 1.0f / sqrtf(d)"""
    sc = np.float32(1.0) / np.sqrt(np.float32(d)) if scale is None else np.float32(scale)
    return np.float32(sc * LOG2E_F32)


def prescaled_q(q, scale=None):
    """q * (scale * log2 e) rounded back to fp16, the operand of the kernel's QK^T product (fp16 tensor)"""
    c2 = float(kernel_scale_log2e(q.shape[-1], scale))
    return (q.float() * torch.tensor(c2, dtype=torch.float32)).half()


def attention_emulated(q, k, v, scale=None):
    """attention64 with the kernel's documented roundings only: s = fp16(q * scale * log2 e) . k (log2 units, exact sums),
    p = fp16(exp2(s - rowmax)), out = sum p v / sum p over the rounded p.  fp64 everywhere else."""
    s = torch.einsum("blhd,bshd->bhls", prescaled_q(q, scale).double(), k.double())
    p = torch.exp2(s - s.amax(dim=-1, keepdim=True)).half().double()
    return torch.einsum("bhls,bshd->blhd", p, v.double()) / p.sum(dim=-1).permute(0, 2, 1).unsqueeze(-1)


@functools.lru_cache(maxsize=None)
def attention_case(B, H, L, S, d, gain, seed):
    """(q, k, v fp16; fp64 reference; emulation; floor = max |emulation - fp64|) for q, k = randn * gain, v = randn.  Computed
    once per case and shared (treat as read-only)."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, L, H, d, generator=g) * gain).half()
    k = (torch.randn(B, S, H, d, generator=g) * gain).half()
    v = torch.randn(B, S, H, d, generator=g).half()
    ref, emu = attention64(q, k, v), attention_emulated(q, k, v)
    return q, k, v, ref, emu, (emu - ref).abs().max().item()


# The large-logit attention cases: (B, H, L, S, d, seed).  A seed is kept only if the emulation's floor stays under the cap at
# both gains (tests/test_numeric_stress_host.py asserts it); the cap never moves.
ATTN_GAINS = (2, 3)                    # q, k = randn * gain: max |s| ~ 20 and ~ 45
FLOOR_CAP = {2: 2.5e-3, 3: 8e-3}
ATTN_CASES = [(1, 2, 128, 128, 40, 4), (1, 2, 96, 200, 64, 1), (1, 2, 64, 130, 80, 5), (1, 1, 64, 257, 160, 4)]
VARIANT_CASE = (1, 2, 300, 200, 40, 2)     # one shape for every forced tiling: two 8-wave workgroups per head, ragged last key tile
# The d = 40 rotated-stagger image is chosen from B * H * ceil(L / 256) >= 256 workgroups; L = 256 is the smallest L at which all
# eight computing waves of a workgroup own query rows.  256 (batch, head) pairs of four distinct heads: the floor is a maximum over
# rows, and 65 536 independent rows would exceed any cap that 1024 rows meet.
ROTATED_BASE, ROTATED_BH = (1, 4, 256, 200, 40, 4), (16, 16)


def rotated_case(gain):
    """attention_case(ROTATED_BASE) laid out as [16, L, 16, d]: head h of batch row b is base head (b + h) % 4"""
    q, k, v, ref, emu, floor = attention_case(*ROTATED_BASE[:5], gain, ROTATED_BASE[5])
    B, H = ROTATED_BH
    idx = (torch.arange(B).view(B, 1) + torch.arange(H).view(1, H)) % q.shape[2]               # [B, H]

    def lay(t):
        return t[0][:, idx].permute(1, 0, 2, 3).contiguous()                                   # [L, B, H, d] -> [B, L, H, d]
    return lay(q), lay(k), lay(v), lay(ref), lay(emu), floor


def max_logit(q, k, scale=None):
    d = q.shape[-1]
    sc = 1.0 / math.sqrt(d) if scale is None else float(scale)
    return (torch.einsum("blhd,bshd->bhls", q.double(), k.double()) * sc).abs().max().item()


def region_attention64(q, k, v, w, sigma, n_std_groups=1):
    """oracle/region_attention.py::region_attention without rounding emulation, restated in fp64: q [Bc, H, L, d], k / v
    [Bc, H, S, d], w [Bw, L, S]; bias = w * sigma * std(scores of the row's std group), unbiased std"""
    Bc, H, L, d = q.shape
    S = k.shape[-2]
    a = (q.double() @ k.double().transpose(-2, -1)) / math.sqrt(d)
    grp = a.reshape(Bc // n_std_groups, n_std_groups, -1).transpose(0, 1).reshape(n_std_groups, -1)
    std = grp.std(dim=1, unbiased=True)
    wrow = torch.repeat_interleave(w.double(), (Bc * H) // w.shape[0], dim=0).reshape(Bc, H, L, S)
    a = a + wrow * float(sigma) * std[torch.arange(Bc) % n_std_groups].reshape(Bc, 1, 1, 1)
    return torch.softmax(a, dim=-1) @ v.double()


def ip_restated64(q, k, v, io, row_scale, weight=None):
    """io + row_scale[b] * weight[b, l] * softmax(q k^T / sqrt d) v, the formula of dsc_ip_xattn_add(_masked)_f16 in fp64;
    q [B, L, H, d], k / v [B, T, H, d], io [B, L, H * d]"""
    B, L, H, d = q.shape
    o = attention64(q, k, v).reshape(B, L, H * d)
    if weight is not None:
        o = o * weight.double().reshape(B, L, 1)
    return io.double() + torch.tensor(row_scale, dtype=torch.float64).view(B, 1, 1) * o


def softmax64(scores, scale=1.0):
    return torch.softmax(scores.double() * float(scale), dim=-1)


def gelu64(x):
    """x / 2 * (1 + erf(x / sqrt 2)) in fp64; the negative side through erfc (no 1 - erf cancellation)"""
    xd = x.double()
    return 0.5 * xd * torch.special.erfc(-xd / math.sqrt(2.0))


def geglu64(hid, gate):
    return hid.double() * gelu64(gate)


# ----------------------------------------------------------------------------- prescribed logits
STAIRCASE_SCALE = LN2          # with it the kernel's scale * log2 e is 1 up to an fp32 ulp: a logit IS its value in log2 units


def staircase_qkv(L, S, d, steps, tile=64):
    """q [1, L, 1, d], k / v [1, S, 1, d] fp16 whose attention logits are prescribed exactly, and those logits [L, S] (log2 units,
    fp64) - to be run with scale = STAIRCASE_SCALE.

    steps[p][t] is the level (log2 units) of pattern p in key tile t (tiles of `tile` keys, the last one ragged): key j of the tile
    gets level - jitter_j with jitter_j in {0, 1/8, .., 7/8} and jitter 0 on the tile's first key, so the tile's maximum is the
    level itself.  Query row i follows pattern i % len(steps): q[i] is the unit vector of channel i % len(steps) and k[s] carries
    pattern p's logit of key s in channel p, so s[i, s] = k[s, i % P] with nothing to round.  V is one-hot per key (channel s % d):
    the output row is the probability row, folded modulo d.

    Asserted here: the levels are fp16 values, and q survives the kernel's pre-scale (q * fp32(scale * log2 e) rounded to fp16)
    unchanged - so the products the kernel forms are the prescribed logits bit for bit."""
    P = len(steps)
    ntile = (S + tile - 1) // tile
    assert P <= d and all(len(row) == ntile for row in steps), (P, d, ntile)
    jitter = torch.tensor([((5 * j) % 8) / 8.0 for j in range(tile)], dtype=torch.float64)
    logits = torch.empty(P, S, dtype=torch.float64)
    for p_, row in enumerate(steps):
        for t, level in enumerate(row):
            n = min(tile, S - t * tile)
            logits[p_, t * tile:t * tile + n] = float(level) - jitter[:n]
    assert torch.equal(logits.half().double(), logits), "levels must be exactly representable in fp16"
    k = torch.zeros(1, S, 1, d, dtype=torch.float16)
    k[0, :, 0, :P] = logits.t().half()
    q = torch.zeros(1, L, 1, d, dtype=torch.float16)
    q[0, torch.arange(L), 0, torch.arange(L) % P] = 1.0
    v = torch.zeros(1, S, 1, d, dtype=torch.float16)
    v[0, torch.arange(S), 0, torch.arange(S) % d] = 1.0
    assert torch.equal(prescaled_q(q, STAIRCASE_SCALE), q), "q must survive the kernel's pre-scale exactly"
    return q, k, v, logits[torch.arange(L) % P]


def staircase_patterns(S, tile=64):
    """the four running-maximum patterns of the stress tests for S keys in tiles of `tile` (levels per tile, log2 units):
    0 climbs 9 per tile (above the kernel's lazy-rescale threshold of 8: every tile rescales); 1 climbs 7.5 above tile 0 and stays
    (below the threshold: no rescale on its own, P ~ 181 in fp16 and many of them summed); 2 has its maximum in tile 0 and every
    later key 30 below; 3 has its maximum only in the last (ragged) tile, 20 above everything before."""
    n = (S + tile - 1) // tile
    return [[9.0 * t for t in range(n)],
            [0.0] + [7.5] * (n - 1),
            [0.0] + [-30.0] * (n - 1),
            [0.0] * (n - 1) + [20.0]]
