"""CPU references of tests/test_guard_bands_gpu.py: the plain fp32 / fp64 statement of every operation the guard-band tests run,
on CPU tensors, with nothing of the GPU library imported (tests/test_guards_host.py runs them on a machine without a GPU).
Operands are fp16-representable values held in fp16 tensors; every function widens them itself."""
import math

import torch
import torch.nn.functional as F

# the resample codes of dsc_conv3x3_nhwc_f16 (include/dsc_hip.h DSC_CONV_*; 0 has no name there)
PLAIN, UPSAMPLE2X, STRIDE2, STRIDE2_PAD_BR, UPSAMPLE_CEIL = 0, 1, 2, 3, 4
PHASE_TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}      # R(py, a) of dsc_conv3x3_up2x_pack_f16


def within(out, ref, rel, floor):
    """|out - ref| <= rel |ref| + floor, element by element"""
    return bool(torch.all((out.detach().cpu().to(ref.dtype) - ref).abs() <= rel * ref.abs() + floor))


def linear(x, w, bias=None, residual=None, dtype=torch.float32):
    """x @ w.T (+ bias) (+ residual row m % R) in fp32 (or `dtype`)"""
    y = x.to(dtype) @ w.to(dtype).t()
    if bias is not None:
        y = y + bias.to(dtype)
    if residual is not None:
        y = y + residual.to(dtype).repeat(x.shape[0] // residual.shape[0], 1)
    return y


def linear_geglu(x, w, bias):
    """hidden * gelu(gate) of the fp32 projection (test_linear_kernel_tilings_agree_bit_for_bit's reference)"""
    y = linear(x, w, bias)
    n = w.shape[0] // 2
    return y[:, :n] * F.gelu(y[:, n:])


def geglu(x):
    hid, gate = x.float().chunk(2, dim=-1)
    return hid * F.gelu(gate)


def row_block_stats(s):
    """[M, N/64, 2] fp64: (sum, sum of squares) of every 64-column block of the fp16 rows `s`, and the same of |values| for
    the error bound of an fp32 summation"""
    v = s.double().reshape(s.shape[0], s.shape[1] // 64, 64)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], dim=-1), torch.stack([v.abs().sum(-1), (v * v).sum(-1)], dim=-1)


def layernorm_linear(s, gamma, beta, w, bias, eps=1e-5, gated=False):
    """LayerNorm(s) @ w.T + bias in fp32 (test_linear_layernorm_folding's reference)"""
    h = F.layer_norm(s.float(), (s.shape[-1],), gamma.float(), beta.float(), eps)
    y = h @ w.float().t() + bias.float()
    if gated:
        hid, gate = y.chunk(2, dim=-1)
        y = hid * F.gelu(gate)
    return y


def head_major(y, B, L, heads):
    """the fused projection y [B L, 3C] as dsc_linear_qkv_f16 lays it out: q [B L, C] and kv [2, B, heads, L, C / heads]"""
    C = y.shape[1] // 3
    q = y[:, :C]
    kv = y[:, C:].reshape(B, L, 2, heads, C // heads).permute(2, 0, 3, 1, 4).contiguous()
    return q, kv


def conv_geometry(mode, h, w):
    """((H, W) the nine taps run over, (oh, ow) stored) for a source image of h x w; UPSAMPLE_CEIL: the 2s - 1 target"""
    if mode == UPSAMPLE2X:
        return (2 * h, 2 * w), (2 * h, 2 * w)
    if mode == UPSAMPLE_CEIL:
        return (2 * h - 1, 2 * w - 1), (2 * h - 1, 2 * w - 1)
    if mode == STRIDE2:
        return (h, w), ((h + 1) // 2, (w + 1) // 2)
    if mode == STRIDE2_PAD_BR:
        return (h, w), (h // 2, w // 2)
    return (h, w), (h, w)


def conv3x3(x, w, bias=None, residual=None, mode=PLAIN, size=None, add=None, dtype=torch.float32):
    """the 3x3 convolution of x [B, Cin, h, w] in the given resample mode (+ bias) (+ add[b, c]) (+ residual), fp32 (or `dtype`), NCHW"""
    xf, wf = x.to(dtype), w.to(dtype)
    bf = None if bias is None else bias.to(dtype)
    if mode == UPSAMPLE2X:
        y = F.conv2d(F.interpolate(xf, scale_factor=2.0, mode="nearest"), wf, bf, padding=1)
    elif mode == UPSAMPLE_CEIL:
        y = F.conv2d(F.interpolate(xf, size=size, mode="nearest"), wf, bf, padding=1)
    elif mode == STRIDE2:
        y = F.conv2d(xf, wf, bf, stride=2, padding=1)
    elif mode == STRIDE2_PAD_BR:
        y = F.conv2d(F.pad(xf, (0, 1, 0, 1)), wf, bf, stride=2)
    else:
        y = F.conv2d(xf, wf, bf, padding=1)
    if add is not None:
        y = y + add.to(dtype)[:, :, None, None]
    if residual is not None:
        y = y + residual.to(dtype)
    return y


def up2x_pack(w):
    """[Cout, Cin, 3, 3] -> [4, Cout, 4, Cin] fp16: fp32 sums, dy ascending (outer) then dx ascending (inner), one rounding"""
    w32 = w.float()
    out = torch.empty((4, w.shape[0], 4, w.shape[1]), dtype=torch.float16)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    acc = None
                    for dy in PHASE_TAPS[(py, a)]:
                        for dx in PHASE_TAPS[(px, b)]:
                            acc = w32[:, :, dy, dx] if acc is None else acc + w32[:, :, dy, dx]
                    out[2 * py + px, :, 2 * a + b, :] = acc.half()
    return out


def rows_of(t):
    """a [B, C, H, W] tensor as channels-last rows [B H W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def groupnorm(x, groups, gamma, beta, eps=1e-5, silu=False, add=None):
    """GroupNorm (+ SiLU) of x [B, C, ...] (+ add[b, c] first) in fp32"""
    xf = x.float()
    if add is not None:
        xf = xf + add.float().reshape(add.shape[0], add.shape[1], *([1] * (x.dim() - 2)))
    y = F.group_norm(xf, groups, gamma.float(), beta.float(), eps)
    return F.silu(y) if silu else y


def groupnorm_ok(y, ref):
    """the GroupNorm tests' bound: max 4e-3 * max(1, |ref|max), mean 4e-4"""
    err = (y.detach().cpu().float() - ref).abs()
    return err.max().item() < 4e-3 * max(1.0, ref.abs().max().item()) and err.mean().item() < 4e-4


def group_sums(out_rows, B, groups):
    """[B, groups, 2] fp64 (sum, sum of squares) per image and group of a channels-last fp16 tensor given as rows [B hw, C]"""
    v = out_rows.double().reshape(B, -1, groups, out_rows.shape[1] // groups)
    return torch.stack([v.sum(dim=(1, 3)), (v * v).sum(dim=(1, 3))], dim=-1)


def straddles(C, groups):
    """per group: does it cross a 64-channel tile boundary (slot [g][1] of the producers' partial sums is live)"""
    cpg = C // groups
    return torch.tensor([(g * cpg) // 64 != ((g + 1) * cpg - 1) // 64 for g in range(groups)])


def add_layernorm(x, a, gamma, beta, eps=1e-5):
    """(the fp16 sum x + a, LayerNorm of it in fp32)"""
    s = x if a is None else (x.float() + a.float()).half()
    return s, F.layer_norm(s.float(), (x.shape[-1],), gamma.float(), beta.float(), eps)


def sinusoid(t, K):
    """diffusers Timesteps(flip_sin_to_cos=True, freq_shift=0) of fp32 t [M], width K, as fp16"""
    half = K // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    return torch.cat([torch.cos(t[:, None] * freqs[None]), torch.sin(t[:, None] * freqs[None])], dim=-1).half()


def linear_rows(x, w, bias=None, silu=False):
    """act(fp16(x @ w.T + bias)) as test_linear_rows_time_embedding states it"""
    y = x.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    return F.silu(y.half().float()) if silu else y


def act_exact(kind, x):
    """quick_gelu / erf gelu of fp16 x in fp64, rounded to fp16 once (numpy: torch would round through fp32)"""
    x64 = x.double()
    y = x64 * torch.sigmoid(1.702 * x64) if kind == "quick_gelu" else x64 * 0.5 * torch.special.erfc(-x64 * 2.0 ** -0.5)
    return torch.from_numpy(y.numpy().astype("float16"))


def ordinal(h):
    """fp16 values as integers in value order (-0 and +0 coincide): differences are distances in ulps"""
    i = h.view(torch.int16).to(torch.int32)
    return torch.where(i >= 0, i, -(i & 0x7FFF))
