"""GPU parity of the UNet-step kernels (GroupNorm+SiLU, GEGLU, fused sampler step), of the UNet forward and of
the 25-step denoising loop against the CPU oracle (torch fp32 restatement) on identical weights and inputs."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from inputs import FakeTokenizer, prompt_ids, rect_map
from oracle import k_diffusion_ref as kd
from oracle import unet_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("B,C,h,w,G,act,eps", [(2, 320, 64, 64, 32, True, 1e-5), (2, 2560, 16, 16, 32, True, 1e-5),
                                               (2, 64, 2, 2, 8, True, 1e-5), (1, 40, 3, 5, 8, False, 1e-5),
                                               (2, 1280, 8, 8, 32, False, 1e-6), (1, 32, 4, 4, 8, True, 1e-5),
                                               (16, 640, 32, 32, 32, True, 1e-5), (3, 96, 6, 4, 8, False, 1e-5)])
def test_groupnorm_silu(ops, B, C, h, w, G, act, eps):
    g = torch.Generator().manual_seed(B * C + h)
    x = (torch.randn(B, C, h, w, generator=g) * 1.7 + 0.6).half()
    gamma, beta = (torch.randn(C, generator=g) * 0.5 + 1).half(), (torch.randn(C, generator=g) * 0.3).half()
    ref = F.group_norm(x.float(), G, gamma.float(), beta.float(), eps)
    ref = F.silu(ref) if act else ref
    y = ops.groupnorm_silu(x.cuda(), G, gamma.cuda(), beta.cuda(), eps, act)
    err = (y.float().cpu() - ref).abs()
    assert err.max().item() < 4e-3 * max(1.0, ref.abs().max().item()), err.max().item()   # fp16 output rounding
    assert err.mean().item() < 4e-4
    assert torch.equal(y, ops.groupnorm_silu(x.cuda(), G, gamma.cuda(), beta.cuda(), eps, act))   # reproducible


@pytest.mark.parametrize("B,C,h,w,G,act,with_add", [(2, 320, 64, 64, 32, True, True), (2, 2560, 16, 16, 32, True, False),
                                                    (2, 1280, 8, 8, 32, False, False), (1, 32, 2, 2, 8, True, True),
                                                    (16, 640, 32, 32, 32, True, True), (3, 64, 5, 3, 8, False, True),
                                                    (2, 1920, 32, 32, 32, True, False), (2, 960, 64, 64, 32, True, True),
                                                    (2, 2560, 8, 8, 32, True, True), (2, 1280, 16, 16, 32, True, True),
                                                    (2, 2560, 16, 16, 32, True, False), (4, 1280, 8, 8, 32, False, True),
                                                    # single-launch bundle kernel: 10 / 20 / 30 / 40 / 60 channels per group
                                                    (2, 640, 32, 32, 32, True, True), (2, 960, 32, 32, 32, True, False),
                                                    (2, 320, 32, 32, 32, False, True), (2, 1280, 32, 32, 32, True, True),
                                                    (2, 1920, 16, 16, 32, True, True), (2, 640, 16, 16, 32, True, False),
                                                    (3, 96, 24, 24, 8, True, True), (1, 48, 7, 9, 4, False, False)])
def test_groupnorm_silu_nhwc(ops, B, C, h, w, G, act, with_add):
    g = torch.Generator().manual_seed(B * C + h + 1)
    x = (torch.randn(B, C, h, w, generator=g) * 1.7 + 0.6).half()
    add = (torch.randn(B, C, generator=g) * 0.8).half() if with_add else None
    gamma, beta = (torch.randn(C, generator=g) * 0.5 + 1).half(), (torch.randn(C, generator=g) * 0.3).half()
    xin = x.float() + (add.float()[:, :, None, None] if with_add else 0.0)
    ref = F.group_norm(xin, G, gamma.float(), beta.float(), 1e-5)
    ref = F.silu(ref) if act else ref
    xc = x.cuda().contiguous(memory_format=torch.channels_last)
    y = ops.groupnorm_silu_nhwc(xc, G, gamma.cuda(), beta.cuda(), 1e-5, act, add=add.cuda() if with_add else None)
    assert y.shape == x.shape and y.is_contiguous(memory_format=torch.channels_last)
    err = (y.float().cpu() - ref).abs()
    assert err.max().item() < 4e-3 * max(1.0, ref.abs().max().item()), err.max().item()
    assert err.mean().item() < 4e-4
    tok = xc.permute(0, 2, 3, 1).reshape(B, h * w, C)            # token-major view gives the same bytes
    y2 = ops.groupnorm_silu_nhwc(tok, G, gamma.cuda(), beta.cuda(), 1e-5, act, add=add.cuda() if with_add else None)
    assert torch.equal(y2.reshape(B, h, w, C).permute(0, 3, 1, 2), y)
    # the other launch forms of the two-pass kernels (no channel slabs; fine row chunks + finalize launch): same numbers up to
    # the grouping of the fp32 / fp64 partial sums
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    try:
        for mode in (10, 4):
            lib.dsc_debug_set_gn_mode(mode)
            ym = ops.groupnorm_silu_nhwc(xc, G, gamma.cuda(), beta.cuda(), 1e-5, act, add=add.cuda() if with_add else None)
            assert (ym.float() - y.float()).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item()), mode
    finally:
        lib.dsc_debug_set_gn_mode(11)
        lib.dsc_debug_set_gn_mode(0)


@pytest.mark.parametrize("B,C1,C2,h,w,G,act", [(2, 1280, 1280, 8, 8, 32, True),      # single-launch kernel
                                                (2, 1280, 1280, 16, 16, 32, True), (2, 1280, 640, 16, 16, 32, True),
                                                (2, 1280, 640, 32, 32, 32, True), (2, 640, 320, 32, 32, 32, True),
                                                (2, 640, 320, 64, 64, 32, True), (2, 320, 320, 64, 64, 32, True),   # finalize launch
                                                (16, 320, 320, 64, 64, 32, True), (3, 40, 24, 5, 7, 8, False),
                                                (1, 8, 56, 3, 3, 4, True), (2, 1280, 1280, 12, 12, 32, True)])
def test_groupnorm_of_concatenation(ops, B, C1, C2, h, w, G, act):
    """dsc_groupnorm_silu_nhwc_cat: GroupNorm over [x1 | x2] with the concatenation as a by-product of the statistics pass.
    Same arithmetic as the plain kernel on the materialised concatenation -> bit-equal; the concatenation is a byte copy."""
    g = torch.Generator().manual_seed(C1 + C2 + h)
    cl = torch.channels_last
    x1 = (torch.randn(B, C1, h, w, generator=g) * 1.3 + 0.2).half().cuda().contiguous(memory_format=cl)
    x2 = (torch.randn(B, C2, h, w, generator=g) * 0.7 - 0.4).half().cuda().contiguous(memory_format=cl)
    gamma = (torch.randn(C1 + C2, generator=g) * 0.5 + 1).half().cuda()
    beta = (torch.randn(C1 + C2, generator=g) * 0.3).half().cuda()
    assert ops.groupnorm_cat_covers(x1, x2)
    y, cat = ops.groupnorm_silu_nhwc_cat(x1, x2, G, gamma, beta, 1e-5, act)
    want_cat = torch.cat([x1, x2], dim=1).contiguous(memory_format=cl)
    assert cat.is_contiguous(memory_format=cl) and torch.equal(cat, want_cat)
    assert torch.equal(y, ops.groupnorm_silu_nhwc(want_cat, G, gamma, beta, 1e-5, act))
    add = (torch.randn(B, C1 + C2, generator=g) * 0.8).half().cuda()            # the fused per-(b, c) term rides along
    y_add, cat_add = ops.groupnorm_silu_nhwc_cat(x1, x2, G, gamma, beta, 1e-5, act, add=add)
    assert torch.equal(cat_add, want_cat) and torch.equal(y_add, ops.groupnorm_silu_nhwc(want_cat, G, gamma, beta, 1e-5, act, add=add))
    ref = F.group_norm(want_cat.float(), G, gamma.float(), beta.float(), 1e-5)
    ref = F.silu(ref) if act else ref
    assert (y.float() - ref).abs().max().item() < 4e-3 * max(1.0, ref.abs().max().item())


def test_groupnorm_of_concatenation_rejects(ops):
    x1 = torch.randn(1, 12, 4, 4).half().cuda().contiguous(memory_format=torch.channels_last)      # 12 % 8 != 0
    x2 = torch.randn(1, 20, 4, 4).half().cuda().contiguous(memory_format=torch.channels_last)
    assert not ops.groupnorm_cat_covers(x1, x2)
    with pytest.raises(ValueError):
        ops.groupnorm_silu_nhwc_cat(x1, x2, 4, torch.ones(32).half().cuda(), torch.zeros(32).half().cuda(), 1e-5, True)


@pytest.mark.parametrize("B,H,L,d", [(2, 8, 4096, 40), (2, 8, 1024, 80), (2, 8, 256, 160), (2, 8, 64, 160),
                                     (1, 4, 100, 64), (2, 10, 576, 64), (3, 5, 33, 16), (2, 8, 144, 160), (1, 2, 2304, 40),
                                     (2, 20, 1024, 64), (1, 1, 1, 8), (2, 8, 9216, 40), (2, 8, 4000, 40), (16, 8, 1024, 80)])
def test_self_attention(ops, B, H, L, d):
    """flash self-attention vs torch fp32 softmax(QK^T/sqrt(d))V on the same fp16-representable inputs.
    Tolerance: P is packed to fp16 for the PV MFMA and the output is fp16: 2e-3 absolute on |out| <= ~1."""
    g = torch.Generator().manual_seed(L * d + H)
    qkv = torch.randn(B, L, 3 * H * d, generator=g).half()
    C = H * d
    q, k, v = (qkv[..., i * C:(i + 1) * C].unflatten(-1, (H, d)) for i in range(3))     # strided views of a fused QKV
    ref = F.scaled_dot_product_attention(q.float().transpose(1, 2), k.float().transpose(1, 2), v.float().transpose(1, 2))
    ref = ref.transpose(1, 2)
    qc = qkv.cuda()
    qd, kd, vd = (qc[..., i * C:(i + 1) * C].unflatten(-1, (H, d)) for i in range(3))
    out = ops.self_attention(qd, kd, vd)
    assert out.shape == (B, L, H, d) and out.is_contiguous()
    err = (out.float().cpu() - ref).abs()
    assert err.max().item() < 2e-3, err.max().item()
    assert err.mean().item() < 2e-4
    assert torch.equal(out, ops.self_attention(qd, kd, vd))
    # a spiked key forces the online-softmax rescale branch late in the sweep (cdna guide rule 26)
    if L >= 128:
        k2 = k.clone()
        k2[:, L - 5] = q[:, 3] * 4.0
        ref2 = F.scaled_dot_product_attention(q.float().transpose(1, 2), k2.float().transpose(1, 2),
                                              v.float().transpose(1, 2)).transpose(1, 2)
        out2 = ops.self_attention(q.cuda(), k2.cuda(), v.cuda())
        assert (out2.float().cpu() - ref2).abs().max().item() < 3e-3


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18])
@pytest.mark.parametrize("B,H,L,d", [(2, 8, 4096, 40), (2, 10, 1000, 64), (1, 8, 520, 80), (2, 4, 300, 32), (3, 8, 77, 40), (2, 8, 256, 160)])
def test_self_attention_tiling_variants(ops, variant, B, H, L, d):
    """every tiling of the flash kernel, forced through dsc_debug_set_self_attn_variant: 1 = 4 waves per workgroup, 2 = 8 waves
    (two per SIMD from ONE workgroup), 3 = 4 waves with a three-waves-per-SIMD register budget - the configuration that
    faulted in round 1, when the K / V tiles were staged through registers the compiler could not see being written; the
    tiles now arrive by LDS-DMA -, 4 / 5 = 4 / 8 computing waves + a loader wave, 6 / 7 = + two loader waves, 8 / 9 / 10 = the
    compact d = 40 image (other head dims fall through to the automatic choice).  Same fp32 SDPA reference and tolerance as test_self_attention, incl. the rescale branch."""
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    if (3 <= variant <= 14 or variant >= 17) and d > 64:
        pytest.skip("three waves per SIMD / one- and two-loader kernels: head dims <= 64 only")
    g = torch.Generator().manual_seed(L * d + H + variant)
    q, k, v = (torch.randn(B, L, H, d, generator=g).half() for _ in range(3))
    k[:, L - 7] = q[:, 5] * 4.0                       # a late spike: the running max moves near the end of the sweep
    ref = F.scaled_dot_product_attention(q.float().transpose(1, 2), k.float().transpose(1, 2), v.float().transpose(1, 2)).transpose(1, 2)
    lib.dsc_debug_set_self_attn_variant(variant)
    try:
        out = ops.self_attention(q.cuda(), k.cuda(), v.cuda())
        again = ops.self_attention(q.cuda(), k.cuda(), v.cuda())
    finally:
        lib.dsc_debug_set_self_attn_variant(0)
    err = (out.float().cpu() - ref).abs()
    # the spiked rows' outputs are single value rows of magnitude up to ~4.5, where one fp16 ulp is 3.9e-3: 4e-3 absolute
    assert err.max().item() < 4e-3 and err.mean().item() < 2e-4, (err.max().item(), err.mean().item())
    assert torch.equal(out, again)


@pytest.mark.parametrize("M,R,N,K", [(8192, 4096, 320, 320), (2048, 1024, 640, 640), (768, 256, 1280, 1280), (8192, 2048, 320, 1280)])
def test_linear_wraps_a_residual_of_fewer_rows(ops, M, R, N, K):
    """dsc_linear_f16 / _ln_f16 / _gn_f16 with ldr = stride | (R << 32): row m adds residual row m % R (the residual stream of the
    layers in front of the first cross-attention exists once per image, the result once per CFG branch) - the same bytes as with
    the residual repeated"""
    g = torch.Generator().manual_seed(M + R + N)
    x = (torch.randn(M, K, generator=g) * 0.5).half().cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).half().cuda()
    b = torch.randn(N, generator=g).half().cuda()
    r = torch.randn(R, N, generator=g).half().cuda()
    full = r.repeat(M // R, 1)
    a = ops.linear(x, w, b, residual=r, prefer_kernel=True)
    e = ops.linear(x, w, b, residual=full, prefer_kernel=True)
    assert torch.equal(a, e)
    a_ln, st_a = ops.linear_ln(x, w, b, residual=r, ln_stats=True)
    e_ln, st_e = ops.linear_ln(x, w, b, residual=full, ln_stats=True)
    assert torch.equal(a_ln, e_ln) and torch.equal(st_a, st_e)
    if M >= 1024:
        got_a = ops.linear_gn(x.view(2, M // 2, K), w, b, r.view(1, R, N) if M // 2 == R else r, M // 2, 32)
        got_e = ops.linear_gn(x.view(2, M // 2, K), w, b, full.view(2, M // 2, N), M // 2, 32)
        if got_a is not None and got_e is not None:
            assert torch.equal(got_a[0], got_e[0]) and torch.equal(got_a[1].buf[..., 0, :], got_e[1].buf[..., 0, :])   # (slot 1: straddling groups only)
    # a row count the tiles cannot wrap: repeated on the host, same result
    r_odd = torch.randn(M // 2 if (M // 2) % 128 else 64, N, generator=g).half().cuda()
    if M % r_odd.shape[0] == 0:
        assert torch.equal(ops.linear(x, w, b, residual=r_odd, prefer_kernel=True),
                           ops.linear(x, w, b, residual=r_odd.repeat(M // r_odd.shape[0], 1), prefer_kernel=True))


@pytest.mark.parametrize("S", [1, 3, 4, 5, 59, 60, 61, 63, 64, 65, 67, 68, 69, 124, 127, 128, 129, 132])
@pytest.mark.parametrize("d,L", [(40, 4096), (64, 96)])
def test_attention_key_count_edges(ops, S, d, L):
    """the ragged last key tile of the flash kernel is masked with lane masks built from scalar compares (lanes 0-31 hold key c,
    lanes 32-63 key c + 4 of every score element): key counts on both sides of the 64-key tile edge and of the lane-half offset,
    on the rotated-stagger kernel (d = 40, 4096 query rows) and a plain one"""
    g = torch.Generator().manual_seed(S * 131 + d)
    B, H = 2, 8
    q = torch.randn(B, L, H, d, generator=g).half().cuda()
    k = torch.randn(B, S, H, d, generator=g).half().cuda()
    v = torch.randn(B, S, H, d, generator=g).half().cuda()
    k, v = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (k, v))     # head-major, as the QKV projection writes them
    out = ops.self_attention(q, k, v)
    ref = F.scaled_dot_product_attention(q.float().transpose(1, 2), k.float().transpose(1, 2), v.float().transpose(1, 2)).transpose(1, 2)
    err = (out.float() - ref).abs()
    assert torch.isfinite(out).all() and err.max().item() < 3e-3, err.max().item()


@pytest.mark.parametrize("B,H,L,S,d", [(2, 8, 4096, 257, 40), (2, 8, 256, 257, 160), (1, 8, 1024, 77, 80), (2, 5, 64, 300, 64)])
def test_attention_keys_differ_from_queries(ops, B, H, L, S, d):
    """dsc_self_attn_fwd with S != L (a ragged last key tile): the IP-Adapter image-token attention of the 257-token variants"""
    g = torch.Generator().manual_seed(L + S)
    q = torch.randn(B, L, H, d, generator=g).half().cuda()
    k = torch.randn(B, S, H, d, generator=g).half().cuda()
    v = torch.randn(B, S, H, d, generator=g).half().cuda()
    out = ops.self_attention(q, k, v)
    ref = F.scaled_dot_product_attention(q.float().transpose(1, 2), k.float().transpose(1, 2), v.float().transpose(1, 2)).transpose(1, 2)
    err = (out.float() - ref).abs()
    assert out.shape == (B, L, H, d) and err.max().item() < 4e-3 and err.mean().item() < 3e-4, (err.max().item(), err.mean().item())


@pytest.mark.parametrize("M,N,K", [(8192, 320, 320), (8192, 960, 320), (8192, 320, 1280), (2048, 640, 640), (2048, 640, 2560),
                                   (512, 1280, 1280), (512, 3840, 1280), (300, 64, 64), (8192, 320, 960), (256, 1280, 5120)])
def test_linear_kernel(ops, M, N, K):
    """dsc_linear_f16 vs fp32 matmul on fp16-representable operands: one fp16 rounding of the fp32 result."""
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    b = (torch.randn(N, generator=g) * 0.2).half()
    r = torch.randn(M, N, generator=g).half()
    ref = x.float() @ w.float().t() + b.float() + r.float()
    xd, wd, bd, rd = x.cuda(), w.cuda(), b.cuda(), r.cuda()
    out = ops.linear(xd, wd, bd, residual=rd)
    assert out.shape == (M, N)
    assert torch.all((out.float().cpu() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3)
    out2 = ops.linear(xd, wd, None)
    ref2 = x.float() @ w.float().t()
    assert torch.all((out2.float().cpu() - ref2).abs() <= 1.5e-3 * ref2.abs() + 2e-3)
    assert torch.equal(out, ops.linear(xd, wd, bd, residual=rd))
    # strided activation rows (a [B, L, 3C] slice) and 3-D input
    big = torch.randn(2, M // 2, K + 64, generator=g).half().cuda()
    xv = big[..., :K]
    o3 = ops.linear(xv, wd, bd)
    ref3 = xv.float().cpu() @ w.float().t() + b.float()
    assert o3.shape == (2, M // 2, N)
    assert torch.all((o3.float().cpu() - ref3).abs() <= 1.5e-3 * ref3.abs() + 2e-3)


@pytest.mark.parametrize("M,N,K", [(128, 64, 64), (128, 64, 1920)])
def test_linear_with_a_bias_the_kernels_cannot_read(ops, M, N, K):
    """a bias at a 2-byte offset (the library refuses it) takes the torch route instead of raising, at dsc_linear_f16's shape and at
    the split-K one; test_linear_kernel's bound (one fp16 rounding of the fp32 result)"""
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    b = (torch.randn(N + 1, generator=g) * 0.2).half()
    ref = x.float() @ w.float().t() + b[1:].float()
    out = ops.linear(x.cuda(), w.cuda(), b.cuda()[1:])
    assert out.shape == (M, N)
    assert torch.all((out.float().cpu() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3)


@pytest.mark.parametrize("B,Cin,Cout,H,W,splits", [
    (2, 320, 320, 64, 64, 0), (2, 640, 320, 64, 64, 0), (2, 640, 640, 32, 32, 0), (2, 640, 640, 32, 32, 1),
    (2, 1920, 640, 32, 32, 0), (2, 1280, 1280, 16, 16, 0), (2, 2560, 1280, 16, 16, 0), (2, 1280, 1280, 8, 8, 0),
    (2, 2560, 1280, 8, 8, 0), (1, 64, 64, 8, 8, 0), (3, 128, 64, 8, 8, 2), (1, 64, 128, 16, 24, 0), (2, 192, 64, 24, 48, 3),
    (1, 320, 320, 96, 96, 0), (5, 64, 64, 8, 16, 0),
    # image sides that are not multiples of the pixel tile (the 12 x 12 level of a 768 x 768 generation)
    (2, 1280, 1280, 12, 12, 0), (16, 1280, 1280, 12, 12, 0), (2, 128, 64, 12, 20, 2), (1, 64, 64, 5, 7, 0), (3, 64, 128, 9, 30, 0),
    (1, 64, 64, 1, 1, 0)])
def test_conv3x3_kernel(ops, B, Cin, Cout, H, W, splits):
    """dsc_conv3x3_nhwc_f16 vs an fp32 convolution on fp16-representable operands (one fp16 rounding of the fp32 sum):
    image borders (zero padding), 16- and 8-wide tiles, ragged last tile, split input-channel ranges, bias + residual."""
    g = torch.Generator().manual_seed(B * 7 + Cin + Cout + H + W)
    cl = torch.channels_last
    x = torch.randn(B, Cin, H, W, generator=g).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).half()
    b = (torch.randn(Cout, generator=g) * 0.2).half()
    r = torch.randn(B, Cout, H, W, generator=g).half()
    xd, wd = x.cuda().contiguous(memory_format=cl), w.cuda().contiguous(memory_format=cl)
    bd, rd = b.cuda(), r.cuda().contiguous(memory_format=cl)
    assert ops.conv3x3_supported(xd, wd)
    ref = F.conv2d(xd.float(), wd.float(), bd.float(), padding=1).cpu()
    out = ops.conv3x3(xd, wd, bd, splits=splits)
    assert out.shape == (B, Cout, H, W) and out.is_contiguous(memory_format=cl)
    err = (out.float().cpu() - ref).abs()
    assert torch.all(err <= 1.5e-3 * ref.abs() + 2e-3), err.max().item()
    out_r = ops.conv3x3(xd, wd, bd, residual=rd, splits=splits)
    ref_r = ref + r.float()
    assert torch.all((out_r.float().cpu() - ref_r).abs() <= 1.5e-3 * ref_r.abs() + 2e-3)
    out_n = ops.conv3x3(xd, wd, None, splits=splits)
    ref_n = ref - b.float().view(1, -1, 1, 1)
    assert torch.all((out_n.float().cpu() - ref_n).abs() <= 1.5e-3 * ref_n.abs() + 2e-3)
    assert torch.equal(out, ops.conv3x3(xd, wd, bd, splits=splits))          # bit-reproducible, split or not
    # a localised impulse: every tap lands where it should (catches halo / tap-offset indexing independent of tolerance)
    xi = torch.zeros(B, Cin, H, W).half()
    xi[B - 1, 5, H - 1, 0] = 1.0
    xi[0, Cin - 1, min(3, H - 1), W - 1] = 2.0
    oi = ops.conv3x3(xi.cuda().contiguous(memory_format=cl), wd, None, splits=splits).float().cpu()
    ri = F.conv2d(xi.float(), w.float(), None, padding=1)
    assert torch.all((oi - ri).abs() <= 1e-3 * ri.abs() + 1e-6)


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 1280, 1280, 16, 16), (2, 1280, 1280, 8, 8), (2, 640, 640, 32, 32), (1, 64, 128, 16, 24)])
def test_conv3x3_and_gemm_profiles_give_equal_bytes(ops, B, Cin, Cout, H, W):
    """dsc_set_tuning_profile: the latency rules (nine-stage convolution ring for small grids, GEMM loader waves) and the
    throughput rules launch different kernels that add in the same order - equal bytes; so does a forced ring depth"""
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    g = torch.Generator().manual_seed(Cin + Cout + H)
    cl = torch.channels_last
    x = torch.randn(B, Cin, H, W, generator=g).half().cuda().contiguous(memory_format=cl)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).half().cuda().contiguous(memory_format=cl)
    b = (torch.randn(Cout, generator=g) * 0.2).half().cuda()
    xt = torch.randn(B * H * W, Cin, generator=g).half().cuda()
    wt = (torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin)).half().cuda()
    outs = {}
    try:
        for prof in ("latency", "throughput"):
            ops.set_tuning_profile(prof)
            assert ops.tuning_profile() == prof
            outs[prof] = (ops.conv3x3(x, w, b), ops.linear(xt, wt, b) if ops.linear_kernel_covers(B * H * W, Cout, Cin, torch.float16) else None)
        for ring in (3, 9):
            lib.dsc_debug_set_conv_ring(ring)
            outs[ring] = (ops.conv3x3(x, w, b), None)
        lib.dsc_debug_set_conv_ring(400)                      # the nine-stage kernel without / with its loader waves
        outs["9 plain"] = (ops.conv3x3(x, w, b), None)
        lib.dsc_debug_set_conv_ring(402)
        outs["9 loaders"] = (ops.conv3x3(x, w, b), None)
    finally:
        lib.dsc_debug_set_conv_ring(401)
        lib.dsc_debug_set_conv_ring(0)
        ops.set_tuning_profile("latency")
    for k in ("throughput", 3, 9, "9 plain", "9 loaders"):
        assert torch.equal(outs[k][0], outs["latency"][0]), k
    if outs["latency"][1] is not None:
        assert torch.equal(outs["throughput"][1], outs["latency"][1])


@pytest.mark.parametrize("B,C,Cout,h,w", [(2, 1280, 1280, 8, 8), (2, 640, 640, 32, 32), (1, 64, 64, 4, 12), (3, 128, 64, 4, 4),
                                          (2, 1280, 1280, 12, 12), (1, 64, 64, 3, 5)])
def test_conv3x3_upsample(ops, B, C, Cout, h, w):
    """Upsample2D: nearest 2x + conv (diffusers) == the convolution reading the small image through the upsampling map"""
    g = torch.Generator().manual_seed(B + C + h + w)
    cl = torch.channels_last
    x = torch.randn(B, C, h, w, generator=g).half().cuda().contiguous(memory_format=cl)
    wt = (torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(9 * C)).half().cuda().contiguous(memory_format=cl)
    b = (torch.randn(Cout, generator=g) * 0.2).half().cuda()
    assert ops.conv3x3_supported(x, wt, upsample=True)
    out = ops.conv3x3(x, wt, b, upsample=True)
    up = F.interpolate(x, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(up.float(), wt.float(), b.float(), padding=1)
    assert out.shape == (B, Cout, 2 * h, 2 * w)
    assert torch.all((out.float() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3)
    assert torch.equal(out, ops.conv3x3(up, wt, b))                        # same sums in the same order


@pytest.mark.parametrize("M,N,K,geglu", [(8192, 320, 320, False), (512, 1280, 1280, False), (2048, 640, 2560, False), (130, 1280, 1280, False),
                                          (77, 320, 768, False), (2048, 5120, 640, True), (512, 10240, 1280, True), (8192, 2560, 320, True)])
def test_linear_kernel_tilings_agree_bit_for_bit(ops, M, N, K, geglu):
    """gemm_tn_f16's launch variants (dsc_debug_set_gemm_stages: ring depth 2 / 3, 64- / 128-row tiles, with and without the four
    DMA-only loader waves) form the same sums in the same order: equal bytes, and right against fp32."""
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    g = torch.Generator().manual_seed(M + N + K)
    x = (torch.randn(M, K, generator=g) * 0.5).half().cuda()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
    b = (torch.randn(N, generator=g) * 0.2).half().cuda()
    r = torch.randn(M, N // 2 if geglu else N, generator=g).half().cuda()
    saved = (ops.DSC_GEMM_MIN_ROWS, ops.DSC_GEMM_MAX_K, ops.DSC_GEMM_MID_ROWS, ops.DSC_GEMM_MID_K)
    ops.DSC_GEMM_MIN_ROWS, ops.DSC_GEMM_MAX_K, ops.DSC_GEMM_MID_ROWS, ops.DSC_GEMM_MID_K = 1, 1 << 30, 1, 1 << 30
    outs = {}
    try:
        assert ops.linear_kernel_covers(M, N, K, torch.float16, geglu=geglu)
        # 1xxxxx: never the 128-column tile, 2xxxxx: wherever N is a multiple of 128 (GEGLU: the default where the grid allows)
        # [12]xxxxxx: workgroup order plain / XCD-aware
        for knob in (0, 90003, 40003, 90002, 91283, 41283, 100000, 200000, 291282, 1000000, 2000000, 2200000) + (() if geglu else (90643, 40643, 90642)):
            lib.dsc_debug_set_gemm_stages(knob)
            outs[knob] = ops.linear(x, w, b, geglu=True) if geglu else ops.linear(x, w, b, residual=r)
    finally:
        lib.dsc_debug_set_gemm_stages(0)
        ops.DSC_GEMM_MIN_ROWS, ops.DSC_GEMM_MAX_K, ops.DSC_GEMM_MID_ROWS, ops.DSC_GEMM_MID_K = saved
    ref = F.linear(x.float(), w.float(), b.float())
    ref = ref[:, :N // 2] * F.gelu(ref[:, N // 2:]) if geglu else ref + r.float()
    for knob, o in outs.items():
        assert torch.equal(o, outs[0]), knob
    assert torch.all((outs[0].float() - ref).abs() <= 2e-3 * ref.abs() + 3e-3)


@pytest.mark.parametrize("M", [1, 2, 5, 8])
def test_linear_rows_time_embedding(ops, M):
    """dsc_linear_rows_f16: sinusoidal Timesteps + linear_1 + SiLU, linear_2 + SiLU, the stacked time_emb_proj GEMV"""
    g = torch.Generator().manual_seed(M)
    t = (torch.rand(M, generator=g) * 999.0).float()
    half = 160
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    emb = torch.cat([torch.cos(t[:, None] * freqs[None]), torch.sin(t[:, None] * freqs[None])], dim=-1).half()
    w1 = (torch.randn(1280, 320, generator=g) / math.sqrt(320)).half()
    b1 = (torch.randn(1280, generator=g) * 0.1).half()
    w2 = (torch.randn(1280, 1280, generator=g) / math.sqrt(1280)).half()
    b2 = (torch.randn(1280, generator=g) * 0.1).half()
    h_ref = F.silu((emb.float() @ w1.float().t() + b1.float()).half().float()).half()
    h = ops.linear_rows(t.cuda(), w1.cuda(), b1.cuda(), silu_out=True, sinusoid_dim=320)
    assert h.shape == (M, 1280)
    # one timestep expanded over the batch (a scheduler's 0-dim timestep: stride 0, and its neighbour in memory is the NEXT timestep)
    both = torch.tensor([float(t[0]), 3.0]).cuda()
    he = ops.linear_rows(both[0:1].expand(M), w1.cuda(), b1.cuda(), silu_out=True, sinusoid_dim=320)
    assert all(torch.equal(he[m], h[0]) for m in range(M))
    assert torch.all((h.float().cpu() - h_ref.float()).abs() <= 2e-3 * h_ref.float().abs() + 2e-3), (h.float().cpu() - h_ref.float()).abs().max()
    y_ref = F.silu((h_ref.float() @ w2.float().t() + b2.float()).half().float())
    y = ops.linear_rows(h_ref.cuda(), w2.cuda(), b2.cuda(), silu_out=True)
    assert torch.all((y.float().cpu() - y_ref).abs() <= 2e-3 * y_ref.abs() + 2e-3)
    w3 = (torch.randn(18560 // 8, 1280, generator=g) / math.sqrt(1280)).half()      # a slice of the stacked time_emb_proj
    z_ref = h_ref.float() @ w3.float().t()
    big = torch.zeros(M, 1288).half()
    big[:, :1280] = h_ref
    z = ops.linear_rows(big.cuda()[:, :1280], w3.cuda())                          # strided rows, no bias, no activation
    assert torch.all((z.float().cpu() - z_ref).abs() <= 2e-3 * z_ref.abs() + 2e-3)


@pytest.mark.parametrize("B,Cin,Cout,H,W,nchw", [(2, 320, 4, 64, 64, True), (1, 64, 4, 8, 8, True), (2, 128, 40, 16, 16, False),
                                                 (1, 64, 100, 8, 16, False), (2, 64, 72, 8, 8, True)])
def test_conv3x3_ragged_cout_and_nchw(ops, B, Cin, Cout, H, W, nchw):
    """conv_out (320 -> 4, channel-major result) and other channel counts that are not multiples of 64: the ragged
    channel tile reads zero weight rows through the buffer bounds"""
    g = torch.Generator().manual_seed(Cin + Cout + H)
    cl = torch.channels_last
    x = torch.randn(B, Cin, H, W, generator=g).half().cuda().contiguous(memory_format=cl)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).half().cuda().contiguous(memory_format=cl)
    b = (torch.randn(Cout, generator=g) * 0.2).half().cuda()
    assert ops.conv3x3_supported(x, w)
    ref = F.conv2d(x.float(), w.float(), b.float(), padding=1)
    out = ops.conv3x3(x, w, b, out_nchw=nchw)
    assert out.shape == ref.shape and (out.is_contiguous() if nchw else out.is_contiguous(memory_format=cl))
    assert torch.all((out.float() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3), (out.float() - ref).abs().max().item()
    assert torch.equal(out, ops.conv3x3(x, w, b, out_nchw=nchw))


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 4, 320, 64, 64), (1, 4, 320, 96, 96), (3, 8, 64, 8, 16), (1, 3, 128, 16, 8)])
def test_conv3x3_fewcin(ops, B, Cin, Cout, H, W):
    """conv_in: channel-major latents -> channels-last features, bias fused, zero padding at the borders"""
    g = torch.Generator().manual_seed(B + Cin + Cout + H)
    x = torch.randn(B, Cin, H, W, generator=g).half().cuda()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).half().cuda()
    b = (torch.randn(Cout, generator=g) * 0.2).half().cuda()
    ref = F.conv2d(x.float(), w.float(), b.float(), padding=1)
    out = ops.conv3x3_fewcin(x, w.reshape(Cout, -1).t().contiguous(), b, Cout)
    assert out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last)
    assert torch.all((out.float() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3), (out.float() - ref).abs().max().item()
    xi = torch.zeros(B, Cin, H, W).half()
    xi[B - 1, Cin - 1, H - 1, 0] = 1.0
    xi[0, 0, 0, W - 1] = -2.0
    oi = ops.conv3x3_fewcin(xi.cuda(), w.reshape(Cout, -1).t().contiguous(), None, Cout).float().cpu()
    ri = F.conv2d(xi.float(), w.float().cpu(), None, padding=1)
    assert torch.all((oi - ri).abs() <= 1e-3 * ri.abs() + 1e-6)


@pytest.mark.parametrize("B,C,Cout,H,W,splits", [(2, 320, 320, 64, 64, 0), (2, 640, 640, 32, 32, 0), (2, 1280, 1280, 16, 16, 0),
                                                 (1, 64, 64, 8, 16, 1), (3, 128, 64, 16, 8, 2), (2, 1280, 1280, 12, 12, 0),
                                                 (1, 64, 64, 6, 10, 0)])
def test_conv3x3_stride2(ops, B, C, Cout, H, W, splits):
    """Downsample2D: the stride-2 / pad-1 convolution as the even pixels of the stride-1 taps"""
    g = torch.Generator().manual_seed(B + C + H + W)
    cl = torch.channels_last
    x = torch.randn(B, C, H, W, generator=g).half().cuda().contiguous(memory_format=cl)
    w = (torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(9 * C)).half().cuda().contiguous(memory_format=cl)
    b = (torch.randn(Cout, generator=g) * 0.2).half().cuda()
    ref = F.conv2d(x.float(), w.float(), b.float(), stride=2, padding=1)
    out = ops.conv3x3(x, w, b, stride2=True, splits=splits)
    assert out.shape == ref.shape and out.is_contiguous(memory_format=cl)
    assert torch.all((out.float() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3), (out.float() - ref).abs().max().item()
    assert torch.equal(out, ops.conv3x3(x, w, b, stride2=True, splits=splits))
    assert torch.equal(out, ops.conv3x3(x, w, b, splits=splits)[:, :, ::2, ::2])     # the same sums in the same order


def test_conv3x3_unsupported(ops):
    x = torch.randn(1, 4, 64, 64).half().cuda().contiguous(memory_format=torch.channels_last)
    w = torch.randn(320, 4, 3, 3).half().cuda().contiguous(memory_format=torch.channels_last)
    assert not ops.conv3x3_supported(x, w)                                # Cin must be a multiple of 64
    with pytest.raises(Exception):
        ops.conv3x3(x, w)
    x2 = torch.randn(1, 64, 12, 12).half().cuda().contiguous(memory_format=torch.channels_last)
    w2 = torch.randn(64, 64, 3, 3).half().cuda().contiguous(memory_format=torch.channels_last)
    assert ops.conv3x3_supported(x2, w2)                                  # image sides need not be multiples of the tile
    x3 = torch.randn(1, 64, 11, 12).half().cuda().contiguous(memory_format=torch.channels_last)
    with pytest.raises(Exception):
        ops.conv3x3(x3, w2, stride2=True)                                 # the stride-2 form needs even sides


@pytest.mark.parametrize("M,N,K", [(512, 1280, 1280), (512, 1280, 5120), (128, 1280, 1280), (8192, 320, 1280), (2048, 640, 2560),
                                   (77, 320, 768)])
def test_linear_library_bias_residual(ops, M, N, K):
    """dsc_linear_lt_f16: the hipBLASLt GEMM with bias epilogue + residual as beta*C, one launch; also under graph capture.
    The default build does not contain the library (DSC_WITH_HIPBLASLT=1 at build time compiles it in): there the entry point
    must DECLINE and ops.linear must still give the right numbers on the package's own GEMMs."""
    from diffusionspatialcontrol_amd import _lib
    if not _lib.load_library().dsc_has_library_gemm():
        g = torch.Generator().manual_seed(M + N + K + 1)
        x = torch.randn(M, K, generator=g).half().cuda()
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
        b = (torch.randn(N, generator=g) * 0.2).half().cuda()
        r = torch.randn(M, N, generator=g).half().cuda()
        out = torch.empty(M, N, dtype=torch.half, device="cuda")
        import ctypes
        vp = lambda t: ctypes.c_void_p(t.data_ptr())                                 # noqa: E731
        rc = _lib.load_library().dsc_linear_lt_f16(vp(x), vp(w), vp(b), vp(r), vp(out), M, N, K, K, N, N, 0,
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc != 0                                                               # declined, no launch
        ref = x.float() @ w.float().t() + b.float() + r.float()
        y = ops.linear(x, w, b, residual=r)
        assert torch.all((y.float() - ref).abs() <= 2e-3 * ref.abs() + 4e-3)
        return
    g = torch.Generator().manual_seed(M + N + K + 1)
    x = torch.randn(M, K, generator=g).half().cuda()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
    b = (torch.randn(N, generator=g) * 0.2).half().cuda()
    r = torch.randn(M, N, generator=g).half().cuda()
    ref = x.float() @ w.float().t() + b.float() + r.float()
    out = torch.empty(M, N, dtype=torch.half, device="cuda")
    import ctypes
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = _lib.load_library()
    rc = lib.dsc_linear_lt_f16(vp(x), vp(w), vp(b), vp(r), vp(out), M, N, K, K, N, N, 0,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert torch.all((out.float() - ref).abs() <= 2e-3 * ref.abs() + 4e-3), (out.float() - ref).abs().max().item()
    # the dispatch in ops.linear takes this path for shapes outside the hand-written kernel's range
    y = ops.linear(x, w, b, residual=r)
    assert torch.all((y.float() - ref).abs() <= 2e-3 * ref.abs() + 4e-3)
    # no bias / 3-D input with strided rows
    y2 = ops.linear(x, w, None, residual=r)
    assert torch.all((y2.float() - (ref - b.float())).abs() <= 2e-3 * ref.abs() + 4e-3)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            yg = ops.linear(x, w, b, residual=r)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y)


@pytest.mark.parametrize("M,N,K", [(512, 1280, 5120), (128, 1280, 5120), (128, 1280, 2560), (512, 1280, 1920), (300, 64, 1984),
                                   (2048, 640, 2560)])
def test_linear_splitk(ops, M, N, K):
    """dsc_linear_splitk_f16 (the few-row long-K projections that went to hipBLASLt until round 3): vs the fp32 product, every
    split count gives the un-split kernel's result up to the order of the fp32 partial sums, bit-reproducible, capturable, and
    ops.linear takes this route for M <= 512 / K >= 1920 with the library off"""
    g = torch.Generator().manual_seed(M + N + K + 3)
    x = torch.randn(M, K, generator=g).half().cuda()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
    b = (torch.randn(N, generator=g) * 0.2).half().cuda()
    r = torch.randn(M, N, generator=g).half().cuda()
    ref = x.float() @ w.float().t() + b.float() + r.float()
    one = ops.linear(x, w, b, residual=r, prefer_kernel=True) if M > 512 or K < 1920 else None
    for sp in (0, 1, 2, 3, 5, 8, 64):
        y = ops.linear_splitk(x, w, b, r, splits=sp)
        assert torch.all((y.float() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3), (sp, (y.float() - ref).abs().max().item())
        assert torch.equal(y, ops.linear_splitk(x, w, b, r, splits=sp))
        if sp == 1 and one is not None:
            assert torch.equal(y, one)                                       # one split IS dsc_linear_f16
    y0 = ops.linear_splitk(x, w, None, None)
    assert torch.all((y0.float() - (ref - b.float() - r.float())).abs() <= 1.5e-3 * ref.abs() + 2e-3)
    if M <= 512 and K >= 1920 and not ops.USE_LIBRARY_GEMM:
        assert torch.equal(ops.linear(x, w, b, residual=r), ops.linear_splitk(x, w, b, r))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for _ in range(2):
            ops.linear_splitk(x, w, b, r)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            yg = ops.linear_splitk(x, w, b, r)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, ops.linear_splitk(x, w, b, r))


@pytest.mark.parametrize("M,C,N,geglu", [(8192, 320, 960, False), (2048, 640, 640, False), (8192, 320, 2560, True),
                                          (1100, 64, 128, False), (2048, 640, 5120, True), (512, 1280, 3840, False)])
def test_linear_layernorm_folding(ops, M, C, N, geglu):
    """dsc_linear_ln_f16: producer GEMM emits row statistics, consumer GEMM applies the folded LayerNorm
    == add + LayerNorm + linear of the three-launch path"""
    g = torch.Generator().manual_seed(M + C + N)
    a = torch.randn(M, C, generator=g).half().cuda()
    wo = (torch.randn(C, C, generator=g) / math.sqrt(C)).half().cuda()
    bo = (torch.randn(C, generator=g) * 0.2).half().cuda()
    x = (torch.randn(M, C, generator=g) * 2 + 0.7).half().cuda()                  # residual stream with a non-zero mean
    gamma = (torch.randn(C, generator=g) * 0.3 + 1).half().cuda()
    beta = (torch.randn(C, generator=g) * 0.2).half().cuda()
    w = (torch.randn(N, C, generator=g) / math.sqrt(C)).half().cuda()
    b = (torch.randn(N, generator=g) * 0.2).half().cuda()
    assert ops.linear_kernel_covers(M, C, C, torch.float16) and ops.linear_kernel_covers(M, N, C, torch.float16, geglu)
    # producer: s = x + a @ wo.T + bo, with the statistics of the fp16 s rows
    s, st = ops.linear_ln(a, wo, bo, residual=x, ln_stats=True)
    assert torch.equal(s, ops.linear(a, wo, bo, residual=x)) and st.shape == (M, C // 64, 2)
    sf = s.float()
    assert torch.allclose(st[..., 0].sum(1), sf.sum(1), rtol=1e-5, atol=1e-3)
    assert torch.allclose(st[..., 1].sum(1), (sf * sf).sum(1), rtol=1e-5, atol=1e-2)
    # consumer: LayerNorm folded into the weights
    w2, b2, cvec = ops.fold_layernorm(w, b, gamma, beta)
    y = ops.linear_ln(s, w2, b2, geglu=geglu, ln=(st, cvec, 1e-5))
    h = F.layer_norm(sf, (C,), gamma.float(), beta.float(), 1e-5)
    ref = h @ w.float().t() + b.float()
    if geglu:
        hid, gate = ref.chunk(2, dim=-1)
        ref = hid * F.gelu(gate)
    err = (y.float() - ref).abs()
    assert err.max().item() < 2e-2 * max(1.0, ref.abs().max().item()) and err.mean().item() < 2e-3, (err.max().item(), err.mean().item())
    # and against the unfused product path (LayerNorm kernel -> linear): same function to fp16 rounding
    _, hk = ops.add_layernorm(s, None, gamma, beta)
    y0 = ops.linear(hk, w, b, geglu=geglu)
    assert (y.float() - y0.float()).abs().mean().item() < 2e-3
    assert torch.equal(y, ops.linear_ln(s, w2, b2, geglu=geglu, ln=(st, cvec, 1e-5)))
    # the 128-column tile: statistics per 64-column block and folded-LayerNorm epilogue give the same bytes
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    try:
        for knob in (100000, 200000):
            lib.dsc_debug_set_gemm_stages(knob)
            s_k, st_k = ops.linear_ln(a, wo, bo, residual=x, ln_stats=True)
            assert torch.equal(s_k, s) and torch.equal(st_k, st), knob
            assert torch.equal(ops.linear_ln(s, w2, b2, geglu=geglu, ln=(st, cvec, 1e-5)), y), knob
    finally:
        lib.dsc_debug_set_gemm_stages(0)


@pytest.mark.parametrize("offset,outlier", [(8.0, 1.0), (30.0, 1.0), (2.0, 60.0)])
def test_linear_layernorm_folding_with_large_means_and_outlier_channels(ops, offset, outlier):
    """The folded LayerNorm subtracts mu * (row sums of W') from an accumulator that holds the UN-normalised row: rows whose mean
    is many standard deviations (a DC offset of the residual stream) or that carry a few outlier channels (trained SD1.5 streams
    do; the random-init parity cases do not) must not cost more accuracy than the unfused LayerNorm -> linear path loses to the
    fp16 rounding of the normalised row.  Both against the fp32 function."""
    M, C, N = 2048, 640, 640
    g = torch.Generator().manual_seed(int(offset * 10 + outlier))
    a = torch.randn(M, C, generator=g).half().cuda()
    wo = (torch.randn(C, C, generator=g) / math.sqrt(C)).half().cuda()
    x = torch.randn(M, C, generator=g) + offset
    x[:, ::97] *= outlier                                                          # 7 channels, all rows
    x = x.half().cuda()
    gamma = (torch.randn(C, generator=g) * 0.3 + 1).half().cuda()
    beta = (torch.randn(C, generator=g) * 0.2).half().cuda()
    w = (torch.randn(N, C, generator=g) / math.sqrt(C)).half().cuda()
    b = (torch.randn(N, generator=g) * 0.2).half().cuda()
    s, st = ops.linear_ln(a, wo, None, residual=x, ln_stats=True)
    w2, b2, cvec = ops.fold_layernorm(w, b, gamma, beta)
    y = ops.linear_ln(s, w2, b2, ln=(st, cvec, 1e-5))
    ref = F.layer_norm(s.float(), (C,), gamma.float(), beta.float(), 1e-5) @ w.float().t() + b.float()
    _, hk = ops.add_layernorm(s, None, gamma, beta)
    y0 = ops.linear(hk, w, b)
    e_fold, e_plain = (y.float() - ref).abs(), (y0.float() - ref).abs()
    assert torch.isfinite(y).all()
    assert e_fold.mean().item() <= 2.0 * e_plain.mean().item() + 1e-3, (e_fold.mean().item(), e_plain.mean().item())
    assert e_fold.max().item() <= 2.0 * e_plain.max().item() + 2e-2, (e_fold.max().item(), e_plain.max().item())


@pytest.mark.parametrize("B,L,C,H,fold", [(2, 4096, 320, 8, True), (2, 1024, 640, 8, False), (3, 576, 320, 8, True), (16, 64, 320, 5, False),
                                         (1, 9216, 320, 8, False), (2, 1024, 640, 8, True), (2, 256, 1280, 8, True)])
def test_linear_qkv_head_major(ops, B, L, C, H, fold):
    """dsc_linear_qkv_f16: the fused q / k / v projection whose epilogue writes K and V head-major ([2, B, H, L, d]) equals
    the plain fused projection bit for bit (same GEMM, another store address), with and without a folded LayerNorm; token
    blocks that straddle two batch rows (L = 576, 64) included."""
    g = torch.Generator().manual_seed(B * L + C)
    x = (torch.randn(B, L, C, generator=g) * 1.3 + 0.2).half().cuda()
    w = (torch.randn(3 * C, C, generator=g) / C ** 0.5).half().cuda()
    assert ops.linear_qkv_covers(x, w, H)
    d = C // H
    if fold:
        gamma, beta = (torch.randn(C, generator=g) * 0.3 + 1).half().cuda(), (torch.randn(C, generator=g) * 0.2).half().cuda()
        w2, b2, cvec = ops.fold_layernorm(w, None, gamma, beta)
        # row partials as the producing GEMM's epilogue would leave them: per 64-column block (sum, sum of squares)
        xb = x.float().reshape(B * L, C // 64, 64)
        part = torch.stack([xb.sum(-1), (xb * xb).sum(-1)], dim=-1).contiguous()
        ln = (part, cvec, 1e-5)
        ref = ops.linear_ln(x, w2, b2, ln=ln)
        q4, k4, v4 = ops.linear_qkv(x, w2, b2, H, ln=ln)
    else:
        ref = ops.linear_ln(x, w, None)
        q4, k4, v4 = ops.linear_qkv(x, w, None, H)
    rq, rk, rv = (ref[..., i * C:(i + 1) * C].unflatten(-1, (H, d)) for i in range(3))
    assert q4.shape == k4.shape == v4.shape == (B, L, H, d)
    assert k4.stride() == (H * L * d, d, L * d, 1)                     # a head's keys are contiguous
    assert torch.equal(q4, rq) and torch.equal(k4, rk) and torch.equal(v4, rv)
    if (3 * C) % 128 == 0:                  # 128-column tiles: a tile may hold query AND key columns - the scatter is per chunk
        from diffusionspatialcontrol_amd import _lib
        lib = _lib.load_library()
        try:
            lib.dsc_debug_set_gemm_stages(200000)
            qw, kw_, vw = ops.linear_qkv(x, w2, b2, H, ln=ln) if fold else ops.linear_qkv(x, w, None, H)
        finally:
            lib.dsc_debug_set_gemm_stages(0)
        assert torch.equal(qw, rq) and torch.equal(kw_, rk) and torch.equal(vw, rv)
    # and the flash kernel on the head-major views equals the flash kernel on the token-major ones
    assert torch.equal(ops.self_attention(q4, k4, v4), ops.self_attention(rq, rk, rv))


@pytest.mark.parametrize("M,C", [(8192, 320), (2048, 640), (512, 1280), (300, 64)])
def test_linear_geglu_kernel(ops, M, C):
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g).half()
    w = (torch.randn(8 * C, C, generator=g) / math.sqrt(C)).half()
    b = (torch.randn(8 * C, generator=g) * 0.2).half()
    y = (x.float() @ w.float().t() + b.float()).half().float()            # the projection output is an fp16 tensor
    hid, gate = y.chunk(2, dim=-1)
    ref = hid * F.gelu(gate).half().float()
    out = ops.linear(x.cuda(), w.cuda(), b.cuda(), geglu=True)
    assert out.shape == (M, 4 * C)
    err = (out.float().cpu() - ref).abs()
    assert torch.all(err <= 4e-3 * ref.abs() + 4e-3), err.max().item()    # a flipped fp16 rounding of hid or gate moves the product by 1 ulp of each
    assert err.mean().item() < 3e-4


@pytest.mark.parametrize("rows,C", [(8192, 320), (2048, 640), (512, 1280), (77, 64), (5, 4096), (1000, 2560)])
def test_add_layernorm(ops, rows, C):
    g = torch.Generator().manual_seed(rows + C)
    x = (torch.randn(rows, C, generator=g) * 2 + 0.3).half()
    a = torch.randn(rows, C, generator=g).half()
    gamma, beta = (torch.randn(C, generator=g) * 0.3 + 1).half(), (torch.randn(C, generator=g) * 0.2).half()
    s_ref = (x.float() + a.float()).half()
    y_ref = F.layer_norm(s_ref.float(), (C,), gamma.float(), beta.float(), 1e-5)
    s, y = ops.add_layernorm(x.cuda(), a.cuda(), gamma.cuda(), beta.cuda())
    assert torch.equal(s.cpu(), s_ref)
    assert torch.all((y.float().cpu() - y_ref).abs() <= 1.5e-3 * y_ref.abs() + 2e-3)
    s0, y0 = ops.add_layernorm(x.cuda(), None, gamma.cuda(), beta.cuda())
    y0_ref = F.layer_norm(x.float(), (C,), gamma.float(), beta.float(), 1e-5)
    assert torch.all((y0.float().cpu() - y0_ref).abs() <= 1.5e-3 * y0_ref.abs() + 2e-3)


def test_geglu(ops):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(2, 100, 2 * 1280, generator=g) * 2).half()
    hid, gate = x.float().chunk(2, dim=-1)
    ref = hid * F.gelu(gate)
    y = ops.geglu(x.cuda()).float().cpu()
    # two fp16 roundings (gelu, product): relative 2^-10 each
    assert torch.all((y - ref).abs() <= 2.5e-3 * ref.abs() + 1e-3) and (y - ref).abs().mean().item() < 3e-4


def _sampler_launches_and_checks(ops, row_prepare=None, row_step=None):
    """dsc_prepare_unet_input, then dsc_cfg_dpmpp2m_step, on seeded latents (each with an optional row broadcast): everything
    each launch leaves in x_in / t_buf / sigma_buf, x and old against fp32 restatements; returns (x, eps, old, (a, b, c))"""
    g = torch.Generator().manual_seed(11)
    n, shp = 3, (3, 4, 16, 16)
    x = (torch.randn(shp, generator=g) * 10).half()
    eps = torch.randn((2 * n,) + shp[1:], generator=g).half()
    old = torch.randn(shp, generator=g).half()
    sigma, gs, a, b, c, cin, tn, sn = 3.17, 7.5, 0.8, 0.25, -0.05, 0.3, 412.5, 2.55
    xi, tb, sb = torch.zeros(2 * n, *shp[1:], dtype=torch.half).cuda(), torch.zeros(2 * n).cuda(), torch.zeros(1).cuda()
    ops.prepare_unet_input(x.cuda(), 0.123, 999.0, 14.6, xi, tb, sb, row=row_prepare)
    assert (xi.float().cpu() - torch.cat([x, x]).float() * 0.123).abs().max() < 2e-3
    assert tb.tolist() == [999.0] * (2 * n) and abs(sb.item() - 14.6) < 1e-6
    xd, od = x.cuda().clone(), old.cuda().clone()
    ops.cfg_dpmpp2m_step(xd, eps.cuda(), od, sigma, gs, a, b, c, cin, tn, sn, xi, tb, sb, row=row_step)
    eu, ec = eps.float().chunk(2)
    D = x.float() - sigma * (eu + gs * (ec - eu))
    xn = a * x.float() + b * D.half().float() + c * old.float()     # D is stored (and reused) as an fp16 tensor
    close = lambda got, ref: bool(torch.all((got.float().cpu() - ref).abs() <= 2e-3 * ref.abs() + 2e-3))  # noqa: E731
    assert close(od, D)                                         # one fp16 rounding: relative 2^-11
    assert close(xd, xn)
    assert close(xi, torch.cat([xn, xn]) * cin)
    assert tb.tolist() == [tn] * (2 * n) and abs(sb.item() - sn) < 1e-6
    return x, eps, old, (a, b, c)


def test_sampler_kernels(ops):
    x, eps, old, (a, b, c) = _sampler_launches_and_checks(ops)
    n = x.shape[0]
    out = ops.dpmpp2m_update(x.cuda(), eps[:n].cuda(), old.cuda(), a, b, c)
    assert (out.float().cpu() - (a * x.float() + b * eps[:n].float() + c * old.float())).abs().max() < 0.01
    out = ops.dpmpp2m_update(x.cuda(), eps[:n].cuda(), None, a, b, 0.0)
    assert (out.float().cpu() - (a * x.float() + b * eps[:n].float())).abs().max() < 0.01


@pytest.mark.parametrize("copies", [1, 2, 6])
@pytest.mark.parametrize("halfs", [8, 1280, 2560 + 8])
def test_sampler_kernels_row_broadcast(ops, copies, halfs):
    """row = (src, dst): the step's row of the per-schedule time-embedding table copied into every row of the static buffer
    the captured step reads, in the same launch as the sampler arithmetic (which must come out as without it)"""
    g = torch.Generator().manual_seed(copies * 10000 + halfs)
    table = (torch.randn(3, halfs, generator=g) * 4).half().cuda()           # rows of a table, as the pipeline hands them
    nan = torch.full((copies, halfs), float("nan"), dtype=torch.half, device="cuda")
    dst_prepare, dst_step = nan.clone(), nan.clone()
    _sampler_launches_and_checks(ops, row_prepare=(table[1], dst_prepare), row_step=(table[2], dst_step))
    assert torch.equal(dst_prepare, table[1].expand(copies, halfs))
    assert torch.equal(dst_step, table[2].expand(copies, halfs))


def test_sampler_row_broadcast_refuses_ragged_rows(ops):
    """a row of halfs % 8 != 0 is refused before the launch: neither the row nor the sampler buffers are written"""
    x = torch.randn(1, 4, 8, 8).half().cuda()
    x_in, tb, sb = torch.zeros(2, 4, 8, 8, dtype=torch.half, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda")
    src, dst = torch.ones(12, dtype=torch.half, device="cuda"), torch.zeros(2, 12, dtype=torch.half, device="cuda")
    from diffusionspatialcontrol_amd import _lib
    with pytest.raises(_lib.DscLibraryError):
        ops.prepare_unet_input(x, 0.5, 10.0, 1.0, x_in, tb, sb, row=(src, dst))
    with pytest.raises(_lib.DscLibraryError):
        ops.cfg_dpmpp2m_step(x, x_in, x.clone(), 1.0, 7.5, 0.5, 0.5, 0.0, 1.0, 10.0, 1.0, x_in, tb, sb, row=(src, dst))
    torch.cuda.synchronize()
    assert not dst.any() and not x_in.any() and not tb.any() and not sb.any()


def _tiny_setup(n_img=1, seed=0):
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(seed)
    cfg = UNetConfig.tiny()
    unet = UNet2DConditionModel(cfg).half()
    sd = {k: v.clone() for k, v in unet.state_dict().items()}      # fp16-representable weights shared with the oracle
    g = torch.Generator().manual_seed(7)
    text = torch.randn(2 * n_img, 77, cfg.cross_attention_dim, generator=g).half()
    return cfg, unet.cuda(), sd, text


def _region_state(W=128, H=128, n_img=1):
    from diffusionspatialcontrol_amd.modules.encode_region_map_function import encode_region_map
    import types
    P = "a photo of a red apple on a wooden table near a blue vase"
    ids = [prompt_ids("blurry"), prompt_ids(P)]
    state = {"red apple": {"map": rect_map(H, W, 0, 0, 1, 2), "weight": 0.5, "mask_outsides": 0.0},
             "blue vase": {"map": rect_map(H, W, 1, 0, 2, 1), "weight": 0.8, "mask_outsides": 0.2}}
    pipe = types.SimpleNamespace(tokenizer=FakeTokenizer(), unet=types.SimpleNamespace(down_blocks=[0] * 4),
                                 vae_scale_factor=8, do_classifier_free_guidance=True)
    return state, ids, encode_region_map(pipe, state, W, H, n_img, text_ids=ids)


def test_unet_forward_matches_oracle(ops):
    cfg, unet, sd, text = _tiny_setup()
    _, _, rs = _region_state()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 16, 16, generator=g).half()
    t = torch.tensor([731.25, 731.25])
    sigma = torch.tensor([4.0], device="cuda")
    rp = {"region_state": rs, "sigma": sigma, "weight_func": lambda w, s, qk: w * s * qk.std()}
    out = unet(x.cuda(), t.cuda(), text.cuda(), cross_attention_kwargs={"region_prompt": rp}).sample.float().cpu()
    rp_o = {"region_state": rs, "sigma": 4.0, "weight_func": None}
    ref = unet_ref.unet_forward(sd, cfg, x.float(), t, text.float(), region_prompt=rp_o)
    scale = ref.abs().max().item()
    err = (out - ref).abs()
    # 60+ fp16 layers deep: relative 1e-2 of the output range, mean 2e-3
    assert err.max().item() < 1e-2 * scale + 1e-3, (err.max().item(), scale)
    assert err.mean().item() < 2e-3 * scale
    # the region bias is live: without it the output differs
    out0 = unet(x.cuda(), t.cuda(), text.cuda()).sample.float().cpu()
    assert (out0 - out).abs().max().item() > 10 * err.max().item() or (out0 - out).abs().max().item() > 1e-2 * scale


@pytest.mark.parametrize("n_img", [1, 2])
def test_denoise_loop_fused_protocol_oracle(ops, n_img):
    """6-step DPM++ 2M Karras loop on the tiny UNet: fused (graph) == protocol (closure) ~= CPU oracle."""
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    cfg, unet, sd, text = _tiny_setup(n_img)
    state, ids, rs = _region_state(n_img=1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    g = torch.Generator().manual_seed(1000)
    lat = torch.randn(n_img, 4, 16, 16, generator=g).half()
    pe, ne = text[n_img:n_img + 1], text[:1]
    kw = dict(height=128, width=128, num_inference_steps=6, guidance_scale=7.5, latents=lat.clone(), output_type="latent",
              region_map_state=state, sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"},
              prompt_embeds=pe.repeat(1, 1, 1), negative_prompt_embeds=ne, text_input_ids=ids,
              num_images_per_prompt=n_img)
    if n_img > 1:
        kw["latents"] = lat.clone()
    fused = pipe.txt2img(None, fused=True, **kw)[0].float().cpu()
    proto = pipe.txt2img(None, fused=False, **kw)[0].float().cpu()
    sig = pipe.get_sigmas(6, {"scheduler": "karras"}).half().float().tolist()
    text_rows = torch.cat([ne.repeat(n_img, 1, 1), pe.repeat(n_img, 1, 1)]).float()
    rs_rows = {L: t for L, t in rs.items()}
    ref = unet_ref.denoise_loop(sd, cfg, lat.float() * math.sqrt(sig[0] ** 2 + 1), sig, text_rows, rs_rows, 7.5)
    scale = ref.abs().max().item()
    assert torch.isfinite(fused).all()
    assert (fused - proto).abs().max().item() < 2e-2 * scale      # same kernels, different rounding points
    assert (fused - ref).abs().max().item() < 4e-2 * scale, ((fused - ref).abs().max().item(), scale)
    assert (fused - ref).abs().mean().item() < 6e-3 * scale
    # a second generation re-captures the graph and lands within rounding noise of the first (bitwise equality is
    # checked at the real SD1.5 shapes below: MIOpen's convolutions at this toy 2x2 / 4x4 resolution use atomics)
    again = pipe.txt2img(None, fused=True, **kw)[0].float().cpu()
    assert (fused - again).abs().max().item() < 2e-2 * scale
    if n_img == 2:      # images are independent: image 0 of the pair equals the single-image run (per-image std groups)
        kw1 = dict(kw, latents=lat[:1].clone(), num_images_per_prompt=1)
        single = pipe.txt2img(None, fused=True, **kw1)[0].float().cpu()
        assert (single[0] - fused[0]).abs().max().item() < 2e-2 * scale


@pytest.mark.parametrize("name,opt", [("sample_euler", {"scheduler": "karras"}), ("sample_heun", {"scheduler": "exponential"}),
                                      ("sample_dpm_2", {"scheduler": "karras", "discard_next_to_last_sigma": True}),
                                      ("sample_lms", {}), ("sample_dpmpp_2s_ancestral", {"scheduler": "polyexponential"}),
                                      ("sample_dpmpp_2m_sde", {"scheduler": "karras", "brownian_noise": True, "solver_type": "heun"}),
                                      ("heunpp2", {"scheduler": "karras"}), ("restart", {"scheduler": "karras"})])
def test_other_samplers_protocol_vs_oracle(ops, name, opt):
    """The other samplers app.py offers (k-diffusion names resolved by get_scheduler, the reference's extra samplers passed
    as callables) drive the same model_fn: product protocol loop on the GPU against the SAME sampler driving the fp32 CPU
    oracle model.  eta = 0 (the pipeline default) makes the ancestral / SDE ones deterministic."""
    from diffusionspatialcontrol_amd.modules import sampling, samplers_extra_k_diffusion as sx
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    cfg, unet, sd, text = _tiny_setup(1)
    state, ids, rs = _region_state(n_img=1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(77)).half()
    fn = {"heunpp2": sx.sample_heunpp2, "restart": sx.restart_sampler}.get(name) or getattr(sampling, name)
    steps = 5
    kw = dict(height=128, width=128, num_inference_steps=steps, guidance_scale=7.5, latents=lat.clone(), output_type="latent",
              region_map_state=state, sampler_name=name if hasattr(sampling, name) else fn, sampler_opt=opt,
              prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], text_input_ids=ids, eta=0.0, seed=3)
    out = pipe.txt2img(None, **kw)[0].float().cpu()
    assert torch.isfinite(out).all()
    # repeatable to rounding (the toy channel counts fall back to MIOpen's atomic kernels; bitwise equality is asserted at
    # the real SD1.5 shapes in test_sd15_unet_step_full_size)
    assert (out - pipe.txt2img(None, **kw)[0].float().cpu()).abs().max().item() < 5e-2 * out.abs().max().item()
    sig = pipe.get_sigmas(steps, opt).half().float()
    extra = {k: v for k, v in pipe.get_sampler_extra_args_t2i(sig, 0.0, steps, opt, lat, 3, fn).items() if k != "sigmas"}
    if name == "restart":
        return                                                                # stochastic by construction: finiteness only
    ref = unet_ref.denoise_loop(sd, cfg, lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), text.float(), rs, 7.5,
                                sampler=fn, sampler_kwargs=extra)
    scale = ref.abs().max().item()
    assert (out - ref).abs().max().item() < 4e-2 * scale, ((out - ref).abs().max().item(), scale)
    assert (out - ref).abs().mean().item() < 6e-3 * scale


def test_v_prediction_pipeline_vs_oracle(ops):
    """prediction_type == "v_prediction": CompVisVDenoiser in protocol mode against the oracle's v-denoiser loop (the
    reference drops the region prompt on this branch - reproduced; `pass_kwargs` restores it)"""
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    cfg, unet, sd, text = _tiny_setup(1)
    state, ids, rs = _region_state(n_img=1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler(prediction_type="v_prediction"))
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(5)).half()
    kw = dict(height=128, width=128, num_inference_steps=5, guidance_scale=7.5, latents=lat.clone(), output_type="latent",
              region_map_state=state, sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"},
              prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], text_input_ids=ids)
    out = pipe.txt2img(None, **kw)[0].float().cpu()
    sig = pipe.get_sigmas(5, {"scheduler": "karras"}).half().float().cpu()
    ref = unet_ref.denoise_loop(sd, cfg, lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), text.float(), rs, 7.5,
                                v_prediction=True)
    scale = ref.abs().max().item()
    assert torch.isfinite(out).all() and (out - ref).abs().max().item() < 4e-2 * scale
    pipe.k_diffusion_model.pass_kwargs = True
    ctl = pipe.txt2img(None, **kw)[0].float().cpu()
    assert (ctl - out).abs().max().item() > 1e-3 * scale               # with the kwargs forwarded the region bias is live


def test_sd15_unet_step_full_size(ops):
    """Full-size SD1.5 UNet (random weights, seed 0), one CFG step with the region bias at all 16 cross-attention
    layers: finite output, the bias is live, and a repeat is BIT-IDENTICAL - every convolution of the step now runs on
    the hand-written kernels (fixed summation orders, ordered split-K), the library GEMMs are hipBLASLt's plain kernels;
    MIOpen's atomic split-K solvers (`*_GKGS`), which made the step reproducible only to rounding, are gone from it."""
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    with torch.device("cuda"):
        unet = UNet2DConditionModel(UNetConfig.sd15())
    unet = unet.half().eval()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 64, 64, generator=g).half().cuda()
    enc = torch.randn(2, 77, 768, generator=g).half().cuda()
    t = torch.tensor([500.5, 500.5], device="cuda")
    rs = {}
    for L in (4096, 1024, 256, 64):
        w = torch.zeros(2, L, 77)
        w[:, : L // 3, 2:4] = 0.5
        w[:, L // 2:, 4:6] = 0.5
        rs[L] = w
    rp = {"region_state": rs, "sigma": torch.tensor([3.0], device="cuda"), "weight_func": lambda w, s, qk: w * s * qk.std()}
    with torch.no_grad():
        outs = [unet(x, t, enc, cross_attention_kwargs={"region_prompt": rp}).sample.clone() for _ in range(2)]
        plain = unet(x, t, enc).sample
    assert torch.isfinite(outs[0]).all()
    scale = outs[0].float().abs().max().item()
    assert torch.equal(outs[0], outs[1])
    assert (plain.float() - outs[0].float()).abs().max().item() > 1e-3 * scale   # the region bias is live
    # LayerNorm folding (dsc_linear_ln_f16) on vs off: the same function up to fp16 rounding of one intermediate
    ops.USE_LN_FOLD = False
    try:
        with torch.no_grad():
            unfolded = unet(x, t, enc, cross_attention_kwargs={"region_prompt": rp}).sample
    finally:
        ops.USE_LN_FOLD = True
    assert (unfolded.float() - outs[0].float()).abs().max().item() < 1e-2 * scale


@pytest.mark.parametrize("C,heads,hw", [(320, 8, 64), (640, 8, 32)])
def test_transformer_block_layernorm_folding(ops, C, heads, hw):
    """Transformer2DModel with the three LayerNorms of its block folded into the neighbouring GEMMs against the unfolded
    launch sequence and against the fp32 torch restatement of the block on the same weights."""
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import Transformer2DModel
    torch.manual_seed(C)
    with torch.device("cuda"):
        tr = Transformer2DModel(C, heads, 1, 768, 32, False)
    for n_ in (tr.transformer_blocks[0].norm1, tr.transformer_blocks[0].norm2, tr.transformer_blocks[0].norm3):
        torch.nn.init.normal_(n_.weight, 1.0, 0.3)
        torch.nn.init.normal_(n_.bias, 0.0, 0.2)
    tr = tr.half().eval()
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(2, C, hw, hw, generator=g) * 1.5 + 0.3).half().cuda().contiguous(memory_format=torch.channels_last)
    enc = torch.randn(2, 77, 768, generator=g).half().cuda()
    with torch.no_grad():
        assert ops.USE_LN_FOLD and tr.transformer_blocks[0]._can_fold(torch.empty(2, hw * hw, C, device="cuda", dtype=torch.float16), True)
        y1 = tr(x, enc, None)
        ops.USE_LN_FOLD = False
        try:
            y0 = tr(x, enc, None)
        finally:
            ops.USE_LN_FOLD = True
        assert torch.equal(y1, tr(x, enc, None))
        # fp32 restatement (diffusers BasicTransformerBlock order of operations)
        blk = tr.transformer_blocks[0]
        f = lambda m: m.float()
        xf = x.float()
        h = F.group_norm(xf, 32, f(tr.norm.weight), f(tr.norm.bias), 1e-6)
        tks = h.permute(0, 2, 3, 1).reshape(2, hw * hw, C) @ f(tr.proj_in.weight).flatten(1).t() + f(tr.proj_in.bias)

        def attn(a, hn, ctx):
            q, k, v = hn @ f(a.to_q.weight).t(), ctx @ f(a.to_k.weight).t(), ctx @ f(a.to_v.weight).t()
            sp = lambda z: z.unflatten(-1, (heads, C // heads)).transpose(1, 2)
            o = F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).flatten(2)
            return o @ f(a.to_out[0].weight).t() + f(a.to_out[0].bias)
        ln = lambda n_, z: F.layer_norm(z, (C,), f(n_.weight), f(n_.bias), n_.eps)
        hn = ln(blk.norm1, tks)
        tks = tks + attn(blk.attn1, hn, hn)
        tks = tks + attn(blk.attn2, ln(blk.norm2, tks), enc.float())
        pr = ln(blk.norm3, tks) @ f(blk.ff.net[0].proj.weight).t() + f(blk.ff.net[0].proj.bias)
        hid, gate = pr.chunk(2, dim=-1)
        tks = tks + (hid * F.gelu(gate)) @ f(blk.ff.net[2].weight).t() + f(blk.ff.net[2].bias)
        ref = (tks @ f(tr.proj_out.weight).flatten(1).t() + f(tr.proj_out.bias)).reshape(2, hw, hw, C).permute(0, 3, 1, 2) + xf
    scale = ref.abs().max().item()
    e1, e0 = (y1.float() - ref).abs().max().item(), (y0.float() - ref).abs().max().item()
    assert e1 < 1e-2 * scale and e0 < 1e-2 * scale, (e1, e0, scale)
    assert e1 < 2.0 * e0 + 1e-3 * scale, (e1, e0)             # folding is not less accurate than the unfolded sequence


def _region_tables(levels, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    rs = {}
    for L in levels:
        w = torch.zeros(2, L, S)
        m1 = torch.rand(L, generator=g) < 0.3
        m2 = torch.rand(L, generator=g) < 0.3
        w[:, m1, 2:4] = 0.5
        w[:, m2, 4:6] += 0.5
        rs[L] = w
    return rs


def test_config4_sd15_768_step(ops):
    """BASELINE configs[3] shape: SD1.5 at 768x768 (L = 9216 / 2304 / 576 / 144), 2 region masks, one CFG step.
    Region cross-attention at every level is checked against the oracle on the actual q/k/v of that layer (captured
    with a recording processor), the whole step for finiteness."""
    from diffusionspatialcontrol_amd.modules.attention_modify import AttnProcessor2_0
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    from oracle import region_attention as ra
    torch.manual_seed(0)
    with torch.device("cuda"):
        unet = UNet2DConditionModel(UNetConfig.sd15())
    unet = unet.half().eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 4, 96, 96, generator=g).half().cuda()
    enc = torch.randn(2, 77, 768, generator=g).half().cuda()
    t = torch.tensor([700.25, 700.25], device="cuda")
    rs = _region_tables((9216, 2304, 576, 144), 77)
    rp = {"region_state": rs, "sigma": torch.tensor([5.0], device="cuda"), "weight_func": lambda w, s, qk: w * s * qk.std()}
    seen = {}

    class Recorder(AttnProcessor2_0):
        # region_prompt must be a NAMED parameter: Attention.forward drops kwargs the processor does not declare
        def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, region_prompt=None):
            out = super().__call__(attn, hidden_states, encoder_hidden_states=encoder_hidden_states,
                                   region_prompt=region_prompt)
            L = hidden_states.shape[1]
            if encoder_hidden_states is not None and L not in seen:
                q = attn.to_q(hidden_states)
                k, v = attn.to_k(encoder_hidden_states), attn.to_v(encoder_hidden_states)
                B, _, C = q.shape
                H = attn.heads
                seen[L] = (q.view(B, L, H, C // H), k.view(B, 77, H, C // H), v.view(B, 77, H, C // H),
                           attn.to_out[0], out)
            return out

    unet.set_attn_processor(Recorder())
    with torch.no_grad():
        y = unet(x, t, enc, cross_attention_kwargs={"region_prompt": rp}).sample
    assert y.shape == (2, 4, 96, 96) and torch.isfinite(y).all()
    assert sorted(seen) == [144, 576, 2304, 9216]
    for L, (q, k, v, to_out, got) in seen.items():
        qc, kc, vc = (z.float().cpu().transpose(1, 2) for z in (q, k, v))
        exp = ra.region_attention(qc, kc, vc, rs[L], 5.0)                          # [B, H, L, d] fp32
        exp = exp.transpose(1, 2).reshape(2, L, -1)
        exp = torch.nn.functional.linear(exp, to_out.weight.float().cpu(), to_out.bias.float().cpu())
        err = (got.float().cpu() - exp).abs()
        assert err.max().item() < 8e-3 * max(1.0, exp.abs().max().item()), (L, err.max().item())


def test_config5_sdxl_shape_step(ops):
    """BASELINE configs[4] shape: SDXL-base UNet geometry (3 levels, transformer depth 0/2/10, 5/10/20 heads of dim
    64, context dim 2048) at a 1024x1024 latent, region tables at L = 4096 and 1024.  The reference has no SDXL
    pipeline; this extrapolates the same processor contract.  One CFG step: finite, bias live."""
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    cfg = UNetConfig.sdxl_base()
    with torch.device("cuda"):
        unet = UNet2DConditionModel(cfg).half().eval()
    assert len(unet.attn_processors) == 140
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 4, 128, 128, generator=g).half().cuda()
    enc = torch.randn(2, 77, 2048, generator=g).half().cuda()
    t = torch.tensor([400.0, 400.0], device="cuda")
    rs = _region_tables((16384, 4096, 1024), 77, seed=2)
    rp = {"region_state": rs, "sigma": torch.tensor([4.0], device="cuda"), "weight_func": lambda w, s, qk: w * s * qk.std()}
    with torch.no_grad():
        y = unet(x, t, enc, cross_attention_kwargs={"region_prompt": rp}).sample
        y0 = unet(x, t, enc).sample
    assert y.shape == (2, 4, 128, 128) and torch.isfinite(y).all()
    assert (y.float() - y0.float()).abs().max().item() > 1e-3


def test_vae_decoder_matches_oracle(ops):
    """VAE decode on a toy-width decoder: product (fp16, channels-last, HIP GroupNorm) vs the fp32
    oracle restatement on shared weights; and `decode_latents` end to end through the pipeline."""
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKLDecoder, VaeConfig
    from oracle import vae_ref
    torch.manual_seed(1)
    cfg = VaeConfig.tiny()
    vae = AutoencoderKLDecoder(cfg).half()
    sd = {k: v.clone() for k, v in vae.state_dict().items()}
    vae = vae.cuda()
    g = torch.Generator().manual_seed(2)
    z = (torch.randn(2, 4, 16, 16, generator=g) * 0.9).half()
    with torch.no_grad():
        ref = vae_ref.vae_decode(sd, z.float(), groups=cfg.norm_num_groups)
        out = vae.decode(z.cuda()).sample.float().cpu()
    assert out.shape == (2, 3, 128, 128)
    scale = ref.abs().max().item()
    assert (out - ref).abs().max().item() < 1.5e-2 * scale and (out - ref).abs().mean().item() < 2e-3 * scale
    unet = UNet2DConditionModel(UNetConfig.tiny()).half().cuda()
    pipe = StableDiffusionPipeline(vae, None, None, unet, SD15Scheduler())
    img = pipe.decode_latents(z.cuda() * cfg.scaling_factor)
    with torch.no_grad():
        ref_img = vae_ref.decode_latents(sd, z.float() * cfg.scaling_factor, cfg.scaling_factor, cfg.norm_num_groups)
    assert img.shape == (2, 128, 128, 3) and img.min() >= 0.0 and img.max() <= 1.0
    assert np.abs(img - ref_img).max() < 2e-2


def test_vae_decoder_full_size(ops):
    """SD1.x decoder geometry at a 64x64 latent -> 512x512 RGB: finite, right shape (random weights)."""
    from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKLDecoder
    torch.manual_seed(0)
    with torch.device("cuda"):
        vae = AutoencoderKLDecoder().half().eval()
    z = torch.randn(1, 4, 64, 64, device="cuda").half()
    with torch.no_grad():
        y = vae.decode(z).sample
    assert y.shape == (1, 3, 512, 512) and torch.isfinite(y).all()


@pytest.mark.parametrize("full", [False, True])
def test_vae_encoder_matches_oracle(ops, full):
    """VAE encode (img2img / inpainting front end): product (few-channel conv_in kernel, stride-2 convolutions as the odd
    pixels of the stride-1 taps, HIP GroupNorm) vs the fp32 oracle restatement on shared weights - toy width (library
    convolutions) and the SD1.x geometry (hand-written kernels) at 256x256."""
    from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKL, VaeConfig
    from oracle import vae_ref
    torch.manual_seed(3)
    cfg = VaeConfig() if full else VaeConfig.tiny()
    vae = AutoencoderKL(cfg).half()
    sd = {k: v.clone() for k, v in vae.state_dict().items()}
    vae = vae.cuda().eval()
    g = torch.Generator().manual_seed(4)
    hw = 256 if full else 64
    x = (torch.rand(2, 3, hw, hw, generator=g) * 2 - 1).half()
    with torch.no_grad():
        ref = vae_ref.vae_encode_moments(sd, x.float(), groups=cfg.norm_num_groups)
        dist = vae.encode(x.cuda()).latent_dist
    out = dist.parameters.float().cpu()
    assert out.shape == (2, 8, hw // 8, hw // 8)
    scale = ref.abs().max().item()
    assert (out - ref).abs().max().item() < 2e-2 * scale and (out - ref).abs().mean().item() < 3e-3 * scale, \
        ((out - ref).abs().max().item(), scale)
    gen = torch.Generator().manual_seed(9)
    smp = dist.sample(gen).float().cpu()
    noise = torch.randn(2, 4, hw // 8, hw // 8, generator=torch.Generator().manual_seed(9), dtype=torch.float16).float()
    assert (smp - vae_ref.gaussian_sample(out, noise)).abs().max().item() < 2e-3 * max(1.0, smp.abs().max().item())
    assert torch.equal(dist.mode(), dist.mean)


def test_conv3x3_stride2_pad_bottom_right(ops):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 128, 32, 48, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(192, 128, 3, 3, generator=g) / 34).half().cuda().contiguous(memory_format=torch.channels_last)
    b = torch.randn(192, generator=g).half().cuda()
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), b.float(), stride=2)
    for splits in (0, 2):
        y = ops.conv3x3(x, w, b, stride2_pad_br=True, splits=splits)
        assert y.shape == ref.shape
        assert (y.float() - ref).abs().max().item() < 2e-2 * ref.abs().max().item()


def test_img2img_and_inpainting_pipeline(ops):
    """img2img (reference :543-846) and the 4-channel inpainting branch (:1365-1760) on the tiny UNet + tiny VAE: fused ==
    protocol ~= the fp32 CPU oracle loop started from the same noised latents; the inpainting hook keeps the known region."""
    from diffusionspatialcontrol_amd.modules import sampling
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKL, VaeConfig
    cfg, unet, sd, text = _tiny_setup(1)
    state, ids, rs = _region_state(n_img=1)
    torch.manual_seed(12)
    vae = AutoencoderKL(VaeConfig.tiny()).half().cuda().eval()
    pipe = StableDiffusionPipeline(vae, None, FakeTokenizer(), unet, SD15Scheduler())
    steps, strength = 8, 0.6
    lat0 = (torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(21)) * 0.8).half()
    common = dict(num_inference_steps=steps, guidance_scale=7.5, output_type="latent", region_map_state=state,
                  sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"}, prompt_embeds=text[1:2],
                  negative_prompt_embeds=text[:1], text_input_ids=ids, width=128, height=128)
    outs = {}
    for fused in (True, False):
        gen = torch.Generator().manual_seed(33)
        outs[fused] = pipe.img2img(None, latents=lat0.clone(), strength=strength, generator=gen, fused=fused, **common)[0].float().cpu()
    sig = pipe.get_sigmas(steps, {"scheduler": "karras"}).half().float().cpu()
    t_start = steps - min(int(steps * strength), steps)
    sched = sig[t_start:]
    assert len(sched) == int(steps * strength) + 1
    noise = torch.randn(lat0.shape, generator=torch.Generator().manual_seed(33), dtype=torch.float16)
    start = (lat0 + noise * (sched[0].half() ** 2 + 1) ** 0.5).float()                 # the reference's start (:647)
    ref = unet_ref.denoise_loop(sd, cfg, start, sched.tolist(), text.float(), rs, 7.5)
    scale = ref.abs().max().item()
    assert (outs[True] - outs[False]).abs().max().item() < 2e-2 * scale
    assert (outs[True] - ref).abs().max().item() < 4e-2 * scale and (outs[True] - ref).abs().mean().item() < 6e-3 * scale
    # from pixels: the VAE encoder path runs and strength = 1 keeps the whole schedule
    img = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(2)) * 2 - 1
    px = pipe.img2img(None, image=img, strength=1.0, generator=torch.Generator().manual_seed(1), **common)[0]
    assert px.shape == (1, 4, 16, 16) and torch.isfinite(px).all()
    # inpainting: left half known, right half repainted; Euler sampler so that the oracle can run the same sampler
    mask = torch.zeros(1, 1, 128, 128)
    mask[..., 64:] = 1.0
    common.pop("sampler_name")
    gen = torch.Generator().manual_seed(44)
    inp = pipe.inpaiting(None, image=lat0.clone(), mask_image=mask, strength=1.0, generator=gen,
                         sampler_name="sample_euler", **common)[0].float().cpu()
    n = torch.randn(lat0.shape, generator=torch.Generator().manual_seed(44), dtype=torch.float16).float()
    m16 = F.interpolate(mask, size=(16, 16))
    img_lat = lat0.float()

    def hook(x, sigma, k):
        if k == 0:
            return x
        s = float(sigma[0])
        known = img_lat + s * n if s > 0 else img_lat
        return (1 - m16) * known + m16 * x
    ref_i = unet_ref.denoise_loop(sd, cfg, n * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), text.float(), rs, 7.5,
                                  sampler=sampling.sample_euler, input_hook=hook)
    sc = ref_i.abs().max().item()
    assert (inp - ref_i).abs().max().item() < 4e-2 * sc, ((inp - ref_i).abs().max().item(), sc)
    with pytest.raises(NotImplementedError):
        pipe.inpaiting(None, image=lat0, mask_image=mask, padding_mask_crop=8, **common)
    # latent previews (reference :1083-1084, :1169-1170, :1229-1230): the start + one estimate per model call, nothing else
    common["sampler_name"] = "sample_heun"
    prev = pipe.txt2img(None, latents=lat0.clone(), latent_processing=1, **common)
    assert len(prev) == 1 + (2 * steps - 1) and all(p_.shape == (1, 4, 16, 16) for p_ in prev)       # Heun: 2 calls per step but the last
    # hires pass (reference :1176-1228): txt2img, latents x1.5 by bicubic interpolation, img2img at strength 0.5
    common["sampler_name"] = "sample_dpmpp_2m"
    hi = pipe.txt2img(None, latents=lat0.clone(), upscale=True, upscale_x=1.5, upscale_denoising_strength=0.5,
                      generator=torch.Generator().manual_seed(3), **common)[0]
    assert hi.shape == (1, 4, 24, 24) and torch.isfinite(hi).all()


def _controlnet(cfg, seed=5):
    """a ControlNet with its zero-initialised convolutions re-drawn (otherwise every residual is zero)"""
    from diffusionspatialcontrol_amd.modules.controlnet import ControlNetModel
    torch.manual_seed(seed)
    cn = ControlNetModel(cfg)
    for conv in list(cn.controlnet_down_blocks) + [cn.controlnet_mid_block, cn.controlnet_cond_embedding.conv_out]:
        torch.nn.init.normal_(conv.weight, 0.0, 0.15)
        torch.nn.init.normal_(conv.bias, 0.0, 0.05)
    cn = cn.half()
    return cn, {k: v.clone() for k, v in cn.state_dict().items()}


@pytest.mark.parametrize("full", [False, True])
def test_controlnet_forward_matches_oracle(ops, full):
    """ControlNetModel (the UNet's encoder half + conditioning embedding + 1x1 output convolutions) against the fp32 oracle on
    shared weights: toy width, and the SD1.5 geometry at a 32x32 latent."""
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNetConfig
    cfg = UNetConfig.sd15() if full else UNetConfig.tiny()
    cn, sd = _controlnet(cfg)
    cn = cn.cuda().eval()
    g = torch.Generator().manual_seed(8)
    hw = 32 if full else 16
    x = torch.randn(2, 4, hw, hw, generator=g).half()
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half()
    cond = torch.rand(2, 3, hw * 8, hw * 8, generator=g).half()
    t = torch.tensor([321.5, 321.5])
    with torch.no_grad():
        down, mid = cn(x.cuda(), t.cuda(), enc.cuda(), cond.cuda(), conditioning_scale=0.7, return_dict=False)
        rdown, rmid = unet_ref.controlnet_forward(sd, cfg, x.float(), t, enc.float(), cond.float(), 0.7)
    assert len(down) == 12
    for a, b in zip(down + [mid], rdown + [rmid]):
        sc = max(b.abs().max().item(), 1e-3)
        assert a.shape == b.shape and (a.float().cpu() - b).abs().max().item() < 2e-2 * sc, (a.shape, sc)
    with torch.no_grad():      # guess mode: residual k scaled by logspace(-1, 0, 13)[k]
        d2, m2 = cn(x.cuda(), t.cuda(), enc.cuda(), cond.cuda(), conditioning_scale=1.0, guess_mode=True, return_dict=False)
        rd2, rm2 = unet_ref.controlnet_forward(sd, cfg, x.float(), t, enc.float(), cond.float(), 1.0, guess_mode=True)
    for a, b in zip(d2 + [m2], rd2 + [rm2]):
        assert (a.float().cpu() - b).abs().max().item() < 2e-2 * max(b.abs().max().item(), 1e-3)


def test_controlnet_pipeline_vs_oracle(ops):
    """txt2img with a ControlNet (reference model_k_diffusion.py:1118-1152): every model call evaluates the ControlNet on the
    duplicated latent / sqrt(sigma^2 + 1) and hands its residuals to the UNet; guidance window [0, 0.6] switches it off for the
    last steps.  Product (protocol mode) against the oracle loop with the oracle ControlNet."""
    from diffusionspatialcontrol_amd.modules import sampling
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    cfg, unet, sd, text = _tiny_setup(1)
    state, ids, rs = _region_state(n_img=1)
    cn, cn_sd = _controlnet(cfg)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    pipe.setup_controlnet(cn.cuda().eval())
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(6)).half()
    ctrl = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(7))
    steps = 5
    kw = dict(height=128, width=128, num_inference_steps=steps, guidance_scale=7.5, latents=lat.clone(), output_type="latent",
              region_map_state=state, sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"},
              prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], text_input_ids=ids)
    out = pipe.txt2img(None, control_img=ctrl, controlnet_conditioning_scale=0.9, control_guidance_start=0.0,
                       control_guidance_end=0.6, **kw)[0].float().cpu()
    sig = pipe.get_sigmas(steps, {"scheduler": "karras"}).half().float().cpu()
    keep = [1.0 - float(i / steps < 0.0 or (i + 1) / steps > 0.6) for i in range(steps)]
    assert keep == [1.0, 1.0, 1.0, 0.0, 0.0]
    control = {"sd": cn_sd, "cond": torch.cat([ctrl.half().float()] * 2), "scale": [0.9 * k for k in keep]}
    ref = unet_ref.denoise_loop(sd, cfg, lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), text.float(), rs, 7.5,
                                controlnet=control)
    scale = ref.abs().max().item()
    assert torch.isfinite(out).all() and (out - ref).abs().max().item() < 4e-2 * scale, ((out - ref).abs().max().item(), scale)
    pipe.setup_controlnet(None)
    plain = pipe.txt2img(None, fused=False, **kw)[0].float().cpu()
    assert (plain - out).abs().max().item() > 1e-2 * scale                # the ControlNet residuals are live
    pipe.setup_controlnet(cn)
    with pytest.raises(NotImplementedError):
        pipe.txt2img(None, control_img=ctrl, fused=True, **kw)


def test_t2i_adapter_pipeline_vs_oracle(ops):
    """T2I-Adapter (reference t2i_adapter.py, model_k_diffusion.py:1086-1117, u_net_condition_modify.py:1194-1230): the
    adapter's four feature maps enter the UNet's down blocks during the first `adapter_conditioning_factor` of the steps.
    Adapter features against the oracle restatement; txt2img against the oracle loop with the same features."""
    from diffusionspatialcontrol_amd.modules import t2i_adapter as t2i
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    cfg, unet, sd, text = _tiny_setup(1)
    state, ids, rs = _region_state(n_img=1)
    torch.manual_seed(9)
    ad = t2i.T2IAdapter(channels=cfg.block_out_channels, num_res_blocks=2).half()
    ad_sd = {k: v.clone() for k, v in ad.state_dict().items()}
    ad = ad.cuda().eval()
    img = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(10))
    with torch.no_grad():
        feats = ad(img.half().cuda())
        rfeats = unet_ref.t2i_adapter_forward(ad_sd, img.half().float())
    assert [tuple(f.shape) for f in feats] == [(1, 32, 16, 16), (1, 64, 8, 8), (1, 64, 4, 4), (1, 64, 2, 2)]
    for a, b in zip(feats, rfeats):
        assert (a.float().cpu() - b).abs().max().item() < 1e-2 * max(b.abs().max().item(), 1e-3)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    t2i.setup_model_t2i_adapter(pipe, ad)
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(11)).half()
    steps = 5
    kw = dict(num_inference_steps=steps, guidance_scale=7.5, latents=lat.clone(), output_type="latent", region_map_state=state,
              sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"}, prompt_embeds=text[1:2],
              negative_prompt_embeds=text[:1], text_input_ids=ids)
    out = pipe.txt2img(None, height=None, width=None, image_t2i_adapter=img, adapter_conditioning_scale=0.8,
                       adapter_conditioning_factor=0.5, fused=False, **kw)[0].float().cpu()   # sizes from the adapter image (:990)
    sig = pipe.get_sigmas(steps, {"scheduler": "karras"}).half().float().cpu()
    adapter = {"state": [torch.cat([f * 0.8] * 2) for f in rfeats], "limit": int(len(sig) * 0.5)}
    ref = unet_ref.denoise_loop(sd, cfg, lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), text.float(), rs, 7.5,
                                adapter=adapter)
    scale = ref.abs().max().item()
    assert torch.isfinite(out).all() and (out - ref).abs().max().item() < 4e-2 * scale, ((out - ref).abs().max().item(), scale)
    plain = pipe.txt2img(None, height=128, width=128, fused=False, **kw)[0].float().cpu()
    assert (plain - out).abs().max().item() > 1e-2 * scale                       # the adapter features are live
    with pytest.raises(ValueError):
        t2i.setup_model_t2i_adapter(pipe, None)
        pipe.txt2img(None, height=128, width=128, image_t2i_adapter=img, **kw)


def test_inpainting_9_channel_unet(ops):
    """The inpainting checkpoints' UNet takes 9 input channels: [latents | mask | masked-image latents] (reference
    model_k_diffusion.py:1617-1619; the denoiser's c_in scales all nine, as the reference's call order makes it).  conv_in runs
    on the few-channel kernel (<= 16 channels).  Product vs the oracle loop with the same extra channels."""
    from diffusionspatialcontrol_amd.modules import sampling
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    import dataclasses
    torch.manual_seed(4)
    cfg = dataclasses.replace(UNetConfig.tiny(), in_channels=9)
    unet = UNet2DConditionModel(cfg).half()
    sd = {k: v.clone() for k, v in unet.state_dict().items()}
    unet = unet.cuda()
    g = torch.Generator().manual_seed(7)
    text = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half()
    state, ids, rs = _region_state(n_img=1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    img_lat = (torch.randn(1, 4, 16, 16, generator=g) * 0.7).half()
    mil = (torch.randn(1, 4, 16, 16, generator=g) * 0.7).half()
    mask = torch.zeros(1, 1, 128, 128)
    mask[..., 32:96] = 1.0
    steps = 4
    out = pipe.inpaiting(None, image=img_lat.clone(), mask_image=mask, masked_image_latents=mil.clone(), height=128, width=128,
                         num_inference_steps=steps, guidance_scale=7.5, output_type="latent", region_map_state=state,
                         sampler_name="sample_euler", sampler_opt={"scheduler": "karras"}, prompt_embeds=text[1:2],
                         negative_prompt_embeds=text[:1], text_input_ids=ids,
                         generator=torch.Generator().manual_seed(3))[0].float().cpu()
    sig = pipe.get_sigmas(steps, {"scheduler": "karras"}).half().float().cpu()
    noise = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3), dtype=torch.float16).float()
    m16 = F.interpolate(mask, size=(16, 16))
    extra = torch.cat([torch.cat([m16] * 2), torch.cat([mil.float()] * 2)], dim=1)
    ref = unet_ref.denoise_loop(sd, cfg, noise * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), text.float(), rs, 7.5,
                                sampler=sampling.sample_euler, extra_input=extra)
    sc = ref.abs().max().item()
    assert out.shape == (1, 4, 16, 16) and torch.isfinite(out).all()
    assert (out - ref).abs().max().item() < 4e-2 * sc, ((out - ref).abs().max().item(), sc)
    with pytest.raises(ValueError):
        pipe.inpaiting(None, image=img_lat.clone(), mask_image=mask, height=128, width=128, num_inference_steps=2,
                       prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], output_type="latent",
                       sampler_name="sample_euler")                                    # no pixels, no masked latents


def test_ip_adapter_unet_and_pipeline(ops):
    """IP-Adapter weights load into the UNet with the published key numbering (cross-attention
    layers numbered 1, 3, 5, ... over down_blocks, up_blocks, mid_block), the image tokens reach every cross-attention
    processor as the reference's (text, [tokens]) tuple, scale 0 is the identity, and fused == protocol mode."""
    from diffusionspatialcontrol_amd.modules import u_net_condition_modify as um, attention_modify as am
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import StableDiffusionPipeline
    torch.manual_seed(0)
    cfg = um.UNetConfig.tiny()
    unet = um.UNet2DConditionModel(cfg).half().cuda().eval()
    ctx = cfg.cross_attention_dim
    cross = [(n, m) for pre in ("down_blocks", "up_blocks", "mid_block") for n, m in unet.named_modules()
             if isinstance(m, um.Attention) and m.is_cross_attention and n.startswith(pre)]
    g = torch.Generator().manual_seed(3)
    emb_dim = 48
    sd = {"image_proj": {"proj.weight": torch.randn(4 * ctx, emb_dim, generator=g) * 0.1, "proj.bias": torch.zeros(4 * ctx),
                         "norm.weight": torch.ones(ctx), "norm.bias": torch.zeros(ctx)}, "ip_adapter": {}}
    for i, (n, m) in enumerate(cross):
        sd["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"] = torch.randn(m.inner_dim, ctx, generator=g) * 0.2 + i
        sd["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"] = torch.randn(m.inner_dim, ctx, generator=g) * 0.2
    x = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
    text = torch.randn(2, 77, ctx, generator=g).half().cuda()
    t = torch.tensor([500.0, 500.0]).cuda()
    with torch.no_grad():
        base = unet(x, t, encoder_hidden_states=text).sample
        assert unet._load_ip_adapter_weights([sd]) == {}
        procs = unet.attn_processors
        assert sum(isinstance(p, am.IPAdapterAttnProcessor2_0) for p in procs.values()) == len(cross)
        assert all(isinstance(p, am.AttnProcessor2_0) for n, p in procs.items() if ".attn1." in n)
        last = dict(unet.named_modules())[cross[-1][0]].processor           # the mid block carries the LAST key id
        assert cross[-1][0].startswith("mid_block")
        assert abs(last.to_k_ip[0].weight.float().mean().item() - (len(cross) - 1)) < 0.05
        img = [torch.randn(2, 1, emb_dim, generator=g).half().cuda()]
        with pytest.raises(ValueError):
            unet(x, t, encoder_hidden_states=text)                         # image_embeds required now (reference :1031-1034)
        out = unet(x, t, encoder_hidden_states=text, added_cond_kwargs={"image_embeds": img}).sample
        assert torch.isfinite(out).all() and (out - base).abs().max().item() > 1e-3
        for p in procs.values():
            if isinstance(p, am.IPAdapterAttnProcessor2_0):
                p.scale = [0.0]
        out0 = unet(x, t, encoder_hidden_states=text, added_cond_kwargs={"image_embeds": img}).sample
        # identity up to the run-to-run noise of MIOpen's atomic convolutions at this toy resolution (see the loop test)
        assert (out0 - base).abs().max().item() < 5e-3 < (out - base).abs().max().item()
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    pipe.set_ip_adapter_scale(0.7)
    lat = torch.randn(1, 4, 16, 16, generator=g).half()
    emb = torch.cat([torch.zeros_like(img[0][:1]), img[0][1:]])            # [negative; positive] along dim 0 (:207-215)
    kw = dict(height=128, width=128, num_inference_steps=4, guidance_scale=5.0, output_type="latent",
              sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"}, prompt_embeds=text[1:],
              negative_prompt_embeds=text[:1], ip_adapter_image_embeds=[emb])
    a = pipe.txt2img(None, fused=True, latents=lat.clone(), **kw)[0].float().cpu()
    b = pipe.txt2img(None, fused=False, latents=lat.clone(), **kw)[0].float().cpu()
    assert torch.isfinite(a).all() and (a - b).abs().max().item() < 3e-2 * max(1.0, b.abs().max().item())
    kw0 = dict(kw)
    kw0.pop("ip_adapter_image_embeds")
    with pytest.raises(ValueError):
        pipe.txt2img(None, fused=False, latents=lat.clone(), **kw0)        # adapter loaded, no image embeddings
    pipe.unload_ip_adapter()
    assert unet.encoder_hid_proj is None and all(isinstance(p, am.AttnProcessor) for p in unet.attn_processors.values())
    c = pipe.txt2img(None, fused=True, latents=lat.clone(), **kw0)[0].float().cpu()
    assert torch.isfinite(c).all() and (c - a).abs().max().item() > 1e-3   # the image prompt did steer the result


@pytest.mark.parametrize("n_img", [1, 2])
def test_diffusers_scheduler_pipeline_vs_oracle(ops, n_img):
    """the diffusers-scheduler loop (second caller of the processor boundary) with the Euler
    scheduler vs the oracle's restatement; n_img = 2 batches two images in ONE UNet call with the std of the scores over
    the whole call, exactly like the reference's num_images_per_prompt > 1."""
    from oracle import diffusers_ref
    from diffusionspatialcontrol_amd.modules.model_diffusers import EulerDiscreteScheduler, StableDiffusionPipeline_finetune
    cfg, unet, sd, text = _tiny_setup(n_img)
    state, ids, rs = _region_state(n_img=n_img)
    pipe = StableDiffusionPipeline_finetune(None, None, FakeTokenizer(), unet, EulerDiscreteScheduler())
    g = torch.Generator().manual_seed(2000)
    lat = torch.randn(n_img, 4, 16, 16, generator=g).half()
    pe, ne = text[n_img:n_img + 1], text[:1]
    text_rows = torch.cat([ne.repeat(n_img, 1, 1), pe.repeat(n_img, 1, 1)]).float()
    # ONE UNet call on all 2 * n_img rows with the whole-batch std (what every step of this loop does), tight tolerance
    with torch.no_grad():
        xr = torch.randn(2 * n_img, 4, 16, 16, generator=g).half()
        tr = torch.full((2 * n_img,), 601.0)
        rp = {"region_state": rs, "sigma": torch.tensor(3.5), "weight_func": lambda w, s, qk: w * s * qk.std()}
        o1 = unet(xr.cuda(), tr.cuda(), text_rows.half().cuda(), cross_attention_kwargs={"region_prompt": rp}).sample.float().cpu()
        r1 = unet_ref.unet_forward(sd, cfg, xr.float(), tr, text_rows, region_prompt={"region_state": rs, "sigma": 3.5, "weight_func": None},
                                   n_std_groups=1)
        sc1 = r1.abs().max().item()
        assert (o1 - r1).abs().max().item() < 1e-2 * sc1 + 1e-3 and (o1 - r1).abs().mean().item() < 2e-3 * sc1
    # mild guidance: tight agreement (CFG multiplies the fp16-vs-fp32 difference of eps by the guidance scale, and the
    # Euler steps integrate it over sigma = 8.4 .. 0)
    for gs, tol_max, tol_mean in ((1.5, 6e-2, 1.2e-2), (6.0, 2.5e-1, 4e-2)):
        out = pipe(height=128, width=128, num_inference_steps=5, guidance_scale=gs, latents=lat.clone(), output_type="latent",
                   prompt_embeds=pe, negative_prompt_embeds=ne, region_map_state=state, text_input_ids=ids,
                   num_images_per_prompt=n_img)[0].float().cpu()
        ref = diffusers_ref.euler_txt2img(sd, cfg, lat.float(), text_rows, rs, gs, 5)
        scale = ref.abs().max().item()
        assert torch.isfinite(out).all()
        assert (out - ref).abs().max().item() < tol_max * scale, (gs, (out - ref).abs().max().item(), scale)
        assert (out - ref).abs().mean().item() < tol_mean * scale, (gs, (out - ref).abs().mean().item(), scale)
    # the region masks steer the result
    plain = pipe(height=128, width=128, num_inference_steps=5, guidance_scale=6.0, latents=lat.clone(), output_type="latent",
                 prompt_embeds=pe, negative_prompt_embeds=ne, num_images_per_prompt=n_img)[0].float().cpu()
    assert (plain - out).abs().max().item() > 1e-3 * scale
    # ControlNet residual hooks (reference u_net_condition_modify.py:1236-1245,1269-1270): zero residuals are the identity
    with torch.no_grad():
        x = lat[:1].repeat(2, 1, 1, 1).cuda()
        t = torch.tensor([500.0, 500.0]).cuda()
        base = unet(x, t, text[:2].cuda()).sample
        skips = []
        hooks = []
    from diffusionspatialcontrol_amd.modules import u_net_condition_modify as um
    shapes = [(2, 32, 16, 16)] * 3 + [(2, 32, 8, 8), (2, 64, 8, 8), (2, 64, 8, 8), (2, 64, 4, 4), (2, 64, 4, 4), (2, 64, 4, 4),
                                       (2, 64, 2, 2), (2, 64, 2, 2), (2, 64, 2, 2)]
    res = [torch.zeros(sh, dtype=torch.half, device="cuda").contiguous(memory_format=torch.channels_last) for sh in shapes]
    with torch.no_grad():
        z = unet(x, t, text[:2].cuda(), down_block_additional_residuals=res,
                 mid_block_additional_residual=torch.zeros(2, 64, 2, 2, dtype=torch.half, device="cuda")).sample
        res[0] = res[0] + 0.5
        nz = unet(x, t, text[:2].cuda(), down_block_additional_residuals=res,
                  mid_block_additional_residual=torch.zeros(2, 64, 2, 2, dtype=torch.half, device="cuda")).sample
    assert (z - base).abs().max().item() < 5e-3 and (nz - base).abs().max().item() > 1e-3


def test_diffusers_img2img_inpaint_controlnet_pipelines(ops):
    """The other five classes of reference model_diffusers.py (img2img :1228-, inpaint :1515-, ControlNet :418-, ControlNet
    img2img :826-, ControlNet inpaint :1921-) against the oracle's Euler loop: truncated schedule with the region sigma read at
    the loop index (quirk q5), add_noise start, post-step re-imposition of the known region, per-step ControlNet."""
    from oracle import diffusers_ref
    from diffusionspatialcontrol_amd.modules import model_diffusers as md
    cfg, unet, sd, text = _tiny_setup(1)
    state, ids, rs = _region_state(n_img=1)
    cn, cn_sd = _controlnet(cfg)
    cn = cn.cuda().eval()
    pe, ne = text[1:2], text[:1]
    rows = torch.cat([ne, pe]).float()
    steps, gs = 6, 1.5
    ts, sigmas, init = diffusers_ref.euler_schedule(steps)
    lat0 = (torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(31)) * 0.7).half()
    ctrl = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(32))
    mask = torch.zeros(1, 1, 128, 128)
    mask[..., :64, :] = 1.0
    m16 = F.interpolate(mask, size=(16, 16))
    common = dict(num_inference_steps=steps, guidance_scale=gs, output_type="latent", prompt_embeds=pe,
                  negative_prompt_embeds=ne, region_map_state=state, text_input_ids=ids, height=128, width=128)
    noise = lambda seed: torch.randn(lat0.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float16).float()  # noqa: E731
    control = {"sd": cn_sd, "cond": torch.cat([ctrl.half().float()] * 2)}

    def check(out, ref, what):
        sc = ref.abs().max().item()
        assert torch.isfinite(out).all() and (out - ref).abs().max().item() < 6e-2 * sc, (what, (out - ref).abs().max().item(), sc)

    # img2img: strength 0.5 -> the last 3 of 6 steps
    pipe = md.StableDiffusionImg2ImgPipeline_finetune(None, None, FakeTokenizer(), unet, md.EulerDiscreteScheduler())
    out = pipe(image=lat0.clone(), strength=0.5, generator=torch.Generator().manual_seed(41), **common)[0].float().cpu()
    t0 = steps - int(steps * 0.5)
    start = lat0.float() + float(sigmas[t0]) * noise(41)
    check(out, diffusers_ref.euler_run(sd, cfg, start, ts, sigmas, t0, rows, rs, gs), "img2img")
    # inpainting, strength 1: pure noise start, known region re-imposed after every step
    pipe = md.StableDiffusionInpaintPipeline_finetune(None, None, FakeTokenizer(), unet, md.EulerDiscreteScheduler())
    out = pipe(image=lat0.clone(), mask_image=mask, strength=1.0, generator=torch.Generator().manual_seed(42), **common)[0].float().cpu()
    n42 = noise(42)

    def keep(i, x):
        known = lat0.float() + (float(sigmas[i + 1]) * n42 if i < steps - 1 else 0.0)
        return (1 - m16) * known + m16 * x
    ref = diffusers_ref.euler_run(sd, cfg, n42 * init, ts, sigmas, 0, rows, rs, gs, after_step=keep)
    check(out, ref, "inpaint")
    assert (out * (1 - m16) - lat0.float() * (1 - m16)).abs().max().item() < 2e-2 * lat0.float().abs().max().item()   # known half kept
    # ControlNet t2i, guidance window [0, 0.5]
    pipe = md.StableDiffusionControlNetPipeline_finetune(None, None, FakeTokenizer(), unet, cn, md.EulerDiscreteScheduler())
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(43)).half()
    out = pipe(image=ctrl, latents=lat.clone(), controlnet_conditioning_scale=0.8, control_guidance_end=0.5, **common)[0].float().cpu()
    keep_s = [0.8 * (1.0 - float((i + 1) / steps > 0.5)) for i in range(steps)]
    ref = diffusers_ref.euler_run(sd, cfg, lat.float() * init, ts, sigmas, 0, rows, rs, gs, controlnet=dict(control, scale=keep_s))
    check(out, ref, "controlnet")
    # ControlNet img2img and ControlNet inpaint: the same pieces combined
    pipe = md.StableDiffusionControlNetImg2ImgPipeline_finetune(None, None, FakeTokenizer(), unet, cn, md.EulerDiscreteScheduler())
    out = pipe(image=lat0.clone(), control_image=ctrl, strength=0.5, generator=torch.Generator().manual_seed(44), **common)[0].float().cpu()
    start = lat0.float() + float(sigmas[t0]) * noise(44)
    ref = diffusers_ref.euler_run(sd, cfg, start, ts, sigmas, t0, rows, rs, gs, controlnet=dict(control, scale=[1.0] * 3))
    check(out, ref, "controlnet img2img")
    pipe = md.StableDiffusionControlNetInpaintPipeline_finetune(None, None, FakeTokenizer(), unet, cn, md.EulerDiscreteScheduler())
    out = pipe(image=lat0.clone(), mask_image=mask, control_image=ctrl, generator=torch.Generator().manual_seed(42), **common)[0].float().cpu()
    ref = diffusers_ref.euler_run(sd, cfg, n42 * init, ts, sigmas, 0, rows, rs, gs, after_step=keep,
                                  controlnet=dict(control, scale=[1.0] * steps))
    check(out, ref, "controlnet inpaint")
    with pytest.raises(ValueError):
        md.StableDiffusionControlNetImg2ImgPipeline_finetune(None, None, FakeTokenizer(), unet, cn, md.EulerDiscreteScheduler())(
            image=lat0.clone(), strength=0.5, **common)                       # control_image missing


def test_prompt_string_pipeline(ops):
    """`txt2img(prompt=..., negative_prompt=...)` through the A1111-style encoder (emphasis, BREAK,
    75-token chunks) on a fake tokenizer / text encoder == the same call with the embeddings and token ids passed in;
    a prompt longer than one chunk (S = 154) generates through the long-prompt attention path."""
    from inputs import FakeClipTokenizer, fake_text_encoder
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.encoder_prompt_modify import encode_prompt_function
    cfg, unet, sd, _ = _tiny_setup(1)
    tok, enc = FakeClipTokenizer(), fake_text_encoder(dim=cfg.cross_attention_dim)
    pipe = StableDiffusionPipeline(None, enc, tok, unet, SD15Scheduler())
    state = {"red apple": {"map": rect_map(128, 128, 0, 0, 1, 2), "weight": 0.5, "mask_outsides": 0.0}}
    prompt, neg = "a photo of a (red apple:1.3) on a [wooden] table, near a blue vase", "blurry, low quality"
    g = torch.Generator().manual_seed(31)
    lat = torch.randn(1, 4, 16, 16, generator=g).half()
    kw = dict(height=128, width=128, num_inference_steps=4, guidance_scale=5.0, output_type="latent",
              sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"}, region_map_state=state)
    a = pipe.txt2img(prompt, negative_prompt=neg, latents=lat.clone(), **kw)[0].float().cpu()
    pe, ne, ids = encode_prompt_function(pipe, prompt, "cpu", 1, True, neg, long_encode=0)
    assert pe.shape == (1, 77, cfg.cross_attention_dim) and ids[1].shape == (1, 77)
    b = pipe.txt2img(None, latents=lat.clone(), prompt_embeds=pe.half(), negative_prompt_embeds=ne.half(), text_input_ids=ids,
                     **kw)[0].float().cpu()
    assert torch.isfinite(a).all() and (a - b).abs().max().item() < 2e-2 * max(1.0, b.abs().max().item())
    long_prompt = ", ".join(f"item{i} with (detail:1.2)" for i in range(30)) + " BREAK a red apple"
    c = pipe.txt2img(long_prompt, negative_prompt=neg, latents=lat.clone(), **kw)[0].float().cpu()
    pe2, _, ids2 = encode_prompt_function(pipe, long_prompt, "cpu", 1, True, neg, long_encode=0)
    assert pe2.shape[1] > 77 and pe2.shape[1] % 77 == 0 and ids2[0].shape == ids2[1].shape
    assert torch.isfinite(c).all() and (c - a).abs().max().item() > 1e-3


@pytest.fixture
def library_routing(ops):
    """ops.linear with the round-2 routing (few-row / long-K GEMMs to hipBLASLt): off by default since round 3"""
    saved = (ops.USE_LIBRARY_GEMM, ops.USE_LT_RESIDUAL, ops.USE_LT_ALL)
    ops.USE_LIBRARY_GEMM = ops.USE_LT_RESIDUAL = ops.USE_LT_ALL = True
    yield ops
    ops.USE_LIBRARY_GEMM, ops.USE_LT_RESIDUAL, ops.USE_LT_ALL = saved


def test_library_gemms_on_two_streams_finish_and_need_no_workspace(library_routing):
    """(The library is no longer in the step - every linear runs on the package's own kernels - but dsc_linear_lt_f16 stays as a
    non-default fallback, DSC_LIBRARY_GEMM=1, and keeps its guarantees.)  The recorded two-stream hang (round 1: every hipBLASLt candidate timed as a concurrent pair on two streams) came from
    stream-K / split-K algorithms whose workgroups spin on partial tiles of workgroups that a second stream's kernels keep
    from being scheduled.  dsc_linear_lt_f16 only admits workspace-free algorithms (each workgroup owns its output tiles: no
    inter-workgroup wait, live under any residency).  Here: two host threads push every library-GEMM shape of the SD1.5 step
    through it on two streams at once, 40 rounds each, inside a time bound; results equal the one-stream results; and the
    library's own bookkeeping shows that no admitted algorithm asked for a workspace."""
    import ctypes
    import threading
    from diffusionspatialcontrol_amd import _lib
    if not _lib.load_library().dsc_has_library_gemm():
        pytest.skip("default build: hipBLASLt is not compiled in (DSC_WITH_HIPBLASLT=1 at build time restores the fallback)")
    ops = library_routing
    shapes = [(512, 1280, 5120), (2048, 640, 2560), (8192, 320, 1280), (512, 1280, 2560), (512, 1280, 1920), (128, 1280, 1280),
              (128, 1280, 5120), (128, 1280, 2560), (2048, 640, 1920), (2048, 640, 1280), (8192, 320, 960)]
    g = torch.Generator().manual_seed(9)
    ops_in = []
    for M, N, K in shapes:
        x = torch.randn(M, K, generator=g).half().cuda()
        w = (torch.randn(N, K, generator=g) / K ** 0.5).half().cuda()
        b = torch.randn(N, generator=g).half().cuda()
        r = torch.randn(M, N, generator=g).half().cuda()
        ops_in.append((x, w, b, r))
    want = [ops.linear(x, w, b, residual=r).clone() for x, w, b, r in ops_in]       # plans built, one stream
    torch.cuda.synchronize()
    st3 = (ctypes.c_longlong * 3)()
    _lib.load_library().dsc_linear_lt_stats(st3)
    assert st3[0] >= 8 and st3[1] > 0                                              # these shapes do go through the library
    streams = [torch.cuda.Stream() for _ in range(2)]
    bad, errs = [], []

    def drive(j):
        try:
            _lib.load_library().dsc_set_workspace_slot(j)
            with torch.cuda.stream(streams[j]):
                for _ in range(40):
                    for (x, w, b, r), ref in zip(ops_in, want):
                        if not torch.equal(ops.linear(x, w, b, residual=r), ref):
                            bad.append(j)
            streams[j].synchronize()
        except BaseException as e:   # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=drive, args=(j,), daemon=True) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "library GEMMs on two streams did not finish within 120 s"
    assert not errs and not bad, (errs, bad)


def test_two_generations_in_flight_match_sequential(ops):
    """Generation slots: two host threads drive two different generations (prompt rows, masks, latents) on two streams
    through one pipeline - each slot has its own static buffers, captured step, packed text K/V and library-GEMM
    workspace.  Every kernel is bit-reproducible, so the concurrent results must EQUAL the sequential ones; a shared
    buffer between the slots would show up as a difference."""
    import threading
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    import bench
    torch.manual_seed(3)
    with torch.device("cuda"):
        unet = UNet2DConditionModel(UNetConfig.sd15())
    unet = unet.half().eval()
    emb0, ids, state, tok = bench.synthetic_inputs(512, 2)
    pipe = StableDiffusionPipeline(None, None, tok, unet, SD15Scheduler())
    jobs = []
    for j in range(2):
        g = torch.Generator().manual_seed(50 + j)
        emb = (emb0 + 0.05 * j * torch.randn(emb0.shape, generator=g)).half().cuda()
        lat = torch.randn(1, 4, 64, 64, generator=g).half().cuda()
        jobs.append(dict(height=512, width=512, num_inference_steps=6, guidance_scale=7.5, latents=lat, output_type="latent",
                         region_map_state=state, sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"},
                         prompt_embeds=emb[1:2], negative_prompt_embeds=emb[0:1], text_input_ids=ids))
    torch.cuda.synchronize()
    want = [pipe.txt2img(None, **job)[0].clone() for job in jobs]                    # sequential, slot 0
    # no synchronisation here: slot 0's buffers are about to be driven from another stream while the default stream may
    # still be replaying the second job - the slot's completion event orders the two
    streams = [torch.cuda.Stream() for _ in jobs]
    for j, job in enumerate(jobs):                                                   # per-slot capture, one at a time
        with torch.cuda.stream(streams[j]):
            pipe.txt2img(None, slot=j, **job)
        torch.cuda.synchronize()
    got, errs = [[], []], []

    def drive(j):
        try:
            with torch.cuda.stream(streams[j]):
                for _ in range(3):
                    got[j].append(pipe.txt2img(None, slot=j, **jobs[j])[0])
        except BaseException as e:   # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=drive, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs
    assert not torch.equal(want[0], want[1])
    diffs = [[(o.float() - want[j].float()).abs().max().item() for o in got[j]] for j in range(2)]
    assert all(d == 0.0 for row in diffs for d in row), diffs
    # protocol mode (any sampler, graph-backed model calls) in the slots: Euler, two threads, against slot 0 alone
    ejobs = [dict(job, sampler_name="sample_euler", fused=False) for job in jobs]
    ewant = [pipe.txt2img(None, **job)[0].clone() for job in ejobs]
    for j, job in enumerate(ejobs):
        with torch.cuda.stream(streams[j]):
            pipe.txt2img(None, slot=j, **job)
        torch.cuda.synchronize()
    egot = [None, None]

    def edrive(j):
        try:
            with torch.cuda.stream(streams[j]):
                for _ in range(2):
                    egot[j] = pipe.txt2img(None, slot=j, **ejobs[j])[0]
        except BaseException as e:   # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=edrive, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errs, errs
    assert all(torch.equal(egot[j], ewant[j]) for j in range(2)) and not torch.equal(ewant[0], ewant[1])
    with pytest.raises(NotImplementedError):                      # CFG rescale needs the eager model call: no slots there
        pipe.txt2img(None, slot=1, fused=False, guidance_rescale=0.5, **jobs[0])


def test_diffusers_pipeline_graph_replay_equals_eager(ops):
    """The captured-step path of the diffusers-scheduler pipelines (`_denoise_graph`: PROTOCOL_GRAPH on) against the eager loop
    (off) on the same inputs: the captured UNet reads the ResNets' time-embedding terms from a static buffer that the loop
    must fill per timestep (round-2 advisor finding: it stayed zero, the denoiser was timestep-blind, and a 6e-2 tolerance on
    a random-init UNet did not notice).  Tight tolerance: the two are the same kernels with the same operands up to the shared
    CFG prefix's launch geometry; and the buffer holds `temb_add_table(t)` for the last replayed timestep."""
    from diffusionspatialcontrol_amd import ops as dops
    from diffusionspatialcontrol_amd.modules.model_diffusers import EulerDiscreteScheduler, StableDiffusionPipeline_finetune
    cfg, unet, sd, text = _tiny_setup(1)
    state, ids, rs = _region_state(n_img=1)
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(2001)).half()
    pe, ne = text[1:2], text[:1]
    outs = {}
    saved = (dops.PROTOCOL_GRAPH, dops.USE_TEMB_HOIST, dops.USE_CFG_SHARED_PREFIX)
    try:
        for name, (graph, hoist, prefix) in {"eager": (False, True, True), "graph": (True, True, True),
                                             "graph_nohoist": (True, False, True), "graph_noprefix": (True, True, False)}.items():
            dops.PROTOCOL_GRAPH, dops.USE_TEMB_HOIST, dops.USE_CFG_SHARED_PREFIX = graph, hoist, prefix
            pipe = StableDiffusionPipeline_finetune(None, None, FakeTokenizer(), unet, EulerDiscreteScheduler())
            outs[name] = pipe(height=128, width=128, num_inference_steps=5, guidance_scale=6.0, latents=lat.clone(),
                              output_type="latent", prompt_embeds=pe, negative_prompt_embeds=ne, region_map_state=state,
                              text_input_ids=ids)[0].float().cpu()
            if graph:
                st = next(iter(pipe._graphs.values()))
                assert (st["tadd"] is not None) == hoist
                if hoist:                                   # the buffer holds the last timestep's rows, not zeros
                    t_last = float(pipe.scheduler.timesteps[-1])
                    want = unet.temb_add_table(torch.tensor([t_last], dtype=torch.float32, device="cuda"))[0]
                    assert st["tadd"].abs().max().item() > 0
                    assert torch.equal(st["tadd"][0], want) and torch.equal(st["tadd"][1], want)
    finally:
        dops.PROTOCOL_GRAPH, dops.USE_TEMB_HOIST, dops.USE_CFG_SHARED_PREFIX = saved
    scale = outs["eager"].abs().max().item()
    for name in ("graph", "graph_nohoist", "graph_noprefix"):
        err = (outs[name] - outs["eager"]).abs()
        # 5 Euler steps at guidance 6 on the same kernels: rounding-level differences only (shared prefix: other launch geometry
        # in the first layers; toy widths also run MIOpen's atomic convolutions).  A zero time-embedding buffer gives > 0.3 here.
        assert err.max().item() < 2e-2 * scale and err.mean().item() < 3e-3 * scale, (name, err.max().item(), err.mean().item(), scale)


@pytest.mark.parametrize("rows,n", [(7, 64), (300, 4096), (33, 1000), (5, 16384)])
def test_softmax_rows(ops, rows, n):
    """dsc_softmax_rows_f16 (the VAE attention head's middle step) vs fp32 torch softmax of the same fp16 scores; in place too"""
    g = torch.Generator().manual_seed(rows + n)
    s = (torch.randn(rows, n, generator=g) * 6).half()
    ref = torch.softmax(s.float() * 0.37, dim=-1)
    sc = s.cuda()
    out = ops.softmax_rows(sc, scale=0.37)
    assert (out.float().cpu() - ref).abs().max().item() < 1e-3 * ref.max().item() + 1e-6
    assert (out.float().sum(-1).cpu() - 1).abs().max().item() < 2e-3
    again = ops.softmax_rows(sc, scale=0.37, out=sc)               # in place: each workgroup owns its row
    assert again.data_ptr() == sc.data_ptr() and torch.equal(again, out)


@pytest.mark.parametrize("B,hw,cin,cout,groups", [(2, 64, 320, 320, 32), (2, 32, 640, 640, 32), (2, 32, 320, 640, 32), (1, 96, 320, 320, 32),
                                                  (3, 16, 64, 128, 8), (2, 64, 64, 64, 1)])
def test_groupnorm_statistics_from_the_convolution_epilogue(ops, B, hw, cin, cout, groups):
    """dsc_conv3x3_gn_nhwc_f16 + dsc_groupnorm_apply_nhwc (round 3): the convolution adds the per-image bias row (the ResNet
    block's time-embedding term), stores the same bytes as dsc_conv3x3_nhwc_f16 would for that sum, and emits per-(pixel tile,
    group) partial sums from which the GroupNorm runs in ONE launch - against the two-launch GroupNorm of the same tensor and
    an fp32 reference; groups that straddle the 64-channel tiles (cpg = 10, 20), 72 partial rows per image (96 x 96), bit-stable."""
    g = torch.Generator().manual_seed(B * hw + cin + cout)
    x = (torch.randn(B, cin, hw, hw, generator=g) * 0.7).half().cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).half().cuda().contiguous(memory_format=torch.channels_last)
    bias = (torch.randn(cout, generator=g) * 0.2).half().cuda()
    add = (torch.randn(B, cout, generator=g) * 0.5).half().cuda()
    res = torch.randn(B, cout, hw, hw, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    gamma = (1 + 0.1 * torch.randn(cout, generator=g)).half().cuda()
    beta = (0.1 * torch.randn(cout, generator=g)).half().cuda()
    rows = ops.conv3x3_gn_rows(x, w, groups)
    if rows == 0:
        pytest.skip("shape not covered by the statistics-emitting form (split-K convolution or 8-wide tiles)")
    assert rows == ((hw + 7) // 8) * ((hw + 15) // 16)
    for kw in ({"add": add}, {"bias": bias, "residual": res}, {"bias": bias, "add": add, "residual": res}, {}):
        out = ops.conv3x3_gn(x, w, groups, **kw)
        part = ops.gn_partials_of(out)
        assert part is not None and part.rows == rows and tuple(part.buf.shape) == (B, rows, groups, 2, 2)
        ref = F.conv2d(x.float(), w.float(), kw.get("bias").float() if "bias" in kw else None, padding=1)
        if "add" in kw:
            ref = ref + add.float()[:, :, None, None]
        if "residual" in kw:
            ref = ref + res.float()
        assert torch.all((out.float() - ref).abs() <= 2e-3 * ref.abs() + 4e-3)
        if "add" not in kw:                                    # without the per-image row: the bytes of the plain entry
            assert torch.equal(out, ops.conv3x3(x, w, kw.get("bias"), kw.get("residual"), splits=1))
        for act in (True, False):
            one = ops.groupnorm_apply_nhwc(out, part, groups, gamma, beta, 1e-5, act)
            two = ops.groupnorm_silu_nhwc(out, groups, gamma, beta, 1e-5, act)
            gref = F.group_norm(out.float(), groups, gamma.float(), beta.float(), 1e-5)
            gref = F.silu(gref) if act else gref
            assert (one.float() - gref).abs().max().item() < 6e-3 and (one.float() - two.float()).abs().max().item() < 4e-3
        again = ops.conv3x3_gn(x, w, groups, **kw)               # (slot [g][1] of a group that straddles no tile boundary is never written)
        assert torch.equal(again, out) and torch.equal(ops.gn_partials_of(again).buf[..., 0, :], part.buf[..., 0, :])
        assert torch.equal(ops.groupnorm_apply_nhwc(again, ops.gn_partials_of(again), groups, gamma, beta, 1e-5, True),
                           ops.groupnorm_apply_nhwc(out, part, groups, gamma, beta, 1e-5, True))


@pytest.mark.parametrize("offset", [12.0, 60.0])
def test_groupnorm_epilogue_statistics_with_a_large_channel_offset(ops, offset):
    """The epilogue statistics are fp32 (sum, sum of squares) partials per (pixel tile, group) reduced in fp64: a group whose mean is
    tens of standard deviations (a large bias / DC offset of the residual stream, as trained checkpoints have in some channels)
    must normalise as well from them as from the two-launch GroupNorm's own pass over the tensor.  Against fp32 group_norm."""
    B, hw, cin, cout, groups = 2, 32, 320, 640, 32
    g = torch.Generator().manual_seed(int(offset))
    x = (torch.randn(B, cin, hw, hw, generator=g) * 0.7).half().cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).half().cuda().contiguous(memory_format=torch.channels_last)
    bias = torch.randn(cout, generator=g) * 0.2
    bias[: cout // 2] += offset                                  # half of the groups sit far from zero
    bias = bias.half().cuda()
    gamma = (1 + 0.1 * torch.randn(cout, generator=g)).half().cuda()
    beta = (0.1 * torch.randn(cout, generator=g)).half().cuda()
    out = ops.conv3x3_gn(x, w, groups, bias=bias)
    part = ops.gn_partials_of(out)
    assert part is not None
    gref = F.group_norm(out.float(), groups, gamma.float(), beta.float(), 1e-5)
    one = ops.groupnorm_apply_nhwc(out, part, groups, gamma, beta, 1e-5, False)
    two = ops.groupnorm_silu_nhwc(out, groups, gamma, beta, 1e-5, False)
    e1, e2 = (one.float() - gref).abs(), (two.float() - gref).abs()
    assert e1.max().item() <= 2.0 * e2.max().item() + 4e-3 and e1.mean().item() <= 2.0 * e2.mean().item() + 2e-4, \
        (e1.max().item(), e2.max().item(), e1.mean().item(), e2.mean().item())
    # the relative bound alone passes when both forms are wrong together: each against an fp64 GroupNorm of the same tensor, with
    # the bound of test_groupnorm_silu_nhwc
    grp = out.double().reshape(B, groups, -1)
    mean = grp.mean(dim=2, keepdim=True)
    norm = ((grp - mean) / torch.sqrt(((grp - mean) ** 2).mean(dim=2, keepdim=True) + 1e-5)).reshape(B, cout, hw, hw)
    ref64 = norm * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
    for name, y in (("one", one), ("two", two)):
        err = (y.double() - ref64).abs()
        assert err.max().item() < 4e-3 * max(1.0, ref64.abs().max().item()) and err.mean().item() < 4e-4, \
            (name, err.max().item(), err.mean().item())


@pytest.mark.parametrize("B,L,K,N,groups", [(2, 4096, 320, 320, 32), (2, 1024, 640, 640, 32), (2, 4096, 960, 320, 32), (2, 1024, 1920, 640, 32),
                                            (4, 256, 128, 64, 4)])
def test_groupnorm_statistics_from_the_gemm_epilogue(ops, B, L, K, N, groups):
    """dsc_linear_gn_f16: the 1x1 convolutions (proj_out, conv_shortcut) as token-major GEMMs that also emit the GroupNorm partial
    sums of their output - same bytes as dsc_linear_f16, one-launch GroupNorm equal to the two-launch one up to summation order"""
    g = torch.Generator().manual_seed(B + L + K + N)
    x = torch.randn(B, L, K, generator=g).half().cuda()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
    b = (torch.randn(N, generator=g) * 0.2).half().cuda()
    r = torch.randn(B, L, N, generator=g).half().cuda()
    gamma = (1 + 0.1 * torch.randn(N, generator=g)).half().cuda()
    beta = (0.1 * torch.randn(N, generator=g)).half().cuda()
    got = ops.linear_gn(x, w, b, r, L, groups)
    assert got is not None
    y, part = got
    assert torch.equal(y, ops.linear(x, w, b, residual=r, prefer_kernel=True))
    side = int(round(L ** 0.5))
    img = y.reshape(B, side, side, N).permute(0, 3, 1, 2)                          # channels_last view of the token tensor
    for act in (True, False):
        one = ops.groupnorm_apply_nhwc(img, part, groups, gamma, beta, 1e-6, act)
        two = ops.groupnorm_silu_nhwc(img, groups, gamma, beta, 1e-6, act)
        gref = F.group_norm(img.float(), groups, gamma.float(), beta.float(), 1e-6)
        gref = F.silu(gref) if act else gref
        assert (one.float() - gref).abs().max().item() < 6e-3 and (one.float() - two.float()).abs().max().item() < 4e-3
    y2, part2 = ops.linear_gn(x, w, b, r, L, groups)
    assert torch.equal(y2, y) and torch.equal(part2.buf[..., 0, :], part.buf[..., 0, :])
    assert torch.equal(ops.groupnorm_apply_nhwc(img, part2, groups, gamma, beta, 1e-6, True), ops.groupnorm_apply_nhwc(img, part, groups, gamma, beta, 1e-6, True))


def test_groupnorm_partials_are_dropped_after_an_in_place_write(ops):
    """the partial sums ride on the tensor OBJECT the producer returned; a view made later or an in-place write since (torch's
    version counter) must not find them - the GroupNorm then computes its own statistics"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 32, 32, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24).half().cuda().contiguous(memory_format=torch.channels_last)
    if ops.conv3x3_gn_rows(x, w, 8) == 0:
        pytest.skip("shape not covered")
    out = ops.conv3x3_gn(x, w, 8)
    assert ops.gn_partials_of(out) is not None
    assert ops.gn_partials_of(out[:]) is None and ops.gn_partials_of(out.clone()) is None
    out.mul_(2.0)
    assert ops.gn_partials_of(out) is None
