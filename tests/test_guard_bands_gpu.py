"""Guard bands around the C entry points of include/dsc_hip.h: where the kernels write, at which strides, into how much scratch.

ops.py allocates outputs, partial sums and scratch itself, from torch's caching allocator, always with ldo = N / Cout, ldx = Cin and
a workspace rounded up: a store one row, pixel or chunk past the end, a stride argument that is ignored, or a *_workspace_bytes
answer that is too small would land in a neighbouring block and no value test would see it.  Here every entry point is called the
way ops.py calls it (raw pointers, torch's current stream) with

    destinations   views into sentinel-filled buffers (tests/guards.py `fenced`) at a row stride that differs from the row length,
                   followed by one full kernel tile of fence (128 rows): an overhanging store fails the test, never faults;
    strided inputs `poisoned`: NaN in every row gap, before the first and after the last row - a read past K, Cin, row M - 1 or the
                   last pixel that reaches a stored value turns it into NaN;
    scratch        of EXACTLY the bytes the *_workspace_bytes function answers, at exactly the alignment the entry point asks for,
                   NaN-filled, fenced on both sides (`exact_scratch`).

Each case asserts (a) DSC_OK, (b) every fence intact after the launch, (c) the fenced result equal bit for bit to the same
operation through ops.* on compact operands - strides move addresses, not the order of any sum - and (d) that compact result within
the bound the existing test of the op uses, against an fp32 / fp64 reference computed on the CPU (tests/guard_band_refs.py).
No case hands a launching call less memory than it needs; the only "one byte short" call is of an entry point that refuses before
any launch (dsc_linear_splitk_f16: the size check precedes linear_impl).  Shapes are the smallest at which the named edge exists.
"""
import pytest
import torch

import guard_band_refs as R
import guards as G
from inputs import attn_inputs
from oracle import region_attention as ra
from test_region_xattn_gpu import tol16

pytestmark = pytest.mark.gpu

DSC_OK, DSC_ERR_UNSUPPORTED, DSC_ERR_WORKSPACE = 0, -2, -3
# dsc_debug_set_gemm_stages settings (tests/test_unet_pipeline_gpu.py::test_linear_kernel_tilings_agree_bit_for_bit): ring depth,
# 64- / 128-row tiles, loader waves, 128-column tiles, workgroup order.  GEGLU has no 64-row tiles: those three are skipped there.
GEMM_STAGES = (0, 90643, 40643, 90642, 91283, 41283, 90002, 200000, 291282, 1000000, 2000000)
GEMM_STAGES_64_ROWS = (90643, 40643, 90642)
CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from diffusionspatialcontrol_amd import _lib
    return _lib.load_library()


@pytest.fixture
def gemm_stages(lib):
    """set(knob) switches the GEMM launch variant; the measured rule is back after the test, whatever it did"""
    try:
        yield lib.dsc_debug_set_gemm_stages
    finally:
        lib.dsc_debug_set_gemm_stages(0)


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * s for i, s in enumerate(seed)) % (1 << 31))


def _breached(*pairs):
    """after the stream has drained: the indices of the (buf, view) pairs with a sentinel outside the view gone; [] = all intact"""
    torch.cuda.synchronize()
    return [i for i, (buf, view) in enumerate(pairs) if not G.untouched(buf, view)]


def _gemm_operands(M, N, K, seed, R_rows=None):
    """test_linear_kernel's distributions: (x, w, bias, residual) on the CPU"""
    g = _gen(M, N, K, seed)
    x = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    b = (torch.randn(N, generator=g) * 0.2).half()
    r = torch.randn(R_rows or M, N, generator=g).half()
    return x, w, b, r


def test_the_detector_on_the_device():
    """tests/test_guards_host.py on CUDA tensors, in short: a stray element written with torch (no kernel is edited) is seen in the
    lead, in a row gap, behind the last row and around an exact scratch; writes inside the view are not"""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    buf, view = G.fenced(5, 24, 32, lead=16, tail_rows=2)
    view.fill_(1.0)
    assert view.is_cuda and view.data_ptr() % 16 == 0 and G.untouched(buf, view)
    for index in (15, 16 + 24, 16 + 4 * 32 + 24, 16 + 5 * 32, buf.numel() - 1):
        G.bits(buf)[index] = 0
        assert not G.untouched(buf, view), index
        G.bits(buf)[index] = G.sentinel(torch.float16)
        assert G.untouched(buf, view), index
    pbuf, pview = G.poisoned(torch.arange(12, dtype=torch.float32, device="cuda").view(3, 4), 8)
    assert torch.equal(pview, torch.arange(12, device="cuda").view(3, 4).float()) and G.untouched(pbuf, pview)
    assert int(torch.isnan(pbuf).sum()) == pbuf.numel() - 12
    sbuf, ws = G.exact_scratch(4096 + 16, 8, torch.float64)
    assert ws.data_ptr() % 16 == 8 and torch.isnan(ws).all() and G.untouched(sbuf, ws)
    ws.zero_()
    assert G.untouched(sbuf, ws)
    sbuf[ws.storage_offset() + ws.numel()] = 0.0
    assert not G.untouched(sbuf, ws)


# ============================================================================= GEMM family (gemm.hip)
@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("N", [64, 192, 256])
@pytest.mark.parametrize("M", [1, 63, 65, 129, 200])
def test_linear_f16(ops, lib, gemm_stages, M, N, K):
    """dsc_linear_f16 with ldx = K + 8, ldr = N + 16, ldo = N + 8: rows on both sides of the 64- and 128-row tile edges, one to
    four 64-column blocks (N = 192: an odd count, no 128-column tile), one and three K steps.  M = 65, N = 192 under the XCD-aware
    order is 2 x 3 = 6 tiles in a grid padded to 8: the two surplus workgroups store nothing."""
    x, w, b, r = _gemm_operands(M, N, K, 1)
    xp, rp = G.poisoned(x.cuda(), K + 8), G.poisoned(r.cuda(), N + 16)
    wd, bd = w.cuda(), b.cuda()
    for epilogue in (False, True):
        bias, res = (bd, rp[1]) if epilogue else (None, None)
        gemm_stages(0)
        compact = ops.linear(x.cuda(), wd, bias, residual=r.cuda() if epilogue else None, prefer_kernel=True)
        assert R.within(compact, R.linear(x, w, b if epilogue else None, r if epilogue else None), 1.5e-3, 2e-3)
        for knob in GEMM_STAGES:
            gemm_stages(knob)
            out = G.fenced(M, N, N + 8)
            rc = lib.dsc_linear_f16(ops._p(xp[1]), ops._p(wd), ops._p(bias), ops._p(res), ops._p(out[1]), M, N, K, K + 8, N + 16,
                                    N + 8, 0, 0, ops._stream_ptr(wd))
            assert rc == DSC_OK, (knob, epilogue)
            assert not _breached(out, xp, rp), (knob, epilogue)
            assert torch.equal(out[1], compact), (knob, epilogue)


def test_linear_f16_wrapped_residual(ops, lib, gemm_stages):
    """a residual of R = 128 rows under M = 256 (ldr = stride | R << 32): row m adds residual row m % R, and no row >= R is read
    into a stored value - behind row R - 1 the residual buffer is NaN"""
    M, R_rows, N, K = 256, 128, 192, 64
    x, w, b, r = _gemm_operands(M, N, K, 2, R_rows)
    xp, rp = G.poisoned(x.cuda(), K + 8), G.poisoned(r.cuda(), N + 16)
    wd, bd = w.cuda(), b.cuda()
    compact = ops.linear(x.cuda(), wd, bd, residual=r.cuda(), prefer_kernel=True)
    assert R.within(compact, R.linear(x, w, b, r), 1.5e-3, 2e-3)
    for knob in GEMM_STAGES:
        gemm_stages(knob)
        out = G.fenced(M, N, N + 8)
        rc = lib.dsc_linear_f16(ops._p(xp[1]), ops._p(wd), ops._p(bd), ops._p(rp[1]), ops._p(out[1]), M, N, K, K + 8,
                                (N + 16) | (R_rows << 32), N + 8, 0, 0, ops._stream_ptr(wd))
        assert rc == DSC_OK, knob
        assert not _breached(out, xp, rp), knob
        assert torch.equal(out[1], compact) and not torch.isnan(out[1]).any(), knob


@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("M", [1, 129])
def test_linear_f16_geglu(ops, lib, gemm_stages, M, N):
    """the GEGLU epilogue: out is [M, N / 2] at ldo = N / 2 + 8; N / 2 a multiple of 64, so 200000 launches the 128-column tile"""
    K = 64
    x, w, b, _ = _gemm_operands(M, N, K, 3)
    xp = G.poisoned(x.cuda(), K + 8)
    wd, bd = w.cuda(), b.cuda()
    compact = ops.linear(x.cuda(), wd, bd, geglu=True, prefer_kernel=True)
    assert R.within(compact, R.linear_geglu(x, w, b), 2e-3, 3e-3)
    for knob in GEMM_STAGES:
        if knob in GEMM_STAGES_64_ROWS:
            continue
        gemm_stages(knob)
        out = G.fenced(M, N // 2, N // 2 + 8)
        rc = lib.dsc_linear_f16(ops._p(xp[1]), ops._p(wd), ops._p(bd), None, ops._p(out[1]), M, N, K, K + 8, 0, N // 2 + 8, 1, 0,
                                ops._stream_ptr(wd))
        assert rc == DSC_OK, knob
        assert not _breached(out, xp), knob
        assert torch.equal(out[1], compact), knob


@pytest.mark.parametrize("N", [192, 256])
@pytest.mark.parametrize("M", [65, 129])
def test_linear_ln_f16(ops, lib, gemm_stages, M, N):
    """dsc_linear_ln_f16.  Producer: the row statistics ln_out [M][N / 64][2] (fp32, dense) in a fence - rows >= M of the last tile
    write none - and equal to the sums of the stored fp16 rows.  Consumer: ln_in with NaN behind row M - 1.  N = 256: under 291282
    the 128-column tile writes two statistics blocks per row and tile (another index into ln_out)."""
    K = 64
    a, wo, bo, xres = _gemm_operands(M, N, K, 4)
    xres = (xres.float() * 2 + 0.7).half()                         # a residual stream with a non-zero mean
    ap, rp = G.poisoned(a.cuda(), K + 8), G.poisoned(xres.cuda(), N + 16)
    wod, bod = wo.cuda(), bo.cuda()
    s_c, st_c = ops.linear_ln(a.cuda(), wod, bod, residual=xres.cuda(), ln_stats=True)
    assert R.within(s_c, R.linear(a, wo, bo, xres), 1.5e-3, 2e-3)
    # every block's fp32 sum of 64 values against fp64: at most 64 * 2^-24 of the sum of the magnitudes, whatever the order
    exact, mags = R.row_block_stats(s_c.cpu())
    assert torch.all((st_c.cpu().double() - exact).abs() <= 64 * 2.0 ** -24 * mags + 1e-30)
    g = _gen(M, N, 5)
    gamma, beta = (torch.randn(N, generator=g) * 0.3 + 1).half(), (torch.randn(N, generator=g) * 0.2).half()
    w, b = (torch.randn(N, N, generator=g) / N ** 0.5).half(), (torch.randn(N, generator=g) * 0.2).half()
    w2, b2, cvec = ops.fold_layernorm(w.cuda(), b.cuda(), gamma.cuda(), beta.cuda())
    y_c = ops.linear_ln(s_c, w2, b2, ln=(st_c, cvec, 1e-5))
    ref = R.layernorm_linear(s_c.cpu(), gamma, beta, w, b)
    err = (y_c.float().cpu() - ref).abs()
    assert err.max().item() < 2e-2 * max(1.0, ref.abs().max().item()) and err.mean().item() < 2e-3   # test_linear_layernorm_folding
    sp, stp = G.poisoned(s_c, N + 8), G.poisoned(st_c.reshape(M, -1))
    for knob in GEMM_STAGES:
        gemm_stages(knob)
        out, stats = G.fenced(M, N, N + 8), G.fenced(M, N // 64 * 2, dtype=torch.float32)
        rc = lib.dsc_linear_ln_f16(ops._p(ap[1]), ops._p(wod), ops._p(bod), ops._p(rp[1]), ops._p(out[1]), M, N, K, K + 8, N + 16,
                                   N + 8, 0, None, 0, None, 0.0, ops._p(stats[1]), 0, ops._stream_ptr(wod))
        assert rc == DSC_OK, knob
        assert not _breached(out, stats, ap, rp), knob
        assert torch.equal(out[1], s_c) and torch.equal(stats[1].view(M, N // 64, 2), st_c), knob
        y = G.fenced(M, N, N + 8)
        rc = lib.dsc_linear_ln_f16(ops._p(sp[1]), ops._p(w2), ops._p(b2), None, ops._p(y[1]), M, N, N, N + 8, 0, N + 8, 0,
                                   ops._p(stp[1]), N // 64, ops._p(cvec), 1e-5, None, 0, ops._stream_ptr(w2))
        assert rc == DSC_OK, knob
        assert not _breached(y, sp, stp), knob
        assert torch.equal(y[1], y_c), knob


@pytest.mark.parametrize("B,L,C,H", [(3, 40, 64, 2), (2, 64, 128, 4)])
def test_linear_qkv_f16(ops, lib, gemm_stages, B, L, C, H):
    """dsc_linear_qkv_f16: q_out at ldq = C + 8, kv_out [2][B][H][L][d] dense in a fence.  M = 120: row tiles straddle images and
    the last one is ragged, so the head-major scatter of rows >= M would land behind the last value row."""
    M, d = B * L, C // H
    g = _gen(B, L, C, H)
    x = (torch.randn(B, L, C, generator=g) * 1.3 + 0.2).half()
    w = (torch.randn(3 * C, C, generator=g) / C ** 0.5).half()
    b = (torch.randn(3 * C, generator=g) * 0.2).half()
    xp = G.poisoned(x.reshape(M, C).cuda(), C + 8)
    wd, bd = w.cuda(), b.cuda()
    q4, k4, v4 = ops.linear_qkv(x.cuda(), wd, bd, H)
    ref_q, ref_kv = R.head_major(R.linear(x.reshape(M, C), w, b), B, L, H)
    assert R.within(q4.reshape(M, C), ref_q, 1.5e-3, 2e-3)
    assert R.within(torch.stack([k4.permute(0, 2, 1, 3), v4.permute(0, 2, 1, 3)]), ref_kv, 1.5e-3, 2e-3)
    for knob in GEMM_STAGES:
        gemm_stages(knob)
        q, kv = G.fenced(M, C, C + 8), G.fenced(2 * B * H * L, d)
        rc = lib.dsc_linear_qkv_f16(ops._p(xp[1]), ops._p(wd), ops._p(bd), ops._p(q[1]), ops._p(kv[1]), M, C, C, C + 8, C + 8, H, L,
                                    None, 0, None, 0.0, 0, ops._stream_ptr(wd))
        assert rc == DSC_OK, knob
        assert not _breached(q, kv, xp), knob
        kv5 = kv[1].view(2, B, H, L, d)
        assert torch.equal(q[1], q4.reshape(M, C)), knob
        assert torch.equal(kv5[0], k4.permute(0, 2, 1, 3)) and torch.equal(kv5[1], v4.permute(0, 2, 1, 3)), knob


def _partials_whole(part, C, groups):
    """the producers' partial sums [B, rows, G, 2, 2] taken from a fence: every slot the consumer reads is written (slot 0 of every
    group, slot 1 of the groups that cross a 64-channel boundary), and every (sum, sum of squares) pair is finite or still the
    sentinel - never half-written"""
    words = G.bits(part)
    written = words != G.sentinel(torch.float32)
    live = torch.stack([torch.ones(groups, dtype=torch.bool), R.straddles(C, groups)], dim=1).to(part.device)
    return (bool(written[..., live, :].all()) and bool(torch.isfinite(part[written]).all())
            and bool((written[..., 0] == written[..., 1]).all()))


def _apply_from(lib, ops, rows_t, part, part_rows, B, C, hw, groups, gamma, beta, eps):
    """dsc_groupnorm_apply_nhwc of the compact rows [B hw, C] from the partial sums `part`, into a fenced y; the fence pair"""
    y = G.fenced(B * hw, C)
    rc = lib.dsc_groupnorm_apply_nhwc(ops._p(rows_t), ops._p(y[1]), ops._p(gamma), ops._p(beta), ops._p(part), part_rows, B, C, hw,
                                      groups, eps, 1, 0, ops._stream_ptr(rows_t))
    assert rc == DSC_OK
    return y


@pytest.mark.parametrize("B,L,K,N,groups", [(2, 64, 64, 64, 8), (3, 128, 64, 192, 32)])
def test_linear_gn_f16(ops, lib, gemm_stages, B, L, K, N, groups):
    """dsc_linear_gn_f16: gn_part [B][rows][G][2][2] in a fence, rows from dsc_linear_gn_rows under the same launch variant.  N = 192
    with 32 groups: 6 channels per group, groups cross the 64-column tiles, slot [g][1] is live.  A variant whose tile height does
    not divide the image's rows (128-row tiles, 64 rows) is refused before any launch."""
    M = B * L
    x, w, b, r = _gemm_operands(M, N, K, 6)
    g = _gen(N, groups)
    gamma, beta = (1 + 0.1 * torch.randn(N, generator=g)).half().cuda(), (0.1 * torch.randn(N, generator=g)).half().cuda()
    xp, rp = G.poisoned(x.cuda(), K + 8), G.poisoned(r.cuda(), N + 16)
    wd, bd = w.cuda(), b.cuda()
    ref = R.linear(x, w, b, r)
    h, wimg = 8, L // 8                      # the image behind the token rows
    first, ran = None, 0
    for knob in GEMM_STAGES:
        gemm_stages(knob)
        rows = lib.dsc_linear_gn_rows(M, N, K, L, groups)
        out, part = G.fenced(M, N, N + 8), G.fenced(B * max(rows, 1), groups * 4, dtype=torch.float32)
        rc = lib.dsc_linear_gn_f16(ops._p(xp[1]), ops._p(wd), ops._p(bd), ops._p(rp[1]), ops._p(out[1]), M, N, K, K + 8, N + 16,
                                   N + 8, L, ops._p(part[1]), groups, 0, ops._stream_ptr(wd))
        if rows == 0:
            torch.cuda.synchronize()
            assert rc == DSC_ERR_UNSUPPORTED and G.all_sentinel(out[0]) and G.all_sentinel(part[0]), knob
            continue
        ran += 1
        assert rc == DSC_OK, knob
        assert not _breached(out, part, xp, rp), knob
        y_c, part_c = ops.linear_gn(x.cuda().reshape(B, L, K), wd, bd, r.cuda().reshape(B, L, N), L, groups)   # same variant
        assert part_c.rows == rows and torch.equal(out[1], y_c.reshape(M, N)), knob
        first = y_c if first is None else first
        assert torch.equal(y_c, first), knob                                                  # every variant: equal bytes
        p5 = part[1].view(B, rows, groups, 2, 2)
        assert _partials_whole(p5, N, groups), knob
        live = R.straddles(N, groups).cuda()
        assert torch.equal(p5[..., 0, :], part_c.buf[..., 0, :]) and torch.equal(p5[:, :, live, 1, :], part_c.buf[:, :, live, 1, :]), knob
        # what the consumer adds up, against the stored tensor in fp64 (ops.groupnorm_apply_nhwc's DSC_GN_CHECK bound)
        sums = p5[..., 0, 0].double().sum(1) + torch.where(live, p5[..., 1, 0].double().sum(1), torch.zeros((), dtype=torch.float64, device="cuda"))
        want = R.group_sums(y_c.reshape(M, N).cpu(), B, groups)[..., 0]
        assert torch.allclose(sums.cpu(), want, rtol=1e-3, atol=1e-2 * (N // groups) * h * wimg ** 0.5), knob
        rows_t = out[1].contiguous()
        y = _apply_from(lib, ops, rows_t, part[1], rows, B, N, L, groups, gamma, beta, 1e-6)
        assert not _breached(y, part), knob
        img = y_c.reshape(B, h, wimg, N).permute(0, 3, 1, 2)
        y_ops = ops.groupnorm_apply_nhwc(img, part_c, groups, gamma, beta, 1e-6, True)
        assert torch.equal(y[1], R.rows_of(y_ops)), knob
        assert R.groupnorm_ok(y_ops, R.groupnorm(img.cpu(), groups, gamma.cpu(), beta.cpu(), 1e-6, True)), knob
    assert ran >= 5 and R.within(first.reshape(M, N), ref, 1.5e-3, 2e-3)


@pytest.mark.parametrize("M,N,K,splits", [(5, 64, 1024, 0), (70, 128, 512, 3), (70, 64, 1024, 2)])
def test_linear_splitk_f16(ops, lib, gemm_stages, M, N, K, splits):
    """dsc_linear_splitk_f16 on a workspace of exactly dsc_linear_splitk_workspace_bytes.  (70, 128, 512, 3): 8 K tiles give 3, 3 and
    2 per split, an uneven last split.  One byte less is DSC_ERR_WORKSPACE with nothing written: that check precedes every launch."""
    x, w, b, r = _gemm_operands(M, N, K, 7)
    xp, rp = G.poisoned(x.cuda(), K + 8), G.poisoned(r.cuda(), N + 16)
    wd, bd = w.cuda(), b.cuda()
    nbytes = lib.dsc_linear_splitk_workspace_bytes(M, N, K, splits)
    assert nbytes > 0 and nbytes % (M * N * 4) == 0 and nbytes // (M * N * 4) == (splits or 2)
    compact = ops.linear_splitk(x.cuda(), wd, bd, r.cuda(), splits=splits)
    assert R.within(compact, R.linear(x, w, b, r), 1.5e-3, 2e-3)
    for knob in GEMM_STAGES:
        gemm_stages(knob)
        out, ws = G.fenced(M, N, N + 8), G.exact_scratch(nbytes, 16)
        args = (ops._p(xp[1]), ops._p(wd), ops._p(bd), ops._p(rp[1]), ops._p(out[1]), M, N, K, K + 8, N + 16, N + 8, splits, ops._p(ws[1]))
        rc = lib.dsc_linear_splitk_f16(*args, nbytes - 1, 0, ops._stream_ptr(wd))
        torch.cuda.synchronize()
        assert rc == DSC_ERR_WORKSPACE and G.all_sentinel(out[0]) and G.all_sentinel(ws[0]), knob
        rc = lib.dsc_linear_splitk_f16(*args, nbytes, 0, ops._stream_ptr(wd))
        assert rc == DSC_OK, knob
        assert not _breached(out, ws, xp, rp), knob
        assert torch.equal(out[1], compact) and not torch.isnan(ws[1]).any(), knob          # (every scratch element is written)


# ============================================================================= 3x3 convolution (conv3x3.hip)
def _conv_operands(B, Cin, Cout, h, w, seed):
    """test_conv3x3_kernel's distributions: x [B, Cin, h, w], weight [Cout, Cin, 3, 3], bias on the CPU"""
    g = _gen(B, Cin, Cout, h, w, seed)
    x = torch.randn(B, Cin, h, w, generator=g).half()
    wt = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half()
    b = (torch.randn(Cout, generator=g) * 0.2).half()
    return g, x, wt, b


_CONV_KW = {R.PLAIN: lambda size: {}, R.UPSAMPLE2X: lambda size: {"upsample": True}, R.UPSAMPLE_CEIL: lambda size: {"upsample_size": size},
            R.STRIDE2: lambda size: {"stride2_ceil": True}, R.STRIDE2_PAD_BR: lambda size: {"stride2_pad_br": True}}


def _conv_case(ops, lib, B, h, w, Cin, Cout, mode, residuals=(False, True), splits=0, nchw=False, ldo_pad=8, ldr_pad=16, rings=((),)):
    """dsc_conv3x3_nhwc_f16 on a source image of h x w in the given mode: x at ldx = Cin + 8 (poisoned), the residual at ldr =
    Cout + 16 (poisoned), out at ldo = Cout + 8 in a fence (channel-major: dense [B, Cout, oh ow] in a fence), a split's workspace
    exact.  (a) - (d) of the module docstring.  rings: dsc_debug_set_conv_ring call sequences, one fenced launch under each."""
    g, x, wt, b = _conv_operands(B, Cin, Cout, h, w, mode)
    (H, W), (oh, ow) = R.conv_geometry(mode, h, w)
    r = torch.randn(B, Cout, oh, ow, generator=g).half()
    xd, wtd, bd, rd = x.cuda().contiguous(memory_format=CL), wt.cuda().contiguous(memory_format=CL), b.cuda(), r.cuda().contiguous(memory_format=CL)
    xp, rp = G.poisoned(R.rows_of(xd), Cin + 8), G.poisoned(R.rows_of(rd), Cout + ldr_pad)
    w_rows = wtd.permute(0, 2, 3, 1).contiguous()                   # [Cout, 3, 3, Cin]: the bytes of the channels_last weight
    nbytes = lib.dsc_conv3x3_workspace_bytes(B, H, W, Cin, Cout, splits)
    assert (nbytes > 0) == (splits > 1)
    for with_res in residuals:
        for setting in (401, 0) if rings != ((),) else ():           # the compact run under the launch rule's own choice
            lib.dsc_debug_set_conv_ring(setting)
        compact = ops.conv3x3(xd, wtd, bd, residual=rd if with_res else None, splits=splits, out_nchw=nchw, **_CONV_KW[mode]((H, W)))
        ref = R.conv3x3(x, wt, b, r if with_res else None, mode, (H, W))
        assert compact.shape == ref.shape and R.within(compact, ref, 1.5e-3, 2e-3), (mode, with_res)
        want = compact.reshape(B * Cout, oh * ow) if nchw else R.rows_of(compact)
        for ring in rings:
            for setting in ring:
                lib.dsc_debug_set_conv_ring(setting)
            out = G.fenced(B * Cout, oh * ow) if nchw else G.fenced(B * oh * ow, Cout, Cout + ldo_pad)
            ws = G.exact_scratch(nbytes, 16) if nbytes else None
            rc = lib.dsc_conv3x3_nhwc_f16(ops._p(xp[1]), ops._p(w_rows), ops._p(bd), ops._p(rp[1]) if with_res else None, ops._p(out[1]),
                                          B, H, W, Cin, Cout, Cin + 8, Cout + ldr_pad if with_res else 0, Cout + ldo_pad, mode,
                                          1 if nchw else 0, splits, 0, ops._p(ws[1]) if ws else None, nbytes, ops._stream_ptr(xd))
            assert rc == DSC_OK, (mode, with_res, ring)
            assert not _breached(out, xp, rp, *([ws] if ws else [])), (mode, with_res, ring)
            assert torch.equal(out[1], want) and not torch.isnan(out[1]).any(), (mode, with_res, ring)


# source images: one pixel | 8-wide tiles ragged on both sides | several tiles per row, ragged | 8-wide tiles that hold two images'
# sub-blocks, B odd | ragged rows, wide | 16-wide tiles ragged on both sides (tile_width: every W above takes the 8-wide kernel in
# the plain and stride-2 modes; W = 30: two 16-wide tiles per row, the second ragged)
CONV_IMAGES = [(1, 1, 1), (2, 5, 7), (1, 9, 17), (3, 8, 8), (2, 3, 20), (2, 9, 30)]


@pytest.mark.parametrize("mode", [R.PLAIN, R.UPSAMPLE2X, R.UPSAMPLE_CEIL, R.STRIDE2, R.STRIDE2_PAD_BR])
@pytest.mark.parametrize("B,h,w", CONV_IMAGES)
def test_conv3x3_modes(ops, lib, B, h, w, mode):
    """every resample mode with and without a residual, Cin = Cout = 64 (one slice, one channel tile): UPSAMPLE2X to the even
    targets 2s, UPSAMPLE_CEIL to 2s - 1, STRIDE2 storing ceil(H / 2) x ceil(W / 2) of odd sides, STRIDE2_PAD_BR on the sides rounded
    up to even ones"""
    if mode == R.STRIDE2_PAD_BR:
        h, w = h + h % 2, w + w % 2
    _conv_case(ops, lib, B, h, w, 64, 64, mode)


@pytest.mark.parametrize("Cout", [40, 72, 100])
@pytest.mark.parametrize("B,h,w", [(2, 5, 7), (2, 9, 30)])
def test_conv3x3_ragged_channel_tiles(ops, lib, B, h, w, Cout):
    """a last channel tile of 40, 8 and 36 live channels, channels-last.  Cout = 100 is no multiple of 8: check_operands then takes
    any stride >= Cout (the rows are 8-byte aligned at best), the 16-byte chunks below channel 96 go the vector way and the last
    four channels - bias and residual included - the element-wise one (`p.res[gp * p.ldr + c]`)"""
    _conv_case(ops, lib, B, h, w, 64, Cout, R.PLAIN)


@pytest.mark.parametrize("B,h,w", [(2, 5, 7), (2, 9, 30)])
def test_conv3x3_ring_forms(ops, lib, B, h, w):
    """the kernel forms the launch rule picks for other grids, forced (dsc_debug_set_conv_ring; the small grids here take the
    nine-stage ring by themselves, with loader waves for 16-wide tiles): three-stage ring, nine stages without and with loader waves
    for both tile widths - the loader waves leave before the epilogue.  Equal bytes, fenced, at ragged tiles and a ragged Cout."""
    try:
        _conv_case(ops, lib, B, h, w, 64, 72, R.PLAIN, rings=((3,), (9, 400), (9, 402)))
    finally:
        lib.dsc_debug_set_conv_ring(401)
        lib.dsc_debug_set_conv_ring(0)


@pytest.mark.parametrize("Cout", [4, 72])
@pytest.mark.parametrize("B,h,w", [(2, 5, 7), (1, 9, 17)])
def test_conv3x3_out_nchw(ops, lib, B, h, w, Cout):
    """channel-major output [B, Cout, H, W]: no stride applies; the pixels behind H W of the last channel stay untouched"""
    _conv_case(ops, lib, B, h, w, 64, Cout, R.PLAIN, residuals=(False,), nchw=True)


@pytest.mark.parametrize("mode", [R.PLAIN, R.STRIDE2])
@pytest.mark.parametrize("B,h,w", [(2, 5, 7), (2, 9, 30)])
def test_conv3x3_split_scratch(ops, lib, B, h, w, mode):
    """splits = 2 over Cin = 128 on exactly dsc_conv3x3_workspace_bytes of NaN-filled scratch: conv3x3_reduce reads only what the
    split pass wrote (no NaN comes out).  Stride 2: the query sizes the scratch by H x W, the launch needs oh x ow - it stays inside."""
    _conv_case(ops, lib, B, h, w, 128, 64, mode, splits=2)


@pytest.mark.parametrize("B,H,W,Cin,Cout,groups,ceil", [(2, 9, 17, 64, 64, 8, False), (3, 16, 16, 64, 128, 32, False),
                                                        (2, 9, 30, 64, 64, 8, False), (2, 9, 16, 64, 64, 8, True)])
def test_conv3x3_gn_nhwc_f16(ops, lib, B, H, W, Cin, Cout, groups, ceil):
    """dsc_conv3x3_gn_nhwc_f16: gn_part [B][rows][G][2][2] in a fence with rows from dsc_conv3x3_gn_rows, the per-image row `add` at
    add_ld = Cout + 8 (poisoned), strided x / residual / out.  9 x 17 takes the 8-wide tiles, which emit no statistics: the entry
    refuses it before any launch; 9 x 30 is its ragged 16-wide neighbour; `ceil`: H x W is the DSC_CONV_UPSAMPLE_CEIL target of a
    ((H + 1) / 2) x ((W + 1) / 2) source."""
    mode = R.UPSAMPLE_CEIL if ceil else R.PLAIN
    h, w = ((H + 1) // 2, (W + 1) // 2) if ceil else (H, W)
    g, x, wt, b = _conv_operands(B, Cin, Cout, h, w, 9)
    add, r = (torch.randn(B, Cout, generator=g) * 0.5).half(), torch.randn(B, Cout, H, W, generator=g).half()
    gamma, beta = (1 + 0.1 * torch.randn(Cout, generator=g)).half().cuda(), (0.1 * torch.randn(Cout, generator=g)).half().cuda()
    xd, wtd, bd, rd = x.cuda().contiguous(memory_format=CL), wt.cuda().contiguous(memory_format=CL), b.cuda(), r.cuda().contiguous(memory_format=CL)
    xp, rp, addp = G.poisoned(R.rows_of(xd), Cin + 8), G.poisoned(R.rows_of(rd), Cout + 16), G.poisoned(add.cuda(), Cout + 8, tail_rows=8)
    w_rows = wtd.permute(0, 2, 3, 1).contiguous()
    rows = lib.dsc_conv3x3_gn_rows(B, H, W, Cin, Cout, groups, mode)
    out, part = G.fenced(B * H * W, Cout, Cout + 8), G.fenced(B * max(rows, 1), groups * 4, dtype=torch.float32)
    rc = lib.dsc_conv3x3_gn_nhwc_f16(ops._p(xp[1]), ops._p(w_rows), ops._p(bd), ops._p(addp[1]), Cout + 8, ops._p(rp[1]), ops._p(out[1]),
                                     B, H, W, Cin, Cout, Cin + 8, Cout + 16, Cout + 8, mode, ops._p(part[1]), groups, 0, ops._stream_ptr(xd))
    assert (rows == 0) == ((H, W) == (9, 17))
    if rows == 0:
        torch.cuda.synchronize()
        assert rc == DSC_ERR_UNSUPPORTED and G.all_sentinel(out[0]) and G.all_sentinel(part[0])
        return
    assert rows == ((H + 7) // 8) * ((W + 15) // 16) and rc == DSC_OK
    assert not _breached(out, part, xp, rp, addp)
    y_c = ops.conv3x3_gn(xd, wtd, groups, bias=bd, add=add.cuda(), residual=rd, upsample_size=(H, W) if ceil else None)
    part_c = ops.gn_partials_of(y_c)
    assert R.within(y_c, R.conv3x3(x, wt, b, r, mode, (H, W), add=add), 1.5e-3, 2e-3)
    assert part_c.rows == rows and torch.equal(out[1], R.rows_of(y_c))
    p5, live = part[1].view(B, rows, groups, 2, 2), R.straddles(Cout, groups).cuda()
    assert _partials_whole(p5, Cout, groups)
    assert torch.equal(p5[..., 0, :], part_c.buf[..., 0, :]) and torch.equal(p5[:, :, live, 1, :], part_c.buf[:, :, live, 1, :])
    y = _apply_from(lib, ops, out[1].contiguous(), part[1], rows, B, Cout, H * W, groups, gamma, beta, 1e-5)
    assert not _breached(y, part)
    y_ops = ops.groupnorm_apply_nhwc(y_c, part_c, groups, gamma, beta, 1e-5, True)
    assert torch.equal(y[1], R.rows_of(y_ops))
    assert R.groupnorm_ok(y_ops, R.groupnorm(y_c.cpu(), groups, gamma.cpu(), beta.cpu(), 1e-5, True))


@pytest.mark.parametrize("splits", [0, 2])
@pytest.mark.parametrize("B,h,w", [(1, 3, 5), (2, 4, 4), (1, 3, 16)])
def test_conv3x3_up2x_nhwc_f16(ops, lib, B, h, w, splits):
    """the phase form: weights packed by dsc_conv3x3_up2x_pack_f16 into a fenced [4, Cout, 4, Cin], source at ldx = Cin + 8, out
    [B, 2h, 2w, Cout] at ldo = Cout + 8, a split's scratch exact.  (1, 3, 16): the 16-wide kernel, ragged rows."""
    Cin, Cout = (128, 64) if splits else (64, 64)
    _, x, wt, b = _conv_operands(B, Cin, Cout, h, w, 11)
    xd, wtd, bd = x.cuda().contiguous(memory_format=CL), wt.cuda().contiguous(memory_format=CL), b.cuda()
    w_rows = wtd.permute(0, 2, 3, 1).contiguous()
    packed = G.fenced(16 * Cout, Cin)
    assert lib.dsc_conv3x3_up2x_pack_f16(ops._p(w_rows), ops._p(packed[1]), Cin, Cout, ops._stream_ptr(xd)) == DSC_OK
    assert not _breached(packed)
    packed_c = ops.conv3x3_up2x_pack(wtd)
    assert torch.equal(packed[1].view(4, Cout, 4, Cin), packed_c) and torch.equal(packed_c.cpu(), R.up2x_pack(wt))
    compact = ops.conv3x3_up2x(xd, packed_c, bd, splits=splits)
    assert R.within(compact, R.conv3x3(x, wt, b, mode=R.UPSAMPLE2X), 1.5e-3, 2e-3)
    nbytes = lib.dsc_conv3x3_up2x_workspace_bytes(B, h, w, Cin, Cout, splits)
    assert (nbytes > 0) == (splits > 1)
    xp, out = G.poisoned(R.rows_of(xd), Cin + 8), G.fenced(B * 4 * h * w, Cout, Cout + 8)
    ws = G.exact_scratch(nbytes, 16) if nbytes else None
    rc = lib.dsc_conv3x3_up2x_nhwc_f16(ops._p(xp[1]), ops._p(packed[1]), ops._p(bd), ops._p(out[1]), B, h, w, Cin, Cout, splits,
                                       ops._p(ws[1]) if ws else None, nbytes, Cin + 8, Cout + 8, 0, ops._stream_ptr(xd))
    assert rc == DSC_OK
    assert not _breached(out, xp, packed, *([ws] if ws else []))
    assert torch.equal(out[1], R.rows_of(compact)) and not torch.isnan(out[1]).any()


# ============================================================================= normalisation and element-wise kernels
def _scratch_whole(ws):
    """an fp64-filled scratch after the launch: every 8-byte word is still the sentinel, a finite double or two finite floats (the
    partial sums are doubles, the (mean, rstd) pairs behind them floats) - nothing half-written, no NaN of the kernel's own"""
    sentinel = G.bits(ws) == G.sentinel(torch.float64)
    return bool((sentinel | torch.isfinite(ws) | torch.isfinite(ws.view(torch.float32)).view(-1, 2).all(1)).all())


def _gn_operands(B, C, hw, seed):
    """test_groupnorm_silu's distributions: x [B, C, hw] (channel-major), gamma, beta, add [B, C] on the CPU"""
    g = _gen(B, C, hw, seed)
    x = (torch.randn(B, C, hw, generator=g) * 1.7 + 0.6).half()
    gamma, beta = (torch.randn(C, generator=g) * 0.5 + 1).half(), (torch.randn(C, generator=g) * 0.3).half()
    add = (torch.randn(B, C, generator=g) * 0.8).half()
    return x, gamma, beta, add


@pytest.mark.parametrize("B,C,hw,groups", [(1, 40, 15, 8), (2, 64, 64, 8), (3, 32, 8, 8)])
def test_groupnorm_silu_nchw(ops, lib, B, C, hw, groups):
    """dsc_groupnorm_silu: y in a fence, the workspace exact at the 8-byte alignment the entry asks for; hw = 15 takes the scalar path"""
    x, gamma, beta, _ = _gn_operands(B, C, hw, 1)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    compact = ops.groupnorm_silu(xd.view(B, C, hw, 1), groups, gd, bd, 1e-5, True)
    assert R.groupnorm_ok(compact.view(B, C, hw), R.groupnorm(x, groups, gamma, beta, 1e-5, True))
    nbytes = lib.dsc_groupnorm_workspace_bytes(B, C, hw, groups)
    y, ws = G.fenced(B * C, hw), G.exact_scratch(nbytes, 8, torch.float64)
    rc = lib.dsc_groupnorm_silu(ops._p(xd), ops._p(y[1]), ops._p(gd), ops._p(bd), B, C, hw, groups, 1e-5, 1, 0, ops._p(ws[1]), nbytes,
                                ops._stream_ptr(xd))
    assert rc == DSC_OK
    assert not _breached(y, ws) and _scratch_whole(ws[1])
    assert torch.equal(y[1], compact.view(B * C, hw)) and not torch.isnan(y[1]).any()


def _gn_modes():
    """(name, calls) of dsc_debug_set_gn_mode: the shape's own choice, never a single launch, the 1024-thread bundle, the three-launch
    form, statistics workgroups without channel slabs"""
    return (("auto", (11, 0)), ("two launches", (11, 2)), ("wide bundle", (11, 3)), ("three launches", (11, 4)), ("no slabs", (0, 10)))


@pytest.mark.parametrize("B,C,hw,groups", [(1, 8, 1, 1), (3, 64, 15, 8), (2, 96, 576, 8), (2, 320, 1024, 32), (1, 48, 63, 4)])
def test_groupnorm_silu_nhwc(ops, lib, B, C, hw, groups):
    """dsc_groupnorm_silu_nhwc in every launch form (small, bundle, slabs, three launches): y in a fence, `add` strided and poisoned,
    the workspace exactly dsc_groupnorm_nhwc_workspace_bytes - sized by the apply pass's row chunks, indexed by the statistics pass's
    - and NaN-filled: whatever the apply pass reads of it was written, or y would hold a NaN"""
    x, gamma, beta, add = _gn_operands(B, C, hw, 2)
    tok, gd, bd = x.transpose(1, 2).contiguous().cuda(), gamma.cuda(), beta.cuda()            # [B, hw, C]
    addp = G.poisoned(add.cuda(), C + 8, tail_rows=8)
    ref = R.groupnorm(x, groups, gamma, beta, 1e-5, True, add).transpose(1, 2)
    nbytes = lib.dsc_groupnorm_nhwc_workspace_bytes(B, C, hw, groups)
    assert nbytes >= B * groups * 2 * 12
    try:
        for name, calls in _gn_modes():
            for mode in calls:
                lib.dsc_debug_set_gn_mode(mode)
            compact = ops.groupnorm_silu_nhwc(tok, groups, gd, bd, 1e-5, True, add=add.cuda())
            assert R.groupnorm_ok(compact, ref), name
            y, ws = G.fenced(B * hw, C), G.exact_scratch(nbytes, 8, torch.float64)
            rc = lib.dsc_groupnorm_silu_nhwc(ops._p(tok), ops._p(y[1]), ops._p(gd), ops._p(bd), ops._p(addp[1]), C + 8, B, C, hw,
                                             groups, 1e-5, 1, 0, ops._p(ws[1]), nbytes, ops._stream_ptr(tok))
            assert rc == DSC_OK, name
            assert not _breached(y, ws, addp) and _scratch_whole(ws[1]), name
            assert torch.equal(y[1], compact.reshape(B * hw, C)) and not torch.isnan(y[1]).any(), name
    finally:
        lib.dsc_debug_set_gn_mode(11)
        lib.dsc_debug_set_gn_mode(0)


@pytest.mark.parametrize("B,C1,C2,hw,groups", [(3, 40, 24, 35, 8), (1, 8, 56, 9, 4)])
def test_groupnorm_silu_nhwc_cat(ops, lib, B, C1, C2, hw, groups):
    """dsc_groupnorm_silu_nhwc_cat: the concatenation and y both in fences, cat the bytes of torch.cat; the single-launch form and
    the statistics pass (modes 2 and 4) write the concatenation from different kernels"""
    C = C1 + C2
    x, gamma, beta, add = _gn_operands(B, C, hw, 3)
    tok, gd, bd = x.transpose(1, 2).contiguous().cuda(), gamma.cuda(), beta.cuda()
    x1, x2 = tok[..., :C1].contiguous(), tok[..., C1:].contiguous()
    img = lambda t: t.reshape(B, hw, 1, t.shape[-1]).permute(0, 3, 1, 2)                     # channels_last [B, c, hw, 1]
    addp = G.poisoned(add.cuda(), C + 8, tail_rows=8)
    ref = R.groupnorm(x, groups, gamma, beta, 1e-5, True, add).transpose(1, 2)
    nbytes = lib.dsc_groupnorm_nhwc_workspace_bytes(B, C, hw, groups)
    try:
        for mode in (0, 2, 4):
            lib.dsc_debug_set_gn_mode(mode)
            y_c, cat_c = ops.groupnorm_silu_nhwc_cat(img(x1), img(x2), groups, gd, bd, 1e-5, True, add=add.cuda())
            assert torch.equal(R.rows_of(cat_c), tok.reshape(B * hw, C)) and R.groupnorm_ok(R.rows_of(y_c).view(B, hw, C), ref), mode
            cat, y, ws = G.fenced(B * hw, C), G.fenced(B * hw, C), G.exact_scratch(nbytes, 8, torch.float64)
            rc = lib.dsc_groupnorm_silu_nhwc_cat(ops._p(x1), ops._p(x2), C1, ops._p(cat[1]), ops._p(y[1]), ops._p(gd), ops._p(bd),
                                                 ops._p(addp[1]), C + 8, B, C, hw, groups, 1e-5, 1, 0, ops._p(ws[1]), nbytes,
                                                 ops._stream_ptr(tok))
            assert rc == DSC_OK, mode
            assert not _breached(cat, y, ws, addp) and _scratch_whole(ws[1]), mode
            assert torch.equal(cat[1], tok.reshape(B * hw, C)), mode
            assert torch.equal(y[1], R.rows_of(y_c)) and not torch.isnan(y[1]).any(), mode
    finally:
        lib.dsc_debug_set_gn_mode(0)


@pytest.mark.parametrize("with_a", [True, False])
@pytest.mark.parametrize("C", [8, 320, 4096])
@pytest.mark.parametrize("rows", [1, 5, 9])
def test_add_layernorm(ops, lib, rows, C, with_a):
    """dsc_add_layernorm: one wave per row, four rows per workgroup - the last workgroup's idle waves store nothing; sum_out and y fenced"""
    g = _gen(rows, C)
    x, a = (torch.randn(rows, C, generator=g) * 2 + 0.3).half(), torch.randn(rows, C, generator=g).half()
    gamma, beta = (torch.randn(C, generator=g) * 0.3 + 1).half(), (torch.randn(C, generator=g) * 0.2).half()
    xd, ad, gd, bd = x.cuda(), a.cuda() if with_a else None, gamma.cuda(), beta.cuda()
    s_c, y_c = ops.add_layernorm(xd, ad, gd, bd)
    s_ref, y_ref = R.add_layernorm(x, a if with_a else None, gamma, beta)
    assert torch.equal(s_c.cpu(), s_ref) and R.within(y_c, y_ref, 1.5e-3, 2e-3)
    s, y = G.fenced(rows, C), G.fenced(rows, C)
    rc = lib.dsc_add_layernorm(ops._p(xd), ops._p(ad), ops._p(gd), ops._p(bd), ops._p(s[1]) if with_a else None, ops._p(y[1]), rows, C,
                               1e-5, 0, ops._stream_ptr(xd))
    assert rc == DSC_OK
    assert not _breached(s, y)
    assert torch.equal(y[1], y_c) and (torch.equal(s[1], s_c) if with_a else G.all_sentinel(s[0]))


@pytest.mark.parametrize("rows,n", [(1, 8), (3, 1000), (5, 2560)])
def test_geglu(ops, lib, rows, n):
    g = _gen(rows, n)
    x = (torch.randn(rows, 2 * n, generator=g) * 2).half()
    compact = ops.geglu(x.cuda())
    ref = R.geglu(x)
    assert R.within(compact, ref, 2.5e-3, 1e-3) and (compact.float().cpu() - ref).abs().mean().item() < 3e-4      # test_geglu
    y = G.fenced(rows, n)
    assert lib.dsc_geglu(ops._p(x.cuda()), ops._p(y[1]), rows, n, 0, ops._stream_ptr(compact)) == DSC_OK
    assert not _breached(y) and torch.equal(y[1], compact)


@pytest.mark.parametrize("rows,C", [(1, 8), (7, 320)])
def test_add_bias_residual(ops, lib, rows, C):
    """dsc_add_bias_residual: fp16(a + b + bias) from an fp32 sum - one fp16 rounding, the GEMM epilogue's bound"""
    g = _gen(rows, C)
    a, b = torch.randn(rows, C, generator=g).half(), torch.randn(rows, C, generator=g).half()
    bias = (torch.randn(C, generator=g) * 0.2).half()
    ad, bd, biasd = a.cuda(), b.cuda(), bias.cuda()
    compact = ops.add_bias_residual(ad, bd, biasd)
    assert R.within(compact, a.float() + b.float() + bias.float(), 1.5e-3, 2e-3)
    out = G.fenced(rows, C)
    assert lib.dsc_add_bias_residual(ops._p(ad), ops._p(bd), ops._p(biasd), ops._p(out[1]), rows, C, 0, ops._stream_ptr(ad)) == DSC_OK
    assert not _breached(out) and torch.equal(out[1], compact)


@pytest.mark.parametrize("N", [8, 320, 1288])
@pytest.mark.parametrize("M", [1, 5, 8])
def test_linear_rows_f16(ops, lib, M, N):
    """dsc_linear_rows_f16 (K = 320): out at ldo = N + 8, x at ldx = K + 8 (poisoned); with DSC_ROWS_SINUSOID_IN the input is fp32
    t[M] with NaN right behind its last element.  N = 1288 = 4 * 322: whole workgroups; 8 and 320 too - the tail is `n >= N`."""
    K = 320
    g = _gen(M, N)
    x = torch.randn(M, K, generator=g).half()
    t = (torch.rand(M, generator=g) * 999.0).float()
    w, b = (torch.randn(N, K, generator=g) / K ** 0.5).half(), (torch.randn(N, generator=g) * 0.1).half()
    wd, bd = w.cuda(), b.cuda()
    xp, tp = G.poisoned(x.cuda(), K + 8, tail_rows=8), G.poisoned(t.cuda().view(1, M), tail_rows=8)
    for sinus in (False, True):
        compact = (ops.linear_rows(t.cuda(), wd, bd, silu_out=True, sinusoid_dim=K) if sinus else ops.linear_rows(x.cuda(), wd, None))
        ref = R.linear_rows(R.sinusoid(t, K), w, b, True) if sinus else R.linear_rows(x, w)
        assert R.within(compact, ref, 2e-3, 2e-3), sinus                         # test_linear_rows_time_embedding
        out = G.fenced(M, N, N + 8, tail_rows=8)
        rc = lib.dsc_linear_rows_f16(ops._p(tp[1] if sinus else xp[1]), ops._p(wd), ops._p(bd) if sinus else None, ops._p(out[1]), M, N,
                                     K, 0 if sinus else K + 8, N + 8, 3 if sinus else 0, 0, ops._stream_ptr(wd))
        assert rc == DSC_OK, sinus
        assert not _breached(out, xp, tp), sinus
        assert torch.equal(out[1], compact), sinus


@pytest.mark.parametrize("rows,n", [(1, 8), (7, 1000), (3, 16384)])
def test_softmax_rows_f16(ops, lib, rows, n):
    """dsc_softmax_rows_f16 with ld_scores = n + 8 (poisoned) and ld_probs = n + 16"""
    g = _gen(rows, n)
    s = (torch.randn(rows, n, generator=g) * 6).half()
    compact = ops.softmax_rows(s.cuda(), scale=0.37)
    ref = torch.softmax(s.float() * 0.37, dim=-1)
    assert (compact.float().cpu() - ref).abs().max().item() < 1e-3 * ref.max().item() + 1e-6      # test_softmax_rows
    assert (compact.float().sum(-1).cpu() - 1).abs().max().item() < 2e-3
    sp, out = G.poisoned(s.cuda(), n + 8, tail_rows=8), G.fenced(rows, n, n + 16, tail_rows=8)
    rc = lib.dsc_softmax_rows_f16(ops._p(sp[1]), ops._p(out[1]), rows, n, n + 8, n + 16, 0.37, 0, ops._stream_ptr(compact))
    assert rc == DSC_OK
    assert not _breached(out, sp) and torch.equal(out[1], compact)


@pytest.mark.parametrize("kind", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("n", [8, 1000, 63488 + 8])
def test_act_f16(ops, lib, n, kind):
    """dsc_act_f16 in place over the first n elements of a fenced buffer; n = 63496: 7937 vectors, the last workgroup a single thread"""
    g = _gen(n)
    x = (torch.randn(n, generator=g) * 3).half()
    compact = ops.act_(x.cuda().clone(), kind)
    assert int((R.ordinal(compact.cpu()) - R.ordinal(R.act_exact(kind, x))).abs().max()) <= 1      # test_act_over_every_finite_fp16_value
    io = G.poisoned(x.cuda().view(1, n), tail_rows=2)
    assert lib.dsc_act_f16(ops._p(io[1]), n, ops.ACT_KINDS[kind], 0, ops._stream_ptr(compact)) == DSC_OK
    assert not _breached(io) and torch.equal(io[1].view(n), compact)


def test_region_xattn_workspace(ops, lib):
    """dsc_region_xattn_fwd on exactly dsc_region_xattn_workspace_bytes of NaN-filled scratch at the 8-byte alignment it asks for
    (the destinations: tests/test_output_paths.py)"""
    Bc, H, L, S, d, sigma = 2, 2, 100, 77, 40, 2.0
    xin = attn_inputs("guard", Bc=Bc, H=H, L=L, S=S, d=d)
    q, k, v, w = (torch.from_numpy(xin[n]) for n in ("q", "k", "v", "w"))
    qd, kd, vd, wd = q.cuda().half(), k.cuda().half(), v.cuda().half(), w.cuda()
    compact = ops.region_xattn(qd, kd, vd, wd, sigma)
    err = (compact.float().cpu() - ra.region_attention(q, k, v, w, sigma, fp16_rounding=True)).abs()
    assert err.max().item() < tol16(q, k, w, sigma) and err.mean().item() < 3e-4                    # test_region_xattn_gpu.py
    nbytes = lib.dsc_region_xattn_workspace_bytes(Bc, H, L, S, d, 1)
    assert nbytes > 0
    out, ws = G.fenced(Bc * H * L, d), G.exact_scratch(nbytes, 8, torch.float64)
    qs, ks = ops._i64x3(H * L * d, d, L * d), ops._i64x3(H * S * d, d, S * d)                      # [B, H, L, d]: (sb, sl, sh)
    rc = lib.dsc_region_xattn_fwd(ops._p(qd), ops._p(kd), ops._p(vd), ops._p(out[1]), ops._p(wd), Bc, H, L, S, d, w.shape[0], 1,
                                  qs, ks, ks, qs, sigma, None, 0.0, 0, ops.FLAG_REF_FP16_ROUNDING,
                                  ops._p(ws[1]), nbytes, ops._stream_ptr(qd))
    assert rc == DSC_OK
    assert not _breached(out, ws) and _scratch_whole(ws[1])
    assert torch.equal(out[1].view(Bc, H, L, d), compact) and not torch.isnan(out[1]).any()
