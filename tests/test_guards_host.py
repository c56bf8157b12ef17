"""tests/guards.py on CPU tensors: the evidence that the detector detects (no kernel is edited to prove it), and the CPU
references of the guard-band tests against each other in fp64.  No GPU, no GPU library."""
import pytest
import torch
import torch.nn.functional as F

import guard_band_refs as R
import guards as G

DTYPES = [torch.float16, torch.float32, torch.float64]


def _plant(buf, index):
    """flip one element of buf's bits (a stray one-element store)"""
    G.bits(buf)[index] = 0


@pytest.mark.parametrize("dtype", DTYPES + [torch.uint8])
def test_sentinels_are_nan_payloads_no_kernel_stores(dtype):
    buf = G.filled(16, dtype, "cpu")
    assert G.all_sentinel(buf)
    if dtype != torch.uint8:
        assert torch.isnan(buf).all()
        canonical = torch.tensor([float("nan")], dtype=dtype)
        assert int(G.bits(canonical)[0]) != G.sentinel(dtype) and int(G.bits(-canonical)[0]) != G.sentinel(dtype)
    else:
        assert int(buf[0]) == 0xA5
    # the fp64 sentinel is a NaN in either width: scratch that holds doubles and floats stays poisoned for both
    assert torch.isnan(G.filled(4, torch.float64, "cpu").view(torch.float32)).all()
    assert G.sentinel(torch.float16) == 0x7E5A and G.sentinel(torch.float32) == 0x7FC5A5A5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,row_len,ld,lead,tail_rows", [(5, 8, 16, 8, 2), (3, 24, 32, 64, 128), (1, 8, 8, 0, 1), (7, 13, 16, 16, 4)])
def test_untouched_flags_one_planted_element_anywhere_outside(dtype, rows, row_len, ld, lead, tail_rows):
    buf, view = G.fenced(rows, row_len, ld, dtype, lead, tail_rows, "cpu")
    assert view.shape == (rows, row_len) and view.stride() == (ld, 1) and view.storage_offset() == lead
    assert view.data_ptr() % 16 == 0
    assert buf.numel() >= lead + rows * ld + tail_rows * ld
    assert G.untouched(buf, view) and G.all_sentinel(buf)
    # arbitrary writes inside the view are accepted - sentinel bits included
    view.copy_(torch.randn(rows, row_len).to(dtype))
    view[0, 0] = float("inf")
    G.bits(view)[-1, -1] = 12345
    assert G.untouched(buf, view) and not G.all_sentinel(buf)
    behind = lead + (rows - 1) * ld + row_len                   # right behind the last row's last element
    spots = {"behind the last row": behind, "the far end": buf.numel() - 1, "one row past the end": lead + rows * ld}
    if lead:
        spots["the lead, first"] = 0
        spots["the lead, last"] = lead - 1
    if ld > row_len:
        spots["first row's gap"] = lead + row_len
        spots["a middle row's gap"] = lead + (rows // 2) * ld + ld - 1
    for where, index in spots.items():
        saved = int(G.bits(buf)[index])
        assert saved == G.sentinel(dtype), where
        _plant(buf, index)
        assert not G.untouched(buf, view), where
        G.bits(buf)[index] = saved
        assert G.untouched(buf, view), where
    # a NaN that is not the sentinel is a write too: the comparison is of bits, not of values
    buf[behind] = float("nan")
    assert not G.untouched(buf, view)


def test_untouched_with_dense_rows_and_higher_dimensional_views():
    buf, view = G.fenced(6, 8, None, torch.float16, 8, 1, "cpu")            # ld == row_len: no gaps, lead and tail only
    assert view.is_contiguous() and G.untouched(buf, view)
    view.fill_(1.0)
    assert G.untouched(buf, view)
    _plant(buf, 8 + 6 * 8)
    assert not G.untouched(buf, view)
    # [B, H, W, C] pixels with a padded pixel stride, and a [2, B, H] split of the rows: same fence
    buf, view = G.fenced(2 * 3 * 4, 8, 16, torch.float16, 16, 2, "cpu")
    v4 = view.unflatten(0, (2, 3, 4))
    assert v4.shape == (2, 3, 4, 8) and v4.stride() == (192, 64, 16, 1)
    v4.fill_(2.0)
    assert G.untouched(buf, v4) and G.untouched(buf, view.unflatten(0, (6, 4)))
    _plant(buf, 16 + 5 * 16 + 8)                                             # pixel 5's gap
    assert not G.untouched(buf, v4) and not G.untouched(buf, view)
    # a narrower view of the same buffer: what the wider one wrote now counts as outside
    buf, view = G.fenced(4, 16, 16, torch.float32, 4, 1, "cpu")
    view.fill_(0.0)
    assert G.untouched(buf, view) and not G.untouched(buf, view[:, :8]) and not G.untouched(buf, view[:3])
    with pytest.raises(ValueError):
        G.untouched(buf, torch.zeros(4, 16))                                 # not a view of buf


def test_fenced_refuses_layouts_that_break_alignment_or_overlap():
    for bad in (dict(rows=2, row_len=8, ld=4), dict(rows=0, row_len=8), dict(rows=2, row_len=8, lead=4),
                dict(rows=2, row_len=8, dtype=torch.float32, lead=2)):
        with pytest.raises(ValueError):
            G.fenced(device="cpu", **bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_keeps_the_payload_bits_and_surrounds_it_with_nan(dtype):
    t = torch.randn(5, 24).to(dtype)
    t[1, 3], t[2, 2], t[4, 23] = float("nan"), float("-inf"), -0.0          # payload NaNs and signed zeros survive bit for bit
    buf, view = G.poisoned(t, ld=32, lead=16, tail_rows=3)
    assert torch.equal(G.bits(view), G.bits(t)) and view.stride() == (32, 1)
    assert G.untouched(buf, view)
    outside = torch.ones(buf.numel(), dtype=torch.bool)
    outside.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(False)
    assert torch.isnan(buf[outside]).all() and int(outside.sum()) == buf.numel() - 5 * 24
    assert torch.isnan(buf[:16]).all() and torch.isnan(buf[16 + 24:16 + 32]).all() and torch.isnan(buf[16 + 4 * 32 + 24:]).all()
    # a read past a row's end, or past the last row, reaches a NaN
    wide = buf[16:16 + 5 * 32].view(5, 32)
    assert torch.isnan(wide[:, 24:]).all() and torch.isnan(buf[16 + 5 * 32:16 + 8 * 32]).all()
    with pytest.raises(ValueError):
        G.poisoned(torch.zeros(2, 3, 8, dtype=dtype))


@pytest.mark.parametrize("nbytes,align,fill", [(16, 16, torch.float32), (4096 + 8, 8, torch.float64), (3 * 70 * 128 * 4, 16, torch.float32),
                                               (24, 8, torch.float64), (5, 1, torch.uint8)])
def test_exact_scratch_is_exact_aligned_and_fenced_on_both_sides(nbytes, align, fill):
    buf, ws = G.exact_scratch(nbytes, align, fill, "cpu")
    assert ws.numel() * ws.element_size() == nbytes and ws.dtype == fill
    assert ws.data_ptr() % align == 0 and ws.data_ptr() % (2 * align) != 0   # held to the alignment it asks for, no better
    front = (ws.data_ptr() - buf.data_ptr())
    back = buf.numel() * buf.element_size() - front - nbytes
    assert front >= max(4096, nbytes) and back >= max(4096, nbytes)
    assert G.all_sentinel(buf) and G.untouched(buf, ws)
    if fill != torch.uint8:
        assert torch.isnan(ws).all()
    ws.fill_(0)
    assert G.untouched(buf, ws)
    first, last = ws.storage_offset(), ws.storage_offset() + ws.numel() - 1
    for index in (first - 1, last + 1, 0, buf.numel() - 1):
        saved = int(G.bits(buf)[index])
        _plant(buf, index)
        assert not G.untouched(buf, ws), index
        G.bits(buf)[index] = saved
    assert G.untouched(buf, ws)
    with pytest.raises(ValueError):
        G.exact_scratch(nbytes + 1 if fill != torch.uint8 else 0, align, fill, "cpu")


# ----------------------------------------------------------------------------- the CPU references, against fp64 / each other
def test_conv_reference_modes_agree_with_their_definitions():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 8, 5, 7, generator=g).half()
    w = (torch.randn(6, 8, 3, 3, generator=g) / 8).half()
    b = torch.randn(6, generator=g).half()
    full = R.conv3x3(x, w, b)
    assert torch.allclose(R.conv3x3(x, w, b, mode=R.STRIDE2), full[:, :, ::2, ::2], atol=1e-6)        # stride 2 / pad 1: the even pixels
    xe = x[:, :, :4, :6]
    assert torch.allclose(R.conv3x3(xe, w, b, mode=R.STRIDE2_PAD_BR), R.conv3x3(xe, w, b)[:, :, 1::2, 1::2], atol=1e-6)   # the odd ones
    up = R.conv3x3(x, w, b, mode=R.UPSAMPLE2X)
    ceil = R.conv3x3(x, w, b, mode=R.UPSAMPLE_CEIL, size=(9, 13))
    assert up.shape == (2, 6, 10, 14) and ceil.shape == (2, 6, 9, 13)
    # the 2s - 1 target reads source pixel dst >> 1, like the exact doubling: interior pixels agree, the last row / column do not
    assert torch.allclose(ceil[:, :, :8, :12], up[:, :, :8, :12], atol=1e-6) and not torch.allclose(ceil[:, :, 8, :12], up[:, :, 8, :12])
    for mode, (h, wd) in ((R.PLAIN, (5, 7)), (R.UPSAMPLE2X, (5, 7)), (R.UPSAMPLE_CEIL, (5, 7)), (R.STRIDE2, (5, 7)), (R.STRIDE2_PAD_BR, (4, 6))):
        (H, W), (oh, ow) = R.conv_geometry(mode, h, wd)
        out = R.conv3x3(x[:, :, :h, :wd], w, None, mode=mode, size=(H, W))
        assert out.shape[2:] == (oh, ow), mode
    add, res = torch.randn(2, 6, generator=g).half(), torch.randn(2, 6, 5, 7, generator=g).half()
    assert torch.allclose(R.conv3x3(x, w, b, residual=res, add=add), full + add.float()[:, :, None, None] + res.float(), atol=1e-6)
    assert torch.equal(R.rows_of(res).reshape(2, 5, 7, 6).permute(0, 3, 1, 2), res)


def test_phase_weights_reference_reproduces_the_upsampled_convolution():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 8, 3, 5, generator=g).half()
    w = (torch.randn(4, 8, 3, 3, generator=g) / 8).half()
    packed = R.up2x_pack(w)
    assert packed.shape == (4, 4, 4, 8)
    ref = R.conv3x3(x, w, mode=R.UPSAMPLE2X)
    xp = F.pad(x.float(), (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            k = packed[2 * py + px].float().view(4, 2, 2, 8).permute(0, 3, 1, 2)
            got = F.conv2d(xp[:, :, py:py + 4, px:px + 6], k)
            assert R.within(got, ref[:, :, py::2, px::2], 1.5e-3, 2e-3)


def test_gemm_family_references():
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(6, 64, generator=g).half(), (torch.randn(128, 64, generator=g) / 8).half(), torch.randn(128, generator=g).half()
    r = torch.randn(3, 128, generator=g).half()
    y = R.linear(x, w, b, r)
    y64 = x.double() @ w.double().t() + b.double() + torch.cat([r, r]).double()
    assert torch.allclose(y.double(), y64, atol=1e-4)
    assert R.within(y.half(), y64.float(), 1.5e-3, 2e-3) and not R.within(y.half() + 1, y64.float(), 1.5e-3, 2e-3)
    gg = R.linear_geglu(x, w, b)
    assert gg.shape == (6, 64) and torch.allclose(gg, R.geglu(R.linear(x, w, b)), atol=1e-6)
    stats, bound = R.row_block_stats(y.half())
    assert stats.shape == (6, 2, 2) and torch.allclose(stats[..., 0].sum(1), y.half().double().sum(1))
    assert torch.all(bound[..., 0] >= stats[..., 0].abs())
    q, kv = R.head_major(torch.arange(4 * 24).reshape(4, 24).float(), 2, 2, 2)         # B = 2, L = 2, C = 8, heads = 2, d = 4
    assert q.shape == (4, 8) and kv.shape == (2, 2, 2, 2, 4)
    assert torch.equal(kv[0, 1, 1, 0], torch.arange(4).float() + (2 * 24 + 8 + 4))      # keys of image 1, head 1, token 0
    assert torch.equal(kv[1, 0, 0, 1], torch.arange(4).float() + (1 * 24 + 16))         # values of image 0, head 0, token 1
    gamma, beta = torch.ones(64).half(), torch.zeros(64).half()
    ln = R.layernorm_linear(x, gamma, beta, w, b)
    assert torch.allclose(ln, F.layer_norm(x.float(), (64,)) @ w.float().t() + b.float(), atol=1e-5)
    assert list(R.straddles(192, 32)[:12]) == [False] * 10 + [True, False]              # 6 channels per group: 60..65 crosses 64


def test_normalisation_and_elementwise_references():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 16, 3, 5, generator=g).half()
    gamma, beta, add = torch.randn(16, generator=g).half(), torch.randn(16, generator=g).half(), torch.randn(2, 16, generator=g).half()
    y = R.groupnorm(x, 4, gamma, beta, 1e-5, True, add)
    xd = (x.double() + add.double()[:, :, None, None]).reshape(2, 4, -1)
    n = ((xd - xd.mean(2, keepdim=True)) / torch.sqrt(xd.var(2, unbiased=False, keepdim=True) + 1e-5)).reshape(2, 16, 3, 5)
    y64 = F.silu(n * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1))
    assert torch.allclose(y.double(), y64, atol=1e-4) and R.groupnorm_ok(y.half(), y64.float()) and not R.groupnorm_ok(y.half() + 0.1, y64.float())
    sums = R.group_sums(R.rows_of(x), 2, 4)
    assert torch.allclose(sums[..., 0], x.double().reshape(2, 4, -1).sum(2)) and sums.shape == (2, 4, 2)
    s, ln = R.add_layernorm(x[0, 0], x[1, 0], torch.ones(5).half(), torch.zeros(5).half())
    assert torch.equal(s, (x[0, 0].float() + x[1, 0].float()).half()) and torch.allclose(ln.mean(-1), torch.zeros(3), atol=1e-6)
    emb = R.sinusoid(torch.tensor([0.0, 7.0]), 16)
    assert emb.shape == (2, 16) and torch.equal(emb[0], torch.cat([torch.ones(8), torch.zeros(8)]).half())
    v = torch.tensor([-3.0, -0.5, 0.0, 0.5, 3.0]).half()
    for kind, fn in (("quick_gelu", lambda t: t * torch.sigmoid(1.702 * t)), ("gelu", F.gelu)):
        assert int((R.ordinal(R.act_exact(kind, v)) - R.ordinal(fn(v.float()).half())).abs().max()) <= 1
    assert int(R.ordinal(torch.tensor([-0.0]).half())[0]) == int(R.ordinal(torch.tensor([0.0]).half())[0])
