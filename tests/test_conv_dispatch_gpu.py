"""ops.conv3x3_try and the call sites that go through it, on the MI355X (`-m gpu`): every resample mode gives the bytes of
ops.conv3x3 with the mode's older keyword, None where no kernel covers the call, and the modules route as they did.

Shapes: the smallest that still have ragged tiles at both tile widths (5 x 7: 8-wide, 11 x 12: 16-wide, both with overhang; the
stride-2 form of the VAE encoder needs even sides: 6 x 8 and 10 x 12) and one split over two 64-channel slices.
Kernel tolerance: that of tests/test_any_size_gpu.py, |out - ref| <= 1.5e-3 |ref| + 2e-3 against an fp32 F.conv2d."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


def _close(out, ref):
    return torch.all((out.float() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3)


def _operands(B, C, Cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, h, w, generator=g).half().cuda().contiguous(memory_format=CL)
    wt = (torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(9 * C)).half().cuda().contiguous(memory_format=CL)
    b = (torch.randn(Cout, generator=g) * 0.2).half().cuda()
    return g, x, wt, b


# mode name -> (old keywords, conv3x3_try keywords, the F.conv2d restatement in fp32), given the source sides
def _modes(h, w):
    size = (2 * h - 1, 2 * w)
    return {
        "plain": ({}, {}, lambda x, wt, b: F.conv2d(x, wt, b, padding=1)),
        "upsample2x": ({"upsample": True}, {"mode": 1}, lambda x, wt, b: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, b, padding=1)),
        "stride2": ({"stride2_ceil": True}, {"mode": 2}, lambda x, wt, b: F.conv2d(x, wt, b, stride=2, padding=1)),
        "stride2_pad_br": ({"stride2_pad_br": True}, {"mode": 3}, lambda x, wt, b: F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2)),
        "upsample_size": ({"upsample_size": size}, {"mode": 4, "size": size}, lambda x, wt, b: F.conv2d(F.interpolate(x, size=size, mode="nearest"), wt, b, padding=1)),
    }


@pytest.mark.parametrize("mode", ["plain", "upsample2x", "stride2", "stride2_pad_br", "upsample_size"])
@pytest.mark.parametrize("B,C,Cout,hw,splits", [(2, 64, 64, (5, 7), 0), (2, 64, 64, (11, 12), 0), (2, 128, 64, (8, 8), 2)])
def test_try_is_conv3x3_in_every_mode(ops, mode, B, C, Cout, hw, splits):
    if mode == "stride2_pad_br":
        hw = {(5, 7): (6, 8), (11, 12): (10, 12)}.get(hw, hw)               # even sides; same tile widths, ragged as well
    g, x, wt, b = _operands(B, C, Cout, *hw, seed=C + hw[0] + hw[1])
    old, new, restate = _modes(*hw)[mode]
    assert new.get("mode", ops.CONV_PLAIN) == getattr(ops, "CONV_" + mode.upper())
    ref = restate(x.float(), wt.float(), b.float())
    out = ops.conv3x3_try(x, wt, b, splits=splits, **new)
    assert out is not None and out.shape == ref.shape and out.is_contiguous(memory_format=CL)
    assert torch.equal(out, ops.conv3x3(x, wt, b, splits=splits, **old))
    assert _close(out, ref), (out.float() - ref).abs().max().item()
    r = torch.randn(ref.shape, generator=g).half().cuda().contiguous(memory_format=CL)
    out_r = ops.conv3x3_try(x, wt, b, r, splits=splits, **new)
    assert torch.equal(out_r, ops.conv3x3(x, wt, b, r, splits=splits, **old))
    assert _close(out_r, ref + r.float())
    if mode == "plain":                 # (with splits=2 too: a channel-major launch runs unsplit, the reduce launch stores pixel-major)
        out_n = ops.conv3x3_try(x, wt, b, out_nchw=True, splits=splits)
        assert out_n.is_contiguous() and torch.equal(out_n, ops.conv3x3(x, wt, b, out_nchw=True, splits=splits))
        assert _close(out_n, ref)


def test_try_returns_none_where_no_kernel_covers(ops, monkeypatch):
    _, x, wt, b = _operands(2, 64, 64, 5, 7, seed=1)
    _, x4, wt4, _ = _operands(2, 4, 64, 5, 7, seed=2)
    assert ops.conv3x3_try(x4, wt4, b) is None                               # 4 input channels
    assert ops.conv3x3_try(x.float(), wt.float(), b.float()) is None         # fp32
    assert ops.conv3x3_try(x[:, :, :, :6], wt, b, mode=ops.CONV_STRIDE2_PAD_BR) is None   # that mode's even-sides rule
    monkeypatch.setattr(ops, "USE_DSC_CONV", False)
    assert ops.conv3x3_try(x, wt, b) is None
    monkeypatch.undo()
    assert ops.conv3x3_try(x, wt, b) is not None


def _module(cls, *args):
    torch.manual_seed(3)
    return cls(*args).half().cuda().eval()


def test_downsample2d_routes_to_the_stride2_kernel(ops):
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import Downsample2D
    m = _module(Downsample2D, 64)
    _, x, _, _ = _operands(1, 64, 64, 11, 12, seed=4)
    with torch.no_grad():
        assert torch.equal(m(x), ops.conv3x3(x, m.conv.weight, m.conv.bias, stride2_ceil=True))


@pytest.mark.parametrize("phases", [True, False])
def test_upsample2d_routing(ops, monkeypatch, phases):
    """the phase form for the exact doubling when it is switched on, else the gather: code 1 without an output_size, code 4 with
    one (also for (2h, 2w)); a size that is no 2s / 2s-1 goes to the library path without raising"""
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import Upsample2D
    monkeypatch.setattr(ops, "USE_UP2X_PHASES", phases)
    m = _module(Upsample2D, 64)
    w, b = m.conv.weight, m.conv.bias
    _, x, _, _ = _operands(1, 64, 64, 6, 5, seed=5)
    doubled = ops.conv3x3_up2x(x, ops.conv3x3_up2x_pack(w), b) if phases else None
    with torch.no_grad():
        assert torch.equal(m(x), doubled if phases else ops.conv3x3(x, w, b, upsample=True))
        assert torch.equal(m(x, (12, 10)), doubled if phases else ops.conv3x3(x, w, b, upsample_size=(12, 10)))
        for size in ((11, 10), (11, 9)):
            assert torch.equal(m(x, size), ops.conv3x3(x, w, b, upsample_size=size))
        out = m(x, (13, 10))
    assert out.shape == (1, 64, 13, 10) and torch.isfinite(out).all()


def test_vae_conv_sites(ops, monkeypatch):
    """the decoder's _conv with the fused upsampling, and the encoder's downsampler on 6 x 8 (seen through a recording wrapper of
    conv3x3_try: the site sits inside AutoencoderKL.encode)"""
    from diffusionspatialcontrol_amd.modules import vae_decoder as vd
    conv = _module(torch.nn.Conv2d, 64, 64, 3, 1, 1)
    g, x, _, _ = _operands(1, 64, 64, 6, 5, seed=6)
    r = torch.randn(1, 64, 12, 10, generator=g).half().cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        assert torch.equal(vd._conv(conv, x, upsample=True), ops.conv3x3(x, conv.weight, conv.bias, upsample=True))
        assert torch.equal(vd._conv(conv, x, r, upsample=True), ops.conv3x3(x, conv.weight, conv.bias, r, upsample=True))
        assert torch.equal(vd._conv(conv, x), ops.conv3x3(x, conv.weight, conv.bias))
    calls, real = [], ops.conv3x3_try

    def recording(x, weight, bias=None, residual=None, **kw):
        y = real(x, weight, bias, residual, **kw)
        calls.append((x, weight, bias, kw, y))
        return y

    monkeypatch.setattr(ops, "conv3x3_try", recording)
    vae = _module(vd.AutoencoderKL, vd.VaeConfig(block_out_channels=(64, 64), layers_per_block=1, norm_num_groups=8))
    with torch.no_grad():
        vae.encode(torch.randn(1, 3, 6, 8, generator=g).half().cuda())
    down = [c for c in calls if c[3].get("mode") == ops.CONV_STRIDE2_PAD_BR]
    assert len(down) == 1
    x, weight, bias, _, y = down[0]
    assert tuple(x.shape[2:]) == (6, 8) and y is not None
    assert torch.equal(y, ops.conv3x3(x, weight, bias, stride2_pad_br=True))


def test_resnet_block_keeps_the_groupnorm_partials(ops, monkeypatch):
    """ResnetBlock2D at 32 x 32 (GN_FUSE_MIN_ROWS reached): conv1 and conv2 take the statistics-emitting form, the output carries
    the next GroupNorm's partial sums.  No existing test pins the block to its USE_GN_FUSE-off bytes (conv1's time-embedding row is
    added before the fp16 rounding in one form and inside norm2 in the other), so the two are compared with the tolerance of
    test_groupnorm_statistics_from_the_convolution_epilogue: |out - ref| <= 2e-3 |ref| + 4e-3"""
    from diffusionspatialcontrol_amd.modules import u_net_condition_modify as u
    assert 32 * 32 >= u.GN_FUSE_MIN_ROWS
    blk = _module(u.ResnetBlock2D, 64, 64, 128, 32, 1e-5)
    g, x, _, _ = _operands(1, 64, 64, 32, 32, seed=7)
    temb = torch.randn(1, 128, generator=g).half().cuda()
    with torch.no_grad():
        out = blk(x, temb)
        part = ops.gn_partials_of(out)
        assert part is not None and (part.groups, part.C, part.B, part.hw) == (32, 64, 1, 32 * 32)
        monkeypatch.setattr(ops, "USE_GN_FUSE", False)
        plain = blk(x, temb)
    assert ops.gn_partials_of(plain) is None
    assert torch.all((out.float() - plain.float()).abs() <= 2e-3 * plain.float().abs() + 4e-3), (out.float() - plain.float()).abs().max().item()
