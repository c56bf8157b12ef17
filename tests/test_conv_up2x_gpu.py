"""Upsample2D's convolution as four 2x2 phase convolutions of the source (dsc_conv3x3_up2x_nhwc_f16, dsc_conv3x3_up2x_pack_f16).

    out[2i+py, 2j+px] = sum_{a,b in {0,1}} K[py][px][a][b] . x[i+py+a-1, j+px+b-1]          (x = 0 outside the source)
    K[py][px][a][b]   = sum_{dy in R(py,a)} sum_{dx in R(px,b)} w[dy][dx],  R(0,0)={0} R(0,1)={1,2} R(1,0)={0,1} R(1,1)={2}

Tolerances.  Against the fp32 convolution of the materialised image: the existing convolution tests' |out - ref| <= 1.5e-3 |ref| +
2e-3 (tests/test_unet_pipeline_gpu.py::test_conv3x3_upsample); the phase arithmetic alone - fp16 rounding of the summed weights,
exact accumulation - stays at <= 0.5 of it on these operand distributions.  Against four fp32 2x2 convolutions with the PACKED
weights (no weight rounding left: only the kernel's fp32 accumulation order and its one output rounding) the same bound; the
ratio printed there should sit near 0.25, the figure of the 9-tap kernel against its own reference.  Split against unsplit: both
round the same sum up to fp32 reassociation (~1e-6 relative), so the fp16 results differ by at most one fp16 spacing,
2^-10 |v| < 1.0e-3 |v|, plus 1e-5 for sums that cancel to near zero."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from inputs import FakeTokenizer
from oracle import unet_ref

CL = torch.channels_last
gpu = pytest.mark.gpu
R = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}

# (B, Cin, Cout, h, w) of the SOURCE: ragged both ways + a single slice | 8-wide tiles pairing sub-blocks of different images, B = 3 |
# several 16-wide tiles with overhang | 5 slices (odd, against halo-buffer parity and the ring) | 10 slices | 20 slices, split
SHAPES = [(1, 64, 64, 3, 5), (3, 128, 64, 4, 4), (1, 64, 64, 9, 17), (2, 320, 320, 16, 16), (2, 640, 640, 8, 8)]
SPLIT_SHAPE = (2, 1280, 1280, 8, 8)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


def _operands(B, C, Cout, h, w, seed):
    """the operand distributions of tests/test_any_size_gpu.py::_conv_operands"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, h, w, generator=g).half().cuda().contiguous(memory_format=CL)
    wt = (torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(9 * C)).half().cuda().contiguous(memory_format=CL)
    b = (torch.randn(Cout, generator=g) * 0.2).half().cuda()
    return x, wt, b


def _pack_ref(wt):
    """[Cout, Cin, 3, 3] -> [4, Cout, 4, Cin]: fp32 sums, dy ascending (outer) then dx ascending (inner), one rounding"""
    w32 = wt.float()
    out = torch.empty((4, wt.shape[0], 4, wt.shape[1]), dtype=torch.float16, device=wt.device)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    acc = None
                    for dy in R[(py, a)]:
                        for dx in R[(px, b)]:
                            acc = w32[:, :, dy, dx] if acc is None else acc + w32[:, :, dy, dx]
                    out[2 * py + px, :, 2 * a + b, :] = acc.half()
    return out


def _phase_ref(x, packed, bias):
    """four fp32 2x2 convolutions of the zero-padded source with the packed weights, interleaved into [B, Cout, 2h, 2w]"""
    B, C, h, w = x.shape
    Cout = packed.shape[1]
    xp = F.pad(x.float(), (1, 1, 1, 1))
    out = torch.empty((B, Cout, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    for py in range(2):
        for px in range(2):
            k = packed[2 * py + px].float().view(Cout, 2, 2, C).permute(0, 3, 1, 2).contiguous()
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + w + 1], k, None if bias is None else bias.float())
    return out


def _ratio(out, ref):
    """worst |out - ref| as a fraction of the bound 1.5e-3 |ref| + 2e-3"""
    return ((out.float() - ref).abs() / (1.5e-3 * ref.abs() + 2e-3)).max().item()


def test_phase_identity_on_the_cpu():
    """the identity itself, in fp64 with unrounded summed weights, borders included (no GPU)"""
    g = torch.Generator().manual_seed(3)
    for h, w in ((1, 1), (3, 5), (4, 4)):
        x = torch.randn(2, 8, h, w, generator=g, dtype=torch.float64)
        wt = torch.randn(5, 8, 3, 3, generator=g, dtype=torch.float64)
        ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, padding=1)
        xp = F.pad(x, (1, 1, 1, 1))
        for py in range(2):
            for px in range(2):
                k = torch.zeros(5, 8, 2, 2, dtype=torch.float64)
                for a in range(2):
                    for b in range(2):
                        for dy in R[(py, a)]:
                            for dx in R[(px, b)]:
                                k[:, :, a, b] += wt[:, :, dy, dx]
                got = F.conv2d(xp[:, :, py:py + h + 1, px:px + w + 1], k)
                assert torch.allclose(got, ref[:, :, py::2, px::2], rtol=1e-12, atol=1e-12), (h, w, py, px)


@gpu
@pytest.mark.parametrize("B,C,Cout,h,w", SHAPES + [SPLIT_SHAPE])
def test_pack_entry_equals_the_same_sums_in_torch(ops, B, C, Cout, h, w):
    _, wt, _ = _operands(B, C, Cout, h, w, seed=C + Cout)
    packed = ops.conv3x3_up2x_pack(wt)
    assert packed.shape == (4, Cout, 4, C) and packed.dtype == torch.float16 and packed.is_contiguous()
    assert torch.equal(packed, _pack_ref(wt))
    assert torch.equal(packed, ops.conv3x3_up2x_pack(wt.contiguous()))          # any memory format of the weight


@gpu
@pytest.mark.parametrize("B,C,Cout,h,w", SHAPES)
def test_up2x_against_the_reference_and_the_packed_weights(ops, B, C, Cout, h, w):
    for seed in range(3):
        x, wt, b = _operands(B, C, Cout, h, w, seed=seed * 101 + B + C + h + w)
        assert ops.conv3x3_up2x_supported(x, wt)
        packed = ops.conv3x3_up2x_pack(wt)
        out = ops.conv3x3_up2x(x, packed, b)
        assert out.shape == (B, Cout, 2 * h, 2 * w) and out.is_contiguous(memory_format=CL) and out.dtype == torch.float16
        ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest").float(), wt.float(), b.float(), padding=1)
        ref_p = _phase_ref(x, packed, b)
        r1, r2 = _ratio(out, ref), _ratio(out, ref_p)
        print(f"up2x {(B, C, Cout, h, w)} seed {seed}: worst ratio vs reference {r1:.3f}, vs packed weights {r2:.3f}")
        assert r1 <= 1.0, r1
        assert r2 <= 1.0, r2
        assert torch.equal(out, ops.conv3x3_up2x(x, packed, b))                   # reproducible
        out_n = ops.conv3x3_up2x(x, packed, None)
        assert _ratio(out_n, ref_p - b.float().view(1, -1, 1, 1)) <= 1.0
    # a localised impulse: every tap of every phase lands where it should, independent of the tolerance
    xi = torch.zeros(B, C, h, w).half()
    xi[B - 1, 5, h - 1, 0] = 1.0
    xi[0, C - 1, min(2, h - 1), w - 1] = 2.0
    xi = xi.cuda().contiguous(memory_format=CL)
    oi = ops.conv3x3_up2x(xi, packed, None).float()
    ri = _phase_ref(xi, packed, None)
    assert torch.all((oi - ri).abs() <= 1e-3 * ri.abs() + 1e-6)


@gpu
@pytest.mark.parametrize("splits", [0, 1, 2, 3])
def test_up2x_split_over_input_channels(ops, splits):
    B, C, Cout, h, w = SPLIT_SHAPE
    x, wt, b = _operands(B, C, Cout, h, w, seed=17)
    packed = ops.conv3x3_up2x_pack(wt)
    out = ops.conv3x3_up2x(x, packed, b, splits=splits)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest").float(), wt.float(), b.float(), padding=1)
    r1, r2 = _ratio(out, ref), _ratio(out, _phase_ref(x, packed, b))
    print(f"up2x {SPLIT_SHAPE} splits {splits}: worst ratio vs reference {r1:.3f}, vs packed weights {r2:.3f}")
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
    assert torch.equal(out, ops.conv3x3_up2x(x, packed, b, splits=splits))
    one = ops.conv3x3_up2x(x, packed, b, splits=1).float()
    assert torch.all((out.float() - one).abs() <= 1.0e-3 * one.abs() + 1e-5)     # one fp16 spacing (module docstring)


@gpu
@pytest.mark.parametrize("B,C,Cout,h,w,splits", [SHAPES[1] + (0,), SHAPES[3] + (0,), SPLIT_SHAPE + (0,), SPLIT_SHAPE + (2,)])
def test_up2x_profiles_and_ring_settings_give_equal_bytes(ops, B, C, Cout, h, w, splits):
    """the tuning profiles and every dsc_debug_set_conv_ring setting (forced ring depths, loader waves off / by rule / always)"""
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    x, wt, b = _operands(B, C, Cout, h, w, seed=5)
    packed = ops.conv3x3_up2x_pack(wt)
    outs = {}
    try:
        for prof in ("latency", "throughput"):
            ops.set_tuning_profile(prof)
            outs[prof] = ops.conv3x3_up2x(x, packed, b, splits=splits)
        for setting in (3, 9, 400, 402):
            lib.dsc_debug_set_conv_ring(setting)
            outs[setting] = ops.conv3x3_up2x(x, packed, b, splits=splits)
    finally:
        lib.dsc_debug_set_conv_ring(401)
        lib.dsc_debug_set_conv_ring(0)
        ops.set_tuning_profile("latency")
    for k, v in outs.items():
        assert torch.equal(v, outs["latency"]), k


@gpu
def test_up2x_reads_nothing_beyond_its_source(ops):
    """x is a view into a larger buffer whose remainder is NaN (the pattern of
    test_conv3x3_sized_upsample_reads_nothing_beyond_its_source): a halo that reached past the source would bring NaNs in"""
    for B, C, Cout, h, w in ((2, 64, 64, 4, 4), (1, 64, 64, 3, 5), (1, 64, 64, 9, 17)):
        x, wt, b = _operands(B, C, Cout, h, w, seed=11)
        packed = ops.conv3x3_up2x_pack(wt)
        want = ops.conv3x3_up2x(x, packed, b)
        n = B * h * w * C
        buf = torch.full((n + 4096,), float("nan"), dtype=torch.float16, device="cuda")
        buf[:n] = x.permute(0, 2, 3, 1).reshape(-1)
        view = buf[:n].view(B, h, w, C).permute(0, 3, 1, 2)
        assert view.is_contiguous(memory_format=CL) and view.data_ptr() == buf.data_ptr()
        got = ops.conv3x3_up2x(view, packed, b)
        assert torch.isfinite(got).all() and torch.equal(got, want)


def test_up2x_refusals_need_no_gpu(monkeypatch):
    from diffusionspatialcontrol_amd import _lib, build as dsc_build, ops
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import Upsample2D
    dsc_build.build(verbose=False)
    lib = _lib.load_library()
    d = ctypes.c_void_p(0x1000)
    call = lambda **kw: lib.dsc_conv3x3_up2x_nhwc_f16(  # noqa: E731
        kw.get("x", d), kw.get("wp", d), kw.get("bias", None), kw.get("out", d), kw.get("B", 2), 8, 8, kw.get("Cin", 64),
        kw.get("Cout", 64), kw.get("splits", 1), None, 0, kw.get("ldx", kw.get("Cin", 64)), kw.get("ldo", kw.get("Cout", 64)),
        kw.get("dtype", 0), None)
    assert call(x=None) == -1 and call(wp=None) == -1 and call(out=None) == -1 and call(B=0) == -1
    for k in ("x", "wp", "out", "bias"):
        assert call(**{k: ctypes.c_void_p(0x1004)}) == -2, k                       # unaligned pointers
    assert call(Cin=96) == -2 and call(Cin=32) == -2                               # Cin not a multiple of 64
    assert call(Cout=40) == -2 and call(dtype=7) == -2 and call(ldx=68) == -2 and call(ldx=32) == -1
    assert call(Cin=1280, Cout=1280, splits=2) == -3                               # a split needs its workspace
    assert lib.dsc_conv3x3_up2x_supported(2, 8, 8, 64, 64) == 1 and lib.dsc_conv3x3_up2x_supported(2, 5, 7, 64, 64) == 1
    assert lib.dsc_conv3x3_up2x_supported(2, 8, 8, 96, 64) == 0 and lib.dsc_conv3x3_up2x_supported(2, 8, 8, 64, 40) == 0
    assert lib.dsc_conv3x3_up2x_supported(0, 8, 8, 64, 64) == 0 and lib.dsc_conv3x3_up2x_supported(4096, 64, 64, 1280, 1280) == 0
    assert lib.dsc_conv3x3_up2x_workspace_bytes(2, 8, 8, 1280, 1280, 2) == 2 * (2 * 16 * 16) * 1280 * 4
    assert lib.dsc_conv3x3_up2x_workspace_bytes(2, 8, 8, 1280, 1280, 1) == 0
    assert lib.dsc_conv3x3_up2x_pack_f16(d, d, 96, 64, None) == -2 and lib.dsc_conv3x3_up2x_pack_f16(None, d, 64, 64, None) == -1
    assert lib.dsc_conv3x3_up2x_pack_f16(ctypes.c_void_p(0x1004), d, 64, 64, None) == -2
    # a packed tensor of the wrong shape (checked before anything asks for a GPU)
    x = torch.zeros(1, 64, 4, 4, dtype=torch.float16)
    for bad in (torch.zeros(4, 64, 9, 64), torch.zeros(4, 64, 4, 128), torch.zeros(64, 64, 3, 3), torch.zeros(3, 64, 4, 64)):
        with pytest.raises(ValueError):
            ops.conv3x3_up2x(x, bad.half())
    with pytest.raises(ValueError):
        ops.conv3x3_up2x(x, torch.zeros(4, 64, 4, 64))                             # fp32
    # odd skip-sized targets keep the gather form; None and exactly (2h, 2w) take the phase entry
    calls = []
    monkeypatch.setattr(ops, "USE_UP2X_PHASES", True)
    monkeypatch.setattr(ops, "conv3x3_up2x_supported", lambda x, w: True)
    monkeypatch.setattr(ops, "conv3x3_up2x_pack", lambda w: "packed")
    monkeypatch.setattr(ops, "conv3x3_up2x", lambda x, packed, bias: calls.append(packed) or "phases")
    monkeypatch.setattr(ops, "conv3x3_supported", lambda *a, **k: True)
    monkeypatch.setattr(ops, "conv3x3", lambda *a, **k: "gather")
    up = Upsample2D(64).half()
    assert up(x) == "phases" and up(x, output_size=(8, 8)) == "phases" and calls == ["packed", "packed"]
    for odd in ((7, 7), (8, 7), (7, 8)):
        assert up(x, output_size=odd) == "gather"
    monkeypatch.setattr(ops, "USE_UP2X_PHASES", False)
    assert up(x) == "gather" and up(x, output_size=(8, 8)) == "gather" and len(calls) == 2


@gpu
def test_upsample2d_packs_once_per_weight_and_replays_in_a_graph(ops, monkeypatch):
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import Upsample2D
    monkeypatch.setattr(ops, "USE_UP2X_PHASES", True)
    torch.manual_seed(3)
    up = Upsample2D(64).half().cuda()
    up.conv.weight.data = up.conv.weight.data.contiguous(memory_format=CL)
    x, _, _ = _operands(2, 64, 64, 8, 8, seed=1)
    x2, _, _ = _operands(2, 64, 64, 8, 8, seed=2)
    packs = []
    real_pack = ops.conv3x3_up2x_pack
    monkeypatch.setattr(ops, "conv3x3_up2x_pack", lambda w: packs.append(1) or real_pack(w))
    with torch.no_grad():
        y = up(x)
        assert torch.equal(y, up(x, output_size=(16, 16))) and len(packs) == 1        # cached
        ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest").float(), up.conv.weight.float(), up.conv.bias.float(), padding=1)
        assert _ratio(y, ref) <= 1.0
        assert torch.equal(up(x, output_size=(15, 16)), ops.conv3x3(x, up.conv.weight, up.conv.bias, upsample_size=(15, 16)))
        xs = x.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yg = up(xs)
        xs.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, up(x2)) and len(packs) == 1
        up.conv.weight.mul_(0.5)                                                      # an in-place write re-packs
        y_half = up(x)
        assert len(packs) == 2
        assert torch.equal(y_half, ops.conv3x3_up2x(x, real_pack(up.conv.weight), up.conv.bias))
        assert not torch.equal(y_half, y)


def _tiny_unet(seed=0):
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(seed)
    cfg = UNetConfig.tiny()
    unet = UNet2DConditionModel(cfg).half()
    sd = {k: v.clone() for k, v in unet.state_dict().items()}
    text = torch.randn(2, 77, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(7)).half()
    return cfg, unet.cuda(), sd, text


@gpu
def test_toy_unet_forward_with_and_without_the_phase_form(ops, monkeypatch):
    """toy widths (tests/test_unet_pipeline_gpu.py::test_unet_forward_matches_oracle and its bound): DSC_UP2X_PHASES on and off,
    each against the fp32 oracle; on, the three upsamplers run the phase entry, off, none does"""
    cfg, unet, sd, text = _tiny_unet()
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(5)).half()
    t = torch.tensor([731.25, 731.25])
    ref = unet_ref.unet_forward(sd, cfg, x.float(), t, text.float())
    scale = ref.abs().max().item()
    calls = []
    real = ops.conv3x3_up2x
    monkeypatch.setattr(ops, "conv3x3_up2x", lambda *a, **k: calls.append(1) or real(*a, **k))
    outs = {}
    for flag in (True, False):
        monkeypatch.setattr(ops, "USE_UP2X_PHASES", flag)
        del calls[:]
        outs[flag] = unet(x.cuda(), t.cuda(), text.cuda()).sample.float().cpu()
        assert len(calls) == (3 if flag else 0)
        err = (outs[flag] - ref).abs()
        print(f"toy UNet, phases {flag}: max {err.max().item() / scale:.2e} mean {err.mean().item() / scale:.2e} of the range")
        assert err.max().item() < 1e-2 * scale + 1e-3, (flag, err.max().item(), scale)
        assert err.mean().item() < 2e-3 * scale
    d = (outs[True] - outs[False]).abs()
    print(f"toy UNet, phases on vs off: max {d.max().item() / scale:.2e} mean {d.mean().item() / scale:.2e} of the range")


@gpu
def test_captured_step_replays_like_eager_with_the_phase_form(ops, monkeypatch):
    """the captured-step path against the eager loop with the flag on, at the bound of
    tests/test_unet_pipeline_gpu.py::test_diffusers_pipeline_graph_replay_equals_eager (same kernels and operands up to the shared
    CFG prefix's launch geometry and MIOpen's atomic convolutions at toy widths)"""
    from inputs import prompt_ids, rect_map
    from diffusionspatialcontrol_amd.modules.model_diffusers import EulerDiscreteScheduler, StableDiffusionPipeline_finetune
    monkeypatch.setattr(ops, "USE_UP2X_PHASES", True)
    cfg, unet, sd, text = _tiny_unet()
    ids = [prompt_ids("blurry"), prompt_ids("a photo of a red apple on a wooden table near a blue vase")]
    state = {"red apple": {"map": rect_map(128, 128, 0, 0, 1, 2), "weight": 0.5, "mask_outsides": 0.0}}
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(2001)).half()
    calls = []
    real = ops.conv3x3_up2x
    monkeypatch.setattr(ops, "conv3x3_up2x", lambda *a, **k: calls.append(1) or real(*a, **k))
    outs = {}
    for name, graph in (("eager", False), ("graph", True)):
        monkeypatch.setattr(ops, "PROTOCOL_GRAPH", graph)
        pipe = StableDiffusionPipeline_finetune(None, None, FakeTokenizer(), unet, EulerDiscreteScheduler())
        outs[name] = pipe(height=128, width=128, num_inference_steps=5, guidance_scale=6.0, latents=lat.clone(), output_type="latent",
                          prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], region_map_state=state,
                          text_input_ids=ids)[0].float().cpu()
        if graph:
            assert pipe._graphs
    assert calls
    scale = outs["eager"].abs().max().item()
    err = (outs["graph"] - outs["eager"]).abs()
    assert err.max().item() < 2e-2 * scale and err.mean().item() < 3e-3 * scale, (err.max().item(), err.mean().item(), scale)
