"""The hires pass of the continuous batcher on the host: the tap tables of the latent resample (modules/latent_resample.py)
against torch.nn.functional.interpolate on the CPU, the target-size formula, and the chained pair of batchers
(ServingBatcher.chain_hires / HiresPair) against a fake executor: submit-time rejections, hand-off order, futures, stats."""
import pytest
import torch
import torch.nn.functional as F

from inputs import FakeTokenizer
from serving_fakes import RecordingExec

from diffusionspatialcontrol_amd.modules.latent_resample import MODES, hires_target_size, resample_taps
from diffusionspatialcontrol_amd.modules.serving import HiresPair, ServingBatcher

S = 77
VARIANTS = [(m, aa) for m in MODES for aa in ((False, True) if m in ("bilinear", "bicubic") else (False,))]
SIZES = [(5, 7), (16, 16), (16, 19), (16, 24), (16, 32), (64, 76), (64, 71)]


def _interp(x, size, mode, aa):
    return F.interpolate(x, size=size, mode=mode, **({"antialias": aa} if mode in ("bilinear", "bicubic") else {}))


def _matrix(n_in, n_out, mode, aa, dtype):
    """the table as a dense [n_out, n_in] matrix (taps that share an index add up, as they do in the kernel's sum)"""
    idx, w = resample_taps(n_in, n_out, mode, aa)
    assert idx.dtype == torch.int32 and w.dtype == torch.float32 and idx.shape == w.shape == (n_out, 4)
    assert idx.min() >= 0 and idx.max() < n_in                           # unused taps: weight 0 and a VALID index
    m = torch.zeros(n_out, n_in, dtype=dtype)
    for k in range(4):
        m[torch.arange(n_out), idx[:, k].long()] += w[:, k].to(dtype)
    return m


def _fma32(a, b, c):
    """fp32 fused multiply-add: the fp64 product of two fp32 numbers is exact, one rounding of the sum to fp32"""
    return (a.double() * b.double() + c.double()).float()


def _kernel_fp32(x, HW, mode, aa):
    """the fp32 value dsc_latent_resample_noise rounds to fp16, restated: per source row the taps of x in table order (a product,
    then one fma per tap), then the rows along y the same way (csrc/latent_resample.hip)"""
    iy, wy = resample_taps(x.shape[-2], HW[0], mode, aa)
    ix, wx = resample_taps(x.shape[-1], HW[1], mode, aa)
    out = None
    for i in range(4):
        rows, t = x[:, :, iy[:, i].long(), :], None
        for j in range(4):
            v = rows[..., ix[:, j].long()]
            t = v * wx[:, j] if t is None else _fma32(v, wx[:, j].expand_as(v), t)
        wcol = wy[:, i][:, None].expand_as(t)
        out = t * wcol if out is None else _fma32(t, wcol, out)
    return out


BIT_EXACT = {("bicubic", False), ("bicubic", True), ("bilinear", True)}


def _check_against_interpolate(hw, HW, mode, aa, seed):
    (h, w), (H, W) = hw, HW
    x = torch.randn(2, 4, h, w, generator=torch.Generator().manual_seed(seed))
    ref = _interp(x, (H, W), mode, aa)
    my, mx = _matrix(h, H, mode, aa, torch.float64), _matrix(w, W, mode, aa, torch.float64)
    got = my @ x.double() @ mx.T                                           # two small matrix products in fp64
    if mode in ("nearest", "nearest-exact"):
        assert torch.equal(got.float(), ref), (hw, HW, mode)
        return
    # three fp32 evaluation orders of the same sum: the kernel's, and rows first / columns first as matrix products
    my32, mx32 = my.float(), mx.float()
    kern = _kernel_fp32(x, (H, W), mode, aa)
    a, b = (my32 @ x) @ mx32.T, my32 @ (x @ mx32.T)
    spread = max((a - b).abs().max().item(), (a - kern).abs().max().item(), (b - kern).abs().max().item())
    err64, err = (got - ref.double()).abs().max().item(), (kern - ref).abs().max().item()
    print(f"{hw}->{HW} {mode}{' aa' if aa else ''}: fp64 tap sum vs interpolate {err64:.2e}, the kernel's fp32 order vs interpolate "
          f"{err:.2e}, three fp32 orders of the sum differ by up to {spread:.2e}")
    if hw == HW or (mode, aa) in BIT_EXACT:
        # the weights are torch's bit for bit and the order is torch's: the fp32 value is torch's, in every element
        assert torch.equal(kern, ref), (hw, HW, mode, aa, err)
    else:
        # plain bilinear (torch's 2-D kernel sums in an order not restated here) and area: torch's is a fourth fp32 order of the
        # same sum; it may be twice as far from the kernel's as the three above are from each other, and no further
        assert err <= 2 * spread, (hw, HW, mode, aa, err, spread)


@pytest.mark.parametrize("mode, aa", VARIANTS)
@pytest.mark.parametrize("n_in, n_out", SIZES)
def test_tap_tables_equal_interpolate(n_in, n_out, mode, aa):
    _check_against_interpolate((n_in, n_in), (n_out, n_out), mode, aa, seed=n_in * 100 + n_out)


@pytest.mark.parametrize("mode, aa", VARIANTS)
def test_tap_tables_non_square(mode, aa):
    _check_against_interpolate((16, 40), (19, 57), mode, aa, seed=3)
    _check_against_interpolate((5, 64), (7, 64), mode, aa, seed=4)         # one axis kept


def _reachable_pairs():
    """every (n_in, n_out) one axis of the feature can reach: sizes 64 .. 1600 px in steps of 8, factors 1.0 .. 2.0 in steps of 0.1,
    targets up to the kernel's 256 latent rows"""
    pairs = set()
    for n_in in range(8, 201):
        for f in range(10, 21):
            n_out = hires_target_size(n_in * 8, n_in * 8, f / 10)[0] // 8
            if n_out <= 256:
                pairs.add((n_in, n_out))
    return sorted(pairs)


@pytest.mark.parametrize("mode", ["nearest", "nearest-exact"])
def test_gather_indices_over_every_reachable_pair(mode):
    """the fp32 rounding of `scale` decides the sample: equal indices for every pair, not only a few"""
    pairs = _reachable_pairs()
    assert len(pairs) > 1000
    for n_in, n_out in pairs:
        idx, w = resample_taps(n_in, n_out, mode)
        ref = _interp(torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in), (1, n_out), mode, False).view(-1)
        assert torch.equal(idx[:, 0].float(), ref), (n_in, n_out, mode)
        assert torch.equal(w[:, 0], torch.ones(n_out)) and not w[:, 1:].any()


def test_taps_refuse_shrinking_and_unknown_modes():
    with pytest.raises(ValueError, match="enlarging"):
        resample_taps(16, 15, "bilinear")
    with pytest.raises(ValueError, match="mode"):
        resample_taps(16, 19, "lanczos")
    a = resample_taps(16, 19, "bicubic", True)
    assert a[0] is resample_taps(16, 19, "bicubic", True)[0]               # cached per (n_in, n_out, mode, antialias)
    assert not torch.equal(a[1], resample_taps(16, 19, "bicubic", False)[1])   # a different filter even when enlarging


@pytest.mark.parametrize("x", [1.0, 1.1, 1.2, 1.3, 1.5, 1.7, 1.9, 2.0])
@pytest.mark.parametrize("height, width", [(512, 512), (512, 768), (128, 128), (472, 600)])
def test_target_size_is_the_reference_expression(height, width, x):
    th, tw = hires_target_size(height, width, x)
    assert th == int(height * x // 8) * 8 and tw == int(width * x // 8) * 8            # model_k_diffusion.py:1177-1178
    if x == 1.0:
        assert (th, tw) == (height, width)
    assert hires_target_size(512, 512, 1.2) == (608, 608) and hires_target_size(512, 512, 1.1) == (560, 560)
    assert hires_target_size(512, 472, 1.2)[1] // 8 == 70                                # latent widths such as 70 occur


# ----------------------------------------------------------------------------- the chained pair against a fake executor
class FakeHiresExec(RecordingExec):
    """one event log shared by both batchers of a pair; a request's result says which batcher finished it"""
    step_keys, join_keys = ("step", "sigma"), None

    def result(self, r, h):
        return (self.name, r.output_type, self.applied[id(r)])


@pytest.fixture(scope="module")
def pipe():
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    unet = UNet2DConditionModel(UNetConfig.tiny()).half()
    return StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())


def _req(name, steps=4, **kw):
    emb = torch.randn(2, S, 64, generator=torch.Generator().manual_seed(len(name) + steps))
    r = {"name": name, "prompt_embeds": emb[1:2].half(), "negative_prompt_embeds": emb[0:1].half(),
         "num_inference_steps": steps, "guidance_scale": 7.5, "sampler_opt": {"scheduler": "karras"}}
    r.update(kw)
    return r


LAT = torch.zeros(1, 4, 16, 16).half()
HIRES = dict(upscale=True, upscale_x=1.5)


def _pair(pipe, **kw):
    log = []
    kw = dict(dict(max_batch=2, buckets=(1, 2)), **kw)
    base = ServingBatcher(pipe, 128, 128, slot=0, executor=FakeHiresExec("base", log), **kw)
    hi = ServingBatcher(pipe, 192, 192, slot=1, executor=FakeHiresExec("hires", log), **kw)
    return HiresPair(base, hi), log


def test_chain_hires_refuses_itself_and_a_shared_slot(pipe):
    log = []
    a = ServingBatcher(pipe, 128, 128, slot=0, executor=FakeHiresExec("a", log))
    same_slot = ServingBatcher(pipe, 192, 192, slot=0, executor=FakeHiresExec("b", log))
    smaller = ServingBatcher(pipe, 64, 64, slot=1, executor=FakeHiresExec("c", log))
    with pytest.raises(ValueError, match="itself"):
        a.chain_hires(a)
    with pytest.raises(ValueError, match="slot"):
        a.chain_hires(same_slot)
    with pytest.raises(ValueError, match="smaller"):
        a.chain_hires(smaller)
    with pytest.raises(TypeError):
        a.chain_hires(None)
    with pytest.raises(ValueError, match="shrinks"):
        pipe.serve_hires(128, 128, 0.5)
    with pytest.raises(ValueError, match="multiples of 8 "):          # 128 * 1.2 -> 152 px = 19 latent rows: the skips do not line up
        pipe.serve_hires(128, 128, 1.2)


def test_unchained_batcher_still_refuses_upscale(pipe):
    b = ServingBatcher(pipe, 128, 128, executor=FakeHiresExec("solo", []))
    with pytest.raises(ValueError, match="upscale.*chained"):
        b.submit(_req("X", latents=LAT, **HIRES))
    pair, _ = _pair(pipe)
    with pytest.raises(ValueError, match="upscale.*chained"):                # the second batcher of a pair is not chained on
        pair.hires.submit(_req("X", **HIRES))


@pytest.mark.parametrize("bad, match", [
    ({"upscale_x": 1.2}, "152x152"),                                         # another target than the chained batcher's
    ({"upscale_x": 2.0}, "256x256"),
    ({"upscale_x": 0.5}, "shrinks.*txt2img"),                                # names the pipeline method
    ({"upscale_x": "big"}, "upscale_x"),
    ({"upscale_denoising_strength": 0.1}, "upscale_denoising_strength"),     # int(4 * 0.1) == 0 steps of the second pass
    ({"upscale_denoising_strength": 0.0}, "upscale_denoising_strength"),
    ({"upscale_denoising_strength": 1.5}, "upscale_denoising_strength"),
    ({"image": LAT, "mask_image": torch.ones(1, 1, 128, 128)}, "mask_image"),
    ({"sampler_name_hires": "sample_heun"}, "sampler_name_hires"),
    ({"upscale_method": "lanczos"}, "upscale_method"),
    ({"hires_latents": torch.zeros(1, 4, 16, 16).half()}, "hires_latents"),
    ({"region_map_state_hires": {64: torch.zeros(2, 64, S)}}, "region tables"),
])
def test_hires_rejections_at_submit(pipe, bad, match, monkeypatch):
    pair, log = _pair(pipe)
    if "region_map_state_hires" in bad:        # tables of another image size: what encode_region_map gives for a wrong state
        from diffusionspatialcontrol_amd.modules.serving import batcher as serving
        real = serving.encode_region_map
        monkeypatch.setattr(serving, "encode_region_map",
                            lambda p, state, **kw: state if isinstance(state, dict) and 64 in state else real(p, state, **kw))
    with pytest.raises(ValueError, match=match):
        pair.submit(_req("X", latents=LAT, **dict(HIRES, **bad)))
    assert not [e for e in log if e[0] == "prepare"]                         # rejected before either pass touched the device
    f = pair.submit(_req("ok", latents=LAT, **HIRES))                        # the pair goes on serving
    pair.run_until_idle()
    assert f.done() and f.result()[0] == "hires"


def test_hand_off_order_future_and_stats(pipe):
    """one hires request (Euler a in the second pass, its own schedule) next to a plain one: both passes are prepared at submit,
    first pass first; the hand-off happens when the first pass's last step is applied, the second batcher loads the row with the
    hand-off's event, and the ONE future resolves with the second pass's output"""
    pair, log = _pair(pipe)
    fh = pair.submit(_req("H", steps=5, latents=LAT, output_type="pil", sampler_name_hires="sample_euler_ancestral",
                          sampler_opt_hires={"scheduler": "exponential"}, upscale_denoising_strength=0.6, **HIRES))
    fp = pair.submit(_req("P", steps=3, latents=LAT))
    assert log[:3] == [("prepare", "base", "H", "txt2img"), ("prepare", "hires", "H", "second"), ("noise", "hires", "H")]
    assert log[3] == ("prepare", "base", "P", "txt2img")
    pair.run_until_idle()
    where, out_type, applied = fh.result()
    assert (where, out_type) == ("hires", "pil")                             # output_type applies to the second pass
    sig2 = pipe._schedule(5, {"scheduler": "exponential"}, "cpu", torch.float16).float().tolist()[2:]     # int(5 * 0.6) steps
    assert [a[1:] for a in applied] == [(i, s) for i, s in enumerate(sig2[:3])]
    assert fp.result()[0] == "base" and len(fp.result()[2]) == 3
    kinds = [e[0] for e in log]
    i_hand, i_load = kinds.index("hand_off"), [i for i, e in enumerate(log) if e[:3] == ("load", "hires", "H")][0]
    assert log[i_hand] == ("hand_off", "base", "H", "bicubic", sig2[0]) and i_hand < i_load
    assert log[i_load][3] == ("event", "H")                                  # the second batcher waits on the hand-off's event
    assert ("finish", "base", "H") not in log and ("finish", "hires", "H") in log and ("finish", "base", "P") in log
    st = pair.stats()
    assert st["handoffs"] == 1 and st["base"]["leaves"] == 2 and st["hires"]["joins"] == 1 and st["hires"]["leaves"] == 1
    assert st["hires"]["linear_transitions"] == 3 and st["base"]["linear_transitions"] == 0
    assert fh.dsc_latency_s >= fh.dsc_first_pass_s >= 0.0                    # the latency spans both passes


def test_hand_off_into_a_full_second_batcher(pipe):
    """max_batch = 1 on both: the second batcher is busy with an outside request of its own size when H finishes pass one.  H's
    row is handed off at once (its slot in the first batcher frees for W), waits in the second batcher's queue, and runs when
    the outside request has left; a second hires request follows it (FIFO)"""
    pair, log = _pair(pipe, max_batch=1, buckets=(1,))
    big = torch.zeros(1, 4, 24, 24).half()
    fo = pair.hires.submit(_req("outside", steps=12, latents=big))
    fh = pair.submit(_req("H", steps=2, latents=LAT, **HIRES))
    fw = pair.submit(_req("W", steps=2, latents=LAT, upscale_method="nearest-exact", **HIRES))
    while not any(e[:3] == ("hand_off", "base", "H") for e in log):
        assert pair.step()
    st = pair.stats()
    assert st["hires"]["active"] == 1 and st["hires"]["queued"] == 1 and not fh.done() and not fo.done()
    assert pair.base._slots[0] is None or pair.base._slots[0].req["name"] == "W"       # H's first-pass slot is free again
    pair.run_until_idle()
    assert fo.result()[0] == "hires" and len(fo.result()[2]) == 12
    assert fh.result()[0] == "hires" and fw.result()[0] == "hires"
    loads = [e[2] for e in log if e[0] == "load" and e[1] == "hires"]
    assert loads == ["outside", "H", "W"]
    assert [e[3] for e in log if e[0] == "hand_off"] == ["bicubic", "nearest-exact"]
    st = pair.stats()
    assert st["handoffs"] == 2 and st["hires"]["joins"] == 3 and st["base"]["queued"] == 0 and st["hires"]["queued"] == 0


def test_requests_without_upscale_are_untouched(pipe):
    """a plain request on the pair never reaches the second batcher, and carries no hires state"""
    pair, log = _pair(pipe)
    f = pair.submit(_req("P", steps=3, image=LAT, strength=0.7))
    pair.run_until_idle()
    assert f.result()[0] == "base" and not [e for e in log if e[1] == "hires"]
    assert pair.stats()["handoffs"] == 0 and pair.stats()["hires"]["joins"] == 0


def test_second_pass_defaults_follow_the_pipeline_methods(pipe):
    """no hires keys but `upscale`: factor 2.0, bicubic, strength 0.7, the first pass's sampler and options; img2img + hires runs"""
    log = []
    base = ServingBatcher(pipe, 128, 128, slot=0, max_batch=2, buckets=(1, 2), executor=FakeHiresExec("base", log))
    hi = ServingBatcher(pipe, 256, 256, slot=1, max_batch=2, buckets=(1, 2), executor=FakeHiresExec("hires", log))
    pair = HiresPair(base, hi)
    f = pair.submit(_req("H", steps=10, image=LAT, strength=0.5, upscale=True, sampler_name="sample_euler"))
    pair.run_until_idle()
    sig = pipe._schedule(10, {"scheduler": "karras"}, "cpu", torch.float16).float().tolist()
    assert [a[2] for a in f.result()[2]] == sig[3:10]                        # int(10 * 0.7) steps of the same schedule
    assert ("prepare", "base", "H", "img2img") in log and ("hand_off", "base", "H", "bicubic", sig[3]) in log
    assert pair.stats()["hires"]["linear_transitions"] == 7                  # Euler in the second pass too
