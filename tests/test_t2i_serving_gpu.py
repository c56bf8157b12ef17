"""T2I-Adapter requests in the continuous batcher on the MI355X (`-m gpu`): dsc_add_rows_gated_f16 (a residual added with one
gate per batch row, read on the device) against torch's fp16 add and an fp64 restatement, its skip / capture / determinism
properties and the wrapper's refusals; the UNet's `down_intrablock_gated` keyword against the eager hook; and the serving batcher
with control images against the oracle loop, `txt2img` / `img2img` and itself."""
import dataclasses
import math

import pytest
import torch

from inputs import FakeTokenizer
from oracle import unet_ref

pytestmark = pytest.mark.gpu
CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- the kernel
SHAPES = [(4, 2, 32, 16, 16),
          (4, 2, 64, 2, 2),            # 256 halfs per row: less than one wave of 16-byte pieces
          (6, 3, 320, 19, 19),         # odd, with a ragged last block
          (2, 1, 1280, 8, 8),
          (4, 4, 64, 4, 4),            # feat_rows == rows
          (4, 2, 320, 64, 64)]         # one real level: the grid cap and the stride


def _operands(rows, feat_rows, C, h, w, seed):
    """x and feat of the same size of values, channels-last, on the GPU"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, h, w, generator=g).half().contiguous(memory_format=CL).cuda()
    feat = torch.randn(feat_rows, C, h, w, generator=g).half().contiguous(memory_format=CL).cuda()
    return x, feat


@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("rows, feat_rows, C, h, w", SHAPES)
def test_gate_one_is_torchs_fp16_add_and_gate_zero_is_x(ops, rows, feat_rows, C, h, w, in_place):
    x, feat = _operands(rows, feat_rows, C, h, w, seed=rows + C + h)
    gate = torch.tensor([1.0, 0.0] * (rows // 2), device="cuda")
    ref = x + feat.repeat(rows // feat_rows, 1, 1, 1)                       # torch's fp16 add: x[r] + feat[r % F]
    src = x.clone(memory_format=torch.preserve_format)
    out = ops.add_rows_gated(src, feat, gate, out=src if in_place else None)
    torch.cuda.synchronize()
    assert (out.data_ptr() == src.data_ptr()) == in_place and out.shape == x.shape and out.is_contiguous(memory_format=CL)
    assert torch.equal(src, x) or in_place                                   # out of place: the source is not written
    for r in range(rows):
        assert torch.equal(out[r], ref[r] if r % 2 == 0 else x[r]), r
    assert not torch.equal(out[0], x[0])


def test_general_gates_within_one_ulp_of_the_fp64_value(ops):
    """every element within one fp16 ulp of x + g * feat in fp64, the ulp taken at max(|value|, 2**-14): one fp32 fma (relative
    error 2**-24) and one fp16 rounding (half an ulp of the result).  Measured on one MI355X: worst error 0.600 ulp."""
    rows, F_, C, h, w = 6, 3, 320, 19, 19
    x, feat = _operands(rows, F_, C, h, w, seed=7)
    gates = [0.7, -0.5, 2.0, 2.0, 0.7, -0.5]
    got = ops.add_rows_gated(x, feat, torch.tensor(gates, device="cuda")).double().cpu()
    want = x.double().cpu() + torch.tensor(gates, dtype=torch.float64).view(-1, 1, 1, 1) * feat.double().cpu().repeat(2, 1, 1, 1)
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -14))) - 10)
    worst = ((got - want).abs() / ulp).max().item()
    print(f"general gates: worst error {worst:.3f} ulp")
    assert worst <= 1.0


@pytest.mark.parametrize("in_place", [True, False])
def test_skipped_rows_read_nothing(ops, in_place):
    """feature rows that belong only to gate-0 batch rows hold NaN: the output is finite and equals x there"""
    rows, F_, C, h, w = 4, 4, 64, 4, 4
    x, feat = _operands(rows, F_, C, h, w, seed=8)
    feat[1], feat[3] = float("nan"), float("nan")
    gate = torch.tensor([1.0, 0.0, 0.5, 0.0], device="cuda")
    src = x.clone(memory_format=torch.preserve_format)
    out = ops.add_rows_gated(src, feat, gate, out=src if in_place else None)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(out[1], x[1]) and torch.equal(out[3], x[3]) and not torch.equal(out[2], x[2])


def test_under_graph_capture_the_replay_reads_the_device_values_of_that_moment(ops):
    """one captured in-place call; gate and feat are overwritten in place and x reset before the replay"""
    rows, F_, C, h, w = 4, 2, 32, 16, 16
    x, feat = _operands(rows, F_, C, h, w, seed=9)
    _, feat2 = _operands(rows, F_, C, h, w, seed=10)
    gate = torch.tensor([1.0, 0.0, 1.0, 0.0], device="cuda")
    gate2 = torch.tensor([0.0, 1.0, 0.25, 0.0], device="cuda")
    buf = x.clone(memory_format=torch.preserve_format)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.add_rows_gated(buf, feat, gate, out=buf)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    buf.copy_(x)
    with torch.cuda.graph(g):
        ops.add_rows_gated(buf, feat, gate, out=buf)
    gate.copy_(gate2)
    feat.copy_(feat2)
    buf.copy_(x)
    g.replay()
    fresh = ops.add_rows_gated(x, feat2, gate2)
    torch.cuda.synchronize()
    assert torch.equal(buf, fresh)
    assert torch.equal(buf[0], x[0]) and torch.equal(buf[3], x[3]) and not torch.equal(buf[1], x[1])


def test_determinism_and_features_as_a_view_into_a_flat_buffer(ops):
    rows, F_, C, h, w = 6, 3, 320, 19, 19
    x, feat = _operands(rows, F_, C, h, w, seed=11)
    gate = torch.tensor([1.0, 0.3, 0.0, -1.0, 1.0, 2.0], device="cuda")
    a = ops.add_rows_gated(x, feat, gate)
    b = ops.add_rows_gated(x, feat, gate)
    n = C * h * w
    flat = torch.zeros(F_ * n + 64, dtype=torch.float16, device="cuda")
    view = flat[8:8 + F_ * n].view(F_, h, w, C).permute(0, 3, 1, 2)          # channels-last rows, 16 bytes into the buffer
    view.copy_(feat)
    assert view.is_contiguous(memory_format=CL) and view.data_ptr() % 16 == 0 and view.data_ptr() != flat.data_ptr()
    c = ops.add_rows_gated(x, view, gate)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_wrapper_refusals_and_dropped_partial_sums(ops):
    from diffusionspatialcontrol_amd import DscLibraryError
    x, feat = _operands(4, 2, 32, 4, 4, seed=12)
    gate = torch.ones(4, device="cuda")
    assert ops.add_rows_gated_supported(x, feat)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.add_rows_gated(*_operands(2, 1, 4, 3, 3, seed=1), torch.ones(2, device="cuda"))                 # 36 halfs per row
    assert not ops.add_rows_gated_supported(*_operands(2, 1, 4, 3, 3, seed=1))
    with pytest.raises(ValueError, match="not a multiple of feat"):
        ops.add_rows_gated(*_operands(3, 2, 32, 4, 4, seed=1), torch.ones(3, device="cuda"))
    with pytest.raises(ValueError, match="channels-last"):
        ops.add_rows_gated(x, feat.contiguous(), gate)                                                        # mismatched layouts
    assert not ops.add_rows_gated_supported(x, feat.contiguous())
    with pytest.raises(ValueError, match="trailing shape"):
        ops.add_rows_gated(x, feat[:, :16], gate)
    big = torch.zeros(5, 32, 4, 4, dtype=torch.float16, device="cuda").contiguous(memory_format=CL)
    with pytest.raises(ValueError, match="overlaps x"):
        ops.add_rows_gated(big[:4], feat, gate, out=big[1:5])                                                 # partial overlap
    with pytest.raises(ValueError, match="gate"):
        ops.add_rows_gated(x, feat, torch.ones(4, device="cuda", dtype=torch.float16))
    with pytest.raises(DscLibraryError):
        ops.add_rows_gated(x, feat, torch.ones(4))                                                            # the gate is read on the device
    with pytest.raises(ValueError, match="out has shape"):
        ops.add_rows_gated(x, feat, gate, out=big)
    for in_place in (True, False):
        dst = x.clone(memory_format=torch.preserve_format) if in_place else torch.empty_like(x)
        ops.attach_gn_partials(dst, ops.GnPartials(torch.zeros(4, 1, 8, 2, 2, device="cuda"), 1, 8, 32, 4, 16))
        assert ops.gn_partials_of(dst) is not None
        ops.add_rows_gated(dst if in_place else x, feat, gate, out=dst)
        assert ops.gn_partials_of(dst) is None
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the UNet keyword
def _unet(cfg=None, seed=0):
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(seed)
    return UNet2DConditionModel(cfg or UNetConfig.tiny()).half().cuda().eval()


@pytest.mark.parametrize("first_attn, hw", [(True, (16, 16)), (True, (9, 11)), (False, (16, 16))])
def test_unet_gated_keyword_equals_the_eager_hook(ops, first_attn, hw):
    """gates all one: the bits of `down_intrablock_additional_residuals` (the kernel's gate-1 result is torch's fp16 add, and both
    routes hand the next GroupNorm a tensor without producer statistics); gates all zero over NaN features: the bits of no
    residuals (at these sizes - below 1024 pixel rows - no producer emits statistics); one row on, one off: each row its own.
    (9, 11): an odd latent size, features of the sizes the batcher computes for it (ceil halving on both sides).  Without
    attention in the first block its add comes after the downsampler, at the next level's size, into a new tensor."""
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNetConfig
    unet = _unet(None if first_attn else dataclasses.replace(UNetConfig.tiny(), transformer_layers_per_block=(0, 1, 1, 0)))
    g = torch.Generator().manual_seed(5)
    H, W = hw
    half = lambda v, k: -(-v // 2 ** k)                                                                # noqa: E731
    lv = [(32, half(H, 0), half(W, 0)), (64, half(H, 1), half(W, 1)), (64, half(H, 2), half(W, 2)), (64, half(H, 3), half(W, 3))]
    if not first_attn:
        lv[0] = (32, lv[1][1], lv[1][2])
    x = torch.randn(1, 4, H, W, generator=g).half().cuda().repeat(2, 1, 1, 1)
    text = torch.randn(2, 77, 64, generator=g).half().cuda()
    t = torch.tensor([300.0, 300.0], device="cuda")
    feats = [(torch.randn((1,) + s, generator=g) * 0.5).half().contiguous(memory_format=CL).cuda() for s in lv]
    full = [f.repeat(2, 1, 1, 1) for f in feats]
    nan = [f * float("nan") for f in feats]
    ones, zeros = torch.ones(2, device="cuda"), torch.zeros(2, device="cuda")
    with torch.no_grad():
        plain = unet(x, t, text).sample
        eager = unet(x, t, text, down_intrablock_additional_residuals=[f.clone() for f in full]).sample
        got1 = unet(x, t, text, down_intrablock_gated=(feats, ones)).sample
        got0 = unet(x, t, text, down_intrablock_gated=(nan, zeros)).sample
        mixed = unet(x, t, text, down_intrablock_gated=(feats, torch.tensor([0.0, 1.0], device="cuda"))).sample
        shared = unet(x, t, text, down_intrablock_gated=(feats, ones), cfg_shared_prefix=True).sample
        with pytest.raises(ValueError, match="mutually exclusive"):
            unet(x, t, text, down_intrablock_gated=(feats, ones), down_intrablock_additional_residuals=full)
        with pytest.raises(ValueError, match="does not fit"):
            unet(x, t, text, down_intrablock_gated=([feats[0][:, :16].contiguous(memory_format=CL)] + feats[1:], ones))
    torch.cuda.synchronize()
    rng = eager.float().abs().max().item()
    assert (eager.float() - plain.float()).abs().max().item() > 1e-2 * rng
    assert torch.equal(got1, eager) and torch.equal(got0, plain)
    assert torch.equal(mixed[0], plain[0]) and torch.equal(mixed[1], eager[1])
    # the shared CFG prefix stays allowed with the keyword (the first add comes after the batch is whole again): the bound of a
    # served run against its own solo run, 2e-3 of the range
    assert (shared.float() - got1.float()).abs().max().item() < 2e-3 * rng


# ----------------------------------------------------------------------------- the batcher
KARRAS = {"scheduler": "karras"}
STEPS, SCALE, FACTOR = 5, 0.8, 0.5


def _serve_one(b, req, **kw):
    fut = b.submit(dict(req, **kw))
    b.run_until_idle()
    return fut.result().float().cpu()


def _adapter(cfg, seed):
    from diffusionspatialcontrol_amd.modules import t2i_adapter as t2i
    torch.manual_seed(seed)
    ad = t2i.T2IAdapter(channels=cfg.block_out_channels, num_res_blocks=2).half()
    sd = {k: v.clone() for k, v in ad.state_dict().items()}
    return ad.cuda().eval(), sd


def _image(seed):
    return torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(seed))


def _latents(seed):
    return torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).half()


def _setup(seed=0):
    import types
    import test_unet_pipeline_gpu as up
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    cfg, unet, sd, text = up._tiny_setup(1, seed=seed)
    state, ids, rs = up._region_state(n_img=1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    base = {"prompt_embeds": text[1:2].cuda(), "negative_prompt_embeds": text[:1].cuda(), "text_input_ids": ids,
            "region_map_state": state, "guidance_scale": 7.5, "sampler_opt": KARRAS}
    common = dict(guidance_scale=7.5, output_type="latent", region_map_state=state, sampler_name="sample_dpmpp_2m",
                  sampler_opt=KARRAS, prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], text_input_ids=ids, width=128,
                  height=128)
    return types.SimpleNamespace(cfg=cfg, sd=sd, text=text, rs=rs, pipe=pipe, base=base, common=common)


@pytest.fixture(scope="module")
def served():
    """one tiny pipeline (the oracle shares its weights): a request served BEFORE setup_model_t2i_adapter, then the adapter, a
    batcher built without the flag and a warm batcher built with it (one bucket of two slots: slot 1 is idle in a solo run)"""
    from diffusionspatialcontrol_amd.modules import t2i_adapter as t2i
    tn = _setup()
    tn.req = dict(tn.base, latents=_latents(11).cuda(), num_inference_steps=4)
    tn.before = _serve_one(tn.pipe.serve(128, 128, max_batch=2, buckets=(2,)).warm(), tn.req)
    tn.ad, tn.ad_sd = _adapter(tn.cfg, 9)
    t2i.setup_model_t2i_adapter(tn.pipe, tn.ad)
    tn.off = tn.pipe.serve(128, 128, max_batch=2, buckets=(2,)).warm()
    tn.b = tn.pipe.serve(128, 128, max_batch=2, buckets=(2,), t2i_adapter=True).warm()
    return tn


def test_flag_off_batcher_is_the_batcher_it_was(served):
    """a batcher built WITHOUT the flag on a pipeline WITH an adapter: bit for bit the request served before
    setup_model_t2i_adapter, and the key is still refused"""
    got = _serve_one(served.off, served.req)
    assert torch.equal(got, served.before), (got - served.before).abs().max().item()
    with pytest.raises(ValueError, match="image_t2i_adapter"):
        served.off.submit(dict(served.req, image_t2i_adapter=_image(10)))
    assert served.off.stats()["adapter_gate_updates"] == 0


def test_flag_on_without_control_image_equals_the_flag_off_batcher(served):
    """the adapter-capable step with every gate 0 computes, bit for bit, what the step without the keyword computes: three
    in-place launches return before they touch anything and the fourth copies its rows.  At this shape (4 batch rows of 2 x 2 at
    the last level, 16 pixel rows; a producer emits GroupNorm statistics from 1024 pixel rows on) no GroupNorm on the path takes
    producer statistics that the adds invalidate, so every launch after them is the launch it was."""
    got = _serve_one(served.b, served.req)
    assert torch.equal(got, served.before), (got - served.before).abs().max().item()
    assert served.b.stats()["adapter_gate_updates"] == 0


@pytest.mark.parametrize("kw", [{"adapter_conditioning_scale": 0.0}, {"adapter_conditioning_factor": 0.0}])
def test_scale_zero_or_factor_zero_equals_no_control_image(served, kw):
    got = _serve_one(served.b, served.req, image_t2i_adapter=_image(10), **kw)
    assert torch.equal(got, served.before)
    st = served.b.stats()
    assert st["captures_after_warm"] == 0 and st["adapter_gate_updates"] == 0


def _oracle_state(ad_sds, images, scales):
    """the oracle's adapter features times their scales, summed over the adapters and duplicated for CFG"""
    acc = None
    for sd, img, s in zip(ad_sds, images, scales):
        f = unet_ref.t2i_adapter_forward(sd, img.half().float())
        acc = [v * s for v in f] if acc is None else [a + v * s for a, v in zip(acc, f)]
    return [torch.cat([v] * 2) for v in acc]


def _relations(what, got, own, ref, plain):
    """(10): d(served, oracle) < 4e-2 range (the bound of test_t2i_adapter_pipeline_vs_oracle for this path); d(served, oracle)
    <= 2 d(pipeline method, oracle) (the served route is no worse an approximation; 2: one seed's noise, as in the IP test); the
    control is live: > 1e-2 range from the same request without it"""
    rng = ref.abs().max().item()
    d_served, d_own = (got - ref).abs().max().item(), (own - ref).abs().max().item()
    print(f"{what}: d(served, oracle) {d_served:.3e}  d(pipeline method, oracle) {d_own:.3e}  d(served, pipeline method) "
          f"{(got - own).abs().max().item():.3e}  d(served, no control) {(got - plain).abs().max().item():.3e}  range {rng:.2f}")
    assert torch.isfinite(got).all()
    assert d_served < 4e-2 * rng, (d_served, rng)
    assert d_served <= 2 * d_own, (d_served, d_own)
    assert (got - plain).abs().max().item() > 1e-2 * rng


def test_adapter_request_against_the_oracle_and_txt2img(served):
    """5 steps, scale 0.8, factor 0.5 (the window: int(6 * 0.5) = 3 model calls), built as
    tests/test_unet_pipeline_gpu.py::test_t2i_adapter_pipeline_vs_oracle builds it.
    Measured on one MI355X (one run): d(served, oracle) 1.292e-01, d(txt2img, oracle) 1.292e-01, d(served, txt2img) 0.000e+00
    (both routes add the same fp16 features with the same rounding, and the tiny step runs the same launches otherwise),
    d(served, no control) 4.438e+00, range 62.51."""
    tn, img, lat = served, _image(10), _latents(11)
    req = dict(tn.base, latents=lat.cuda(), num_inference_steps=STEPS)
    got = _serve_one(tn.b, req, image_t2i_adapter=img, adapter_conditioning_scale=SCALE, adapter_conditioning_factor=FACTOR)
    plain = _serve_one(tn.b, req)
    own = tn.pipe.txt2img(None, num_inference_steps=STEPS, latents=lat.clone(), image_t2i_adapter=img,
                          adapter_conditioning_scale=SCALE, adapter_conditioning_factor=FACTOR, fused=False,
                          **tn.common)[0].float().cpu()
    sig = tn.pipe.get_sigmas(STEPS, KARRAS).half().float().cpu()
    adapter = {"state": _oracle_state([tn.ad_sd], [img], [SCALE]), "limit": int(len(sig) * FACTOR)}
    ref = unet_ref.denoise_loop(tn.sd, tn.cfg, lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), tn.text.float(), tn.rs,
                                7.5, adapter=adapter)
    _relations("txt2img request", got, own, ref, plain)
    assert tn.b.stats()["captures_after_warm"] == 0


def test_img2img_adapter_request_against_the_oracle_and_img2img(served):
    """`image` = 4-channel latents, strength 0.6 of 5 steps: 3 model calls on sigmas[2:] (4 sigmas), the window int(4 * 0.5) = 2
    of them.  The oracle loop takes a start latent and any schedule, so it covers the truncated schedule with an adapter: the
    oracle bound is asserted, against `img2img(fused=False)` as the existing route.
    Measured on one MI355X (one run): d(served, oracle) 1.396e-02, d(img2img, oracle) 1.396e-02, d(served, img2img) 0.000e+00,
    d(served, no control) 2.817e-01, range 5.35."""
    tn, img = served, _image(12)
    lat0 = (_latents(21) * 0.8).half()
    gen = lambda: torch.Generator().manual_seed(33)                                                    # noqa: E731
    req = dict(tn.base, image=lat0.clone().cuda(), strength=0.6, num_inference_steps=STEPS)
    got = _serve_one(tn.b, dict(req, generator=gen()), image_t2i_adapter=img, adapter_conditioning_scale=SCALE,
                     adapter_conditioning_factor=FACTOR)
    plain = _serve_one(tn.b, dict(req, generator=gen()))
    own = tn.pipe.img2img(None, num_inference_steps=STEPS, latents=lat0.clone(), strength=0.6, generator=gen(),
                          image_t2i_adapter=img, adapter_conditioning_scale=SCALE, adapter_conditioning_factor=FACTOR, fused=False,
                          **tn.common)[0].float().cpu()
    sig = tn.pipe.get_sigmas(STEPS, KARRAS).half().float().cpu()
    sched = sig[STEPS - min(int(STEPS * 0.6), STEPS):]
    noise = torch.randn(lat0.shape, generator=gen(), dtype=torch.float16).float()
    adapter = {"state": _oracle_state([tn.ad_sd], [img], [SCALE]), "limit": int(len(sched) * FACTOR)}
    assert len(sched) == 4 and adapter["limit"] == 2
    ref = unet_ref.denoise_loop(tn.sd, tn.cfg, lat0.float() + noise * math.sqrt(float(sched[0]) ** 2 + 1), sched.tolist(),
                                tn.text.float(), tn.rs, 7.5, adapter=adapter)
    _relations("img2img request", got, own, ref, plain)
    assert tn.b.stats()["captures_after_warm"] == 0


def test_mixed_membership_equals_each_request_alone(served):
    """A (control, factor 0.5, 4 steps: a window of int(5 * 0.5) = 2 model calls) starts; its window closes at its third call,
    where nothing else happens: the gate vector is uploaded and nothing is refreshed.  B (no control, exponential schedule, 3
    steps) joins after those 2 steps; C (another image, scale 0.3, factor 1.0) joins the slot A frees.  Each equals its own solo
    served run within 2e-3 of the range (the bound of test_mixed_membership_equals_each_request_alone of the IP tests: both sides
    run the same kernels); no capture after warm().  Measured on one MI355X (one run): 0.0 for all three, range 57.47."""
    b = served.b
    specs = {"A": dict(served.base, latents=_latents(41).cuda(), num_inference_steps=4, image_t2i_adapter=_image(51),
                       adapter_conditioning_factor=0.5),
             "B": dict(served.base, latents=_latents(42).cuda(), num_inference_steps=3, sampler_opt={"scheduler": "exponential"}),
             "C": dict(served.base, latents=_latents(43).cuda(), num_inference_steps=4, guidance_scale=5.0,
                       image_t2i_adapter=_image(53), adapter_conditioning_scale=0.3, adapter_conditioning_factor=1.0)}
    s0 = b.stats()
    futs = {"A": b.submit(dict(specs["A"]))}
    b.step()
    b.step()
    s2 = b.stats()
    b.step()                                             # A's third model call: only its window closes
    s3 = b.stats()
    assert s2["adapter_gate_updates"] == s0["adapter_gate_updates"] + 1 and s2["refreshes"] == s0["refreshes"] + 1
    assert s3["adapter_gate_updates"] == s2["adapter_gate_updates"] + 1 and s3["refreshes"] == s2["refreshes"], (s2, s3)
    futs["B"] = b.submit(dict(specs["B"]))
    for _ in range(3):
        b.step()
    assert b._slots[0] is None                           # A has left
    futs["C"] = b.submit(dict(specs["C"]))
    b.step()
    assert b._slots[0] is not None and b._slots[0].adapter["scale"] == 0.3
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["joins"] - s0["joins"] == 3, st
    got = {n: f.result().float().cpu() for n, f in futs.items()}
    solo = {n: _serve_one(b, dict(s)) for n, s in specs.items()}
    rng = max(v.abs().max().item() for v in solo.values())
    for n in specs:
        d = (got[n] - solo[n]).abs().max().item()
        print(f"request {n}: vs its own solo served run {d:.3e} (range {rng:.2f})")
        assert d < 2e-3 * rng, (n, d, rng)
    no_control = _serve_one(b, {k: v for k, v in specs["A"].items() if "adapter" not in k})
    assert (got["A"] - no_control).abs().max().item() > 1e-2 * rng
    assert b.stats()["captures_after_warm"] == 0


def test_multi_adapter_against_the_oracle_and_txt2img():
    """a MultiAdapter of two tiny adapters, two images, scales [0.6, 0.4]: the relations of the single-adapter test, the oracle's
    features being the same weighted sum of the two adapters' (MultiAdapter.forward).
    Measured on one MI355X (one run): d(served, oracle) 1.467e-01, d(txt2img, oracle) 1.467e-01, d(served, txt2img) 0.000e+00,
    d(served, no control) 4.703e+00, range 81.75."""
    from diffusionspatialcontrol_amd.modules import t2i_adapter as t2i
    tn = _setup(seed=1)
    (ad1, sd1), (ad2, sd2) = _adapter(tn.cfg, 19), _adapter(tn.cfg, 29)
    t2i.setup_model_t2i_adapter(tn.pipe, [ad1, ad2])
    b = tn.pipe.serve(128, 128, max_batch=2, buckets=(2,), t2i_adapter=True).warm()
    imgs, scales, lat = [_image(61), _image(62)], [0.6, 0.4], _latents(63)
    req = dict(tn.base, latents=lat.cuda(), num_inference_steps=STEPS)
    got = _serve_one(b, req, image_t2i_adapter=imgs, adapter_conditioning_scale=scales, adapter_conditioning_factor=FACTOR)
    plain = _serve_one(b, req)
    own = tn.pipe.txt2img(None, num_inference_steps=STEPS, latents=lat.clone(), image_t2i_adapter=imgs,
                          adapter_conditioning_scale=scales, adapter_conditioning_factor=FACTOR, fused=False,
                          **tn.common)[0].float().cpu()
    sig = tn.pipe.get_sigmas(STEPS, KARRAS).half().float().cpu()
    adapter = {"state": _oracle_state([sd1, sd2], imgs, scales), "limit": int(len(sig) * FACTOR)}
    ref = unet_ref.denoise_loop(tn.sd, tn.cfg, lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), tn.text.float(), tn.rs,
                                7.5, adapter=adapter)
    _relations("MultiAdapter request", got, own, ref, plain)
    assert b.stats()["captures_after_warm"] == 0
