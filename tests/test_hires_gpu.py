"""The hires pass of the continuous batcher on the MI355X (`-m gpu`): dsc_latent_resample_noise against
torch.nn.functional.interpolate and against torch's own fp16 noise composition, and the chained pair of batchers
(pipe.serve_hires) against its parts done by hand, against the pipeline's own txt2img(upscale=True), and under mixed traffic.

The tiny pipeline of the serving tests: 128x128, 8 steps, upscale_x = 1.5 -> 192x192 (latents 16x16 -> 24x24), strength 0.6."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from inputs import FakeTokenizer

pytestmark = pytest.mark.gpu

MODES = [("bilinear", False), ("bilinear", True), ("bicubic", False), ("bicubic", True), ("nearest", False),
         ("nearest-exact", False), ("area", False)]
SHAPES = [((5, 6), (7, 9)), ((16, 16), (19, 24)), ((16, 16), (16, 16)), ((16, 16), (32, 32)), ((64, 64), (76, 71))]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _interp(x, size, mode, aa):
    return F.interpolate(x, size=size, mode=mode, **({"antialias": aa} if mode in ("bilinear", "bicubic") else {}))


_REFS = {}


def _case(n, hw, HW, mode, aa):
    """(src fp16 on the GPU, the CPU reference rounded to fp16), computed once per case and shared"""
    key = (n, hw, HW, mode, aa)
    if key not in _REFS:
        src = torch.randn(n, 4, *hw, generator=_gen(n * 1000 + hw[0] * 10 + HW[1])).half()
        _REFS[key] = (src.cuda(), _interp(src.float(), HW, mode, aa).half())
    return _REFS[key]


def _spacing(ref16):
    """the fp16 spacing at each reference value's magnitude (2^-24 in the subnormal range)"""
    e = torch.floor(torch.log2(ref16.float().abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def _both_store_paths(ops, src, ref, HW, mode, aa):
    numel = ref.numel()
    plain = ops.latent_resample_noise(src, HW, mode, aa)
    buf = torch.full((numel + 16,), 7.0, dtype=torch.float16, device="cuda")
    view = buf[4:4 + numel].view(ref.shape)
    assert view.data_ptr() % 16 == 8
    got = ops.latent_resample_noise(src, HW, mode, aa, out=view)
    torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr() and (buf[:4] == 7.0).all() and (buf[4 + numel:] == 7.0).all()
    assert torch.equal(plain, view)                                      # 16-byte and 2-byte stores: the same bits
    return plain.cpu()


@pytest.mark.parametrize("mode, aa", MODES)
@pytest.mark.parametrize("hw, HW", SHAPES)
@pytest.mark.parametrize("n", [1, 3])
def test_kernel_against_interpolate(ops, n, hw, HW, mode, aa):
    """once into a plain buffer (16-byte stores when W % 8 == 0) and once into an `out=` view offset by 4 halfs (2-byte stores).
    Gather modes and the identity size: equal.  The others: within one fp16 spacing at the reference's magnitude - the only
    difference allowed is the fp32 summation order before the one rounding.

    Where a bicubic sum nearly cancels (|ref| ~ 1e-4: an fp16 spacing of 1e-7) that bound is below the distance of two arbitrary
    fp32 evaluation orders of the sum, so the kernel evaluates it in torch's own order with torch's own weights (csrc/
    latent_resample.hip, modules/latent_resample.py): for both bicubic modes the fp32 value before the rounding is torch's."""
    src, ref = _case(n, hw, HW, mode, aa)
    out = _both_store_paths(ops, src, ref, HW, mode, aa)
    if mode in ("nearest", "nearest-exact") or hw == HW:
        assert torch.equal(out, ref), (mode, hw, HW)
        return
    d = (out.float() - ref.float()).abs()
    sp = _spacing(ref)
    print(f"n {n} {hw}->{HW} {mode}{' aa' if aa else ''}: {int((d > 0).sum())} of {ref.numel()} elements differ from interpolate, "
          f"worst {float((d / sp).max()):.2f} spacings")
    assert (d <= sp).all(), (mode, aa, hw, HW, float((d / sp).max()))


@pytest.mark.parametrize("hw, HW", [((16, 16), (24, 24)), ((5, 6), (7, 9)), ((64, 64), (76, 71))])
@pytest.mark.parametrize("offset", [0, 4])
def test_noise_composition_is_torchs_own(ops, hw, HW, offset):
    """with noise and sigma0: equal to R + noise * s16 computed by torch on fp16 GPU tensors, R the kernel's own no-noise output
    and s16 the fp16 0-dim tensor img2img computes (model_k_diffusion.py: `(sigma_sched[0] ** 2 + 1) ** 0.5`); guard halfs
    around the destination untouched"""
    src, _ = _case(3, hw, HW, "bicubic", False)
    shape = (3, 4) + HW
    numel = 3 * 4 * HW[0] * HW[1]
    for sigma in (14.6171875, 2.37109375, 0.029296875):                   # fp16-representable sigmas
        noise = torch.randn(shape, generator=_gen(int(sigma * 100))).half().cuda()
        sig16 = torch.tensor(sigma, dtype=torch.float16, device="cuda")
        assert float(sig16) == sigma
        s16 = (sig16 ** 2 + 1) ** 0.5
        r = ops.latent_resample_noise(src, HW, "bicubic")
        want = r + noise * s16
        buf = torch.full((numel + 24,), 7.0, dtype=torch.float16, device="cuda")
        view = buf[8 + offset:8 + offset + numel].view(shape)
        ops.latent_resample_noise(src, HW, "bicubic", noise=noise, sigma0=sigma, out=view)
        torch.cuda.synchronize()
        assert float(s16) == ops.noise_scale_f16(sigma)
        assert torch.equal(view, want), (sigma, (view.float() - want.float()).abs().max().item())
        assert (buf[:8 + offset] == 7.0).all() and (buf[8 + offset + numel:] == 7.0).all()


def test_argument_checks_write_nothing(ops):
    from diffusionspatialcontrol_amd import _lib
    src = torch.randn(1, 4, 16, 16, generator=_gen(1)).half().cuda()
    out = torch.full((1, 4, 24, 24), 7.0, dtype=torch.float16, device="cuda")
    noise = torch.zeros(1, 4, 24, 24, dtype=torch.float16, device="cuda")
    with pytest.raises(TypeError):
        ops.latent_resample_noise(src.float(), (24, 24), "bicubic", out=out)                   # wrong dtype
    with pytest.raises(TypeError):
        ops.latent_resample_noise(src, (24, 24), "bicubic", out=out.float())
    with pytest.raises(TypeError):
        ops.latent_resample_noise(src, (24, 24), "bicubic", noise=noise.float(), sigma0=1.0, out=out)
    with pytest.raises(ValueError):
        ops.latent_resample_noise(src, (24, 25), "bicubic", out=out)                           # wrong destination size
    with pytest.raises(ValueError):
        ops.latent_resample_noise(src, (24, 24), "bicubic", noise=noise[..., :23], sigma0=1.0, out=out)
    with pytest.raises(ValueError):
        ops.latent_resample_noise(src, (12, 24), "bicubic")                                    # H < h
    with pytest.raises(ValueError):
        ops.latent_resample_noise(src, (24, 24), "bicubic", noise=noise, out=out)              # noise without sigma0
    with pytest.raises(ValueError):
        ops.latent_resample_noise(src, (24, 24), "lanczos", out=out)
    with pytest.raises(_lib.DscLibraryError):
        ops.latent_resample_noise(src.cpu(), (24, 24), "bicubic")                              # no CPU fallback
    # the entry itself: a null source, H < h and a zero count are DSC_ERR_BAD_ARG before any launch
    from diffusionspatialcontrol_amd.modules.latent_resample import device_taps
    iy, wy = device_taps(16, 24, "bicubic", False, src.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                                # noqa: E731
    lib = _lib.load_library()
    tabs = (p(iy), p(wy), p(iy), p(wy))
    assert lib.dsc_latent_resample_noise(None, None, p(out), 1, 4, 16, 16, 24, 24, *tabs, 1.0, None) == -1
    assert lib.dsc_latent_resample_noise(p(src), None, None, 1, 4, 16, 16, 24, 24, *tabs, 1.0, None) == -1
    assert lib.dsc_latent_resample_noise(p(src), None, p(out), 1, 4, 16, 16, 12, 24, *tabs, 1.0, None) == -1
    assert lib.dsc_latent_resample_noise(p(src), None, p(out), 1, 4, 16, 16, 24, 12, *tabs, 1.0, None) == -1
    assert lib.dsc_latent_resample_noise(p(src), None, p(out), 0, 4, 16, 16, 24, 24, *tabs, 1.0, None) == -1
    assert lib.dsc_latent_resample_noise(p(src), None, p(out), 1, 4, 16, 16, 24, 24, None, p(wy), p(iy), p(wy), 1.0, None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_destination_drops_groupnorm_partials(ops):
    """the contract of every raw-pointer writer in ops (tests/test_output_paths.py): sums attached to the destination describe
    the bytes before the write and must go"""
    src = torch.randn(1, 4, 8, 8, generator=_gen(2)).half().cuda()
    out = torch.zeros(1, 4, 12, 12, dtype=torch.float16, device="cuda")
    ops.attach_gn_partials(out, ops.GnPartials(torch.zeros(4, dtype=torch.float32, device="cuda"), 1, 1, 1, 1, 1))
    assert ops.gn_partials_of(out) is not None
    ops.latent_resample_noise(src, (12, 12), "bilinear", out=out)
    torch.cuda.synchronize()
    assert ops.gn_partials_of(out) is None and out.any()


# ----------------------------------------------------------------------------- the chained pair on the tiny UNet
STEPS = 8
OPT = {"scheduler": "karras"}
X, STRENGTH = 1.5, 0.6                                 # 128x128 -> 192x192; int(8 * 0.6) = 4 steps of the second pass
LAT2 = (1, 4, 24, 24)


@pytest.fixture(scope="module")
def tiny():
    import types
    import test_unet_pipeline_gpu as up
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    cfg, unet, sd, text = up._tiny_setup(1)
    state, ids, rs = up._region_state(n_img=1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    base = {"prompt_embeds": text[1:2].cuda(), "negative_prompt_embeds": text[:1].cuda(), "text_input_ids": ids,
            "region_map_state": state, "guidance_scale": 7.5, "sampler_opt": OPT, "num_inference_steps": STEPS}
    hires = dict(upscale=True, upscale_x=X, upscale_method="bicubic", upscale_denoising_strength=STRENGTH)
    common = dict(guidance_scale=7.5, output_type="latent", region_map_state=state, sampler_opt=OPT, prompt_embeds=text[1:2],
                  negative_prompt_embeds=text[:1], text_input_ids=ids, width=128, height=128, num_inference_steps=STEPS)
    pair = pipe.serve_hires(128, 128, X, max_batch=2, buckets=(1, 2)).warm()
    assert (pair.hires.height, pair.hires.width) == (192, 192)
    sig2 = pipe._schedule(STEPS, OPT, "cpu", torch.float16).float().tolist()[STEPS - int(STEPS * STRENGTH)]
    return types.SimpleNamespace(pipe=pipe, pair=pair, base=base, hires=hires, common=common, sig2=sig2)


def _run(pair, fut):
    pair.run_until_idle()
    return fut.result()


def test_chain_equals_its_parts(tiny, ops):
    """one chained request == the same pair driven by hand: the request served without `upscale`, ops.latent_resample_noise on its
    result with the same noise, and that start row submitted to the second batcher as `image` latents with zero `latents`
    noise (img2img's start then adds 0 * sqrt(sigma_0^2 + 1)).  Two solo runs of the batcher are bit-equal (asserted here
    first), so the comparison is torch.equal"""
    pair = tiny.pair
    lat = torch.randn(1, 4, 16, 16, generator=_gen(50)).half().cuda()
    noise = torch.randn(LAT2, generator=_gen(51)).half().cuda()
    first = _run(pair, pair.submit(dict(tiny.base, latents=lat)))
    again = _run(pair, pair.submit(dict(tiny.base, latents=lat)))
    assert torch.equal(first, again), (first.float() - again.float()).abs().max().item()
    chained = _run(pair, pair.submit(dict(tiny.base, latents=lat, hires_latents=noise, **tiny.hires)))
    assert chained.shape == LAT2 and torch.isfinite(chained).all()
    start = ops.latent_resample_noise(first, LAT2[2:], "bicubic", noise=noise, sigma0=tiny.sig2)
    torch.cuda.synchronize()
    by_hand = _run(pair, pair.hires.submit(dict(tiny.base, image=start, latents=torch.zeros_like(noise), strength=STRENGTH)))
    d = (chained.float() - by_hand.float()).abs().max().item()
    print(f"chained vs its parts by hand: max |diff| {d:.3e}")
    assert torch.equal(chained, by_hand), d
    st = pair.stats()
    assert st["handoffs"] >= 1 and st["base"]["captures_after_warm"] == 0 and st["hires"]["captures_after_warm"] == 0


def test_chain_against_the_pipelines_own_call(tiny):
    """against pipe.txt2img(fused=True, upscale=True) with the same seeded CPU generator.  Yardstick: the distance from that
    call of a route of served pieces that existed before the chain - served txt2img, torch's interpolate, served img2img; the
    chain may be at most twice as far (the routes differ by isolated one-spacing differences in the enlarged latent) or 2e-3 of
    the reference's range, the served-versus-pipeline bound of the other serving tests, whichever is larger"""
    pipe, pair = tiny.pipe, tiny.pair
    ref = pipe.txt2img(None, fused=True, generator=_gen(77), sampler_name="sample_dpmpp_2m", upscale=True, upscale_x=X,
                       upscale_method="bicubic", upscale_denoising_strength=STRENGTH, **tiny.common)[0].float().cpu()
    assert ref.shape == LAT2
    chained = _run(pair, pair.submit(dict(tiny.base, generator=_gen(77), **tiny.hires))).float().cpu()
    g = _gen(77)
    first = _run(pair, pair.submit(dict(tiny.base, generator=g)))
    noise = pipe._randn_like_ref(LAT2, g, first.device, first.dtype)                      # the generator's next draw
    big = F.interpolate(first.float(), size=LAT2[2:], mode="bicubic").to(first.dtype)
    route = _run(pair, pair.hires.submit(dict(tiny.base, image=big, latents=noise, strength=STRENGTH))).float().cpu()
    scale = ref.abs().max().item()
    d_chain, d_route = (chained - ref).abs().max().item(), (route - ref).abs().max().item()
    print(f"vs pipe.txt2img(upscale=True): chained {d_chain:.3e}, served txt2img + interpolate + served img2img {d_route:.3e} "
          f"(range {scale:.2f}); chained vs that route {(chained - route).abs().max().item():.3e}")
    assert d_chain <= max(2 * d_route, 2e-3 * scale), (d_chain, d_route, scale)


def test_mixed_traffic(tiny):
    """max_batch = 2: hires A (Euler a in its second pass), plain B, and hires C arriving mid-run.  Each hires result equals its
    solo chained run on the same pair (same rule as test_chain_equals_its_parts), although alone it runs bucket 1's captured step
    and in company bucket 2's; no capture after warm; two hand-offs"""
    pipe = tiny.pipe
    pair = pipe.serve_hires(128, 128, X, max_batch=2, buckets=(1, 2), slots=(2, 3)).warm()
    lat = [torch.randn(1, 4, 16, 16, generator=_gen(60 + i)).half().cuda() for i in range(3)]
    noise = [torch.randn(LAT2, generator=_gen(70 + i)).half().cuda() for i in range(3)]
    # (Euler a's own noise table is drawn from `generator` at submit; a fresh generator of the same seed repeats it)
    req_a = lambda: dict(tiny.base, latents=lat[0], hires_latents=noise[0], sampler_name_hires="sample_euler_ancestral",  # noqa: E731
                         generator=_gen(81), **tiny.hires)
    req_c = lambda: dict(tiny.base, latents=lat[2], hires_latents=noise[2], num_inference_steps=6,                       # noqa: E731
                         **dict(tiny.hires, upscale_method="nearest-exact", upscale_denoising_strength=0.5))
    fa = pair.submit(req_a())
    fb = pair.submit(dict(tiny.base, latents=lat[1]))
    for _ in range(4):
        pair.step()
    fc = pair.submit(req_c())
    pair.run_until_idle()
    st = pair.stats()
    assert st["handoffs"] == 2 and st["base"]["captures_after_warm"] == 0 and st["hires"]["captures_after_warm"] == 0, st
    assert st["base"]["joins"] == 3 and st["hires"]["joins"] == 2
    got_a, got_b, got_c = fa.result(), fb.result(), fc.result()
    assert got_a.shape == LAT2 and got_c.shape == LAT2 and got_b.shape == (1, 4, 16, 16)
    solo_a = _run(pair, pair.submit(req_a()))
    solo_c = _run(pair, pair.submit(req_c()))
    for name, got, solo in (("A", got_a, solo_a), ("C", got_c, solo_c)):
        d = (got.float() - solo.float()).abs().max().item()
        print(f"mixed traffic, hires request {name}: vs its solo chained run max |diff| {d:.3e}")
        assert torch.isfinite(got).all() and torch.equal(got, solo), (name, d)
    assert not torch.equal(got_a, got_c)
    assert pair.stats()["base"]["captures_after_warm"] == 0 and pair.stats()["hires"]["captures_after_warm"] == 0


def test_threads_drive_both_batchers(tiny):
    """start(): one driver thread per batcher; the future of a hires request resolves with the second pass's output and its
    latency spans both passes"""
    pair = tiny.pair
    lat = torch.randn(1, 4, 16, 16, generator=_gen(50)).half().cuda()
    noise = torch.randn(LAT2, generator=_gen(51)).half().cuda()
    want = _run(pair, pair.submit(dict(tiny.base, latents=lat, hires_latents=noise, **tiny.hires)))
    pair.start()
    try:
        fut = pair.submit(dict(tiny.base, latents=lat, hires_latents=noise, **tiny.hires))
        got = fut.result(timeout=60)
    finally:
        pair.stop()
    assert torch.equal(got, want)
    assert fut.dsc_latency_s >= fut.dsc_first_pass_s > 0.0
