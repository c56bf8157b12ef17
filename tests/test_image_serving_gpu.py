"""Finished images in the continuous batcher on the MI355X (`-m gpu`): dsc_image_finish against the reference chain on the CPU
(decode_latents' fp16 `(image / 2 + 0.5).clamp(0, 1)`, NHWC float32, numpy_to_pil's rounding to bytes) over every fp16 value and
at the edges of its launch, and the decode lane of `pipe.serve(..., decode=True)` against the pipeline's own `latent_to_image`,
the eager decoder and the fp32 oracle (oracle/vae_ref.py)."""
import numpy as np
import pytest
import torch

from inputs import FakeTokenizer

pytestmark = pytest.mark.gpu
SIZE, STEPS, OPT = 128, 3, {"scheduler": "karras"}
# the decoder's bound against the fp32 oracle, 1.5e-2 of the image range, in grey levels, plus the rounding
LEVELS = 255 * 1.5e-2 + 0.5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- the kernel
def _chain(img):
    """the reference chain on the CPU, line for line -> (float32 [n, H, W, 3], uint8 [n, H, W, 3]) numpy arrays"""
    image = (img.cpu() / 2 + 0.5).clamp(0, 1)                                # decode_latents, on the fp16 tensor
    f32 = image.permute(0, 2, 3, 1).float().numpy()
    return f32, (f32 * 255).round().astype("uint8")                         # numpy_to_pil


def test_image_finish_every_fp16_value(ops):
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.float16)
    x = x[~torch.isnan(x)]
    assert x.numel() == 63490
    n = 3 * 152 * 144
    img = x.repeat(-(-n // x.numel()))[:n].reshape(1, 3, 152, 144).contiguous()
    f32, u8 = _chain(img)
    got_u8 = ops.image_finish(img.cuda(), "uint8")
    got_f32 = ops.image_finish(img.cuda(), "float32")
    torch.cuda.synchronize()
    assert got_u8.dtype == torch.uint8 and got_f32.dtype == torch.float32 and tuple(got_u8.shape) == (1, 152, 144, 3)
    assert np.array_equal(got_f32.cpu().numpy(), f32)
    assert np.array_equal(got_u8.cpu().numpy(), u8)
    assert np.array_equal(ops.image_finish_torch(img, "uint8").numpy(), u8)          # (the restatement the tools use)


@pytest.mark.parametrize("kind", ["uint8", "float32"])
@pytest.mark.parametrize("n, H, W", [(1, 8, 8), (3, 24, 40), (2, 8, 264)])
def test_image_finish_shapes_and_bounds(ops, n, H, W, kind):
    """one lane, a partial last block, more than one block; sentinel bytes in front of and behind `out` stay as they were"""
    img = (1.5 * torch.randn(n, 3, H, W, generator=torch.Generator().manual_seed(n * H + W))).half()
    f32, u8 = _chain(img)
    dtype = torch.uint8 if kind == "uint8" else torch.float32
    nbytes = n * H * W * 3 * (1 if kind == "uint8" else 4)
    raw = torch.full((64 + nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = raw[64:64 + nbytes].view(dtype).view(n, H, W, 3)
    ret = ops.image_finish(img.cuda(), kind, out=out)
    torch.cuda.synchronize()
    assert ret is out
    assert np.array_equal(out.cpu().numpy(), u8 if kind == "uint8" else f32)
    assert bool((raw[:64] == 0xA5).all()) and bool((raw[64 + nbytes:] == 0xA5).all())


def test_image_finish_refusals(ops):
    ok = torch.zeros(1, 3, 16, 16, dtype=torch.float16, device="cuda")
    for H, W in ((12, 16), (16, 12)):
        with pytest.raises(ValueError, match="multiples of 8"):
            ops.image_finish(torch.zeros(1, 3, H, W, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        ops.image_finish(torch.zeros(1, 16, 16, 3, dtype=torch.float16, device="cuda").permute(0, 3, 1, 2))
    with pytest.raises(ValueError, match="contiguous"):
        ops.image_finish(torch.zeros(1, 3, 16, 32, dtype=torch.float16, device="cuda")[..., ::2])
    with pytest.raises(TypeError, match="fp16"):
        ops.image_finish(ok.float())
    with pytest.raises(ValueError, match=r"\[n, 3, H, W\]"):
        ops.image_finish(torch.zeros(1, 4, 16, 16, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match="kind"):
        ops.image_finish(ok, "int8")
    with pytest.raises(TypeError, match="out must be"):
        ops.image_finish(ok, "uint8", out=torch.zeros(1, 16, 16, 3, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError, match="out must be"):
        ops.image_finish(ok, "float32", out=torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        ops.image_finish(ok, "uint8", out=torch.zeros(1, 3, 16, 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        ops.image_finish(ok, "uint8", out=torch.zeros(1, 16, 8, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="is on"):
        ops.image_finish(ok, "uint8", out=torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="contiguous"):
        ops.image_finish(ok, "uint8", out=torch.zeros(1, 16, 16, 6, dtype=torch.uint8, device="cuda")[..., ::2])


# ----------------------------------------------------------------------------- the decode lane
class _Env:
    pass


@pytest.fixture(scope="module")
def env(ops):
    """tests/test_serving_gpu.py's tiny pipeline with a tiny VAE decoder as its first argument; the decoder's weights as an fp32
    oracle state dict"""
    import test_serving_gpu as sg
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKLDecoder, VaeConfig
    torch.manual_seed(7)
    e = _Env()
    e.cfg, e.vcfg = UNetConfig.tiny(), VaeConfig.tiny()
    unet = UNet2DConditionModel(e.cfg).half().cuda()
    vae = AutoencoderKLDecoder(e.vcfg).half()
    e.sd = {k: v.clone() for k, v in vae.state_dict().items()}
    e.pipe = StableDiffusionPipeline(vae.cuda(), None, FakeTokenizer(), unet, SD15Scheduler())
    e.reqs = [dict(r, num_inference_steps=STEPS + i % 2, guidance_scale=7.5, sampler_opt=OPT)
              for i, r in enumerate(sg._tiny_requests(e.cfg.cross_attention_dim, 4))]
    return e


def _serve(pipe, **kw):
    return pipe.serve(SIZE, SIZE, max_batch=2, buckets=(1, 2), **kw).warm()


def _staggered(b, reqs, types):
    """four requests on two slots, joining at different steps (the same way on every batcher) -> their results"""
    futs = [b.submit(dict(reqs[0], output_type=types[0]))]
    b.step()
    futs.append(b.submit(dict(reqs[1], output_type=types[1])))
    b.step()
    b.step()
    futs.append(b.submit(dict(reqs[2], output_type=types[2])))
    futs.append(b.submit(dict(reqs[3], output_type=types[3])))
    b.run_until_idle()
    return [f.result(timeout=0) for f in futs]


def test_lane_images_equal_latent_to_image(env):
    pipe = env.pipe
    lats = _staggered(_serve(pipe), env.reqs, ["latent"] * 4)
    b = _serve(pipe, decode=True, decode_batch=1)
    types = ["uint8", "np", "latent", "uint8"]
    got = _staggered(b, env.reqs, types)
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["decodes"] == 3 and st["decode_rows"] == 3 and st["leaves"] == 4, st
    for i, (t, g, lat) in enumerate(zip(types, got, lats)):
        if t == "latent":
            assert torch.is_tensor(g) and torch.equal(g, lat), i
        elif t == "uint8":
            ref = np.asarray(pipe.latent_to_image(lat, "pil"))
            assert isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.shape == (SIZE, SIZE, 3)
            assert np.array_equal(g, ref), (i, np.abs(g.astype(int) - ref.astype(int)).max())
            assert ref.std() > 1.0                                            # (an image, not a constant)
        else:
            ref = pipe.latent_to_image(lat, "np")
            assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == (SIZE, SIZE, 3)
            assert np.array_equal(g, ref), (i, np.abs(g - ref).max())
    assert not b.exec.lane.inflight and not b.exec.lane.pending and len(b.exec.lane.free) == len(b.exec.lane.ring)


def test_two_rows_share_one_decode(env, ops):
    """two requests that leave together: one decode of two rows, bit for bit the eager decoder on the same two-row batch followed
    by ops.image_finish, and within the decoder's bound of the fp32 oracle on the same weights"""
    from oracle import vae_ref
    pipe = env.pipe
    pair = [dict(r, num_inference_steps=STEPS) for r in env.reqs[:2]]
    plain = _serve(pipe)
    futs = [plain.submit(dict(r)) for r in pair]
    plain.run_until_idle()
    z = torch.cat([f.result(timeout=0) for f in futs])
    b = _serve(pipe, decode=True, decode_batch=2)
    futs = [b.submit(dict(r, output_type="uint8")) for r in pair]
    b.run_until_idle()
    got = [f.result(timeout=0) for f in futs]
    st = b.stats()
    assert st["decodes"] == 1 and st["decode_rows"] == 2 and st["captures_after_warm"] == 0, st
    with torch.no_grad():
        img = pipe.vae.decode(1 / pipe.vae.config.scaling_factor * z).sample
        eager = ops.image_finish(img, "uint8").cpu().numpy()
        ref = vae_ref.decode_latents(env.sd, z.float().cpu(), env.vcfg.scaling_factor, env.vcfg.norm_num_groups) * 255.0
    for i in range(2):
        assert got[i].shape == (SIZE, SIZE, 3) and np.array_equal(got[i], eager[i]), i
        worst = np.abs(got[i].astype(np.float64) - ref[i]).max()
        inline = np.abs(np.asarray(pipe.latent_to_image(z[i:i + 1], "pil")).astype(np.float64) - ref[i]).max()
        print(f"row {i}: |latent| max {z[i].abs().max().item():.2f}; served uint8 vs the fp32 oracle: {worst:.3f} levels (the inline "
              f"path: {inline:.3f}; bound {LEVELS:.3f}); image std {got[i].std():.1f} levels")
        assert worst <= LEVELS, (i, worst)


def test_pil_request(env):
    Image = pytest.importorskip("PIL.Image")
    b = _serve(env.pipe, decode=True, decode_batch=2)
    f_pil = b.submit(dict(env.reqs[0], output_type="pil"))
    b.run_until_idle()
    f_u8 = b.submit(dict(env.reqs[0], output_type="uint8"))                    # the same request again, alone again: the same bits
    b.run_until_idle()
    img, arr = f_pil.result(timeout=0), f_u8.result(timeout=0)
    assert isinstance(img, Image.Image) and img.size == (SIZE, SIZE) and img.mode == "RGB"
    assert img.tobytes() == arr.tobytes() and np.array_equal(np.asarray(img), arr)


def test_driver_thread_resolves_images(env):
    b = _serve(env.pipe, decode=True, decode_batch=2)
    b.start()
    try:
        futs = [b.submit(dict(r, output_type=t)) for r, t in zip(env.reqs[:3], ("uint8", "np", "uint8"))]
        got = [f.result(timeout=120) for f in futs]
    finally:
        b.stop()
    assert [g.dtype for g in got] == [np.uint8, np.float32, np.uint8] and all(g.shape == (SIZE, SIZE, 3) for g in got)
    lane, st = b.exec.lane, b.stats()
    assert st["decode_rows"] == 3 and 2 <= st["decodes"] <= 3 and st["active"] == 0 and st["queued"] == 0, st
    assert not lane.inflight and not lane.pending and len(lane.free) == len(lane.ring) and not b._done
    assert all(hasattr(f, "dsc_latency_s") and f.dsc_latency_s > 0 for f in futs)


@pytest.mark.parametrize("x, target", [(1.5, 192), (1.25, 160)])
def test_hires_pair_decodes_at_both_sizes(env, x, target):
    """a request with `upscale` gives an image of the target size from the second batcher's lane, one without it an image of
    the base size from the first's; each equals latent_to_image of its latent on a pair without the flag.  `serve_hires`
    builds the 1.5 pair; it refuses 1.25 at 128 on this four-level UNet (20 x 20 latents; its guard on multiples of 8), so that
    pair - the 160 x 160 case - is chained by hand from two batchers, which run any latent size."""
    from diffusionspatialcontrol_amd.modules.serving import HiresPair
    pipe = env.pipe

    def build(slots, **kw):
        if x == 1.5:
            return pipe.serve_hires(SIZE, SIZE, upscale_x=x, max_batch=2, buckets=(1, 2), slots=slots, **kw).warm()
        return HiresPair(pipe.serve(SIZE, SIZE, max_batch=2, buckets=(1, 2), slot=slots[0], **kw),
                         pipe.serve(target, target, max_batch=2, buckets=(1, 2), slot=slots[1], **kw)).warm()

    noise = torch.randn(1, 4, target // 8, target // 8, generator=torch.Generator().manual_seed(9)).half().cuda()
    big = dict(env.reqs[0], num_inference_steps=4, upscale=True, upscale_x=x, upscale_denoising_strength=0.5, hires_latents=noise)
    small = dict(env.reqs[1])

    def run(pair, out_type):
        futs = [pair.submit(dict(big, output_type=out_type)), pair.submit(dict(small, output_type=out_type))]
        pair.run_until_idle()
        return [f.result(timeout=0) for f in futs]

    lat_big, lat_small = run(build((0, 1)), "latent")
    assert tuple(lat_big.shape) == (1, 4, target // 8, target // 8) and tuple(lat_small.shape) == (1, 4, SIZE // 8, SIZE // 8)
    pair = build((2, 3), decode=True)
    got_big, got_small = run(pair, "uint8")
    assert got_big.shape == (target, target, 3) and got_small.shape == (SIZE, SIZE, 3)
    assert np.array_equal(got_big, np.asarray(pipe.latent_to_image(lat_big, "pil")))
    assert np.array_equal(got_small, np.asarray(pipe.latent_to_image(lat_small, "pil")))
    st = pair.stats()
    assert st["handoffs"] == 1 and st["base"]["decodes"] == 1 and st["hires"]["decodes"] == 1, st
    assert st["base"]["captures_after_warm"] == 0 and st["hires"]["captures_after_warm"] == 0, st
