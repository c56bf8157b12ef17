"""Pixel inputs on the encode lane of the continuous batcher (modules/serving/encode_lane.py), the host half: the eager chains the
two kernels replace (ops.image_prepare_torch, ops.latent_start_torch - the GPU tests' references) against the pipeline's own lines,
the scalar each start latent is formed with, the constructor's refusals, the buckets, and the queue logic against a recording
executor whose lane events the test controls."""
import dataclasses
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from inputs import FakeTokenizer
from serving_fakes import RecordingExec

from diffusionspatialcontrol_amd import ops
from diffusionspatialcontrol_amd.modules.serving import ServingBatcher, encode_buckets, step_launch

S = 77
H = W = 128
LAT = torch.zeros(1, 4, 16, 16).half()
MIL = torch.ones(1, 4, 16, 16).half()
MASK = torch.ones(1, 1, H, W)
PIXELS = torch.zeros(1, 3, H, W)
PLAIN_STATS = {"captures", "joins", "leaves", "bucket_switches", "steps", "refreshes", "linear_transitions", "handoffs",
               "adapter_gate_updates", "control_steps", "control_gate_updates", "captures_after_warm", "queued", "active", "bucket"}


def _pipe(in_channels=4, vae="full"):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKL, AutoencoderKLDecoder, VaeConfig
    torch.manual_seed(0)
    unet = UNet2DConditionModel(dataclasses.replace(UNetConfig.tiny(), in_channels=in_channels)).half()
    v = {"full": AutoencoderKL, "decoder": AutoencoderKLDecoder}[vae](VaeConfig.tiny()).half() if vae else None
    return StableDiffusionPipeline(v, None, FakeTokenizer(), unet, SD15Scheduler())


@pytest.fixture(scope="module")
def pipe():
    return _pipe()


@pytest.fixture(scope="module")
def pipe9():
    return _pipe(9)


# ----------------------------------------------------------------------------- the eager chains
def test_image_prepare_torch_is_the_pipelines_chain_on_bytes(pipe):
    """a PIL image and a PIL mask: `_image_tensor`, `init * (mask < 0.5)`, the VAE's `.to(fp16)`, `F.interpolate(mask, (h, w))`"""
    from PIL import Image
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (24, 40, 3), generator=g, dtype=torch.uint8)
    img[0, :16, 0] = torch.arange(16, dtype=torch.uint8) * 17                      # (0 and 255 are in)
    mask = torch.randint(0, 256, (24, 40), generator=g, dtype=torch.uint8)
    mask[0, :4] = torch.tensor([127, 128, 0, 255], dtype=torch.uint8)
    init = pipe._image_tensor(Image.fromarray(img.numpy()), 24, 40)
    m = pipe._image_tensor(Image.fromarray(mask.numpy(), "L"), 24, 40, mask=True)
    got = ops.image_prepare_torch(img, mask, rep=4)
    assert torch.equal(got[0], init[0].half())
    assert torch.equal(got[1].view(torch.int16), (init * (m < 0.5))[0].half().view(torch.int16))
    assert torch.equal(got[2], F.interpolate(m, size=(3, 5))[0].half().expand(4, 3, 5))
    assert m[0, 0, 0, :4].tolist() == [0.0, 1.0, 0.0, 1.0]                         # the flip is between 127 and 128
    only = ops.image_prepare_torch(img)
    assert torch.equal(only[0], got[0]) and only[1] is None and only[2] is None


def test_image_prepare_torch_is_the_pipelines_chain_on_floats(pipe):
    g = torch.Generator().manual_seed(4)
    img = torch.rand(1, 3, 16, 24, generator=g) * 2 - 1
    mask = torch.rand(1, 1, 16, 24, generator=g)
    mask[0, 0, 0, :3] = torch.tensor([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))])
    init = pipe._image_tensor(img, 16, 24)
    m = pipe._image_tensor(mask, 16, 24, mask=True)
    got = ops.image_prepare_torch(img[0], mask[0, 0], rep=1)
    assert torch.equal(got[0], init[0].half())
    assert torch.equal(got[1].view(torch.int16), (init * (m < 0.5))[0].half().view(torch.int16))
    assert torch.equal(got[2], F.interpolate(m, size=(2, 3))[0].half())
    assert got[2].shape == (1, 2, 3) and m[0, 0, 0, :3].tolist() == [1.0, 0.0, 1.0]
    neg = (got[1].view(torch.int16) == -32768)                                     # -0.0: a negative pixel under a repainted mask
    assert neg.any() and torch.equal(neg, ((init[0] < 0) & (m[0] >= 0.5)))


class _FixedVae:
    """a VAE whose encoder returns these moments: what `_encode_vae_image` needs of one"""

    def __init__(self, moments, scaling):
        from diffusionspatialcontrol_amd.modules.vae_decoder import DiagonalGaussianDistribution
        self._dist = lambda: DiagonalGaussianDistribution(moments)
        self.config = types.SimpleNamespace(scaling_factor=scaling)
        self.device, self.dtype = moments.device, moments.dtype

    def encode(self, x):
        return types.SimpleNamespace(latent_dist=self._dist())


@pytest.mark.parametrize("kind", ["img2img", "inpaint", "inpaint_max", "masked"])
def test_latent_start_torch_is_the_pipelines_chain(pipe, monkeypatch, kind):
    """DiagonalGaussianDistribution.sample x scaling through `_encode_vae_image`, then prepare_image's line (img2img) or
    prepare_latents_inpating's branches, fp16 CPU tensors, one seeded generator; and the kernel's arithmetic with start_form's
    scalar (fp32 operations, fp16 where the chain holds a tensor) gives the same bits"""
    g = torch.Generator().manual_seed(11)
    moments = (torch.randn(1, 8, 5, 3, generator=g) * 2).half()
    moments[0, 4, 0, :3] = torch.tensor([-40.0, 30.0, 20.0]).half()                # the clamp at both ends
    scaling = 0.18215
    monkeypatch.setattr(pipe, "vae", _FixedVae(moments, scaling))
    monkeypatch.setattr(pipe, "vae_scale_factor", 8)
    sig0 = torch.tensor(3.3).half()
    pixels = torch.zeros(1, 3, 40, 24)
    if kind == "img2img":
        lat = pipe._encode_vae_image(pixels, torch.Generator().manual_seed(5))
        gen = torch.Generator().manual_seed(5)
        eps = torch.randn(lat.shape, generator=gen, dtype=torch.float16)
        noise = pipe._randn_like_ref(lat.shape, gen, torch.device("cpu"), torch.float16)
        start = lat + noise * (sig0 ** 2 + 1) ** 0.5                               # executor.prepare_image's line (:647)
    elif kind == "masked":
        lat, start, noise = pipe._encode_vae_image(pixels, torch.Generator().manual_seed(5)), None, None
        eps = torch.randn(lat.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float16)
    else:
        start, noise, lat = pipe.prepare_latents_inpating(1, 4, 40, 24, torch.float16, torch.device("cpu"),
                                                          torch.Generator().manual_seed(5), None, image=pixels, sigma=sig0,
                                                          is_strength_max=kind == "inpaint_max", return_noise=True,
                                                          return_image_latents=True)
        gen = torch.Generator().manual_seed(5)
        eps = torch.randn(lat.shape, generator=gen, dtype=torch.float16)
        assert torch.equal(noise, torch.randn(lat.shape, generator=gen, dtype=torch.float16))
    got_lat, got_start = ops.latent_start_torch(moments, eps, noise, scaling, kind, sig0)
    assert torch.equal(got_lat, lat) and torch.isfinite(lat).all()
    assert (got_start is None and start is None) or torch.equal(got_start, start)
    form, coef = ops.start_form(kind, sig0)
    assert form == {"img2img": "add", "inpaint": "add", "inpaint_max": "scale", "masked": "none"}[kind]
    if start is not None:                                                          # what the kernel computes with that scalar
        scaled = (noise.float() * torch.tensor(coef, dtype=torch.float32)).half()
        mine = (lat.float() + scaled.float()).half() if form == "add" else scaled
        assert torch.equal(mine, start)
    assert ops.start_form("inpaint", sig0, given_latents=True) == ops.start_form("inpaint_max", sig0)
    with pytest.raises(ValueError, match="kind"):
        ops.start_form("txt2img", sig0)


# ----------------------------------------------------------------------------- construction
class LaneExec(RecordingExec):
    """RecordingExec plus the encode lane's interface, with events the test completes: `dispatch_encodes` marks a request's rows
    sent and gives it an event that is not done; `complete(name)` finishes it; `encode_wait` logs the wait and finishes it"""

    def __init__(self, encode_batch=2, **kw):
        super().__init__(**kw)
        self.encode_batch = encode_batch
        self.sent, self.waits, self.launches = [], [], []

    def prepare_image(self, r):
        super().prepare_image(r)
        if r.kind == "inpaint_unet":
            r.extra = ("extra", r.req.get("name"))

    def prepare_encode(self, r):
        self._prepared(r, "encode:" + r.kind)
        if r.kind == "inpaint_unet":
            r.extra = ("extra", r.req.get("name"))
        elif r.kind == "inpaint":
            r.known = {"image": 1, "noise": 2, "mask": 3}

    def ensure_encode(self):
        return int(self._ensure("encode"))

    def dispatch_encodes(self, requests):
        rows = 0
        for r in requests:
            rows += r.enc.rows - r.enc.sent
            r.enc.sent = r.enc.rows
            r.enc.ev = types.SimpleNamespace(done=False)
            self.sent.append((r.req.get("name"), r.enc.roles))
        self._event("dispatch_encodes", [r.req.get("name") for r in requests])
        return -(-rows // self.encode_batch), rows

    def encode_ready(self, r):
        return r.enc.ev is not None and r.enc.ev.done

    def encode_wait(self, r):
        self.waits.append(r.req.get("name"))
        r.enc.ev.done = True

    def transition(self, n_src, n_dst, recs, known=None, extras=None):
        self.launches.append(step_launch(recs, known, extras))
        super().transition(n_src, n_dst, recs, known)


def _req(name, steps=4, **kw):
    emb = torch.randn(2, S, 64, generator=torch.Generator().manual_seed(len(name) + steps))
    r = {"name": name, "prompt_embeds": emb[1:2].half(), "negative_prompt_embeds": emb[0:1].half(),
         "num_inference_steps": steps, "guidance_scale": 7.5, "sampler_opt": {"scheduler": "karras"}}
    r.update(kw)
    return r


def _batcher(pipe, **kw):
    ex = LaneExec(encode_batch=kw.get("encode_batch", 2))
    return ServingBatcher(pipe, H, W, executor=ex, **kw), ex


@pytest.mark.parametrize("vae", [None, "decoder"])
def test_encode_needs_an_encoder(vae):
    bare = _pipe(vae=vae)
    with pytest.raises(ValueError, match="encode=True.*without a VAE encoder"):
        ServingBatcher(bare, H, W, executor=LaneExec(), encode=True)
    with pytest.raises(ValueError, match="encode=True.*without a VAE encoder"):
        bare.serve(H, W, encode=True)
    with pytest.raises(ValueError, match="encode=True.*without a VAE encoder"):
        bare.serve_hires(H, W, 1.5, encode=True)
    ServingBatcher(bare, H, W, executor=LaneExec())                                # without the flag such a pipeline serves


@pytest.mark.parametrize("bad", [0, -1, 5, 2.0, True, None, "2"])
def test_encode_batch_range(pipe, bad):
    with pytest.raises(ValueError, match="encode_batch"):
        ServingBatcher(pipe, H, W, max_batch=4, buckets=(1, 2, 4), executor=LaneExec(), encode=True, encode_batch=bad)


def test_encode_batch_bounds_are_inclusive_and_buckets(pipe):
    for ok in (1, 4):
        b = ServingBatcher(pipe, H, W, max_batch=4, buckets=(1, 2, 4), executor=LaneExec(), encode=True, encode_batch=ok)
        assert b.encode and b.encode_batch == ok
    assert encode_buckets(1) == (1,) and encode_buckets(2) == (1, 2) and encode_buckets(3) == (1, 2, 3)
    assert encode_buckets(8) == (1, 2, 4, 8)


def test_stats_keys_only_with_the_flag(pipe):
    plain, _ = _batcher(pipe)
    lane, _ = _batcher(pipe, encode=True)
    assert not plain.encode and set(plain.stats()) == PLAIN_STATS
    assert set(lane.stats()) - set(plain.stats()) == {"encodes", "encode_rows"}
    assert lane.stats()["encodes"] == 0 and lane.stats()["encode_rows"] == 0


def test_flagless_batcher_prepares_pixels_inline(pipe):
    b, ex = _batcher(pipe, max_batch=2, buckets=(1, 2))
    fut = b.submit(_req("P", image=PIXELS, strength=0.5))
    assert ex.prepared == [("img2img", "P")]
    b.run_until_idle()
    assert fut.done() and not ex.sent and not ex.waits and set(b.stats()) == PLAIN_STATS
    assert not any(e[0] in ("dispatch_encodes",) or (e[0] == "ensure" and e[2] == "encode") for e in ex.events)


# ----------------------------------------------------------------------------- queue logic
def test_encoding_head_waits_and_is_not_overtaken(pipe):
    """A (latents) runs; P (pixels) is queued behind it and then L (latents) behind P: while P's encode has not completed, a slot
    is free and neither P nor L is admitted, and A keeps stepping; when it completes both join, P first"""
    b, ex = _batcher(pipe, max_batch=4, buckets=(1, 2, 4), encode=True)
    fa = b.submit(_req("A", steps=8, latents=LAT))
    assert b.step() and b.stats()["active"] == 1
    fp = b.submit(_req("P", steps=4, image=PIXELS, strength=1.0))
    fl = b.submit(_req("L", steps=4, image=LAT, strength=1.0))
    assert ("encode:img2img", "P") in ex.prepared and ("img2img", "L") in ex.prepared     # L takes the inline path
    for _ in range(3):
        assert b.step()
        st = b.stats()
        assert st["active"] == 1 and st["queued"] == 2 and not ex.waits
    assert ex.sent == [("P", ("image",))] and b.stats()["encodes"] == 1 and b.stats()["encode_rows"] == 1
    assert b.stats()["steps"] == 4                                                  # the member's step went on meanwhile
    head = b._queue[0]
    head.enc.ev.done = True
    assert b.step()
    st = b.stats()
    assert st["active"] == 3 and st["queued"] == 0 and st["joins"] == 3
    loads = [e[2] for e in ex.events if e[0] == "load"]
    assert loads == ["A", "P", "L"]
    b.run_until_idle()
    assert fa.done() and fp.done() and fl.done() and not ex.waits
    assert b.stats()["encodes"] == 1 and head.enc is None                           # (its draws are released when it leaves)


def test_idle_batcher_waits_for_the_encoding_head(pipe):
    """nobody steps and the head is still encoding: the step waits for its event and admits it instead of reporting idle, so
    run_until_idle never returns with a request queued"""
    b, ex = _batcher(pipe, max_batch=2, buckets=(1, 2), encode=True)
    fut = b.submit(_req("P", steps=3, image=PIXELS, strength=1.0))
    assert b.stats()["queued"] == 1
    assert b.step() is True
    assert ex.waits == ["P"] and b.stats()["active"] == 1 and b.stats()["queued"] == 0
    b.run_until_idle()
    assert fut.done() and b.stats()["queued"] == 0 and ex.waits == ["P"]
    fut2 = b.submit(_req("Q", steps=3, image=PIXELS, mask_image=MASK, strength=0.7))
    b.run_until_idle()
    assert fut2.done() and ex.waits == ["P", "Q"] and ("encode:inpaint", "Q") in ex.prepared


def test_txt2img_and_latent_inputs_do_not_touch_the_lane(pipe):
    b, ex = _batcher(pipe, max_batch=2, buckets=(1, 2), encode=True)
    futs = [b.submit(_req("T", latents=LAT)), b.submit(_req("L", image=LAT, strength=0.5)),
            b.submit(_req("M", image=LAT, mask_image=MASK))]
    b.run_until_idle()
    assert all(f.done() for f in futs) and not ex.sent and not ex.waits
    assert b.stats()["encodes"] == 0 and b.stats()["encode_rows"] == 0 and "encode" not in ex.captured


def test_given_latents_of_another_dtype_stay_inline(pipe):
    """prepare_latents_inpating multiplies given `latents` in their own dtype: an inpainting request with fp32 latents keeps the
    inline path (and its bits); img2img converts them first on both paths, so it takes the lane"""
    b, ex = _batcher(pipe, max_batch=4, buckets=(1, 2, 4), encode=True)
    futs = [b.submit(_req("F", image=PIXELS, mask_image=MASK, latents=LAT.float())),
            b.submit(_req("H", image=PIXELS, mask_image=MASK, latents=LAT)),
            b.submit(_req("I", image=PIXELS, strength=0.5, latents=LAT.float()))]
    b.run_until_idle()
    assert all(f.done() for f in futs)
    assert ("inpaint", "F") in ex.prepared and ("encode:inpaint", "H") in ex.prepared and ("encode:img2img", "I") in ex.prepared
    assert [name for name, _ in ex.sent] == ["H", "I"]


def test_nine_channel_requests_count_their_rows(pipe9):
    """a request of an `inpaint_unet=True` batcher is two lane rows (the image and the masked image), one with
    `masked_image_latents`, none when `image` is latents"""
    b, ex = _batcher(pipe9, max_batch=4, buckets=(1, 2, 4), encode=True, encode_batch=2, inpaint_unet=True)
    assert set(b.stats()) == PLAIN_STATS | {"cat_transitions", "encodes", "encode_rows"}
    futs = [b.submit(_req("two", image=PIXELS, mask_image=MASK)),
            b.submit(_req("one", image=PIXELS, mask_image=MASK, masked_image_latents=MIL)),
            b.submit(_req("none", image=LAT, mask_image=MASK, masked_image_latents=MIL))]
    b.run_until_idle()
    assert all(f.done() for f in futs)
    assert ex.sent == [("two", ("image", "masked")), ("one", ("image",))]
    assert b.stats()["encode_rows"] == 3 and b.stats()["encodes"] == 2              # three rows, two per encode
    assert ("inpaint_unet", "none") in ex.prepared and set(ex.launches) == {"cat"}


def test_hires_pair_gives_the_lane_to_the_base_batcher_only(pipe, monkeypatch):
    from diffusionspatialcontrol_amd.modules.serving import batcher as batcher_module
    monkeypatch.setattr(batcher_module, "_GraphExecutor", lambda b: LaneExec())   # (no device in this test)
    pair = pipe.serve_hires(H, W, 1.5, max_batch=2, buckets=(1, 2), encode=True, encode_batch=2)
    assert pair.base.encode and pair.base.encode_batch == 2 and not pair.hires.encode
    assert "encodes" in pair.base._stats and "encodes" not in pair.hires._stats
    plain = pipe.serve_hires(H, W, 1.5, max_batch=2, buckets=(1, 2))
    assert not plain.base.encode and not plain.hires.encode
