"""img2img / inpainting requests in the continuous-batching scheduler (modules/serving/) on the host, against a fake
executor: schedule truncation by `strength`, the known-region records handed to the per-row step, which launch a transition
takes, and the submit-time rejections of the image keys."""
import pytest
import torch

from inputs import FakeTokenizer
from serving_fakes import RecordingExec

from diffusionspatialcontrol_amd import ops
from diffusionspatialcontrol_amd.modules import sampling
from diffusionspatialcontrol_amd.modules.serving import ServingBatcher

S = 77


class FakeImgExec(RecordingExec):
    """a request's result is what was applied to it: no guidance, and the known-region record each entry was launched with"""
    step_keys = tuple(k for k in RecordingExec.step_keys if k != "guidance")
    applied_known = True

    def result(self, r, h):
        return self.applied[id(r)]


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
MASK = torch.ones(1, 1, 128, 128)


def _batcher(pipe, **kw):
    ex = FakeImgExec()
    return ServingBatcher(pipe, 128, 128, executor=ex, **kw), ex


@pytest.mark.parametrize("steps", [4, 8, 25])
@pytest.mark.parametrize("strength", [1.0, 0.6, 0.3])
@pytest.mark.parametrize("kind", ["img2img", "inpaint"])
def test_truncated_schedule_sequences(pipe, steps, strength, kind):
    """sigma, (a, b, c), c_in, t and time-embedding index sequences of an image request are those of
    pipe._schedule(...)[t_start:], t_start as img2img computes it (reference :637-638); the first step has c = 0"""
    b, ex = _batcher(pipe, max_batch=2, buckets=(1, 2))
    extra = {"mask_image": MASK} if kind == "inpaint" else {}
    fut = b.submit(_req("R", steps=steps, image=LAT, strength=strength, **extra))
    b.run_until_idle()
    applied = fut.result()
    init = min(int(steps * strength), steps)
    t_start = max(steps - init, 0)
    sig = pipe._schedule(steps, {"scheduler": "karras"}, "cpu", torch.float16).float().tolist()[t_start:]
    coeffs = sampling.dpmpp_2m_coefficients(sig)
    kdm = pipe.k_diffusion_model
    assert len(coeffs) == init and coeffs[0][2] == 0.0 and len(applied) == init + 1
    c_in0, _, t0 = kdm.step_scalars(sig[0])
    assert applied[0][:5] == ("join", c_in0, float(t0), sig[0], ("temb", "R", 0))
    for i, (a, b_, c) in enumerate(coeffs):
        if i + 1 < init:
            c_in_n, _, t_n = kdm.step_scalars(sig[i + 1])
            exp = ("step", i, sig[i], a, b_, c, c_in_n, float(t_n), ("temb", "R", i + 1))
        else:
            exp = ("step", i, sig[i], a, b_, c, 0.0, 0.0, None)
        assert applied[i + 1][:9] == exp, i
    assert ex.prepared == [(kind, "R")]


def test_inpainting_records_and_launch_choice(pipe):
    """an inpainting request's first transition is a JOIN on the plain launch (no blend); its step k carries
    blend_now == (k >= 1) and blend_next == (not leaving) with its three rows; slots of other requests carry no record; a
    transition in which no inpainting slot steps takes the plain launch"""
    b, ex = _batcher(pipe, max_batch=4, buckets=(1, 2, 4))
    ft = b.submit(_req("T", steps=6, latents=LAT))
    b.step()
    fi = b.submit(_req("I", steps=3, image=LAT, mask_image=MASK))
    fm = b.submit(_req("M", steps=5, image=LAT, strength=0.6))
    b.run_until_idle()
    kinds = [c[0] for c in ex.calls]
    assert kinds[0] == "rows" and kinds[1] == "rows"                 # T joins; then I and M join while T steps
    assert ex.calls[1][3][1]["mode"] == ops.ROW_JOIN and ex.calls[1][3][1]["req"].req["name"] == "I"
    steps_i = [a for a in fi.result() if a[0] == "step"]
    assert len(steps_i) == 3 and fi.result()[0][0] == "join" and fi.result()[0][-1] is None
    for k, a in enumerate(steps_i):
        kn = a[-1]
        assert kn["blend_now"] == (k >= 1) and kn["blend_next"] == (k < 2), (k, kn)
        assert (kn["image"], kn["noise"], kn["mask"]) == (("image", "I"), ("noise", "I"), ("mask", "I"))
    assert kinds[2:5] == ["known"] * 3 and set(kinds[5:]) == {"rows"}  # once I has left, the plain launch again
    for call in ex.calls[2:5]:
        for rec, kn in zip(call[3], call[4]):
            name = None if rec["req"] is None else rec["req"].req["name"]
            assert (kn is not None) == (name == "I" and rec["mode"] == ops.ROW_STEP)
    assert all(a[-1] is None for a in ft.result() + fm.result())
    assert len([a for a in fm.result() if a[0] == "step"]) == 3         # int(5 * 0.6) steps
    st = b.stats()
    assert st["joins"] == 3 and st["leaves"] == 3


def test_batch_without_inpainting_never_takes_the_known_launch(pipe):
    b, ex = _batcher(pipe, max_batch=4, buckets=(1, 2, 4))
    futs = [b.submit(_req("A", steps=3, latents=LAT)), b.submit(_req("B", steps=4, image=LAT, strength=0.5)),
            b.submit(_req("C", steps=2, latents=LAT))]
    b.run_until_idle()
    assert all(f.done() for f in futs) and {c[0] for c in ex.calls} == {"rows"}
    assert ex.prepared == [("txt2img", "A"), ("img2img", "B"), ("txt2img", "C")]


def test_known_rows_are_released_when_the_request_leaves(pipe):
    b, ex = _batcher(pipe, max_batch=2, buckets=(1, 2))
    b.submit(_req("I", steps=2, image=LAT, mask_image=MASK))
    b.step()
    r = b._slots[0]
    assert r.known is not None
    b.run_until_idle()
    assert r.known is None


class _NineChannels:
    def __init__(self, pipe):
        self.pipe = pipe

    def __enter__(self):
        self.old = self.pipe.unet.config.in_channels
        self.pipe.unet.config.in_channels = 9

    def __exit__(self, *exc):
        self.pipe.unet.config.in_channels = self.old


@pytest.mark.parametrize("bad, match", [
    ({"image": LAT, "strength": 0.0}, "strength"),
    ({"image": LAT, "strength": 1.5}, "strength"),
    ({"image": LAT, "strength": -0.2}, "strength"),
    ({"image": LAT, "strength": 0.1}, "strength"),                        # int(4 * 0.1) == 0 steps
    ({"strength": 0.5}, "strength"),                                      # txt2img has no strength
    ({"mask_image": MASK}, "mask_image"),
    ({"image": torch.zeros(1, 4, 32, 32).half()}, "image"),
    ({"image": torch.zeros(1, 3, 256, 256)}, "image"),
    ({"image": LAT, "mask_image": torch.ones(1, 1, 64, 64)}, "mask_image"),
    ({"image": torch.zeros(1, 3, 128, 128)}, "VAE"),                      # pixels, but the pipeline has no encoder
    ({"image": LAT, "mask_image": MASK, "padding_mask_crop": 8}, "padding_mask_crop"),
    ({"image": LAT, "upscale": True}, "upscale"),
])
def test_image_key_rejections(pipe, bad, match):
    b, ex = _batcher(pipe)
    with pytest.raises(ValueError, match=match):
        b.submit(_req("X", **bad))
    f = b.submit(_req("ok", latents=LAT))                                   # a plain txt2img request next to it is accepted
    b.run_until_idle()
    assert f.done() and ex.prepared == [("txt2img", "ok")]


def test_nine_channel_unet_rejects_mask(pipe):
    b, ex = _batcher(pipe)
    with _NineChannels(pipe):
        with pytest.raises(ValueError, match="mask_image"):
            b.submit(_req("X", image=LAT, mask_image=MASK))
    f = b.submit(_req("ok", latents=LAT))
    b.run_until_idle()
    assert f.done()


def test_mask_at_latent_size_is_accepted(pipe):
    b, ex = _batcher(pipe)
    f = b.submit(_req("I", steps=2, image=LAT, mask_image=torch.ones(1, 1, 16, 16)))
    b.run_until_idle()
    assert f.done() and ex.prepared == [("inpaint", "I")]
