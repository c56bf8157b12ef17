"""IP-Adapter requests in the continuous batcher on the host (modules/serving/ against a fake executor): the submit-time
refusals of the image-prompt keys, the default scale, the row scales `refresh` writes, the hires pair, stale batchers, and the
C entry (declared, exported, validating its arguments without a GPU)."""
import ctypes
import subprocess

import pytest
import torch

from inputs import FakeTokenizer
from serving_fakes import RecordingExec

import diffusionspatialcontrol_amd as dsc
from diffusionspatialcontrol_amd import _lib, build as dsc_build, ops
from diffusionspatialcontrol_amd.modules.serving import HiresPair, ServingBatcher, _GraphExecutor

S, EMB = 77, 48


FakeExec = RecordingExec


def _pipe(adapters=()):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    unet = UNet2DConditionModel(UNetConfig.tiny()).half()
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    if adapters:
        pipe.load_ip_adapter([_adapter(pipe.unet, kind) for kind in adapters])
    return pipe


def _adapter(unet, kind):
    from diffusionspatialcontrol_amd.modules import u_net_condition_modify as um
    ctx = unet.config.cross_attention_dim
    cross = [m for pre in ("down_blocks", "up_blocks", "mid_block") for n, m in unet.named_modules()
             if isinstance(m, um.Attention) and m.is_cross_attention and n.startswith(pre)]
    ip = {}
    for i, m in enumerate(cross):
        ip[f"{2 * i + 1}.to_k_ip.weight"] = torch.zeros(m.inner_dim, ctx)
        ip[f"{2 * i + 1}.to_v_ip.weight"] = torch.zeros(m.inner_dim, ctx)
    if kind == "full":                                # 257 tokens
        full = um.IPAdapterFullImageProjection(EMB, ctx)
        proj = {"proj.0.weight": full.ff.net[0]["proj"].weight.data, "proj.0.bias": full.ff.net[0]["proj"].bias.data,
                "proj.2.weight": full.ff.net[2].weight.data, "proj.2.bias": full.ff.net[2].bias.data,
                "proj.3.weight": full.norm.weight.data, "proj.3.bias": full.norm.bias.data}
    else:                                             # the standard 4-token projection
        proj = {"proj.weight": torch.zeros(4 * ctx, EMB), "proj.bias": torch.zeros(4 * ctx), "norm.weight": torch.ones(ctx),
                "norm.bias": torch.zeros(ctx)}
    return {"image_proj": proj, "ip_adapter": ip}


def _req(name, steps=3, **kw):
    emb = torch.randn(2, S, 64, generator=torch.Generator().manual_seed(len(name) + steps))
    r = {"name": name, "prompt_embeds": emb[1:2].half(), "negative_prompt_embeds": emb[0:1].half(),
         "num_inference_steps": steps, "guidance_scale": 7.5, "sampler_opt": {"scheduler": "karras"}}
    r.update(kw)
    return r


def _embeds(n=1):
    return [torch.zeros(2, 1, EMB).half() for _ in range(n)]


@pytest.fixture(scope="module")
def pipe1():
    return _pipe(("standard",))


def _batcher(pipe, **kw):
    ex = FakeExec()
    return ServingBatcher(pipe, 128, 128, executor=ex, **dict(dict(max_batch=2, buckets=(2,)), **kw)), ex


@pytest.mark.parametrize("bad, match", [
    ({"ip_adapter_image_embeds": _embeds(2)}, "one tensor per loaded IP-Adapter"),                    # list length
    ({"ip_adapter_image_embeds": _embeds(1)[0]}, "one tensor per loaded IP-Adapter"),                 # not a list
    ({"ip_adapter_image_embeds": [torch.zeros(1, 1, EMB).half()]}, "negative; positive"),            # dim 0 is not 2
    ({"ip_adapter_image_embeds": [torch.zeros(2, EMB).half()]}, "negative; positive"),
    ({"ip_adapter_image_embeds": [torch.zeros(2, 2, EMB).half()]}, "8 image tokens"),                # token count
    ({"ip_adapter_image_embeds": _embeds(1), "ip_adapter_scale": [0.5, 0.5]}, "ip_adapter_scale"),     # scale list length
    ({"ip_adapter_scale": [0.5, 0.5]}, "ip_adapter_scale"),
    ({"ip_adapter_image_embeds": _embeds(1), "ip_adapter_scale": "high"}, "ip_adapter_scale"),
    ({"ip_adapter_image_embeds": _embeds(1), "cross_attention_kwargs": {"ip_adapter_masks": torch.zeros(1, 1, 8, 8)}},
     "ip_adapter_masks"),
    ({"ip_adapter_image": object()}, "encode_image"),                                                # raw image: still refused
])
def test_submit_refusals_leave_the_batcher_usable(pipe1, bad, match):
    b, _ = _batcher(pipe1)
    with pytest.raises(ValueError, match=match):
        b.submit(_req("X", **bad))
    assert b.stats()["queued"] == 0
    fut = b.submit(_req("plain"))
    b.run_until_idle()
    assert fut.result()[0] == "plain"


def test_embeds_without_an_adapter_are_refused():
    b, _ = _batcher(_pipe())
    with pytest.raises(ValueError, match="without an IP-Adapter"):
        b.submit(_req("X", ip_adapter_image_embeds=_embeds(1)))
    fut = b.submit(_req("plain"))
    b.run_until_idle()
    assert fut.result()[0] == "plain"


def test_submit_accepts_embeds_and_takes_the_default_scale_at_submit_time(pipe1):
    b, _ = _batcher(pipe1)
    pipe1.set_ip_adapter_scale(0.6)
    e = _embeds(1)
    b.submit(_req("A", ip_adapter_image_embeds=e))
    pipe1.set_ip_adapter_scale(0.25)                              # no new batcher, no capture: the scale is per request
    b.submit(_req("B", ip_adapter_image_embeds=e))
    b.submit(_req("C", ip_adapter_image_embeds=e, ip_adapter_scale=0.9))
    b.submit(_req("D", ip_adapter_image_embeds=e, ip_adapter_scale=[0.1]))
    got = {r.req["name"]: (r.ip_scale, r.ip_embeds is not None) for r in b._queue}
    assert got == {"A": ([0.6], True), "B": ([0.25], True), "C": ([0.9], True), "D": ([0.1], True)}
    pipe1.set_ip_adapter_scale(1.0)


def test_refresh_is_handed_zero_row_scales_for_scale_zero_and_absent_embeds(pipe1):
    b, ex = _batcher(pipe1, max_batch=4, buckets=(4,))
    e = _embeds(1)
    b.submit(_req("with", ip_adapter_image_embeds=e, ip_adapter_scale=0.7))
    b.submit(_req("zero", ip_adapter_image_embeds=e, ip_adapter_scale=0.0))
    b.submit(_req("none"))
    b.step()
    n, members = ex.refreshes[-1]
    assert n == 4 and [None if m is None else m.req["name"] for m in members] == ["with", "zero", "none", None]
    assert _GraphExecutor.ip_row_scales(n, members, 0) == [0.7, 0.0, 0.0, 0.0, 0.7, 0.0, 0.0, 0.0]
    assert members[1].ip_embeds is None and members[2].ip_embeds is None          # nothing to project for either
    b.run_until_idle()


def test_hires_pair_hands_the_keys_to_the_second_pass(pipe1):
    base = ServingBatcher(pipe1, 128, 128, slot=0, executor=FakeExec(), max_batch=2, buckets=(2,))
    hi = ServingBatcher(pipe1, 192, 192, slot=1, executor=FakeExec(), max_batch=2, buckets=(2,))
    pair = HiresPair(base, hi)
    e = _embeds(1)
    fut = pair.submit(_req("H", upscale=True, upscale_x=1.5, ip_adapter_image_embeds=e, ip_adapter_scale=0.4))
    first = base._queue[0]
    assert first.ip_scale == [0.4] and first.ip_embeds[0] is e[0]
    assert first.hires.ip_scale == [0.4] and first.hires.ip_embeds[0] is e[0]
    pair.run_until_idle()
    assert fut.result()[0] == "H" and base.stats()["handoffs"] == 1
    with pytest.raises(ValueError, match="one tensor per loaded IP-Adapter"):
        pair.submit(_req("bad", upscale=True, upscale_x=1.5, ip_adapter_image_embeds=_embeds(2)))


def test_a_batcher_is_stale_after_load_or_unload():
    pipe = _pipe()
    before, _ = _batcher(pipe)
    before.submit(_req("ok"))
    pipe.load_ip_adapter(_adapter(pipe.unet, "standard"))
    with pytest.raises(RuntimeError, match="stale"):
        before.submit(_req("X"))
    loaded, _ = _batcher(pipe)
    loaded.submit(_req("ok", ip_adapter_image_embeds=_embeds(1)))
    pipe.unload_ip_adapter()
    with pytest.raises(RuntimeError, match="stale"):
        loaded.submit(_req("X"))
    after, _ = _batcher(pipe)
    after.submit(_req("ok"))


def test_an_adapter_with_too_many_tokens_is_refused_at_serve():
    pipe = _pipe(("standard", "full"))
    with pytest.raises(ValueError, match="txt2img") as e:
        pipe.serve(128, 128)
    assert "257" in str(e.value) and str(ops.IP_MAX_TOKENS) in str(e.value)


# ----------------------------------------------------------------------------- the C entry
@pytest.fixture(scope="module")
def lib():
    dsc_build.build(verbose=False)
    return dsc.load_library()


def test_entry_is_declared_and_exported(lib):
    name = "dsc_ip_xattn_add_f16"
    assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(lib, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", dsc.lib_path()], capture_output=True, text=True).stdout
    assert f" T {name}" in nm
    header = open(_lib.header_path()).read()
    assert f"#define DSC_IP_MAX_TOKENS {ops.IP_MAX_TOKENS}" in header and ops.IP_MAX_TOKENS >= 16


def test_entry_validates_its_arguments_without_a_gpu(lib):
    p = lambda a: ctypes.c_void_p(a)  # noqa: E731

    def call(**kw):
        H, d, T = kw.get("H", 8), kw.get("d", 40), kw.get("T", 4)
        return lib.dsc_ip_xattn_add_f16(kw.get("q", p(0x1000)), kw.get("sb", 64 * H * d), kw.get("sl", H * d), kw.get("sh", d),
                                        kw.get("k", p(0x2000)), kw.get("v", p(0x3000)), kw.get("skv", T * H * d),
                                        kw.get("rs", p(0x4000)), kw.get("io", p(0x5000)), kw.get("B", 2), kw.get("L", 64), H, d, T,
                                        0.0, None)

    for null in ("q", "k", "v", "rs", "io"):
        assert call(**{null: None}) == -1, null
    assert call(B=0) == -1 and call(L=0) == -1 and call(H=0) == -1 and call(T=0) == -1 and call(d=0) == -1
    assert call(sb=-8) == -1 and call(sl=0) == -1 and call(skv=8) == -1          # rows of k_ip / v_ip would overlap
    assert call(io=p(0x1000)) == -1                                               # in place on its own query
    assert call(d=12) == -2 and call(d=168) == -2 and call(T=ops.IP_MAX_TOKENS + 1) == -2
    assert call(q=p(0x1004)) == -2 and call(io=p(0x5008)) == -2 and call(rs=p(0x4002)) == -2          # misaligned
    assert call(sl=324) == -2 and call(skv=4 * 8 * 40 + 4) == -2                   # 16-byte pieces


def test_wrapper_fails_loudly_without_a_gpu():
    q = torch.zeros(2, 16, 2, 8, dtype=torch.float16)
    k = torch.zeros(2, 4, 2, 8, dtype=torch.float16)
    with pytest.raises(dsc.DscLibraryError):
        ops.ip_xattn_add(q, k, k.clone(), torch.ones(2), torch.zeros(2, 16, 16, dtype=torch.float16))      # no CPU fallback
