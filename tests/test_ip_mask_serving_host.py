"""IP-Adapter region masks in the continuous batcher on the host (modules/serving/ against a fake executor): the opt-in at
construction, the submit-time refusals of `ip_adapter_masks`, the per-level weights recorded at submit (square and ragged
levels, a hires pair), the rows `refresh` is handed, and the masked C entry (declared, exported, validating without a GPU)."""
import ctypes
import subprocess

import pytest
import torch

from inputs import FakeTokenizer
from serving_fakes import RecordingExec

import diffusionspatialcontrol_amd as dsc
from diffusionspatialcontrol_amd import _lib, build as dsc_build, ops
from diffusionspatialcontrol_amd.modules.attention_modify import IPAdapterMaskProcessor
from diffusionspatialcontrol_amd.modules.serving import HiresPair, ServingBatcher, _GraphExecutor

S, EMB = 77, 48


FakeExec = RecordingExec


def _adapter(unet):
    from diffusionspatialcontrol_amd.modules import u_net_condition_modify as um
    ctx = unet.config.cross_attention_dim
    cross = [m for pre in ("down_blocks", "up_blocks", "mid_block") for n, m in unet.named_modules()
             if isinstance(m, um.Attention) and m.is_cross_attention and n.startswith(pre)]
    ip = {}
    for i, m in enumerate(cross):
        ip[f"{2 * i + 1}.to_k_ip.weight"] = torch.zeros(m.inner_dim, ctx)
        ip[f"{2 * i + 1}.to_v_ip.weight"] = torch.zeros(m.inner_dim, ctx)
    proj = {"proj.weight": torch.zeros(4 * ctx, EMB), "proj.bias": torch.zeros(4 * ctx), "norm.weight": torch.ones(ctx),
            "norm.bias": torch.zeros(ctx)}
    return {"image_proj": proj, "ip_adapter": ip}


def _pipe(adapters=0):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    unet = UNet2DConditionModel(UNetConfig.tiny()).half()
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    if adapters:
        pipe.load_ip_adapter([_adapter(pipe.unet) for _ in range(adapters)])
    return pipe


def _req(name, steps=3, **kw):
    emb = torch.randn(2, S, 64, generator=torch.Generator().manual_seed(len(name) + steps))
    r = {"name": name, "prompt_embeds": emb[1:2].half(), "negative_prompt_embeds": emb[0:1].half(),
         "num_inference_steps": steps, "guidance_scale": 7.5, "sampler_opt": {"scheduler": "karras"}}
    r.update(kw)
    return r


def _embeds(n=1):
    return [torch.zeros(2, 1, EMB).half() for _ in range(n)]


def _masks(t):
    return {"ip_adapter_masks": t}


def _smooth_mask(n, h, w, seed):
    """values in [0, 1] that vary over the image: the bicubic down-sampling has something to interpolate (and overshoots)"""
    return torch.rand(n, 1, h, w, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def pipe1():
    return _pipe(1)


def _batcher(pipe, height=128, width=128, **kw):
    ex = FakeExec()
    return ServingBatcher(pipe, height, width, executor=ex, **dict(dict(max_batch=2, buckets=(2,), ip_masks=True), **kw)), ex


def _still_usable(b):
    assert b.stats()["queued"] == 0
    fut = b.submit(_req("plain"))
    b.run_until_idle()
    assert fut.result()[0] == "plain"


def test_a_mask_capable_batcher_accepts_what_the_default_one_refuses(pipe1):
    """the request tests/test_ip_serving_host.py pins as refused: zeros(1, 1, 8, 8) with one adapter"""
    request = dict(ip_adapter_image_embeds=_embeds(1), cross_attention_kwargs=_masks(torch.zeros(1, 1, 8, 8)))
    b, _ = _batcher(pipe1)
    fut = b.submit(_req("masked", **request))
    assert b._queue[0].ip_weights is not None
    b.run_until_idle()
    assert fut.result()[0] == "masked"
    default, _ = _batcher(pipe1, ip_masks=False)
    with pytest.raises(ValueError, match="ip_adapter_masks") as e:
        default.submit(_req("X", **request))
    assert "ip_masks=True" in str(e.value)
    _still_usable(default)
    assert ServingBatcher(pipe1, 128, 128, executor=FakeExec()).ip_masks is False


@pytest.mark.parametrize("masks, match", [
    ([[[[1.0] * 8] * 8]], "tensor of shape"),                                   # not a tensor
    (torch.ones(1, 8, 8), "tensor of shape"),                                    # ndim != 4
    (torch.ones(1, 2, 8, 8), "tensor of shape"),                                 # shape[1] != 1
    (torch.ones(2, 1, 8, 8), "2 masks, the pipeline has 1"),                     # count
    (torch.full((1, 1, 8, 8), float("nan")), "finite"),
    (torch.full((1, 1, 8, 8), float("inf")), "finite"),
])
def test_mask_refusals_leave_the_batcher_usable(pipe1, masks, match):
    b, _ = _batcher(pipe1)
    with pytest.raises(ValueError, match=match):
        b.submit(_req("X", ip_adapter_image_embeds=_embeds(1), cross_attention_kwargs=_masks(masks)))
    _still_usable(b)


def test_a_hires_request_with_masks_needs_a_mask_capable_second_batcher(pipe1):
    base = ServingBatcher(pipe1, 128, 128, slot=0, executor=FakeExec(), max_batch=2, buckets=(2,), ip_masks=True)
    hi = ServingBatcher(pipe1, 192, 192, slot=1, executor=FakeExec(), max_batch=2, buckets=(2,))
    pair = HiresPair(base, hi)
    with pytest.raises(ValueError, match="ip_masks=True"):
        pair.submit(_req("X", upscale=True, upscale_x=1.5, ip_adapter_image_embeds=_embeds(1),
                         cross_attention_kwargs=_masks(torch.ones(1, 1, 16, 16))))
    assert base.stats()["queued"] == 0 and hi.stats()["queued"] == 0
    fut = pair.submit(_req("plain", upscale=True, upscale_x=1.5, ip_adapter_image_embeds=_embeds(1)))
    pair.run_until_idle()
    assert fut.result()[0] == "plain"


def _expected(mask_a, L):
    return IPAdapterMaskProcessor.downsample(mask_a, 1, L, 1)[0, :, 0].to(torch.float16)


@pytest.mark.parametrize("height, width, levels", [(128, 128, [256, 64, 16, 4]), (72, 80, [90, 25, 9, 4])])
def test_weights_are_recorded_per_level_at_submit(height, width, levels):
    """two adapters, one mask each at the image size: per adapter and level of THIS batcher the weights are
    IPAdapterMaskProcessor.downsample of the adapter's mask (the aspect-ratio arithmetic and pad / truncate of the restatement
    included), rounded to fp16.  72 x 80 is 9 x 10 latents: levels 90, 25, 9 and 4 queries"""
    pipe = _pipe(2)
    b, _ = _batcher(pipe, height, width)
    assert sorted(b.levels(), reverse=True) == levels
    masks = _smooth_mask(2, height, width, seed=height)
    masks[1, :, : height // 2] = 1.0
    masks[1, :, height // 2:] = 0.0
    b.submit(_req("M", ip_adapter_image_embeds=_embeds(2), cross_attention_kwargs=_masks(masks)))
    w = b._queue[0].ip_weights
    assert len(w) == 2
    for a in range(2):
        assert sorted(w[a], reverse=True) == levels
        for L in levels:
            assert w[a][L].dtype == torch.float16 and tuple(w[a][L].shape) == (L,)
            assert torch.equal(w[a][L], _expected(masks[a], L)), (a, L)
    assert not torch.equal(w[0][levels[0]], w[1][levels[0]])
    top = w[1][levels[0]]
    assert (top[: levels[0] // 4] == 1).all() and (top[-levels[0] // 4:] == 0).all()       # a half-image mask has exact zeros


def test_a_hires_second_pass_records_weights_at_its_own_levels(pipe1):
    base = ServingBatcher(pipe1, 128, 128, slot=0, executor=FakeExec(), max_batch=2, buckets=(2,), ip_masks=True)
    hi = ServingBatcher(pipe1, 192, 192, slot=1, executor=FakeExec(), max_batch=2, buckets=(2,), ip_masks=True)
    pair = HiresPair(base, hi)
    masks = _smooth_mask(1, 128, 128, seed=9)
    fut = pair.submit(_req("H", upscale=True, upscale_x=1.5, ip_adapter_image_embeds=_embeds(1),
                           cross_attention_kwargs=_masks(masks)))
    first = base._queue[0]
    assert sorted(first.ip_weights[0]) == sorted(base.levels()) and sorted(first.hires.ip_weights[0]) == sorted(hi.levels())
    assert 576 in first.hires.ip_weights[0] and 576 not in first.ip_weights[0]
    for L in hi.levels():
        assert torch.equal(first.hires.ip_weights[0][L], _expected(masks[0], L))
    pair.run_until_idle()
    assert fut.result()[0] == "H"


def test_masks_without_an_image_prompt_are_ignored(pipe1):
    b, _ = _batcher(pipe1)
    m = _masks(torch.ones(1, 1, 8, 8))
    b.submit(_req("none", cross_attention_kwargs=m))
    b.submit(_req("zero", ip_adapter_image_embeds=_embeds(1), ip_adapter_scale=0.0, cross_attention_kwargs=m))
    assert [(r.ip_embeds, r.ip_weights) for r in b._queue] == [(None, None), (None, None)]
    b.run_until_idle()


def test_refresh_plan_of_a_masked_an_unmasked_and_an_idle_member(pipe1):
    b, ex = _batcher(pipe1, max_batch=4, buckets=(4,))
    masks = _smooth_mask(1, 128, 128, seed=4)
    e = _embeds(1)
    b.submit(_req("masked", ip_adapter_image_embeds=e, ip_adapter_scale=0.7, cross_attention_kwargs=_masks(masks)))
    b.submit(_req("unmasked", ip_adapter_image_embeds=e, ip_adapter_scale=0.5))
    b.step()
    n, members = ex.refreshes[-1]
    assert n == 4 and [None if m is None else m.req["name"] for m in members] == ["masked", "unmasked", None, None]
    assert _GraphExecutor.ip_row_scales(n, members, 0) == [0.7, 0.5, 0.0, 0.0, 0.7, 0.5, 0.0, 0.0]
    for L in b.levels():
        rows = _GraphExecutor.ip_row_weights(n, members, 0, L)
        assert rows.dtype == torch.float16 and tuple(rows.shape) == (2 * n, L)
        want = _expected(masks[0], L)
        for i in range(2 * n):
            assert torch.equal(rows[i], want if i in (0, n) else torch.ones(L, dtype=torch.float16)), (L, i)
    b.run_until_idle()


def test_ip_masks_without_an_adapter_is_refused():
    pipe = _pipe()
    with pytest.raises(ValueError, match="without an IP-Adapter"):
        ServingBatcher(pipe, 128, 128, executor=FakeExec(), ip_masks=True)
    with pytest.raises(ValueError, match="without an IP-Adapter"):
        pipe.serve(128, 128, ip_masks=True)
    with pytest.raises(ValueError, match="without an IP-Adapter"):
        pipe.serve_hires(128, 128, upscale_x=1.5, ip_masks=True)


# ----------------------------------------------------------------------------- the processor's rows
def test_masks_keyword_beside_prepared_rows_is_still_an_error(pipe1):
    from diffusionspatialcontrol_amd.modules.serving import _ip_layers
    proc = _ip_layers(pipe1)[0][1]
    q4 = torch.zeros(2, 16, 2, 8, dtype=torch.float16)
    with pytest.raises(ValueError, match="inside the rows"):
        proc._ip_rows_branch(q4, torch.zeros(2, 16, 16, dtype=torch.float16), [(None, None, None, None)], torch.ones(1, 1, 8, 8), None)


# ----------------------------------------------------------------------------- the C entry
@pytest.fixture(scope="module")
def lib():
    dsc_build.build(verbose=False)
    return dsc.load_library()


def test_masked_entry_is_declared_and_exported(lib):
    name = "dsc_ip_xattn_add_masked_f16"
    assert name in _lib.declared_symbols() and name in _lib._SIGNATURES and hasattr(lib, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", dsc.lib_path()], capture_output=True, text=True).stdout
    assert f" T {name}" in nm
    assert "attention_modify.py:371-385 / :676-685" in open(_lib.header_path()).read()


def test_masked_entry_validates_its_arguments_without_a_gpu(lib):
    p = lambda a: ctypes.c_void_p(a)  # noqa: E731

    def call(**kw):
        H, d, T, L = kw.get("H", 8), kw.get("d", 40), kw.get("T", 4), kw.get("L", 64)
        return lib.dsc_ip_xattn_add_masked_f16(kw.get("q", p(0x1000)), kw.get("sb", 64 * H * d), kw.get("sl", H * d), kw.get("sh", d),
                                               kw.get("k", p(0x2000)), kw.get("v", p(0x3000)), kw.get("skv", T * H * d),
                                               kw.get("rs", p(0x4000)), kw.get("io", p(0x5000)), kw.get("w", p(0x6000)),
                                               kw.get("sw", L), kw.get("B", 2), L, H, d, T, 0.0, None)

    for null in ("q", "k", "v", "rs", "io", "w"):
        assert call(**{null: None}) == -1, null
    assert call(sw=63) == -1 and call(sw=0) == -1                                 # weight rows would overlap
    assert call(w=p(0x5000)) == -1                                                # the weights are the output
    assert call(w=p(0x6001)) == -2                                                # fp16: 2-byte aligned
    assert call(B=0) == -1 and call(L=0) == -1 and call(io=p(0x1000)) == -1       # the unmasked entry's checks still hold
    assert call(d=12) == -2 and call(T=ops.IP_MAX_TOKENS + 1) == -2 and call(q=p(0x1004)) == -2


def test_wrapper_checks_the_weight_and_fails_loudly_without_a_gpu():
    q = torch.zeros(2, 16, 2, 8, dtype=torch.float16)
    k = torch.zeros(2, 4, 2, 8, dtype=torch.float16)
    with pytest.raises(dsc.DscLibraryError):                                     # no CPU fallback
        ops.ip_xattn_add(q, k, k.clone(), torch.ones(2), torch.zeros(2, 16, 16, dtype=torch.float16),
                         q_weight=torch.ones(2, 16, dtype=torch.float16))
