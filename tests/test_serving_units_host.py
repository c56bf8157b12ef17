"""The single copies the serving package keeps of what used to be repeated: step_launch (which launch serves a transition), the
submit-time validators of requests.py, the request record's defaults, and the names the package re-exports."""
import pytest
import torch

from serving_fakes import RecordingExec
from test_serving_img_host import LAT, MASK, _req

from diffusionspatialcontrol_amd import ops
from diffusionspatialcontrol_amd.modules.serving import ServingBatcher, requests, step_launch

INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def pipe():
    from test_linear_step_host import _pipe
    return _pipe()


def _batcher(pipe):
    ex = RecordingExec()
    return ServingBatcher(pipe, 128, 128, executor=ex, max_batch=2, buckets=(1, 2)), ex


# ----------------------------------------------------------------------------- step_launch
@pytest.mark.parametrize("extra, stepping", [
    ({}, "rows"),                                                            # DPM++ 2M on an eps-prediction model
    ({"sampler_name": "sample_euler"}, "linear"),                            # a record with c_skip ...
    ({"sampler_name": "sample_euler_ancestral", "guidance_rescale": 0.5}, "linear"),   # ... and with `rescale`
    ({"guidance_rescale": 0.5}, "linear"),                                   # DPM++ 2M with a rescale spells its c_skip out
    ({"image": LAT, "mask_image": MASK}, "known"),                           # an inpainting slot steps
])
def test_step_launch_of_the_records_the_batcher_builds(pipe, extra, stepping):
    """R (the case) joins beside P (DPM++ 2M, already stepping): the JOIN-only transition and the one in which only P steps are
    "rows", every transition in which R steps is the case's launch, and after R has left P is back on "rows" """
    b, ex = _batcher(pipe)
    b.submit(_req("P", steps=6, latents=LAT))
    b.step()
    b.submit(_req("R", steps=2, **dict({"latents": LAT}, **extra)))
    b.run_until_idle()
    kinds = [c[0] for c in ex.calls]
    assert kinds == ["rows", "rows", stepping, stepping] + ["rows"] * 3
    for launch, _, _, recs, known in ex.calls:
        assert step_launch(recs, known) == launch
        assert any("rescale" in r for r in recs) == (launch == "linear" and "guidance_rescale" in extra)
    assert b.stats()["linear_transitions"] == (2 if stepping == "linear" else 0)
    join_only = ex.calls[0][3]
    assert [r["mode"] for r in join_only] == [ops.ROW_JOIN] and step_launch(join_only, [None]) == "rows"
    assert step_launch([{"mode": ops.ROW_IDLE}], None) == "rows"
    assert step_launch([{"mode": ops.ROW_JOIN, "c_skip": 1.0}]) == "rows"      # only STEP records choose the launch


def test_known_with_a_linear_record_is_refused_before_the_launch(pipe):
    b, ex = _batcher(pipe)
    b._launch_compatible = lambda head, members: True                          # the admission rule, bypassed
    b.submit(_req("I", steps=3, image=LAT, mask_image=MASK))
    b.submit(_req("E", steps=3, latents=LAT, sampler_name="sample_euler"))
    b.step()                                                                   # both join: nothing steps yet
    assert [e[2] for e in ex.events if e[0] == "transition"] == ["rows"]
    with pytest.raises(RuntimeError, match="inpainting slot and a slot of another sampler"):
        b.step()
    assert len([e for e in ex.events if e[0] == "transition"]) == 1 and len(ex.calls) == 1 and ex.runs == [2]


# ----------------------------------------------------------------------------- the validators
@pytest.mark.parametrize("v, ok", [(0, True), (1.5, True), (-2, True), (10 ** 400, True), (True, False), (NAN, False),
                                   (INF, False), (-INF, False), ("1", False), (None, False), ([1.0], False)])
def test_finite(v, ok):
    assert requests.finite(v) is ok


@pytest.mark.parametrize("v, n, lists, want", [
    (0.5, 2, True, [0.5, 0.5]), (1, 1, False, [1.0]), ([0.1, 2], 2, True, [0.1, 2.0]), ((0.3,), 1, True, [0.3]),
    ("x", 0, True, []),                                                       # nothing to hold it against: as before
    (True, 1, True, None), (NAN, 1, True, None), (INF, 2, True, None), (-INF, 1, True, None), ("1", 1, True, None),
    ([0.5], 2, True, None), ([0.5, 0.5, 0.5], 2, True, None), ([0.5, "x"], 2, True, None), ([0.5, NAN], 2, True, None),
    ([0.5, True], 2, True, None), ([1.0], 1, False, None),                     # a list for a single model
])
def test_per_item(v, n, lists, want):
    if want is not None:
        assert requests.per_item("some_key", v, n, "pipe.thing", lists=lists) == want
        return
    with pytest.raises(ValueError, match="some_key") as e:
        requests.per_item("some_key", v, n, "pipe.thing", lists=lists)
    assert "pipe.thing" in str(e.value) and (repr(v) in str(e.value) or "list" in str(e.value))


@pytest.mark.parametrize("v, ok", [(0, True), (1, True), (0.25, True), (-0.1, False), (1.5, False), (True, False), (NAN, False),
                                   (INF, False), ("half", False), ([0.5], False)])
def test_fraction(v, ok):
    if ok:
        assert requests.fraction("some_key", v) == float(v)
        return
    with pytest.raises(ValueError, match=r"some_key.*\[0, 1\].*got"):
        requests.fraction("some_key", v)


class _Pil:
    size, resize = (32, 16), None


IMG = torch.rand(1, 3, 16, 32)


@pytest.mark.parametrize("image, multi, cins, size, ok", [
    (IMG, False, [3], None, True), (IMG, False, [3], (16, 32), True), (_Pil(), False, [3], (16, 32), True),
    ([IMG, _Pil()], True, [3, 3], None, True), ((IMG, IMG), True, [3, 3], (16, 32), True),
    ([IMG], False, [3], None, False),                                         # a list for a single model
    (IMG, True, [3, 3], None, False),                                         # one image for a Multi* model
    ([IMG], True, [3, 3], None, False), ([IMG] * 3, True, [3, 3], None, False),
    (IMG, False, [1], None, False), ([IMG, IMG], True, [3, 1], None, False),  # channels, per model
    (IMG[0], False, [3], None, False), (IMG.repeat(2, 1, 1, 1), False, [3], None, False),
    ((IMG * 255).to(torch.uint8), False, [3], None, False), (IMG, False, [3], (32, 32), False),
    (torch.rand(1, 3, 0, 8), False, [3], None, False), (object(), False, [3], None, False), ("img.png", False, [3], None, False),
])
def test_control_images(image, multi, cins, size, ok):
    if ok:
        out = requests.control_images("some_img", image, multi, cins, "pipe.thing", size=size)
        assert len(out) == len(cins) and out[0] is (image[0] if multi else image)
        return
    with pytest.raises(ValueError, match="some_img.*got"):
        requests.control_images("some_img", image, multi, cins, "pipe.thing", size=size)


# ----------------------------------------------------------------------------- the record, the package
def test_a_fresh_request_has_every_field_readable():
    r = requests._Request()
    fields = list(r.__slots__)
    assert len(fields) == 44 == len(set(fields)) and not hasattr(r, "__dict__")
    for name in fields:
        getattr(r, name)
    assert (r.i, r.kind, r.strength, r.second, r.adapter_limit, r.rescale, r.output_type) == (0, "txt2img", 1.0, False, 0, 0.0, "latent")
    assert r != requests._Request() and r in [r] and hash(r) != hash(requests._Request())       # identity, as the scheduler needs
    with pytest.raises(AttributeError):
        r.no_such_field = 1
    with pytest.raises(TypeError, match="no_such_field"):
        requests._Request(no_such_field=1)


def test_the_package_re_exports_what_was_imported_from_the_module():
    from diffusionspatialcontrol_amd.modules import serving
    for name in ("ServingBatcher", "HiresPair", "decode_buckets", "_GraphExecutor", "_ip_layers", "MAX_TEXT_KEYS", "step_launch"):
        assert hasattr(serving, name), name
    from diffusionspatialcontrol_amd.modules.serving import (HiresPair, MAX_TEXT_KEYS, ServingBatcher, _GraphExecutor,  # noqa: F401
                                                             _ip_layers, decode_buckets)
    assert MAX_TEXT_KEYS == 384 and serving.batcher.ServingBatcher is ServingBatcher
