"""Live previews in the continuous batcher, the host half: dsc_latent_preview's C ABI (exported, declared, bound; its argument
checks run before any GPU call), the numpy restatement of its arithmetic (ops.latent_preview_numpy, the GPU tests' reference)
against an independent float64 computation and on hand-picked ties, and the scheduling of previews - which steps are due, drops,
held futures, callback errors, refusals, stats - against a recording executor."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from inputs import FakeTokenizer
from serving_fakes import RecordingExec

import diffusionspatialcontrol_amd as dsc
from diffusionspatialcontrol_amd import _lib, build as dsc_build, ops
from diffusionspatialcontrol_amd.modules.serving import HiresPair, ServingBatcher

S = 77
BAD_ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    dsc_build.build(verbose=False)
    return dsc.load_library()


# ----------------------------------------------------------------------------- the C ABI
def test_symbol_is_exported_declared_and_bound(lib):
    assert "dsc_latent_preview" in _lib.declared_symbols()
    assert "dsc_latent_preview" in _lib._SIGNATURES
    assert hasattr(lib, "dsc_latent_preview")
    nm = subprocess.run(["nm", "-D", "--defined-only", dsc.lib_path()], capture_output=True, text=True).stdout
    assert " T dsc_latent_preview" in nm
    header = open(_lib.header_path()).read()
    assert re.search(r"#define\s+DSC_PREVIEW_MAX_ROWS\s+16\b", header)
    assert re.search(r"#define\s+DSC_PREVIEW_MAX_CHANNELS\s+8\b", header)
    assert ops.PREVIEW_MAX_ROWS == 16 and ops.PREVIEW_MAX_CHANNELS == 8 and ops.PREVIEW_SCALES == (1, 2, 4, 8)
    k = np.asarray(ops.LATENT_RGB_SD15, dtype=np.float32)
    assert k.shape == (5, 3) and not k[4].any()                       # a 4 x 3 matrix, then a zero bias


def test_argument_checks_need_no_gpu(lib):
    """every call here fails a check, so none reaches a launch; `rows` and `coef` are real host arrays (the entry reads them)"""
    lat, out = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    rows = (ctypes.c_int * 16)(*range(16))
    coef = (ctypes.c_float * 27)(*([0.25] * 27))

    def call(lat=lat, stride=4 * 8 * 16, rows=rows, n=2, C=4, h=8, w=16, coef=coef, up=1, out=out):
        return lib.dsc_latent_preview(lat, stride, rows, n, C, h, w, coef, up, out, None)

    assert call(lat=None) == BAD_ARG and call(out=None) == BAD_ARG and call(rows=None) == BAD_ARG and call(coef=None) == BAD_ARG
    for key in ("n", "C", "h", "w"):
        assert call(**{key: 0}) == BAD_ARG and call(**{key: -2}) == BAD_ARG, key
    assert call(n=17) == BAD_ARG and call(C=9) == BAD_ARG
    for up in (0, 3, 5, 6, 7, 16, -1):
        assert call(up=up) == BAD_ARG, up
    assert call(rows=(ctypes.c_int * 2)(0, -1)) == BAD_ARG
    assert call(rows=(ctypes.c_int * 2)(-3, 1)) == BAD_ARG
    # one lane owns 8 pixels of an output row
    assert call(w=12, up=1) == UNSUPPORTED and call(w=10, up=2) == UNSUPPORTED and call(w=9, up=4) == UNSUPPORTED
    assert call(w=3, up=1) == UNSUPPORTED
    # the load width `up` selects: 16, 8, 4 or 2 bytes, for the base and for the row stride
    for up, off in ((1, 8), (2, 4), (4, 2), (8, 1)):
        assert call(lat=ctypes.c_void_p(0x10000 + off), up=up) == UNSUPPORTED, up
    for up, stride in ((1, 4 * 8 * 16 + 4), (2, 4 * 8 * 16 + 2), (4, 4 * 8 * 16 + 1)):
        assert call(stride=stride, up=up) == UNSUPPORTED, up
    assert call(out=ctypes.c_void_p(0x20004)) == UNSUPPORTED          # 8-byte stores
    assert call(h=1 << 20, w=1 << 20, up=8) == UNSUPPORTED            # a grid that overflows
    # the order: a bad argument is reported before an unsupported shape
    assert call(w=12, n=17) == BAD_ARG


def test_wrapper_refuses_cpu_tensors():
    with pytest.raises(_lib.DscLibraryError, match="GPU only"):
        ops.latent_preview(torch.zeros(1, 4, 8, 8, dtype=torch.float16), [0])


# ----------------------------------------------------------------------------- the restatement
def _float64(lat, coef, up):
    """an independent computation: float64 throughout, einsum for the map, no intermediate rounding -> grey levels, unrounded"""
    z = np.asarray(lat, dtype=np.float64)
    flat = np.asarray(coef, dtype=np.float32).reshape(-1).astype(np.float64)
    C = z.shape[1]
    v = np.einsum("nchw,cq->nhwq", z, flat[:3 * C].reshape(C, 3)) + flat[3 * C:]
    y = np.clip(v / 2 + 0.5, 0.0, 1.0) * 255.0
    return np.kron(y, np.ones((1, up, up, 1)))


@pytest.mark.parametrize("C, up", [(4, 1), (4, 2), (8, 4), (3, 8)])
def test_restatement_against_float64(C, up):
    rng = np.random.default_rng(C * 10 + up)
    lat = (1.5 * rng.standard_normal((3, C, 9, 10))).astype(np.float16)
    coef = (0.3 * rng.standard_normal(3 * C + 3)).astype(np.float32)
    got = ops.latent_preview_numpy(lat, coef, up)
    ref = _float64(lat, coef, up)
    assert got.dtype == np.uint8 and got.shape == (3, 9 * up, 10 * up, 3) and got.flags["C_CONTIGUOUS"]
    worst = np.abs(got.astype(np.float64) - ref).max()
    assert worst <= 1.0, worst
    assert got.min() == 0 and got.max() == 255 and 20 < got.std()                  # (clamped at both ends, and an image)
    assert np.array_equal(ops.latent_preview_numpy(torch.from_numpy(lat), coef, up), got)
    # the default coefficients are the C = 4 ones
    if C == 4:
        assert np.array_equal(ops.latent_preview_numpy(lat, None, up), ops.latent_preview_numpy(lat, ops.LATENT_RGB_SD15, up))
    else:
        with pytest.raises(ValueError, match="coef"):
            ops.latent_preview_numpy(lat, None, up)


def test_restatement_ties_and_clamps():
    one = np.ones((1, 1, 1, 1), dtype=np.float16)

    def byte(k, bias, z=1.0):
        out = ops.latent_preview_numpy(one * np.float16(z), [k, k, k, bias, bias, bias], 1)
        assert out.shape == (1, 1, 1, 3) and len(set(out.reshape(-1).tolist())) == 1
        return int(out[0, 0, 0, 0])

    assert byte(0.0, 0.0) == 128                                      # y * 255 = 127.5: the tie goes to the even 128
    assert byte(1.0, -1.0) == 128                                     # ... reached through a product and a sum
    assert byte(0.0, -1.0) == 0 and byte(0.0, -3.0) == 0 and byte(-0.5, 0.0, z=8.0) == 0
    assert byte(0.0, 1.0) == 255 and byte(0.0, 3.0) == 255 and byte(0.5, 0.0, z=8.0) == 255
    assert byte(0.0, -1.0 + 2.0 / 255.0) == 1 and byte(0.0, 1.0 - 2.0 / 255.0) == 254
    with pytest.raises(ValueError, match="up"):
        ops.latent_preview_numpy(one, [0, 0, 0, 0, 0, 0], 3)


# ----------------------------------------------------------------------------- the batcher against a recording executor
class PreviewExec(RecordingExec):
    """RecordingExec plus the preview interface: `preview` records the slots and hands out a handle that is ready at once
    (`hold = True`: only after `release()`), or None while `full`; a thumbnail is a 2 x 2 image filled with its slot number"""
    step_keys, join_keys = ("step", "sigma"), None

    def __init__(self, name=None, events=None):
        super().__init__(name, events)
        self.preview_calls, self.handles, self.ensured = [], [], 0
        self.full = self.hold = False

    def ensure_preview(self):
        self.ensured += 1

    def preview(self, slots):
        self._event("preview", list(slots))
        if self.full:
            return None
        self.preview_calls.append(list(slots))
        h = {"slots": list(slots), "ready": not self.hold, "taken": 0}
        self.handles.append(h)
        return h

    def release(self):
        for h in self.handles:
            h["ready"] = True

    def preview_ready(self, h):
        return h["ready"]

    def preview_image(self, h, j):
        h["taken"] += 1
        return np.full((2, 2, 3), h["slots"][j], dtype=np.uint8)

    def result(self, r, h):
        return (self.name, r.req.get("name"), len(self.applied[id(r)]))


@pytest.fixture(scope="module")
def pipe():
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    unet = UNet2DConditionModel(UNetConfig.tiny()).half()
    return StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())


def _req(name, steps=5, **kw):
    emb = torch.randn(2, S, 64, generator=torch.Generator().manual_seed(len(name) + steps))
    r = {"name": name, "prompt_embeds": emb[1:2].half(), "negative_prompt_embeds": emb[0:1].half(),
         "num_inference_steps": steps, "guidance_scale": 7.5, "sampler_opt": {"scheduler": "karras"}}
    r.update(kw)
    return r


def _batcher(pipe, ex=None, **kw):
    ex = ex or PreviewExec("b")
    kw = dict(dict(max_batch=2, buckets=(1, 2), previews=True), **kw)
    return ServingBatcher(pipe, 128, 128, executor=ex, **kw), ex


def _watch(log, name):
    def on_preview(step, steps, image):
        assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.shape == (2, 2, 3)
        log.append((name, step, steps, int(image[0, 0, 0])))
    return on_preview


@pytest.mark.parametrize("k, due", [(1, [1, 2, 3, 4]), (2, [2, 4]), (3, [3])])
def test_due_steps_never_the_last(pipe, k, due):
    b, ex = _batcher(pipe)
    log = []
    f = b.submit(_req("A", preview_every=k, on_preview=_watch(log, "A")))
    b.run_until_idle()
    assert f.result(timeout=0) == ("b", "A", 5)
    assert log == [("A", s, 5, 0) for s in due]                       # (slot 0's row; `step` counts the steps applied)
    assert ex.preview_calls == [[0]] * len(due)
    st = b.stats()
    assert st["previews"] == len(due) and st["preview_rows"] == len(due) and st["previews_dropped"] == 0
    assert st["preview_callback_errors"] == 0 and all(h["taken"] == 1 for h in ex.handles)
    # the launch sits between the transition that applied the step and the run of the next bucket
    names = [e[0] for e in ex.events]
    for i, name in enumerate(names):
        if name == "preview":
            assert names[i - 1] == "transition" and names[i + 1] == "run", names[i - 1:i + 2]


def test_a_one_step_request_gets_none_and_absent_keys_mean_none(pipe):
    b, ex = _batcher(pipe)
    log = []
    futs = [b.submit(_req("one", steps=1, preview_every=1, on_preview=_watch(log, "one"))),
            b.submit(_req("plain")), ]
    b.run_until_idle()
    futs += [b.submit(_req("zero", preview_every=0, on_preview=_watch(log, "zero"))),
             b.submit(_req("none", preview_every=None)), b.submit(_req("callback only", on_preview=_watch(log, "cb")))]
    b.run_until_idle()
    assert all(f.done() for f in futs) and log == [] and ex.preview_calls == [] and b.stats()["previews"] == 0


def test_two_requests_share_one_launch_only_the_asking_one_is_called(pipe):
    b, ex = _batcher(pipe)
    log = []
    fa = b.submit(_req("A", preview_every=1, on_preview=_watch(log, "A")))
    b.step()
    fb = b.submit(_req("B"))
    fc = None
    b.step()
    b.step()
    fc = b.submit(_req("C", steps=3, preview_every=2, on_preview=_watch(log, "C")))      # waits for a slot, then takes A's
    b.run_until_idle()
    assert fa.done() and fb.done() and fc.done()
    assert [e for e in log if e[0] == "A"] == [("A", s, 5, 0) for s in (1, 2, 3, 4)]
    assert [e for e in log if e[0] == "C"] == [("C", 2, 3, 0)]
    assert all(len(c) == 1 for c in ex.preview_calls) and b.stats()["preview_rows"] == 5
    # two due slots in one step: one launch, two rows, in slot order
    b2, ex2 = _batcher(pipe)
    log2 = []
    for name in ("X", "Y"):
        b2.submit(_req(name, steps=3, preview_every=1, on_preview=_watch(log2, name)))
    b2.run_until_idle()
    assert ex2.preview_calls == [[0, 1], [0, 1]] and b2.stats()["previews"] == 2 and b2.stats()["preview_rows"] == 4
    assert log2 == [("X", 1, 3, 0), ("Y", 1, 3, 1), ("X", 2, 3, 0), ("Y", 2, 3, 1)]


def test_hires_pair_previews_both_passes(pipe):
    events = []
    base, hi = PreviewExec("base", events), PreviewExec("hires", events)
    kw = dict(max_batch=2, buckets=(1, 2), previews=True)
    pair = HiresPair(ServingBatcher(pipe, 128, 128, slot=0, executor=base, **kw),
                     ServingBatcher(pipe, 192, 192, slot=1, executor=hi, **kw))
    log = []
    f = pair.submit(_req("H", steps=4, preview_every=1, on_preview=_watch(log, "H"), upscale=True, upscale_x=1.5,
                         upscale_denoising_strength=0.75))
    pair.run_until_idle()
    assert f.result(timeout=0)[0] == "hires"
    # the first pass counts its 4 steps, the second its own 3 (int(4 * 0.75)); neither previews its last
    assert log == [("H", 1, 4, 0), ("H", 2, 4, 0), ("H", 3, 4, 0), ("H", 1, 3, 0), ("H", 2, 3, 0)]
    assert len(base.preview_calls) == 3 and len(hi.preview_calls) == 2
    st = pair.stats()
    assert st["base"]["previews"] == 3 and st["hires"]["previews"] == 2 and st["handoffs"] == 1
    # serve_hires and serve take the arguments (checked before anything touches a device)
    with pytest.raises(ValueError, match="preview_scale"):
        pipe.serve_hires(128, 128, 1.5, previews=True, preview_scale=3)
    with pytest.raises(ValueError, match="preview_ring"):
        pipe.serve(128, 128, previews=True, preview_scale=4, preview_ring=0)


def test_a_dropped_preview_is_counted_and_the_step_proceeds(pipe):
    b, ex = _batcher(pipe)
    log = []
    f = b.submit(_req("A", preview_every=1, on_preview=_watch(log, "A")))
    b.step()                                                          # the join
    ex.full = True
    b.step()                                                          # step 1: no free entry
    b.step()                                                          # step 2: still none
    ex.full = False
    b.run_until_idle()
    assert f.result(timeout=0) == ("b", "A", 5) and ex.runs == [1] * 5
    assert log == [("A", 3, 5, 0), ("A", 4, 5, 0)]
    st = b.stats()
    assert st["previews_dropped"] == 2 and st["previews"] == 2 and st["preview_rows"] == 2 and st["steps"] == 5


def test_the_future_is_held_until_its_previews_are_delivered(pipe):
    b, ex = _batcher(pipe)
    ex.hold = True
    log = []
    fa = b.submit(_req("A", steps=3, preview_every=1, on_preview=_watch(log, "A")))
    fb = b.submit(_req("B", steps=3))
    fa.add_done_callback(lambda _: log.append(("A", "done")))
    while b.step():
        pass
    assert fb.done() and not fa.done() and log == []                  # B has no previews queued: it is not held
    assert not b.step() and not fa.done()
    ex.release()
    assert not b.step()                                               # idle: the poll alone delivers, then resolves
    assert fa.done() and log == [("A", 1, 3, 0), ("A", 2, 3, 0), ("A", "done")]
    # `wait=True` (run_until_idle / stop) takes the previews first, ready or not
    b2, ex2 = _batcher(pipe)
    ex2.hold = True
    log2 = []
    f2 = b2.submit(_req("A", steps=3, preview_every=2, on_preview=_watch(log2, "A")))
    f2.add_done_callback(lambda _: log2.append(("A", "done")))
    b2.run_until_idle()
    assert log2 == [("A", 2, 3, 0), ("A", "done")]


def test_a_callback_that_raises_is_counted_and_disturbs_nobody(pipe):
    b, ex = _batcher(pipe)
    log = []

    def bad(step, steps, image):
        raise RuntimeError(f"client bug at step {step}")

    fa = b.submit(_req("A", steps=4, preview_every=1, on_preview=bad))
    fb = b.submit(_req("B", steps=4, preview_every=2, on_preview=_watch(log, "B")))
    b.run_until_idle()
    assert fa.result(timeout=0) == ("b", "A", 4) and fb.result(timeout=0) == ("b", "B", 4)
    assert log == [("B", 2, 4, 1)]
    st = b.stats()
    assert st["preview_callback_errors"] == 3 and st["previews"] == 3 and st["preview_rows"] == 4 and st["leaves"] == 2


def test_preview_keys_are_validated_at_submit(pipe):
    b, _ = _batcher(pipe)
    ok = lambda *a: None                                              # noqa: E731
    for bad in (-1, 1.0, "2", True, [1]):
        with pytest.raises(ValueError, match="preview_every"):
            b.submit(_req("A", preview_every=bad, on_preview=ok))
    with pytest.raises(ValueError, match="preview_every.*on_preview"):
        b.submit(_req("A", preview_every=2))
    for bad in (3, "print", [ok]):
        with pytest.raises(ValueError, match="on_preview.*callable"):
            b.submit(_req("A", preview_every=2, on_preview=bad))
    assert b.stats()["queued"] == 0


def test_preview_every_is_refused_without_the_flag(pipe):
    plain = ServingBatcher(pipe, 128, 128, executor=RecordingExec())
    with pytest.raises(ValueError, match=r"preview_every.*previews=True"):
        plain.submit(_req("A", preview_every=1, on_preview=lambda *a: None))
    plain.submit(_req("A"))                                           # and it serves what it served
    plain.submit(_req("A", preview_every=0))
    assert plain.stats()["queued"] == 2
    # a flagless batcher never calls a preview method: RecordingExec has none
    f = plain.submit(_req("B"))
    plain.run_until_idle()
    assert f.done() and not hasattr(plain.exec, "preview")


def test_a_bad_preview_scale_is_refused_at_construction(pipe):
    with pytest.raises(ValueError, match=r"preview_scale.*76.*2, 4, 8") as e:
        ServingBatcher(pipe, 608, 608, executor=PreviewExec(), previews=True, preview_scale=1)
    assert "1, 2" not in str(e.value)
    for scale in (2, 4, 8):
        assert ServingBatcher(pipe, 608, 608, executor=PreviewExec(), previews=True, preview_scale=scale).preview_scale == scale
    for bad in (0, 3, 16, 2.0, True, None, "8"):
        with pytest.raises(ValueError, match="preview_scale"):
            ServingBatcher(pipe, 128, 128, executor=PreviewExec(), previews=True, preview_scale=bad)
    with pytest.raises(ValueError, match="preview_scale.*use one of 8$"):
        ServingBatcher(pipe, 120, 120, executor=PreviewExec(), previews=True, preview_scale=4)       # 15 wide: only 8 works
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="preview_ring"):
            ServingBatcher(pipe, 128, 128, executor=PreviewExec(), previews=True, preview_ring=bad)
    with pytest.raises(ValueError, match="coef"):
        ServingBatcher(pipe, 128, 128, executor=PreviewExec(), previews=True, preview_coef=[0.0] * 12)
    with pytest.raises(TypeError):
        ServingBatcher(pipe, 128, 128, executor=PreviewExec(), preview=True)
    # without the flag the other arguments are not looked at
    assert not ServingBatcher(pipe, 608, 608, executor=RecordingExec(), preview_scale=1).previews


def test_stats_keys_only_with_the_flag(pipe):
    plain = ServingBatcher(pipe, 128, 128, executor=RecordingExec())
    lane, ex = _batcher(pipe)
    new = {"previews", "preview_rows", "previews_dropped", "preview_callback_errors"}
    assert not plain.previews and not new & set(plain.stats())
    assert set(lane.stats()) - set(plain.stats()) == new and all(lane.stats()[k] == 0 for k in new)
    lane.warm()
    assert ex.ensured == 1 and lane.stats()["captures_after_warm"] == 0
