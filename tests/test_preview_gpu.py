"""Live previews in the continuous batcher on the MI355X (`-m gpu`): dsc_latent_preview against its numpy float32 restatement
(ops.latent_preview_numpy, checked on the CPU by tests/test_preview_host.py), bit for bit - over every finite fp16 value, at the
edges of its launch, with rows picked out of order from a strided buffer and guard bytes around the output - and the preview path
of `pipe.serve(..., previews=True)`: every delivered image against the restatement of `exec.old[slot]`, the final latents
against a batcher without the flag, the driver thread's ordering, and a hires pair."""
import numpy as np
import pytest
import torch

from inputs import FakeTokenizer

pytestmark = pytest.mark.gpu
SIZE, STEPS, OPT = 128, 4, {"scheduler": "karras"}
GUARD = 64


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- the kernel
def _guarded(ops, lat, rows, coef, up):
    """the launch into a buffer with GUARD bytes of 0xAB on both sides -> the thumbnails on the CPU; the guards must survive"""
    n, (_, _, h, w) = len(rows), lat.shape
    nbytes = n * h * up * w * up * 3
    raw = torch.full((GUARD + nbytes + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    out = raw[GUARD:GUARD + nbytes].view(n, h * up, w * up, 3)
    ret = ops.latent_preview(lat, rows, coef, up, out=out)
    torch.cuda.synchronize()
    assert ret is out
    assert bool((raw[:GUARD] == 0xAB).all()) and bool((raw[GUARD + nbytes:] == 0xAB).all())
    return out.cpu().numpy()


def test_every_finite_fp16_value_in_each_channel(ops):
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.float16).clone()
    x[~torch.isfinite(x)] = 0.0                                       # NaN and inf patterns are outside the contract
    assert int(torch.isfinite(x).sum()) == 1 << 16 and x.unique().numel() >= 63487
    gen = torch.Generator().manual_seed(11)
    lat = torch.stack([x[torch.randperm(1 << 16, generator=gen)] for _ in range(4)]).reshape(1, 4, 256, 256).contiguous()
    ref = ops.latent_preview_numpy(lat, None, 1)
    got = _guarded(ops, lat.cuda(), [0], None, 1)
    assert got.shape == (1, 256, 256, 3) and got.dtype == np.uint8
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert ref.min() == 0 and ref.max() == 255


@pytest.mark.parametrize("C", [4, 8])
@pytest.mark.parametrize("n, h, w, up", [(1, 8, 8, 1), (3, 8, 12, 2), (2, 9, 10, 4), (2, 5, 3, 8), (16, 8, 8, 1)])
def test_shapes_with_random_coefficients(ops, n, h, w, up, C):
    """one lane; a partial block; odd sides; a width no load wider than 2 bytes fits; every thumbnail the grid takes"""
    rng = np.random.default_rng(1000 * n + 100 * h + 10 * w + up + C)
    lat = torch.from_numpy((1.5 * rng.standard_normal((n, C, h, w))).astype(np.float16))
    coef = (0.3 * rng.standard_normal(3 * C + 3)).astype(np.float32)
    ref = ops.latent_preview_numpy(lat, coef, up)
    got = _guarded(ops, lat.cuda(), list(range(n)), coef, up)
    assert got.shape == (n, h * up, w * up, 3)
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert ref.std() > 10                                             # (an image, not a constant)


@pytest.mark.parametrize("up, w", [(1, 16), (2, 12), (8, 5)])
def test_rows_out_of_order_from_a_strided_buffer(ops, up, w):
    C, h, pad = 4, 6, 8
    chw = C * h * w
    gen = torch.Generator().manual_seed(5 + up)
    buf = (1.5 * torch.randn(6, chw + pad, generator=gen)).half().cuda()
    lat = buf[:, :chw].unflatten(1, (C, h, w))
    assert lat.stride(0) == chw + pad and not lat.is_contiguous()
    rows = [4, 0, 2]
    coef = (0.3 * torch.randn(15, generator=gen)).numpy()
    ref = ops.latent_preview_numpy(lat[rows].cpu(), coef, up)
    got = _guarded(ops, lat, rows, coef, up)
    assert np.array_equal(got, ref)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    # a new tensor when no `out` is given, on the current stream
    again = ops.latent_preview(lat, rows, coef, up)
    torch.cuda.synchronize()
    assert again.dtype == torch.uint8 and np.array_equal(again.cpu().numpy(), ref)


def test_wrapper_refusals(ops):
    from diffusionspatialcontrol_amd import _lib
    ok = torch.zeros(2, 4, 8, 8, dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.DscLibraryError, match="GPU only"):
        ops.latent_preview(ok.cpu(), [0])
    with pytest.raises(TypeError, match="fp16"):
        ops.latent_preview(ok.float(), [0])
    for up in (0, 3, 16, None):
        with pytest.raises(ValueError, match="up must be"):
            ops.latent_preview(ok, [0], up=up)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.latent_preview(torch.zeros(1, 4, 8, 12, dtype=torch.float16, device="cuda"), [0], up=1)
    with pytest.raises(ValueError, match="contiguous"):
        ops.latent_preview(ok, [0], out=torch.zeros(1, 8, 8, 6, dtype=torch.uint8, device="cuda")[..., ::2])
    with pytest.raises(ValueError, match="shape"):
        ops.latent_preview(ok, [0, 1], out=torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError, match="uint8"):
        ops.latent_preview(ok, [0], out=torch.zeros(1, 8, 8, 3, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="is on"):
        ops.latent_preview(ok, [0], out=torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    for rows in ([], [2], [-1], list(range(2)) * 9):
        with pytest.raises(ValueError, match="rows"):
            ops.latent_preview(ok, rows)
    with pytest.raises(ValueError, match="dense"):
        ops.latent_preview(torch.zeros(2, 4, 8, 16, dtype=torch.float16, device="cuda")[..., ::2], [0])
    with pytest.raises(ValueError, match="coef"):
        ops.latent_preview(ok, [0], coef=[0.0] * 12)
    with pytest.raises(ValueError, match="channels"):
        ops.latent_preview(torch.zeros(1, 9, 8, 8, dtype=torch.float16, device="cuda"), [0], coef=[0.0] * 30)


# ----------------------------------------------------------------------------- the preview path of the batcher
class _Env:
    pass


@pytest.fixture(scope="module")
def env(ops):
    """tests/test_serving_gpu.py's tiny pipeline and requests; one batcher with the preview path and one without, both warm"""
    import test_serving_gpu as sg
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(7)
    e = _Env()
    e.cfg = UNetConfig.tiny()
    unet = UNet2DConditionModel(e.cfg).half().cuda()
    e.pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    e.reqs = [dict(r, num_inference_steps=STEPS, guidance_scale=7.5, sampler_opt=OPT)
              for r in sg._tiny_requests(e.cfg.cross_attention_dim, 3)]
    e.plain = e.pipe.serve(SIZE, SIZE, max_batch=2, buckets=(1, 2), slot=0).warm()
    e.live = e.pipe.serve(SIZE, SIZE, max_batch=2, buckets=(1, 2), slot=1, previews=True, preview_scale=8).warm()
    return e


def _collector(log, name=None):
    def on_preview(step, steps, image):
        log.append((name, step, steps, image))
    return on_preview


@pytest.mark.parametrize("k", [1, 2])
def test_stepped_by_hand_every_image_is_the_restatement_of_old(env, ops, k):
    b = env.live
    log = []
    f = b.submit(dict(env.reqs[0], preview_every=k, on_preview=_collector(log)))
    olds = {}                                                         # steps applied -> the row of `old` after that step() call
    calls = 0
    while b.step():
        calls += 1
        torch.cuda.synchronize()
        if calls >= 2:
            olds[calls - 1] = b.exec.old[0].cpu().clone()             # (call 1 is the join: no step applied yet)
    b.run_until_idle()
    assert calls == STEPS + 1 and sorted(olds) == list(range(1, STEPS + 1))
    want = [s for s in range(1, STEPS) if s % k == 0]                 # never the last step
    assert [(step, steps) for _, step, steps, _ in log] == [(s, STEPS) for s in want]
    for _, step, _, image in log:
        assert image.dtype == np.uint8 and image.shape == (SIZE, SIZE, 3) and image.flags["OWNDATA"]
        ref = ops.latent_preview_numpy(olds[step][None], None, 8)[0]
        assert np.array_equal(image, ref), (step, int((image != ref).sum()))
        assert image.std() > 5.0                                      # (an image, not a constant)
    assert not np.array_equal(log[0][3], ops.latent_preview_numpy(olds[STEPS][None], None, 8)[0])
    # the final latents: bit for bit the same request on a batcher built without `previews`
    g = env.plain.submit(dict(env.reqs[0]))
    env.plain.run_until_idle()
    assert torch.equal(f.result(timeout=0), g.result(timeout=0))
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["previews_dropped"] == 0 and st["preview_callback_errors"] == 0, st
    lane = b.exec.previews
    assert len(lane.free) == len(lane.ring) == 8 and not b._preview_queue


def test_two_requests_one_step_apart_only_the_first_is_called(env, ops):
    b = env.live
    before = b.stats()
    log = []
    fa = b.submit(dict(env.reqs[0], preview_every=1, on_preview=_collector(log, "A")))
    b.step()
    fb = b.submit(dict(env.reqs[1]))
    olds, calls = {}, 1
    while b.step():
        calls += 1
        torch.cuda.synchronize()
        olds[calls - 1] = b.exec.old[0].cpu().clone()
    b.run_until_idle()
    assert [(name, step, steps) for name, step, steps, _ in log] == [("A", s, STEPS) for s in range(1, STEPS)]
    for _, step, _, image in log:
        assert np.array_equal(image, ops.latent_preview_numpy(olds[step][None], None, 8)[0]), step
    st = b.stats()
    assert st["previews"] - before["previews"] == STEPS - 1 and st["preview_rows"] - before["preview_rows"] == STEPS - 1
    assert st["bucket_switches"] > before["bucket_switches"]          # they did share a batch (bucket 2)
    # each equals its own run on the flagless batcher, staggered the same way
    ga = env.plain.submit(dict(env.reqs[0]))
    env.plain.step()
    gb = env.plain.submit(dict(env.reqs[1]))
    env.plain.run_until_idle()
    assert torch.equal(fa.result(timeout=0), ga.result(timeout=0)) and torch.equal(fb.result(timeout=0), gb.result(timeout=0))
    assert st["captures_after_warm"] == 0


def test_driver_thread_previews_in_order_and_before_the_future(env):
    b = env.live
    before = b.stats()
    log = []
    b.start()
    try:
        futs = []
        for i, r in enumerate(env.reqs):
            f = b.submit(dict(r, preview_every=1, on_preview=lambda step, steps, image, i=i: log.append((i, step, steps))))
            f.add_done_callback(lambda _, i=i: log.append((i, "done", None)))
            futs.append(f)
        for f in futs:
            f.result(timeout=120)
    finally:
        b.stop()
    st = b.stats()
    rows = st["preview_rows"] - before["preview_rows"]
    assert sum(1 for e in log if e[1] != "done") == rows and rows >= 1
    for i in range(len(env.reqs)):
        mine = [e[1] for e in log if e[0] == i]
        assert mine[-1] == "done" and mine.count("done") == 1, mine    # every preview of it came before its future resolved
        steps = mine[:-1]
        assert steps == sorted(set(steps)) and all(1 <= s < STEPS for s in steps), mine
        if st["previews_dropped"] == before["previews_dropped"]:
            assert steps == list(range(1, STEPS)), mine
    assert st["captures_after_warm"] == 0 and st["active"] == 0 and st["queued"] == 0 and not b._preview_queue, st
    assert len(b.exec.previews.free) == len(b.exec.previews.ring)


def test_hires_pair_previews_at_both_sizes(env, ops):
    """128 -> 160 (20 x 20 latents, chained by hand as in test_image_serving_gpu.py): each pass counts its own steps and
    previews at its own size; the result equals the pair without the flag"""
    from diffusionspatialcontrol_amd.modules.serving import HiresPair
    pipe, target, scale = env.pipe, 160, 2

    def build(slots, **kw):
        return HiresPair(pipe.serve(SIZE, SIZE, max_batch=2, buckets=(1, 2), slot=slots[0], **kw),
                         pipe.serve(target, target, max_batch=2, buckets=(1, 2), slot=slots[1], **kw)).warm()

    noise = torch.randn(1, 4, target // 8, target // 8, generator=torch.Generator().manual_seed(9)).half().cuda()
    big = dict(env.reqs[0], upscale=True, upscale_x=1.25, upscale_denoising_strength=0.5, hires_latents=noise)
    f0 = (plain := build((2, 3))).submit(dict(big))
    plain.run_until_idle()
    pair = build((2, 3), previews=True, preview_scale=scale)     # (the first pair is idle: the slots are free)
    log = []
    f1 = pair.submit(dict(big, preview_every=1, on_preview=_collector(log)))
    pair.run_until_idle()
    assert torch.equal(f0.result(timeout=0), f1.result(timeout=0))
    assert [(step, steps) for _, step, steps, _ in log] == [(1, 4), (2, 4), (3, 4), (1, 2)]
    assert [image.shape for _, _, _, image in log] == [(SIZE // 8 * scale,) * 2 + (3,)] * 3 + [(target // 8 * scale,) * 2 + (3,)]
    assert all(image.std() > 5.0 for _, _, _, image in log)
    st = pair.stats()
    assert st["base"]["previews_dropped"] == 0 and st["hires"]["previews_dropped"] == 0, st
    assert st["handoffs"] == 1 and st["base"]["previews"] == 3 and st["hires"]["previews"] == 1, st
    assert st["base"]["captures_after_warm"] == 0 and st["hires"]["captures_after_warm"] == 0, st
