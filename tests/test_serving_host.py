"""Continuous-batching scheduler (modules/serving/) on the host, against a fake step executor: admission order and slot
placement, bucket choice, the 32-row table admission wait, submit-time rejections, per-request DPM++ 2M coefficient and
time-embedding index sequences (those of txt2img's fused loop for the same schedule), futures in completion order."""
import numpy as np
import pytest
import torch

from inputs import FakeTokenizer
from serving_fakes import RecordingExec

from diffusionspatialcontrol_amd import ops
from diffusionspatialcontrol_amd.modules import sampling
from diffusionspatialcontrol_amd.modules.serving import ServingBatcher

S = 77


FakeExec = RecordingExec


@pytest.fixture(scope="module")
def pipe():
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    unet = UNet2DConditionModel(UNetConfig.tiny()).half()
    return StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())


def _req(name, steps=4, g=7.5, opt=None, state=None, ids=None, **kw):
    emb = torch.randn(2, S, 64, generator=torch.Generator().manual_seed(hash(name) % 1000))
    r = {"name": name, "prompt_embeds": emb[1:2].half(), "negative_prompt_embeds": emb[0:1].half(),
         "num_inference_steps": steps, "guidance_scale": g, "sampler_opt": {"scheduler": "karras"} if opt is None else opt,
         "region_map_state": state, "text_input_ids": ids, "latents": torch.zeros(1, 4, 16, 16).half()}
    r.update(kw)
    return r


def _batcher(pipe, **kw):
    ex = FakeExec()
    return ServingBatcher(pipe, 128, 128, executor=ex, **kw), ex


def _masked(n_masks, weight):
    """region state with n_masks one-cell masks at request-specific weight -> n_masks distinct non-zero rows per level"""
    tok = FakeTokenizer()
    words = [f"object{r}a object{r}b" for r in range(n_masks)]
    ids = [49406, 320]
    for w in words:
        ids += tok(w).input_ids
    ids = ids + [49407] * (S - len(ids))
    pos = np.array([ids], dtype=np.int64)
    state = {}
    for r, w in enumerate(words):
        m = np.full((128, 128), 255, dtype=np.uint8)
        m[0:64, (r % 2) * 64:(r % 2 + 1) * 64] = 0
        state[w] = {"map": m, "weight": weight + 0.01 * r, "mask_outsides": 0.0}
    return state, [pos.copy(), pos]


def test_fifo_admission_lowest_free_slot_and_buckets(pipe):
    b, ex = _batcher(pipe, max_batch=4, buckets=(1, 2, 4))
    fa = b.submit(_req("A", steps=2))
    fb = b.submit(_req("B", steps=5))
    fc = b.submit(_req("C", steps=3))
    assert b.step()                                   # all three join: slots 0, 1, 2 -> bucket 4
    assert [r.req["name"] for r in b._slots[:3]] == ["A", "B", "C"] and ex.runs == [4]
    assert ex.transitions[0][:2] == (0, 4) and [r["mode"] for r in ex.transitions[0][2]] == [ops.ROW_JOIN] * 3 + [ops.ROW_IDLE]
    b.step()                                          # A's 1st step
    b.step()                                          # A's 2nd (last) step: slot 0 frees
    assert b._slots[0] is None and fa.done()
    fd = b.submit(_req("D", steps=1))
    b.step()                                          # D takes slot 0 (the lowest free)
    assert b._slots[0].req["name"] == "D"
    b.step()                                          # C (3 steps) and D (1 step) leave: B alone in slot 1 -> bucket 2
    assert ex.runs[-1] == 2 and b._slots[2] is None
    b.run_until_idle()
    assert ex.runs[-1] == 2 and all(f.done() for f in (fb, fc, fd))
    s = b.stats()
    assert s["joins"] == 4 and s["leaves"] == 4 and s["bucket_switches"] == 1 and s["active"] == 0


def test_bucket_shrinks_when_top_slot_leaves(pipe):
    b, ex = _batcher(pipe, max_batch=4, buckets=(1, 2, 4))
    b.submit(_req("A", steps=6))
    b.submit(_req("B", steps=1))
    b.submit(_req("C", steps=2))
    b.step()
    assert ex.runs == [4]
    b.step()                                          # B leaves (slot 1); C still in slot 2 -> bucket 4
    assert ex.runs[-1] == 4
    b.step()                                          # C leaves: A alone in slot 0 -> bucket 1
    assert ex.runs[-1] == 1
    n_src, n_dst, recs = ex.transitions[-1]
    assert (n_src, n_dst) == (4, 1) and len(recs) == 4 and recs[2]["mode"] == ops.ROW_STEP and recs[2]["c_in_next"] == 0.0
    b.run_until_idle()
    assert ex.captured == [4, 1]


def _distinct(prepared, L):
    rows = torch.cat([p.tables[L].reshape(-1, S) for p in prepared] + [torch.zeros(1, S)])
    return torch.unique(rows, dim=0).shape[0]


def test_table_union_admission_waits(pipe):
    """the rule of the 32-row table budget, at a smaller budget: two requests' rows (plus the zero row of idle slots) fit,
    the third request's do not -> it waits in the queue (FIFO) until a slot frees, then takes the lowest free slot"""
    b, ex = _batcher(pipe, max_batch=4, buckets=(1, 2, 4))
    reqs = []
    for i in range(3):
        st, ids = _masked(2, 0.1 + 0.2 * i)
        reqs.append(_req(f"R{i}", steps=2 + i, state=st, ids=ids))
    prep = [b._prepare(r) for r in reqs]
    lim = max(_distinct(prep[:2], L) for L in b.levels())
    assert max(_distinct(prep, L) for L in b.levels()) > lim
    old = ops.MAX_REGION_ROWS
    try:
        ops.MAX_REGION_ROWS = lim
        futs = [b.submit(r) for r in reqs]
        b.step()
        assert [r is not None for r in b._slots[:3]] == [True, True, False] and b.stats()["queued"] == 1
        b.step()
        b.step()                                      # R0 (2 steps) leaves
        assert b._slots[0] is None and b.stats()["queued"] == 1
        b.step()                                      # R2 takes slot 0
        assert b._slots[0].req["name"] == "R2"
        b.run_until_idle()
        assert all(f.done() for f in futs)
    finally:
        ops.MAX_REGION_ROWS = old


@pytest.mark.parametrize("bad, match", [
    ({"height": 256}, "128x128"),
    ({"guidance_scale": 1.0}, "guidance_scale"),
    ({"weight_func": lambda w, s, qk: w * s}, "weight_func"),
    ({"control_img": object()}, "control_img"),
    ({"image_t2i_adapter": object()}, "image_t2i_adapter"),
    ({"ip_adapter_image": object()}, "ip_adapter_image"),
])
def test_submit_rejections(pipe, bad, match):
    b, _ = _batcher(pipe)
    with pytest.raises(ValueError, match=match):
        b.submit(_req("X", **bad))


def test_submit_rejects_long_prompts_v_prediction_and_incompressible_tables(pipe):
    b, _ = _batcher(pipe)
    r = _req("X")
    r["prompt_embeds"] = torch.zeros(1, 400, 64).half()
    r["negative_prompt_embeds"] = torch.zeros(1, 400, 64).half()
    with pytest.raises(ValueError, match="384"):
        b.submit(r)
    pipe.v_prediction = True
    try:
        with pytest.raises(ValueError, match="v-prediction"):
            b.submit(_req("X"))
    finally:
        pipe.v_prediction = False
    old = ops.MAX_REGION_ROWS
    st, ids = _masked(2, 0.3)
    try:
        ops.MAX_REGION_ROWS = 1
        with pytest.raises(ValueError, match="txt2img"):
            b.submit(_req("X", state=st, ids=ids))
    finally:
        ops.MAX_REGION_ROWS = old


def test_per_request_sequences_equal_the_fused_loop(pipe):
    """each request's (sigma, a, b, c, c_in_next, t_next, temb index) sequence is what _denoise_fused passes for its own
    schedule: coefficients of dpmpp_2m_coefficients(sigmas) (c = 0 first), c_in / t of the next sigma, row i + 1 of its table"""
    b, ex = _batcher(pipe, max_batch=4, buckets=(1, 2, 4))
    specs = [("A", 4, 7.5, {"scheduler": "karras"}), ("B", 6, 5.0, {"scheduler": "exponential"}),
             ("C", 3, 7.5, {})]
    futs = {}
    futs["A"] = b.submit(_req("A", steps=4))
    b.step()
    b.step()
    futs["B"] = b.submit(_req("B", steps=6, g=5.0, opt={"scheduler": "exponential"}))
    b.step()
    futs["C"] = b.submit(_req("C", steps=3, opt={}))
    b.run_until_idle()
    kdm = pipe.k_diffusion_model
    for name, steps, g, opt in specs:
        got_name, applied = futs[name].result()
        assert got_name == name
        sig = pipe._schedule(steps, opt, "cpu", torch.float16).float().tolist()
        coeffs = sampling.dpmpp_2m_coefficients(sig)
        assert len(coeffs) == steps and coeffs[0][2] == 0.0
        c_in0, _, t0 = kdm.step_scalars(sig[0])
        assert applied[0] == ("join", c_in0, float(t0), sig[0], ("temb", name, 0))
        assert len(applied) == steps + 1
        for i, (a, b_, c) in enumerate(coeffs):
            nxt = sig[i + 1]
            if i + 1 < steps:
                c_in_n, _, t_n = kdm.step_scalars(nxt)
                exp = ("step", i, sig[i], g, a, b_, c, c_in_n, float(t_n), ("temb", name, i + 1))
            else:
                exp = ("step", i, sig[i], g, a, b_, c, 0.0, 0.0, None)
            assert applied[i + 1] == exp, (name, i)


def test_futures_resolve_in_completion_order(pipe):
    b, ex = _batcher(pipe, max_batch=4, buckets=(1, 2, 4))
    order = []
    futs = [b.submit(_req(n, steps=s)) for n, s in (("A", 5), ("B", 2), ("C", 3))]
    for f in futs:
        f.add_done_callback(lambda f_: order.append(f_.result()[0]))
    b.run_until_idle()
    assert order == ["B", "C", "A"] == ex.finished


def test_background_driver_thread(pipe):
    b, ex = _batcher(pipe, max_batch=2, buckets=(1, 2))
    b.start()
    try:
        futs = [b.submit(_req(n, steps=s)) for n, s in (("A", 3), ("B", 2), ("C", 2))]
        res = [f.result(timeout=30)[0] for f in futs]
    finally:
        b.stop()
    assert res == ["A", "B", "C"] and b.stats()["leaves"] == 3
