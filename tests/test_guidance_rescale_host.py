"""Guidance rescale (arXiv 2305.08891 sec. 3.4) per request on the host: the serving scheduler's submit-time checks, records and
launch choice on a fake executor, the wrapper's validation of a record's `rescale`, and the fused loop's CPU-side refusals."""
import pytest
import torch

from diffusionspatialcontrol_amd import _lib, ops
from diffusionspatialcontrol_amd.modules.serving import ServingBatcher

from test_linear_step_host import LinearExec, _pipe
from test_serving_host import FakeExec, _req


@pytest.fixture(scope="module")
def pipe():
    return _pipe()


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), "0.7", [0.7], True])
def test_guidance_rescale_outside_the_unit_interval_is_rejected(pipe, bad):
    b = ServingBatcher(pipe, 128, 128, executor=LinearExec(), max_batch=2, buckets=(1, 2))
    with pytest.raises(ValueError, match="guidance_rescale"):
        b.submit(_req("X", guidance_rescale=bad))
    assert b.stats()["queued"] == 0
    for ok in (0, 0.0, 1, 1.0, 0.7, None):
        b.submit(_req("ok", guidance_rescale=ok))
    assert b.stats()["queued"] == 6


def test_inpainting_with_rescale_never_reaches_the_queue(pipe):
    b = ServingBatcher(pipe, 128, 128, executor=LinearExec(), max_batch=2, buckets=(1, 2))
    img, mask = torch.zeros(1, 4, 16, 16), torch.ones(1, 1, 128, 128)
    with pytest.raises(ValueError, match="inpaiting") as e:
        b.submit(_req("X", image=img, mask_image=mask, guidance_rescale=0.5))
    assert "guidance_rescale" in str(e.value) and b.stats()["queued"] == 0 and not b.step()


def test_records_and_launch_choice(pipe):
    """A (DPM++ 2M, phi = 0.7, 3 steps) beside B (DPM++ 2M, no key, 5 steps): while A steps, every transition is the linear
    family's launch, A's records carry `rescale` and the eps-prediction (1, -sigma) spelled out, B's records are what they are
    today (no c_skip / c_out / rescale: the wrapper's defaults); once A has left, the old launch is back"""
    ex = LinearExec()
    b = ServingBatcher(pipe, 128, 128, executor=ex, max_batch=2, buckets=(1, 2))
    fa = b.submit(_req("A", steps=3, guidance_rescale=0.7))
    b.submit(_req("B", steps=5))
    b.run_until_idle()
    assert fa.done() and len(ex.linear) == 3 and b.stats()["linear_transitions"] == 3
    assert len(ex.transitions) == 1 + 2                                   # the two joins, then B's steps 3 and 4 alone
    assert not ex.noise_tables                                            # (DPM++ 2M draws no noise)
    sig = ex.linear[0][2][0]["req"].sig
    for j, t in enumerate(ex.linear):
        ra, rb = t[2][0], t[2][1]
        assert ra["mode"] == ops.ROW_STEP and ra["step"] == j and ra["rescale"] == 0.7
        assert (ra["c_skip"], ra["c_out"]) == (1.0, -sig[j]) and ra["s"] == 0.0 and ra["noise"] is None
        assert rb["mode"] == ops.ROW_STEP and not {"rescale", "c_skip", "c_out", "s", "noise"} & set(rb)
    for t in ex.transitions:
        assert all("rescale" not in r for r in t[2])


def test_v_prediction_and_other_samplers_carry_rescale_beside_their_own_scalars():
    vp = _pipe("v_prediction")
    ex = LinearExec()
    b = ServingBatcher(vp, 128, 128, executor=ex, max_batch=2, buckets=(1, 2))
    b.submit(_req("E", steps=3, sampler_name="sample_euler", guidance_rescale=0.25))
    b.submit(_req("P", steps=3, sampler_name="sample_euler"))
    b.run_until_idle()
    kdm = vp.k_diffusion_model
    for j, t in enumerate(ex.linear):
        re_, rp = t[2][0], t[2][1]
        sg = re_["req"].sig[j]
        assert re_["rescale"] == 0.25 and "rescale" not in rp
        assert (re_["c_skip"], re_["c_out"]) == (kdm.step_skip(sg), kdm.step_scalars(sg)[1]) == (rp["c_skip"], rp["c_out"])


def _strip(transitions):
    return [(s, d, [{k: v for k, v in r.items() if k != "req"} for r in recs]) for s, d, recs in transitions]


def test_phi_zero_is_todays_record_lists_on_the_old_executor_protocol(pipe):
    """phi = 0 requests never reach the linear launch (every transition is step_launch's "rows"), and an explicit 0 leaves every record of every transition as it is without the key"""
    runs = []
    for kw in ({}, {"guidance_rescale": 0.0}, {"guidance_rescale": None}):
        ex = FakeExec()
        b = ServingBatcher(pipe, 128, 128, executor=ex, max_batch=4, buckets=(1, 2, 4))
        b.submit(_req("A", steps=4, **kw))
        b.step()
        b.submit(_req("B", steps=3, g=5.0, **kw))
        b.submit(_req("C", steps=2, **kw))
        b.run_until_idle()
        assert b.stats()["linear_transitions"] == 0 and not ex.linear and b.stats()["leaves"] == 3
        runs.append(_strip(ex.transitions))
    assert runs[0] == runs[1] == runs[2] and len(runs[0]) == 5          # A joins; A steps + B, C join; three more steps
    assert all("rescale" not in r and "c_skip" not in r for t in runs[0] for r in t[2])


def test_the_new_entry_is_declared():
    assert "dsc_cfg_linear_step_rows_rescale" in _lib.declared_symbols()
    assert "dsc_cfg_linear_step_rows" in _lib.declared_symbols()


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan"), "0.7", None])
def test_wrapper_names_a_bad_rescale_before_it_touches_a_tensor(bad):
    recs = [{"mode": ops.ROW_STEP, "sigma": 1.0, "rescale": 0.5}, {"mode": ops.ROW_STEP, "sigma": 1.0, "rescale": bad}]
    for fn in (ops.cfg_linear_step_rows, ops.cfg_linear_step_rows_rescale):
        with pytest.raises(ValueError, match=r"rows\[1\]\['rescale'\]"):
            fn(None, None, None, 2, None, None, None, recs)
    # a JOIN / IDLE record's value is never read
    assert ops._row_rescales("t", [{"mode": ops.ROW_JOIN, "rescale": bad}, {"mode": ops.ROW_STEP}]) == [0.0, 0.0]


def test_fused_rescale_takes_the_per_row_path_and_its_checks(pipe):
    """DPM++ 2M on an eps model with phi > 0 is on the per-row path: its slot limit and its fp16-on-GPU check, with their
    messages; phi outside [0, 1] is a ValueError; phi = 0 stays on the lockstep kernel (whose wrapper refuses CPU tensors)"""
    emb = torch.zeros(1, 77, 64).half()
    kw = dict(height=128, width=128, num_inference_steps=2, sampler_name="sample_dpmpp_2m", fused=True, prompt_embeds=emb,
              negative_prompt_embeds=emb, output_type="latent")
    n = ops.ROW_STEP_MAX_SLOTS + 1
    with pytest.raises(NotImplementedError, match="at most 16 images"):
        pipe.txt2img(None, guidance_rescale=0.7, num_images_per_prompt=n, latents=torch.zeros(n, 4, 16, 16).half(), **kw)
    with pytest.raises(NotImplementedError, match="fp16 latents on the GPU"):
        pipe.txt2img(None, guidance_rescale=0.7, latents=torch.zeros(1, 4, 16, 16).half(), **kw)
    with pytest.raises(ValueError, match="guidance_rescale"):
        pipe.txt2img(None, guidance_rescale=1.5, latents=torch.zeros(1, 4, 16, 16).half(), **kw)
    with pytest.raises(Exception) as e:
        pipe.txt2img(None, guidance_rescale=0.0, latents=torch.zeros(1, 4, 16, 16).half(), **kw)
    assert "per-row" not in str(e.value)
