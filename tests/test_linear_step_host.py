"""The linear-step sampler family on the host: `sampling.linear_step_coefficients` against the tree's own `sample_*` functions
(fp64, analytic denoiser, replayed noise), the noise table against what the samplers draw, and the serving scheduler's launch
choice, records and rejections for per-request samplers / v-prediction on a fake executor."""
import functools

import pytest
import torch

from inputs import FakeTokenizer

from diffusionspatialcontrol_amd import ops
from diffusionspatialcontrol_amd.modules import samplers_extra_k_diffusion as sx
from diffusionspatialcontrol_amd.modules import sampling
from diffusionspatialcontrol_amd.modules.serving import ServingBatcher, step_launch

from test_serving_host import FakeExec, _req

FUNCS = {"euler": sampling.sample_euler, "euler_ancestral": sampling.sample_euler_ancestral, "dpmpp_2m": sampling.sample_dpmpp_2m,
         "dpmpp_2m_sde": sampling.sample_dpmpp_2m_sde, "lcm": sx.sample_lcm}
VARIANTS = [("euler", {}), ("euler_ancestral", {}), ("euler_ancestral", {"eta": 0.6, "s_noise": 1.1}), ("dpmpp_2m", {}),
            ("dpmpp_2m_sde", {}), ("dpmpp_2m_sde", {"solver_type": "heun", "eta": 0.7, "s_noise": 0.9}),
            ("dpmpp_2m_sde", {"eta": 0.0}), ("dpmpp_2m_sde", {"eta": 0.0, "solver_type": "heun"}), ("lcm", {})]


def _sigmas(kind, steps):
    fn = sampling.get_sigmas_karras if kind == "karras" else sampling.get_sigmas_exponential
    return fn(steps, 0.0292, 14.6146).double()


def _denoiser(x, sigma):
    """D(x, sigma) = x / (1 + sigma^2): the posterior mean of unit-variance data"""
    return x / (1 + sigma.reshape(-1, 1, 1, 1) ** 2)


def _recurrence(x, sig, coeffs, noise):
    old = torch.zeros_like(x)
    for i, (a, b, c, s) in enumerate(coeffs):
        d = _denoiser(x, torch.tensor([sig[i]], dtype=torch.float64))
        x = a * x + b * d + c * old + (s * noise[i] if s != 0.0 else 0.0)
        old = d
    return x


@pytest.mark.parametrize("steps", [4, 8, 25])
@pytest.mark.parametrize("kind", ["karras", "exponential"])
@pytest.mark.parametrize("name, kw", VARIANTS)
def test_coefficients_reproduce_the_samplers(name, kw, kind, steps, monkeypatch):
    sigmas = _sigmas(kind, steps)
    g = torch.Generator().manual_seed(steps)
    x0 = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) * sigmas[0]
    noise = torch.randn(steps, 2, 4, 8, 8, generator=g, dtype=torch.float64)
    order = iter(range(steps))
    replay = lambda *_: noise[next(order)]                                           # noqa: E731
    args = dict(kw)
    if name in ("euler_ancestral", "dpmpp_2m_sde", "lcm"):
        args["noise_sampler"] = replay
    if name == "dpmpp_2m":          # its update is a HIP launch: the same a*x + b*D + c*old in fp64 here
        monkeypatch.setattr(sampling.ops, "dpmpp2m_update", lambda x, d, old, a, b, c: a * x + b * d + (c * old if old is not None else 0))
    ref = FUNCS[name](_denoiser, x0.clone(), sigmas, **args)
    coeffs = sampling.linear_step_coefficients(name, sigmas.tolist(), **kw)
    assert len(coeffs) == steps and all(len(c4) == 4 for c4 in coeffs)
    got = _recurrence(x0.clone(), sigmas.tolist(), coeffs, noise)
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    assert err <= 1e-12 * scale, (name, kw, kind, steps, err, scale)
    assert coeffs[-1][3] == 0.0                                                      # the sigma' = 0 step never adds noise
    if kw.get("eta") == 0.0:
        assert all(c4[3] == 0.0 for c4 in coeffs)
    if name in ("euler_ancestral", "lcm") or (name == "dpmpp_2m_sde" and kw.get("eta", 1.0)):
        assert all(c4[3] > 0.0 for c4 in coeffs[:-1])                                # ... and every other step does


def test_dpmpp_2m_is_dpmpp_2m_coefficients_and_names_resolve():
    sig = _sigmas("karras", 9).tolist()
    assert [c4[:3] for c4 in sampling.linear_step_coefficients("dpmpp_2m", sig)] == sampling.dpmpp_2m_coefficients(sig)
    assert all(c4[3] == 0.0 for c4 in sampling.linear_step_coefficients("sample_dpmpp_2m", sig))
    for fam, fn in FUNCS.items():
        assert sampling.linear_family(fn) == fam == sampling.linear_family(fam) == sampling.linear_family("sample_" + fam)
    for other in (sampling.sample_heun, sampling.sample_lms, sx.sample_ddpm, sx.restart_sampler, "sample_dpmpp_sde", "nonsense",
                  functools.partial(sampling.sample_euler, s_churn=1.0), lambda *a, **k: None):
        assert sampling.linear_family(other) is None


@pytest.mark.parametrize("name", ["sample_heun", "sample_dpm_2", "sample_lms", "sample_dpm_2_ancestral", "sample_dpmpp_2s_ancestral",
                                  "sample_dpmpp_sde", "sample_dpmpp_3m_sde", "restart_sampler", "sample_ddpm", "sample_heunpp2"])
def test_unsupported_samplers_raise_by_name(name):
    with pytest.raises(NotImplementedError, match=name):
        sampling.linear_step_coefficients(name, [2.0, 1.0, 0.0])
    with pytest.raises(NotImplementedError, match=name):
        sampling.step_noise_table(name, torch.zeros(1, 4, 2, 2), [2.0, 1.0, 0.0])


def test_noise_table_is_what_the_samplers_draw():
    """seeded CPU generator: table row i is the i-th draw the sampler itself makes in protocol mode (default noise sampler for
    Euler a / LCM, the Brownian tree for DPM++ 2M SDE); ODE samplers and eta = 0 have no table"""
    sigmas = _sigmas("karras", 6).float()
    x = torch.zeros(2, 4, 4, 4)
    for name in ("euler_ancestral", "lcm", "dpmpp_2m_sde"):
        seen = []

        def spy(inner):
            def call(s0, s1):
                seen.append(inner(s0, s1))
                return seen[-1]
            return call
        torch.manual_seed(11)
        inner = sampling.BrownianTreeNoiseSampler(x, sigmas[-2], sigmas[0]) if name == "dpmpp_2m_sde" \
            else sampling.default_noise_sampler(x)
        FUNCS[name](lambda v, s: v * 0.5, x.clone(), sigmas, noise_sampler=spy(inner))
        torch.manual_seed(11)
        tab = sampling.step_noise_table(name, x, sigmas)
        assert tuple(tab.shape) == (6, 2, 4, 4, 4) and len(seen) == 5
        assert torch.equal(tab[:5], torch.stack(seen)) and not tab[5].any()
    assert sampling.step_noise_table("euler", x, sigmas) is None and sampling.step_noise_table("dpmpp_2m", x, sigmas) is None
    assert sampling.step_noise_table("dpmpp_2m_sde", x, sigmas, eta=0.0) is None
    # the pipeline's seeded Brownian sampler (sampler_opt brownian_noise) rides in the same way
    ns = sampling.BrownianTreeNoiseSampler(x, sigmas[-2], sigmas[0], seed=5)
    ref = sampling.BrownianTreeNoiseSampler(x, sigmas[-2], sigmas[0], seed=5)
    tab = sampling.step_noise_table("euler_ancestral", x, sigmas, noise_sampler=ns)
    assert torch.equal(tab[2], [ref(sigmas[i], sigmas[i + 1]) for i in range(3)][2])


# ----------------------------------------------------------------------------- serving host logic
LinearExec = FakeExec


def _pipe(prediction_type="epsilon"):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    unet = UNet2DConditionModel(UNetConfig.tiny()).half()
    return StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler(prediction_type=prediction_type))


@pytest.fixture(scope="module")
def pipe():
    return _pipe()


def test_launch_choice_and_records_per_transition(pipe):
    """A (DPM++ 2M, 5 steps) alone: the old launch.  B (Euler a, 3 steps) joins: every transition in which B steps is the
    linear launch, A's records in it carry no c_skip / c_out (the wrapper's eps-prediction defaults); after B leaves the old
    launch is back.  B's records: its coefficients, eps-prediction scalars, noise row j for step j, none on the last."""
    ex = LinearExec()
    b = ServingBatcher(pipe, 128, 128, executor=ex, max_batch=2, buckets=(1, 2))
    b.submit(_req("A", steps=5))
    b.step()
    b.step()
    assert len(ex.transitions) == 2 and not ex.linear
    fb = b.submit(_req("B", steps=3, sampler_name="sample_euler_ancestral", eta=0.8, s_noise=1.05))
    assert ex.noise_tables == {"B": 0.8}
    b.step()                                            # B joins while A steps: still the old launch (no B step in it)
    assert len(ex.transitions) == 3 and not ex.linear
    for _ in range(3):
        b.step()
    assert len(ex.linear) == 3 and len(ex.transitions) == 3 and fb.done()
    b.run_until_idle()
    assert len(ex.linear) == 3 and b.stats()["linear_transitions"] == 3
    assert len(ex.transitions) + len(ex.linear) == b.stats()["steps"] + 1       # (the last transition runs no step)
    rb = [t[2][1] for t in ex.linear]
    sig = rb[0]["req"].sig
    want = sampling.linear_step_coefficients("euler_ancestral", sig, eta=0.8, s_noise=1.05)
    for j, (rec, (a, b_, c, s)) in enumerate(zip(rb, want)):
        assert (rec["a"], rec["b"], rec["c"], rec["s"]) == (a, b_, c, s) and rec["step"] == j
        assert rec["c_skip"] == 1.0 and rec["c_out"] == -sig[j]
        assert rec["noise"] == (("noise", "B", j) if j < 2 else None)
    for t in ex.linear:
        assert "c_skip" not in t[2][0] and t[2][0]["mode"] == ops.ROW_STEP


def test_all_dpmpp_2m_batch_never_takes_the_linear_launch(pipe):
    ex = LinearExec()
    b = ServingBatcher(pipe, 128, 128, executor=ex, max_batch=4, buckets=(1, 2, 4))
    for n, steps in (("A", 4), ("B", 6), ("C", 3)):
        b.submit(_req(n, steps=steps, sampler_name="sample_dpmpp_2m" if n == "B" else None))
    b.run_until_idle()
    assert not ex.linear and not ex.noise_tables and b.stats()["linear_transitions"] == 0 and b.stats()["leaves"] == 3


def test_ode_and_eta_zero_requests_have_no_noise_table(pipe):
    ex = LinearExec()
    b = ServingBatcher(pipe, 128, 128, executor=ex, max_batch=4, buckets=(1, 2, 4))
    b.submit(_req("E", steps=3, sampler_name="euler"))
    b.submit(_req("S", steps=3, sampler_name=sampling.sample_dpmpp_2m_sde, eta=0.0, solver_type="heun"))
    b.submit(_req("L", steps=3, sampler_name=sx.sample_lcm))
    b.run_until_idle()
    assert list(ex.noise_tables) == ["L"] and len(ex.linear) == 3
    for t in ex.linear:
        assert all(r["noise"] is None for r in t[2][:2] if r["mode"] == ops.ROW_STEP)
    assert [r["a"] for t in ex.linear for r in t[2][2:3]] == [0.0, 0.0, 0.0]


def test_v_prediction_batcher_records():
    """every slot of a v-prediction pipeline goes through the linear launch with CompVisVDenoiser's scalars; with
    pass_kwargs = False the request's region tables are zero"""
    from test_serving_host import _masked
    vp = _pipe("v_prediction")
    ex = LinearExec()
    b = ServingBatcher(vp, 128, 128, executor=ex, max_batch=2, buckets=(1, 2))
    st, ids = _masked(2, 0.3)
    b.submit(_req("A", steps=3, state=st, ids=ids))
    b.step()
    r = b._slots[0]
    assert all(not w.any() for w in r.tables.values())
    b.run_until_idle()
    assert len(ex.linear) == 3 and len(ex.transitions) == 1            # the JOIN alone is the old launch (nothing steps)
    kdm = vp.k_diffusion_model
    for j, t in enumerate(ex.linear):
        rec = t[2][0]
        c_skip, c_out, c_in = (float(v) for v in kdm.get_scalings(torch.tensor(r.sig[j], dtype=torch.float64)))
        assert rec["c_skip"] == pytest.approx(c_skip, rel=1e-12) and rec["c_out"] == pytest.approx(c_out, rel=1e-12)
        assert rec["noise"] is None and rec["s"] == 0.0
        if j:
            assert ex.linear[j - 1][2][0]["c_in_next"] == pytest.approx(c_in, rel=1e-12)
    vp.k_diffusion_model.pass_kwargs = True
    try:
        b2 = ServingBatcher(vp, 128, 128, executor=LinearExec(), max_batch=2, buckets=(1, 2))
        b2.submit(_req("B", steps=2, state=st, ids=ids))
        b2.step()
        assert any(w.any() for w in b2._slots[0].tables.values())
    finally:
        vp.k_diffusion_model.pass_kwargs = False


def test_submit_rejections_name_the_key(pipe):
    b = ServingBatcher(pipe, 128, 128, executor=LinearExec(), max_batch=2, buckets=(1, 2))
    for bad in ("sample_heun", sampling.sample_dpmpp_sde, "sample_dpmpp_3m_sde", sx.restart_sampler):
        with pytest.raises(ValueError, match="sampler_name"):
            b.submit(_req("X", sampler_name=bad))
    img, mask = torch.zeros(1, 4, 16, 16), torch.ones(1, 1, 128, 128)
    with pytest.raises(ValueError, match="mask_image"):
        b.submit(_req("X", sampler_name="sample_euler", image=img, mask_image=mask))
    with pytest.raises(ValueError, match="step_noise"):
        b.submit(_req("X", steps=4, sampler_name="lcm", step_noise=torch.zeros(3, 1, 4, 16, 16)))
    with pytest.raises(ValueError, match="step_noise"):
        b.submit(_req("X", steps=4, sampler_name="lcm", step_noise=torch.zeros(4, 2, 4, 16, 16)))
    with pytest.raises(ValueError, match="solver_type"):
        b.submit(_req("X", sampler_name="dpmpp_2m_sde", solver_type="rk4"))
    vb = ServingBatcher(_pipe("v_prediction"), 128, 128, executor=LinearExec(), max_batch=2, buckets=(1, 2))
    with pytest.raises(ValueError, match="mask_image"):
        vb.submit(_req("X", image=img, mask_image=mask))
    b.submit(_req("ok", steps=4, sampler_name="lcm", step_noise=torch.zeros(4, 1, 4, 16, 16)))


def test_fused_true_with_an_unsupported_sampler_raises(pipe):
    emb = torch.zeros(1, 77, 64).half()
    with pytest.raises(NotImplementedError, match="sample_heun"):
        pipe.txt2img(None, height=128, width=128, num_inference_steps=2, sampler_name="sample_heun", fused=True,
                     prompt_embeds=emb, negative_prompt_embeds=emb, output_type="latent", latents=torch.zeros(1, 4, 16, 16).half())


def test_inpainting_and_other_samplers_never_share_a_batch(pipe):
    """the known-region launch carries DPM++ 2M records only (no c_skip / c_out / noise), so whichever of an inpainting request
    and a request of another sampler comes second waits at the head of the queue until the others have left; DPM++ 2M requests
    share a batch with either"""
    import test_serving_img_host as ih

    class Exec(ih.FakeImgExec):
        def transition(self, n_src, n_dst, recs, known=None):
            launch = step_launch(recs, known)
            if launch == "linear":
                assert not any(rec.get("req") is not None and rec["req"].kind == "inpaint" for rec in recs)
            if launch == "known":
                assert not any(rec["mode"] == ops.ROW_STEP and "c_skip" in rec for rec in recs)
            super().transition(n_src, n_dst, recs, known)

    ex = Exec()
    b = ServingBatcher(pipe, 128, 128, executor=ex, max_batch=4, buckets=(1, 2, 4))
    names = lambda: [None if r is None else r.req["name"] for r in b._slots]          # noqa: E731
    b.submit(ih._req("I", steps=3, image=ih.LAT, mask_image=ih.MASK))
    b.submit(ih._req("E", steps=2, latents=ih.LAT, sampler_name="sample_euler_ancestral"))
    b.submit(ih._req("M", steps=2, latents=ih.LAT))
    b.step()
    assert names() == ["I", None, None, None] and b.stats()["queued"] == 2           # E waits, and M behind it (FIFO)
    for _ in range(3):
        b.step()
    assert names()[0] is None                                                         # I has left ...
    b.step()
    assert names()[:2] == ["E", "M"]                                                  # ... E and M come in together
    b.submit(ih._req("J", steps=2, image=ih.LAT, mask_image=ih.MASK))
    b.step()
    assert "J" not in names() and b.stats()["queued"] == 1                            # the reverse: J waits for E
    b.run_until_idle()
    assert b.stats()["leaves"] == 4 and len(ex.linear) == 2
    b.submit(ih._req("K", steps=2, image=ih.LAT, mask_image=ih.MASK))
    b.submit(ih._req("N", steps=2, latents=ih.LAT, sampler_name="dpmpp_2m"))
    b.step()
    assert names()[:2] == ["K", "N"]                                                  # DPM++ 2M rides beside inpainting as before
    b.run_until_idle()


def test_callables_are_taken_where_names_are():
    sig = _sigmas("karras", 5).tolist()
    for fam, fn in FUNCS.items():
        assert sampling.linear_step_coefficients(fn, sig) == sampling.linear_step_coefficients(fam, sig)
    x = torch.zeros(1, 4, 2, 2)
    torch.manual_seed(3)
    a = sampling.step_noise_table(sx.sample_lcm, x, sig)
    torch.manual_seed(3)
    assert torch.equal(a, sampling.step_noise_table("lcm", x, sig))
    with pytest.raises(NotImplementedError, match="sample_heun"):
        sampling.linear_step_coefficients(sampling.sample_heun, sig)


def test_fused_per_row_path_refuses_more_images_than_slots(pipe):
    emb = torch.zeros(1, 77, 64).half()
    with pytest.raises(NotImplementedError, match="fused=False"):
        pipe.txt2img(None, height=128, width=128, num_inference_steps=2, sampler_name="sample_euler", fused=True,
                     num_images_per_prompt=ops.ROW_STEP_MAX_SLOTS + 1, prompt_embeds=emb, negative_prompt_embeds=emb,
                     output_type="latent", latents=torch.zeros(ops.ROW_STEP_MAX_SLOTS + 1, 4, 16, 16).half())
