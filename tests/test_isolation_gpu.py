"""Row isolation on the MI355X (`-m gpu`): every batched kernel of tests/isolation_cases.py under tests/isolation.py's four hostile
patterns, then the same property through the continuous batcher.

Per case: the benign operands twice (equal bits), then the victim image's activations overwritten with NaN, +inf, +-65504 and NaN in
its first and last row only - same shapes, strides and launch knobs.  Every output element of the other images keeps the bits of
the benign run (`torch.equal` on bit views, no tolerance), and under NaN every output element of the victim is NaN unless the
case states another contract.  Each case asserts the route it took: a fallback to torch never passes silently.

Hostile data are values only - never an index, a gate, a record or an address.
"""
import pytest
import torch

import isolation as iso
import isolation_cases as IC

pytestmark = pytest.mark.gpu

# dsc_debug_set_gemm_stages settings of tests/test_guard_bands_gpu.py: ring depth, 64- / 128-row tiles, loader waves, 128-column
# tiles, workgroup order.  GEGLU has no 64-row tiles.
GEMM_STAGES = (0, 90643, 40643, 90642, 91283, 41283, 90002, 200000, 291282, 1000000, 2000000)
GEMM_STAGES_64_ROWS = (90643, 40643, 90642)
GN_MODES = (("auto", (11, 0)), ("two launches", (11, 2)), ("wide bundle", (11, 3)), ("three launches", (11, 4)), ("no slabs", (0, 10)))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from diffusionspatialcontrol_amd import _lib
    return _lib.load_library()


def _check(case, ops, lib):
    operands = {n: t.cuda() for n, t in case.operands.items()}
    got = iso.check_isolated(case.make_run(ops, lib), operands, case.owners, case.j, B=case.B, seam_axes=case.seam_axes,
                             victim_rules=case.victim_rules, frozen=case.frozen)
    assert set(got["benign"]) == set(case.outputs)
    return got


def _settings(case, ops, lib):
    """(name, apply) for every launch setting the case is repeated under, and the call that restores the measured rule"""
    profile = lambda name: (lambda: ops.set_tuning_profile(name))
    if case.sweep in ("stages", "stages_no64", "stages_gn"):
        knobs = [k for k in GEMM_STAGES if not (case.sweep == "stages_no64" and k in GEMM_STAGES_64_ROWS)]
        return [(f"stages {k}", (lambda k=k: lib.dsc_debug_set_gemm_stages(k))) for k in knobs], lambda: lib.dsc_debug_set_gemm_stages(0)
    if case.sweep in ("profile", "conv"):
        return [("latency", profile("latency")), ("throughput", profile("throughput"))], profile("latency")
    if case.sweep in ("gn", "gn_cat"):
        modes = GN_MODES if case.sweep == "gn" else tuple((str(m), (m,)) for m in (0, 2, 4))
        return ([(name, (lambda calls=calls: [lib.dsc_debug_set_gn_mode(m) for m in calls])) for name, calls in modes],
                lambda: [lib.dsc_debug_set_gn_mode(m) for m in (11, 0)])
    if case.sweep == "sa_variants":
        return ([(f"variant {v}", (lambda v=v: lib.dsc_debug_set_self_attn_variant(v))) for v in range(1, 19)],
                lambda: lib.dsc_debug_set_self_attn_variant(0))
    assert case.sweep == ""
    return [("", lambda: None)], lambda: None


CASES = [c for c in IC.all_cases() if c.family not in ("gemm_lt",)]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_kernel_rows_are_isolated(ops, lib, case):
    settings, restore = _settings(case, ops, lib)
    ran = 0
    try:
        for name, apply in settings:
            apply()
            if case.sweep == "stages_gn" and lib.dsc_linear_gn_rows(*case.gn_dims) == 0:
                continue                                   # a tile height that does not divide the image's rows: refused before any launch
            try:
                _check(case, ops, lib)
            except AssertionError as e:
                raise type(e)(f"[{name}] {e}") from None
            ran += 1
    finally:
        restore()
    assert ran >= (5 if case.sweep == "stages_gn" else len(settings))


def test_library_gemm_rows_are_isolated(ops, lib):
    """dsc_linear_lt_f16 where the build has the library GEMM; a build without it refuses before any launch"""
    (case,) = [c for c in IC.all_cases() if c.family == "gemm_lt"]
    if not lib.dsc_has_library_gemm():
        with pytest.raises(AssertionError, match="-2"):
            case.make_run(ops, lib)({n: t.cuda() for n, t in case.operands.items()})
        return
    _check(case, ops, lib)


# ============================================================================= the same property through the batcher
OPT = {"scheduler": "karras"}


def _hostile(req, latents=None, embeds=None):
    """the request with its start latents and / or prompt rows overwritten: same shapes, region state, steps, guidance and
    schedule, so the launch geometry and every host decision are those of the benign run"""
    r = dict(req)
    if latents is not None:
        r["latents"] = torch.full_like(req["latents"], latents)
    if embeds is not None:
        r["prompt_embeds"] = torch.full_like(req["prompt_embeds"], embeds)
    return r


def _same_bits(a, b):
    return torch.equal(iso.bits(a), iso.bits(b))


def test_batcher_requests_together_are_isolated():
    """four requests submitted before the first step, 5 steps, on ONE warm batcher: benign, request 2 with NaN start latents,
    request 2 with +inf prompt rows, benign again.  The other three final latents carry the benign bits in every run - in the last
    one after every static row (x, old, x_in, tadd, the text rows) has held a diverged tenant - and the victim's result is NaN"""
    import test_serving_gpu as ts
    cfg, pipe = ts._tiny_pipe(1)
    reqs = ts._tiny_requests(cfg.cross_attention_dim, 4)
    b = pipe.serve(128, 128, max_batch=4, buckets=(1, 2, 4)).warm()

    def run(batch):
        futs = [b.submit(dict(r, num_inference_steps=5, guidance_scale=7.5, sampler_opt=OPT)) for r in batch]
        b.run_until_idle()
        return [f.result().cpu() for f in futs]
    benign = run(reqs)
    assert all(bool(torch.isfinite(o).all()) for o in benign)
    nan_lat = run(reqs[:2] + [_hostile(reqs[2], latents=float("nan"))] + reqs[3:])
    inf_emb = run(reqs[:2] + [_hostile(reqs[2], embeds=float("inf"))] + reqs[3:])
    after = run(reqs)
    for i in (0, 1, 3):
        assert _same_bits(nan_lat[i], benign[i]), ("NaN latents", i, (nan_lat[i].float() - benign[i].float()).abs().max().item())
        assert _same_bits(inf_emb[i], benign[i]), ("+inf prompt rows", i, (inf_emb[i].float() - benign[i].float()).abs().max().item())
    assert bool(torch.isnan(nan_lat[2]).all())
    assert not bool(torch.isfinite(inf_emb[2]).any())
    for i in range(4):
        assert _same_bits(after[i], benign[i]), ("slots reused after a diverged tenant", i)
    assert b.stats()["captures_after_warm"] == 0


def test_coalesced_requests_are_isolated():
    """the same NaN-latents pair through txt2img_coalesced"""
    import test_serving_gpu as ts
    cfg, pipe = ts._tiny_pipe(1)
    reqs = ts._tiny_requests(cfg.cross_attention_dim, 4)
    run = lambda batch: [o.cpu() for o in pipe.txt2img_coalesced(batch, height=128, width=128, num_inference_steps=5, guidance_scale=7.5,  # noqa: E731
                                                                  sampler_opt=OPT, output_type="latent")]
    benign = run(reqs)
    got = run(reqs[:2] + [_hostile(reqs[2], latents=float("nan"))] + reqs[3:])
    for i in (0, 1, 3):
        assert _same_bits(got[i], benign[i]), i
    assert bool(torch.isnan(got[2]).all()) and all(bool(torch.isfinite(o).all()) for o in benign)


def _reuse(b, tenants, Bq, C, overlap, n_slots):
    """The first tenants (4 steps each) start together and leave; B and C follow into slots that held them.  Which slot a request
    gets is the batcher's business, so the tenants are as many as makes the answer the same for every choice (the batcher is
    watched through stats() alone):
    overlap      n_slots - 1 tenants; C (10 steps) joins after two steps into the one slot left, the tenants leave, B joins while
                 C is mid-run - every free slot was a tenant's;
    otherwise    n_slots tenants run alone and leave: every slot was a tenant's; C joins, B two steps later beside it.
    -> (the tenants' final latents, B's, C's)"""
    assert len(tenants) == (n_slots - 1 if overlap else n_slots)
    left = b.stats()["leaves"]
    fts = [b.submit(dict(t, num_inference_steps=4)) for t in tenants]
    b.step()
    assert b.stats()["active"] == len(tenants)
    if overlap:
        b.step()
        fc = b.submit(dict(C, num_inference_steps=10))
        b.step()
        assert b.stats()["active"] == n_slots                    # C took the one slot no tenant holds
    for _ in range(6):                                           # the tenants' remaining steps
        if b.stats()["leaves"] == left + len(tenants) or not b.step():
            break
    assert b.stats()["leaves"] == left + len(tenants)            # every tenant has left
    if overlap:
        assert b.stats()["active"] == 1                          # C is mid-run
    else:
        assert b.stats()["active"] == 0
        fc = b.submit(dict(C, num_inference_steps=10))
        b.step()
        b.step()
    fb = b.submit(dict(Bq, num_inference_steps=5))
    b.step()
    assert b.stats()["active"] == 2                              # B runs beside C, both where a tenant sat
    b.run_until_idle()
    return [f.result().cpu() for f in fts], fb.result().cpu(), fc.result().cpu()


@pytest.mark.parametrize("overlap", [True, False])
def test_batcher_slot_reuse_after_a_diverged_tenant(overlap):
    """B's and C's final latents are bit-equal between the run where the first tenants were benign and the run where their latents
    were NaN and their prompt rows +inf: nothing they left in old, mid, x_in, tadd or the text rows reaches the next tenant of a
    slot or its neighbour"""
    import test_serving_gpu as ts
    cfg, pipe = ts._tiny_pipe(2)
    reqs = [dict(r, guidance_scale=7.5, sampler_opt=OPT) for r in ts._tiny_requests(cfg.cross_attention_dim, 6)]
    tenants, Bq, C = reqs[:3 if overlap else 4], reqs[4], reqs[5]
    b = pipe.serve(128, 128, max_batch=4, buckets=(1, 2, 4)).warm()
    benign = _reuse(b, tenants, Bq, C, overlap, 4)
    hostile = _reuse(b, [_hostile(t, latents=float("nan"), embeds=float("inf")) for t in tenants], Bq, C, overlap, 4)
    again = _reuse(b, tenants, Bq, C, overlap, 4)
    assert all(bool(torch.isnan(o).all()) for o in hostile[0]) and all(bool(torch.isfinite(o).all()) for o in benign[0] + [benign[1], benign[2]])
    for name, i in (("B", 1), ("C", 2)):
        assert _same_bits(hostile[i], benign[i]), (name, "beside / after the diverged tenants")
        assert _same_bits(again[i], benign[i]), (name, "one generation after the diverged tenants")
    assert all(_same_bits(x, y) for x, y in zip(again[0], benign[0]))
    assert b.stats()["captures_after_warm"] == 0


def test_batcher_stale_lane_rows_behind_a_closed_gate():
    """the T2I-Adapter lane (tests/test_t2i_serving_gpu.py's tiny setup): A carries a control image - in the hostile run a NaN
    image, NaN latents and +inf prompt rows - and leaves; the lane-less B and C run in and beside its slot with their gates 0.
    The adapter's feature rows still hold what A left: B and C carry the bits of the run where A was benign"""
    import test_t2i_serving_gpu as t2
    from diffusionspatialcontrol_amd.modules import t2i_adapter as t2i
    tn = t2._setup()
    ad, _ = t2._adapter(tn.cfg, 9)
    t2i.setup_model_t2i_adapter(tn.pipe, ad)
    b = tn.pipe.serve(128, 128, max_batch=2, buckets=(1, 2), t2i_adapter=True).warm()
    A, Bq, C = (dict(tn.base, latents=t2._latents(seed).cuda()) for seed in (11, 12, 13))
    img = t2._image(10)
    with_lane = lambda r, image: dict(r, image_t2i_adapter=image, adapter_conditioning_scale=0.8)          # noqa: E731
    benign = _reuse(b, [with_lane(A, img)], Bq, C, True, 2)      # two slots: C holds one, so B sits where A sat
    hostile = _reuse(b, [with_lane(_hostile(A, latents=float("nan"), embeds=float("inf")), torch.full_like(img, float("nan")))], Bq, C, True, 2)
    plain = _reuse(b, [A], Bq, C, True, 2)
    assert bool(torch.isnan(hostile[0][0]).all()) and all(bool(torch.isfinite(o).all()) for o in (benign[0][0], benign[1], benign[2]))
    assert not _same_bits(benign[0][0], plain[0][0])             # the lane was live on A
    for name, i in (("B", 1), ("C", 2)):
        assert _same_bits(hostile[i], benign[i]) and _same_bits(plain[i], benign[i]), name
    assert b.stats()["captures_after_warm"] == 0
