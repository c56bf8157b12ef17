"""Guidance rescale (arXiv 2305.08891 sec. 3.4) inside the per-row sampler step on the MI355X (`-m gpu`):
dsc_cfg_linear_step_rows_rescale against its header formulas and against dsc_cfg_linear_step_rows bit for bit where phi == 0, the
fused loop with `guidance_rescale` against protocol mode's eager rescale_noise_cfg, and the continuous batcher serving it per
request."""
import ctypes
import functools
import math
import os
import re
import subprocess
import tempfile

import pytest
import torch

import diffusionspatialcontrol_amd as dsc
from test_linear_step_gpu import _recs, _replay, _sampler, _table, _toy
from test_serving_gpu import _h, _params, _tiny_pipe, _tiny_requests  # noqa: F401
from test_serving_img_gpu import _f32, _fma, _gen, _ulps

pytestmark = pytest.mark.gpu
TW = 96
G = 7.5
# one vector; four full vectors per wave; one vector past 256 threads; one vector past the 1024 threads of an owned slot's
# workgroup (the second pass of its loops has one live lane); the production row
CHWS = [8, 1024, 2056, 8200, 16384]
NAMES = ("x", "old", "x_in", "t", "sigma_groups", "tadd")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- a. the kernel
def _call(fn, chw, x, eps, old, n_src, n_dst, recs):
    x, old = x.clone(), old.clone()
    x_in = torch.full((2 * n_dst, chw), 7.0, dtype=torch.float16, device="cuda")
    t = torch.full((2 * n_dst,), -1.0, device="cuda")
    s = torch.full((n_dst,), -1.0, device="cuda")
    tadd = torch.zeros(2 * n_dst, TW, dtype=torch.float16, device="cuda")
    fn(x, eps, old, n_src, x_in, t, s, recs, tadd=tadd)
    torch.cuda.synchronize()
    return x, old, x_in, t, s, tadd


def _restate(x, eu, ec, old, p, noise, phi):
    """include/dsc_hip.h's formulas for one STEP slot with phi > 0: fp32 fma for Dc / Dg, float64 sums, K cast to fp32
    -> (x', old', x_in row, K)"""
    x, eu, ec, old = (v.float().cpu() for v in (x, eu, ec, old))
    g, a, b, c, cn, cs, co, s = (_f32(p[k]).float() for k in ("guidance", "a", "b", "c", "c_in_next", "c_skip", "c_out", "s"))
    e = _fma(g, ec - eu, eu)
    sx = cs * x
    dc, dg = _fma(co, ec, sx).double(), _fma(co, e, sx).double()
    n = float(x.numel())
    ssd_c = (dc * dc).sum().item() - dc.sum().item() ** 2 / n
    ssd_g = (dg * dg).sum().item() - dg.sum().item() ** 2 / n
    phi = float(_f32(phi))
    k = torch.tensor(phi * math.sqrt(ssd_c / ssd_g) + (1.0 - phi), dtype=torch.float64).float()
    d = (k * dg.float()).half().float()
    xn = _fma(c, old, _fma(a, x, b * d))
    if noise is not None:
        xn = _fma(s, noise.float().cpu(), xn)
    xn = xn.half().float()
    return xn.half(), d.half(), (xn * cn).half(), k.item()


def _set_v(rec):
    sg = rec["sigma"]
    rec.update(c_skip=1.0 / (sg * sg + 1.0), c_out=-sg / math.sqrt(sg * sg + 1.0))


@pytest.mark.parametrize("phis", [(0.7, 0.0, 1.0, 0.25), (0.0, 1.0, 0.25, 0.7)])
@pytest.mark.parametrize("chw", CHWS)
def test_rescaled_slots_against_the_formulas(ops, chw, phis):
    """slots "SSJSIS" (n_src 6, n_dst 5): 0 v-prediction scalars with a noise row, 1 v without, 2 JOIN, 3 eps-prediction with
    noise, 4 IDLE, 5 a leaving slot (i >= n_dst) with noise; the STEP slots take `phis` in order, so over the two assignments
    each of them runs rescaled and slots 0 and 1 also with phi = 0.  g = 7.5 on independent m_u / m_c: K is far from 1.
    Rescaled slots: at most 1 fp16 ulp from the restated formulas in x', old and the x_in rows (the sibling kernels' bound: K
    can differ from the kernel's by the fp64 summation order only) and another x' than the phi = 0 launch's; phi = 0, JOIN and
    IDLE slots, t_buf, sigma_groups and tadd: dsc_cfg_linear_step_rows' bits"""
    modes, n_src, n_dst = "SSJSIS", 6, 5
    x, eps, old = _h(6, chw, seed=61), _h(12, chw, seed=62), _h(6, chw, seed=63)
    tabs = [_h(TW, seed=70 + i) for i in range(6)]
    noise = _h(6, chw, seed=64)
    recs = _recs(ops, modes, tabs)
    for r in recs:
        r["guidance"] = G
    recs[5].update(c_in_next=0.0, t_next=0.0, sigma_next=1.0, temb_row=None)
    for i in (0, 1, 5):
        _set_v(recs[i])
    recs[3].update(c_skip=1.0, c_out=-recs[3]["sigma"])
    for i in (0, 3, 5):
        recs[i].update(s=0.3 + 0.1 * i, noise=noise[i])
    recs[1].update(s=5.0, noise=None)
    plain = _call(ops.cfg_linear_step_rows, chw, x, eps, old, n_src, n_dst, recs)
    phi_of = dict(zip((0, 1, 3, 5), phis))
    resc = [dict(r, rescale=phi_of[i]) if i in phi_of else r for i, r in enumerate(recs)]
    got = _call(ops.cfg_linear_step_rows, chw, x, eps, old, n_src, n_dst, resc)
    for i, phi in phi_of.items():
        if phi == 0.0:
            continue
        xn, d, xi, k = _restate(x[i], eps[i], eps[n_src + i], old[i], recs[i], recs[i]["noise"], phi)
        u = [_ulps(got[0][i], xn), _ulps(got[1][i], d)]
        if i < n_dst:
            u += [_ulps(got[2][i], xi), _ulps(got[2][n_dst + i], xi)]
        print(f"chw {chw} slot {i} phi {phi}: K = {k:.6f}, ulps x' / old / x_in = {u}")
        assert max(u) <= 1, (i, u)
        assert not torch.equal(got[0][i], plain[0][i]) and abs(k - 1.0) > 1e-2, (i, k)
    for i in [j for j in range(6) if phi_of.get(j, 0.0) == 0.0]:
        assert torch.equal(got[0][i], plain[0][i]) and torch.equal(got[1][i], plain[1][i]), i
        if i < n_dst:
            assert torch.equal(got[2][[i, n_dst + i]], plain[2][[i, n_dst + i]]), i
    assert torch.equal(got[3], plain[3]) and torch.equal(got[4], plain[4]) and torch.equal(got[5], plain[5])


@pytest.mark.parametrize("chw", CHWS)
@pytest.mark.parametrize("n_src, n_dst, modes", [(2, 4, "SSJI"), (4, 2, "SISI"), (4, 4, "JSIS"), (3, 3, "SSS")])
def test_all_phi_zero_is_the_linear_op(ops, chw, n_src, n_dst, modes):
    """the new entry itself with every phi zero (given, and left out): every output buffer carries dsc_cfg_linear_step_rows'
    bits - and the wrapper, seeing no phi > 0, does not even call it"""
    n = len(modes)
    x, eps, old = _h(n, chw, seed=31), _h(2 * n_src, chw, seed=32), _h(n, chw, seed=33)
    tabs = [_h(TW, seed=40 + i) for i in range(n)]
    noise = _h(n, chw, seed=34)
    recs = _recs(ops, modes, tabs)
    for i, r in enumerate(recs):
        if i % 2:
            _set_v(r)
            r.update(s=0.4, noise=noise[i])
    plain = _call(ops.cfg_linear_step_rows, chw, x, eps, old, n_src, n_dst, recs)
    for variant in (recs, [dict(r, rescale=0.0) for r in recs]):
        got = _call(ops.cfg_linear_step_rows_rescale, chw, x, eps, old, n_src, n_dst, variant)
        for name, a, b in zip(NAMES, got, plain):
            assert torch.equal(a, b), (modes, name)


def test_sixteen_owned_slots_twice(ops):
    """chw = 16384, 16 STEP slots all rescaled: the row of every slot belongs to one workgroup, so two launches on the same
    inputs give the same bits and each slot is the restated formula's (a workgroup that read x another had already updated
    would miss both)"""
    chw, n = 16384, 16
    x, eps, old = _h(n, chw, seed=81), _h(2 * n, chw, seed=82), _h(n, chw, seed=83)
    tabs = [_h(TW, seed=90 + i) for i in range(n)]
    recs = _recs(ops, "S" * n, tabs)
    for i, r in enumerate(recs):
        r.update(guidance=G, rescale=(0.7, 1.0, 0.25, 0.5)[i % 4], c_skip=1.0, c_out=-r["sigma"], s=0.0, noise=None)
        if i % 2:
            _set_v(r)
    first = _call(ops.cfg_linear_step_rows, chw, x, eps, old, n, n, recs)
    second = _call(ops.cfg_linear_step_rows, chw, x, eps, old, n, n, recs)
    for name, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), name
    worst = 0
    for i in range(n):
        xn, d, xi, _ = _restate(x[i], eps[i], eps[n + i], old[i], recs[i], None, recs[i]["rescale"])
        worst = max(worst, _ulps(first[0][i], xn), _ulps(first[1][i], d), _ulps(first[2][i], xi), _ulps(first[2][n + i], xi))
    print(f"16 owned slots: worst ulps {worst}")
    assert worst <= 1


def test_argument_status(ops):
    """every call below is refused before a launch (the pointers are not real)"""
    lib = dsc.load_library()
    d = ctypes.c_void_p(0x1000)
    nan = float("nan")

    def call(recs, phis=None, n_src=2, n_dst=2, **kw):
        arr = (ops.RowLinear * len(recs))(*recs)
        ph = (ctypes.c_float * len(recs))(*(phis if phis is not None else [0.5] * len(recs)))
        return lib.dsc_cfg_linear_step_rows_rescale(
            kw.get("x", d), kw.get("eps", d), d, n_src, kw.get("x_in", d), d, d, kw.get("tadd", d), kw.get("tw", 96), n_dst,
            ctypes.cast(arr, ctypes.c_void_p), kw.get("rescale", ctypes.cast(ph, ctypes.c_void_p)), kw.get("n_slots", len(recs)),
            kw.get("chw", 1024), kw.get("dtype", 0), None)

    def rec(mode, temb=None, noise=None):
        return ops.RowLinear(mode, 1.0, 7.5, 0.5, 0.5, 0.0, 1.0, 10.0, 1.0, 1.0, -1.0, 0.1, temb, noise)
    step, join, idle = rec(ops.ROW_STEP), rec(ops.ROW_JOIN), rec(ops.ROW_IDLE)
    assert call([step, step], x=None) == -1 and call([step, step], x_in=None) == -1         # null pointers
    assert call([step, step], rescale=None) == -1                                           # ... the phi array among them
    assert call([step, step], x=ctypes.c_void_p(0x1004)) == -2                              # misaligned
    assert call([step, step], eps=ctypes.c_void_p(0x1008)) == -2
    assert call([step, step], chw=1020) == -2 and call([step, step], dtype=3) == -2
    assert call([step, step], eps=None) == -1                                               # STEP needs the model output
    assert call([step, step, step], n_src=2, n_dst=2) == -1                                 # STEP beyond n_src
    assert call([idle, idle, join], n_src=3, n_dst=2) == -1                                 # JOIN beyond n_dst
    assert call([rec(5), idle]) == -1                                                       # unknown mode
    assert call([step], n_dst=2) == -1                                                      # fewer records than rows
    assert call([idle] * 17, n_src=0, n_dst=1) == -1                                        # more than DSC_ROW_STEP_MAX_SLOTS
    assert call([rec(ops.ROW_STEP, noise=0x2004), step]) == -2                              # misaligned noise row
    assert call([rec(ops.ROW_STEP, temb=0x2004), step]) == -2                               # misaligned embedding row
    assert call([rec(ops.ROW_STEP, temb=0x2000), step], tadd=None) == -1                    # a row but no destination
    assert call([rec(ops.ROW_STEP, temb=0x2000), step], tw=100) == -2
    for bad in (-0.1, 1.5, nan):                                                            # phi of a STEP slot
        assert call([step, step], phis=[0.5, bad]) == -1 and call([step, idle], phis=[bad, 0.0]) == -1, bad
    assert ctypes.sizeof(ops.RowLinear) == 64                                               # phi rides beside the records


def test_code_object_has_no_scratch_or_spill():
    """device-only compile of csrc/sampler.hip with the build's flags: the rescale kernel's metadata"""
    root = os.path.dirname(os.path.dirname(dsc.lib_path()))
    with tempfile.TemporaryDirectory() as tmp:
        work = os.path.join(tmp, "sampler.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only",
                               "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "diffusionspatialcontrol_amd", "csrc"),
                               "-S", os.path.join(root, "diffusionspatialcontrol_amd", "csrc", "sampler.hip"), "-o", work],
                              stderr=subprocess.DEVNULL)
        listing = open(work).read()
    notes = listing[listing.index("amdhsa.kernels:"):]
    kernels = re.findall(r"\.name:\s+(\S*linear_rows_rescale_kernel\S*)(.*?)\.wavefront_size", notes, flags=re.S)
    assert len(kernels) == 1
    body = kernels[0][1]
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", body)
    assert re.search(r"\.vgpr_spill_count:\s+0\b", body) and re.search(r"\.sgpr_spill_count:\s+0\b", body)


# ----------------------------------------------------------------------------- b. the fused loop on the toy UNet
PHI = 0.7
FUSED_G, EMB_SCALE = 7.5, 4.0
FUSED_CASES = [("epsilon", "sample_dpmpp_2m"), ("epsilon", "sample_euler_ancestral"), ("v_prediction", "sample_euler")]


def _toy_case(prediction_type):
    pipe, kw, table, _ = _toy(prediction_type, seed=5 if prediction_type == "v_prediction" else 1000)
    kw = dict(kw, guidance_scale=FUSED_G, prompt_embeds=kw["prompt_embeds"] * EMB_SCALE)
    return pipe, kw, table


def _run(pipe, kw, name, table, fused, phi):
    fn, opt = _sampler(name), {"scheduler": "karras"}
    extra = {} if phi is None else {"guidance_rescale": phi}
    if name != "sample_euler_ancestral":
        return pipe.txt2img(None, fused=fused, sampler_name=fn, sampler_opt=opt, **extra, **kw)[0].float().cpu()
    if fused:
        return pipe.txt2img(None, fused=True, sampler_name=fn, sampler_opt=opt, step_noise=table, **extra, **kw)[0].float().cpu()
    proto_fn = functools.partial(fn, noise_sampler=_replay(table))
    return pipe.txt2img(None, fused=fused, sampler_name=proto_fn, sampler_opt=opt, **extra, **kw)[0].float().cpu()


@pytest.mark.parametrize("prediction_type, name", FUSED_CASES)
def test_fused_rescale_equals_protocol(ops, prediction_type, name):
    """6 steps on the toy UNet (16x16 latents): txt2img(fused=True, guidance_rescale=0.7) against fused=False - protocol
    mode's eager rescale_noise_cfg - within the sibling tests' bound for this comparison, 2e-2 of the result's scale.  Not
    vacuous: in protocol mode alone phi = 0.7 and phi = 0 are first shown to differ by more than three times that bound.
    Chosen: the toy's own guidance_scale 7.5 with the positive embeddings scaled by 4 (FUSED_G, EMB_SCALE above).  The random-init
    toy barely reads unscaled embeddings: on the fp32 CPU oracle (oracle/unet_ref.py, its CFG line given the same rescale) phi =
    0.7 and 0 then part by 1.2 % of the scale (eps, DPM++ 2M; K of the six steps 0.956, 0.998, 1.000 ..) and 3.4 % (v, Euler)
    - under the 6 % asked for.  With the embeddings x 4 the same oracle gives 35 % (K = 0.41, 0.85, 0.98, 1.00 ..) and 66 % (K =
    0.32, 0.33, 0.43, 0.67, 0.89, 0.98), and 24 - 28 % for the img2img case below; the test prints what the GPU gives."""
    pipe, kw, table = _toy_case(prediction_type)
    proto = _run(pipe, kw, name, table, False, PHI)
    proto0 = _run(pipe, kw, name, table, False, 0.0)
    scale = proto.abs().max().item()
    sep = (proto - proto0).abs().max().item()
    print(f"{prediction_type} {name}: protocol phi {PHI} vs 0: {sep:.3e} (scale {scale:.2f}, {sep / scale:.3f} of it)")
    assert sep > 3 * 2e-2 * scale, (sep, scale)
    fused = _run(pipe, kw, name, table, True, PHI)
    err = (fused - proto).abs().max().item()
    print(f"{prediction_type} {name}: fused vs protocol at phi {PHI}: {err:.3e} (scale {scale:.2f})")
    assert torch.isfinite(fused).all() and err < 2e-2 * scale, (err, scale)


def test_img2img_fused_rescale_equals_protocol(ops):
    """img2img at strength 0.6 of 8 steps, DPM++ 2M: the same two asserts"""
    pipe, kw, _ = _toy_case("epsilon")
    common = {k: v for k, v in kw.items() if k not in ("latents", "num_inference_steps", "eta")}
    lat0 = (torch.randn(1, 4, 16, 16, generator=_gen(21)) * 0.8).half()

    def run(fused, phi):
        return pipe.img2img(None, generator=_gen(33), fused=fused, sampler_name="sample_dpmpp_2m", latents=lat0.clone(),
                            strength=0.6, num_inference_steps=8, sampler_opt={"scheduler": "karras"}, guidance_rescale=phi,
                            **common)[0].float().cpu()
    proto, proto0 = run(False, PHI), run(False, 0.0)
    scale = proto.abs().max().item()
    sep = (proto - proto0).abs().max().item()
    print(f"img2img: protocol phi {PHI} vs 0: {sep:.3e} (scale {scale:.2f})")
    assert sep > 3 * 2e-2 * scale, (sep, scale)
    fused = run(True, PHI)
    err = (fused - proto).abs().max().item()
    print(f"img2img: fused vs protocol at phi {PHI}: {err:.3e} (scale {scale:.2f})")
    assert torch.isfinite(fused).all() and err < 2e-2 * scale, (err, scale)


def test_old_paths_are_untouched(ops):
    """fused=True with guidance_rescale=0.0 is the call without the keyword, bit for bit (DPM++ 2M's lockstep kernel and the
    per-row path); fused=None with a rescale still selects protocol mode"""
    pipe, kw, table = _toy_case("epsilon")
    for name in ("sample_dpmpp_2m", "sample_euler_ancestral"):
        assert torch.equal(_run(pipe, kw, name, table, True, 0.0), _run(pipe, kw, name, table, True, None)), name
    auto = _run(pipe, kw, "sample_dpmpp_2m", table, None, PHI)
    assert torch.equal(auto, _run(pipe, kw, "sample_dpmpp_2m", table, False, PHI))
    assert not torch.equal(auto, _run(pipe, kw, "sample_dpmpp_2m", table, None, None))


# ----------------------------------------------------------------------------- c. serving on the toy UNet
K = {"scheduler": "karras"}


def _own(pipe, r, steps, extra):
    return pipe.txt2img(None, height=128, width=128, num_inference_steps=steps, guidance_scale=G, fused=True,
                        sampler_name=_sampler(extra.get("sampler_name", "sample_dpmpp_2m")), eta=1.0, sampler_opt=K,
                        step_noise=extra.get("step_noise"), latents=r["latents"], region_map_state=r["region_map_state"],
                        prompt_embeds=r["prompt_embeds"], negative_prompt_embeds=r["negative_prompt_embeds"],
                        text_input_ids=r["text_input_ids"], output_type="latent",
                        **({"guidance_rescale": extra["guidance_rescale"]} if "guidance_rescale" in extra else {}))[0].float().cpu()


def _submit(b, r, steps, extra):
    return b.submit(dict(r, num_inference_steps=steps, guidance_scale=G, sampler_opt=K, **extra))


def test_batcher_mixed_rescales_equal_their_own_fused_txt2img(ops):
    """Two slots (buckets 1 / 2, the geometry at which test_batcher_mixed_samplers_equal_their_own_fused_txt2img asserts bit
    equality): A (DPM++ 2M, phi 0.7, 5 steps) starts; B (Euler a with a noise table, phi 0, 3 steps) joins 2 steps in; C
    (Euler, phi 0.3, 4 steps) waits for the first free slot.  Every latent is its own txt2img(fused=True,
    guidance_rescale=phi)'s, bit for bit - that test's bound; the phi = 0 request served alone equals the call without the key.
    Positive embeddings x EMB_SCALE, as in the fused tests, so that phi visibly moves a rescaled request's result"""
    cfg, pipe = _tiny_pipe(2)
    ra, rb, rc = (dict(r, prompt_embeds=r["prompt_embeds"] * EMB_SCALE) for r in _tiny_requests(cfg.cross_attention_dim, 3))
    specs = {"A": (ra, 5, {"guidance_rescale": 0.7}),
             "B": (rb, 3, {"sampler_name": "sample_euler_ancestral", "eta": 1.0, "step_noise": _table(3, 1), "guidance_rescale": 0.0}),
             "C": (rc, 4, {"sampler_name": "sample_euler", "guidance_rescale": 0.3})}
    b = pipe.serve(128, 128, max_batch=2, buckets=(1, 2)).warm()
    futs = {"A": _submit(b, *specs["A"])}
    for _ in range(3):
        b.step()
    futs["B"] = _submit(b, *specs["B"])
    futs["C"] = _submit(b, *specs["C"])
    b.step()
    assert b._slots[1] is not None and b._slots[1].family == "euler_ancestral" and b.stats()["queued"] == 1
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["joins"] == 3 and st["leaves"] == 3, st
    for n, (r, steps, extra) in specs.items():
        own = _own(pipe, r, steps, extra)
        got = futs[n].result().float().cpu()
        print(f"request {n}: vs its own fused txt2img {(got - own).abs().max().item():.3e}")
        assert torch.equal(got, own), n
        if extra["guidance_rescale"] > 0.0:            # (phi was live)
            bare = _own(pipe, r, steps, {k: v for k, v in extra.items() if k != "guidance_rescale"})
            assert (got - bare).abs().max().item() > 2e-2 * own.abs().max().item(), n
    r, steps, extra = specs["B"]
    alone = pipe.serve(128, 128, max_batch=2, buckets=(1, 2)).warm()
    f0 = _submit(alone, r, steps, extra)
    f1 = _submit(alone, r, steps, {k: v for k, v in extra.items() if k != "guidance_rescale"})
    alone.run_until_idle()
    assert torch.equal(f0.result(), f1.result())
    assert torch.equal(f0.result().float().cpu(), _own(pipe, r, steps, {k: v for k, v in extra.items() if k != "guidance_rescale"}))


def test_batcher_issues_the_rescale_launch_only_while_a_rescaled_request_steps(ops, monkeypatch):
    cfg, pipe = _tiny_pipe(3)
    reqs = _tiny_requests(cfg.cross_attention_dim, 3)
    calls = {"old": 0, "linear": 0, "rescale": 0}

    def counted(name, fn):
        def call(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return call
    monkeypatch.setattr(ops, "cfg_dpmpp2m_step_rows", counted("old", ops.cfg_dpmpp2m_step_rows))
    monkeypatch.setattr(ops, "cfg_linear_step_rows_rescale", counted("rescale", ops.cfg_linear_step_rows_rescale))
    monkeypatch.setattr(ops, "cfg_linear_step_rows", counted("linear", ops.cfg_linear_step_rows))
    b = pipe.serve(128, 128, max_batch=4, buckets=(1, 2, 4)).warm()
    # no phi > 0 (one request of another sampler, one with an explicit 0): never the new entry
    _submit(b, reqs[0], 4, {"guidance_rescale": 0.0})
    _submit(b, reqs[1], 3, {"sampler_name": "sample_euler"})
    b.run_until_idle()
    assert calls == {"old": 2, "linear": 3, "rescale": 0}, calls          # the join, 3 steps beside Euler, the 4th alone
    transitions = b.stats()["steps"] + 1                                   # (the last transition runs no step)
    assert calls["old"] + calls["linear"] == transitions
    # one phi > 0 request (3 steps) beside a 5-step DPM++ 2M: the new entry exactly while it steps, one launch per step
    calls.update(old=0, linear=0, rescale=0)
    s0 = b.stats()["steps"]
    f = _submit(b, reqs[2], 3, {"guidance_rescale": 0.7})
    _submit(b, reqs[0], 5, {})
    b.run_until_idle()
    assert calls == {"old": 1 + 2, "linear": 3, "rescale": 3}, calls       # (the wrapper hands all three on to the new entry)
    assert calls["old"] + calls["linear"] == b.stats()["steps"] - s0 + 1 and torch.isfinite(f.result()).all()
