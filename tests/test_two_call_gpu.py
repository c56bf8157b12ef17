"""The two-call sampler family on the MI355X (`-m gpu`): dsc_cfg_staged_step_rows against dsc_cfg_linear_step_rows (and its
rescale form) bit for bit where every slot is FULL, against its header formulas where slots PREDICT and CORRECT, the fused loop
for Heun / DPM2 / DPM2 a / DPM++ 2S a / DPM++ SDE against protocol mode, and the continuous batcher serving them beside
requests of the one-call samplers."""
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
from test_guidance_rescale_gpu import _restate as _restate_rescaled, _set_v
from test_linear_step_gpu import _recs, _toy
from test_serving_gpu import _h, _tiny_pipe, _tiny_requests
from test_serving_img_gpu import _f32, _fma, _gen, _ulps, tiny  # noqa: F401 (tiny: a fixture)

pytestmark = pytest.mark.gpu
TW = 96
NAMES = ("x", "old", "x_in", "t", "sigma_groups", "tadd")
SENTINEL = 3.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- a. the kernel
def _call(fn, chw, x, eps, old, n_src, n_dst, recs, mid=None):
    """-> (x, old, x_in, t, sigma_groups, tadd[, mid]) after one launch on copies of the state rows"""
    x, old = x.clone(), old.clone()
    x_in = torch.full((2 * n_dst, chw), 7.0, dtype=torch.float16, device="cuda")
    t = torch.full((2 * n_dst,), -1.0, device="cuda")
    s = torch.full((n_dst,), -1.0, device="cuda")
    tadd = torch.zeros(2 * n_dst, TW, dtype=torch.float16, device="cuda")
    if mid is None:
        fn(x, eps, old, n_src, x_in, t, s, recs, tadd=tadd)
        torch.cuda.synchronize()
        return x, old, x_in, t, s, tadd
    mid = mid.clone()
    fn(x, mid, eps, old, n_src, x_in, t, s, recs, tadd=tadd)
    torch.cuda.synchronize()
    return x, old, x_in, t, s, tadd, mid


@pytest.mark.parametrize("chw", [1024, 2056, 16384])
@pytest.mark.parametrize("n_src, n_dst, modes", [(2, 4, "SSJI"), (4, 2, "SISI")])
@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_every_slot_full_is_the_linear_op(ops, chw, n_src, n_dst, modes, phi):
    """every STEP slot FULL (given, and left to the wrapper's default), v scalars and a noise row on the odd slots: all six
    outputs carry dsc_cfg_linear_step_rows' bits - with a slot at phi > 0: dsc_cfg_linear_step_rows_rescale's - and `mid`
    keeps its sentinel.  Bucket switches in both directions"""
    n = len(modes)
    x, eps, old = _h(n, chw, seed=31), _h(2 * n_src, chw, seed=32), _h(n, chw, seed=33)
    tabs = [_h(TW, seed=40 + i) for i in range(n)]
    noise = _h(n, chw, seed=34)
    recs = _recs(ops, modes, tabs)
    for i, r in enumerate(recs):
        if i % 2:
            _set_v(r)
            r.update(s=0.4, noise=noise[i])
    if phi:
        recs[0]["rescale"] = phi
    plain = _call(ops.cfg_linear_step_rows, chw, x, eps, old, n_src, n_dst, recs)      # (picks the rescale entry from the records)
    mid = torch.full_like(x, SENTINEL)
    for variant in (recs, [dict(r, stage=ops.ROW_STAGE_FULL, m=0.9) for r in recs]):
        got = _call(ops.cfg_staged_step_rows, chw, x, eps, old, n_src, n_dst, variant, mid=mid)
        for name, a, b in zip(NAMES, got, plain):
            assert torch.equal(a, b), (modes, name)
        assert (got[6] == SENTINEL).all()


def _restate(x, mid, eu, ec, old, p, noise, stage):
    """include/dsc_hip.h's formulas for one PREDICT (1) / CORRECT (2) slot, every multiply-add an fp32 fma
    -> (the row written: mid' or x', old', x_in row)"""
    x, mid, eu, ec, old = (v.float().cpu() for v in (x, mid, eu, ec, old))
    g, a, m, b, c, cn, cs, co, s = (_f32(p[k]).float() for k in ("guidance", "a", "m", "b", "c", "c_in_next", "c_skip", "c_out", "s"))
    e = _fma(g, ec - eu, eu)
    seen = mid if stage == 2 else x
    d = _fma(co, e, cs * seen).half().float()
    out = _fma(a, x, b * d)
    if stage == 2:
        out = _fma(m, mid, _fma(c, old, out))
    if noise is not None:
        out = _fma(s, noise.float().cpu(), out)
    out = out.half().float()
    return out.half(), d.half(), (out * cn).half()


@pytest.mark.parametrize("chw", [1024, 2056, 16384])
def test_predict_and_correct_against_the_formulas(ops, chw):
    """slots (n_src 7, n_dst 6): 0 PREDICT with noise and v scalars, 1 PREDICT without noise, 2 JOIN, 3 CORRECT with m, c and
    noise, 4 IDLE, 5 FULL with noise, 6 a leaving CORRECT slot at i >= n_dst with v scalars.  PREDICT / CORRECT: at most 1 fp16
    ulp from the restated formulas in the row written, old and the x_in rows (the sibling kernels' bound); PREDICT leaves x
    bit-identical, CORRECT and FULL leave mid bit-identical; FULL / JOIN / IDLE and t_buf / sigma_groups / tadd carry
    dsc_cfg_linear_step_rows' bits; CORRECT follows mid"""
    P, C = ops.ROW_STAGE_PREDICT, ops.ROW_STAGE_CORRECT
    modes, n_src, n_dst = "SSJSISS", 7, 6
    x, eps, old, mid = _h(7, chw, seed=61), _h(14, chw, seed=62), _h(7, chw, seed=63), _h(7, chw, seed=65)
    tabs = [_h(TW, seed=70 + i) for i in range(7)]
    noise = _h(7, chw, seed=64)
    recs = _recs(ops, modes, tabs)
    recs[6].update(c_in_next=0.0, t_next=0.0, sigma_next=1.0, temb_row=None, s=0.0)
    for i in (0, 6):
        _set_v(recs[i])
    for i in (1, 3, 5):
        recs[i].update(c_skip=1.0, c_out=-recs[i]["sigma"])
    for i in (0, 3, 5):
        recs[i].update(s=0.3 + 0.1 * i, noise=noise[i])
    recs[1].update(s=5.0, noise=None)
    stages = {0: P, 1: P, 3: C, 6: C}
    for i, st in stages.items():
        recs[i].update(stage=st, m=0.35 + 0.05 * i)
    plain = _call(ops.cfg_linear_step_rows, chw, x, eps, old, n_src, n_dst, recs)          # (ignores stage / m)
    got = _call(ops.cfg_staged_step_rows, chw, x, eps, old, n_src, n_dst, recs, mid=mid)
    for i, st in stages.items():
        out, d, xi = _restate(x[i], mid[i], eps[i], eps[n_src + i], old[i], recs[i], recs[i].get("noise"), st)
        u = [_ulps(got[6][i] if st == P else got[0][i], out), _ulps(got[1][i], d)]
        if i < n_dst:
            u += [_ulps(got[2][i], xi), _ulps(got[2][n_dst + i], xi)]
        print(f"chw {chw} slot {i} stage {st}: ulps row / old / x_in = {u}")
        assert max(u) <= 1, (i, u)
        if st == P:
            assert torch.equal(got[0][i], x[i]) and not torch.equal(got[6][i], mid[i])
        else:
            assert torch.equal(got[6][i], mid[i]) and not torch.equal(got[0][i], plain[0][i])
    for i in (2, 4, 5):
        assert torch.equal(got[0][i], plain[0][i]) and torch.equal(got[1][i], plain[1][i]), i
        assert torch.equal(got[2][[i, n_dst + i]], plain[2][[i, n_dst + i]]) and torch.equal(got[6][i], mid[i]), i
    assert torch.equal(got[3], plain[3]) and torch.equal(got[4], plain[4]) and torch.equal(got[5], plain[5])
    # CORRECT reads mid: another intermediate point, another x' and another D
    other = _call(ops.cfg_staged_step_rows, chw, x, eps, old, n_src, n_dst, recs, mid=_h(7, chw, seed=66))
    assert not torch.equal(other[0][3], got[0][3]) and not torch.equal(other[1][3], got[1][3])
    assert torch.equal(other[6][0], got[6][0]) and torch.equal(other[0][5], got[0][5])      # PREDICT and FULL do not


@pytest.mark.parametrize("chw", [1024, 8200, 16384])
def test_rescaled_correct_slot_against_the_formulas(ops, chw):
    """a CORRECT slot with phi = 0.7 (g = 7.5 on independent rows: K far from 1) beside a rescaled PREDICT slot and a FULL one:
    the rescale's sums run over mid in CORRECT and over x in PREDICT.  Against the header formulas with fp64 sums, at most 1
    fp16 ulp (test_guidance_rescale_gpu.py's bound: K differs from the kernel's by the summation order only); two launches give
    equal bits"""
    P, C = ops.ROW_STAGE_PREDICT, ops.ROW_STAGE_CORRECT
    n = 3
    x, eps, old, mid = _h(n, chw, seed=81), _h(2 * n, chw, seed=82), _h(n, chw, seed=83), _h(n, chw, seed=85)
    tabs = [_h(TW, seed=90 + i) for i in range(n)]
    noise = _h(n, chw, seed=84)
    recs = _recs(ops, "SSS", tabs)
    for i, r in enumerate(recs):
        r.update(guidance=7.5, rescale=0.7, c_skip=1.0, c_out=-r["sigma"], s=0.4, noise=noise[i])
    _set_v(recs[1])
    recs[0].update(stage=C, m=0.45)
    recs[1].update(stage=P, m=0.0, noise=None)
    got = _call(ops.cfg_staged_step_rows, chw, x, eps, old, n, n, recs, mid=mid)
    again = _call(ops.cfg_staged_step_rows, chw, x, eps, old, n, n, recs, mid=mid)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    plain = _call(ops.cfg_linear_step_rows, chw, x, eps, old, n, n, recs)
    assert torch.equal(got[0][2], plain[0][2]) and torch.equal(got[1][2], plain[1][2])      # the FULL slot: the rescale entry's bits
    # the restated rescale of the row the model saw; the m * mid term enters through `old`'s fma: x' = fma(m, mid, t2) needs its own line
    for i, st in ((0, C), (1, P)):
        seen = mid[i] if st == C else x[i]
        _, d, _, k = _restate_rescaled(seen, eps[i], eps[n + i], old[i], recs[i], None, 0.7)
        xf, mf, of, df = x[i].float().cpu(), mid[i].float().cpu(), old[i].float().cpu(), d.float()
        a, m, b, c, cn, s = (_f32(recs[i][key]).float() for key in ("a", "m", "b", "c", "c_in_next", "s"))
        out = _fma(a, xf, b * df)
        if st == C:
            out = _fma(s, noise[i].float().cpu(), _fma(m, mf, _fma(c, of, out)))
        out = out.half().float()
        u = [_ulps(got[6][i] if st == P else got[0][i], out.half()), _ulps(got[1][i], d),
             _ulps(got[2][i], (out * cn).half()), _ulps(got[2][n + i], (out * cn).half())]
        print(f"chw {chw} slot {i} stage {st}: K = {k:.6f}, ulps row / old / x_in = {u}")
        assert max(u) <= 1 and abs(k - 1.0) > 1e-2, (i, u, k)


def test_argument_status(ops):
    lib = dsc.load_library()
    d = ctypes.c_void_p(0x1000)
    F, P, C = ops.ROW_STAGE_FULL, ops.ROW_STAGE_PREDICT, ops.ROW_STAGE_CORRECT

    def call(recs, stages, n_src=2, n_dst=2, **kw):
        arr = (ops.RowLinear * len(recs))(*recs)
        st = None if stages is None else ctypes.cast((ops.RowStage * len(stages))(*(ops.RowStage(s, 0.5) for s in stages)), ctypes.c_void_p)
        phi = kw.get("phi")
        phi = None if phi is None else ctypes.cast((ctypes.c_float * len(phi))(*phi), ctypes.c_void_p)
        return lib.dsc_cfg_staged_step_rows(kw.get("x", d), kw.get("mid", d), kw.get("eps", d), d, n_src, kw.get("x_in", d), d, d,
                                            kw.get("tadd", d), kw.get("tw", 96), n_dst, ctypes.cast(arr, ctypes.c_void_p), st, phi,
                                            kw.get("n_slots", len(recs)), kw.get("chw", 1024), kw.get("dtype", 0), None)

    def rec(mode, temb=None, noise=None):
        return ops.RowLinear(mode, 1.0, 7.5, 0.5, 0.5, 0.0, 1.0, 10.0, 1.0, 1.0, -1.0, 0.1, temb, noise)
    step, join, idle = rec(ops.ROW_STEP), rec(ops.ROW_JOIN), rec(ops.ROW_IDLE)
    # everything the linear entry checks
    assert call([step, step], [P, C], x=None) == -1 and call([step, step], [P, C], x_in=None) == -1
    assert call([step, step], [P, C], x=ctypes.c_void_p(0x1004)) == -2 and call([step, step], [P, C], eps=ctypes.c_void_p(0x1008)) == -2
    assert call([step, step], [P, C], chw=1020) == -2 and call([step, step], [P, C], chw=1028) == -2       # chw % 8 != 0
    assert call([step, step], [P, C], dtype=3) == -2 and call([step, step], [P, C], eps=None) == -1
    assert call([step, step, step], [F] * 3, n_src=2, n_dst=2) == -1 and call([idle, idle, join], [F] * 3, n_src=3, n_dst=2) == -1
    assert call([rec(5), idle], [F, F]) == -1 and call([step], [F], n_dst=2) == -1
    assert call([idle] * 17, [F] * 17, n_src=0, n_dst=1) == -1
    assert call([rec(ops.ROW_STEP, noise=0x2004), step], [P, C]) == -2 and call([rec(ops.ROW_STEP, temb=0x2004), step], [P, C]) == -2
    assert call([rec(ops.ROW_STEP, temb=0x2000), step], [P, C], tadd=None) == -1
    assert call([step, step], [F, F], phi=[0.5, 1.5]) == -1 and call([step, step], [F, F], phi=[float("nan"), 0.0]) == -1
    # its own
    assert call([step, step], None) == -1                                                   # stages == NULL
    assert call([step, step], [F, 3]) == -1 and call([step, step], [-1, F]) == -1            # an unknown stage
    assert call([step, step], [F, P], mid=None) == -1 and call([step, step], [C, F], mid=None) == -1
    assert call([step, step], [F, P], mid=ctypes.c_void_p(0x1008)) == -2                    # misaligned mid
    assert ctypes.sizeof(ops.RowStage) == 8
    assert 16 * (ctypes.sizeof(ops.RowLinear) + ctypes.sizeof(ops.RowStage) + 4) <= 2048    # well inside the 4 KB kernarg segment


def test_code_object_has_no_scratch_or_spill():
    """device-only compile of csrc/sampler.hip with the build's flags: the metadata of the two new kernels"""
    root = os.path.dirname(os.path.dirname(dsc.lib_path()))
    with tempfile.TemporaryDirectory() as tmp:
        work = os.path.join(tmp, "sampler.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only",
                               "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "diffusionspatialcontrol_amd", "csrc"),
                               "-S", os.path.join(root, "diffusionspatialcontrol_amd", "csrc", "sampler.hip"), "-o", work],
                              stderr=subprocess.DEVNULL)
        listing = open(work).read()
    notes = listing[listing.index("amdhsa.kernels:"):]
    kernels = re.findall(r"\.name:\s+(\S*staged_rows\S*kernel\S*)(.*?)\.wavefront_size", notes, flags=re.S)
    assert len(kernels) == 2, [k[0] for k in kernels]
    for name, body in kernels:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", body), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", body) and re.search(r"\.sgpr_spill_count:\s+0\b", body), name
        print(name, re.search(r"\.vgpr_count:\s+(\d+)", body).group(1), "VGPRs")


# ----------------------------------------------------------------------------- b. the fused loop on the toy UNet
NOISY = ("sample_dpm_2_ancestral", "sample_dpmpp_2s_ancestral", "sample_dpmpp_sde")
FUSED_CASES = [("sample_heun", {"scheduler": "karras"}), ("sample_dpm_2", {"scheduler": "exponential"}),
               ("sample_dpm_2_ancestral", {"scheduler": "karras"}), ("sample_dpmpp_2s_ancestral", {"scheduler": "karras"}),
               ("sample_dpmpp_sde", {"scheduler": "karras"})]


def _call_table(name, steps, seed, sigmas=None):
    """a noise table with one row per model call (2 steps - 1), zero where the sampler draws none, as call_noise_table lays it out"""
    from diffusionspatialcontrol_amd.modules import sampling
    sig = [float(steps - i) for i in range(steps)] + [0.0] if sigmas is None else sigmas
    plan = sampling.call_plan(name, sig)
    tab = torch.randn(len(plan), 1, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).half()
    for k, call in enumerate(plan):
        if call.query is None:
            tab[k] = 0
    return tab.cuda()


def _replay_nonzero(table):
    rows = iter([table[k] for k in range(table.shape[0]) if table[k].any()])
    return lambda *_: next(rows)


@pytest.mark.parametrize("name, opt", FUSED_CASES)
def test_fused_equals_protocol_with_the_same_noise(ops, name, opt):
    """6 steps on the toy UNet: txt2img(fused=True, two_call=True, step_noise=T) against fused=False with a noise sampler that
    replays T's non-zero rows, within test_linear_step_gpu.py's bound for the same comparison at this step count (2e-2 of the
    result's scale); eta = 1.  Observed on one MI355X: see DESIGN.md section 12"""
    from diffusionspatialcontrol_amd.modules import sampling
    pipe, kw, _, _ = _toy()
    fn = getattr(sampling, name)
    table = _call_table(name, 6, 1001) if name in NOISY else None
    fused = pipe.txt2img(None, fused=True, two_call=True, sampler_name=fn, sampler_opt=opt, step_noise=table, **kw)[0].float().cpu()
    proto_fn = functools.partial(fn, noise_sampler=_replay_nonzero(table)) if name in NOISY else fn
    proto = pipe.txt2img(None, fused=False, sampler_name=proto_fn, sampler_opt=opt, **kw)[0].float().cpu()
    scale = proto.abs().max().item()
    err = (fused - proto).abs().max().item()
    print(f"{name} {opt}: fused vs protocol {err:.3e} (scale {scale:.2f}, ratio {err / scale:.3e})")
    assert torch.isfinite(fused).all() and err < 2e-2 * scale, (err, scale)
    by_name = pipe.txt2img(None, fused=True, two_call=True, sampler_name=name, sampler_opt=opt, step_noise=table, **kw)[0].float().cpu()
    assert torch.equal(by_name, fused)
    if name in NOISY:                             # the table is live: other noise, another image
        other = pipe.txt2img(None, fused=True, two_call=True, sampler_name=fn, sampler_opt=opt,
                             step_noise=table.flip(0).contiguous(), **kw)[0]
        assert (other.float().cpu() - fused).abs().max().item() > 2e-2 * scale
        with pytest.raises(ValueError, match="step_noise"):
            pipe.txt2img(None, fused=True, two_call=True, sampler_name=fn, sampler_opt=opt, step_noise=table[:6], **kw)


def test_the_flag_is_opt_in_and_v_prediction(ops):
    pipe, kw, table, _ = _toy("v_prediction", seed=5)
    opt = {"scheduler": "karras"}
    with pytest.raises(NotImplementedError, match="sample_heun"):
        pipe.txt2img(None, fused=True, sampler_name="sample_heun", sampler_opt=opt, **kw)
    with pytest.raises(NotImplementedError, match="sample_lms"):
        pipe.txt2img(None, fused=True, two_call=True, sampler_name="sample_lms", sampler_opt=opt, **kw)
    fused = pipe.txt2img(None, fused=True, two_call=True, sampler_name="sample_heun", sampler_opt=opt, **kw)[0].float().cpu()
    proto = pipe.txt2img(None, fused=False, sampler_name="sample_heun", sampler_opt=opt, **kw)[0].float().cpu()
    scale = proto.abs().max().item()
    err = (fused - proto).abs().max().item()
    print(f"v-prediction sample_heun: fused vs protocol {err:.3e} (scale {scale:.2f}, ratio {err / scale:.3e})")
    assert torch.isfinite(fused).all() and err < 2e-2 * scale, (err, scale)
    # two_call=True with a linear-family sampler changes nothing
    a = pipe.txt2img(None, fused=True, sampler_name="sample_euler_ancestral", sampler_opt=opt, step_noise=table, **kw)[0]
    b = pipe.txt2img(None, fused=True, two_call=True, sampler_name="sample_euler_ancestral", sampler_opt=opt, step_noise=table, **kw)[0]
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------- c. serving on the toy UNet
def _own(pipe, r, spec):
    """the request's own txt2img(fused=True, two_call=True) with its sampler, noise table and eta"""
    steps, g, opt, extra = spec
    return pipe.txt2img(None, height=128, width=128, num_inference_steps=steps, guidance_scale=g, fused=True, two_call=True,
                        sampler_name=extra.get("sampler_name", "sample_dpmpp_2m"), eta=extra.get("eta", 1.0), sampler_opt=opt,
                        step_noise=extra.get("step_noise"), latents=r["latents"], region_map_state=r["region_map_state"],
                        prompt_embeds=r["prompt_embeds"], negative_prompt_embeds=r["negative_prompt_embeds"],
                        text_input_ids=r["text_input_ids"], output_type="latent")[0].float().cpu()


def _submit(b, r, spec):
    steps, g, opt, extra = spec
    return b.submit(dict(r, num_inference_steps=steps, guidance_scale=g, sampler_opt=opt, **extra))


def test_batcher_two_call_requests_equal_their_own_fused_txt2img(ops):
    """Two slots (buckets 1 / 2, the geometry in which the UNet is bit-stable, see test_linear_step_gpu.py): A (Heun, 3 steps =
    5 model calls) starts; B (DPM++ SDE, 3 steps, a noise row per call) joins two transitions in; when A has left, C (DPM++ 2M, 4
    steps) takes the freed slot and rides beside B's PREDICT / CORRECT records as a FULL one.  Every request's latent is its own
    txt2img(fused=True[, two_call=True], step_noise=...)'s, bit for bit; no capture after warm()"""
    cfg, pipe = _tiny_pipe(2)
    ra, rb, rc = _tiny_requests(cfg.cross_attention_dim, 3)
    K, E = {"scheduler": "karras"}, {"scheduler": "exponential"}
    specs = {"A": (ra, (3, 7.5, K, {"sampler_name": "sample_heun"})),
             "B": (rb, (3, 6.0, E, {"sampler_name": "sample_dpmpp_sde", "eta": 1.0, "step_noise": _call_table("dpmpp_sde", 3, 7)})),
             "C": (rc, (4, 7.5, K, {}))}
    b = pipe.serve(128, 128, max_batch=2, buckets=(1, 2), two_call=True).warm()
    futs = {"A": _submit(b, *specs["A"])}
    for _ in range(3):                                # the join, then A's first PREDICT and CORRECT
        b.step()
    futs["B"] = _submit(b, *specs["B"])
    for _ in range(3):                                # B joins; A's second CORRECT and its FULL step: A leaves
        b.step()
    assert b._slots[0] is None and b._slots[1] is not None and b._slots[1].family == "dpmpp_sde"
    futs["C"] = _submit(b, *specs["C"])
    b.step()
    assert b._slots[0] is not None and b._slots[0].family == "dpmpp_2m"           # A's slot, reused
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["joins"] == 3 and st["leaves"] == 3 and st["staged_transitions"] >= 6, st
    for n, (r, spec) in specs.items():
        own = _own(pipe, r, spec)
        got = futs[n].result().float().cpu()
        d = (got - own).abs().max().item()
        print(f"request {n}: vs its own fused txt2img {d:.3e}")
        assert torch.equal(got, own), (n, d)
    # and C is what the flagless path computes for it
    plain = pipe.txt2img(None, height=128, width=128, num_inference_steps=4, guidance_scale=7.5, fused=True, sampler_opt=K,
                         sampler_name="sample_dpmpp_2m", latents=rc["latents"], region_map_state=rc["region_map_state"],
                         prompt_embeds=rc["prompt_embeds"], negative_prompt_embeds=rc["negative_prompt_embeds"],
                         text_input_ids=rc["text_input_ids"], output_type="latent")[0].float().cpu()
    assert torch.equal(futs["C"].result().float().cpu(), plain)


def test_served_img2img_with_dpm_2_ancestral(tiny, ops):
    """img2img at strength 0.6 of 8 steps (4 steps run: 7 model calls, a noise row after every CORRECT call): the served request
    against img2img(fused=True, two_call=True) with the same table, within test_served_img2img_equals_its_own_pipeline_call's
    bound (2e-3 of the range), and that call against protocol mode replaying the table (2e-2 of the scale)"""
    from diffusionspatialcontrol_amd.modules import sampling
    pipe = tiny.pipe
    table = _call_table("dpm_2_ancestral", 4, 60)
    kw = dict(latents=tiny.lat0.clone(), strength=0.6, num_inference_steps=8, **tiny.common)
    fused = pipe.img2img(None, generator=_gen(33), fused=True, two_call=True, sampler_name="sample_dpm_2_ancestral",
                         step_noise=table, **kw)[0].float().cpu()
    proto = pipe.img2img(None, generator=_gen(33), fused=False,
                         sampler_name=functools.partial(sampling.sample_dpm_2_ancestral, noise_sampler=_replay_nonzero(table)),
                         **kw)[0].float().cpu()
    scale = proto.abs().max().item()
    print(f"img2img DPM2 a: fused vs protocol {(fused - proto).abs().max().item():.3e} (scale {scale:.2f})")
    assert (fused - proto).abs().max().item() < 2e-2 * scale
    b = pipe.serve(128, 128, max_batch=2, buckets=(1, 2), two_call=True).warm()
    fut = b.submit(dict(tiny.base, image=tiny.lat0.clone(), strength=0.6, num_inference_steps=8, generator=_gen(33),
                        sampler_name="sample_dpm_2_ancestral", step_noise=table))
    b.run_until_idle()
    d = (fut.result().float().cpu() - fused).abs().max().item()
    print(f"served img2img DPM2 a vs img2img(fused=True, two_call=True): {d:.3e} (range {scale:.2f})")
    assert d < 2e-3 * scale and b.stats()["staged_transitions"] == 6
