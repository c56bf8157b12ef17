"""The linear-step sampler family on the MI355X (`-m gpu`): dsc_cfg_linear_step_rows against dsc_cfg_dpmpp2m_step_rows bit for
bit and against its header formulas, the fused loop for Euler / Euler a / DPM++ 2M SDE / LCM and v-prediction against protocol
mode and the CPU oracle, and the continuous batcher serving them per request, mixed in one batch."""
import ctypes
import functools
import math
import os
import re
import subprocess
import tempfile

import pytest
import torch

from inputs import FakeTokenizer
from oracle import unet_ref

import diffusionspatialcontrol_amd as dsc
from test_serving_gpu import _h, _params, _tiny_pipe, _tiny_requests
from test_serving_img_gpu import _f32, _fma, _gen, _inpaint_oracle, _ulps, tiny  # noqa: F401 (tiny: a fixture)
from test_unet_pipeline_gpu import _region_state, _tiny_setup

pytestmark = pytest.mark.gpu
TW = 96


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- a. the kernel
def _call(ops, linear, chw, x, eps, old, n_src, n_dst, recs):
    x, old = x.clone(), old.clone()
    x_in = torch.full((2 * n_dst, chw), 7.0, dtype=torch.float16, device="cuda")
    t = torch.full((2 * n_dst,), -1.0, device="cuda")
    s = torch.full((n_dst,), -1.0, device="cuda")
    tadd = torch.zeros(2 * n_dst, TW, dtype=torch.float16, device="cuda")
    (ops.cfg_linear_step_rows if linear else ops.cfg_dpmpp2m_step_rows)(x, eps, old, n_src, x_in, t, s, recs, tadd=tadd)
    torch.cuda.synchronize()
    return x, old, x_in, t, s, tadd


def _recs(ops, modes, tabs):
    recs = []
    for i, m in enumerate(modes):
        p = _params(i)
        p["mode"] = {"S": ops.ROW_STEP, "J": ops.ROW_JOIN, "I": ops.ROW_IDLE}[m]
        p["temb_row"] = tabs[i] if m != "I" else None
        recs.append(p)
    return recs


@pytest.mark.parametrize("chw", [1024, 2056, 16384])
@pytest.mark.parametrize("n_src, n_dst, modes", [(2, 4, "SSJI"), (4, 2, "SISI"), (4, 4, "JSIS"), (3, 3, "SSS")])
def test_eps_prediction_without_noise_is_the_dpmpp2m_op(ops, chw, n_src, n_dst, modes):
    """c_skip = 1, c_out = -sigma, no noise row (spelled out, and as the wrapper's defaults): every output buffer carries the
    bits of dsc_cfg_dpmpp2m_step_rows - STEP / JOIN / IDLE, bucket switches in both directions"""
    n = len(modes)
    x, eps, old = _h(n, chw, seed=31), _h(2 * n_src, chw, seed=32), _h(n, chw, seed=33)
    tabs = [_h(TW, seed=40 + i) for i in range(n)]
    recs = _recs(ops, modes, tabs)
    plain = _call(ops, False, chw, x, eps, old, n_src, n_dst, recs)
    spelled = [dict(r, c_skip=1.0, c_out=-r["sigma"], s=0.7, noise=None) for r in recs]
    for variant in (recs, spelled):
        got = _call(ops, True, chw, x, eps, old, n_src, n_dst, variant)
        for name, a, b in zip(("x", "old", "x_in", "t", "sigma_groups", "tadd"), got, plain):
            assert torch.equal(a, b), (modes, name)


def _restate(x, eu, ec, old, p, noise):
    """include/dsc_hip.h's formulas for one STEP slot, every multiply-add an fp32 fma -> (x', old', x_in row)"""
    x, eu, ec, old = (v.float().cpu() for v in (x, eu, ec, old))
    g, a, b, c, cn, cs, co, s = (_f32(p[k]).float() for k in ("guidance", "a", "b", "c", "c_in_next", "c_skip", "c_out", "s"))
    e = _fma(g, ec - eu, eu)
    d = _fma(co, e, cs * x).half().float()
    xn = _fma(c, old, _fma(a, x, b * d))
    if noise is not None:
        xn = _fma(s, noise.float().cpu(), xn)
    xn = xn.half().float()
    return xn.half(), d.half(), (xn * cn).half()


@pytest.mark.parametrize("chw", [1024, 2056, 16384])
def test_noise_and_v_scalars_against_the_formulas(ops, chw):
    """slots: v-prediction scalars with noise, v without noise, JOIN, eps-prediction with noise, IDLE, a leaving slot at
    i >= n_dst with noise.  STEP slots: at most 1 fp16 ulp from the restated formulas (the bound of the known-region kernel's
    test); JOIN / IDLE: the DPM++ 2M op's bits; a slot without noise ignores `s`"""
    modes, n_src, n_dst = "SSJSIS", 6, 5
    x, eps, old = _h(6, chw, seed=61), _h(12, chw, seed=62), _h(6, chw, seed=63)
    tabs = [_h(TW, seed=70 + i) for i in range(6)]
    noise = _h(6, chw, seed=64)
    recs = _recs(ops, modes, tabs)
    recs[5].update(c_in_next=0.0, t_next=0.0, sigma_next=1.0, temb_row=None)
    for i in (0, 1, 5):
        sg = recs[i]["sigma"]
        recs[i].update(c_skip=1.0 / (sg * sg + 1.0), c_out=-sg / math.sqrt(sg * sg + 1.0))
    recs[3].update(c_skip=1.0, c_out=-recs[3]["sigma"])
    for i in (0, 3, 5):
        recs[i].update(s=0.3 + 0.1 * i, noise=noise[i])
    recs[1].update(s=5.0, noise=None)
    plain = _call(ops, False, chw, x, eps, old, n_src, n_dst, recs)
    got = _call(ops, True, chw, x, eps, old, n_src, n_dst, recs)
    for i in (0, 1, 3, 5):
        xn, d, xi = _restate(x[i], eps[i], eps[n_src + i], old[i], recs[i], recs[i]["noise"])
        u = [_ulps(got[0][i], xn), _ulps(got[1][i], d)]
        if i < n_dst:
            u += [_ulps(got[2][i], xi), _ulps(got[2][n_dst + i], xi)]
        print(f"chw {chw} slot {i}: ulps x' / old / x_in = {u}")
        assert max(u) <= 1, (i, u)
        assert not torch.equal(got[0][i], plain[0][i])                       # (the scalars / the noise do matter)
    for i in (2, 4):
        assert torch.equal(got[0][i], plain[0][i]) and torch.equal(got[1][i], plain[1][i]), i
        assert torch.equal(got[2][[i, n_dst + i]], plain[2][[i, n_dst + i]]), i
    assert torch.equal(got[3], plain[3]) and torch.equal(got[4], plain[4]) and torch.equal(got[5], plain[5])


def test_argument_status(ops):
    lib = dsc.load_library()
    d = ctypes.c_void_p(0x1000)

    def call(recs, n_src=2, n_dst=2, **kw):
        arr = (ops.RowLinear * len(recs))(*recs)
        return lib.dsc_cfg_linear_step_rows(kw.get("x", d), kw.get("eps", d), d, n_src, kw.get("x_in", d), d, d, kw.get("tadd", d),
                                            kw.get("tw", 96), n_dst, ctypes.cast(arr, ctypes.c_void_p), kw.get("n_slots", len(recs)),
                                            kw.get("chw", 1024), kw.get("dtype", 0), None)

    def rec(mode, temb=None, noise=None):
        return ops.RowLinear(mode, 1.0, 7.5, 0.5, 0.5, 0.0, 1.0, 10.0, 1.0, 1.0, -1.0, 0.1, temb, noise)
    step, join, idle = rec(ops.ROW_STEP), rec(ops.ROW_JOIN), rec(ops.ROW_IDLE)
    assert call([step, step], x=None) == -1 and call([step, step], x_in=None) == -1         # null pointers
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
    assert ctypes.sizeof(ops.RowLinear) == 64 and 16 * ctypes.sizeof(ops.RowLinear) <= 1024  # well inside the 4 KB kernarg segment


def test_linear_entries_refuse_8_byte_rows(ops):
    """chw = 1444 (19 x 19 latents: 361 four-half vectors).  The linear, rescale and cat entries move 8 halfs per lane: each is
    refused before any launch, nothing written - such rows stay with dsc_cfg_dpmpp2m_step_rows and its known-region form"""
    chw, n = 1444, 2
    x, eps, old = _h(n, chw, seed=81), _h(2 * n, chw, seed=82), _h(n, chw, seed=83)
    recs = [_params(i) for i in range(n)]
    rescaled = [dict(r, rescale=0.7) for r in recs]
    for fn, rs, more, row in ((ops.cfg_linear_step_rows, recs, (), chw), (ops.cfg_linear_step_rows_rescale, rescaled, (), chw),
                              (ops.cfg_linear_step_rows_cat, recs, ([None, None],), chw + 8)):
        xr, oldr = x.clone(), old.clone()
        x_in = torch.full((2 * n, row), 7.0, dtype=torch.float16, device="cuda")
        t, s = torch.full((2 * n,), -1.0, device="cuda"), torch.full((n,), -1.0, device="cuda")
        with pytest.raises(dsc.DscLibraryError):
            fn(xr, eps, oldr, n, x_in, t, s, rs, *more)
        torch.cuda.synchronize()
        assert torch.equal(xr, x) and torch.equal(oldr, old) and (x_in == 7.0).all() and (t == -1.0).all() and (s == -1.0).all()


def test_code_object_has_no_scratch_or_spill():
    """device-only compile of csrc/sampler.hip with the build's flags: the new kernel's metadata (as tests/test_cabi.py reads
    the self-attention kernel's), and nothing in the listing from the scalar-store family"""
    root = os.path.dirname(os.path.dirname(dsc.lib_path()))
    with tempfile.TemporaryDirectory() as tmp:
        work = os.path.join(tmp, "sampler.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only",
                               "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "diffusionspatialcontrol_amd", "csrc"),
                               "-S", os.path.join(root, "diffusionspatialcontrol_amd", "csrc", "sampler.hip"), "-o", work],
                              stderr=subprocess.DEVNULL)
        listing = open(work).read()
    notes = listing[listing.index("amdhsa.kernels:"):]
    kernels = re.findall(r"\.name:\s+(\S*linear_rows_kernel\S*)(.*?)\.wavefront_size", notes, flags=re.S)
    assert len(kernels) == 1
    body = kernels[0][1]
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", body)
    assert re.search(r"\.vgpr_spill_count:\s+0\b", body) and re.search(r"\.sgpr_spill_count:\s+0\b", body)
    # (the mnemonics are assembled from halves: source files of this repository must not spell them, tests included; the
    # listing is checked as a whole because the metadata above says nothing about which store instructions a kernel uses)
    family = "|".join("s_" + w for w in ("store_dword", "buffer_store", "scratch_store", "atomic", "buffer_atomic", "dcache_wb", "dcache_discard"))
    assert not re.search(r"\b(" + family + ")", listing)


# ----------------------------------------------------------------------------- b. the fused loop on the toy UNet
def _replay(table):
    order = iter(range(table.shape[0]))
    return lambda *_: table[next(order)]


def _sampler(name):
    from diffusionspatialcontrol_amd.modules import sampling, samplers_extra_k_diffusion as sx
    return sx.sample_lcm if name == "sample_lcm" else getattr(sampling, name)


FUSED_CASES = [("sample_euler", {"scheduler": "karras"}), ("sample_euler_ancestral", {"scheduler": "karras"}),
               ("sample_dpmpp_2m_sde", {"scheduler": "exponential"}), ("sample_dpmpp_2m_sde", {"scheduler": "karras", "solver_type": "heun"}),
               ("sample_lcm", {"scheduler": "karras"})]


def _toy(prediction_type="epsilon", seed=1000):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    cfg, unet, sd, text = _tiny_setup(1)
    state, ids, rs = _region_state(n_img=1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler(prediction_type=prediction_type))
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).half()
    kw = dict(height=128, width=128, num_inference_steps=6, guidance_scale=7.5, latents=lat.clone(), output_type="latent",
              region_map_state=state, prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], text_input_ids=ids, eta=1.0)
    table = torch.randn(6, 1, 4, 16, 16, generator=torch.Generator().manual_seed(seed + 1)).half().cuda()
    return pipe, kw, table, (cfg, sd, text, rs, lat)


@pytest.mark.parametrize("name, opt", FUSED_CASES)
def test_fused_equals_protocol_with_the_same_noise(ops, name, opt):
    """6 steps on the toy UNet: txt2img(fused=True, step_noise=T) against fused=False with a noise_sampler that replays T, within
    test_denoise_loop_fused_protocol_oracle's bound for the same comparison (2e-2 of the result's scale); eta = 1"""
    pipe, kw, table, _ = _toy()
    fn = _sampler(name)
    fused = pipe.txt2img(None, fused=True, sampler_name=fn, sampler_opt=opt, step_noise=table, **kw)[0].float().cpu()
    proto_fn = fn if name == "sample_euler" else functools.partial(fn, noise_sampler=_replay(table))
    proto = pipe.txt2img(None, fused=False, sampler_name=proto_fn, sampler_opt=opt, **kw)[0].float().cpu()
    scale = proto.abs().max().item()
    err = (fused - proto).abs().max().item()
    print(f"{name} {opt}: fused vs protocol {err:.3e} (scale {scale:.2f})")
    assert torch.isfinite(fused).all() and err < 2e-2 * scale, (err, scale)
    if name != "sample_euler":                    # the table is live: other noise, another image
        other = pipe.txt2img(None, fused=True, sampler_name=fn, sampler_opt=opt, step_noise=table.flip(0).contiguous(), **kw)[0]
        assert (other.float().cpu() - fused).abs().max().item() > 2e-2 * scale


def test_fused_true_never_substitutes_a_sampler(ops):
    from diffusionspatialcontrol_amd.modules import sampling
    pipe, kw, table, _ = _toy()
    with pytest.raises(NotImplementedError, match="sample_heun"):
        pipe.txt2img(None, fused=True, sampler_name="sample_heun", sampler_opt={"scheduler": "karras"}, **kw)
    with pytest.raises(ValueError, match="step_noise"):
        pipe.txt2img(None, fused=True, sampler_name="sample_euler_ancestral", sampler_opt={}, step_noise=table[:5], **kw)
    # fused=None keeps its rule: Euler runs in protocol mode, DPM++ 2M fused; and fused Euler is not DPM++ 2M
    e_auto = pipe.txt2img(None, sampler_name="sample_euler", sampler_opt={"scheduler": "karras"}, **kw)[0].float().cpu()
    e_proto = pipe.txt2img(None, fused=False, sampler_name=sampling.sample_euler, sampler_opt={"scheduler": "karras"}, **kw)[0]
    e_fused = pipe.txt2img(None, fused=True, sampler_name="sample_euler", sampler_opt={"scheduler": "karras"}, **kw)[0].float().cpu()
    m_fused = pipe.txt2img(None, fused=True, sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"}, **kw)[0].float().cpu()
    scale = e_auto.abs().max().item()
    assert (e_auto - e_proto.float().cpu()).abs().max().item() < 2e-2 * scale
    near, far = (e_fused - e_auto).abs().max().item(), (e_fused - m_fused).abs().max().item()
    print(f"fused Euler: vs protocol Euler {near:.3e}, vs fused DPM++ 2M {far:.3e} (scale {scale:.2f})")
    assert near < 2e-2 * scale and near < far


@pytest.mark.parametrize("name", ["sample_euler", "sample_dpmpp_2m"])
@pytest.mark.parametrize("pass_kwargs", [False, True])
def test_v_prediction_fused_equals_protocol(ops, name, pass_kwargs):
    pipe, kw, _, _ = _toy("v_prediction", seed=5)
    pipe.k_diffusion_model.pass_kwargs = pass_kwargs
    opt = {"scheduler": "karras"}
    fused = pipe.txt2img(None, fused=True, sampler_name=name, sampler_opt=opt, **kw)[0].float().cpu()
    proto = pipe.txt2img(None, fused=False, sampler_name=name, sampler_opt=opt, **kw)[0].float().cpu()
    scale = proto.abs().max().item()
    err = (fused - proto).abs().max().item()
    print(f"v-prediction {name} pass_kwargs={pass_kwargs}: fused vs protocol {err:.3e} (scale {scale:.2f})")
    assert torch.isfinite(fused).all() and err < 2e-2 * scale, (err, scale)


def test_fused_euler_ancestral_against_the_cpu_oracle(ops):
    """the fp32 CPU oracle model driven by the same sampler with the same noise, at test_other_samplers_protocol_vs_oracle's bound"""
    from diffusionspatialcontrol_amd.modules import sampling
    pipe, kw, table, (cfg, sd, text, rs, lat) = _toy(seed=77)
    opt = {"scheduler": "karras"}
    out = pipe.txt2img(None, fused=True, sampler_name="sample_euler_ancestral", sampler_opt=opt, step_noise=table, **kw)[0].float().cpu()
    sig = pipe.get_sigmas(6, opt).half().float()
    ref = unet_ref.denoise_loop(sd, cfg, lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), text.float(), rs, 7.5,
                                sampler=sampling.sample_euler_ancestral,
                                sampler_kwargs={"eta": 1.0, "noise_sampler": _replay(table.float().cpu())})
    scale = ref.abs().max().item()
    e = (out - ref).abs()
    print(f"fused Euler a vs oracle: max {e.max().item():.3e} mean {e.mean().item():.3e} (scale {scale:.2f})")
    assert e.max().item() < 4e-2 * scale, (e.max().item(), scale)
    assert e.mean().item() < 6e-3 * scale


# ----------------------------------------------------------------------------- c. serving on the toy UNet
def _own(pipe, r, spec):
    """the request's own txt2img(fused=True) with its sampler, noise table and eta"""
    steps, g, opt, extra = spec
    return pipe.txt2img(None, height=128, width=128, num_inference_steps=steps, guidance_scale=g, fused=True,
                        sampler_name=_sampler(extra.get("sampler_name", "sample_dpmpp_2m")), eta=extra.get("eta", 1.0),
                        sampler_opt=dict(opt, **({"solver_type": extra["solver_type"]} if "solver_type" in extra else {})),
                        step_noise=extra.get("step_noise"), latents=r["latents"], region_map_state=r["region_map_state"],
                        prompt_embeds=r["prompt_embeds"], negative_prompt_embeds=r["negative_prompt_embeds"],
                        text_input_ids=r["text_input_ids"], output_type="latent")[0].float().cpu()


def _table(steps, seed):
    return torch.randn(steps, 1, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).half().cuda()


def _submit(b, r, spec):
    steps, g, opt, extra = spec
    return b.submit(dict(r, num_inference_steps=steps, guidance_scale=g, sampler_opt=opt, **extra))


def _mixed_specs(reqs, mixed=True):
    ra, rb, rc, rd = reqs
    K, E = {"scheduler": "karras"}, {"scheduler": "exponential"}
    if not mixed:
        return {"A": (ra, (5, 7.5, K, {})), "B": (rb, (3, 7.5, K, {})), "C": (rc, (4, 5.0, E, {})), "D": (rd, (4, 7.5, K, {}))}
    return {"A": (ra, (5, 7.5, K, {})),
            "B": (rb, (3, 7.5, K, {"sampler_name": "sample_euler_ancestral", "eta": 1.0, "step_noise": _table(3, 1)})),
            "C": (rc, (4, 5.0, E, {"sampler_name": "sample_dpmpp_2m_sde", "solver_type": "heun", "eta": 1.0, "step_noise": _table(4, 2)})),
            "D": (rd, (4, 7.5, K, {"sampler_name": "sample_lcm", "step_noise": _table(4, 3)}))}


def test_batcher_mixed_samplers_equal_their_own_fused_txt2img(ops):
    """Two slots (buckets 1 / 2, the geometry in which test_batcher_staggered_joins_equal_their_own_txt2img observes 0.0): A
    (DPM++ 2M, 5 steps) starts; B (Euler a, 3 steps) joins 2 steps in; both leave; C (DPM++ 2M SDE heun, 4 steps, exponential,
    guidance 5) takes the freed slot 0 and D (LCM, 4 steps) joins it one step in.  Every request's latent is its own
    txt2img(fused=True, step_noise=...)'s, bit for bit; no capture after warm().

    Measured on one MI355X while writing this test: with three requests active in a 4-row bucket the served latents differ from
    the one-image txt2img by up to 3.3e-1 (6e-3 of the range) - and by the same amounts when all four requests are DPM++ 2M on
    the old launch (A: 3.125e-2 in both), i.e. the UNet's kernels round differently at 8 rows than at 2, not the sampler step.
    So bit equality against a one-image run is asserted at the geometry where the UNet itself is bit-stable, and the 4-row
    bucket is covered by test_dpmpp_2m_request_rides_in_the_linear_launch_with_the_same_bits below."""
    cfg, pipe = _tiny_pipe(2)
    specs = _mixed_specs(_tiny_requests(cfg.cross_attention_dim, 4))
    b = pipe.serve(128, 128, max_batch=2, buckets=(1, 2)).warm()
    futs = {"A": _submit(b, *specs["A"])}
    for _ in range(3):
        b.step()
    futs["B"] = _submit(b, *specs["B"])
    for _ in range(4):
        b.step()
    assert b._slots[0] is None and b._slots[1] is None  # A and B have left
    futs["C"] = _submit(b, *specs["C"])
    b.step()
    b.step()
    assert b._slots[0] is not None and b._slots[0].family == "dpmpp_2m_sde"        # A's slot, reused
    futs["D"] = _submit(b, *specs["D"])
    b.step()
    assert b._slots[1] is not None and b._slots[1].family == "lcm"
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["joins"] == 4 and st["leaves"] == 4 and st["linear_transitions"] > 0, st
    for n, (r, spec) in specs.items():
        own = _own(pipe, r, spec)
        got = futs[n].result().float().cpu()
        d = (got - own).abs().max().item()
        print(f"request {n}: vs its own fused txt2img {d:.3e}")
        assert torch.equal(got, own), (n, d)


def test_dpmpp_2m_request_rides_in_the_linear_launch_with_the_same_bits(ops):
    """Three requests active in the 4-row bucket: A (DPM++ 2M) beside Euler a and DPM++ 2M SDE neighbours steps through
    dsc_cfg_linear_step_rows; beside DPM++ 2M neighbours, same timeline, through dsc_cfg_dpmpp2m_step_rows.  Same bucket, same
    rows, nothing in the UNet couples rows: A's latent is the same bits in both batches"""
    outs = {}
    for mixed in (True, False):
        cfg, pipe = _tiny_pipe(2)
        specs = _mixed_specs(_tiny_requests(cfg.cross_attention_dim, 4), mixed)
        b = pipe.serve(128, 128, max_batch=4, buckets=(1, 2, 4)).warm()
        fa = _submit(b, *specs["A"])
        for _ in range(3):
            b.step()
        _submit(b, *specs["B"])
        _submit(b, *specs["C"])
        b.run_until_idle()
        st = b.stats()
        assert (st["linear_transitions"] > 0) == mixed and st["captures_after_warm"] == 0, st
        outs[mixed] = fa.result().float().cpu()
    print(f"A beside other samplers vs beside DPM++ 2M: {(outs[True] - outs[False]).abs().max().item():.3e}")
    assert torch.equal(outs[True], outs[False])


def test_batcher_of_dpmpp_2m_requests_issues_the_old_launch(ops, monkeypatch):
    cfg, pipe = _tiny_pipe(3)
    reqs = _tiny_requests(cfg.cross_attention_dim, 3)
    calls = {"old": 0, "linear": 0}
    old_fn, lin_fn = ops.cfg_dpmpp2m_step_rows, ops.cfg_linear_step_rows
    monkeypatch.setattr(ops, "cfg_dpmpp2m_step_rows", lambda *a, **k: (calls.__setitem__("old", calls["old"] + 1), old_fn(*a, **k))[1])
    monkeypatch.setattr(ops, "cfg_linear_step_rows", lambda *a, **k: (calls.__setitem__("linear", calls["linear"] + 1), lin_fn(*a, **k))[1])
    b = pipe.serve(128, 128, max_batch=4, buckets=(1, 2, 4)).warm()
    K = {"scheduler": "karras"}
    futs = [_submit(b, reqs[0], (4, 7.5, K, {})), _submit(b, reqs[1], (3, 7.5, K, {"sampler_name": "sample_dpmpp_2m"}))]
    b.run_until_idle()
    assert calls["linear"] == 0 and calls["old"] == 5 and all(f.done() for f in futs)         # the join + 4 steps
    f = _submit(b, reqs[2], (2, 7.5, K, {"sampler_name": "sample_euler"}))
    b.run_until_idle()
    assert calls["linear"] == 2 and calls["old"] == 6 and torch.isfinite(f.result()).all()    # its join, then its 2 steps


def test_v_prediction_batcher(ops):
    """a v-prediction pipeline is served: Euler and DPM++ 2M requests in one batch, each its own fused txt2img bit for bit"""
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    cfg, pipe = _tiny_pipe(4)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), pipe.unet, SD15Scheduler(prediction_type="v_prediction"))
    ra, rb = _tiny_requests(cfg.cross_attention_dim, 2)
    K = {"scheduler": "karras"}
    specs = {"A": (ra, (4, 7.5, K, {"sampler_name": "sample_euler"})), "B": (rb, (3, 6.0, K, {}))}
    b = pipe.serve(128, 128, max_batch=2, buckets=(1, 2)).warm()
    futs = {"A": _submit(b, *specs["A"])}
    b.step()
    b.step()
    futs["B"] = _submit(b, *specs["B"])
    b.run_until_idle()
    assert b.stats()["captures_after_warm"] == 0
    for n, (r, spec) in specs.items():
        own = _own(pipe, r, spec)
        got = futs[n].result().float().cpu()
        print(f"v-prediction request {n}: vs its own fused txt2img {(got - own).abs().max().item():.3e}")
        assert torch.equal(got, own), n
    eps_pipe = _tiny_pipe(4)[1]
    assert not torch.equal(_own(eps_pipe, ra, specs["A"][1]), futs["A"].result().float().cpu())       # (v scalars were live)


def test_inpainting_with_euler_is_rejected(ops):
    cfg, pipe = _tiny_pipe(5)
    r = _tiny_requests(cfg.cross_attention_dim, 1)[0]
    b = pipe.serve(128, 128, max_batch=2, buckets=(1, 2))
    with pytest.raises(ValueError, match="mask_image"):
        b.submit(dict(r, sampler_name="sample_euler", image=torch.zeros(1, 4, 16, 16).half().cuda(),
                      mask_image=torch.ones(1, 1, 128, 128)))
    with pytest.raises(ValueError, match="sampler_name"):
        b.submit(dict(r, sampler_name="sample_heun"))


def test_inpainting_beside_euler_ancestral_each_against_its_own_reference(tiny, ops):
    """The known-region launch carries DPM++ 2M records only, so the two never step in one transition: E1 (Euler a) runs,
    inpainting B - submitted two steps in - waits until E1 has left, E2 (Euler a) - submitted while B runs - waits for B.  E1 / E2
    equal their own txt2img(fused=True, step_noise=...) bit for bit (they keep their noise); B is within the served-inpainting
    test's bounds of the fp32 oracle loop (4e-2 max / 6e-3 mean of its range)"""
    pipe = tiny.pipe
    b = pipe.serve(128, 128, max_batch=2, buckets=(1, 2)).warm()
    lats = [torch.randn(1, 4, 16, 16, generator=_gen(500 + i)).half().cuda() for i in range(2)]
    tabs = [_table(4, 50 + i) for i in range(2)]
    euler = lambda i: dict(tiny.base, num_inference_steps=4, latents=lats[i], sampler_name="sample_euler_ancestral",  # noqa: E731
                           eta=1.0, step_noise=tabs[i])
    f1 = b.submit(euler(0))
    for _ in range(3):
        b.step()
    fb = b.submit(dict(tiny.base, image=tiny.lat0.clone(), mask_image=tiny.mask, num_inference_steps=8, generator=_gen(44)))
    b.step()
    assert b._slots[1] is None and b.stats()["queued"] == 1            # B waits for E1
    b.step()
    b.step()
    assert b._slots[0] is not None and b._slots[0].kind == "inpaint"   # E1 has left, B is in
    f2 = b.submit(euler(1))
    b.step()
    assert b._slots[1] is None and b.stats()["queued"] == 1            # E2 waits for B
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["leaves"] == 3 and st["linear_transitions"] == 8, st
    for i, f in enumerate((f1, f2)):
        own = pipe.txt2img(None, num_inference_steps=4, sampler_name="sample_euler_ancestral", latents=lats[i], eta=1.0, fused=True,
                           step_noise=tabs[i], **tiny.common)[0].float().cpu()
        got = f.result().float().cpu()
        print(f"Euler a request {i + 1}: vs its own fused txt2img {(got - own).abs().max().item():.3e}")
        assert torch.equal(got, own), i
        quiet = pipe.txt2img(None, num_inference_steps=4, sampler_name="sample_euler_ancestral", latents=lats[i], eta=0.0, fused=True,
                             **tiny.common)[0].float().cpu()
        assert (got - quiet).abs().max().item() > 2e-2 * own.abs().max().item()      # (a dropped noise term would land here)
    ref = _inpaint_oracle(tiny, 1.0, 44)
    e = (fb.result().float().cpu() - ref).abs()
    sc = ref.abs().max().item()
    print(f"inpainting request: vs oracle max {e.max().item():.3e} mean {e.mean().item():.3e} (range {sc:.2f})")
    assert e.max().item() < 4e-2 * sc and e.mean().item() < 6e-3 * sc


def test_img2img_euler_ancestral_fused_protocol_and_served(tiny, ops):
    """img2img at strength 0.6 of 8 steps (the schedule's tail; img2img hands the sampler no eta: its default 1 holds):
    fused=True with a noise table against fused=False replaying it (2e-2 of the scale, the fused-versus-protocol bound), and the
    served request against the fused call (2e-3 of the range, test_served_img2img_equals_its_own_pipeline_call's bound)"""
    from diffusionspatialcontrol_amd.modules import sampling
    pipe = tiny.pipe
    table = _table(4, 60)                                   # min(int(8 * 0.6), 8) = 4 steps run
    kw = dict(latents=tiny.lat0.clone(), strength=0.6, num_inference_steps=8, **tiny.common)
    fused = pipe.img2img(None, generator=_gen(33), fused=True, sampler_name="sample_euler_ancestral", step_noise=table, **kw)[0]
    proto = pipe.img2img(None, generator=_gen(33), fused=False,
                         sampler_name=functools.partial(sampling.sample_euler_ancestral, noise_sampler=_replay(table)), **kw)[0]
    fused, proto = fused.float().cpu(), proto.float().cpu()
    scale = proto.abs().max().item()
    print(f"img2img Euler a: fused vs protocol {(fused - proto).abs().max().item():.3e} (scale {scale:.2f})")
    assert (fused - proto).abs().max().item() < 2e-2 * scale
    b = pipe.serve(128, 128, max_batch=2, buckets=(1, 2)).warm()
    fut = b.submit(dict(tiny.base, image=tiny.lat0.clone(), strength=0.6, num_inference_steps=8, generator=_gen(33),
                        sampler_name="sample_euler_ancestral", step_noise=table))
    b.run_until_idle()
    d = (fut.result().float().cpu() - fused).abs().max().item()
    print(f"served img2img Euler a vs img2img(fused=True): {d:.3e} (range {scale:.2f})")
    assert d < 2e-3 * scale and b.stats()["linear_transitions"] == 4


# ----------------------------------------------------------------------------- d. full size
def test_full_size_euler_ancestral_joins_a_dpmpp_2m_batch():
    """SD1.5 at 512x512, 25 steps: an Euler a request joins a batch of two DPM++ 2M requests 10 steps in; against its own
    txt2img(fused=True) with the same noise table within the end-to-end bound (8e-3 max / 1e-3 mean of the range)"""
    import test_full_size_parity_gpu as fs
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    with torch.device("cuda"):
        unet = UNet2DConditionModel(UNetConfig.sd15())
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet.half().eval(), SD15Scheduler())
    reqs = [{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in r.items()} for r in fs._requests(3)]
    kw = dict(num_inference_steps=25, guidance_scale=7.5, sampler_opt={"scheduler": "karras"})
    table = torch.randn(25, 1, 4, 64, 64, generator=torch.Generator().manual_seed(9)).half().cuda()
    b = pipe.serve(512, 512, max_batch=4, buckets=(1, 2, 4)).warm()
    b.submit(dict(reqs[1], **kw))
    b.submit(dict(reqs[2], **kw))
    for _ in range(10):
        b.step()
    fut = b.submit(dict(reqs[0], sampler_name="sample_euler_ancestral", eta=1.0, step_noise=table, **kw))
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["linear_transitions"] == 25, st
    got = fut.result().float().cpu()
    r = reqs[0]
    ref = pipe.txt2img(None, height=512, width=512, fused=True, sampler_name="sample_euler_ancestral", eta=1.0, step_noise=table,
                       latents=r["latents"], region_map_state=r["region_map_state"], prompt_embeds=r["prompt_embeds"],
                       negative_prompt_embeds=r["negative_prompt_embeds"], text_input_ids=r["text_input_ids"], output_type="latent",
                       **kw)[0].float().cpu()
    e = (got - ref).abs()
    scale = ref.abs().max().item()
    print(f"Euler a joined at step 10: max {e.max().item():.3e} mean {e.mean().item():.3e} (range {scale:.2f})")
    assert e.max().item() < 8e-3 * scale and e.mean().item() < 1e-3 * scale
