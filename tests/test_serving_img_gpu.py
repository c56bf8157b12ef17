"""img2img / inpainting in the continuous batcher on the MI355X (`-m gpu`): the per-row step with a known region
(dsc_cfg_dpmpp2m_step_rows_known) against the plain per-row step and a restatement of its formulas, and served image requests
against the pipeline's own img2img call and the fp32 CPU oracle loop with the inpainting hook."""
import math

import pytest
import torch
import torch.nn.functional as F

from inputs import FakeTokenizer
from oracle import unet_ref

pytestmark = pytest.mark.gpu
TW = 96


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


def _h(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).half().cuda()


def _params(i):
    return {"mode": 0, "sigma": 14.6 / (i + 1), "guidance": 7.5 - i, "a": 0.8 - 0.05 * i, "b": 0.2 + 0.03 * i,
            "c": 0.0 if i == 0 else -0.01 * i, "c_in_next": 0.07 * (i + 1), "t_next": 900.0 - 50 * i, "sigma_next": 12.0 / (i + 1)}


def _recs(ops, modes, tabs):
    recs = []
    for i, m in enumerate(modes):
        p = _params(i)
        p["mode"] = {"S": ops.ROW_STEP, "J": ops.ROW_JOIN, "I": ops.ROW_IDLE}[m]
        p["temb_row"] = tabs[i] if m != "I" else None
        recs.append(p)
    return recs


def _call(ops, chw, x, eps, old, n_src, n_dst, recs, known=None):
    """-> (x, old, x_in, t, sigma, tadd) after the plain op (known is None) or the known-region op, on copies"""
    x, old = x.clone(), old.clone()
    x_in = torch.full((2 * n_dst, chw), 7.0, dtype=torch.float16, device="cuda")
    t = torch.full((2 * n_dst,), -1.0, device="cuda")
    s = torch.full((n_dst,), -1.0, device="cuda")
    tadd = torch.zeros(2 * n_dst, TW, dtype=torch.float16, device="cuda")
    if known is None:
        ops.cfg_dpmpp2m_step_rows(x, eps, old, n_src, x_in, t, s, recs, tadd=tadd)
    else:
        ops.cfg_dpmpp2m_step_rows_known(x, eps, old, n_src, x_in, t, s, recs, known, tadd=tadd)
    torch.cuda.synchronize()
    return x, old, x_in, t, s, tadd


def _inputs(n_slots, n_src, chw, seed):
    return (_h(n_slots, chw, seed=seed), _h(2 * n_src, chw, seed=seed + 1), _h(n_slots, chw, seed=seed + 2),
            [_h(TW, seed=seed + 10 + i) for i in range(n_slots)])


def _f32(v):
    return torch.tensor(v, dtype=torch.float32).double()


def _fma(a, b, c):
    """fp32 fused multiply-add: the exact product and sum (fp64 holds the product of two fp32 values exactly), one rounding"""
    return (a.double() * b.double() + c.double()).float()


def _restate(x, eu, ec, old, p, img, noise, mask, now, nxt):
    """the header's formulas for one known slot (include/dsc_hip.h), every multiply-add as an fp32 fma, fp16 where marked
    -> (x', old', x_in row)"""
    x, eu, ec, old, img, noise, mask = (v.float().cpu() for v in (x, eu, ec, old, img, noise, mask))
    sg, g, a, b, c, cn, sn = (_f32(p[k]).float() for k in ("sigma", "guidance", "a", "b", "c", "c_in_next", "sigma_next"))
    e = _fma(g, ec - eu, eu)
    kn = lambda s_: _fma(s_, noise, img)                                    # noqa: E731
    blend = lambda v, s_: _fma(mask, v, (1.0 - mask) * kn(s_))              # noqa: E731
    xh = blend(x, sg) if now else x
    d = _fma(-sg, e, xh).half().float()
    xn = _fma(c, old, _fma(a, x, b * d)).half().float()
    xo = blend(xn, sn) if nxt else xn
    return xn.half(), d.half(), (xo * cn).half()


def _ulps(a, b):
    def key(v):
        i = v.cpu().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs().max().item()


@pytest.mark.parametrize("chw", [1024, 1444, 2056, 16384])
@pytest.mark.parametrize("n_src, n_dst, modes", [(2, 4, "SSJI"), (4, 2, "SISI"), (4, 4, "JSIS")])
def test_known_all_null_is_the_plain_op(ops, chw, n_src, n_dst, modes):
    """no slot has a known region: every output buffer carries the bits of dsc_cfg_dpmpp2m_step_rows"""
    x, eps, old, tabs = _inputs(len(modes), n_src, chw, seed=31)
    recs = _recs(ops, modes, tabs)
    plain = _call(ops, chw, x, eps, old, n_src, n_dst, recs)
    got = _call(ops, chw, x, eps, old, n_src, n_dst, recs, known=[None] * len(modes))
    for name, a, b in zip(("x", "old", "x_in", "t", "sigma", "tadd"), got, plain):
        assert torch.equal(a, b), (modes, name)


@pytest.mark.parametrize("chw", [1024, 16384])
def test_known_mask_of_ones_and_mask_of_zeros(ops, chw):
    """mask == 1 everywhere with both blends on: the plain op's bits.  mask == 0 everywhere: the next model input is
    fp16(fma(sigma_next, noise, image) * c_in_next) and old = fp16(kn(sigma) - sigma * e) whatever x holds, while x' still
    follows the unblended x"""
    n = 3
    x, eps, old, tabs = _inputs(n, n, chw, seed=41)
    recs = _recs(ops, "SSS", tabs)
    img, noise = _h(n, chw, seed=47), _h(n, chw, seed=48)
    plain = _call(ops, chw, x, eps, old, n, n, recs)
    ones = torch.ones(chw, dtype=torch.float16, device="cuda")
    known = [{"image": img[i], "noise": noise[i], "mask": ones, "blend_now": True, "blend_next": True} for i in range(n)]
    got = _call(ops, chw, x, eps, old, n, n, recs, known=known)
    for name, a, b in zip(("x", "old", "x_in", "t", "sigma", "tadd"), got, plain):
        assert torch.equal(a, b), name
    zeros = torch.zeros(chw, dtype=torch.float16, device="cuda")
    known = [dict(k, mask=zeros) for k in known]
    got = _call(ops, chw, x, eps, old, n, n, recs, known=known)
    other = _call(ops, chw, _h(n, chw, seed=49), eps, old, n, n, recs, known=known)           # another x altogether
    assert torch.equal(got[1], other[1]) and torch.equal(got[2], other[2])                    # old and x_in do not see x
    for i in range(n):
        p = recs[i]
        xn, d, xi = _restate(x[i], eps[i], eps[n + i], old[i], p, img[i], noise[i], zeros, True, True)
        kn_next = _fma(_f32(p["sigma_next"]).float(), noise[i].float().cpu(), img[i].float().cpu())
        assert torch.equal(xi, (kn_next * _f32(p["c_in_next"]).float()).half())
        assert torch.equal(got[2][i].cpu(), xi) and torch.equal(got[2][n + i].cpu(), xi), i
        assert torch.equal(got[1][i].cpu(), d), i
        # x' = fma(c, old, fma(a, x, b * D)) with the blended D but the sampler's own x
        assert torch.equal(got[0][i].cpu(), xn), i
    assert not torch.equal(got[0], other[0])


@pytest.mark.parametrize("chw", [1024, 1444, 2056, 16384])
def test_known_mixed_slots_against_the_formulas(ops, chw):
    """half / half 0-1 mask; slots: known (both blends), plain STEP, JOIN, a known slot on its first step (blend_next only)
    IDLE, and a known slot at i >= n_dst that leaves (blend_now only).  Known slots: at most 1 fp16 ulp from the restated
    formulas; every slot without a record: the plain op's bits"""
    modes, n_src, n_dst = "SSJSIS", 6, 5
    x, eps, old, tabs = _inputs(6, n_src, chw, seed=61)
    recs = _recs(ops, modes, tabs)
    recs[5].update(c_in_next=0.0, t_next=0.0, sigma_next=1.0, temb_row=None)                  # leaves
    img, noise = _h(6, chw, seed=67), _h(6, chw, seed=68)
    mask = torch.zeros(chw, dtype=torch.float16, device="cuda")
    mask[chw // 2:] = 1.0
    flags = {0: (True, True), 3: (False, True), 5: (True, False)}
    known = [None] * 6
    for i, (now, nxt) in flags.items():       # (clones: row i of a [6, 1444] tensor is 8-byte aligned only, the entry wants 16)
        known[i] = {"image": img[i].clone(), "noise": noise[i].clone(), "mask": mask, "blend_now": now, "blend_next": nxt}
    known[2] = {"image": img[2], "noise": noise[2], "mask": mask, "blend_now": True, "blend_next": True}      # JOIN ignores it
    plain = _call(ops, chw, x, eps, old, n_src, n_dst, recs)
    got = _call(ops, chw, x, eps, old, n_src, n_dst, recs, known=known)
    worst = 0
    for i, (now, nxt) in flags.items():
        xn, d, xi = _restate(x[i], eps[i], eps[n_src + i], old[i], recs[i], img[i], noise[i], mask, now, nxt)
        u = [_ulps(got[0][i], xn), _ulps(got[1][i], d)]
        if i < n_dst:
            u += [_ulps(got[2][i], xi), _ulps(got[2][n_dst + i], xi)]
        worst = max(worst, *u)
        print(f"chw {chw} slot {i} (blend_now {now}, blend_next {nxt}): ulps x' / old / x_in = {u}")
        assert max(u) <= 1, (i, u)
        half = chw // 2
        assert torch.equal(got[1][i, half:], plain[1][i, half:])            # mask == 1: the model input is x itself
        if i < n_dst:
            assert torch.equal(got[2][i, half:], plain[2][i, half:])
        if now:
            assert not torch.equal(got[1][i, :half], plain[1][i, :half])    # mask == 0: the known region went in
    for i in (1, 2, 4):
        assert torch.equal(got[0][i], plain[0][i]) and torch.equal(got[1][i], plain[1][i]), i
        assert torch.equal(got[2][[i, n_dst + i]], plain[2][[i, n_dst + i]]), i
    assert torch.equal(got[3], plain[3]) and torch.equal(got[4], plain[4]) and torch.equal(got[5], plain[5])


def test_known_refuses_partial_records_and_misaligned_rows(ops):
    """one of the three pointers NULL, or a row that is not 16-byte aligned: DscLibraryError before any launch, nothing written"""
    from diffusionspatialcontrol_amd import DscLibraryError
    chw, n = 1024, 2
    x, eps, old, tabs = _inputs(n, n, chw, seed=71)
    recs = _recs(ops, "SS", tabs)
    img, noise = _h(n, chw, seed=77), _h(n, chw, seed=78)
    ones = torch.ones(chw, dtype=torch.float16, device="cuda")
    buf = _h(chw + 8, seed=79)
    good = {"image": img[1], "noise": noise[1], "mask": ones, "blend_now": True, "blend_next": True}
    for bad in (dict(good, noise=None), dict(good, image=None), dict(good, mask=None), dict(good, mask=buf[4:4 + chw])):
        xr, oldr = x.clone(), old.clone()
        x_in = torch.full((2 * n, chw), 7.0, dtype=torch.float16, device="cuda")
        t = torch.full((2 * n,), -1.0, device="cuda")
        s = torch.full((n,), -1.0, device="cuda")
        tadd = torch.zeros(2 * n, TW, dtype=torch.float16, device="cuda")
        with pytest.raises(DscLibraryError):
            ops.cfg_dpmpp2m_step_rows_known(xr, eps, oldr, n, x_in, t, s, recs, [None, bad], tadd=tadd)
        torch.cuda.synchronize()
        assert torch.equal(xr, x) and torch.equal(oldr, old) and (x_in == 7.0).all() and (t == -1.0).all() and not tadd.any()
    with pytest.raises(ValueError):
        ops.cfg_dpmpp2m_step_rows_known(x.clone(), eps, old.clone(), n, x_in, t, s, recs, [None, dict(good, image=img[1].float())],
                                        tadd=tadd)


# ----------------------------------------------------------------------------- the batcher on the tiny UNet at 128x128
STEPS = 8
OPT = {"scheduler": "karras"}


@pytest.fixture(scope="module")
def tiny():
    import types
    import test_unet_pipeline_gpu as up
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKL, VaeConfig
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    cfg, unet, sd, text = up._tiny_setup(1)
    state, ids, rs = up._region_state(n_img=1)
    torch.manual_seed(12)
    vae = AutoencoderKL(VaeConfig.tiny()).half().cuda().eval()
    pipe = StableDiffusionPipeline(vae, None, FakeTokenizer(), unet, SD15Scheduler())
    lat0 = (torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(21)) * 0.8).half()
    mask = torch.zeros(1, 1, 128, 128)
    mask[..., 64:] = 1.0                                   # left half kept, right half repainted
    base = {"prompt_embeds": text[1:2].cuda(), "negative_prompt_embeds": text[:1].cuda(), "text_input_ids": ids,
            "region_map_state": state, "guidance_scale": 7.5, "sampler_opt": OPT}
    common = dict(guidance_scale=7.5, output_type="latent", region_map_state=state, sampler_opt=OPT, prompt_embeds=text[1:2],
                  negative_prompt_embeds=text[:1], text_input_ids=ids, width=128, height=128)
    sig = pipe.get_sigmas(STEPS, OPT).half().float().cpu()
    return types.SimpleNamespace(cfg=cfg, sd=sd, text=text, rs=rs, pipe=pipe, lat0=lat0, mask=mask, base=base, common=common,
                                 sig=sig)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _inpaint_oracle(tn, strength, seed, steps=STEPS):
    """the fp32 CPU loop (DPM++ 2M) with the hook of test_img2img_and_inpainting_pipeline, from the pipeline method's start"""
    sig = tn.pipe.get_sigmas(steps, OPT).half().float().cpu()
    t_start = steps - min(int(steps * strength), steps)
    sched = sig[t_start:]
    n = torch.randn(tn.lat0.shape, generator=_gen(seed), dtype=torch.float16).float()
    img = tn.lat0.float()
    m16 = F.interpolate(tn.mask, size=(16, 16))

    def hook(x, sigma, k):
        if k == 0:
            return x
        s = float(sigma[0])
        known = img + s * n if s > 0 else img
        return (1 - m16) * known + m16 * x
    start = n * math.sqrt(float(sched[0]) ** 2 + 1) if strength == 1.0 else img + float(sched[0]) * n
    return unet_ref.denoise_loop(tn.sd, tn.cfg, start, sched.tolist(), tn.text.float(), tn.rs, 7.5, input_hook=hook)


def _own_img2img(tn, strength, seed, steps=STEPS):
    return tn.pipe.img2img(None, latents=tn.lat0.clone(), strength=strength, generator=_gen(seed), fused=True,
                           num_inference_steps=steps, sampler_name="sample_dpmpp_2m", **tn.common)[0].float().cpu()


def test_served_img2img_equals_its_own_pipeline_call(tiny):
    """`image` = 4-channel latents, strength 0.6, 8 steps, seeded generator: within 2e-3 of the range of pipe.img2img(fused)"""
    b = tiny.pipe.serve(128, 128, max_batch=2, buckets=(1, 2)).warm()
    fut = b.submit(dict(tiny.base, image=tiny.lat0.clone(), strength=0.6, num_inference_steps=STEPS, generator=_gen(33)))
    b.run_until_idle()
    got = fut.result().float().cpu()
    ref = _own_img2img(tiny, 0.6, 33)
    scale = ref.abs().max().item()
    d = (got - ref).abs().max().item()
    txt = _served_txt2img(tiny, b, seed=33)
    print(f"served img2img vs pipe.img2img: {d:.3e} (range {scale:.2f}); a txt2img answer would be "
          f"{(txt - ref).abs().max().item():.3e} away")
    assert d < 2e-3 * scale, (d, scale)
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["steps"] >= int(STEPS * 0.6)


def _served_txt2img(tn, b, seed):
    fut = b.submit(dict(tn.base, num_inference_steps=STEPS, generator=_gen(seed)))
    b.run_until_idle()
    return fut.result().float().cpu()


@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_served_inpainting_against_the_oracle(tiny, strength):
    """left half kept: within 4e-2 max / 6e-3 mean of the oracle's range (test_img2img_and_inpainting_pipeline's bounds for this
    UNet); pipe.inpaiting in protocol mode on the same request is printed beside it, and the served result may not be further
    from the oracle than that by more than the fused-versus-protocol spread allowed there (2e-2 of the range)"""
    b = tiny.pipe.serve(128, 128, max_batch=2, buckets=(1, 2)).warm()
    fut = b.submit(dict(tiny.base, image=tiny.lat0.clone(), mask_image=tiny.mask, strength=strength,
                        num_inference_steps=STEPS, generator=_gen(44)))
    b.run_until_idle()
    got = fut.result().float().cpu()
    ref = _inpaint_oracle(tiny, strength, 44)
    proto = tiny.pipe.inpaiting(None, image=tiny.lat0.clone(), mask_image=tiny.mask, strength=strength, generator=_gen(44),
                                num_inference_steps=STEPS, sampler_name="sample_dpmpp_2m", **tiny.common)[0].float().cpu()
    sc = ref.abs().max().item()
    e, ep = (got - ref).abs(), (proto - ref).abs()
    print(f"inpainting strength {strength}: served vs oracle max {e.max().item():.3e} mean {e.mean().item():.3e}; protocol-mode "
          f"inpaiting vs oracle max {ep.max().item():.3e} mean {ep.mean().item():.3e}; served vs protocol "
          f"{(got - proto).abs().max().item():.3e} (range {sc:.2f})")
    assert e.max().item() < 4e-2 * sc and e.mean().item() < 6e-3 * sc, (e.max().item(), e.mean().item(), sc)
    assert e.max().item() <= ep.max().item() + 2e-2 * sc
    assert b.stats()["captures_after_warm"] == 0


def test_mixed_batch_txt2img_inpainting_img2img(tiny):
    """txt2img A (4 steps) starts; inpainting B joins after 2 steps; img2img C joins into the slot A frees.  A against its own
    txt2img and C against its own img2img: 2e-3 of the range; B against the oracle: 4e-2 max / 6e-3 mean; no capture"""
    pipe = tiny.pipe
    b = pipe.serve(128, 128, max_batch=4, buckets=(1, 2, 4)).warm()
    lat_a = torch.randn(1, 4, 16, 16, generator=_gen(400)).half().cuda()
    fa = b.submit(dict(tiny.base, num_inference_steps=4, latents=lat_a))
    for _ in range(3):                                   # A joins, then two of its steps
        b.step()
    fb = b.submit(dict(tiny.base, image=tiny.lat0.clone(), mask_image=tiny.mask, num_inference_steps=STEPS, generator=_gen(44)))
    b.step()
    b.step()
    assert b._slots[0] is None and b._slots[1] is not None and b._slots[1].kind == "inpaint"     # A has left
    fc = b.submit(dict(tiny.base, image=tiny.lat0.clone(), strength=0.6, num_inference_steps=STEPS, generator=_gen(33)))
    b.step()
    assert b._slots[0] is not None and b._slots[0].kind == "img2img"
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["joins"] == 3 and st["leaves"] == 3, st
    own_a = pipe.txt2img(None, num_inference_steps=4, sampler_name="sample_dpmpp_2m", latents=lat_a,
                         **tiny.common)[0].float().cpu()
    own_c = _own_img2img(tiny, 0.6, 33)
    scale = max(own_a.abs().max().item(), own_c.abs().max().item())
    for name, got, own in (("A", fa.result(), own_a), ("C", fc.result(), own_c)):
        d = (got.float().cpu() - own).abs().max().item()
        print(f"mixed batch, request {name}: vs its own pipeline call {d:.3e} (range {scale:.2f})")
        assert d < 2e-3 * scale, (name, d, scale)
    ref = _inpaint_oracle(tiny, 1.0, 44)
    e = (fb.result().float().cpu() - ref).abs()
    sc = ref.abs().max().item()
    print(f"mixed batch, request B: vs oracle max {e.max().item():.3e} mean {e.mean().item():.3e} (range {sc:.2f})")
    assert e.max().item() < 4e-2 * sc and e.mean().item() < 6e-3 * sc


def test_pixels_in_equal_latents_in(tiny):
    """`image` as [1, 3, 128, 128] pixels runs through the tiny VAE's encoder and equals the same request given
    pipe._encode_vae_image(image, <same seed>) as latents (the generator then stands where the encoder left it), bit for bit"""
    pipe = tiny.pipe
    img = torch.rand(1, 3, 128, 128, generator=_gen(2)) * 2 - 1
    b = pipe.serve(128, 128, max_batch=2, buckets=(1, 2)).warm()
    kw = dict(tiny.base, strength=0.6, num_inference_steps=5)
    f_px = b.submit(dict(kw, image=img, generator=_gen(9)))
    b.run_until_idle()
    g = _gen(9)
    lat = pipe._encode_vae_image(img, g)
    assert lat.shape == (1, 4, 16, 16)
    f_lat = b.submit(dict(kw, image=lat, generator=g))
    b.run_until_idle()
    px, lt = f_px.result(), f_lat.result()
    assert torch.isfinite(px).all() and torch.equal(px, lt), (px - lt).abs().max().item()
    f_in = b.submit(dict(kw, image=img, mask_image=tiny.mask, generator=_gen(9)))          # inpainting from pixels runs too
    b.run_until_idle()
    assert torch.isfinite(f_in.result()).all() and not torch.equal(f_in.result(), px)


# ----------------------------------------------------------------------------- full size
def test_full_size_inpainting_joins_mid_batch():
    """SD1.5 at 512x512, 25 steps: an inpainting request at strength 1.0 joins a batch 10 steps into a txt2img request.  The
    fp32 CPU oracle loop with a hook takes minutes at this size, so the comparison here is with pipe.inpaiting in protocol
    mode (the eager hook) on the same request, inside the end-to-end bound (8e-3 max / 1e-3 mean of the range); the oracle
    comparison is pinned at the tiny size (test_served_inpainting_against_the_oracle)"""
    import test_full_size_parity_gpu as fs
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    with torch.device("cuda"):
        unet = UNet2DConditionModel(UNetConfig.sd15())
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet.half().eval(), SD15Scheduler())
    reqs = [{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in r.items()} for r in fs._requests(2)]
    first, inp = reqs[1], reqs[0]
    img_lat = (torch.randn(1, 4, 64, 64, generator=_gen(5)) * 0.8).half().cuda()
    mask = torch.zeros(1, 1, 512, 512)
    mask[..., 256:] = 1.0
    kw = dict(num_inference_steps=25, guidance_scale=7.5, sampler_opt=OPT)
    b = pipe.serve(512, 512, max_batch=2, buckets=(1, 2)).warm()
    b.submit(dict(first, **kw))
    for _ in range(10):
        b.step()
    fut = b.submit(dict(inp, image=img_lat, mask_image=mask, strength=1.0, **kw))          # `latents` is the noise
    b.run_until_idle()
    assert b.stats()["captures_after_warm"] == 0
    got = fut.result().float().cpu()
    ref = pipe.inpaiting(None, image=img_lat, mask_image=mask, strength=1.0, latents=inp["latents"], height=512, width=512,
                         sampler_name="sample_dpmpp_2m", output_type="latent", region_map_state=inp["region_map_state"],
                         prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"],
                         text_input_ids=inp["text_input_ids"], **kw)[0].float().cpu()
    e = (got - ref).abs()
    scale = ref.abs().max().item()
    print(f"inpainting joined at step 10 vs protocol-mode inpaiting: max {e.max().item():.3e} mean {e.mean().item():.3e} "
          f"(range {scale:.2f})")
    assert e.max().item() < 8e-3 * scale and e.mean().item() < 1e-3 * scale
