"""9-channel inpainting UNets on the hot path, on the MI355X (`-m gpu`): dsc_cfg_linear_step_rows_cat against the two entries it
shares its arithmetic with (bit for bit) and a CPU restatement of its extra channels, its refusals, `inpaiting(fused=True)` against
protocol mode and the CPU oracle, and a batcher built with `inpaint_unet=True`."""
import dataclasses
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from inputs import FakeTokenizer
from oracle import unet_ref

from test_serving_gpu import _h, _params
from test_unet_pipeline_gpu import _region_state

pytestmark = pytest.mark.gpu
TW = 96
OPT = {"scheduler": "karras"}
SENTINEL = 7.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------- a. the kernel
# slot:  0 STEP (eps scalars)   1 STEP + noise (v scalars)   2 JOIN   3 IDLE (handed a row all the same: zeros)
#        4 STEP, extra = None (v scalars)   5 STEP at i >= n_dst (a request that leaves; eps scalars)
MODES, N_SRC, N_DST = "SSJISS", 6, 5
# (2056, 8): 257 latent vectors - a second workgroup with one live lane - and a single vector of extra channels;
# (8200, 16): 1025 vectors - the second pass of an owned slot's 1024-thread loop with one live lane
SHAPES = [(64, 80), (288, 360), (1024, 1280), (16384, 20480), (2056, 8), (8200, 16)]


def _case(ops, chw, eh, rescale=()):
    n = len(MODES)
    x, eps, old = _h(n, chw, seed=11), _h(2 * N_SRC, chw, seed=12), _h(n, chw, seed=13)
    noise, extra = _h(n, chw, seed=14), _h(n, eh, seed=15)
    tabs = [_h(TW, seed=20 + i) for i in range(n)]
    recs = []
    for i, m in enumerate(MODES):
        p = _params(i)
        p["mode"] = {"S": ops.ROW_STEP, "J": ops.ROW_JOIN, "I": ops.ROW_IDLE}[m]
        p["temb_row"] = tabs[i] if m != "I" else None
        recs.append(p)
    recs[5].update(c_in_next=0.0, t_next=0.0, sigma_next=1.0, temb_row=None)
    for i in (0, 5):
        recs[i].update(c_skip=1.0, c_out=-recs[i]["sigma"])
    for i in (1, 4):
        sg = recs[i]["sigma"]
        recs[i].update(c_skip=1.0 / (sg * sg + 1.0), c_out=-sg / math.sqrt(sg * sg + 1.0))
    recs[1].update(s=0.4, noise=noise[1])
    for i in rescale:
        recs[i]["rescale"] = 0.7
    extras = [extra[0], extra[1], extra[2], extra[3], None, extra[5]]
    return x, eps, old, recs, extra, extras


def _buffers(row):
    """sentinel-filled destinations of bucket N_DST with two rows (one entry) of slack behind each: what a slot >= N_DST would hit"""
    back = {"x_in": torch.full((2 * N_DST + 2, row), SENTINEL, dtype=torch.float16, device="cuda"),
            "t": torch.full((2 * N_DST + 2,), -1.0, device="cuda"), "s": torch.full((N_DST + 1,), -1.0, device="cuda"),
            "tadd": torch.full((2 * N_DST + 2, TW), SENTINEL, dtype=torch.float16, device="cuda")}
    view = {"x_in": back["x_in"][:2 * N_DST], "t": back["t"][:2 * N_DST], "s": back["s"][:N_DST], "tadd": back["tadd"][:2 * N_DST]}
    return back, view


def _run(fn, x, eps, old, recs, row, extras=None):
    x, old = x.clone(), old.clone()
    back, v = _buffers(row)
    args = (x, eps, old, N_SRC, v["x_in"], v["t"], v["s"], recs) + (() if extras is None else (extras,))
    fn(*args, tadd=v["tadd"])
    torch.cuda.synchronize()
    return {"x": x, "old": old, "x_in": v["x_in"], "t": v["t"], "sigma_groups": v["s"], "tadd": v["tadd"]}, back


def _check_against(ops, chw, eh, got, back, want, recs, extra):
    for name in ("x", "old", "t", "sigma_groups", "tadd"):
        assert torch.equal(got[name], want[name]), name
    assert torch.equal(got["x_in"][:, :chw], want["x_in"]), "x_in[:, :chw]"
    tail = got["x_in"][:, chw:].cpu()
    for i in (0, 1, 2):                                   # STEP, STEP + noise, JOIN: extra * c_in_next, fp32 with one rounding
        exp = (extra[i].float().cpu() * torch.tensor(recs[i]["c_in_next"], dtype=torch.float32)).half()
        assert exp.abs().max().item() > 0
        assert torch.equal(tail[i], exp) and torch.equal(tail[N_DST + i], exp), i
    for i in (3, 4):                                      # IDLE (whatever it is handed), STEP with extra = None
        assert not tail[i].any() and not tail[N_DST + i].any(), i
    assert not got["x_in"][3].any() and not got["x_in"][N_DST + 3].any()     # an IDLE slot's whole row
    # slot 5 >= N_DST wrote no destination row: the entries behind each buffer keep their fill (and row 5 = slot 0's second row,
    # compared above)
    assert (back["x_in"][2 * N_DST:] == SENTINEL).all() and (back["tadd"][2 * N_DST:] == SENTINEL).all()
    assert (back["t"][2 * N_DST:] == -1.0).all() and (back["s"][N_DST:] == -1.0).all()


@pytest.mark.parametrize("chw, eh", SHAPES)
def test_cat_is_the_linear_entry_plus_the_extra_channels(ops, chw, eh):
    """x, old, t_buf, sigma_groups, tadd and x_in[:, :chw]: the bits of dsc_cfg_linear_step_rows on a 4-channel x_in; the extra
    channels: (extra.float() * float32(c_in_next)).half() from the CPU in both rows, zeros for IDLE / None"""
    x, eps, old, recs, extra, extras = _case(ops, chw, eh)
    want, _ = _run(ops.cfg_linear_step_rows, x, eps, old, recs, chw)
    got, back = _run(ops.cfg_linear_step_rows_cat, x, eps, old, recs, chw + eh, extras)
    assert not torch.equal(got["x"], x)
    _check_against(ops, chw, eh, got, back, want, recs, extra)


@pytest.mark.parametrize("chw, eh", SHAPES)
def test_cat_with_rescale_is_the_rescale_entry_plus_the_extra_channels(ops, chw, eh):
    """phi = 0.7 on slots 0 and 4: dsc_cfg_linear_step_rows_rescale's bits, the same extra channels, and two calls agree"""
    x, eps, old, recs, extra, extras = _case(ops, chw, eh, rescale=(0, 4))
    plain, _ = _run(ops.cfg_linear_step_rows_cat, x, eps, old, [{k: v for k, v in r.items() if k != "rescale"} for r in recs],
                    chw + eh, extras)
    want, _ = _run(ops.cfg_linear_step_rows_rescale, x, eps, old, recs, chw)
    got, back = _run(ops.cfg_linear_step_rows_cat, x, eps, old, recs, chw + eh, extras)
    again, _ = _run(ops.cfg_linear_step_rows_cat, x, eps, old, recs, chw + eh, extras)
    _check_against(ops, chw, eh, got, back, want, recs, extra)
    for name in got:
        assert torch.equal(got[name], again[name]), name
    assert not torch.equal(got["x"][0], plain["x"][0]) and torch.equal(got["x"][1], plain["x"][1])    # (phi matters, per slot)


def test_cat_refusals_write_nothing(ops):
    """extra_halfs of 4 and of 0, a misaligned extra, chw % 8 != 0: DscLibraryError before any launch; a float extra: ValueError;
    the sentinel-filled outputs stay as they were"""
    from diffusionspatialcontrol_amd import DscLibraryError
    n = 2

    def attempt(chw, eh, extras, error):
        x, eps, old = _h(n, chw, seed=51), _h(2 * n, chw, seed=52), _h(n, chw, seed=53)
        tabs = [_h(TW, seed=54 + i) for i in range(n)]
        recs = [dict(_params(i), temb_row=tabs[i]) for i in range(n)]
        xr, oldr = x.clone(), old.clone()
        x_in = torch.full((2 * n, chw + eh), SENTINEL, dtype=torch.float16, device="cuda")
        t = torch.full((2 * n,), -1.0, device="cuda")
        s = torch.full((n,), -1.0, device="cuda")
        tadd = torch.zeros(2 * n, TW, dtype=torch.float16, device="cuda")
        with pytest.raises(error):
            ops.cfg_linear_step_rows_cat(xr, eps, oldr, n, x_in, t, s, recs, extras, tadd=tadd)
        torch.cuda.synchronize()
        assert torch.equal(xr, x) and torch.equal(oldr, old) and (x_in == SENTINEL).all() and (t == -1.0).all() \
            and (s == -1.0).all() and not tadd.any(), (chw, eh)

    chw, eh = 1024, 1280
    buf = _h(eh + 8, seed=59)
    attempt(chw, 4, [_h(4, seed=60), None], DscLibraryError)
    attempt(chw, 0, [None, None], DscLibraryError)
    attempt(chw, eh, [buf[:eh], buf[4:4 + eh]], DscLibraryError)
    attempt(1020, eh, [buf[:eh], None], DscLibraryError)
    attempt(chw, eh, [buf[:eh], buf[:eh].float()], ValueError)
    # and the same call with nothing wrong goes through
    x, eps, old = _h(n, chw, seed=51), _h(2 * n, chw, seed=52), _h(n, chw, seed=53)
    x_in = torch.full((2 * n, chw + eh), SENTINEL, dtype=torch.float16, device="cuda")
    ops.cfg_linear_step_rows_cat(x, eps, old, n, x_in, torch.zeros(2 * n, device="cuda"), torch.zeros(n, device="cuda"),
                                 [_params(i) for i in range(n)], [buf[:eh], None])
    torch.cuda.synchronize()
    assert not (x_in == SENTINEL).any()


# ----------------------------------------------------------------------------- b. the fused loop on the tiny 9-channel UNet
STEPS = 6


@pytest.fixture(scope="module")
def nine():
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKL, VaeConfig
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.manual_seed(4)
    cfg = dataclasses.replace(UNetConfig.tiny(), in_channels=9)
    unet = UNet2DConditionModel(cfg).half()
    sd = {k: v.clone() for k, v in unet.state_dict().items()}
    unet = unet.cuda()
    g = _gen(7)
    text = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half()
    state, ids, rs = _region_state(n_img=1)
    torch.manual_seed(12)
    vae = AutoencoderKL(VaeConfig.tiny()).half().cuda().eval()
    pipe = StableDiffusionPipeline(vae, None, FakeTokenizer(), unet, SD15Scheduler())
    img_lat = (torch.randn(1, 4, 16, 16, generator=g) * 0.7).half()
    mil = (torch.randn(1, 4, 16, 16, generator=g) * 0.7).half()
    lat = torch.randn(1, 4, 16, 16, generator=g).half()
    mask = torch.zeros(1, 1, 128, 128)
    mask[..., 32:96] = 1.0
    mask2 = torch.zeros(1, 1, 128, 128)
    mask2[..., :48, :] = 1.0
    common = dict(height=128, width=128, guidance_scale=7.5, output_type="latent", region_map_state=state, sampler_opt=OPT,
                  prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], text_input_ids=ids)
    base = {"prompt_embeds": text[1:2].cuda(), "negative_prompt_embeds": text[:1].cuda(), "text_input_ids": ids,
            "region_map_state": state, "guidance_scale": 7.5, "sampler_opt": OPT}
    table = torch.randn(STEPS, 1, 4, 16, 16, generator=_gen(8)).half().cuda()
    return types.SimpleNamespace(cfg=cfg, sd=sd, text=text, rs=rs, pipe=pipe, img_lat=img_lat, mil=mil, lat=lat, mask=mask,
                                 mask2=mask2, common=common, base=base, table=table)


def _inpaint(nn, **kw):
    args = dict(image=nn.img_lat.clone(), mask_image=nn.mask, masked_image_latents=nn.mil.clone(), latents=nn.lat.clone(),
                num_inference_steps=STEPS, eta=1.0)
    args.update(nn.common)
    args.update(kw)
    return nn.pipe.inpaiting(None, **args)[0].float().cpu()


def _replay(table):
    order = iter(range(table.shape[0]))
    return lambda *_: table[next(order)]


def _count_cat_launches(monkeypatch, ops):
    """the calls of ops.cfg_linear_step_rows_cat from here on (`fused=` must not be swallowed into protocol mode)"""
    calls, real = [], ops.cfg_linear_step_rows_cat

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "cfg_linear_step_rows_cat", counted)
    return calls


@pytest.mark.parametrize("name, phi", [("sample_dpmpp_2m", 0.0), ("sample_euler", 0.0), ("sample_euler_ancestral", 0.0),
                                       ("sample_euler", 0.7)])
def test_fused_inpaiting_equals_protocol(ops, nine, monkeypatch, name, phi):
    """6 steps on the tiny 9-channel pipe: inpaiting(fused=True) - the first input and every step one launch of the new entry -
    against fused=False (Euler a: with its noise table replayed to protocol mode) within the project's fused-versus-protocol
    bound, 2e-2 of the range"""
    from diffusionspatialcontrol_amd.modules import sampling
    fn = getattr(sampling, name)
    noisy = name == "sample_euler_ancestral"
    launches = _count_cat_launches(monkeypatch, ops)
    fused = _inpaint(nine, fused=True, sampler_name=fn, guidance_rescale=phi, step_noise=nine.table if noisy else None)
    assert len(launches) == STEPS + 1
    proto = _inpaint(nine, fused=False, sampler_name=functools.partial(fn, noise_sampler=_replay(nine.table)) if noisy else fn,
                     guidance_rescale=phi)
    assert len(launches) == STEPS + 1                     # (protocol mode: none)
    scale = proto.abs().max().item()
    err = (fused - proto).abs().max().item()
    print(f"9-channel {name} phi {phi}: fused vs protocol {err:.3e} (range {scale:.2f})")
    assert fused.shape == (1, 4, 16, 16) and torch.isfinite(fused).all() and err < 2e-2 * scale, (err, scale)
    if noisy:                                             # the table is live: other noise, another image
        other = _inpaint(nine, fused=True, sampler_name=fn, step_noise=nine.table.flip(0).contiguous())
        assert (other - fused).abs().max().item() > 2e-2 * scale
    if phi > 0.0:                                         # ... and so is the rescale
        assert (_inpaint(nine, fused=True, sampler_name=fn) - fused).abs().max().item() > 0


def test_fused_inpaiting_against_the_cpu_oracle(ops, nine, monkeypatch):
    """sample_euler, fused, against unet_ref.denoise_loop with the same extra channels: test_inpainting_9_channel_unet's bounds"""
    from diffusionspatialcontrol_amd.modules import sampling
    launches = _count_cat_launches(monkeypatch, ops)
    out = _inpaint(nine, fused=True, sampler_name="sample_euler")
    assert len(launches) == STEPS + 1
    sig = nine.pipe.get_sigmas(STEPS, OPT).half().float().cpu()
    m16 = F.interpolate(nine.mask, size=(16, 16))
    extra = torch.cat([torch.cat([m16] * 2), torch.cat([nine.mil.float()] * 2)], dim=1)
    ref = unet_ref.denoise_loop(nine.sd, nine.cfg, nine.lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(),
                                nine.text.float(), nine.rs, 7.5, sampler=sampling.sample_euler, extra_input=extra)
    sc = ref.abs().max().item()
    e = (out - ref).abs()
    print(f"9-channel fused Euler vs oracle: max {e.max().item():.3e} mean {e.mean().item():.3e} (range {sc:.2f})")
    assert e.max().item() < 4e-2 * sc and e.mean().item() < 6e-3 * sc, (e.max().item(), e.mean().item(), sc)


def test_fused_inpaiting_refuses_the_four_channel_unet(ops):
    from test_serving_gpu import _tiny_pipe
    cfg, pipe = _tiny_pipe(3)
    text = torch.randn(2, 77, cfg.cross_attention_dim, generator=_gen(1)).half()
    with pytest.raises(NotImplementedError, match="fused=False"):
        pipe.inpaiting(None, image=torch.zeros(1, 4, 16, 16).half(), mask_image=torch.ones(1, 1, 128, 128), height=128, width=128,
                       num_inference_steps=2, prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], output_type="latent",
                       sampler_name="sample_dpmpp_2m", fused=True)


# ----------------------------------------------------------------------------- c. the batcher
@pytest.fixture(scope="module")
def served(nine):
    return nine.pipe.serve(128, 128, max_batch=2, buckets=(1, 2), inpaint_unet=True).warm()


def _request(nn, **kw):
    r = dict(nn.base, image=nn.img_lat.clone(), mask_image=nn.mask, masked_image_latents=nn.mil.clone(), latents=nn.lat.clone(),
             num_inference_steps=STEPS)
    r.update(kw)
    return r


def test_served_request_equals_its_own_fused_inpaiting(ops, nine, served):
    """latents + mask + masked_image_latents: within 2e-3 of the range of its own inpaiting(fused=True) call
    (test_served_img2img_equals_its_own_pipeline_call's bound)"""
    fut = served.submit(_request(nine))
    served.run_until_idle()
    got = fut.result().float().cpu()
    ref = _inpaint(nine, fused=True, sampler_name="sample_dpmpp_2m")
    scale = ref.abs().max().item()
    d = (got - ref).abs().max().item()
    print(f"served 9-channel request vs inpaiting(fused=True): {d:.3e} (range {scale:.2f})")
    assert got.shape == (1, 4, 16, 16) and d < 2e-3 * scale, (d, scale)
    st = served.stats()
    assert st["captures_after_warm"] == 0 and st["cat_transitions"] >= STEPS + 1


def test_served_requests_joining_a_step_apart_equal_their_solo_runs(ops, nine, served):
    """A (mask 1, DPM++ 2M, 6 steps) and B (mask 2, Euler a with its own noise, guidance rescale, 4 steps) one step apart: each
    equals its solo served result bit for bit; no capture after warm()"""
    specs = [_request(nine),
             _request(nine, mask_image=nine.mask2, masked_image_latents=(nine.mil * 0.5).half(), num_inference_steps=4,
                      sampler_name="sample_euler_ancestral", eta=1.0, step_noise=nine.table[:4].contiguous(), guidance_rescale=0.5,
                      latents=torch.randn(1, 4, 16, 16, generator=_gen(77)).half())]
    fa = served.submit(dict(specs[0]))
    served.step()
    fb = served.submit(dict(specs[1]))
    served.run_until_idle()
    got = [fa.result(), fb.result()]
    assert served.stats()["captures_after_warm"] == 0
    for i, spec in enumerate(specs):
        f = served.submit(dict(spec))
        served.run_until_idle()
        solo = f.result()
        assert torch.isfinite(solo).all()
        assert torch.equal(got[i], solo), (i, (got[i].float() - solo.float()).abs().max().item())
    assert not torch.equal(got[0], got[1])
    assert served.stats()["captures_after_warm"] == 0


def test_served_pixels_through_the_vae(ops, nine, served):
    """`image` as pixels: the start latent and the masked-image latents come from the tiny VAE; finite, and the mask matters"""
    image = torch.rand(1, 3, 128, 128, generator=_gen(9)) * 2.0 - 1.0
    outs = []
    for mask in (nine.mask, torch.ones(1, 1, 128, 128)):
        fut = served.submit(dict(nine.base, image=image.clone(), mask_image=mask, num_inference_steps=4, generator=_gen(5)))
        served.run_until_idle()
        outs.append(fut.result().float().cpu())
    assert all(o.shape == (1, 4, 16, 16) and torch.isfinite(o).all() for o in outs)
    assert not torch.equal(outs[0], outs[1])
    assert served.stats()["captures_after_warm"] == 0
