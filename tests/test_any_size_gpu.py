"""Latents of any size on the MI355X (`-m gpu`): the skip-sized upsampling gather and the odd-sided stride-2 form of
dsc_conv3x3_nhwc_f16, dsc_conv3x3_fewcin_f16 at any width, and the UNet / ControlNet / pipeline / batcher at 152 x 152 and
176 x 152 pixels (19 x 19 and 19 x 22 latents: 19 -> 10 -> 5 -> 3 on the way down, 6 against 5 on the way up unless the
upsamplers are told the size of the skip tensor they meet).

Kernel tolerance: the existing convolution tests' |out - ref| <= 1.5e-3 |ref| + 2e-3 against an fp32 F.conv2d."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import any_size_ref as ar
from inputs import FakeTokenizer
from oracle import unet_ref

pytestmark = pytest.mark.gpu
CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


def _close(out, ref):
    return torch.all((out.float() - ref).abs() <= 1.5e-3 * ref.abs() + 2e-3)


def _conv_operands(B, C, Cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, h, w, generator=g).half().cuda().contiguous(memory_format=CL)
    wt = (torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(9 * C)).half().cuda().contiguous(memory_format=CL)
    b = (torch.randn(Cout, generator=g) * 0.2).half().cuda()
    return g, x, wt, b


SIZED = [(1, 64, 64, (3, 5), (5, 9)), (1, 64, 64, (3, 5), (6, 9)), (1, 64, 64, (3, 5), (5, 10)), (3, 128, 64, (4, 4), (7, 7)),
         (1, 64, 64, (9, 17), (17, 33)), (2, 640, 640, (10, 10), (19, 19)), (2, 1280, 1280, (5, 5), (10, 9))]


@pytest.mark.parametrize("B,C,Cout,src,dst", SIZED)
def test_conv3x3_sized_upsample(ops, B, C, Cout, src, dst):
    """the convolution reading x through F.interpolate(x, size=dst, mode="nearest") == the convolution of the materialised image,
    bit for bit (same sums in the same order); B >= 2: a wrong source extent shows as rows of the next image"""
    g, x, wt, b = _conv_operands(B, C, Cout, *src, seed=B + C + src[0] + dst[0] + dst[1])
    r = torch.randn(B, Cout, *dst, generator=g).half().cuda().contiguous(memory_format=CL)
    assert ops.conv3x3_supported(x, wt, upsample_size=dst)
    up = F.interpolate(x, size=dst, mode="nearest")
    ref = F.conv2d(up.float(), wt.float(), b.float(), padding=1)
    out = ops.conv3x3(x, wt, b, upsample_size=dst)
    assert out.shape == (B, Cout) + dst and out.is_contiguous(memory_format=CL)
    assert _close(out, ref), (out.float() - ref).abs().max().item()
    assert torch.equal(out, ops.conv3x3(up, wt, b))
    assert torch.equal(out, ops.conv3x3(x, wt, b, upsample_size=dst))                     # reproducible
    out_r = ops.conv3x3(x, wt, b, residual=r, upsample_size=dst)
    assert _close(out_r, ref + r.float()) and torch.equal(out_r, ops.conv3x3(up, wt, b, residual=r))
    out_n = ops.conv3x3(x, wt, None, upsample_size=dst)
    assert _close(out_n, ref - b.float().view(1, -1, 1, 1))
    if dst[0] % 2 == 0 and dst[1] % 2 == 0:
        assert torch.equal(out, ops.conv3x3(x, wt, b, upsample=True))


def test_conv3x3_sized_upsample_even_targets_are_the_2x_bytes(ops):
    """code 4 on even targets == code 1, split or not"""
    for B, C, Cout, h, w, splits in ((2, 1280, 1280, 5, 5, 0), (3, 128, 64, 4, 6, 2), (1, 64, 64, 9, 17, 1)):
        _, x, wt, b = _conv_operands(B, C, Cout, h, w, seed=C + h)
        assert torch.equal(ops.conv3x3(x, wt, b, upsample_size=(2 * h, 2 * w), splits=splits),
                           ops.conv3x3(x, wt, b, upsample=True, splits=splits))


def test_conv3x3_sized_upsample_reads_nothing_beyond_its_source(ops):
    """x is a view into a larger buffer whose remainder is NaN: with the source extent of the 2x form ((H/2) x (W/2) pixels) the
    last source row / column would be cut off, with a larger one the NaNs behind the image would be read as padding"""
    B, C, Cout, (h, w), dst = 2, 64, 64, (4, 4), (7, 7)
    _, x, wt, b = _conv_operands(B, C, Cout, h, w, seed=11)
    want = ops.conv3x3(x, wt, b, upsample_size=dst)
    n = B * h * w * C
    buf = torch.full((n + 4096,), float("nan"), dtype=torch.float16, device="cuda")
    buf[:n] = x.permute(0, 2, 3, 1).reshape(-1)
    view = buf[:n].view(B, h, w, C).permute(0, 3, 1, 2)
    assert view.is_contiguous(memory_format=CL) and view.data_ptr() == buf.data_ptr()
    got = ops.conv3x3(view, wt, b, upsample_size=dst)
    assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.parametrize("B,C,Cout,H,W,splits", [(1, 64, 64, 5, 9, 1), (1, 64, 64, 6, 9, 0), (3, 128, 64, 7, 7, 2),
                                                 (2, 320, 320, 19, 22, 0), (2, 1280, 1280, 19, 19, 0)])
def test_conv3x3_stride2_odd_sides(ops, B, C, Cout, H, W, splits):
    """Downsample2D on odd sides: out is [B, Cout, ceil(H/2), ceil(W/2)], the even pixels of the stride-1 result"""
    g, x, wt, b = _conv_operands(B, C, Cout, H, W, seed=B + C + H + W)
    ref = F.conv2d(x.float(), wt.float(), b.float(), stride=2, padding=1)
    assert ref.shape == (B, Cout, (H + 1) // 2, (W + 1) // 2)
    out = ops.conv3x3(x, wt, b, stride2_ceil=True, splits=splits)
    assert out.shape == ref.shape and out.is_contiguous(memory_format=CL)
    assert _close(out, ref), (out.float() - ref).abs().max().item()
    assert torch.equal(out, ops.conv3x3(x, wt, b, splits=splits)[:, :, ::2, ::2])
    assert torch.equal(out, ops.conv3x3(x, wt, b, stride2_ceil=True, splits=splits))
    r = torch.randn(ref.shape, generator=g).half().cuda().contiguous(memory_format=CL)
    out_r = ops.conv3x3(x, wt, b, residual=r, stride2_ceil=True, splits=splits)
    assert _close(out_r, ref + r.float())
    if H % 2 == 0 and W % 2 == 0:
        assert torch.equal(out, ops.conv3x3(x, wt, b, stride2=True, splits=splits))


def test_groupnorm_statistics_rows_for_the_new_codes(ops):
    """the statistics-emitting form covers the sized upsampling and keeps refusing both stride-2 codes (and an unknown code)"""
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    assert lib.dsc_conv3x3_gn_rows(2, 75, 76, 320, 320, 32, 2) == 0 and lib.dsc_conv3x3_gn_rows(2, 76, 76, 320, 320, 32, 3) == 0
    assert lib.dsc_conv3x3_gn_rows(2, 75, 76, 320, 320, 32, 5) == 0
    assert lib.dsc_conv3x3_gn_rows(2, 75, 76, 320, 320, 32, 4) == 10 * 5


@pytest.mark.parametrize("B,cin,cout,groups,src,dst", [(2, 320, 320, 32, (38, 38), (75, 76)), (3, 64, 128, 8, (8, 8), (15, 16)),
                                                       (2, 320, 640, 32, (16, 16), (31, 32))])
def test_groupnorm_statistics_from_the_sized_upsample_epilogue(ops, B, cin, cout, groups, src, dst):
    """test_groupnorm_statistics_from_the_convolution_epilogue's checks for resample code 4 (the gather is the only thing that
    differs: the tile sums are of the stored H x W tensor): the per-image `add` row, bias, residual, the bytes of the plain entry,
    the one-launch GroupNorm from the emitted partials against the two-launch one and fp32, and a second run bit-equal in the
    tensor, the partials and the GroupNorm.  Odd H with several tile rows per image, B = 3, groups that straddle the 64-channel
    tiles (cpg 20)"""
    g, x, wt, bias = _conv_operands(B, cin, cout, *src, seed=cin + cout + dst[0])
    add = (torch.randn(B, cout, generator=g) * 0.5).half().cuda()
    res = torch.randn(B, cout, *dst, generator=g).half().cuda().contiguous(memory_format=CL)
    gamma = (1 + 0.1 * torch.randn(cout, generator=g)).half().cuda()
    beta = (0.1 * torch.randn(cout, generator=g)).half().cuda()
    rows = ops.conv3x3_gn_rows(x, wt, groups, upsample_size=dst)
    assert rows == ((dst[0] + 7) // 8) * ((dst[1] + 15) // 16)
    up = F.interpolate(x, size=dst, mode="nearest")
    for kw in ({"add": add}, {"bias": bias, "residual": res}, {"bias": bias, "add": add, "residual": res}, {"bias": bias}, {}):
        out = ops.conv3x3_gn(x, wt, groups, upsample_size=dst, **kw)
        part = ops.gn_partials_of(out)
        assert part is not None and part.rows == rows and part.hw == dst[0] * dst[1]
        assert tuple(part.buf.shape) == (B, rows, groups, 2, 2)
        ref = F.conv2d(up.float(), wt.float(), kw["bias"].float() if "bias" in kw else None, padding=1)
        if "add" in kw:
            ref = ref + add.float()[:, :, None, None]
        if "residual" in kw:
            ref = ref + res.float()
        assert torch.all((out.float() - ref).abs() <= 2e-3 * ref.abs() + 4e-3)
        assert torch.equal(out, ops.conv3x3_gn(up, wt, groups, **kw))                          # the materialised image, same form
        if "add" not in kw:                                                                    # the bytes of the plain entry
            assert torch.equal(out, ops.conv3x3(x, wt, kw.get("bias"), kw.get("residual"), splits=1, upsample_size=dst))
        for act in (True, False):
            one = ops.groupnorm_apply_nhwc(out, part, groups, gamma, beta, 1e-5, act)
            two = ops.groupnorm_silu_nhwc(out, groups, gamma, beta, 1e-5, act)
            gref = F.group_norm(out.float(), groups, gamma.float(), beta.float(), 1e-5)
            gref = F.silu(gref) if act else gref
            assert (one.float() - gref).abs().max().item() < 6e-3 and (one.float() - two.float()).abs().max().item() < 4e-3
        again = ops.conv3x3_gn(x, wt, groups, upsample_size=dst, **kw)
        assert torch.equal(again, out) and torch.equal(ops.gn_partials_of(again).buf[..., 0, :], part.buf[..., 0, :])
        assert torch.equal(ops.groupnorm_apply_nhwc(again, ops.gn_partials_of(again), groups, gamma, beta, 1e-5, True),
                           ops.groupnorm_apply_nhwc(out, part, groups, gamma, beta, 1e-5, True))


FEWCIN = [(1, 4, 320, 19, 19), (2, 4, 320, 10, 76), (3, 8, 64, 5, 13), (1, 9, 320, 10, 7), (1, 4, 64, 3, 3)]


@pytest.mark.parametrize("B,Cin,Cout,H,W", FEWCIN)
def test_conv3x3_fewcin_any_width(ops, B, Cin, Cout, H, W):
    from diffusionspatialcontrol_amd import _lib
    g = torch.Generator().manual_seed(B + Cin + Cout + H + W)
    x = torch.randn(B, Cin, H, W, generator=g).half().cuda()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).half().cuda()
    b = (torch.randn(Cout, generator=g) * 0.2).half().cuda()
    wt = w.reshape(Cout, -1).t().contiguous()
    ref = F.conv2d(x.float(), w.float(), b.float(), padding=1)
    out = ops.conv3x3_fewcin(x, wt, b, Cout)
    assert out.shape == ref.shape and out.is_contiguous(memory_format=CL)
    assert _close(out, ref), (out.float() - ref).abs().max().item()
    xi = torch.zeros(B, Cin, H, W).half()
    xi[B - 1, Cin - 1, H - 1, 0] = 1.0
    xi[0, 0, 0, W - 1] = -2.0
    oi = ops.conv3x3_fewcin(xi.cuda(), wt, None, Cout).float().cpu()
    ri = F.conv2d(xi.float(), w.float().cpu(), None, padding=1)
    assert torch.all((oi - ri).abs() <= 1e-3 * ri.abs() + 1e-6)
    # through the C ABI into a sentinel-filled buffer: the overhanging lanes of a row's last block store nothing, neither into
    # the next row's first pixels (they hold that row's values) nor behind the last pixel
    n = B * H * W * Cout
    buf = torch.full((n + 8 * Cout,), 7.0, dtype=torch.float16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                                # noqa: E731
    rc = _lib.load_library().dsc_conv3x3_fewcin_f16(p(x), p(wt), p(b), p(buf), B, Cin, H, W, Cout, 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and (buf[n:] == 7.0).all()
    assert torch.equal(buf[:n].view(B, H, W, Cout).permute(0, 3, 1, 2), out)


# ----------------------------------------------------------------------------- the tiny UNet at 19 x 19 and 19 x 22 latents
def _setup(n_img=1):
    import test_unet_pipeline_gpu as up
    return up._tiny_setup(n_img)


def _region(W, H):
    import test_unet_pipeline_gpu as up
    return up._region_state(W=W, H=H)


@pytest.mark.parametrize("h,w", [(19, 19), (19, 22)])
def test_unet_forward_odd_latents_match_the_sized_oracle(ops, h, w):
    """test_unet_forward_matches_oracle's bounds against the sized restatement.  Without the skip sizes the up path meets 6 rows
    against 5 at its first concatenation and raises"""
    cfg, unet, sd, text = _setup()
    _, _, rs = _region(W=8 * w, H=8 * h)
    assert sorted(rs) == sorted({a * b for a, b in ar.skip_sizes(h, w, 3)[0]})
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, h, w, generator=g).half()
    t = torch.tensor([731.25, 731.25])
    sigma = torch.tensor([4.0], device="cuda")
    rp = {"region_state": rs, "sigma": sigma, "weight_func": lambda w_, s, qk: w_ * s * qk.std()}
    out = unet(x.cuda(), t.cuda(), text.cuda(), cross_attention_kwargs={"region_prompt": rp}).sample.float().cpu()
    assert out.shape == (2, 4, h, w)
    ref = ar.sized_unet_forward(sd, cfg, x.float(), t, text.float(), region_prompt={"region_state": rs, "sigma": 4.0, "weight_func": None})
    scale = ref.abs().max().item()
    err = (out - ref).abs()
    print(f"{h}x{w}: max err {err.max().item():.3e}, mean {err.mean().item():.3e}, range {scale:.3f}")
    assert err.max().item() < 1e-2 * scale + 1e-3, (err.max().item(), scale)
    assert err.mean().item() < 2e-3 * scale
    # the region bias is live: without it the GPU output is the oracle's output without it (same bounds), and the two GPU outputs
    # are at least half as far apart as the oracle says the bias moves the result (a dropped bias would make them equal)
    out0 = unet(x.cuda(), t.cuda(), text.cuda()).sample.float().cpu()
    ref0 = ar.sized_unet_forward(sd, cfg, x.float(), t, text.float())
    err0 = (out0 - ref0).abs()
    moved, moved_ref = (out0 - out).abs().max().item(), (ref0 - ref).abs().max().item()
    print(f"{h}x{w}: without the region prompt max err {err0.max().item():.3e}; the bias moves the output by {moved:.3e} "
          f"(oracle {moved_ref:.3e})")
    assert err0.max().item() < 1e-2 * ref0.abs().max().item() + 1e-3 and err0.mean().item() < 2e-3 * ref0.abs().max().item()
    assert moved_ref > 0 and moved > 0.5 * moved_ref


def test_controlnet_forward_odd_latents(ops):
    """the shared encoder half: odd-sided downsampling, no upsampler (the oracle serves these sizes as it is)"""
    import test_unet_pipeline_gpu as up
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNetConfig
    cfg = UNetConfig.tiny()
    cn, sd = up._controlnet(cfg)
    cn = cn.cuda().eval()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 4, 19, 19, generator=g).half()
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half()
    cond = torch.rand(2, 3, 152, 152, generator=g).half()
    t = torch.tensor([321.5, 321.5])
    with torch.no_grad():
        down, mid = cn(x.cuda(), t.cuda(), enc.cuda(), cond.cuda(), conditioning_scale=0.7, return_dict=False)
        rdown, rmid = unet_ref.controlnet_forward(sd, cfg, x.float(), t, enc.float(), cond.float(), 0.7)
    assert len(down) == 12 and tuple(mid.shape[2:]) == (3, 3)
    for a, b in zip(down + [mid], rdown + [rmid]):
        sc = max(b.abs().max().item(), 1e-3)
        assert a.shape == b.shape and (a.float().cpu() - b).abs().max().item() < 2e-2 * sc, (a.shape, sc)


@pytest.fixture(scope="module")
def tiny():
    import types
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    cfg, unet, sd, text = _setup(1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    return types.SimpleNamespace(cfg=cfg, pipe=pipe, sd=sd, text=text)


def test_denoise_loop_152_fused_protocol_oracle(ops, tiny):
    """test_denoise_loop_fused_protocol_oracle's assertions at 152 x 152 (19 x 19 latents: 1444 halfs per image, the sampler
    step's 8-byte form) against the sized oracle loop"""
    pipe, text = tiny.pipe, tiny.text
    state, ids, rs = _region(W=152, H=152)
    lat = torch.randn(1, 4, 19, 19, generator=torch.Generator().manual_seed(1000)).half()
    pe, ne = text[1:2], text[:1]
    kw = dict(height=152, width=152, num_inference_steps=6, guidance_scale=7.5, latents=lat.clone(), output_type="latent",
              region_map_state=state, sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"},
              prompt_embeds=pe, negative_prompt_embeds=ne, text_input_ids=ids, num_images_per_prompt=1)
    fused = pipe.txt2img(None, fused=True, **kw)[0].float().cpu()
    proto = pipe.txt2img(None, fused=False, **kw)[0].float().cpu()
    sig = pipe.get_sigmas(6, {"scheduler": "karras"}).half().float().tolist()
    ref = ar.sized_denoise_loop(tiny.sd, tiny.cfg, lat.float() * math.sqrt(sig[0] ** 2 + 1), sig, torch.cat([ne, pe]).float(),
                                dict(rs), 7.5)
    scale = ref.abs().max().item()
    print(f"152x152: fused vs protocol {(fused - proto).abs().max().item():.3e}, fused vs oracle max "
          f"{(fused - ref).abs().max().item():.3e} mean {(fused - ref).abs().mean().item():.3e}, range {scale:.3f}")
    assert fused.shape == (1, 4, 19, 19) and torch.isfinite(fused).all()
    assert (fused - proto).abs().max().item() < 2e-2 * scale
    assert (fused - ref).abs().max().item() < 4e-2 * scale, ((fused - ref).abs().max().item(), scale)
    assert (fused - ref).abs().mean().item() < 6e-3 * scale
    again = pipe.txt2img(None, fused=True, **kw)[0].float().cpu()
    assert (fused - again).abs().max().item() < 2e-2 * scale


def test_fused_refuses_the_linear_step_at_odd_by_odd_latents(ops, tiny):
    """19 x 19 latents hold 1444 = 4 * 361 halfs; dsc_cfg_linear_step_rows and its rescale form move 8 per lane.  fused=True says
    so before the loop, in the error class of the path's other limits; protocol mode runs the same request"""
    pipe, text = tiny.pipe, tiny.text
    lat = torch.randn(1, 4, 19, 19, generator=torch.Generator().manual_seed(3)).half()
    kw = dict(height=152, width=152, num_inference_steps=3, guidance_scale=7.5, output_type="latent",
              sampler_opt={"scheduler": "karras"}, prompt_embeds=text[1:2], negative_prompt_embeds=text[:1],
              num_images_per_prompt=1)
    for extra in ({"sampler_name": "sample_euler"}, {"sampler_name": "sample_dpmpp_2m", "guidance_rescale": 0.7}):
        with pytest.raises(NotImplementedError, match="multiple of 8 halfs"):
            pipe.txt2img(None, fused=True, latents=lat.clone(), **kw, **extra)
    out = pipe.txt2img(None, fused=False, latents=lat.clone(), sampler_name="sample_euler", **kw)[0]
    assert out.shape == (1, 4, 19, 19) and torch.isfinite(out).all()
    # one even side: 19 x 22 = 8 * 209 halfs, the fused linear step runs
    lat2 = torch.randn(1, 4, 19, 22, generator=torch.Generator().manual_seed(4)).half()
    kw2 = dict(kw, width=176)
    f = pipe.txt2img(None, fused=True, latents=lat2.clone(), sampler_name="sample_euler", **kw2)[0].float().cpu()
    p = pipe.txt2img(None, fused=False, latents=lat2.clone(), sampler_name="sample_euler", **kw2)[0].float().cpu()
    assert f.shape == (1, 4, 19, 22) and (f - p).abs().max().item() < 2e-2 * p.abs().max().item()


STEPS, OPT, X, STRENGTH = 8, {"scheduler": "karras"}, 1.2, 0.6
LAT2 = (1, 4, 19, 19)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _hires_kwargs(tiny):
    state, ids, _ = _region(W=128, H=128)
    text = tiny.text
    common = dict(guidance_scale=7.5, output_type="latent", region_map_state=state, sampler_opt=OPT, prompt_embeds=text[1:2],
                  negative_prompt_embeds=text[:1], text_input_ids=ids, num_inference_steps=STEPS)
    base = {"prompt_embeds": text[1:2].cuda(), "negative_prompt_embeds": text[:1].cuda(), "text_input_ids": ids,
            "region_map_state": state, "guidance_scale": 7.5, "sampler_opt": OPT, "num_inference_steps": STEPS}
    hires = dict(upscale=True, upscale_x=X, upscale_method="bicubic", upscale_denoising_strength=STRENGTH)
    return common, base, hires


def test_txt2img_default_hires_factor(ops, tiny):
    """the app's default factor: 128 x 128 -> 152 x 152.  txt2img(upscale=True) is its first pass + F.interpolate + img2img; done
    by hand with the same seeded generator the three calls are the same launches on the same inputs"""
    pipe = tiny.pipe
    common, _, hires = _hires_kwargs(tiny)
    out = pipe.txt2img(None, fused=True, generator=_gen(77), sampler_name="sample_dpmpp_2m", width=128, height=128,
                       **hires, **common)[0]
    assert out.shape == LAT2 and torch.isfinite(out).all()
    g = _gen(77)
    first = pipe.txt2img(None, fused=True, generator=g, sampler_name="sample_dpmpp_2m", width=128, height=128, **common)[0]
    big = F.interpolate(first.float(), size=LAT2[2:], mode="bicubic").to(first.dtype)
    route = pipe.img2img(latents=big, width=152, height=152, generator=g, strength=STRENGTH, sampler_name="sample_dpmpp_2m",
                         fused=None, **common)[0]
    scale = route.float().abs().max().item()
    d = (out.float() - route.float()).abs().max().item()
    print(f"txt2img(upscale_x=1.2) vs first pass + interpolate + img2img by hand: {d:.3e} (range {scale:.2f})")
    assert d <= 2e-3 * scale, (d, scale)


def test_serving_152_joins_equal_solo_runs(ops, tiny):
    """ServingBatcher(pipe, 152, 152): B joins two steps after A; each equals its solo served run bit for bit"""
    from diffusionspatialcontrol_amd.modules.serving import ServingBatcher
    state, ids, _ = _region(W=152, H=152)
    text = tiny.text
    b = ServingBatcher(tiny.pipe, 152, 152, max_batch=2, buckets=(1, 2), slot=2).warm()
    req = lambda i, steps: {"prompt_embeds": text[1:2].cuda(), "negative_prompt_embeds": text[:1].cuda(), "text_input_ids": ids,  # noqa: E731
                            "region_map_state": state, "guidance_scale": 7.5, "sampler_opt": OPT, "num_inference_steps": steps,
                            "latents": torch.randn(LAT2, generator=_gen(90 + i)).half().cuda()}
    fa = b.submit(req(0, 6))
    b.step()
    b.step()
    fb = b.submit(req(1, 5))
    b.run_until_idle()
    got = [fa.result(), fb.result()]
    assert b.stats()["captures_after_warm"] == 0 and b.stats()["joins"] == 2
    for i, steps in ((0, 6), (1, 5)):
        f = b.submit(req(i, steps))
        b.run_until_idle()
        solo = f.result()
        assert solo.shape == LAT2 and torch.isfinite(solo).all()
        assert torch.equal(got[i], solo), (i, (got[i].float() - solo.float()).abs().max().item())
    assert not torch.equal(got[0], got[1])


def test_hand_built_pair_serves_the_default_factor(ops, tiny):
    """HiresPair(ServingBatcher 128, ServingBatcher 152) serving upscale_x = 1.2 == the chain driven by hand (the pattern of
    tests/test_hires_gpu.py::test_chain_equals_its_parts); pipe.serve_hires still refuses the factor (its guard is pinned by an
    older test and is the remaining item)"""
    from diffusionspatialcontrol_amd.modules.serving import HiresPair, ServingBatcher
    pipe = tiny.pipe
    _, base, hires = _hires_kwargs(tiny)
    with pytest.raises(ValueError):
        pipe.serve_hires(128, 128, 1.2)
    kw = dict(max_batch=2, buckets=(1, 2))
    pair = HiresPair(ServingBatcher(pipe, 128, 128, slot=0, **kw), ServingBatcher(pipe, 152, 152, slot=1, **kw)).warm()
    assert (pair.hires.height, pair.hires.width) == (152, 152)
    sig2 = pipe._schedule(STEPS, OPT, "cpu", torch.float16).float().tolist()[STEPS - int(STEPS * STRENGTH)]
    run = lambda p, fut: (p.run_until_idle(), fut.result())[1]                                  # noqa: E731
    lat = torch.randn(1, 4, 16, 16, generator=_gen(50)).half().cuda()
    noise = torch.randn(LAT2, generator=_gen(51)).half().cuda()
    first = run(pair, pair.submit(dict(base, latents=lat)))
    assert torch.equal(first, run(pair, pair.submit(dict(base, latents=lat))))
    chained = run(pair, pair.submit(dict(base, latents=lat, hires_latents=noise, **hires)))
    assert chained.shape == LAT2 and torch.isfinite(chained).all()
    start = ops.latent_resample_noise(first, LAT2[2:], "bicubic", noise=noise, sigma0=sig2)
    torch.cuda.synchronize()
    by_hand = run(pair, pair.hires.submit(dict(base, image=start, latents=torch.zeros_like(noise), strength=STRENGTH)))
    assert torch.equal(chained, by_hand), (chained.float() - by_hand.float()).abs().max().item()
    st = pair.stats()
    assert st["handoffs"] >= 1 and st["base"]["captures_after_warm"] == 0 and st["hires"]["captures_after_warm"] == 0
