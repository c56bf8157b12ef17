"""IP-Adapter region masks in the continuous batcher on the MI355X (`-m gpu`): dsc_ip_xattn_add_masked_f16 (one weight per query
folded into the image-token attention's coefficient; zero-weight queries not stored, all-zero tiles not read) against an fp32
restatement and against the unmasked entry, and a batcher built with `ip_masks=True` against
`txt2img(cross_attention_kwargs={"ip_adapter_masks": ...})`, against a default batcher and against itself.  Helpers follow
tests/test_ip_serving_gpu.py."""
import gc

import pytest
import torch
import torch.nn.functional as F

from inputs import FakeTokenizer

pytestmark = pytest.mark.gpu
ATOL32 = 6e-3        # tests/test_ip_serving_gpu.py / tests/test_region_xattn_gpu.py: the project's attention-output tolerance
ROW_SCALE = [0.7, 0.0, -0.4]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- the kernel
def _inputs(B, L, H, d, T, seed):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, L, H, d, generator=g) * 0.5).half()
    k = (torch.randn(B, T, H, d, generator=g) * 0.5).half()
    v = torch.randn(B, T, H, d, generator=g).half()
    io = torch.randn(B, L, H * d, generator=g).half()
    return q, k, v, io


def _weights(B, L, seed):
    """uniform in [-0.2, 1.2] (bicubic down-sampling overshoots), rounded to fp16, about a quarter exact zeros"""
    g = torch.Generator().manual_seed(1000 + seed)
    w = (torch.rand(B, L, generator=g) * 1.4 - 0.2).half()
    w[torch.rand(B, L, generator=g) < 0.25] = 0.0
    return w


def _restated(q, k, v, io, row_scale, w):
    """io + rs * w * softmax(s q k^T) v in fp32 on the CPU, before the final rounding"""
    B, L, H, d = q.shape
    scores = torch.einsum("blhd,bthd->bhlt", q.float(), k.float()) * d ** -0.5
    p = torch.softmax(scores - scores.amax(-1, keepdim=True), dim=-1)
    o = torch.einsum("bhlt,bthd->blhd", p, v.float()).reshape(B, L, H * d)
    return io.float() + torch.tensor(row_scale).view(B, 1, 1) * w.float().view(B, L, 1) * o


def _bound(ref_b, rs, w_b):
    """|rs| * max|w| * 6e-3 + half an fp16 ulp of the largest |result| (the one final rounding)"""
    top = ref_b.abs().max().item()
    half_ulp = 2.0 ** (torch.tensor(top).log2().floor().item() - 10) / 2
    return abs(rs) * w_b.float().abs().max().item() * ATOL32 + half_ulp


def _run(ops, q, k, v, io, rs, w=None):
    got = ops.ip_xattn_add(q.cuda(), k.cuda(), v.cuda(), torch.tensor(rs, device="cuda"), io.cuda().clone(),
                           q_weight=None if w is None else w.cuda())
    torch.cuda.synchronize()
    return got.cpu()


CASES = [(16, 1, 8, 1), (40, 2, 40, 4), (72, 2, 64, 16), (48, 1, 160, 4)]


@pytest.mark.parametrize("L, H, d, T", CASES)
def test_masked_entry_against_fp32_restatement(ops, L, H, d, T):
    B = len(ROW_SCALE)
    q, k, v, io = _inputs(B, L, H, d, T, seed=L + d + T)
    w = _weights(B, L, seed=L)
    assert (w == 0).any() and (w != 0).any()
    ref = _restated(q, k, v, io, ROW_SCALE, w)
    got = _run(ops, q, k, v, io, ROW_SCALE, w)
    assert got.shape == io.shape
    for b, rs in enumerate(ROW_SCALE):
        err = (got[b].float() - ref[b]).abs().max().item()
        print(f"L={L} H={H} d={d} T={T} row {b} scale {rs}: max error {err:.3e} (bound {_bound(ref[b], rs, w[b]):.3e})")
        assert err <= _bound(ref[b], rs, w[b]), (b, err)
    assert torch.equal(got[1], io[1])                                         # scale 0: untouched
    zero = (w[0] == 0)
    assert torch.equal(got[0][zero], io[0][zero])                             # weight 0: not stored
    assert (got[0][~zero].float() - io[0][~zero].float()).abs().max().item() > 0.01


@pytest.mark.parametrize("B, L, H, d, T", [(3,) + c for c in CASES] + [(2, 4096, 2, 40, 4)])
def test_all_ones_weights_give_the_unmasked_entrys_bits(ops, B, L, H, d, T):
    """(rs * 1.0) / sum is rs / sum: a row of ones reproduces dsc_ip_xattn_add_f16, the four-tiles-per-wave launch (L = 4096:
    256 query tiles) included"""
    q, k, v, io = _inputs(B, L, H, d, T, seed=7 + L)
    rs = ROW_SCALE if B == 3 else [0.7, -0.4]
    plain = _run(ops, q, k, v, io, rs)
    ones = _run(ops, q, k, v, io, rs, torch.ones(B, L, dtype=torch.float16))
    assert not torch.equal(plain, io)
    assert torch.equal(ones, plain), (ones.float() - plain.float()).abs().max().item()


def test_zero_weights_leave_io_alone_whatever_q_holds(ops):
    """one whole 16-query tile of zeros (no load, no store) and single zeros in mixed tiles (store predicated), the ragged last
    tile among them; q is NaN exactly at those queries: a NaN would reach io through any load that is consumed"""
    B, L, H, d, T = 3, 72, 2, 64, 16
    rs = [0.7, 1.0, -0.4]
    q, k, v, _ = _inputs(B, L, H, d, T, seed=11)
    io = (torch.arange(B * L * H * d) % 251).view(B, L, H * d).half() / 16 - 4          # a pattern, not noise
    w = (torch.rand(B, L, generator=torch.Generator().manual_seed(12)) * 1.4 - 0.2).half()
    w[w == 0] = 0.5
    zero = torch.zeros(L, dtype=torch.bool)
    zero[16:32] = True
    zero[[3, 40, 47, 70]] = True
    w[:, zero] = 0.0
    ref = _restated(q, k, v, io, rs, w)
    q_nan = q.clone()
    q_nan[:, zero] = float("nan")
    got = _run(ops, q_nan, k, v, io, rs, w)
    assert torch.equal(got[:, zero], io[:, zero])
    assert torch.isfinite(got).all()
    for b in range(B):
        err = (got[b][~zero].float() - ref[b][~zero]).abs().max().item()
        assert err <= _bound(ref[b], rs[b], w[b]), (b, err)
    assert (got[:, ~zero].float() - io[:, ~zero].float()).abs().max().item() > 0.05


def test_weight_batch_stride_and_determinism(ops):
    B, L, H, d, T = 3, 72, 2, 64, 16
    q, k, v, io = (t.cuda() for t in _inputs(B, L, H, d, T, seed=13))
    w = _weights(B, L, seed=13).cuda()
    rs = torch.tensor(ROW_SCALE, device="cuda")
    wide = torch.full((B, L + 37), float("nan"), dtype=torch.float16, device="cuda")
    view = wide[:, 5:5 + L]                                                   # batch stride L + 37, 2-byte aligned only
    view.copy_(w)
    assert view.stride() == (L + 37, 1) and view.data_ptr() % 4 == 2
    a = ops.ip_xattn_add(q, k, v, rs, io.clone(), q_weight=w)
    b = ops.ip_xattn_add(q, k, v, rs, io.clone(), q_weight=view)
    c = ops.ip_xattn_add(q, k, v, rs, io.clone(), q_weight=w)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and not torch.equal(a, io)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_masked_entry_under_graph_capture(ops):
    """one captured call; the weight buffer is rewritten in place and io reset before each replay: the replay reads the weights
    of that moment, and the scale-0 row is still skipped"""
    B, L, H, d, T = 3, 72, 2, 64, 16
    q, k, v, io = (t.cuda() for t in _inputs(B, L, H, d, T, seed=17))
    w1, w2 = _weights(B, L, seed=17).cuda(), _weights(B, L, seed=18).cuda()
    rs = torch.tensor(ROW_SCALE, device="cuda")
    buf, wbuf = io.clone(), torch.ones(B, L, dtype=torch.float16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ip_xattn_add(q, k, v, rs, buf, q_weight=wbuf)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    buf.copy_(io)
    gc.collect()                                       # no collection of earlier tests' dead graphs inside the capture
    with torch.cuda.graph(g):
        ops.ip_xattn_add(q, k, v, rs, buf, q_weight=wbuf)
    outs = []
    for w in (w1, w2):
        wbuf.copy_(w)
        buf.copy_(io)
        g.replay()
        outs.append(buf.clone())
        fresh = ops.ip_xattn_add(q, k, v, rs, io.clone(), q_weight=w)
        torch.cuda.synchronize()
        assert torch.equal(outs[-1], fresh)
        assert torch.equal(outs[-1][1], io[1])
    assert not torch.equal(outs[0], outs[1])


def test_wrapper_refuses_a_bad_weight(ops):
    B, L = 2, 16
    q, k, v, io = (t.cuda() for t in _inputs(B, L, 2, 40, 4, seed=19))
    rs = torch.ones(B, device="cuda")
    ones = torch.ones(B, L, dtype=torch.float16, device="cuda")
    ops.ip_xattn_add(q, k, v, rs, io, q_weight=ones)
    for bad in (ones.float(),                                                  # dtype
                torch.ones(B, L + 1, dtype=torch.float16, device="cuda"),      # shape
                ones[0],
                torch.ones(B, 2 * L, dtype=torch.float16, device="cuda")[:, ::2],   # inner stride
                ones.cpu()):                                                   # device
        before = io.clone()
        with pytest.raises(ValueError, match="q_weight|one device"):
            ops.ip_xattn_add(q, k, v, rs, io, q_weight=bad)
        torch.cuda.synchronize()
        assert torch.equal(io, before)


# ----------------------------------------------------------------------------- the batcher
EMB = 48
KARRAS = {"scheduler": "karras"}
KW = dict(num_inference_steps=4, guidance_scale=7.5, sampler_opt=KARRAS)


def _tiny_pipe(seed):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(seed)
    cfg = UNetConfig.tiny()
    unet = UNet2DConditionModel(cfg).half().cuda().eval()
    return cfg, StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())


def _cross_layers(unet):
    from diffusionspatialcontrol_amd.modules import u_net_condition_modify as um
    return [(n, m) for pre in ("down_blocks", "up_blocks", "mid_block") for n, m in unet.named_modules()
            if isinstance(m, um.Attention) and m.is_cross_attention and n.startswith(pre)]


def _adapter_weights(unet, ctx, g, offset=True):
    sd = {}
    for i, (n, m) in enumerate(_cross_layers(unet)):
        sd[f"{2 * i + 1}.to_k_ip.weight"] = torch.randn(m.inner_dim, ctx, generator=g) * 0.2 + (i if offset else 0)
        sd[f"{2 * i + 1}.to_v_ip.weight"] = torch.randn(m.inner_dim, ctx, generator=g) * 0.2
    return sd


def _standard_adapter(unet, ctx, g):
    return {"image_proj": {"proj.weight": torch.randn(4 * ctx, EMB, generator=g) * 0.1, "proj.bias": torch.zeros(4 * ctx),
                           "norm.weight": torch.ones(ctx), "norm.bias": torch.zeros(ctx)},
            "ip_adapter": _adapter_weights(unet, ctx, g)}


def _plus_adapter(unet, ctx, g):
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import IPAdapterPlusImageProjection
    torch.manual_seed(11)
    src = IPAdapterPlusImageProjection(embed_dims=24, output_dims=ctx, hidden_dims=128, depth=1, dim_head=64, heads=2, num_queries=16,
                                       ffn_ratio=2)
    proj = {"latents": src.latents.data, "proj_in.weight": src.proj_in.weight.data, "proj_in.bias": src.proj_in.bias.data,
            "proj_out.weight": src.proj_out.weight.data, "proj_out.bias": src.proj_out.bias.data,
            "norm_out.weight": src.norm_out.weight.data, "norm_out.bias": src.norm_out.bias.data}
    for i, (ln0, ln1, attn, ff) in enumerate(src.layers):
        proj.update({f"layers.{i}.0.norm1.weight": ln0.weight.data, f"layers.{i}.0.norm1.bias": ln0.bias.data,
                     f"layers.{i}.0.norm2.weight": ln1.weight.data, f"layers.{i}.0.norm2.bias": ln1.bias.data,
                     f"layers.{i}.0.to_q.weight": attn.to_q.weight.data,
                     f"layers.{i}.0.to_kv.weight": torch.cat([attn.to_k.weight.data, attn.to_v.weight.data]),
                     f"layers.{i}.0.to_out.weight": attn.to_out[0].weight.data,
                     f"layers.{i}.1.0.weight": ff[0].weight.data, f"layers.{i}.1.0.bias": ff[0].bias.data,
                     f"layers.{i}.1.1.weight": ff[1].net[0]["proj"].weight.data, f"layers.{i}.1.3.weight": ff[1].net[2].weight.data})
    return {"image_proj": proj, "ip_adapter": _adapter_weights(unet, ctx, g, offset=False)}


def _request(ctx, i, h=16, w=16):
    emb = torch.randn(2, 77, ctx, generator=torch.Generator().manual_seed(300 + i)).half()
    return {"prompt_embeds": emb[1:2].cuda(), "negative_prompt_embeds": emb[0:1].cuda(),
            "latents": torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(400 + i)).half().cuda()}


def _image_embeds(i):
    e = torch.randn(2, 1, EMB, generator=torch.Generator().manual_seed(500 + i)).half()
    e[0] = 0
    return e.cuda()


def _region(n, h, w, boxes):
    """[n, 1, h, w] fp32 on the GPU, ones inside adapter a's box (y0, y1, x0, x1): what the app hands over per region map"""
    m = torch.zeros(n, 1, h, w)
    for a, (y0, y1, x0, x1) in enumerate(boxes):
        m[a, :, y0:y1, x0:x1] = 1.0
    return m.cuda()


def _masks(m):
    return {"cross_attention_kwargs": {"ip_adapter_masks": m}}


def _serve_one(b, req, **kw):
    fut = b.submit(dict(req, **kw))
    b.run_until_idle()
    return fut.result().float().cpu()


def _txt2img(pipe, req, steps, fused, size=(128, 128), **kw):
    return pipe.txt2img(None, height=size[0], width=size[1], num_inference_steps=steps, guidance_scale=7.5,
                        sampler_name="sample_dpmpp_2m", sampler_opt=KARRAS, latents=req["latents"].clone(),
                        prompt_embeds=req["prompt_embeds"], negative_prompt_embeds=req["negative_prompt_embeds"],
                        output_type="latent", fused=fused, **kw)[0].float().cpu()


def _against_txt2img(pipe, b, req, embeds, masks, what, size=(128, 128)):
    """tests/test_ip_serving_gpu.py's criterion: d_served = served vs txt2img(fused=True); d_routes = txt2img(fused=True) vs
    txt2img(fused=False); d_served <= 2 d_routes and d_served < 3e-2 range.  One mask per pipeline: the fused loop's captured
    step keeps the mask tensor it was captured with"""
    got = _serve_one(b, req, ip_adapter_image_embeds=embeds, **_masks(masks), **KW)
    ref = dict(ip_adapter_image_embeds=embeds, size=size, **_masks(masks))
    fused = _txt2img(pipe, req, 4, True, **ref)
    proto = _txt2img(pipe, req, 4, False, **ref)
    rng = max(1.0, fused.abs().max().item())
    d_served = (got - fused).abs().max().item()
    d_routes = (fused - proto).abs().max().item()
    print(f"{what}: d_served {d_served:.3e}  d_routes {d_routes:.3e}  range {rng:.2f}")
    assert torch.isfinite(got).all()
    assert d_served < 3e-2 * rng, (d_served, rng)
    assert d_served <= 2 * d_routes, (d_served, d_routes)
    return got


@pytest.fixture(scope="module")
def served():
    """one tiny pipeline with the 4-token adapter, a default batcher and a mask-capable one on two workspace slots (one bucket
    of two slots each: slot 1 is an idle row in every solo run)"""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    cfg, pipe = _tiny_pipe(3)
    ctx = cfg.cross_attention_dim
    pipe.load_ip_adapter(_standard_adapter(pipe.unet, ctx, torch.Generator().manual_seed(3)))
    pipe.set_ip_adapter_scale(0.7)
    default = pipe.serve(128, 128, max_batch=2, buckets=(2,), slot=0).warm()
    b = pipe.serve(128, 128, max_batch=2, buckets=(2,), slot=1, ip_masks=True).warm()
    return {"pipe": pipe, "ctx": ctx, "b": b, "default": default, "req": _request(ctx, 0)}


def test_unmasked_requests_equal_a_default_batcher(served):
    """the mask-capable step launches the masked entry with weights of ones: the bits of the unmasked entry"""
    b, default, req = served["b"], served["default"], served["req"]
    for kw in ({}, {"ip_adapter_image_embeds": [_image_embeds(0)]}):
        got, want = _serve_one(b, req, **kw, **KW), _serve_one(default, req, **kw, **KW)
        assert torch.equal(got, want), (sorted(kw), (got - want).abs().max().item())
    served["plain"], served["unmasked"] = _serve_one(b, req, **KW), got
    assert (served["unmasked"] - served["plain"]).abs().max().item() > 1e-3
    with pytest.raises(ValueError, match="ip_masks=True"):
        default.submit(dict(req, ip_adapter_image_embeds=[_image_embeds(0)], **_masks(_region(1, 128, 128, [(0, 64, 0, 128)])), **KW))


def test_ones_mask_is_no_mask_and_zeros_mask_is_no_image_prompt(served):
    b, req = served["b"], served["req"]
    e = [_image_embeds(0)]
    plain, unmasked = _serve_one(b, req, **KW), _serve_one(b, req, ip_adapter_image_embeds=e, **KW)
    ones = _serve_one(b, req, ip_adapter_image_embeds=e, **_masks(torch.ones(1, 1, 128, 128).cuda()), **KW)
    zeros = _serve_one(b, req, ip_adapter_image_embeds=e, **_masks(torch.zeros(1, 1, 128, 128).cuda()), **KW)
    assert torch.equal(ones, unmasked), (ones - unmasked).abs().max().item()
    assert torch.equal(zeros, plain), (zeros - plain).abs().max().item()
    assert not torch.equal(plain, unmasked)
    assert b.stats()["captures_after_warm"] == 0


def test_top_half_mask_against_txt2img(served):
    """one adapter, rows 0-63 of a 128 x 128 mask are ones: the lower half of the 16 x 16 level is all-zero tiles.
    Measured on one MI355X (one run): d_served 2.188e-01, d_routes 5.625e-01, range 59.53; 45.3 from the unmasked served run
    and 34.0 from the run without an image prompt."""
    pipe, b, req = served["pipe"], served["b"], served["req"]
    e = [_image_embeds(0)]
    m = _region(1, 128, 128, [(0, 64, 0, 128)])
    got = _against_txt2img(pipe, b, req, e, m, "top-half mask")
    unmasked, plain = _serve_one(b, req, ip_adapter_image_embeds=e, **KW), _serve_one(b, req, **KW)
    d_un, d_plain = (got - unmasked).abs().max().item(), (got - plain).abs().max().item()
    print(f"top-half mask: vs unmasked served {d_un:.3e}, vs no image prompt {d_plain:.3e}")
    assert d_un > 1e-3 and d_plain > 1e-3
    assert b.stats()["captures_after_warm"] == 0


def test_mixed_membership_equals_each_request_alone(served):
    """A (top-half mask, scale 0.7, 4 steps) starts; B (no image prompt, 3 steps) joins after 2 steps; C (left-half mask, other
    embeds, scale 0.3) joins into the slot A frees: its weights replace A's in rows {0, 2}.  Each equals its own solo served run
    within 2e-3 of the range (tests/test_ip_serving_gpu.py's bound: both sides run the same kernels); no capture after warm()"""
    b, ctx = served["b"], served["ctx"]
    specs = {"A": dict(_request(ctx, 1), num_inference_steps=4, guidance_scale=7.5, sampler_opt=KARRAS,
                       ip_adapter_image_embeds=[_image_embeds(1)], ip_adapter_scale=0.7,
                       **_masks(_region(1, 128, 128, [(0, 64, 0, 128)]))),
             "B": dict(_request(ctx, 2), num_inference_steps=3, guidance_scale=7.5, sampler_opt={"scheduler": "exponential"}),
             "C": dict(_request(ctx, 3), num_inference_steps=4, guidance_scale=5.0, sampler_opt=KARRAS,
                       ip_adapter_image_embeds=[_image_embeds(3)], ip_adapter_scale=0.3,
                       **_masks(_region(1, 128, 128, [(0, 128, 0, 64)])))}
    joins0 = b.stats()["joins"]
    futs = {"A": b.submit(dict(specs["A"]))}
    for _ in range(3):
        b.step()
    futs["B"] = b.submit(dict(specs["B"]))
    for _ in range(3):
        b.step()
    assert b._slots[0] is None                          # A has left
    futs["C"] = b.submit(dict(specs["C"]))
    b.step()
    assert b._slots[0] is not None and b._slots[0].ip_scale == [0.3] and b._slots[0].ip_weights is not None
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["joins"] - joins0 == 3, st
    got = {n: f.result().float().cpu() for n, f in futs.items()}
    solo = {n: _serve_one(b, dict(s)) for n, s in specs.items()}
    rng = max(v.abs().max().item() for v in solo.values())
    for n in specs:
        d = (got[n] - solo[n]).abs().max().item()
        print(f"request {n}: vs its own solo served run {d:.3e} (range {rng:.2f})")
        assert d < 2e-3 * rng, (n, d, rng)
    for n in "AC":                                       # the masks did steer both
        dropped = _serve_one(b, {k: v for k, v in specs[n].items() if k != "cross_attention_kwargs"})
        assert (got[n] - dropped).abs().max().item() > 1e-3, n
    assert b.stats()["captures_after_warm"] == 0


def test_two_adapters_with_top_and_bottom_masks_against_txt2img():
    """a 4-token and a 16-token (Plus) adapter, scales 0.7 / 0.5, the first in the top half and the second in the bottom half.
    Measured on one MI355X (one run): d_served 2.188e-01, d_routes 6.250e-01, range 59.94."""
    cfg, pipe = _tiny_pipe(4)
    ctx = cfg.cross_attention_dim
    g = torch.Generator().manual_seed(5)
    pipe.load_ip_adapter([_standard_adapter(pipe.unet, ctx, g), _plus_adapter(pipe.unet, ctx, g)])
    pipe.set_ip_adapter_scale([0.7, 0.5])
    b = pipe.serve(128, 128, max_batch=2, buckets=(2,), ip_masks=True).warm()
    hidden = (torch.randn(2, 1, 9, 24, generator=torch.Generator().manual_seed(6)) * 0.5).half().cuda()     # CLIP hidden states
    embeds = [_image_embeds(7), hidden]
    req = _request(ctx, 5)
    m = _region(2, 128, 128, [(0, 64, 0, 128), (64, 128, 0, 128)])
    got = _against_txt2img(pipe, b, req, embeds, m, "two adapters, top / bottom")
    unmasked = _serve_one(b, req, ip_adapter_image_embeds=embeds, **KW)
    swapped = _serve_one(b, req, ip_adapter_image_embeds=embeds, **_masks(m.flip(0)), **KW)
    assert (got - unmasked).abs().max().item() > 1e-3 and (got - swapped).abs().max().item() > 1e-3
    assert b.stats()["captures_after_warm"] == 0


def test_non_square_batcher_against_txt2img():
    """128 x 192 (16 x 24 latents: levels of 384, 96, 24 and 6 queries - ragged last tiles), the adapter in the left half.
    Measured on one MI355X (one run): d_served 2.227e-01, d_routes 1.125e+00, range 78.25."""
    cfg, pipe = _tiny_pipe(6)
    ctx = cfg.cross_attention_dim
    pipe.load_ip_adapter(_standard_adapter(pipe.unet, ctx, torch.Generator().manual_seed(7)))
    pipe.set_ip_adapter_scale(0.7)
    b = pipe.serve(128, 192, max_batch=2, buckets=(2,), ip_masks=True).warm()
    assert sorted(b.levels()) == [6, 24, 96, 384]
    req = _request(ctx, 6, 16, 24)
    e = [_image_embeds(8)]
    got = _against_txt2img(pipe, b, req, e, _region(1, 128, 192, [(0, 128, 0, 96)]), "128 x 192, left half", size=(128, 192))
    unmasked = _serve_one(b, req, ip_adapter_image_embeds=e, **KW)
    assert (got - unmasked).abs().max().item() > 1e-3
    assert b.stats()["captures_after_warm"] == 0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_hires_pair_with_masks_against_the_pipelines_own_call():
    """a chained pair 128 x 128 -> 160 x 160 (upscale_x 1.25; 20 x 20 latents: levels of 400, 100, 25 and 9 queries), a masked
    `upscale=True` request against pipe.txt2img(upscale=True) with the same masks and seeded generator, by the comparison of
    tests/test_hires_gpu.py::test_chain_against_the_pipelines_own_call: the chain may be at most twice as far from the pipeline's
    call as a route of served pieces (served txt2img, torch's interpolate, served img2img, each with the mask), or 2e-3 of the
    range.  The second pass uses weights at its own levels: dropping the mask from the second piece changes the result.
    pipe.serve_hires refuses this factor on the four-level tiny UNet (its latent-multiple guard), so the pair is chained by
    hand from two `ip_masks=True` batchers - what serve_hires(..., ip_masks=True) builds, checked at a factor it accepts.
    Measured on one MI355X (one run): chained 1.250e-01, served pieces 1.250e-01, range 59.31; 5.400e-01 from the run whose
    second piece drops the mask."""
    from diffusionspatialcontrol_amd.modules.serving import HiresPair
    STEPS, X, STRENGTH, LAT2 = 8, 1.25, 0.6, (1, 4, 20, 20)
    cfg, pipe = _tiny_pipe(8)
    ctx = cfg.cross_attention_dim
    pipe.load_ip_adapter(_standard_adapter(pipe.unet, ctx, torch.Generator().manual_seed(9)))
    pipe.set_ip_adapter_scale(0.7)
    built = pipe.serve_hires(128, 128, 1.5, max_batch=2, buckets=(2,), slots=(2, 3), ip_masks=True)
    assert built.base.ip_masks and built.hires.ip_masks and (built.hires.height, built.hires.width) == (192, 192)
    kw = dict(max_batch=2, buckets=(2,), ip_masks=True)
    pair = HiresPair(pipe.serve(128, 128, slot=0, **kw), pipe.serve(160, 160, slot=1, **kw)).warm()
    assert sorted(pair.hires.levels()) == [9, 25, 100, 400]
    text = _request(ctx, 9)
    e = [_image_embeds(9)]
    m = _masks(_region(1, 128, 128, [(0, 64, 0, 128)]))
    base = dict(prompt_embeds=text["prompt_embeds"], negative_prompt_embeds=text["negative_prompt_embeds"], guidance_scale=7.5,
                sampler_opt=KARRAS, num_inference_steps=STEPS, ip_adapter_image_embeds=e)
    hires = dict(upscale=True, upscale_x=X, upscale_method="bicubic", upscale_denoising_strength=STRENGTH)

    def run(p, request):
        fut = p.submit(request)
        pair.run_until_idle()
        return fut.result()

    ref = pipe.txt2img(None, fused=True, generator=_gen(77), sampler_name="sample_dpmpp_2m", output_type="latent", width=128,
                       height=128, **base, **hires, **m)[0].float().cpu()
    assert ref.shape == LAT2
    chained = run(pair, dict(base, generator=_gen(77), **hires, **m)).float().cpu()
    g = _gen(77)
    first = run(pair, dict(base, generator=g, **m))
    noise = pipe._randn_like_ref(LAT2, g, first.device, first.dtype)                      # the generator's next draw
    big = F.interpolate(first.float(), size=LAT2[2:], mode="bicubic").to(first.dtype)
    route = run(pair.hires, dict(base, image=big, latents=noise, strength=STRENGTH, **m)).float().cpu()
    no_mask = run(pair.hires, dict(base, image=big, latents=noise, strength=STRENGTH)).float().cpu()
    scale = ref.abs().max().item()
    d_chain, d_route = (chained - ref).abs().max().item(), (route - ref).abs().max().item()
    d_drop = (chained - no_mask).abs().max().item()
    print(f"vs pipe.txt2img(upscale=True, masks): chained {d_chain:.3e}, served pieces {d_route:.3e} (range {scale:.2f}); "
          f"chained vs second pass without the mask {d_drop:.3e}")
    assert torch.isfinite(chained).all()
    assert d_chain <= max(2 * d_route, 2e-3 * scale), (d_chain, d_route, scale)
    assert d_drop > 1e-3
    st = pair.stats()
    assert st["handoffs"] == 1 and st["base"]["captures_after_warm"] == 0 and st["hires"]["captures_after_warm"] == 0
