"""IP-Adapter requests in the continuous batcher on the MI355X (`-m gpu`): dsc_ip_xattn_add_f16 (the image-token attention
accumulated in place with one scale per batch row) against an fp32 restatement of its formula, its skip / stride / capture
properties, and the serving batcher with image prompts against `txt2img(ip_adapter_image_embeds=...)` and against itself."""
import pytest
import torch

from inputs import FakeTokenizer

pytestmark = pytest.mark.gpu
ATOL32 = 6e-3        # tests/test_region_xattn_gpu.py: the project's attention-output tolerance
ROW_SCALE = [0.0, 0.7, 1.0, -0.5]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- the kernel
def _inputs(B, L, H, d, T, seed):
    """q, k, v drawn as tests/test_serving_gpu.py `_xattn_inputs` draws them, and the text branch's output the term lands on"""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, L, H, d, generator=g) * 0.5).half()
    k = (torch.randn(B, T, H, d, generator=g) * 0.5).half()
    v = torch.randn(B, T, H, d, generator=g).half()
    io = torch.randn(B, L, H * d, generator=g).half()
    return q, k, v, io


def _restated(q, k, v, io, row_scale, scale=None):
    """the header's formula in fp32 on the CPU, before the final rounding"""
    B, L, H, d = q.shape
    s = d ** -0.5 if scale is None else scale
    scores = torch.einsum("blhd,bthd->bhlt", q.float(), k.float()) * s
    p = torch.softmax(scores - scores.amax(-1, keepdim=True), dim=-1)
    o = torch.einsum("bhlt,bthd->blhd", p, v.float()).reshape(B, L, H * d)
    return io.float() + torch.tensor(row_scale).view(B, 1, 1) * o


CASES = [(64, 4, 8, 4), (256, 4, 16, 4), (361, 8, 40, 16), (64, 8, 80, 16), (16, 8, 160, 4), (4, 8, 160, 16), (100, 10, 64, 16)]


@pytest.mark.parametrize("L, H, d, T", CASES)
def test_ip_xattn_add_against_fp32_restatement(ops, L, H, d, T):
    """|error| <= |row_scale| * 6e-3 (the attention-output tolerance) + half an fp16 ulp of the largest |result| (the one
    final rounding), per row"""
    B = len(ROW_SCALE)
    q, k, v, io = _inputs(B, L, H, d, T, seed=L + d + T)
    ref = _restated(q, k, v, io, ROW_SCALE)
    got = ops.ip_xattn_add(q.cuda(), k.cuda(), v.cuda(), torch.tensor(ROW_SCALE, device="cuda"), io.cuda().clone())
    torch.cuda.synchronize()
    got = got.float().cpu()
    assert got.shape == io.shape
    for b, rs in enumerate(ROW_SCALE):
        top = ref[b].abs().max().item()
        half_ulp = 2.0 ** (torch.tensor(top).log2().floor().item() - 10) / 2
        err = (got[b] - ref[b]).abs().max().item()
        print(f"L={L} H={H} d={d} T={T} row {b} scale {rs}: max error {err:.3e} (bound {abs(rs) * ATOL32 + half_ulp:.3e})")
        assert err <= abs(rs) * ATOL32 + half_ulp, (b, err)
    assert torch.equal(got[0], io[0].float())                       # scale 0: untouched
    assert (got[1] - io[1].float()).abs().max().item() > 0.05       # (the term is not small)


def test_ip_xattn_add_several_tiles_per_wave_and_a_ragged_token_count(ops):
    """from 256 query tiles on (L > 4080) a wave walks four tiles and re-uses its K / V operands: the sizes either side of that
    threshold with a ragged last tile, and T = 5 (one token in the second group of four: the masked softmax lanes)"""
    for L in (4080, 4101):
        q, k, v, io = _inputs(4, L, 2, 16, 5, seed=L)
        ref = _restated(q, k, v, io, ROW_SCALE)
        got = ops.ip_xattn_add(q.cuda(), k.cuda(), v.cuda(), torch.tensor(ROW_SCALE, device="cuda"), io.cuda().clone())
        got = got.float().cpu()
        for b, rs in enumerate(ROW_SCALE):
            top = ref[b].abs().max().item()
            half_ulp = 2.0 ** (torch.tensor(top).log2().floor().item() - 10) / 2
            err = (got[b] - ref[b]).abs().max().item()
            assert err <= abs(rs) * ATOL32 + half_ulp, (L, b, err)
        assert torch.equal(got[0], io[0].float())


def test_ip_xattn_add_skipped_row_reads_nothing(ops):
    q, k, v, io = _inputs(4, 100, 8, 40, 16, seed=1)
    k[0], v[0] = float("nan"), float("nan")
    got = ops.ip_xattn_add(q.cuda(), k.cuda(), v.cuda(), torch.tensor(ROW_SCALE, device="cuda"), io.cuda().clone())
    torch.cuda.synchronize()
    assert torch.equal(got[0].cpu(), io[0])
    assert torch.isfinite(got[1:]).all()


def test_ip_xattn_add_query_strides_batch_stride_and_determinism(ops):
    B, L, H, d, T = 4, 361, 8, 40, 16
    q, k, v, io = _inputs(B, L, H, d, T, seed=2)
    rs = torch.tensor(ROW_SCALE, device="cuda")
    base = q[:1].cuda()
    shared = base.expand(B, -1, -1, -1)
    assert shared.stride(0) == 0
    a = ops.ip_xattn_add(shared, k.cuda(), v.cuda(), rs, io.cuda().clone())
    b = ops.ip_xattn_add(shared.contiguous(), k.cuda(), v.cuda(), rs, io.cuda().clone())
    c = ops.ip_xattn_add(shared, k.cuda(), v.cuda(), rs, io.cuda().clone())
    # k_ip / v_ip as views into one flat buffer with one row per batch row (the batcher's layout)
    flat = torch.zeros(B, 3 * T * H * d + 64, dtype=torch.float16, device="cuda")
    kv = flat[:, 64:64 + T * H * d].unflatten(-1, (T, H, d))
    vv = flat[:, 64 + T * H * d:64 + 2 * T * H * d].unflatten(-1, (T, H, d))
    kv.copy_(k)
    vv.copy_(v)
    e = ops.ip_xattn_add(shared, kv, vv, rs, io.cuda().clone())
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, e)


def test_ip_xattn_add_under_graph_capture(ops):
    """one captured call; row_scale, k_ip and v_ip are overwritten in place and io reset before the replay: the replay reads
    the device values of that moment"""
    B, L, H, d, T = 4, 100, 10, 64, 16
    q, k, v, io = (t.cuda() for t in _inputs(B, L, H, d, T, seed=3))
    _, k2, v2, _ = (t.cuda() for t in _inputs(B, L, H, d, T, seed=4))
    rs = torch.tensor(ROW_SCALE, device="cuda")
    rs2 = torch.tensor([0.4, 0.0, -1.0, 0.25], device="cuda")
    buf = io.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ip_xattn_add(q, k, v, rs, buf)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    buf.copy_(io)
    with torch.cuda.graph(g):
        ops.ip_xattn_add(q, k, v, rs, buf)
    rs.copy_(rs2)
    k.copy_(k2)
    v.copy_(v2)
    buf.copy_(io)
    g.replay()
    fresh = ops.ip_xattn_add(q, k2, v2, rs2, io.clone())
    torch.cuda.synchronize()
    assert torch.equal(buf, fresh)
    assert torch.equal(buf[1], io[1]) and not torch.equal(buf[0], io[0])


def test_ip_xattn_add_wrapper_refusals(ops):
    from diffusionspatialcontrol_amd import DscLibraryError

    def call(d=40, T=4, cpu_scale=False, H=2, L=16):
        q, k, v, io = (t.cuda() for t in _inputs(2, L, H, d, T, seed=5))
        rs = torch.ones(2) if cpu_scale else torch.ones(2, device="cuda")
        return ops.ip_xattn_add(q, k, v, rs, io)

    call()
    with pytest.raises(ValueError, match="head dim"):
        call(d=12)
    with pytest.raises(ValueError, match="head dim"):
        call(d=168)
    with pytest.raises(ValueError, match="IP_MAX_TOKENS"):
        call(T=ops.IP_MAX_TOKENS + 1)
    with pytest.raises(DscLibraryError):
        call(cpu_scale=True)                                        # row_scale is read on the device: no CPU tensor
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the batcher
EMB = 48
KARRAS = {"scheduler": "karras"}


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
    """to_k_ip / to_v_ip of every cross-attention layer, as tests/test_unet_pipeline_gpu.py::test_ip_adapter_unet_and_pipeline
    builds them (the published key numbering 1, 3, 5, ...)"""
    sd = {}
    for i, (n, m) in enumerate(_cross_layers(unet)):
        sd[f"{2 * i + 1}.to_k_ip.weight"] = torch.randn(m.inner_dim, ctx, generator=g) * 0.2 + (i if offset else 0)
        sd[f"{2 * i + 1}.to_v_ip.weight"] = torch.randn(m.inner_dim, ctx, generator=g) * 0.2
    return sd


def _standard_adapter(unet, ctx, g):
    """the 4-token adapter of the existing pipeline test (Linear + LayerNorm image projection)"""
    return {"image_proj": {"proj.weight": torch.randn(4 * ctx, EMB, generator=g) * 0.1, "proj.bias": torch.zeros(4 * ctx),
                           "norm.weight": torch.ones(ctx), "norm.bias": torch.zeros(ctx)},
            "ip_adapter": _adapter_weights(unet, ctx, g)}


def _plus_adapter(unet, ctx, g):
    """a 16-token Plus (Resampler) adapter in the checkpoint's original key layout (tests/test_host_logic.py writes the same)"""
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


def _request(ctx, i):
    emb = torch.randn(2, 77, ctx, generator=torch.Generator().manual_seed(300 + i)).half()
    return {"prompt_embeds": emb[1:2].cuda(), "negative_prompt_embeds": emb[0:1].cuda(),
            "latents": torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(400 + i)).half().cuda()}


def _image_embeds(i):
    """[negative; positive] along dim 0: a zero negative half, as encode_image returns for a plain image prompt"""
    e = torch.randn(2, 1, EMB, generator=torch.Generator().manual_seed(500 + i)).half()
    e[0] = 0
    return e.cuda()


def _serve_one(b, req, **kw):
    fut = b.submit(dict(req, **kw))
    b.run_until_idle()
    return fut.result().float().cpu()


def _txt2img(pipe, req, steps, fused, opt=KARRAS, **kw):
    return pipe.txt2img(None, height=128, width=128, num_inference_steps=steps, guidance_scale=7.5, sampler_name="sample_dpmpp_2m",
                        sampler_opt=opt, latents=req["latents"].clone(), prompt_embeds=req["prompt_embeds"],
                        negative_prompt_embeds=req["negative_prompt_embeds"], output_type="latent", fused=fused, **kw)[0].float().cpu()


@pytest.fixture(scope="module")
def served():
    """one tiny pipeline: a request served BEFORE the adapter is loaded, then the 4-token adapter and a warm batcher on it
    (one bucket of two slots: slot 1 is an idle row in every solo run)"""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    cfg, pipe = _tiny_pipe(3)
    ctx = cfg.cross_attention_dim
    kw = dict(num_inference_steps=4, guidance_scale=7.5, sampler_opt=KARRAS)
    req = _request(ctx, 0)
    before = _serve_one(pipe.serve(128, 128, max_batch=2, buckets=(2,)).warm(), req, **kw)
    pipe.load_ip_adapter(_standard_adapter(pipe.unet, ctx, torch.Generator().manual_seed(3)))
    pipe.set_ip_adapter_scale(0.7)
    b = pipe.serve(128, 128, max_batch=2, buckets=(2,)).warm()
    return {"pipe": pipe, "ctx": ctx, "b": b, "kw": kw, "req": req, "before": before}


def test_request_without_image_prompt_equals_a_batcher_without_adapter(served):
    """the IP-capable step with every row scale 0 computes, bit for bit, what the step computed before load_ip_adapter: the 16
    extra launches return before they touch anything and the text branch runs the launches it ran before"""
    got = _serve_one(served["b"], served["req"], **served["kw"])
    assert torch.equal(got, served["before"]), (got - served["before"]).abs().max().item()
    served["plain"] = got


def test_zero_scale_equals_no_image_prompt(served):
    plain = _serve_one(served["b"], served["req"], **served["kw"])
    zero = _serve_one(served["b"], served["req"], ip_adapter_image_embeds=[_image_embeds(0)], ip_adapter_scale=0.0, **served["kw"])
    assert torch.equal(zero, plain)
    assert served["b"].stats()["captures_after_warm"] == 0


def _against_txt2img(pipe, b, req, embeds, kw, what):
    """d_served = served vs txt2img(fused=True); d_routes = txt2img(fused=True) vs txt2img(fused=False), the two routes the
    pipeline had before: d_served <= 2 d_routes (the served route moves the IP branch's rounding points - one rounding instead
    of three - and the launch geometry at once) and d_served < 3e-2 range (the existing IP pipeline test's bound)"""
    got = _serve_one(b, req, ip_adapter_image_embeds=embeds, **kw)
    fused = _txt2img(pipe, req, 4, True, ip_adapter_image_embeds=embeds)
    proto = _txt2img(pipe, req, 4, False, ip_adapter_image_embeds=embeds)
    rng = max(1.0, fused.abs().max().item())
    d_served = (got - fused).abs().max().item()
    d_routes = (fused - proto).abs().max().item()
    print(f"{what}: d_served {d_served:.3e}  d_routes {d_routes:.3e}  range {rng:.2f}")
    assert torch.isfinite(got).all()
    assert d_served < 3e-2 * rng, (d_served, rng)
    assert d_served <= 2 * d_routes, (d_served, d_routes)
    return got


def test_one_ip_request_against_txt2img(served):
    """one 4-token adapter, scale 0.7 (the processors' scale at submit time: no `ip_adapter_scale` in the request).
    Measured on one MI355X (one run): d_served 2.031e-01, d_routes 8.750e-01, range 58.34."""
    pipe, b = served["pipe"], served["b"]
    got = _against_txt2img(pipe, b, served["req"], [_image_embeds(0)], served["kw"], "one adapter")
    plain = _serve_one(b, served["req"], **served["kw"])
    assert (got - plain).abs().max().item() > 1e-3                   # the image prompt did steer the result
    assert b.stats()["captures_after_warm"] == 0


def test_mixed_membership_equals_each_request_alone(served):
    """A (image prompt, scale 0.7, 4 steps) starts; B (no image prompt, exponential schedule, 3 steps) joins after 2 steps; C
    (other embeds, scale 0.3) joins into the slot A frees.  Each equals its own solo served run within 2e-3 of the range (the
    bound of test_batcher_staggered_joins_equal_their_own_txt2img: both sides run the same kernels); no capture after warm()"""
    b, ctx = served["b"], served["ctx"]
    specs = {"A": dict(_request(ctx, 1), num_inference_steps=4, guidance_scale=7.5, sampler_opt=KARRAS,
                       ip_adapter_image_embeds=[_image_embeds(1)], ip_adapter_scale=0.7),
             "B": dict(_request(ctx, 2), num_inference_steps=3, guidance_scale=7.5, sampler_opt={"scheduler": "exponential"}),
             "C": dict(_request(ctx, 3), num_inference_steps=4, guidance_scale=5.0, sampler_opt=KARRAS,
                       ip_adapter_image_embeds=[_image_embeds(3)], ip_adapter_scale=0.3)}
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
    assert b._slots[0] is not None and b._slots[0].ip_scale == [0.3]
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
    no_prompt = _serve_one(b, {k: v for k, v in specs["A"].items() if not k.startswith("ip_adapter")})
    assert (got["A"] - no_prompt).abs().max().item() > 1e-3
    assert b.stats()["captures_after_warm"] == 0


def test_two_adapters_against_txt2img():
    """a 4-token and a 16-token (Plus) adapter on one pipeline, scales 0.7 / 0.5: two launches per layer.
    Measured on one MI355X (one run): d_served 1.875e-01, d_routes 5.625e-01, range 69.88."""
    cfg, pipe = _tiny_pipe(4)
    ctx = cfg.cross_attention_dim
    g = torch.Generator().manual_seed(5)
    pipe.load_ip_adapter([_standard_adapter(pipe.unet, ctx, g), _plus_adapter(pipe.unet, ctx, g)])
    pipe.set_ip_adapter_scale([0.7, 0.5])
    b = pipe.serve(128, 128, max_batch=2, buckets=(2,)).warm()
    hidden = (torch.randn(2, 1, 9, 24, generator=torch.Generator().manual_seed(6)) * 0.5).half().cuda()     # CLIP hidden states
    embeds = [_image_embeds(7), hidden]
    kw = dict(num_inference_steps=4, guidance_scale=7.5, sampler_opt=KARRAS)
    req = _request(ctx, 5)
    got = _against_txt2img(pipe, b, req, embeds, kw, "two adapters")
    plain = _serve_one(b, req, **kw)
    assert (got - plain).abs().max().item() > 1e-3
    assert b.stats()["captures_after_warm"] == 0
