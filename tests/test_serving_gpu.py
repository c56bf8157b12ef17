"""Continuous batching on the MI355X (`-m gpu`): the per-row sampler step (dsc_cfg_dpmpp2m_step_rows) against the scalar
kernels bit for bit, per-group sigma in the region cross-attention (DSC_FLAG_SIGMA_PER_GROUP), and the serving batcher
(modules/serving.py) against lockstep `txt2img_coalesced` and each request's own `txt2img` call."""

import numpy as np
import pytest
import torch

from inputs import FakeTokenizer

pytestmark = pytest.mark.gpu
ATOL = 6e-3          # test_region_xattn_gpu.py's fp32-score tolerance against the oracle


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


def _h(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).half().cuda()


# ----------------------------------------------------------------------------- the per-row step kernel
CHW, TW = 4 * 16 * 16, 96


def _scalar_step(ops, x, eps_u, eps_c, old, p, tab_row):
    """cfg_dpmpp2m_step on ONE slot alone -> (x, old, x_in, t, sigma, tadd)"""
    x, old = x.clone(), old.clone()
    x_in = torch.empty(2, *x.shape[1:], dtype=x.dtype, device=x.device)
    t = torch.empty(2, device=x.device)
    s = torch.empty(1, device=x.device)
    tadd = torch.zeros(2, TW, dtype=x.dtype, device=x.device)
    ops.cfg_dpmpp2m_step(x, torch.cat([eps_u, eps_c]).contiguous(), old, p["sigma"], p["guidance"], p["a"], p["b"], p["c"],
                         p["c_in_next"], p["t_next"], p["sigma_next"], x_in, t, s,
                         row=None if tab_row is None else (tab_row, tadd))
    return x, old, x_in, t, s, tadd


def _rows_call(ops, x, eps, old, n_src, n_dst, recs):
    x_in = torch.full((2 * n_dst, *x.shape[1:]), 7.0, dtype=torch.float16, device="cuda")
    t = torch.full((2 * n_dst,), -1.0, device="cuda")
    s = torch.full((n_dst,), -1.0, device="cuda")
    tadd = torch.zeros(2 * n_dst, TW, dtype=torch.float16, device="cuda")
    ops.cfg_dpmpp2m_step_rows(x, eps, old, n_src, x_in, t, s, recs, tadd=tadd)
    return x_in, t, s, tadd


def _params(i):
    return {"mode": 0, "sigma": 14.6 / (i + 1), "guidance": 7.5 - i, "a": 0.8 - 0.05 * i, "b": 0.2 + 0.03 * i,
            "c": 0.0 if i == 0 else -0.01 * i, "c_in_next": 0.07 * (i + 1), "t_next": 900.0 - 50 * i, "sigma_next": 12.0 / (i + 1)}


def test_step_rows_uniform_equals_scalar_kernel(ops):
    n = 3
    x, old, eps = _h(n, 4, 16, 16, seed=1), _h(n, 4, 16, 16, seed=2), _h(2 * n, 4, 16, 16, seed=3)
    tab = _h(TW, seed=4)
    p = _params(1)
    x_in = torch.empty(2 * n, 4, 16, 16, dtype=torch.float16, device="cuda")
    t = torch.empty(2 * n, device="cuda")
    s = torch.empty(1, device="cuda")
    tadd = torch.zeros(2 * n, TW, dtype=torch.float16, device="cuda")
    xs, olds = x.clone(), old.clone()
    ops.cfg_dpmpp2m_step(xs, eps, olds, p["sigma"], p["guidance"], p["a"], p["b"], p["c"], p["c_in_next"], p["t_next"],
                         p["sigma_next"], x_in, t, s, row=(tab, tadd))
    xr, oldr = x.clone(), old.clone()
    got = _rows_call(ops, xr, eps, oldr, n, n, [dict(p, temb_row=tab) for _ in range(n)])
    torch.cuda.synchronize()
    assert torch.equal(xr, xs) and torch.equal(oldr, olds)
    assert torch.equal(got[0], x_in) and torch.equal(got[1], t) and torch.equal(got[3], tadd)
    assert torch.equal(got[2], s.expand(n))


# rows of 1024 halfs, and two lengths with a partial tail: 1444 = 361 four-half vectors (19 x 19 latents: 8-byte rows, a second
# workgroup with 105 live lanes), 2056 = 257 eight-half vectors (a second workgroup with one live lane)
MIXED = [pytest.param(*m, shape, id="-".join(map(str, m)) + tag)
         for shape, tag in (((4, 16, 16), ""), ((4, 19, 19), "-1444"), ((4, 2, 257), "-2056"))
         for m in [(2, 4, "SSJI"), (4, 2, "SISI"), (4, 4, "JSIS")]]


@pytest.mark.parametrize("n_src, n_dst, modes, shape", MIXED)
def test_step_rows_mixed_modes_equal_per_slot_kernels(ops, n_src, n_dst, modes, shape):
    """STEP / JOIN / IDLE mix with distinct scalars per slot, including bucket changes (n_src != n_dst): every slot equals the
    scalar kernel (or prepare_unet_input) run on that slot alone; IDLE slots write zeros and sigma 1"""
    n_slots = len(modes)
    x, old = _h(n_slots, *shape, seed=11), _h(n_slots, *shape, seed=12)
    eps = _h(2 * n_src, *shape, seed=13)
    tabs = [_h(TW, seed=20 + i) for i in range(n_slots)]
    recs = []
    for i, m in enumerate(modes):
        p = _params(i)
        p["mode"] = {"S": ops.ROW_STEP, "J": ops.ROW_JOIN, "I": ops.ROW_IDLE}[m]
        p["temb_row"] = tabs[i] if m != "I" else None
        recs.append(p)
    xr, oldr = x.clone(), old.clone()
    x_in, t, s, tadd = _rows_call(ops, xr, eps, oldr, n_src, n_dst, recs)
    torch.cuda.synchronize()
    for i, (m, p) in enumerate(zip(modes, recs)):
        rows = [i, n_dst + i]
        if m == "S":
            ex = _scalar_step(ops, x[i:i + 1], eps[i:i + 1], eps[n_src + i:n_src + i + 1], old[i:i + 1], p,
                              tabs[i] if i < n_dst else None)
            assert torch.equal(xr[i:i + 1], ex[0]) and torch.equal(oldr[i:i + 1], ex[1]), (modes, i)
            if i < n_dst:
                assert torch.equal(x_in[rows], ex[2]) and torch.equal(t[rows], ex[3]), (modes, i)
                assert s[i].item() == ex[4].item() and torch.equal(tadd[rows], ex[5]), (modes, i)
        elif m == "J":
            x_in1 = torch.empty(2, *shape, dtype=torch.float16, device="cuda")
            t1, s1 = torch.empty(2, device="cuda"), torch.empty(1, device="cuda")
            ops.prepare_unet_input(x[i:i + 1].clone(), p["c_in_next"], p["t_next"], p["sigma_next"], x_in1, t1, s1)
            torch.cuda.synchronize()
            assert torch.equal(x_in[rows], x_in1) and torch.equal(t[rows], t1) and s[i].item() == s1.item(), (modes, i)
            assert torch.equal(xr[i], x[i]) and not oldr[i].any(), (modes, i)
            assert torch.equal(tadd[rows], tabs[i].expand(2, -1)), (modes, i)
        else:
            assert torch.equal(xr[i], x[i]) and torch.equal(oldr[i], old[i]), (modes, i)
            if i < n_dst:
                assert not x_in[rows].any() and s[i].item() == 1.0 and not tadd[rows].any(), (modes, i)


def test_step_rows_clamped_grid_every_entry_equals_the_scalar_kernel(ops):
    """chw = 524296: 65537 eight-half vectors per row, so the grid clamps at 256 workgroups per slot and one of them strides a
    second time.  Two STEP slots: dsc_cfg_dpmpp2m_step_rows, dsc_cfg_linear_step_rows, the known-region entry without a known
    region and x_in[:, :chw] of dsc_cfg_linear_step_rows_cat carry the same bits - those of the scalar kernel on each slot alone"""
    chw, n, eh = 524296, 2, 8
    x, old, eps = _h(n, chw, seed=91), _h(n, chw, seed=92), _h(2 * n, chw, seed=93)
    tabs = [_h(TW, seed=94 + i) for i in range(n)]
    recs = [dict(_params(i), temb_row=tabs[i]) for i in range(n)]

    def run(fn, *more, row=chw):
        xr, oldr = x.clone(), old.clone()
        x_in = torch.full((2 * n, row), 7.0, dtype=torch.float16, device="cuda")
        t, s = torch.full((2 * n,), -1.0, device="cuda"), torch.full((n,), -1.0, device="cuda")
        tadd = torch.zeros(2 * n, TW, dtype=torch.float16, device="cuda")
        fn(xr, eps, oldr, n, x_in, t, s, recs, *more, tadd=tadd)
        torch.cuda.synchronize()
        return xr, oldr, x_in[:, :chw], t, s, tadd

    rows = run(ops.cfg_dpmpp2m_step_rows)
    others = {"linear": run(ops.cfg_linear_step_rows), "known": run(ops.cfg_dpmpp2m_step_rows_known, [None, None]),
              "cat": run(ops.cfg_linear_step_rows_cat, [_h(eh, seed=96), None], row=chw + eh)}
    for entry, got in others.items():
        for name, a, b in zip(("x", "old", "x_in", "t", "sigma_groups", "tadd"), got, rows):
            assert torch.equal(a, b), (entry, name)
    for i in range(n):
        pair = [i, n + i]
        ex = _scalar_step(ops, x[i:i + 1], eps[i:i + 1], eps[n + i:n + i + 1], old[i:i + 1], recs[i], tabs[i])
        torch.cuda.synchronize()
        assert torch.equal(rows[0][i:i + 1], ex[0]) and torch.equal(rows[1][i:i + 1], ex[1]), i
        assert torch.equal(rows[2][pair], ex[2]) and torch.equal(rows[3][pair], ex[3]), i
        assert rows[4][i].item() == ex[4].item() and torch.equal(rows[5][pair], ex[5]), i


# ----------------------------------------------------------------------------- per-group sigma in the region cross-attention
def _xattn_inputs(Bc, L, H, S, d, seed):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(Bc, L, H, d, generator=g) * 0.5).half().cuda()
    k = (torch.randn(Bc, S, H, d, generator=g) * 0.5).half().cuda()
    v = torch.randn(Bc, S, H, d, generator=g).half().cuda()
    base = torch.zeros(5, S)
    base[1:, 2:10] = torch.rand(4, 8, generator=g)
    w = base[torch.randint(0, 5, (Bc, L), generator=g)].contiguous()
    return q, k, v, w


def _run_xattn(ops, kind, q, k, v, w, sigma, groups, ref16, per_group):
    S = k.shape[1]
    if kind == "packed":
        comp = ops.compress_region_table(w)
        comp = (comp[0].cuda(), comp[1].cuda())
        return ops.region_xattn_packed(q, ops.xattn_kv_pack(k, v), S, comp, sigma, n_std_groups=groups,
                                       ref_fp16_rounding=ref16, per_group_sigma=per_group)
    return ops.region_xattn(q, k, v, w.cuda(), sigma, layout="blhd", n_std_groups=groups, ref_fp16_rounding=ref16,
                            per_group_sigma=per_group)


XCASES = [(kind, d, S, ref16) for kind in ("packed", "dense") for d in (40, 80, 160) for S in (77, 154)
          for ref16 in (True, False) if not (S > 96 and (kind == "dense" or ref16))]


@pytest.mark.parametrize("kind, d, S, ref16", XCASES)
def test_sigma_per_group_uniform_is_bit_identical(ops, kind, d, S, ref16):
    Bc, groups = 6, 3
    q, k, v, w = _xattn_inputs(Bc, 64, 2, S, d, seed=d + S)
    off = _run_xattn(ops, kind, q, k, v, w, torch.tensor([2.5], device="cuda"), groups, ref16, False)
    on = _run_xattn(ops, kind, q, k, v, w, torch.full((groups,), 2.5, device="cuda"), groups, ref16, True)
    torch.cuda.synchronize()
    assert torch.equal(on, off)


@pytest.mark.parametrize("kind, d, S, ref16", XCASES)
def test_sigma_per_group_distinct_equals_each_group_alone(ops, kind, d, S, ref16):
    Bc, groups = 6, 3
    q, k, v, w = _xattn_inputs(Bc, 64, 2, S, d, seed=3 * d + S)
    sig = [0.9, 4.0, 11.5]
    out = _run_xattn(ops, kind, q, k, v, w, torch.tensor(sig, device="cuda"), groups, ref16, True).float()
    for g in range(groups):
        rows = list(range(g, Bc, groups))
        alone = _run_xattn(ops, kind, q[rows].contiguous(), k[rows].contiguous(), v[rows].contiguous(), w[rows].contiguous(),
                           sig[g], 1, ref16, False).float()
        err = (out[rows] - alone).abs().max().item()
        assert err < ATOL, (g, err)
    other = _run_xattn(ops, kind, q, k, v, w, torch.tensor([sig[0]], device="cuda"), groups, ref16, False).float()
    assert (out[2::3] - other[2::3]).abs().max().item() > 2 * ATOL          # (the per-group sigmas DO matter)


def test_sigma_per_group_needs_a_group_vector(ops):
    q, k, v, w = _xattn_inputs(4, 64, 2, 77, 40, seed=5)
    with pytest.raises(ValueError, match="n_std_groups"):
        _run_xattn(ops, "dense", q, k, v, w, torch.tensor([1.0], device="cuda"), 2, True, True)


# ----------------------------------------------------------------------------- the batcher
def _tiny_pipe(seed=0):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(seed)
    cfg = UNetConfig.tiny()
    unet = UNet2DConditionModel(cfg).half().cuda()
    return cfg, StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())


def _masked(size, n_masks, weight, S=77):
    tok = FakeTokenizer()
    words = [f"object{r}a object{r}b" for r in range(n_masks)]
    ids = [49406, 320]
    for w in words:
        ids += tok(w).input_ids
    ids = ids + [49407] * (S - len(ids))
    pos = np.array([ids], dtype=np.int64)
    state = {}
    for r, w in enumerate(words):
        m = np.full((size, size), 255, dtype=np.uint8)
        c = size // 2
        m[(r // 2 % 2) * c:(r // 2 % 2 + 1) * c, (r % 2) * c:(r % 2 + 1) * c] = 0
        state[w] = {"map": m, "weight": weight, "mask_outsides": 0.0}
    return state, [pos.copy(), pos]


def _tiny_requests(ctx, n):
    reqs = []
    for i in range(n):
        emb = torch.randn(2, 77, ctx, generator=torch.Generator().manual_seed(300 + i)).half()
        state, ids = _masked(128, 1 + i % 3, 0.3 + 0.1 * i)
        reqs.append({"prompt_embeds": emb[1:2].cuda(), "negative_prompt_embeds": emb[0:1].cuda(), "text_input_ids": ids,
                     "region_map_state": state,
                     "latents": torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(400 + i)).half().cuda()})
    return reqs


def _single(pipe, r, size, steps, g, opt):
    return pipe.txt2img(None, height=size, width=size, num_inference_steps=steps, guidance_scale=g, sampler_name="sample_dpmpp_2m",
                        sampler_opt=opt, latents=r["latents"], region_map_state=r["region_map_state"],
                        prompt_embeds=r["prompt_embeds"], negative_prompt_embeds=r["negative_prompt_embeds"],
                        text_input_ids=r["text_input_ids"], output_type="latent")[0].float().cpu()


def test_batcher_all_start_together_equals_coalesced():
    """k = 4 different requests (= a bucket: no IDLE row changes the launch geometry), submitted before the first step with
    one schedule and guidance scale: bit for bit what txt2img_coalesced computes for them"""
    cfg, pipe = _tiny_pipe(1)
    reqs = _tiny_requests(cfg.cross_attention_dim, 4)
    opt = {"scheduler": "karras"}
    ref = [o.float().cpu() for o in pipe.txt2img_coalesced(reqs, height=128, width=128, num_inference_steps=5, guidance_scale=7.5,
                                                            sampler_opt=opt, output_type="latent")]
    b = pipe.serve(128, 128, max_batch=4, buckets=(1, 2, 4)).warm()
    futs = [b.submit(dict(r, num_inference_steps=5, guidance_scale=7.5, sampler_opt=opt)) for r in reqs]
    b.run_until_idle()
    got = [f.result().float().cpu() for f in futs]
    for i, (g_, r_) in enumerate(zip(got, ref)):
        assert torch.equal(g_, r_), (i, (g_ - r_).abs().max().item())
    assert b.stats()["captures_after_warm"] == 0


def test_batcher_staggered_joins_equal_their_own_txt2img():
    """A (4 steps) starts; B (3 steps, exponential schedule) joins after 2 steps; C (guidance 5) joins 3 steps later into the
    slot A freed.  Each final latent equals its own txt2img call within 2e-3 of the range (the coalesced test's bound); no
    capture after warm()"""
    cfg, pipe = _tiny_pipe(2)
    ra_, rb, rc = _tiny_requests(cfg.cross_attention_dim, 3)
    specs = {"A": (ra_, 4, 7.5, {"scheduler": "karras"}), "B": (rb, 3, 7.5, {"scheduler": "exponential"}),
             "C": (rc, 4, 5.0, {"scheduler": "karras"})}
    b = pipe.serve(128, 128, max_batch=4, buckets=(1, 2, 4)).warm()
    sub = lambda n: b.submit(dict(specs[n][0], num_inference_steps=specs[n][1], guidance_scale=specs[n][2],  # noqa: E731
                                  sampler_opt=specs[n][3]))
    futs = {"A": sub("A")}
    b.step()
    b.step()
    b.step()
    futs["B"] = sub("B")
    for _ in range(3):
        b.step()
    assert b._slots[0] is None                          # A has left
    futs["C"] = sub("C")
    b.step()
    assert b._slots[0] is not None and b._slots[0].req is not None and b._slots[0].guidance == 5.0
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["joins"] == 3 and st["leaves"] == 3, st
    singles = {n: _single(pipe, s[0], 128, s[1], s[2], s[3]) for n, s in specs.items()}
    scale = max(v.abs().max().item() for v in singles.values())
    for n in specs:
        g_ = futs[n].result().float().cpu()
        d = (g_ - singles[n]).abs().max().item()
        print(f"request {n}: vs its own txt2img {d:.3e} (range {scale:.2f})")
        assert d < 2e-3 * scale, (n, d, scale)


def test_batcher_full_size_join_mid_batch():
    """SD1.5 at 512x512, 25 steps: configs[1]'s request joins a batch already 10 steps into another request; its final latents
    against its own txt2img call are within the end-to-end bound (8e-3 max / 1e-3 mean of the range)"""
    import test_full_size_parity_gpu as fs
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    with torch.device("cuda"):
        unet = UNet2DConditionModel(UNetConfig.sd15())
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet.half().eval(), SD15Scheduler())
    reqs = [{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in r.items()} for r in fs._requests(2)]
    first, cfg1 = reqs[1], reqs[0]                    # reqs[0] is configs[1]'s request
    kw = dict(num_inference_steps=25, guidance_scale=7.5, sampler_opt={"scheduler": "karras"})
    b = pipe.serve(512, 512, max_batch=2, buckets=(1, 2)).warm()
    b.submit(dict(first, **kw))
    for _ in range(10):
        b.step()
    fut = b.submit(dict(cfg1, **kw))
    b.run_until_idle()
    assert b.stats()["captures_after_warm"] == 0
    got = fut.result().float().cpu()
    ref = _single(pipe, cfg1, 512, 25, 7.5, {"scheduler": "karras"})
    e = (got - ref).abs()
    scale = ref.abs().max().item()
    print(f"configs[1] joined at step 10: max {e.max().item():.3e} mean {e.mean().item():.3e} (range {scale:.2f})")
    assert e.max().item() < 8e-3 * scale and e.mean().item() < 1e-3 * scale
