"""Prompt strings on the text lane of the continuous batcher on the MI355X (`-m gpu`): dsc_prompt_weight_rows_f16 against the
restatement of its contract (ops.prompt_weight_numpy) bit for bit - shapes on both sides of a slice and of the 1024-lane
workgroup, one and sixteen groups, rows in any order, idle groups, destinations inside guard bands, every refusal - and the lane
of `pipe.serve(..., text=True)` against the encoder's own rows, `encode_prompt_function` and requests that bring embeddings."""
import ctypes

import numpy as np
import pytest
import torch

import guards
from inputs import FakeClipTokenizer
from test_serving_img_gpu import _gen, _ulps, tiny  # noqa: F401  (tiny: the tiny 4-channel pipeline, a fixture)

pytestmark = pytest.mark.gpu
SIZE, STEPS = 128, 5
CLIP = dict(vocab_size=49408, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407)
MULTS = (1.0, 1.1, 1 / 1.1, 1.21, 1.3, 0.5)
P = "a photo of a red apple on a wooden table near a blue vase"
TWO = ", ".join(f"(item{i}:1.2) with [detail]" for i in range(30))            # two chunks, commas near the border
BAD_ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- dsc_prompt_weight_rows_f16
def _z(m, T, C, seed):
    """encoder-like rows: unit spread around a mean of -0.11 and one large channel (what CLIP's last hidden state looks like)"""
    z = torch.randn(m, T, C, generator=_gen(seed)) - 0.11
    z[:, :, min(3, C - 1)] += 6.0
    return z.half()


def _mult(kind, T, seed):
    if kind == "ones":
        return torch.ones(2, T)
    if kind == "zeros":
        return torch.zeros(2, T)
    m = torch.tensor(MULTS, dtype=torch.float32)[torch.randint(0, len(MULTS), (2, T), generator=_gen(seed))]
    if kind == "negative":
        m[1, T // 2] = -1.3
    return m


def _launch(ops, z, kinds, ld_extra=8, seed=0):
    """one launch over len(kinds) groups (a kind of None: an idle group) that read the rows of z back to front -> per group
    (its two row indices, its multipliers, its two fenced destinations as (buf, view))"""
    m, T, C = z.shape
    zd = z.cuda()
    groups, kept = [], []
    for j, kind in enumerate(kinds):
        rows = (m - 1 - 2 * j, m - 2 - 2 * j) if j % 2 == 0 else (m - 2 - 2 * j, m - 1 - 2 * j)
        mult = _mult(kind or "mixed", T, seed + j)
        outs = [guards.fenced(T, C, ld=C + ld_extra, tail_rows=2) for _ in range(2)]
        kept.append((rows, mult, outs))
        groups.append(None if kind is None else {"rows": rows, "mult": mult.cuda(), "out": (outs[0][1], outs[1][1])})
    ops.prompt_weight_rows(zd, groups)
    torch.cuda.synchronize()
    return kept


def _check(ops, z, kinds, kept):
    for kind, (rows, mult, outs) in zip(kinds, kept):
        for buf, view in outs:
            assert guards.untouched(buf, view)
        if kind is None:
            assert all(guards.all_sentinel(buf) for buf, _ in outs)
            continue
        want = torch.from_numpy(ops.prompt_weight_numpy(z[list(rows)].numpy(), mult.numpy()))
        got = torch.stack([view.cpu() for _, view in outs])
        if kind == "zeros":
            assert torch.isnan(want).all() and torch.isnan(got).all()
        else:
            assert torch.isfinite(want).all() and torch.equal(got, want), (kind, rows, _ulps(got, want))


@pytest.mark.parametrize("T, C", [(1, 8), (3, 24), (77, 64), (77, 768)])
@pytest.mark.parametrize("n", [1, 16])
def test_kernel_is_the_restatement(ops, T, C, n):
    """sixteen groups: mixed multipliers, an idle group (its fenced destinations keep every sentinel), all-ones multipliers (not
    the identity, see test_kernel_edge_multipliers_alone), a negative multiplier and all-zero multipliers (after = 0: ratio is
    +-inf and every element NaN, as the eager chain gives).  Rows of z are read back to front, in either order within a group."""
    kinds = ["mixed"] if n == 1 else ["mixed", "ones", None, "negative", "zeros"] + ["mixed"] * 11
    z = _z(2 * n + 1, T, C, seed=T + C)
    _check(ops, z, kinds, _launch(ops, z, kinds, seed=10 * n))


@pytest.mark.parametrize("kind", ["ones", "negative", "zeros"])
def test_kernel_edge_multipliers_alone(ops, kind):
    """All-ones multipliers are NOT the identity: out = fp16(fp32(z * ratio)) with ratio = fp32(fp16(mean)) / fp32(mean), which
    is 1 only when the mean is an fp16 value.  |ratio - 1| is at most 2^-11 (fp16's rounding of the mean) and half an ulp of an
    element is 2^-12 to 2^-11 of it: below 2^-12 nothing moves (seed 3: ratio - 1 = -2.3e-4, the input comes back), above it the
    elements with the larger mantissas move by one ulp (seed 4: ratio - 1 = +3.1e-4, a third of them)."""
    for seed in (3, 4):
        z = _z(2, 77, 64, seed=seed)
        kept = _launch(ops, z, [kind], ld_extra=0)
        _check(ops, z, [kind], kept)
        if kind == "ones":
            got = torch.stack([view.cpu() for _, view in kept[0][2]])
            moved = (got != z[[1, 0]]).float().mean().item()
            print(f"all-ones multipliers, seed {seed}: {100 * moved:.1f} % of the elements move")
            assert _ulps(got, z[[1, 0]]) <= 1 and (moved == 0.0 if seed == 3 else 0.2 < moved < 0.5)


def test_kernel_bits_do_not_depend_on_the_grid(ops):
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    z = _z(4, 77, 768, seed=8)
    outs = []
    try:
        for slices in (1, 3, 8, 64, 0):
            lib.dsc_debug_set_prompt_weight_slices(slices)
            kept = _launch(ops, z, ["mixed", "negative"], seed=4)
            _check(ops, z, ["mixed", "negative"], kept)
            outs.append([view.cpu() for _, _, o in kept for _, view in o])
    finally:
        lib.dsc_debug_set_prompt_weight_slices(0)
    assert all(torch.equal(a, b) for other in outs[1:] for a, b in zip(outs[0], other))


def test_kernel_refusals_launch_nothing(ops):
    """every DSC_ERR_BAD_ARG / DSC_ERR_UNSUPPORTED case of the header through the C ABI itself: the code comes back and no
    destination element is written"""
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    m, T, C, ld = 4, 5, 16, 24
    z = _z(m, T, C, seed=1).cuda()
    mult = torch.ones(2, T + 1, device="cuda")
    fences = [guards.fenced(T, C, ld=ld, tail_rows=2) for _ in range(2)]
    o0, o1 = (view.data_ptr() for _, view in fences)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(z_ptr=z.data_ptr(), m_=m, T_=T, C_=C, n=1, ldo=ld, rows=(0, 1), mp=mult.data_ptr(), out=(o0, o1), null_groups=False):
        recs = (_lib.PromptWeightGroup * 17)()
        for i in range(max(n, 1)):
            rec = recs[i]
            rec.z_row[0], rec.z_row[1], rec.mult, rec.out[0], rec.out[1] = rows[0], rows[1], mp, out[0], out[1]
        return lib.dsc_prompt_weight_rows_f16(ctypes.c_void_p(z_ptr), m_, T_, C_, None if null_groups else recs, n, ldo, stream)

    bad = [dict(z_ptr=None), dict(null_groups=True), dict(m_=0), dict(T_=0), dict(C_=0), dict(n=0), dict(n=17), dict(ldo=C - 8),
           dict(out=(o0, None)), dict(out=(None, o1)), dict(mp=None), dict(rows=(0, m)), dict(rows=(-1, 1)), dict(out=(o0, o0)),
           dict(out=(o0, z.data_ptr())), dict(out=(o0, z.data_ptr() + 2 * T * C)), dict(mp=o0)]
    for kw in bad:
        assert call(**kw) == BAD_ARG, kw
    unsupported = [dict(C_=12, ldo=24), dict(ldo=C + 4), dict(z_ptr=z.data_ptr() + 2), dict(out=(o0 + 2, o1)), dict(out=(o0, o1 + 8)),
                   dict(mp=mult.data_ptr() + 2)]
    for kw in unsupported:
        assert call(**kw) == UNSUPPORTED, kw
    assert call(out=(None, None)) == 0                                          # an idle group: accepted, nothing launched
    torch.cuda.synchronize()
    assert all(guards.all_sentinel(buf) for buf, _ in fences)
    assert call() == 0                                                          # and the call they all vary is a good one
    torch.cuda.synchronize()
    assert all(guards.untouched(buf, view) and torch.isfinite(view).all() for buf, view in fences)
    # the wrapper's own checks, before the library is reached
    ok = {"rows": (0, 1), "mult": mult[:, :T].contiguous(), "out": (fences[0][1], fences[1][1])}
    for groups in ([], [ok] * 17, [dict(ok, rows=(0, 4))], [dict(ok, rows=(0, True))], [dict(ok, mult=mult)], [dict(ok, mult=mult[:, :T].cpu())],
                   [dict(ok, out=(fences[0][1], fences[0][1]))], [dict(ok, out=(fences[0][1], fences[1][1][:, :8]))],
                   [dict(ok, out=(fences[0][1],))], [dict(ok, ldo=24)], [{"rows": (0, 1), "mult": ok["mult"]}]):
        with pytest.raises(ValueError, match="prompt_weight_rows"):
            ops.prompt_weight_rows(z, groups)
    with pytest.raises(TypeError, match="prompt_weight_rows"):
        ops.prompt_weight_rows(z.float(), [ok])
    with pytest.raises(_lib.DscLibraryError):
        ops.prompt_weight_rows(z.cpu(), [ok])                                   # no CPU fallback


# ----------------------------------------------------------------------------- the lane
@pytest.fixture(scope="module")
def env(tiny):    # noqa: F811
    """the tiny pipeline with a tiny native CLIP (hidden 64 = the UNet's cross_attention_dim, one head of 64: the kernel route)
    whose final LayerNorm has a bias, as a trained one has: the mean the weighting restores is away from zero"""
    from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel
    torch.manual_seed(5)
    clip = CLIPTextModel(CLIP)
    with torch.no_grad():
        clip.final_layer_norm.bias.copy_(torch.rand(64) * 0.5 + 0.25)
        clip.final_layer_norm.weight.copy_(torch.rand(64) * 0.5 + 0.75)
    clip = clip.half().cuda().eval()
    assert clip.kernel_route(2, 77)
    tiny.pipe.text_encoder, tiny.pipe.tokenizer = clip, FakeClipTokenizer()
    tiny.plain = {"guidance_scale": 7.5, "sampler_opt": {"scheduler": "karras"}, "num_inference_steps": STEPS}
    return tiny


def _serve(pipe, **kw):
    return pipe.serve(SIZE, SIZE, max_batch=2, buckets=(1, 2), **kw).warm()


def _lat(seed):
    return torch.randn(1, 4, 16, 16, generator=_gen(seed)).half()


def _rows(r):
    torch.cuda.synchronize()
    return torch.cat([r.text[0], r.text[1]]).cpu()                               # [negative; positive], [2, S, C]


def _restated(ops, pipe, ids, mult, clip_skip=None, together=False):
    """the restatement applied to the encoder's own rows for these ids [n, 2, 77] and multipliers -> [2, 77 n, C]; the encoder
    runs one [2, 77] call per chunk, or (`together`) one call on all 2 n rows, as the lane's encode did"""
    from diffusionspatialcontrol_amd.modules.encoder_prompt_modify import final_layer_norm_of

    def encode(flat):
        with torch.no_grad():
            if clip_skip is None:
                return pipe.text_encoder(flat).last_hidden_state
            return final_layer_norm_of(pipe.text_encoder)(pipe.text_encoder(flat, output_hidden_states=True).hidden_states[-clip_skip])

    calls = [ids.reshape(-1, 77)] if together else list(ids)
    z = torch.cat([encode(c.cuda()) for c in calls]).cpu().numpy().reshape(ids.shape[0], 2, 77, -1)
    return torch.from_numpy(np.concatenate([ops.prompt_weight_numpy(z[k], mult[k].numpy()) for k in range(ids.shape[0])], axis=1))


def _eager(pipe, prompt, negative, clip_skip=None):
    from diffusionspatialcontrol_amd.modules.encoder_prompt_modify import encode_prompt_function
    with torch.no_grad():
        pos, neg, ids = encode_prompt_function(pipe, prompt, pipe._execution_device, 1, True, negative, clip_skip=clip_skip, long_encode=0)
    torch.cuda.synchronize()
    return torch.cat([neg, pos]).cpu(), ids


@pytest.mark.parametrize("clip_skip", [None, 2])
def test_lane_rows_at_text_batch_1(ops, env, clip_skip):
    """the request's rows are the restatement applied to the encoder's own output for its ids, bit for bit, and within one fp16
    ulp of encode_prompt_function's default branch; the ids are that function's"""
    pipe = env.pipe
    prompt, negative = "a (red:1.3) apple, on a [wooden] table ((shiny))", "blurry, (low quality:1.4)"
    b = _serve(pipe, text=True, text_batch=1, clip_skip=clip_skip)
    fut = b.submit(dict(env.plain, prompt=prompt, negative_prompt=negative, latents=_lat(1)))
    r = b._queue[0]
    ids, mult = r.txt.ids.clone(), r.txt.mult.clone()
    assert b.step() and b.stats()["active"] == 1 and b.stats()["text_encodes"] == 1 and b.stats()["text_groups"] == 1
    got = _rows(r)
    assert torch.equal(got, _restated(ops, pipe, ids, mult, clip_skip))
    eager, eager_ids = _eager(pipe, prompt, negative, clip_skip)
    print(f"clip_skip={clip_skip}: lane vs encode_prompt_function: {_ulps(got, eager)} ulp max, "
          f"{100.0 * (got != eager).float().mean().item():.3f} % differ")
    assert eager.dtype == torch.float16 and _ulps(got, eager) <= 1
    assert all(np.array_equal(a, w) for a, w in zip(r.txt.np_ids, eager_ids))
    b.run_until_idle()
    assert torch.isfinite(fut.result(timeout=0)).all() and b.stats()["captures_after_warm"] == 0


def test_prompt_equals_its_embeddings_and_region_ids(ops, env):
    """a request with `prompt` (and a region state, nothing else) ends in the bits of the same request submitted with
    encode_text's embeddings and ids, on the lane batcher and on a flagless one; encode_text's ids are the tokenizer's"""
    pipe = env.pipe
    b = _serve(pipe, text=True, text_batch=2)
    given = b.encode_text(P, "blurry")
    assert all(np.array_equal(a, w) for a, w in zip(given["text_input_ids"], env.base["text_input_ids"]))
    assert given["prompt_embeds"].shape == (1, 77, 64) and given["prompt_embeds"].dtype == torch.float16
    outs = {}
    for state in (None, env.base["region_map_state"]):
        reqs = {"prompt": dict(env.plain, prompt=P, negative_prompt="blurry", region_map_state=state),
                "embeds": dict(env.plain, region_map_state=state, **given)}
        for name, req in reqs.items():
            fut = b.submit(dict(req, latents=_lat(2)))
            b.run_until_idle()
            outs[name, state is None] = fut.result(timeout=0)
        flagless = _serve(pipe)
        fut = flagless.submit(dict(reqs["embeds"], latents=_lat(2)))
        flagless.run_until_idle()
        assert torch.isfinite(outs["prompt", state is None]).all()
        assert torch.equal(outs["prompt", state is None], outs["embeds", state is None])
        assert torch.equal(outs["prompt", state is None], fut.result(timeout=0))
    assert not torch.equal(outs["prompt", True], outs["prompt", False])          # the region tables are live
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["text_encodes"] == 3 and st["leaves"] == 4, st


def test_two_requests_that_arrive_together_share_one_encode(ops, env):
    pipe = env.pipe
    b = _serve(pipe, text=True, text_batch=2)
    texts = [("a (cat:1.2) on a mat", "blurry"), ("[dim] light, a ((dog))", "")]
    futs = [b.submit(dict(env.plain, prompt=p, negative_prompt=n, latents=_lat(3 + i))) for i, (p, n) in enumerate(texts)]
    records = list(b._queue)
    ids = torch.cat([r.txt.ids for r in records])
    mult = torch.cat([r.txt.mult for r in records])
    assert b.step()
    st = b.stats()
    assert st["text_encodes"] == 1 and st["text_groups"] == 2 and st["active"] == 2, st
    want = _restated(ops, pipe, ids, mult, together=True)                        # the encoder on the same four-row batch
    for i, r in enumerate(records):
        assert torch.equal(_rows(r), want[:, 77 * i:77 * (i + 1)]), i
    b.run_until_idle()
    assert all(torch.isfinite(f.result(timeout=0)).all() for f in futs) and b.stats()["captures_after_warm"] == 0


def test_two_chunk_prompt_and_a_padded_one_on_154_keys(ops, env):
    pipe = env.pipe
    b = _serve(pipe, text=True, text_batch=1, text_len=154)
    futs = [b.submit(dict(env.plain, prompt=TWO, negative_prompt="blurry", latents=_lat(5))),
            b.submit(dict(env.plain, prompt="a cat", latents=_lat(6)))]
    long, short = list(b._queue)
    assert long.txt.real == 2 and short.txt.real == 1 and short.txt.chunks == 2
    ids, mult = long.txt.ids.clone(), long.txt.mult.clone()
    assert b.step() and b.step()
    st = b.stats()
    assert st["text_encodes"] == 3 and st["text_groups"] == 3, st               # long's two chunks, short's one: its second is no group
    got = _rows(long)
    eager, eager_ids = _eager(pipe, TWO, "blurry")
    assert got.shape == (2, 154, 64) and eager.shape == (2, 154, 64) and _ulps(got, eager) <= 1
    assert torch.equal(got, _restated(ops, pipe, ids, mult))
    assert all(np.array_equal(a, w) for a, w in zip(long.txt.np_ids, eager_ids))
    padded = _rows(short)
    assert _ulps(padded[:, :77], _eager(pipe, "a cat", "")[0]) <= 1
    empty = torch.tensor([b._parser.empty_chunk().tokens] * 2)[None]
    assert torch.equal(padded[:, 77:], _restated(ops, pipe, empty, torch.ones(1, 2, 77)))       # the chunk empty in both rows
    b.run_until_idle()
    assert all(torch.isfinite(f.result(timeout=0)).all() for f in futs) and b.stats()["captures_after_warm"] == 0
    with pytest.raises(ValueError, match="3 chunks"):
        b.submit(dict(env.plain, prompt=" ".join(f"w{i}" for i in range(160))))


def test_driver_thread_resolves_prompt_requests(env):
    b = _serve(env.pipe, text=True, text_batch=2).start()
    try:
        futs = [b.submit(dict(env.plain, prompt=f"a (thing{i}:1.{i})", negative_prompt="blurry", latents=_lat(20 + i)))
                for i in range(3)]
        outs = [f.result(timeout=120) for f in futs]
    finally:
        b.stop()
    st = b.stats()
    assert all(o.shape == (1, 4, 16, 16) and torch.isfinite(o).all() for o in outs)
    assert st["text_groups"] == 3 and st["queued"] == 0 and st["active"] == 0 and st["captures_after_warm"] == 0, st


def test_hires_pair_encodes_once(env):
    """a request with `prompt` and `upscale` is encoded once; its second pass (region tables at the target size included) runs on
    the first's rows and ids: the bits of a flagless pair given encode_text's output"""
    def run(pair, req):
        fut = pair.submit(dict(env.plain, generator=_gen(81), upscale=True, upscale_x=1.5, upscale_denoising_strength=0.5,
                               region_map_state=env.base["region_map_state"], **req))
        pair.run_until_idle()
        return fut.result(timeout=0)
    pair = env.pipe.serve_hires(SIZE, SIZE, 1.5, max_batch=2, buckets=(1, 2), text=True, text_batch=1).warm()
    given = pair.base.encode_text(P, "blurry")
    got = run(pair, dict(prompt=P, negative_prompt="blurry"))
    st = pair.stats()
    assert pair.base.text_on and not pair.hires.text_on and pair.hires.exec.text_lane is None
    assert st["base"]["text_encodes"] == 2 and "text_encodes" not in st["hires"], st       # encode_text's and the request's one
    assert st["handoffs"] == 1 and st["base"]["captures_after_warm"] == 0 and st["hires"]["captures_after_warm"] == 0
    plain = env.pipe.serve_hires(SIZE, SIZE, 1.5, max_batch=2, buckets=(1, 2)).warm()
    ref = run(plain, given)
    assert "text_encodes" not in plain.stats()["base"]
    assert got.shape == (1, 4, 24, 24) and torch.isfinite(got).all() and torch.equal(got, ref)


def test_flagless_batcher_is_unchanged(env):
    b = _serve(env.pipe)
    assert b.exec.text_lane is None and not b.text_on and "text_encodes" not in b.stats()
    with pytest.raises(ValueError, match="a request needs prompt_embeds and negative_prompt_embeds"):
        b.submit(dict(env.plain, prompt="a cat"))
    with pytest.raises(TypeError):
        env.pipe.serve(SIZE, SIZE, txt=True)
    outs = []
    for kw in ({}, {}, {"text": True}):                                          # embeddings run the same bits on all three
        b = _serve(env.pipe, **kw)
        fut = b.submit(dict(env.base, num_inference_steps=STEPS, latents=_lat(9)))
        b.run_until_idle()
        outs.append(fut.result(timeout=0))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
