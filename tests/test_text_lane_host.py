"""Prompt strings on the text lane of the continuous batcher (modules/serving/text_lane.py), the host half: the restatement of
dsc_prompt_weight_rows_f16's contract (ops.prompt_weight_numpy - the GPU tests' reference) against the literal eager chain, the
ids and multipliers `submit` makes against FrozenCLIPEmbedderWithCustomWords' own, every refusal, and the queue logic against a
recording executor whose lane events the test controls."""
import math
import types

import numpy as np
import pytest
import torch

from inputs import FakeClipTokenizer, fake_text_encoder
from serving_fakes import RecordingExec

from diffusionspatialcontrol_amd import ops
from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel
from diffusionspatialcontrol_amd.modules.prompt_parser import FrozenCLIPEmbedderWithCustomWords
from diffusionspatialcontrol_amd.modules.serving import HiresPair, ServingBatcher, text_lane

H = W = 128
LAT = torch.zeros(1, 4, 16, 16).half()
CLIP = dict(vocab_size=49408, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407)
MULTS = (1.0, 1.1, 1 / 1.1, 1.21, 1.3, 0.5)
TWO = " ".join(f"word{i}" for i in range(100))                     # 100 tokens, no commas: two chunks
THREE = " ".join(f"word{i}" for i in range(160))                   # three chunks


# ----------------------------------------------------------------------------- the restatement against the eager chain
def _ulp_key(a):
    i = a.view(np.int16).astype(np.int32)
    return np.where(i < 0, -(i & 0x7FFF), i)


def _case(C, seed):
    """[2, 77, C] with a realistic non-zero mean (CLIP's last hidden state sits near -0.1 with a few large channels) and
    per-token multipliers drawn from what the emphasis syntax produces"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(2, 77, C, generator=g) * 1.0 - 0.11
    z[:, :, 3] += 6.0
    mult = torch.tensor(MULTS, dtype=torch.float32)[torch.randint(0, len(MULTS), (2, 77), generator=g)]
    mult[:, 0] = mult[:, -1] = 1.0                                    # BOS and the closing EOS carry 1
    return z.half(), mult


@pytest.mark.parametrize("C", [32, 64, 768])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_is_the_eager_chain_to_one_ulp(C, seed):
    """ops.prompt_weight_numpy (exact sums, each rounded once) against the literal torch chain on the CPU (fp16 z, fp32
    multipliers: torch.asarray of Python floats is float32, so `z * m` is float32).  torch's means are fp32 accumulations, so
    the ratio may differ by one fp32 ulp, which moves an element that sits on a rounding boundary by one fp16 ulp: every element
    within 1 ulp, at most 1 % of them different at all."""
    z, mult = _case(C, seed)
    assert torch.asarray([[1.0, 1.1]]).dtype == torch.float32
    want = ops.prompt_weight_torch(z, mult).numpy()
    literal = z * mult.reshape(mult.shape + (1,)).expand(z.shape)
    assert literal.dtype == torch.float32
    assert torch.equal((literal * (z.mean() / literal.mean())).to(torch.float16), torch.from_numpy(want))
    got = ops.prompt_weight_numpy(z.numpy(), mult.numpy())
    off = np.abs(_ulp_key(got) - _ulp_key(want))
    print(f"C={C} seed={seed}: max {off.max()} ulp, {100.0 * (off > 0).mean():.3f} % differ")
    assert off.max() <= 1
    assert (off > 0).mean() <= 0.01


def test_sequential_fp64_sum_gives_the_same_means():
    """the kernel adds in fp64 in a fixed order, the restatement with math.fsum: for these inputs both give the same fp16 /
    fp32 means"""
    for C in (32, 64, 768):
        z, mult = _case(C, 0)
        zf = z.numpy().astype(np.float32)
        p = zf * mult.numpy()[:, :, None]
        for values, kind in ((zf, np.float16), (p, np.float32)):
            seq = 0.0
            for v in values.ravel().tolist():
                seq += v
            assert kind(seq / values.size) == kind(math.fsum(values.ravel().tolist()) / values.size)


def test_restatement_edge_values():
    z, _ = _case(32, 5)
    ones = ops.prompt_weight_numpy(z.numpy(), np.ones((2, 77), np.float32))
    assert np.abs(_ulp_key(ones) - _ulp_key(z.numpy())).max() <= 1 and not np.array_equal(ones, z.numpy())   # not the identity
    assert np.isnan(ops.prompt_weight_numpy(z.numpy(), np.zeros((2, 77), np.float32))).all()
    with pytest.raises(ValueError, match="fp16"):
        ops.prompt_weight_numpy(z.float().numpy(), np.ones((2, 77), np.float32))


# ----------------------------------------------------------------------------- ids and multipliers
@pytest.fixture(scope="module")
def parser():
    return FrozenCLIPEmbedderWithCustomWords(FakeClipTokenizer(), fake_text_encoder(), None)


def _parser_rows(parser, negative, prompt):
    """(ids [2, 77 k], multipliers [k][2][77]) of FrozenCLIPEmbedderWithCustomWords' own forward"""
    seen = []
    was = parser.process_tokens
    parser.process_tokens = lambda tokens, mults: (seen.append(mults), was(tokens, mults))[1]
    try:
        ids, _ = parser([negative, prompt])
    finally:
        parser.process_tokens = was
    return ids, seen


@pytest.mark.parametrize("negative, prompt, real", [
    ("blurry", "a (red:1.3) apple, on a [wooden] table", 1), ("", "a ((shiny)) vase", 1), ("bad, (worse:1.4)", TWO, 2),
    ("", THREE, 3), (TWO, "short", 2), ("low quality", "first part BREAK second (part:0.5)", 2)])
def test_ids_and_multipliers_are_the_parsers(parser, negative, prompt, real):
    want_ids, want_mults = _parser_rows(parser, negative, prompt)
    h = text_lane.prompt_chunks(parser, negative, prompt, real, 77 * real)
    assert h.real == real and h.chunks == real and h.sent == 0
    assert np.array_equal(np.concatenate(h.np_ids), want_ids) and h.np_ids[0].shape == (1, 77 * real)
    assert h.ids.dtype == torch.int64 and h.mult.dtype == torch.float32
    assert np.array_equal(h.ids.numpy().transpose(1, 0, 2).reshape(2, -1), want_ids)
    assert np.array_equal(h.mult.numpy(), np.array(want_mults, dtype=np.float32))
    # padded to a batcher of more chunks: the same groups, empty chunks behind them in the ids the region encoder reads
    wide = text_lane.prompt_chunks(parser, negative, prompt, real + 2, 77 * (real + 2))
    empty = parser.empty_chunk().tokens
    assert wide.real == real and wide.chunks == real + 2 and torch.equal(wide.ids, h.ids) and torch.equal(wide.mult, h.mult)
    for j in range(2):
        assert np.array_equal(wide.np_ids[j][:, :77 * real], h.np_ids[j])
        assert wide.np_ids[j][0, 77 * real:].tolist() == empty * 2
    with pytest.raises(ValueError, match=rf"{real} chunks.*text_len = {77 * real - 77}" if real > 1 else "chunks"):
        text_lane.prompt_chunks(parser, negative, prompt, real - 1, 77 * (real - 1))


# ----------------------------------------------------------------------------- construction and refusals
class HostClip(CLIPTextModel):
    """the package's encoder on the CPU, claiming the kernel route: what the constructor's checks read, without a device"""
    route = True

    def kernel_route(self, n, S):
        return self.route


def _pipe(encoder="clip", tokenizer=None, ctx=64):
    import dataclasses
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    unet = UNet2DConditionModel(dataclasses.replace(UNetConfig.tiny(), cross_attention_dim=ctx)).half()
    enc = HostClip(CLIP).half().eval() if encoder == "clip" else encoder
    return StableDiffusionPipeline(None, enc, tokenizer or FakeClipTokenizer(), unet, SD15Scheduler())


@pytest.fixture(scope="module")
def pipe():
    return _pipe()


class TextExec(RecordingExec):
    """RecordingExec plus the text lane's interface, with events the test completes: `dispatch_texts` groups as the lane does,
    marks the groups sent and gives the request an event that is not done; `text_wait` logs the wait and finishes it"""

    def __init__(self, text_batch=2, **kw):
        super().__init__(**kw)
        self.text_batch = text_batch
        self.encodes, self.waits = [], []

    def _prepared(self, r, kind):
        super()._prepared(r, kind)
        if getattr(r, "txt", None) is not None:
            r.text = ("text", r.req.get("name"))

    def prepare_text(self, r):
        r.text = ("text", None)

    def ensure_text(self):
        return int(self._ensure("text"))

    def dispatch_texts(self, requests, batch=None):
        batch = self.text_batch if batch is None else batch
        groups = [(r, k) for r in requests for k in range(r.txt.sent, r.txt.real)]
        for at in range(0, len(groups), batch):
            chunk = groups[at:at + batch]
            self.encodes.append([(r.req.get("name"), k) for r, k in chunk])
            ev = types.SimpleNamespace(done=False)
            for r, k in chunk:
                r.txt.sent = k + 1
                if r.txt.sent == r.txt.real:
                    r.txt.ev = ev
        self._event("dispatch_texts", [r.req.get("name") for r in requests])
        return -(-len(groups) // batch), len(groups)

    def text_ready(self, r):
        return r.txt.ev is not None and r.txt.ev.done

    def text_wait(self, r):
        self.waits.append(r.req.get("name"))
        r.txt.ev.done = True


def _req(name, steps=4, **kw):
    r = {"name": name, "num_inference_steps": steps, "guidance_scale": 7.5, "sampler_opt": {"scheduler": "karras"}, "latents": LAT}
    r.update(kw)
    return r


def _embeds(name, S=77, **kw):
    emb = torch.randn(2, S, 64, generator=torch.Generator().manual_seed(len(name)))
    return _req(name, prompt_embeds=emb[1:2].half(), negative_prompt_embeds=emb[0:1].half(), **kw)


def _batcher(pipe, **kw):
    ex = TextExec(text_batch=kw.get("text_batch", 2))
    kw = dict(dict(max_batch=4, buckets=(1, 2, 4), text=True), **kw)
    return ServingBatcher(pipe, H, W, executor=ex, **kw), ex


def test_construction_refusals(pipe):
    for bad, match in ((_pipe(encoder=None), "CLIPTextModel"), (_pipe(encoder=fake_text_encoder()), "CLIPTextModel"),
                       (_pipe(encoder=HostClip(CLIP).eval()), "fp16"), (_pipe(ctx=128), "hidden_size 64.*cross_attention_dim 128"),
                       (_pipe(tokenizer=types.SimpleNamespace(bos_token_id=1, eos_token_id=2)), "tokenizer")):
        with pytest.raises(NotImplementedError, match=match):
            ServingBatcher(bad, H, W, executor=TextExec(), text=True)
        ServingBatcher(bad, H, W, executor=TextExec())                          # without the flag such a pipeline serves
    off_route = _pipe()
    off_route.text_encoder.route = False
    with pytest.raises(NotImplementedError, match="kernels"):
        off_route.serve(H, W, text=True)
    with pytest.raises(NotImplementedError, match="multiple of 77"):
        ServingBatcher(pipe, H, W, executor=TextExec(), text=True, text_len=80)
    with pytest.raises(NotImplementedError, match="clip_skip"):
        ServingBatcher(pipe, H, W, executor=TextExec(), text=True, clip_skip=4)
    for bad in (0, 17, 2.0, True, None):
        with pytest.raises(ValueError, match="text_batch"):
            ServingBatcher(pipe, H, W, executor=TextExec(), text=True, text_batch=bad)
    plain = ServingBatcher(pipe, H, W, executor=TextExec())
    lane, _ = _batcher(pipe)
    assert set(lane.stats()) - set(plain.stats()) == {"text_encodes", "text_groups"} and not plain.text_on


@pytest.mark.parametrize("bad, match", [
    (dict(prompt_embeds=torch.zeros(1, 77, 64).half()), "`prompt` and `prompt_embeds`"),
    (dict(negative_prompt_embeds=torch.zeros(1, 77, 64).half()), "`prompt` and `negative_prompt_embeds`"),
    (dict(text_input_ids=[np.zeros((1, 77), np.int64)] * 2), "`prompt` and `text_input_ids`"),
    (dict(long_encode=1), "long_encode"), (dict(long_encode=2), "long_encode"), (dict(long_encode=True), "long_encode"),
    (dict(clip_skip=2), "clip_skip"), (dict(negative_prompt=["x"]), "one string each"), (dict(prompt=["a", "b"]), "one string each"),
    (dict(prompt=TWO), "2 chunks of 77 tokens.*text_len = 77")])
def test_submit_refusals(pipe, bad, match):
    b, ex = _batcher(pipe)
    with pytest.raises(ValueError, match=match):
        b.submit(_req("R", **dict(dict(prompt="a cat"), **bad)))
    assert b.stats()["queued"] == 0 and not ex.prepared
    fut = b.submit(_req("ok", prompt="a cat", long_encode=0, clip_skip=None, negative_prompt=None))       # the accepted forms
    b.submit(_req("ok2", prompt="a cat", long_encode=False, clip_skip=1))
    b.run_until_idle()
    assert fut.done()


def test_clip_skip_of_the_batcher_is_accepted(pipe):
    b, _ = _batcher(pipe, clip_skip=2)
    b.submit(_req("s", prompt="a cat", clip_skip=2))
    with pytest.raises(ValueError, match="clip_skip"):
        b.submit(_req("t", prompt="a cat", clip_skip=1))
    b.submit(_req("u", prompt="a cat"))                                # absent: the batcher's


def test_flagless_batcher_refuses_prompt_as_before(pipe):
    b = ServingBatcher(pipe, H, W, executor=TextExec())
    with pytest.raises(ValueError, match="a request needs prompt_embeds and negative_prompt_embeds"):
        b.submit(_req("P", prompt="a cat"))
    with pytest.raises(ValueError, match="text=True"):
        b.encode_text("a cat")
    with pytest.raises(TypeError):
        ServingBatcher(pipe, H, W, executor=TextExec(), txt=True)


# ----------------------------------------------------------------------------- queue logic
def test_groups_are_dispatched_fifo_and_the_head_waits(pipe):
    """E (embeddings) runs; A (two chunks) and B (one chunk) are queued behind it on a batcher of two chunks: encodes of 2 groups
    (A's) and 1 group (B's; its second chunk is empty in both rows and is no group), in that order; while A's event has not
    completed neither joins although slots are free, and E keeps stepping"""
    b, ex = _batcher(pipe, text_len=154, text_batch=2)
    fe = b.submit(_embeds("E", S=154, steps=8))
    assert b.step() and b.stats()["active"] == 1
    fa, fb = b.submit(_req("A", prompt=TWO)), b.submit(_req("B", prompt="a cat", negative_prompt="blurry"))
    assert not ex.encodes                                                       # submit queues nothing on the lane
    for _ in range(3):
        assert b.step()
        st = b.stats()
        assert st["active"] == 1 and st["queued"] == 2 and not ex.waits
    assert ex.encodes == [[("A", 0), ("A", 1)], [("B", 0)]]
    assert b.stats()["text_encodes"] == 2 and b.stats()["text_groups"] == 3 and b.stats()["steps"] == 4
    b._queue[1].txt.ev.done = True                                              # B's encode completes first: nobody overtakes A
    assert b.step() and b.stats()["active"] == 1
    b._queue[0].txt.ev.done = True
    assert b.step() and b.stats()["active"] == 3 and b.stats()["queued"] == 0
    assert [e[2] for e in ex.events if e[0] == "load"] == ["E", "A", "B"]
    b.run_until_idle()
    assert fe.done() and fa.done() and fb.done() and not ex.waits and b.stats()["text_encodes"] == 2


def test_idle_batcher_waits_for_the_head_and_requests_mix(pipe):
    b, ex = _batcher(pipe)
    fp = b.submit(_req("P", prompt="a (cat:1.2)"))
    fe = b.submit(_embeds("E"))
    assert b.step() is True and ex.waits == ["P"]
    assert b.stats()["active"] == 2                                             # both kinds in one batch
    b.run_until_idle()
    assert fp.done() and fe.done() and ex.encodes == [[("P", 0)]] and ex.prepared == [("txt2img", "P"), ("txt2img", "E")]


def test_prompt_makes_the_ids_of_the_region_encoder(pipe, monkeypatch):
    from diffusionspatialcontrol_amd.modules.serving import batcher as batcher_module
    seen = []
    monkeypatch.setattr(batcher_module, "encode_region_map", lambda pipe, state, **kw: seen.append((state, kw["text_ids"])))
    b, _ = _batcher(pipe, text_len=154)
    b.submit(_req("P", prompt="a red apple", negative_prompt="blurry", region_map_state={"k": 1}))
    (state, ids), = seen
    want = text_lane.prompt_chunks(b._parser, "blurry", "a red apple", 2, 154).np_ids
    assert state == {"k": 1} and len(ids) == 2 and all(np.array_equal(a, w) and a.shape == (1, 154) for a, w in zip(ids, want))


def test_encode_text_runs_the_lane_at_bucket_one(pipe):
    b, ex = _batcher(pipe, text_len=154, text_batch=2)
    out = b.encode_text(TWO, "blurry")
    assert ex.encodes == [[(None, 0)], [(None, 1)]] and ex.waits == [None]
    assert set(out) == {"prompt_embeds", "negative_prompt_embeds", "text_input_ids"} and out["text_input_ids"][1].shape == (1, 154)
    assert b.stats()["text_encodes"] == 2 and b.stats()["queued"] == 0


def test_hires_pair_shares_one_encode(pipe, monkeypatch):
    log = []
    base = ServingBatcher(pipe, 128, 128, max_batch=2, buckets=(1, 2), slot=0, executor=TextExec(name="base", events=log), text=True)
    hi = ServingBatcher(pipe, 192, 192, max_batch=2, buckets=(1, 2), slot=1, executor=TextExec(name="hires", events=log))
    pair = HiresPair(base, hi)
    fut = pair.submit(_req("H", prompt="a (cat:1.3)", upscale=True, upscale_x=1.5))
    first = base._queue[0]
    assert first.hires.text is first.text and first.text == ("text", "H") and first.hires.txt is None
    pair.run_until_idle()
    assert fut.done() and base.exec.encodes == [[("H", 0)]] and not hi.exec.encodes
    assert base.stats()["text_encodes"] == 1 and "text_encodes" not in hi.stats()
    with pytest.raises(ValueError, match="77 and 154 text keys"):
        HiresPair(ServingBatcher(pipe, 128, 128, slot=0, executor=TextExec(), text=True),
                  ServingBatcher(pipe, 192, 192, slot=1, executor=TextExec(), text_len=154))
    from diffusionspatialcontrol_amd.modules.serving import batcher as batcher_module
    monkeypatch.setattr(batcher_module, "_GraphExecutor", lambda b: TextExec())  # (no device in this test)
    built = pipe.serve_hires(128, 128, 1.5, max_batch=2, buckets=(1, 2), text=True, text_batch=1, clip_skip=2)
    assert built.base.text_on and built.base.text_batch == 1 and built.base.clip_skip == 2 and not built.hires.text_on
