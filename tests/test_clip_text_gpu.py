"""The CLIP text encoder's kernels and module on the GPU: dsc_causal_attn_f16 (exact properties, accuracy against the device's
own fp16 SDPA), dsc_act_f16 over every finite fp16 value, the module against transformers, launch routing, the captured
encode and the prompt encoders in front of the native module.  Every figure is printed before it is asserted."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_text_ref as cr
from diffusionspatialcontrol_amd import _lib, ops
from diffusionspatialcontrol_amd.modules import clip_text as ct
from diffusionspatialcontrol_amd.modules import encoder_prompt_modify as ep
from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------- dsc_causal_attn_f16
def _qkv(B, S, H, seed, kind="normal", d=64):
    """fp16 q, k, v [B, S, H, d] on the CPU.  "activation": q and k carry one shared per-channel offset of magnitude 2.5 (+ for
    batch row 0, - on k for the others), so the logits sit near 64 * 2.5^2 / 8 = +-50 with a spread of ~10 and reach about +-60
    before the maximum is subtracted; v sits around 30."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, S, H, d, generator=g) for _ in range(3))
    if kind == "activation":
        o = 2.5 * (torch.randint(0, 2, (d,), generator=g) * 2 - 1).float()
        sign = torch.ones(B, 1, 1, 1)
        sign[1:] = -1.0
        q, k, v = q + o, k + sign * o, v + 30.0
    return q.half(), k.half(), v.half()


def _causal64(q, k, v, scale=None):
    """the fp64 restatement: softmax_{j <= i}(scale q_i . k_j) v_j over [B, S, H, d]"""
    S, d = q.shape[1], q.shape[-1]
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) * (d ** -0.5 if scale is None else scale)
    s = s + torch.full((S, S), float("-inf"), dtype=torch.float64).triu(1)
    return torch.einsum("bhij,bjhd->bihd", torch.softmax(s, dim=-1), v.double())


def _run(q, k, v, **kw):
    return ops.causal_attn(q.to(DEV), k.to(DEV), v.to(DEV), **kw).cpu()


def _ulp16(x):
    return 2.0 ** (math.floor(math.log2(x)) - 10)


def test_first_row_is_v_bit_for_bit():
    for S in (1, 17, 77):
        q, k, v = _qkv(2, S, 3, seed=S, kind="activation")
        out = _run(q, k, v)
        assert out.shape == (2, S, 3, 64) and out.dtype == torch.float16
        assert torch.equal(out[:, 0], v[:, 0])


def test_causality_is_exact():
    q, k, v = _qkv(2, 77, 3, seed=1)
    base = _run(q, k, v)
    for p in (1, 15, 16, 40, 76):
        k2, v2 = k.clone(), v.clone()
        k2[:, p] += 3.0
        v2[:, p] = -v2[:, p] + 7.0
        out = _run(q, k2, v2)
        assert torch.equal(out[:, :p], base[:, :p]), p
        assert not torch.equal(out[:, p], base[:, p]), p


def test_batch_rows_and_heads_are_independent():
    q, k, v = _qkv(3, 33, 3, seed=2)
    full = _run(q, k, v)
    for b in range(3):
        assert torch.equal(_run(q[b:b + 1], k[b:b + 1], v[b:b + 1])[0], full[b])
    for h in range(3):
        one = _run(q[:, :, h:h + 1].contiguous(), k[:, :, h:h + 1].contiguous(), v[:, :, h:h + 1].contiguous())
        assert torch.equal(one[:, :, 0], full[:, :, h])


def test_fused_views_and_strided_out():
    """the destination parameter is `into` (tests/test_output_paths.py keeps a closed table of the ops with an `out`); like those
    ops, causal_attn and act_ drop GroupNorm sums a producer attached to what they overwrite"""
    B, S, H, d = 2, 77, 3, 64
    C = H * d
    g = torch.Generator().manual_seed(3)
    fused = torch.randn(B, S, 3 * C, generator=g).half().to(DEV)
    qkv = fused.view(B, S, 3, H, d)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    assert not q.is_contiguous()
    ref = ops.causal_attn(q.contiguous(), k.contiguous(), v.contiguous())
    assert torch.equal(ops.causal_attn(q, k, v), ref)
    wide = torch.full((B, S, 2 * C + 8), 7.0, dtype=torch.float16, device=DEV)      # out rows 8 halfs in, C of 2 C + 8 wide
    view = wide[:, :, 8:8 + C].view(B, S, H, d)
    assert ops.causal_attn(q, k, v, into=view) is view
    assert torch.equal(view, ref)
    assert (wide[:, :, :8] == 7.0).all() and (wide[:, :, 8 + C:] == 7.0).all()
    with pytest.raises(ValueError):
        ops.causal_attn(q, k, v, into=torch.empty(B, S, H, 32, dtype=torch.float16, device=DEV))
    for dest, call in ((view, lambda: ops.causal_attn(q, k, v, into=view)), (fused, lambda: ops.act_(fused, "gelu"))):
        ops.attach_gn_partials(dest, ops.GnPartials(torch.zeros(1, device=DEV), 1, 1, 1, 1, 1))
        assert ops.gn_partials_of(dest) is not None
        call()
        assert ops.gn_partials_of(dest) is None
    with pytest.raises(_lib.DscLibraryError):                                        # 81 tokens: refused, no other route
        ops.causal_attn(*(torch.zeros(1, 81, 1, 64, dtype=torch.float16, device=DEV),) * 3)


@pytest.mark.parametrize("S", [1, 17, 77])
def test_nothing_behind_or_between_the_rows_is_read(S):
    """operands inside NaN-filled buffers: NaN rows after row S - 1 (the padded tile's rows) and NaN between the strided rows"""
    B, H, d = 2, 3, 64
    C = H * d
    q, k, v = _qkv(B, S, H, seed=4 + S, kind="activation")
    clean = _run(q, k, v)
    bufs = [torch.full((B, 96, 2 * C), float("nan"), dtype=torch.float16, device=DEV) for _ in range(3)]
    views = []
    for buf, t in zip(bufs, (q, k, v)):
        view = buf[:, :S, 8:8 + C].view(B, S, H, d)
        view.copy_(t.to(DEV))
        views.append(view)
    out = ops.causal_attn(*views).cpu()
    assert torch.isfinite(out).all()
    assert torch.equal(out, clean)


ACCURACY_S = (1, 15, 16, 17, 33, 77, 80)


@pytest.mark.parametrize("kind", ["normal", "activation"])
def test_accuracy_against_the_device_sdpa(kind):
    """max |kernel - fp64| <= 2 x max |fp16 SDPA - fp64| + one fp16 ulp of max |out|, per shape"""
    failures = []
    for S in ACCURACY_S:
        q, k, v = _qkv(2, S, 3, seed=10 + S, kind=kind)
        ref = _causal64(q, k, v)
        out = _run(q, k, v).double()
        qd, kd, vd = (t.to(DEV).transpose(1, 2) for t in (q, k, v))
        yard = F.scaled_dot_product_attention(qd, kd, vd, is_causal=True).transpose(1, 2).cpu().double()
        e_k, e_y = (out - ref).abs().max().item(), (yard - ref).abs().max().item()
        logit = (torch.einsum("bihd,bjhd->bhij", q.double(), k.double()) / 8).abs().max().item()
        bound = 2 * e_y + _ulp16(ref.abs().max().item())
        print(f"causal_attn {kind} S={S}: kernel {e_k:.3e}  sdpa {e_y:.3e}  bound {bound:.3e}  max|logit| {logit:.1f}")
        if not e_k <= bound:
            failures.append((S, e_k, e_y, bound))
    assert not failures, failures


# ----------------------------------------------------------------------------- dsc_act_f16
def _all_finite_fp16():
    x = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    x = x[torch.isfinite(x)]
    assert x.numel() == 63488
    return x


def _ordinal(h):
    """fp16 values as integers in value order (-0 and +0 coincide): differences are distances in ulps"""
    i = h.view(torch.int16).to(torch.int32)
    return torch.where(i >= 0, i, -(i & 0x7FFF))


def _round_once(x64):
    return torch.from_numpy(x64.numpy().astype(np.float16))          # numpy rounds fp64 -> fp16 once (torch goes through fp32)


def _exact(kind, x):
    x64 = x.double()
    if kind == "quick_gelu":
        return _round_once(x64 * torch.sigmoid(1.702 * x64))
    return _round_once(x64 * 0.5 * torch.special.erfc(-x64 * 2.0 ** -0.5))       # x Phi(x), without the 1 + erf cancellation


def _torch_fp32(kind, x32):
    return (x32 * torch.sigmoid(1.702 * x32) if kind == "quick_gelu" else F.gelu(x32)).half()


@pytest.mark.parametrize("kind", ["quick_gelu", "gelu"])
def test_act_over_every_finite_fp16_value(kind):
    """against the fp64 formula rounded once; yardstick: torch's own fp32 formula on the device, rounded to fp16.  The kernel may
    miss the exact value in at most 1 % more elements than the yardstick does, and by one ulp at the most."""
    x = _all_finite_fp16()
    exact = _exact(kind, x)
    got = ops.act_(x.to(DEV).clone(), kind).cpu()
    yard = _torch_fp32(kind, x.to(DEV).float()).cpu()
    d_k, d_y = (_ordinal(got) - _ordinal(exact)).abs(), (_ordinal(yard) - _ordinal(exact)).abs()
    miss_k, miss_y = int((d_k > 0).sum()), int((d_y > 0).sum())
    worst = x[d_k.argmax()].item()
    print(f"act_ {kind}: kernel off in {miss_k} of {x.numel()} (largest miss {int(d_k.max())} ulp, at x = {worst}); "
          f"torch fp32 off in {miss_y} (largest {int(d_y.max())} ulp)")
    assert torch.isfinite(got).all()
    assert int(d_k.max()) <= 1
    assert miss_k <= miss_y * 1.01


@pytest.mark.parametrize("kind", ["quick_gelu", "gelu"])
def test_act_nan_and_infinities(kind):
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1.0, -1.0, 65504.0], dtype=torch.float16)
    got = ops.act_(x.to(DEV).clone(), kind).cpu()
    want = _torch_fp32(kind, x.to(DEV).float()).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.isnan(got[0]) and got[1] == float("inf") and torch.isnan(got[2])
    assert torch.equal(got[3:], want[3:])
    with pytest.raises(_lib.DscLibraryError):
        ops.act_(torch.zeros(12, dtype=torch.float16, device=DEV), kind)             # not a multiple of 8
    with pytest.raises(ValueError):
        ops.act_(torch.zeros(8, dtype=torch.float16, device=DEV), "relu")


# ----------------------------------------------------------------------------- the module against transformers
_MODELS = {}


def _models(act="quick_gelu", **over):
    """(transformers fp64 on the CPU, native fp16 on the GPU, transformers fp16 eager on the GPU) - built once per config"""
    key = (act, tuple(sorted(over.items())))
    if key not in _MODELS:
        hf = cr.hf_model(cr.hf_config(act, **over), seed=21)
        native = CLIPTextModel.from_transformers(hf).half().to(DEV)
        _MODELS[key] = (hf, native, cr.fp16_eager_copy(hf, DEV))
    return _MODELS[key]


def _triple(out):
    return out.last_hidden_state, out.hidden_states, out.pooler_output


def _check_against_yardstick(hf, native, yard, ids, tag):
    ref = cr.reference_outputs(hf, ids)
    e_n = cr.max_abs_errors(_triple(native(ids.to(DEV), output_hidden_states=True)), ref)
    e_y = cr.max_abs_errors(cr.reference_outputs(yard, ids), ref)
    print(f"clip_text {tag}: [last, hidden 0..L, pooled]\n  native {['%.2e' % e for e in e_n]}\n  eager  {['%.2e' % e for e in e_y]}")
    assert e_n[1] == e_y[1] <= 2.0 ** -10                                         # the embeddings: a gather and one rounded add
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(e_n, e_y)) if not a <= 2 * b]
    assert not bad, bad


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("n", [2, 5])
def test_module_against_transformers(act, n):
    hf, native, yard = _models(act)
    assert native.kernel_route(n, 77)
    _check_against_yardstick(hf, native, yard, cr.ids_for(hf.config, n, 77, seed=n), f"tiny {act} [{n}, 77]")


class _CountingLib:
    """the loaded library with every dsc_* call recorded by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dsc_"):
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


PER_LAYER = ["dsc_add_layernorm", "dsc_linear_f16", "dsc_causal_attn_f16", "dsc_linear_f16", "dsc_add_layernorm",
             "dsc_linear_f16", "dsc_act_f16", "dsc_linear_f16"]


def test_clip_l_shape_against_transformers(monkeypatch):
    """CLIP-L's shape once: the errors as above, and the launches - 768 / 3072-wide GEMMs must stay on dsc_linear_f16"""
    hf, native, yard = _models(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12)
    assert native.kernel_route(2, 77)
    lib = _CountingLib(_lib.load_library())
    monkeypatch.setattr(_lib, "load_library", lambda: lib)
    _check_against_yardstick(hf, native, yard, cr.ids_for(hf.config, 2, 77, seed=9), "CLIP-L shape [2, 77]")
    assert lib.calls == PER_LAYER * 12 + ["dsc_add_layernorm"] and len(lib.calls) == 97


# ----------------------------------------------------------------------------- routing and capture
def test_launch_count_and_the_torch_route(monkeypatch):
    hf, native, yard = _models()
    L = hf.config.num_hidden_layers
    ids = cr.ids_for(hf.config, 2, 77, seed=3).to(DEV)
    lib = _CountingLib(_lib.load_library())
    monkeypatch.setattr(_lib, "load_library", lambda: lib)
    kernel = native(ids, output_hidden_states=True)
    assert len(lib.calls) == 8 * L + 1, lib.calls
    assert lib.calls == PER_LAYER * L + ["dsc_add_layernorm"]
    lib.calls.clear()
    monkeypatch.setattr(ct, "USE_CLIP_TEXT_KERNELS", False)                       # what DSC_CLIP_TEXT=0 sets at import
    assert not native.kernel_route(2, 77)
    plain = native(ids, output_hidden_states=True)
    assert lib.calls == []
    # the tolerance of the module test: 2 x the error of the transformers fp16 eager model against the fp64 result, per entry -
    # for the difference between the two routes, and for the torch route's own error against fp64
    ref = cr.reference_outputs(hf, ids.cpu())
    e_y = cr.max_abs_errors(cr.reference_outputs(yard, ids), ref)
    diff = cr.max_abs_errors(_triple(plain), _triple(kernel))
    e_t = cr.max_abs_errors(_triple(plain), ref)
    print(f"clip_text routes: |torch route - kernel route| {['%.2e' % e for e in diff]}\n  torch route - fp64 {['%.2e' % e for e in e_t]}"
          f"\n  eager yardstick {['%.2e' % e for e in e_y]}")
    assert all(a <= 2 * b for a, b in zip(diff, e_y)), (diff, e_y)
    assert all(a <= 2 * b for a, b in zip(e_t, e_y)), (e_t, e_y)
    for S, why in ((81, "tokens"),):
        assert not native.kernel_route(2, S), why


def test_captured_encode():
    hf = cr.hf_model(cr.hf_config(), seed=22)
    m = CLIPTextModel.from_transformers(hf).half().to(DEV)
    ids_a, ids_b = (cr.ids_for(hf.config, 2, 77, seed=s).to(DEV) for s in (5, 6))
    eager_a, eager_b = m(ids_a, output_hidden_states=True), m(ids_b, output_hidden_states=True)
    assert m.graph_captures == 0
    assert m.enable_graphs(True) is m
    got_a = m(ids_a, output_hidden_states=True)
    assert m.graph_captures == 1
    got_b = m(ids_b, output_hidden_states=True)                                   # same shape, new ids: a replay
    assert m.graph_captures == 1
    for got, eager in ((got_a, eager_a), (got_b, eager_b)):                       # got_a was returned before the second call
        assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])
        assert len(got.hidden_states) == len(eager.hidden_states)
        assert all(torch.equal(x, y) for x, y in zip(got.hidden_states, eager.hidden_states))
    assert not torch.equal(got_a[0], got_b[0])
    ids_c = cr.ids_for(hf.config, 5, 77, seed=7).to(DEV)
    got_c = m(ids_c, output_hidden_states=True)
    assert m.graph_captures == 2
    m.enable_graphs(False)
    assert torch.equal(got_c[0], m(ids_c)[0]) and m.graph_captures == 2
    m.enable_graphs(True)
    plain = m(ids_a)                                                              # no hidden states: its own graph
    assert m.graph_captures == 3 and plain.hidden_states is None and torch.equal(plain[0], eager_a[0])
    assert torch.equal(plain[-1], eager_a[1])
    with torch.no_grad():                                                         # an in-place edit: fused copies and graphs follow
        m.encoder.layers[0].self_attn.k_proj.weight.mul_(0.5)
    edited = m(ids_a)
    assert m.graph_captures == 4 and not torch.equal(edited[0], eager_a[0])
    m.enable_graphs(False)
    assert torch.equal(m(ids_a)[0], edited[0])
    torch.cuda.synchronize()


def test_prompt_encoders_on_the_native_module():
    """encode_prompt_function's three branches on a pipeline namespace with the native encoder on the GPU, against the same call
    on the native module in fp32 on the CPU; yardstick: the same call on the transformers fp16 eager model"""
    from inputs import FakeClipTokenizer, FakeHFClipTokenizer, prompt_encoder_cases
    hf, native, yard = _models(vocab_size=49408, eos_token_id=49407, bos_token_id=49406)
    cpu32 = CLIPTextModel.from_transformers(hf).float()
    neg, pos = prompt_encoder_cases()[2]                                          # its longest case is two 77-token chunks:
    pos = pos + ", " + ", ".join(f"(thing{i}:1.2) with detail" for i in range(8))   # eight more weighted items make it three
    runs = []
    for long_encode, tok, skip in ((2, FakeHFClipTokenizer, None), (2, FakeHFClipTokenizer, 2), (1, FakeHFClipTokenizer, 2),
                                   (0, FakeClipTokenizer, 2)):
        outs = {}
        for name, enc, dev in (("ref", cpu32, "cpu"), ("native", native, DEV), ("yard", yard, DEV)):
            pipe = types.SimpleNamespace(tokenizer=tok(), text_encoder=enc, device=torch.device(dev), unet=None)
            with torch.no_grad():
                pe, ne, ids = ep.encode_prompt_function(pipe, pos, dev, 1, True, neg, clip_skip=skip, long_encode=long_encode)
            outs[name] = (pe, ne, ids)
        assert outs["native"][0].dtype == torch.float16 and outs["native"][0].is_cuda
        assert outs["native"][0].shape == outs["ref"][0].shape and outs["native"][0].shape[1] == (77 if long_encode == 2 else 231)
        assert all(np.array_equal(a, b) for a, b in zip(outs["native"][2], outs["ref"][2]))
        for i in (0, 1):
            ref = outs["ref"][i].double()
            e_n = (outs["native"][i].double().cpu() - ref).abs().max().item()
            e_y = (outs["yard"][i].double().cpu() - ref).abs().max().item()
            print(f"encode_prompt_function long_encode={long_encode} clip_skip={skip} [{('pos', 'neg')[i]}]: native {e_n:.2e}  eager {e_y:.2e}")
            runs.append((long_encode, skip, i, e_n, e_y))
    bad = [r for r in runs if not r[3] <= 2 * r[4]]
    assert not bad, bad
