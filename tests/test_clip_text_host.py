"""The native CLIP text encoder (modules/clip_text.py) on the CPU: the torch path against `transformers.CLIPTextModel` in fp64,
loading, the call surface, causality, the prompt encoders in front of it, and the argument checks of its two C entry points."""
import ctypes
import types

import pytest
import torch

import clip_text_ref as cr
import diffusionspatialcontrol_amd as dsc
from diffusionspatialcontrol_amd import build as dsc_build, ops
from diffusionspatialcontrol_amd.modules import encoder_prompt_modify as ep
from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel
from diffusionspatialcontrol_amd.modules.prompt_parser import FrozenCLIPEmbedderWithCustomWords


@pytest.fixture(scope="module", params=["quick_gelu", "gelu"])
def pair64(request):
    hf = cr.hf_model(cr.hf_config(request.param), seed=1)
    return hf, CLIPTextModel.from_transformers(hf)


@pytest.mark.parametrize("shape", [(2, 77), (3, 20)])
def test_fp64_parity_with_transformers(pair64, shape):
    """both sides evaluate the same fp64 formula: accumulated rounding is ~1e-14 of the values, the bound 1e-10 of the
    reference's max abs leaves four orders for the order of summation and catches any difference in the algorithm"""
    hf, native = pair64
    assert native.dtype == torch.float64
    ids = cr.ids_for(hf.config, *shape)
    r_last, r_hidden, r_pooled = cr.reference_outputs(hf, ids)
    out = native(ids, attention_mask=None, output_hidden_states=True)
    assert len(out.hidden_states) == hf.config.num_hidden_layers + 1
    for got, ref in [(out.last_hidden_state, r_last), (out.pooler_output, r_pooled), *zip(out.hidden_states, r_hidden)]:
        assert got.shape == ref.shape and got.dtype == torch.float64
        assert (got - ref).abs().max().item() <= 1e-10 * ref.abs().max().item()


def test_both_key_layouts_load_to_identical_outputs():
    hf = cr.hf_model(cr.hf_config(), seed=2, dtype=torch.float32)
    sd5 = hf.state_dict()
    assert "embeddings.token_embedding.weight" in sd5
    sd4 = {"text_model." + k: v for k, v in sd5.items()}
    sd4["text_model.embeddings.position_ids"] = torch.arange(77)[None]          # older checkpoints carry the buffer
    a, b = CLIPTextModel(hf.config), CLIPTextModel(hf.config)
    a.load_state_dict(sd5)
    b.load_state_dict(sd4)
    ids = cr.ids_for(hf.config, 2, 77)
    oa, ob = a(ids, output_hidden_states=True), b(ids, output_hidden_states=True)
    assert torch.equal(oa[0], ob[0]) and torch.equal(oa[1], ob[1])
    assert all(torch.equal(x, y) for x, y in zip(oa.hidden_states, ob.hidden_states))
    ref = cr.reference_outputs(hf, ids)[0]
    assert (oa[0] - ref).abs().max().item() < 1e-4 * ref.abs().max().item()     # and they are the weights, not the init
    missing = dict(sd5)
    del missing["encoder.layers.1.mlp.fc1.bias"]
    with pytest.raises(RuntimeError):
        CLIPTextModel(hf.config).load_state_dict(missing)
    with pytest.raises(RuntimeError):
        CLIPTextModel(hf.config).load_state_dict(dict(sd5, **{"text_model.encoder.layers.9.mlp.fc1.bias": torch.zeros(512)}))
    with pytest.raises(RuntimeError):                                           # one tensor under both layouts
        CLIPTextModel(hf.config).load_state_dict(dict(sd5, **{"text_model.final_layer_norm.bias": torch.zeros(128)}))


def test_from_transformers_round_trips_and_takes_dict_configs():
    hf = cr.hf_model(cr.hf_config("gelu"), seed=3, dtype=torch.float32)
    native = CLIPTextModel.from_transformers(hf)
    assert native.dtype == torch.float32 and native.device.type == "cpu"
    assert native.config.hidden_act == "gelu" and native.config.eos_token_id == 999
    back = type(hf)(hf.config).eval()
    back.load_state_dict(native.state_dict())                                   # the native keys ARE the transformers 5.x keys
    ids = cr.ids_for(hf.config, 2, 33)
    assert torch.equal(cr.reference_outputs(back, ids)[0], cr.reference_outputs(hf, ids)[0])
    cfg = dict(cr.TINY, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    assert CLIPTextModel(cfg).config.num_hidden_layers == 3
    with pytest.raises(ValueError):
        CLIPTextModel({k: v for k, v in cfg.items() if k != "eos_token_id"})
    with pytest.raises(ValueError):
        CLIPTextModel(dict(cfg, hidden_act="relu"))


def test_call_surface():
    hf = cr.hf_model(cr.hf_config(), seed=4, dtype=torch.float32)
    m = CLIPTextModel.from_transformers(hf)
    ids = cr.ids_for(hf.config, 2, 77)
    plain, full = m(ids), m(ids, attention_mask=None, output_hidden_states=True)
    assert plain.hidden_states is None and len(plain) == 2 and len(full) == 3
    assert plain[0] is plain.last_hidden_state and plain[1] is plain.pooler_output and plain[-1] is plain.pooler_output
    assert full[0] is full.last_hidden_state and full[1] is full.pooler_output and full[-1] is full.hidden_states
    assert isinstance(full[-1], tuple) and len(full[-1]) == 4 and full[-1][0].shape == (2, 77, 128)
    assert plain[0].shape == (2, 77, 128) and plain[1].shape == (2, 128)
    assert torch.equal(plain[0], full[0])
    assert torch.equal(m.final_layer_norm(full.hidden_states[-1]), full[0])     # hidden states are before the final LayerNorm
    assert m.text_model.final_layer_norm is m.final_layer_norm
    assert m.text_model.embeddings is m.embeddings and m.text_model.encoder is m.encoder
    assert ep.final_layer_norm_of(m) is m.final_layer_norm and ep.final_layer_norm_of(hf) is hf.final_layer_norm
    assert m.device == torch.device("cpu") and m.dtype == torch.float32 and m.config.hidden_size == 128
    assert m.half().dtype == torch.float16
    with pytest.raises(NotImplementedError):
        m(ids, attention_mask=torch.ones_like(ids))
    assert m.graph_captures == 0


def test_pooled_row_selection():
    cfg = cr.hf_config()
    hf = cr.hf_model(cfg, seed=5, dtype=torch.float32)
    m = CLIPTextModel.from_transformers(hf)
    for eos_at in (31, 76):
        ids = cr.ids_for(cfg, 2, 77, eos_at=eos_at)
        ids[1, 50] = cfg.eos_token_id                                           # a second EOS: the FIRST one counts
        out = m(ids)
        first = min(eos_at, 50)
        assert torch.equal(out.pooler_output[0], out.last_hidden_state[0, eos_at])
        assert torch.equal(out.pooler_output[1], out.last_hidden_state[1, first])
        ref = cr.reference_outputs(hf, ids)[2]
        assert (out.pooler_output - ref).abs().max().item() < 1e-4 * ref.abs().max().item()
    legacy = cr.hf_config(eos_token_id=2, bos_token_id=0)
    hf2 = cr.hf_model(legacy, seed=5, dtype=torch.float32)
    m2 = CLIPTextModel.from_transformers(hf2)
    ids = cr.ids_for(legacy, 2, 40, eos_at=39)
    ids[0, 17], ids[1, 5] = 999, 999                                            # the largest id of each row
    out = m2(ids)
    assert torch.equal(out.pooler_output[0], out.last_hidden_state[0, 17])
    assert torch.equal(out.pooler_output[1], out.last_hidden_state[1, 5])
    ref = cr.reference_outputs(hf2, ids)[2]
    assert (out.pooler_output - ref).abs().max().item() < 1e-4 * ref.abs().max().item()


def test_causality_bit_for_bit_fp32():
    m = CLIPTextModel.from_transformers(cr.hf_model(cr.hf_config(), seed=6, dtype=torch.float32))
    ids = cr.ids_for(m.config, 2, 77)
    base = m(ids, output_hidden_states=True)
    for p in (1, 10, 76):
        other = ids.clone()
        other[:, p] = (other[:, p] + 7) % 900 + 3
        out = m(other, output_hidden_states=True)
        for a, b in [(base[0], out[0]), *zip(base.hidden_states, out.hidden_states)]:
            assert torch.equal(a[:, :p], b[:, :p]), p
            assert not torch.equal(a[:, p], b[:, p]), p


@pytest.fixture(scope="module")
def wiring():
    """FakeHFClipTokenizer speaks CLIP's 49408-id vocabulary: a one-layer-deeper tiny encoder with that vocabulary, fp32"""
    from inputs import FakeHFClipTokenizer
    cfg = cr.hf_config(vocab_size=49408, eos_token_id=49407, bos_token_id=49406)
    hf = cr.hf_model(cfg, seed=7, dtype=torch.float32)
    native = CLIPTextModel.from_transformers(hf)
    pipe = lambda enc: types.SimpleNamespace(tokenizer=FakeHFClipTokenizer(), text_encoder=enc, device=torch.device("cpu"),  # noqa: E731
                                             unet=None)
    return pipe(hf), pipe(native)


def _close(a, b):
    return (a - b).abs().max().item() <= 1e-5 * (b.max() - b.min()).item()


def test_prompt_encoders_run_on_transformers_and_on_the_native_module(wiring):
    """clip_skip=2 reads the encoder's final LayerNorm: `text_model.final_layer_norm` does not exist on a transformers 5.x
    CLIPTextModel, so (a) raised AttributeError before final_layer_norm_of"""
    from inputs import prompt_encoder_cases
    pipe_hf, pipe_native = wiring
    neg, pos = prompt_encoder_cases()[0]
    with torch.no_grad():
        got = {}
        for name, pipe in (("hf", pipe_hf), ("native", pipe_native)):
            pe, ne, ids = ep.encode_short_prompt(pipe, pos, "cpu", 1, True, neg, clip_skip=2)
            text_input = pipe.tokenizer([neg, pos], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
            got[name] = (pe, ne, ep.clip_skip_prompt(pipe, text_input, clip_skip=2), ep.clip_skip_prompt(pipe, text_input), ids)
    assert got["hf"][0].shape == (1, 77, 128)
    for a, b in zip(got["native"][:4], got["hf"][:4]):
        assert a.shape == b.shape and _close(a, b)
    assert all((x == y).all() for x, y in zip(got["native"][4], got["hf"][4]))
    assert not _close(got["hf"][2], got["hf"][3])                               # clip skip is not a no-op


def test_a1111_parser_runs_on_both_encoders(wiring):
    from inputs import FakeClipTokenizer, prompt_encoder_cases
    pipe_hf, pipe_native = wiring
    neg, pos = prompt_encoder_cases()[2]                                        # the longest case: two chunks
    tok = FakeClipTokenizer()                                                   # the call surface this parser uses
    with torch.no_grad():
        ids_h, z_h = FrozenCLIPEmbedderWithCustomWords(tok, pipe_hf.text_encoder, 2)([neg, pos])
        ids_n, z_n = FrozenCLIPEmbedderWithCustomWords(tok, pipe_native.text_encoder, 2)([neg, pos])
    assert z_h.shape == z_n.shape and z_h.shape[1] % 77 == 0 and z_h.shape[1] >= 154
    assert (ids_h == ids_n).all() and _close(z_n, z_h)


def test_causal_attn_takes_truth_table():
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        for S in (0, 1, 80, 81):
            for d in (32, 64, 128):
                assert ops.causal_attn_takes(dtype, S, d) == (dtype == torch.float16 and S in (1, 80) and d == 64), (dtype, S, d)
    assert (ops.CAUSAL_ATTN_HEAD_DIM, ops.CAUSAL_ATTN_MAX_TOKENS) == (64, 80)
    header = open(dsc._lib.header_path()).read()
    assert "#define DSC_CAUSAL_ATTN_HEAD_DIM   64" in header and "#define DSC_CAUSAL_ATTN_MAX_TOKENS 80" in header


def test_entry_points_validate_before_any_launch():
    dsc_build.build(verbose=False)
    lib = dsc.load_library()
    s3 = (ctypes.c_int64 * 3)(77 * 3 * 128, 3 * 128, 64)
    dummy = ctypes.c_void_p(0x1000)
    call = lambda **kw: lib.dsc_causal_attn_f16(  # noqa: E731
        kw.get("q", dummy), kw.get("k", dummy), dummy, kw.get("out", dummy), kw.get("B", 2), kw.get("H", 2), kw.get("S", 77),
        kw.get("d", 64), kw.get("qs", s3), s3, s3, kw.get("os", s3), 0.0, kw.get("dtype", 0), None)
    assert call(q=None) == -1 and call(k=None) == -1 and call(out=None) == -1 and call(qs=None) == -1 and call(os=None) == -1
    assert call(B=0) == -1 and call(H=-1) == -1 and call(S=0) == -1 and call(d=0) == -1
    assert call(S=81) == -2 and call(S=4096) == -2
    assert call(d=32) == -2 and call(d=128) == -2
    assert call(dtype=1) == -2
    assert call(qs=(ctypes.c_int64 * 3)(77 * 384, 383, 64)) == -2               # an odd stride
    assert call(os=(ctypes.c_int64 * 3)(77 * 384, 384, 60)) == -2
    assert call(q=ctypes.c_void_p(0x1008)) == -2 and call(out=ctypes.c_void_p(0x1002)) == -2
    act = lambda x=dummy, n=1024, kind=0, dtype=0: lib.dsc_act_f16(x, n, kind, dtype, None)  # noqa: E731
    assert act(x=None) == -1 and act(n=0) == -1 and act(n=-8) == -1 and act(kind=2) == -1 and act(kind=-1) == -1
    assert act(n=1020) == -2 and act(dtype=3) == -2 and act(x=ctypes.c_void_p(0x1004)) == -2


def test_wrappers_refuse_cpu_tensors_and_bad_operands():
    q = torch.zeros(1, 4, 2, 64, dtype=torch.float16)
    with pytest.raises(dsc.DscLibraryError):
        ops.causal_attn(q, q, q)
    with pytest.raises(dsc.DscLibraryError):
        ops.act_(q, "gelu")


def test_fused_qkv_follows_the_parameters_and_parent_loads_rename_too():
    """the fused QKV copies are rebuilt after an in-place edit or a copy_ into a q / k / v parameter, and a parent module's
    load_state_dict (which never calls the encoder's own) renames the `text_model.` keys as well"""
    hf = cr.hf_model(cr.hf_config(), seed=8, dtype=torch.float32)
    m = CLIPTextModel.from_transformers(hf)
    ids = cr.ids_for(hf.config, 2, 33)
    base = m(ids)[0]
    saved = m.encoder.layers[0].self_attn.q_proj.weight.detach().clone()
    with torch.no_grad():
        m.encoder.layers[0].self_attn.q_proj.weight.mul_(0.5)
        hf.encoder.layers[0].self_attn.q_proj.weight.mul_(0.5)
    changed = m(ids)[0]
    ref = cr.reference_outputs(hf, ids)[0]
    assert not torch.equal(changed, base)
    assert (changed - ref).abs().max().item() < 1e-4 * ref.abs().max().item()

    class Parent(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.text_encoder = CLIPTextModel(hf.config)

    parent = Parent()
    parent.load_state_dict({"text_encoder.text_model." + k: v for k, v in hf.state_dict().items()})
    assert torch.equal(parent.text_encoder(ids)[0], changed)
    with pytest.raises(RuntimeError):
        Parent().load_state_dict({"text_encoder." + k: v for k, v in hf.state_dict().items() if "fc2.bias" not in k})
    with torch.no_grad():
        m.encoder.layers[0].self_attn.q_proj.weight.copy_(saved)
    assert torch.equal(m(ids)[0], base)
    m.encoder.layers[1].self_attn.v_proj.bias.data = torch.zeros(128)               # the parameter's tensor replaced
    assert not torch.equal(m(ids)[0], base)
