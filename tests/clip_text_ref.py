"""Shared pieces of the CLIP text encoder tests: the reference network is `transformers.CLIPTextModel` with random weights from
a fixed seed (no checkpoint), scaled so that the attention scores are not flat and every LayerNorm has a real affine."""
import torch

TINY = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, eos_token_id=999)


def hf_config(hidden_act="quick_gelu", attn=None, **over):
    """the tiny config of the tests.  Attention implementation: the library's default for the fp64 reference (its "eager" one
    computes the softmax in fp32 whatever the model's dtype); the fp16 yardstick asks for "eager" when it copies the model"""
    from transformers import CLIPTextConfig
    kw = dict(TINY, max_position_embeddings=77, hidden_act=hidden_act, layer_norm_eps=1e-5)
    kw.update(over)
    kw.setdefault("bos_token_id", kw["eos_token_id"] - 1 if kw["eos_token_id"] > 2 else 0)
    kw.setdefault("pad_token_id", 1)
    return CLIPTextConfig(**kw) if attn is None else CLIPTextConfig(attn_implementation=attn, **kw)


def hf_model(config, seed=0, dtype=torch.float64):
    """the transformers model with seeded weights: unit-variance projections (q / k twice that, so the logits have a standard
    deviation of about 4), biases and LayerNorm affines away from their trivial values.  Every value is an fp16 number, so an fp16
    copy of the model has the reference's weights exactly and the errors the GPU tests compare are errors of the arithmetic"""
    from transformers import CLIPTextModel
    model = CLIPTextModel(config).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            r = torch.randn(p.shape, generator=g, dtype=torch.float64)
            if "token_embedding" in name:
                r = r * 0.5
            elif "position_embedding" in name:
                r = r * 0.1
            elif "layer_norm" in name:
                r = (1.0 + 0.1 * r) if name.endswith("weight") else 0.1 * r
            elif name.endswith("bias"):
                r = r * 0.1
            else:
                r = r * p.shape[1] ** -0.5 * (2.0 if ("q_proj" in name or "k_proj" in name) else 1.0)
            p.copy_(r.half().to(p.dtype))
    return model.to(dtype)


def ids_for(config, n, S, seed=0, eos_at=None):
    """[n, S] ids below the special tokens, the EOS token at `eos_at` (default: a different position in every row)"""
    g = torch.Generator().manual_seed(100 + seed)
    eos = config.eos_token_id
    ids = torch.randint(3, min(config.vocab_size, 40000) - 2, (n, S), generator=g)
    for b in range(n):
        ids[b, (S - 1 - 3 * b) % S if eos_at is None else eos_at] = eos
    return ids


def reference_outputs(model, ids):
    """(last_hidden_state, hidden_states tuple, pooler_output) of the transformers model"""
    with torch.no_grad():
        out = model(ids.to(model.device), attention_mask=None, output_hidden_states=True)
    return out.last_hidden_state, tuple(out.hidden_states), out.pooler_output


def max_abs_errors(got, ref64):
    """[last, hidden_0 .. hidden_L, pooled] max abs differences of a (last, hidden, pooled) triple to the fp64 reference's"""
    last, hidden, pooled = got
    r_last, r_hidden, r_pooled = ref64
    assert len(hidden) == len(r_hidden)
    diff = lambda a, b: (a.detach().double().cpu() - b.double().cpu()).abs().max().item()  # noqa: E731
    return [diff(last, r_last)] + [diff(a, b) for a, b in zip(hidden, r_hidden)] + [diff(pooled, r_pooled)]


def fp16_eager_copy(model, device):
    """the yardstick of the GPU tests: the same transformers model as .half() on `device` with the "eager" attention implementation"""
    cfg = model.config.to_dict()
    keep = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "eos_token_id",
            "bos_token_id", "pad_token_id", "max_position_embeddings", "layer_norm_eps")
    twin = type(model)(hf_config(cfg["hidden_act"], attn="eager", **{k: cfg[k] for k in keep})).eval()
    twin.load_state_dict(model.state_dict())
    return twin.half().to(device)
