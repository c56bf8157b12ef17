"""CLIP text encoder on the package's kernels - the `transformers.CLIPTextModel` the reference loads as `pipe.text_encoder`
and calls from `source/modules/encoder_prompt_modify.py` (:186-210, :540-650) and `source/modules/prompt_parser.py` (:267-279).

The network (pre-LN transformer, causal attention, quick-GELU or erf-GELU MLP, final LayerNorm, pooled row at the EOS token):
    h_0 = token_embedding[ids] + position_embedding[:S]
    a   = LN1(h);  h = h + out_proj(causal_attn(q_proj a, k_proj a, v_proj a))
    m   = LN2(h);  h = h + fc2(act(fc1 m))
    last_hidden_state = final_layer_norm(h_L);  pooler_output = last_hidden_state[b, first position of eos_token_id]

GPU fp16 path (`kernel_route`): eight package launches per layer - dsc_add_layernorm, dsc_linear_f16 over the fused [3C, C] QKV
weight, dsc_causal_attn_f16 on three strided views of its output, dsc_linear_f16 (out_proj + residual), dsc_add_layernorm,
dsc_linear_f16 (fc1), dsc_act_f16 in place, dsc_linear_f16 (fc2 + residual) - and one more for the final LayerNorm.  The embedding
gather, the position add and the pooled-row gather are torch indexing; no torch op touches the activation stream in between.
Residual-stream tensors are never overwritten: `hidden_states` hands them out.

Every other case (CPU, fp32 / fp64, shapes the kernels do not take, DSC_CLIP_TEXT=0) is the same algorithm written out in torch in
the module's dtype, with a -inf upper-triangular mask.

`enable_graphs(True)` makes a GPU call replay one captured graph per (n, S, output_hidden_states): single stream, no parallel
branches, a static ids buffer in, clones out.

Not here: padding masks (`attention_mask` must be None - no caller passes one), the projection head of
CLIPTextModelWithProjection, a tokenizer, textual inversion.  LoRA on the encoder is modules/lora.py's: merged weights, which the
fused QKV copies follow through the version counter."""
import os

import torch
from torch import nn
from torch.nn import functional as F

from .. import ops

USE_CLIP_TEXT_KERNELS = os.environ.get("DSC_CLIP_TEXT", "1") != "0"   # A/B switch: 0 = the torch algorithm everywhere

_CONFIG_FIELDS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                  "max_position_embeddings", "hidden_act", "layer_norm_eps", "eos_token_id")


class CLIPTextConfig:
    """the nine fields the encoder reads, copied from any object or dict that carries them"""

    def __init__(self, source):
        for name in _CONFIG_FIELDS:
            if isinstance(source, dict):
                if name not in source:
                    raise ValueError(f"CLIPTextModel config lacks {name!r}")
                value = source[name]
            else:
                if not hasattr(source, name):
                    raise ValueError(f"CLIPTextModel config lacks {name!r}")
                value = getattr(source, name)
            setattr(self, name, value)
        if self.hidden_act not in ops.ACT_KINDS:
            raise ValueError(f"hidden_act must be one of {sorted(ops.ACT_KINDS)}, got {self.hidden_act!r}")
        if self.hidden_size % self.num_attention_heads != 0:
            raise ValueError("hidden_size must be a multiple of num_attention_heads")


class CLIPTextOutput:
    """what the callers index: [0] / .last_hidden_state, [1] / .pooler_output, [-1] = .hidden_states when they were requested
    (a tuple of num_hidden_layers + 1 tensors, before the final LayerNorm), else the pooled output - as transformers' ModelOutput"""

    def __init__(self, last_hidden_state, pooler_output, hidden_states=None):
        self.last_hidden_state, self.pooler_output, self.hidden_states = last_hidden_state, pooler_output, hidden_states

    def to_tuple(self):
        t = (self.last_hidden_state, self.pooler_output)
        return t if self.hidden_states is None else t + (self.hidden_states,)

    def __getitem__(self, i):
        return self.to_tuple()[i]

    def __len__(self):
        return len(self.to_tuple())

    def __iter__(self):
        return iter(self.to_tuple())


def _kernel_tensor(x):
    return USE_CLIP_TEXT_KERNELS and x.is_cuda and x.dtype == torch.float16


class _LayerNorm(nn.LayerNorm):
    """nn.LayerNorm that runs on dsc_add_layernorm for the fp16 GPU tensors the clip-skip callers hand to `final_layer_norm`"""

    def forward(self, x):
        if _kernel_tensor(x) and self.weight.dtype == torch.float16 and x.shape[-1] % 8 == 0:
            return ops.add_layernorm(x, None, self.weight, self.bias, self.eps)[1]
        return super().forward(x)


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embedding = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)

    def forward(self, ids):
        S = ids.shape[-1]
        if S > self.position_embedding.weight.shape[0]:
            raise ValueError(f"{S} tokens, but max_position_embeddings is {self.position_embedding.weight.shape[0]}")
        return self.token_embedding(ids) + self.position_embedding.weight[:S]


class _Attention(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(C, C) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, C, inner):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, inner), nn.Linear(inner, C)


class _Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        C = cfg.hidden_size
        self.self_attn = _Attention(C)
        self.layer_norm1 = nn.LayerNorm(C, eps=cfg.layer_norm_eps)
        self.mlp = _MLP(C, cfg.intermediate_size)
        self.layer_norm2 = nn.LayerNorm(C, eps=cfg.layer_norm_eps)
        self.qkv_weight = self.qkv_bias = None         # [3C, C] / [3C]: the fused copies (refresh_qkv), not part of the state
        self._qkv_signature = None

    def refresh_qkv(self):
        """(re)build the fused QKV weight and bias when a q / k / v parameter is another tensor than at the last build or has been
        written in place since (identity, address, dtype and torch's version counter) -> True when they were rebuilt"""
        a = self.self_attn
        ps = (a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.q_proj.bias, a.k_proj.bias, a.v_proj.bias)
        signature = tuple((id(p), p.data_ptr(), p.dtype, p._version) for p in ps)
        if signature == self._qkv_signature:
            return False
        with torch.no_grad():
            self.qkv_weight, self.qkv_bias = torch.cat(ps[:3]).contiguous(), torch.cat(ps[3:]).contiguous()
        self._qkv_signature = signature
        return True


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList(_Layer(cfg) for _ in range(cfg.num_hidden_layers))


class _TextModelView:
    """`model.text_model` of the transformers 4.x / diffusers layout: the same three submodules under their old owner"""

    def __init__(self, model):
        self.embeddings, self.encoder, self.final_layer_norm = model.embeddings, model.encoder, model.final_layer_norm


def _act(x, kind):
    return x * torch.sigmoid(1.702 * x) if kind == "quick_gelu" else F.gelu(x)


def _rename_text_model_keys(module, state_dict, prefix, *_):
    """load_state_dict pre-hook (also when the encoder is loaded as part of a parent module): `<prefix>text_model.X` -> `<prefix>X`,
    and the `position_ids` buffer of older checkpoints (an arange) dropped.  `state_dict` is nn.Module's own copy."""
    old = prefix + "text_model."
    for key in [k for k in state_dict if k.startswith(old)]:
        name = prefix + key[len(old):]
        if name in state_dict:
            raise RuntimeError(f"state dict holds {name!r} under both key layouts")
        state_dict[name] = state_dict.pop(key)
    state_dict.pop(prefix + "embeddings.position_ids", None)


class CLIPTextModel(nn.Module):
    """`CLIPTextModel(config)`; weights through `load_state_dict` - both key layouts of the same tensors load:
    `text_model.embeddings.token_embedding.weight` (diffusers / SD checkpoints, transformers 4.x) and
    `embeddings.token_embedding.weight` (transformers 5.x); missing and unexpected keys raise as in any strict load - or through
    `CLIPTextModel.from_transformers(hf_model)`.

    Inference only: `forward` runs under `torch.no_grad()` on every path (the kernels have no backward), so no gradient ever
    flows through this module - training the encoder or textual inversion needs another implementation.

    The fused QKV weights are copies: every call compares the q / k / v parameters with what the copies were built from (tensor
    identity, address, dtype, version counter) and rebuilds them - and drops the captured graphs - after a load, a `.to()`, an
    in-place edit or `copy_`.  A captured graph reads every other parameter in place: in-place edits are seen by the next replay;
    a parameter that was REPLACED by another tensor outside `load_state_dict` / `.to()` needs `enable_graphs(False)` first."""

    def __init__(self, config):
        super().__init__()
        self.config = config if isinstance(config, CLIPTextConfig) else CLIPTextConfig(config)
        cfg = self.config
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.final_layer_norm = _LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.graph_captures = 0
        self._graphs_on = False
        self._graphs = {}
        self.register_load_state_dict_pre_hook(_rename_text_model_keys)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._drop_graphs())
        self._refresh_qkv()                             # built at construction and again right after a load (first use at the latest)

    # ------------------------------------------------------------------------------------------- construction and loading
    @classmethod
    def from_transformers(cls, hf_model):
        """a module with the config and the weights of a transformers CLIPTextModel (either generation), in its dtype and device"""
        model = cls(hf_model.config)
        model.load_state_dict(hf_model.state_dict())
        p = next(hf_model.parameters())
        return model.to(device=p.device, dtype=p.dtype).eval()

    def _drop_graphs(self):
        self._graphs = {}                               # captured graphs read the old tensors' addresses
        self._refresh_qkv()

    def _refresh_qkv(self):
        rebuilt = [layer.refresh_qkv() for layer in self.encoder.layers]
        if any(rebuilt):
            self._graphs = {}

    def _apply(self, fn, *args, **kwargs):              # .to() / .half() / .cuda(): every parameter is another tensor now
        result = super()._apply(fn, *args, **kwargs)
        self._drop_graphs()
        return result

    # ------------------------------------------------------------------------------------------- surface
    @property
    def text_model(self):
        return _TextModelView(self)

    @property
    def device(self):
        return self.final_layer_norm.weight.device

    @property
    def dtype(self):
        return self.final_layer_norm.weight.dtype

    def enable_graphs(self, on=True):
        """GPU calls replay one captured graph per (n, S, output_hidden_states) (honours ops.GRAPHS_ENABLED); off drops them"""
        self._graphs_on = bool(on)
        if not on:
            self._graphs = {}
        return self

    def kernel_route(self, n, S):
        """True when a call with ids [n, S] runs on the package's kernels"""
        cfg = self.config
        return (USE_CLIP_TEXT_KERNELS and self.device.type == "cuda" and n >= 1
                and ops.causal_attn_takes(self.dtype, S, cfg.hidden_size // cfg.num_attention_heads)
                and cfg.hidden_size % 64 == 0 and cfg.intermediate_size % 64 == 0)

    # ------------------------------------------------------------------------------------------- forward
    def forward(self, input_ids, attention_mask=None, output_hidden_states=False):
        if attention_mask is not None:
            raise NotImplementedError("CLIPTextModel: padding masks are not built (every caller passes attention_mask=None)")
        ids = input_ids.reshape(-1, input_ids.shape[-1]).to(self.device)
        n, S = ids.shape
        want_hidden = bool(output_hidden_states)
        self._refresh_qkv()
        with torch.no_grad():
            if not self.kernel_route(n, S):
                last, hidden = self._forward_torch(ids)
            elif self._graphs_on and ops.GRAPHS_ENABLED:
                last, hidden = self._forward_graph(ids, want_hidden)
            else:
                last, hidden = self._forward_kernels(ids)
            pooled = last[torch.arange(n, device=last.device), self._eos_positions(ids)]
        return CLIPTextOutput(last, pooled, tuple(hidden) if want_hidden else None)

    def _eos_positions(self, ids):
        """the pooled row: the first eos_token_id of each row; with the legacy eos_token_id == 2, the row's largest id"""
        eos = self.config.eos_token_id
        if eos == 2:
            return ids.to(torch.int).argmax(dim=-1)
        return (ids.to(torch.int) == eos).int().argmax(dim=-1)

    def _forward_torch(self, ids):
        cfg = self.config
        H = cfg.num_attention_heads
        h = self.embeddings(ids)
        n, S, C = h.shape
        d = C // H
        mask = torch.full((S, S), float("-inf"), dtype=h.dtype, device=h.device).triu(1)
        hidden = [h]
        for layer in self.encoder.layers:
            a = layer.layer_norm1(h)
            q, k, v = F.linear(a, layer.qkv_weight, layer.qkv_bias).view(n, S, 3, H, d).permute(2, 0, 3, 1, 4)
            p = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, dim=-1)
            h = h + layer.self_attn.out_proj((p @ v).transpose(1, 2).reshape(n, S, C))
            h = h + layer.mlp.fc2(_act(layer.mlp.fc1(layer.layer_norm2(h)), cfg.hidden_act))
            hidden.append(h)
        return self.final_layer_norm(h), hidden

    def _layer_kernels(self, layer, h):
        """one encoder layer on the residual stream h [n, S, C] -> the new stream (a new tensor): eight launches"""
        n, S, C = h.shape
        H = self.config.num_attention_heads
        ln1, ln2, att, mlp = layer.layer_norm1, layer.layer_norm2, layer.self_attn, layer.mlp
        _, a = ops.add_layernorm(h, None, ln1.weight, ln1.bias, ln1.eps)
        qkv = ops.linear(a, layer.qkv_weight, layer.qkv_bias, prefer_kernel=True).view(n, S, 3, H, C // H)
        o = ops.causal_attn(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]).view(n, S, C)
        h = ops.linear(o, att.out_proj.weight, att.out_proj.bias, residual=h, prefer_kernel=True)
        _, m = ops.add_layernorm(h, None, ln2.weight, ln2.bias, ln2.eps)
        f = ops.act_(ops.linear(m, mlp.fc1.weight, mlp.fc1.bias, prefer_kernel=True), self.config.hidden_act)
        return ops.linear(f, mlp.fc2.weight, mlp.fc2.bias, residual=h, prefer_kernel=True)

    def _forward_kernels(self, ids):
        h = self.embeddings(ids)
        hidden = [h]
        for layer in self.encoder.layers:
            h = self._layer_kernels(layer, h)
            hidden.append(h)
        fin = self.final_layer_norm
        return ops.add_layernorm(h, None, fin.weight, fin.bias, fin.eps)[1], hidden

    def encode_rows(self, ids, clip_skip=None):
        """What the emphasis parser reads of a call (prompt_parser.py `encode_with_transformers`), for a caller that captures the
        encoder into a graph of its own (modules/serving/text_lane.py): ids [n, S] int64 on the GPU -> fp16 [n, S, C], the last
        hidden state or, with clip_skip > 1, the final LayerNorm of hidden_states[-clip_skip] (the layers behind it do not run).
        Kernel route only, always eager launches on the current stream whatever `enable_graphs` says, no clones: the same launches
        and bits as `forward` on these ids."""
        n, S = ids.shape
        layers = self.encoder.layers
        skip = clip_skip if clip_skip is not None and clip_skip > 1 else 1
        if not self.kernel_route(n, S) or ids.device != self.device:
            raise NotImplementedError(f"CLIPTextModel.encode_rows: [{n}, {S}] ids on {ids.device} do not run on the package's kernels")
        if skip > len(layers) + 1:
            raise ValueError(f"CLIPTextModel.encode_rows: clip_skip {clip_skip} reaches behind {len(layers)} layers")
        self._refresh_qkv()
        with torch.no_grad():
            h = self.embeddings(ids)
            for layer in layers[:len(layers) + 1 - skip]:
                h = self._layer_kernels(layer, h)
            fin = self.final_layer_norm
            return ops.add_layernorm(h, None, fin.weight, fin.bias, fin.eps)[1]

    def _forward_graph(self, ids, want_hidden):
        key = (ids.shape[0], ids.shape[1], want_hidden)
        entry = self._graphs.get(key)
        if entry is None:
            static_ids = ids.clone()
            side = torch.cuda.Stream(device=ids.device)          # warm-up off the capturing stream, as torch's recipe asks
            side.wait_stream(torch.cuda.current_stream(ids.device))
            with torch.cuda.stream(side):
                self._forward_kernels(static_ids)
            torch.cuda.current_stream(ids.device).wait_stream(side)
            from .model_k_diffusion import _capture_without_gc
            graph = torch.cuda.CUDAGraph()
            with _capture_without_gc(), torch.cuda.graph(graph):  # one stream, no parallel branches
                last, hidden = self._forward_kernels(static_ids)
            entry = self._graphs[key] = (graph, static_ids, last, hidden if want_hidden else [])
            self.graph_captures += 1
        graph, static_ids, last, hidden = entry
        static_ids.copy_(ids)
        graph.replay()
        return last.clone(), [t.clone() for t in hidden]
