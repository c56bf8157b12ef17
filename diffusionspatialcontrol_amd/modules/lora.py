"""LoRA adapters merged into the UNet and the text encoder - what the reference does in `load_lora_control_pipeline`
(app.py:532-597) for the `lora_state` / `lora_scale` of a generation: every `lora_unet_<path>` / `lora_te_<path>` pair of a
kohya-format file is multiplied out and added to the weight it names, `W += lora_scale * up @ down`.

Here the merge always starts from a pristine copy of the weight (un-merging by subtraction in fp16 does not give the base weights
back): the first load clones every touched weight, and every change - a load, `set_lora_scale`, an unload - recomputes ALL
touched weights from their bases.  fp16 GPU weights inside the kernel's limits (ops.lora_merge_takes) go through one
dsc_lora_merge_f16 launch over the whole table; every other weight (CPU, fp32 / fp64, rows that are no multiple of 8 halfs,
DSC_LORA=0) through ops.lora_merge_eager, the reference's fp32 statements.  On the kernel route fp32 LoRA tensors are rounded to
fp16 (the reference multiplies them in fp32; files are fp16 in practice); the eager route keeps them as they are.

Keys: `lora_unet_<path>.lora_down.weight`, `.lora_up.weight` and `.alpha`, `<path>` a module name of the UNet with "." written
"_" (the UNet's module names are the diffusers ones); `lora_te_text_model_<path>...` likewise for the text encoder - for this
package's CLIPTextModel with `text_model_` stripped, for a transformers encoder with or without it.  `.alpha` is skipped unless
`use_alpha=True` (the reference skips it and applies `lora_scale` alone); then the gain is `scale * alpha / rank`.  Nothing is
merged partially: every key is resolved and checked before a weight is touched, and a ValueError names the key at fault.

Not here: LoCon 3x3, LoHa and DoRA weights, diffusers / PEFT key formats, LoRA on ControlNets or adapters, the FaceID LoRAs,
textual inversion, pickle files (safetensors and state dicts only)."""
import collections
import os

import torch
from torch import nn

from .. import ops

UNET_PREFIX = "lora_unet_"
TE_PREFIX = "lora_te_"
_SUFFIXES = ("lora_down.weight", "lora_up.weight", "alpha")

Layer = collections.namedtuple("Layer", "key module up down alpha rank")


def read_state_dict(source):
    """a state dict as it is, or the tensors of a .safetensors file (on the CPU); pickle formats are refused"""
    if isinstance(source, dict):
        return source
    path = os.fspath(source)
    if not path.endswith(".safetensors"):
        raise ValueError(f"load_lora_weights: {path!r} is not a .safetensors file (pickle files are not read)")
    from safetensors.torch import load_file
    return load_file(path)


def _names(model, strip=""):
    """{module name with "." as "_": module}; names that start with `strip` also without it"""
    out = {}
    for name, module in model.named_modules():
        flat = name.replace(".", "_")
        out[flat] = module
        if strip and flat.startswith(strip):
            out.setdefault(flat[len(strip):], module)
    return out


def _is_1x1(shape):
    return len(shape) == 4 and tuple(shape[2:]) == (1, 1)


def resolve(state_dict, unet, text_encoder=None):
    """[Layer(key, module, up [N, r], down [r, K], alpha | None, rank)] for every pair of the file, or ValueError naming the key:
    an unknown target, a `lora_up` / `lora_down` without its pair, a 3x3 (LoCon) down weight, rank or shape mismatches, a key of
    another format.  Reads only: no weight is touched."""
    groups = collections.OrderedDict()
    for key, value in state_dict.items():
        head, _, suffix = key.partition(".")
        if suffix not in _SUFFIXES or not (head.startswith(UNET_PREFIX) or head.startswith(TE_PREFIX)):
            raise ValueError(f"LoRA key {key!r}: not a kohya-format key (lora_unet_<path> / lora_te_<path> with .lora_down.weight, "
                             f".lora_up.weight or .alpha); LoHa, DoRA and diffusers / PEFT formats are not read")
        groups.setdefault(head, {})[suffix] = value
    unet_names = _names(unet)
    te_names = None
    layers = []
    for head, parts in groups.items():
        up, down, alpha = parts.get("lora_up.weight"), parts.get("lora_down.weight"), parts.get("alpha")
        if up is None or down is None:
            have = next(s for s in _SUFFIXES if s in parts)
            raise ValueError(f"LoRA key {head + '.' + have!r} has no " + ("lora_up / lora_down pair" if have == "alpha" else
                             "partner " + repr(head + "." + ("lora_up.weight" if up is None else "lora_down.weight"))))
        key = head + ".lora_down.weight"
        if head.startswith(UNET_PREFIX):
            module = unet_names.get(head[len(UNET_PREFIX):])
        else:
            if text_encoder is None:
                raise ValueError(f"LoRA key {key!r} targets the text encoder, but the pipeline has none")
            if te_names is None:
                te_names = _names(text_encoder, strip="text_model_")
            path = head[len(TE_PREFIX):]
            module = te_names.get(path)
            if module is None and path.startswith("text_model_"):
                module = te_names.get(path[len("text_model_"):])
        if module is None:
            raise ValueError(f"LoRA key {key!r}: unknown target (no module of that name)")
        if down.dim() == 4 and not _is_1x1(down.shape):
            raise ValueError(f"LoRA key {key!r}: a {tuple(down.shape[2:])} down weight (LoCon) is not supported, only Linear and "
                             f"1x1-conv updates")
        linear = isinstance(module, nn.Linear)
        if not linear and not (isinstance(module, nn.Conv2d) and tuple(module.kernel_size) == (1, 1)):
            raise ValueError(f"LoRA key {key!r}: the target is a {type(module).__name__}, not a Linear or a 1x1 convolution")
        if up.dim() == 4 and not _is_1x1(up.shape):
            raise ValueError(f"LoRA key {head + '.lora_up.weight'!r}: a {tuple(up.shape[2:])} up weight is not supported")
        if up.dim() not in (2, 4) or down.dim() not in (2, 4):
            raise ValueError(f"LoRA key {key!r}: up {tuple(up.shape)} and down {tuple(down.shape)} are not matrices")
        N, K = module.weight.shape[0], module.weight.shape[1]
        rank = down.shape[0]
        if up.shape[1] != rank or rank < 1:
            raise ValueError(f"LoRA key {key!r}: rank mismatch, down is {tuple(down.shape)} and up {tuple(up.shape)}")
        if up.shape[0] != N or down.shape[1] != K:
            raise ValueError(f"LoRA key {key!r}: shape mismatch, up @ down is [{up.shape[0]}, {down.shape[1]}] and the weight "
                             f"[{N}, {K}]")
        if alpha is not None and torch.as_tensor(alpha).numel() != 1:
            raise ValueError(f"LoRA key {head + '.alpha'!r}: alpha is not a scalar")
        layers.append(Layer(key, module, up.reshape(N, rank), down.reshape(rank, K),
                            None if alpha is None else float(torch.as_tensor(alpha).float().item()), rank))
    if not layers:
        raise ValueError("load_lora_weights: the state dict holds no LoRA pair")
    return layers


def layer_gain(layer, scale, use_alpha):
    """what multiplies up @ down: `scale` (the reference), times alpha / rank only when asked and the file carries an alpha"""
    return float(scale) * (layer.alpha / layer.rank if use_alpha and layer.alpha is not None else 1.0)


class _Adapter:
    def __init__(self, name, scale, use_alpha, layers):
        self.name, self.scale, self.use_alpha = name, float(scale), bool(use_alpha)
        self.layers = {id(l.module.weight): l for l in layers}


class _Target:
    """one touched weight: the live parameter, its pristine copy, and (kernel route) where its segments sit in the table"""

    def __init__(self, param):
        self.param = param
        with torch.no_grad():
            self.base = param.detach().clone()
        self.kernel = False
        self.owners = None                  # kernel route: per segment, the adapter it belongs to


class LoraManager:
    """The LoRA state of one pipeline (pipe.load_lora_weights / set_lora_scale / unload_lora_weights / lora_state)."""

    def __init__(self, pipe):
        self.pipe = pipe
        self.adapters = collections.OrderedDict()
        self.targets = collections.OrderedDict()       # id(param) -> _Target, in first-touched order
        self.table = None                              # ops.LoraMergeTable over the kernel-route targets

    # ------------------------------------------------------------------ surface
    def load(self, source, scale=1.0, name=None, use_alpha=False):
        self._refuse_running_batcher("load_lora_weights")
        layers = resolve(read_state_dict(source), self.pipe.unet, getattr(self.pipe, "text_encoder", None))
        if name is None:
            name = os.path.splitext(os.path.basename(os.fspath(source)))[0] if not isinstance(source, dict) else f"lora{len(self.adapters)}"
        if name in self.adapters:
            raise ValueError(f"load_lora_weights: an adapter named {name!r} is loaded already")
        for l in layers:                               # the rank cap, over this adapter and those already on the weight
            ranks = [a.layers[id(l.module.weight)].rank for a in self.adapters.values() if id(l.module.weight) in a.layers]
            total = sum(ops.lora_padded_rank(r) for r in ranks + [l.rank])
            if total > ops.LORA_MAX_RANK:
                raise ValueError(f"LoRA key {l.key!r}: the adapters of this weight hold {total} padded rank columns, more than "
                                 f"{ops.LORA_MAX_RANK} (ops.LORA_MAX_RANK)")
        placed = [l._replace(up=l.up.detach().to(l.module.weight.device), down=l.down.detach().to(l.module.weight.device))
                  for l in layers]
        self.adapters[name] = _Adapter(name, scale, use_alpha, placed)
        self._rebuild()
        return name

    def set_scale(self, scale):
        self._refuse_running_batcher("set_lora_scale")
        if not self.adapters:
            raise ValueError("set_lora_scale: no LoRA is loaded")
        if isinstance(scale, dict):
            unknown = [n for n in scale if n not in self.adapters]
            if unknown:
                raise ValueError(f"set_lora_scale: no adapter named {unknown[0]!r} (loaded: {list(self.adapters)})")
            for n, s in scale.items():
                self.adapters[n].scale = float(s)
        else:
            for a in self.adapters.values():
                a.scale = float(scale)
        self._apply()

    def unload(self, name=None):
        self._refuse_running_batcher("unload_lora_weights")
        if name is not None and name not in self.adapters:
            raise ValueError(f"unload_lora_weights: no adapter named {name!r} (loaded: {list(self.adapters)})")
        if not self.adapters:
            return
        if name is None:
            self.adapters.clear()
        else:
            del self.adapters[name]
        self._rebuild()

    def state(self):
        return {"adapters": {a.name: {"scale": a.scale, "use_alpha": a.use_alpha, "layers": len(a.layers),
                                      "rank": max(l.rank for l in a.layers.values())} for a in self.adapters.values()},
                "targets": len(self.targets), "kernel_targets": sum(t.kernel for t in self.targets.values()),
                "base_bytes": sum(t.base.numel() * t.base.element_size() for t in self.targets.values()),
                "weights_epoch": self.pipe.weights_epoch}

    # ------------------------------------------------------------------ state
    def _refuse_running_batcher(self, what):
        for b in list(getattr(self.pipe, "_batchers", ())):
            t = getattr(b, "_thread", None)
            if t is not None and t.is_alive():
                raise RuntimeError(f"{what}: a ServingBatcher of this pipeline is running its own thread; stop() it, change the "
                                   f"weights, then build a new batcher")

    def _on(self, target):
        """the adapters that touch this weight, in load order -> [(adapter, layer)]"""
        return [(a, a.layers[id(target.param)]) for a in self.adapters.values() if id(target.param) in a.layers]

    def _rebuild(self):
        """after the set of adapters changed: bases for newly touched weights, the original bits back into weights no adapter
        touches any more, packed operands and the job table for the kernel route, then the merge"""
        touched = collections.OrderedDict()
        for a in self.adapters.values():
            for l in a.layers.values():
                touched.setdefault(id(l.module.weight), l.module.weight)
        with torch.no_grad():
            for pid in [p for p in self.targets if p not in touched]:
                t = self.targets.pop(pid)
                t.param.copy_(t.base)                  # bit for bit; copy_ moves the version counter
        for pid, param in touched.items():
            if pid not in self.targets:
                self.targets[pid] = _Target(param)
        jobs = []
        for t in self.targets.values():
            on = self._on(t)
            t.kernel = ops.lora_merge_takes(t.param, [l.rank for _, l in on])
            t.owners = None
            if t.kernel:
                N, K = t.param.shape[0], t.param.shape[1]
                up, down, owner = ops.lora_pack_adapters([(l.up, l.down) for _, l in on], N, K, device=t.param.device)
                t.owners = [on[i] for i in owner]
                jobs.append((t.param, t.base, up, down))
        self.table = ops.LoraMergeTable(jobs) if jobs else None
        self._apply()

    def _apply(self):
        """every touched weight from its base at the adapters' present scales: one launch for the kernel route, the reference's
        statements for the rest; then what the change invalidates"""
        kernel_gains = []
        for t in self.targets.values():
            if t.kernel:
                kernel_gains.append([layer_gain(l, a.scale, a.use_alpha) for a, l in t.owners])
            else:
                ops.lora_merge_eager(t.param, t.base, [(l.up, l.down, layer_gain(l, a.scale, a.use_alpha)) for a, l in self._on(t)])
        if self.table is not None:
            ops.lora_merge_(self.table, kernel_gains)
        self.pipe._graphs = {}                         # a captured step holds derived weights of the old values
        self.pipe.weights_epoch += 1
