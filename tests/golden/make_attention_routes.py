"""Which entry point an attention call reaches, recorded without a device, with the pieces of make_linear_routes.py: CPU tensors
that claim to be on the GPU, a fake library that records (name, args), ops._stream_ptr / torch.empty patched for the duration of
a call - and F.scaled_dot_product_attention and the score matmul of the library routes patched the way F.linear is there.

    python tests/golden/make_attention_routes.py      (re)writes tests/golden/attention_routes.json

Run it at the commit whose routing is the reference; tests/test_attention_dispatch_host.py replays the same cases through the same
recorder and requires equality with the file.  The cases drive the four public processors through a small Attention module
(L = 64, B = 2, H = 2) and scaled_dot_product_attention_regionstate directly.

A row is [calls, exception type or None]; a call is
  [entry, arg, ...] for dsc_region_xattn*, dsc_self_attn_fwd, dsc_ip_xattn_add* and dsc_xattn_kv_pack, every argument in the
      order of include/dsc_hip.h: an integer or a float (sizes, Bw, nrows, the flag word, the host sigma, the scale) as itself, a
      stride array as a list, a pointer (operands, the device sigma, the region table, ids / rows, the stream) as "p" or None;
  ["sdpa", q shape, k shape, mask shape or None] and ["matmul", a shape, b shape] for the library routes;
  [entry] for anything else (the dsc_linear* of the projections: their routing is pinned by linear_routes.json); the
      *_bytes size queries are left out."""
import contextlib
import ctypes
import itertools
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from diffusionspatialcontrol_amd import _lib, ops  # noqa: E402
from diffusionspatialcontrol_amd.modules import attention_modify as am  # noqa: E402
from diffusionspatialcontrol_amd.modules.u_net_condition_modify import Attention, LNFold  # noqa: E402

PATH = os.path.join(HERE, "attention_routes.json")
B, H, L, CTX = 2, 2, 64, 32
KEYS = (77, 96, 97, 154, 384, 385)
HEAD_DIMS = (40, 64, 160, 168, 36)          # 168: a multiple of 8 above the limit; 36: not a multiple of 8
ARGS_OF = ("dsc_region_xattn", "dsc_self_attn_fwd", "dsc_ip_xattn_add", "dsc_xattn_kv_pack")
PROCESSORS = {"AttnProcessor": am.AttnProcessor, "AttnProcessor2_0": am.AttnProcessor2_0,
              "IPAdapterAttnProcessor": am.IPAdapterAttnProcessor, "IPAdapterAttnProcessor2_0": am.IPAdapterAttnProcessor2_0}

_empty, _matmul = torch.empty, torch.Tensor.__matmul__
_log = []                                   # the calls of the case being recorded: the fake library's and the markers


class OnDevice(torch.Tensor):
    """a CPU tensor that claims to be on the GPU: enough for the wrappers to reach the (fake) library"""
    is_cuda = property(lambda self: True)

    def __matmul__(self, other):
        _log.append(("matmul", (self, other)))
        return _matmul(self, other)


def fake(*shape, dtype=torch.float16):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


class FakeLib:
    def __getattr__(self, name):
        def fn(*args):
            if name == "dsc_xattn_kv_pack_bytes":       # region_xattn_packed.hip: 0 = this (S, d) has no packed image
                Bc, Hh, S, d = args
                return 0 if S > 384 or d % 8 or d > 160 else 2 * Bc * Hh * ((S + 95) // 96) * 96 * d * 2
            if not name.endswith("_bytes"):
                _log.append((name, args))
            return 0
        return fn


@contextlib.contextmanager
def faked():
    """attention on the fake library, the library routes recorded as markers"""
    def sdpa(q, k, v, attn_mask=None, scale=None, **kw):
        _log.append(("sdpa", (q, k, attn_mask)))
        return _empty(q.shape, dtype=q.dtype).as_subclass(OnDevice)

    lib = FakeLib()
    patches = [(_lib, "load_library", lambda: lib), (ops, "_stream_ptr", lambda t: None), (F, "scaled_dot_product_attention", sdpa),
               (torch, "empty", lambda *a, **kw: _empty(*a, **{k: v for k, v in kw.items() if k != "device"}).as_subclass(OnDevice))]
    saved = [(obj, name, getattr(obj, name)) for obj, name, _ in patches]
    try:
        for obj, name, value in patches:
            setattr(obj, name, value)
        yield lib
    finally:
        for obj, name, value in saved:
            setattr(obj, name, value)


def _plain(a):
    if a is None or isinstance(a, (int, str)):
        return a
    if isinstance(a, float):
        return round(a, 6)
    if isinstance(a, ctypes.Array):
        return list(a)
    return "p"                              # c_void_p


def _shape(t):
    return None if t is None else list(t.shape)


def record(run):
    """one row of the file (see the module docstring): `run` is a case's callable"""
    del _log[:]
    error = None
    try:
        run()
    except Exception as e:
        error = type(e).__name__
    calls = []
    for name, a in _log:
        if name in ("sdpa", "matmul"):
            calls.append([name] + [_shape(t) for t in a])
        elif name.startswith(ARGS_OF):
            calls.append([name] + [_plain(x) for x in a])
        else:
            calls.append([name])
    return [calls, error]


# ----------------------------------------------------------------------------- the operands of a case
def default_like(w, sigma, qk):
    return w * sigma * qk.std()


def custom(w, sigma, qk):
    return w * sigma * 0.5


WEIGHT_FUNCS = {"none": None, "default": default_like, "custom": custom}


def table(rows, S, distinct=3, queries=L):
    """region table [rows, queries, S] fp32 with `distinct` different rows per image"""
    w = torch.zeros(rows, queries, S)
    w += (torch.arange(queries) % distinct).float()[None, :, None]
    return w.as_subclass(OnDevice)


def module(d, dtype, processor, cross=True, **proc_kw):
    torch.manual_seed(0)
    attn = Attention(H * d, CTX if cross else None, heads=H, dim_head=d).to(dtype)
    cls = PROCESSORS[processor]
    proc = cls(H * d, CTX, **proc_kw) if cls.is_ip_adapter else cls(**proc_kw)
    attn.set_processor(proc.to(dtype) if isinstance(proc, nn.Module) else proc)
    return attn


def text_cache(attn, text, packed):
    """what the pipeline's _refresh_text_kv leaves on a cross-attention layer; the packed image where the (S, d) has one"""
    k, v = attn.to_k(text), attn.to_v(text)
    c = {"src": text, "k": k, "v": v, "packed": None}
    Bt, S, C = k.shape
    d = C // attn.heads
    if packed and _lib.load_library().dsc_xattn_kv_pack_bytes(Bt, attn.heads, S, d):
        c["packed"] = ops.xattn_kv_pack(k.view(Bt, S, attn.heads, d), v.view(Bt, S, attn.heads, d))
    return c


def region_prompt(kind, S, wf="none", sigma="device", groups=2, per_group=False, level=L, rows=B, table_L=L):
    """kind: absent | dense | compressed | static (compressed=False) | many (more than 32 distinct rows);
    per_group: True, or "short" for a sigma tensor of another size than the groups"""
    if kind == "absent":
        return None
    w = table(rows, S, distinct=40 if kind == "many" else 3, queries=table_L)
    rp = {"region_state": {level: w}, "weight_func": WEIGHT_FUNCS[wf], "n_std_groups": groups}
    if per_group:
        rp["sigma_per_group"] = True
        rp["sigma"] = torch.full((groups + (per_group == "short"),), 2.0).as_subclass(OnDevice)
    else:
        rp["sigma"] = {"float": 2.0, "cpu": torch.tensor(2.0), "device": torch.tensor(2.0).as_subclass(OnDevice),
                       "device-fp16": torch.tensor(2.0, dtype=torch.float16).as_subclass(OnDevice)}[sigma]
    if kind == "compressed":
        ids, rws = ops.compress_region_table(w, pad_rows=True)
        rp["compressed"] = {level: (ids, ops.pad_region_rows(rws) if S <= 96 else rws)}
    elif kind == "static":
        rp["compressed"] = False
    return rp


def processor_case(S=77, d=40, dtype=torch.float16, processor="AttnProcessor2_0", cross=True, region="dense", kv="none", wf="none",
                   mask=False, per_group=False, ref16=False, groups=2, sigma="device", prefix=False, level=L, rows=B, table_L=L, fold=False):
    """-> the callable that runs one processor call; kv: none | cache | packed | other (another slot's cache is the current one)"""
    def run():
        attn = module(d, dtype, processor, cross, ref_fp16_rounding=ref16)
        x = fake(1 if prefix else B, L, H * d, dtype=dtype)
        text = fake(B, S, CTX, dtype=dtype) if cross else None
        if kv != "none":
            mine = text_cache(attn, text, kv != "cache")
            attn.kv_cache = mine
            if kv == "other":
                attn.kv_cache = text_cache(attn, fake(B, S, CTX, dtype=dtype), True)
                attn.kv_caches = [attn.kv_cache, mine]
        kw = {}
        if mask:
            kw["attention_mask"] = fake(B, 1, (S if cross else L) - 7 * (mask == "short"), dtype=dtype)   # short: refused
        if fold:
            norm = nn.LayerNorm(H * d).to(dtype)
            kw["_ln_fold"] = LNFold(norm, fake(x.shape[0] * L, 2, 2, dtype=torch.float32), x)
        if cross:
            kw["region_prompt"] = region_prompt(region, S, wf, sigma, groups, per_group, level, rows, table_L)
        attn(x, text, **kw)
    return run


def ip_case(processor, tokens=(4,), form="tuple", d=40, dtype=torch.float16, region="dense", masks=None, rows=None, cross=True, S=77):
    """form: tuple = (text, [tokens]) | single = the deprecated one tensor; masks: None | good | count | list;
    rows: None | plain | weight | dict | dict-miss | adapters (one adapter too many)"""
    def run():
        attn = module(d, dtype, processor, num_tokens=list(tokens))
        proc = attn.processor
        x, text = fake(B, L, H * d, dtype=dtype), fake(B, S, CTX, dtype=dtype)
        ip = [fake(B, T, CTX, dtype=dtype) for T in tokens]
        rp = region_prompt(region, S) or ({} if rows is None else {"region_state": None})
        kw = {}
        if masks is not None:
            m = fake(len(tokens) + (masks == "count"), 1, 8, 8, dtype=dtype)
            kw["ip_adapter_masks"] = list(m) if masks == "list" else m
        if rows is not None:
            each = []
            for T in tokens:
                r = (fake(B, T, H * d), fake(B, T, H * d), fake(B, dtype=torch.float32))
                if rows in ("weight", "dict", "dict-miss"):
                    qw = fake(B, L)
                    r += (qw if rows == "weight" else {L if rows == "dict" else 2 * L: qw},)
                each.append(r)
            rp["ip_rows"] = {proc: each + each[:1] if rows == "adapters" else each}
            enc = text
        else:
            enc = (text, ip) if form == "tuple" else torch.cat([text, ip[0]], dim=1)
        attn(x, enc if cross else None, region_prompt=rp or None, **kw)
    return run


def functional_case(S, d, dtype=torch.float16, wf="none", mask=None, groups=1, **extra):
    """scaled_dot_product_attention_regionstate; mask: None | float ([L, S]) | float3 ([B, 1, S]: refused) | bool"""
    def run():
        q, k, v = fake(B, H, L, d, dtype=dtype), fake(B, H, S, d, dtype=dtype), fake(B, H, S, d, dtype=dtype)
        m = {None: None, "float": fake(L, S, dtype=dtype), "float3": fake(B, 1, S, dtype=dtype),
             "bool": torch.ones(L, S, dtype=torch.bool).as_subclass(OnDevice)}[mask]
        am.scaled_dot_product_attention_regionstate(q, k, v, attn_mask=m, weight_func=WEIGHT_FUNCS[wf], region_state=table(B, S),
                                                    sigma=torch.tensor(2.0).as_subclass(OnDevice), n_std_groups=groups, **extra)
    return run


def _name(**kw):
    return " ".join(f"{k}={str(v).replace('torch.', '')}" for k, v in kw.items())


def cases():
    """(id, callable), each id once"""
    half, single = torch.float16, torch.float32
    regions = ("absent", "dense", "compressed", "static", "many")
    groups = []
    # every key count against every table form, K/V cache and weight_func
    groups += [dict(S=S, region=r, kv=kv, wf=wf) for S, r, kv, wf in
               itertools.product(KEYS, regions, ("none", "cache", "packed", "other"), WEIGHT_FUNCS)
               if not (r == "absent" and wf != "none")]
    # head dims and dtypes the kernels refuse
    groups += [dict(S=S, d=d, dtype=dt, region=r, kv=kv) for S, (d, dt), r, kv in
               itertools.product(KEYS, [(d, half) for d in HEAD_DIMS[1:]] + [(40, single), (168, single)],
                                 ("absent", "dense", "compressed"), ("none", "packed"))]
    # attention masks
    groups += [dict(S=S, region=r, kv=kv, wf=wf, mask=True, processor=p) for S, r, kv, wf, p in
               itertools.product(KEYS, ("absent", "dense"), ("none", "packed"), WEIGHT_FUNCS, ("AttnProcessor", "AttnProcessor2_0"))
               if not (r == "absent" and wf != "none")]
    groups += [dict(S=S, d=d, dtype=dt, region="absent", mask=True) for S, (d, dt) in
               itertools.product(KEYS, [(168, half), (36, half), (40, single)])]
    groups += [dict(S=77, region=r, wf=wf, mask="short", processor="AttnProcessor") for r, wf in
               (("absent", "none"), ("dense", "none"), ("dense", "custom"))]
    # one sigma per std group (serving)
    groups += [dict(S=S, region=r, kv=kv, wf=wf, per_group=True) for S, r, kv, wf in
               itertools.product(KEYS, regions[1:], ("none", "packed"), WEIGHT_FUNCS)]
    groups += [dict(S=S, region="dense", per_group=True, mask=True, processor="AttnProcessor") for S in (77, 154)]
    groups += [dict(S=77, region=r, kv=kv, per_group="short") for r, kv in (("dense", "none"), ("compressed", "packed"))]   # refused
    # the reference's fp16 rounding, one std group, the other processor, the forms of sigma, the shared CFG prefix
    groups += [dict(S=S, region=r, kv=kv, wf=wf, ref16=True) for S, r, kv, wf in
               itertools.product(KEYS, regions[1:], ("none", "packed"), ("none", "custom"))]
    groups += [dict(S=S, region=r, kv=kv, wf=wf, groups=1) for S, r, kv, wf in
               itertools.product((77, 154), ("dense", "compressed"), ("none", "packed"), ("none", "custom"))]
    groups += [dict(S=S, region=r, kv=kv, processor="AttnProcessor") for S, r, kv in itertools.product(KEYS, regions, ("none", "packed"))]
    groups += [dict(S=S, region=r, kv=kv, sigma=s) for S, r, kv, s in
               itertools.product((77, 154), ("dense", "compressed"), ("none", "packed"), ("float", "cpu", "device-fp16"))]
    groups += [dict(S=S, region=r, kv=kv, prefix=True) for S, r, kv in
               itertools.product((77, 154), ("absent", "dense", "compressed"), ("none", "packed"))]
    # self-attention
    groups += [dict(cross=False, d=d, dtype=dt, processor=p, mask=m) for d, dt, p, m in
               itertools.product(HEAD_DIMS, (half, single), ("AttnProcessor", "AttnProcessor2_0"), (False, True))]
    # the LayerNorm fold, and what the table lookup refuses
    groups += [dict(cross=False, d=64, fold=True), dict(S=77, d=64, kv="packed", region="compressed", fold=True)]
    groups += [dict(S=77, region="dense", level=2 * L), dict(S=77, region="dense", table_L=2 * L), dict(S=77, region="dense", rows=1)]
    for kw in groups:
        yield "processor " + _name(**kw), processor_case(**kw)

    for p in ("IPAdapterAttnProcessor", "IPAdapterAttnProcessor2_0"):
        ip = [dict(tokens=(T,), d=d, dtype=dt) for T, (d, dt) in itertools.product((4, 16, 257), [(40, half), (168, half), (36, half), (40, single)])]
        ip += [dict(tokens=(4, 16)), dict(tokens=(4,), form="single"), dict(tokens=(4,), region="absent"), dict(tokens=(4,), S=154),
               dict(tokens=(4,), cross=False), dict(tokens=(4, 16), masks="good"), dict(tokens=(4,), masks="count"),
               dict(tokens=(4,), masks="list")]
        ip += [dict(tokens=t, rows=r) for t, r in itertools.product(((4,), (4, 16)), ("plain", "weight", "dict"))]
        ip += [dict(tokens=(4,), rows="dict-miss"), dict(tokens=(4,), rows="adapters"), dict(tokens=(4,), rows="plain", masks="good"),
               dict(tokens=(257,), rows="plain"), dict(tokens=(4,), rows="plain", d=168), dict(tokens=(4,), rows="plain", region="absent"),
               dict(tokens=(4,), rows="plain", dtype=single)]
        for kw in ip:
            yield f"{p} " + _name(**kw), ip_case(p, **kw)

    fn = [dict(S=S, d=d, wf=wf, mask=m) for S, d, wf, m in itertools.product(KEYS, (40, 168), WEIGHT_FUNCS, (None, "float", "bool"))]
    fn += [dict(S=77, d=40, mask="float3"), dict(S=77, d=40, dtype=single), dict(S=77, d=40, groups=2), dict(S=154, d=40, groups=2),
           dict(S=77, d=40, is_causal=True), dict(S=77, d=40, dropout_p=0.1)]
    for kw in fn:
        yield "functional " + _name(**kw), functional_case(**kw)


def record_all():
    with faked():
        rows = [(cid, record(run)) for cid, run in cases()]
    assert len(dict(rows)) == len(rows), "case ids repeat"
    return dict(rows)


def load():
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    table_ = record_all()
    with open(PATH, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(c)}: {json.dumps(row, separators=(',', ':'))}" for c, row in table_.items()) + "\n}\n")
    assert load() == json.loads(json.dumps(table_))
    errors = {}
    for row in table_.values():
        errors[row[1]] = errors.get(row[1], 0) + 1
    print(len(table_), errors)
