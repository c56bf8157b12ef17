"""What ops.linear does with its operands, recorded without a device: CPU tensors that claim to be on the GPU, a fake library that
records (name, args), and ops._stream_ptr / torch.empty / F.linear patched for the duration of a call.

    python tests/golden/make_linear_routes.py      (re)writes tests/golden/linear_routes.json

Run it at the commit whose routing is the reference; tests/test_linear_dispatch_host.py replays the same cases through the same
recorder and requires equality with the file.  geglu=True together with a residual is refused by ops.linear and is not a case.

A row is [calls, linear_kernel_covers, linear_kernel_can, linear_qkv_covers (8 heads), exception type or None]; a call is
  [entry, M, N, K, ldx, ldr (with the wrap bits), n_out / ldo, geglu flag, residual rows, x is the caller's, residual is the caller's]
for the dsc_linear* entries, ["torch", M, N, K, residual rows, x is the caller's, residual is the caller's] for F.linear and
[entry] for anything else (dsc_geglu); the residual fields are 0 / None without a residual."""
import contextlib
import json
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from diffusionspatialcontrol_amd import _lib, ops  # noqa: E402

PATH = os.path.join(HERE, "linear_routes.json")

ROWS = (2, 64, 128, 154, 256, 512, 1024, 2048)
N_K = ((320, 320), (320, 1280), (640, 1920), (1280, 5120), (2560, 320), (10240, 1280), (320, 768), (100, 320), (320, 100))
VARIANT_SHAPES = ((1024, 320, 320), (256, 320, 2560))
_LIBRARY = {"USE_LIBRARY_GEMM": True, "USE_LT_RESIDUAL": True, "USE_LT_ALL": True}
SETTINGS = {
    "default": {},
    "library": dict(_LIBRARY, lt_rc=0),
    "library-declines": dict(_LIBRARY, lt_rc=-2),
    "no-splitk": {"USE_SPLITK": False},
    "no-wrap": {"USE_RESIDUAL_WRAP": False},
    "open": {"DSC_GEMM_MIN_ROWS": 1, "DSC_GEMM_MAX_K": 1 << 30, "DSC_GEMM_MID_ROWS": 1, "DSC_GEMM_MID_K": 1 << 30},
}

_empty = torch.empty


class OnDevice(torch.Tensor):
    """a CPU tensor that claims to be on the GPU: enough for the wrappers to reach the (fake) library"""
    is_cuda = property(lambda self: True)


class _Product(OnDevice):
    """what the fake F.linear returns: remembers what is added to it"""
    added = None

    def __add__(self, other):
        _Product.added = other
        return self


def fake(*shape, dtype=torch.float16):
    return _empty(*shape, dtype=dtype).as_subclass(OnDevice)


class FakeLib:
    def __init__(self, lt_rc=0):
        self.calls, self.lt_rc = [], lt_rc

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.lt_rc if name == "dsc_linear_lt_f16" else 0
        return fn


@contextlib.contextmanager
def faked(lt_rc=0, **switches):
    """ops with the switches of one setting, on the fake library -> the library"""
    lib = FakeLib(lt_rc)

    def linear(x, weight, bias=None):
        lib.calls.append(("torch", (x, weight)))
        return _empty(x.shape[:-1] + (weight.shape[0],), dtype=x.dtype).as_subclass(_Product)

    patches = [(ops, k, v) for k, v in switches.items()]
    patches += [(_lib, "load_library", lambda: lib), (ops, "_stream_ptr", lambda t: None), (F, "linear", linear),
                (torch, "empty", lambda *a, **kw: _empty(*a, **kw).as_subclass(OnDevice))]
    saved = [(obj, name, getattr(obj, name)) for obj, name, _ in patches]
    try:
        for obj, name, value in patches:
            setattr(obj, name, value)
        yield lib
    finally:
        for obj, name, value in saved:
            setattr(obj, name, value)


def cases():
    """(id, x, weight, bias, residual, geglu, prefer_kernel) - operands are built once per shape and never written"""
    made = {}

    def t(*shape, dtype=torch.float16):
        key = (shape, dtype)
        if key not in made:
            made[key] = fake(*shape, dtype=dtype)
        return made[key]

    for M in ROWS:
        for N, K in N_K:
            for res in ("none", "full", "half"):
                for geglu in (False, True):
                    if geglu and res != "none":
                        continue
                    r = None if res == "none" else t(2 if res == "full" else 1, M // 2, N)
                    for prefer in (False, True):
                        yield f"{M}x{N}x{K} r={res} geglu={int(geglu)} prefer={int(prefer)}", t(2, M // 2, K), t(N, K), t(N), r, geglu, prefer
    for M, N, K in VARIANT_SHAPES:
        x, w, b = t(M, K), t(N, K), t(N)
        variants = {
            "x at a 2-byte offset": dict(x=t(M * K + 1)[1:].view(M, K)),
            "x row stride 4 mod 8": dict(x=t(M, K + 4)[:, :K]),
            "fp32 x": dict(x=t(M, K, dtype=torch.float32)),
            "transposed weight": dict(w=t(K, N).t()),
            "3-D slice that does not collapse": dict(x=t(2, M // 2 + 1, K)[:, :M // 2]),
            "permuted 3-D x": dict(x=t(M // 2, 2, K).permute(1, 0, 2)),
            "strided residual, good rows": dict(r=t(M, N + 8)[:, :N]),
            "residual row stride 4 mod 8": dict(r=t(M, N + 4)[:, :N]),
            "geglu without a bias": dict(b=None, geglu=True),
            "no bias": dict(b=None),
            "fused q / k / v weight, 3-D x": dict(x=t(2, M // 2, K), w=t(3 * N, K), b=t(3 * N)),   # linear_qkv_covers' True side
        }
        for name, v in variants.items():
            for prefer in (False, True):
                yield (f"{M}x{N}x{K} {name} prefer={int(prefer)}", v.get("x", x), v.get("w", w), v.get("b", b), v.get("r"),
                       v.get("geglu", False), prefer)


def _ptr(arg):
    return getattr(arg, "value", None) if arg is not None else None


def _answer(fn, *args):
    try:
        return bool(fn(*args))
    except Exception as e:                       # an answer too
        return type(e).__name__


def record(lib, x, weight, bias, residual, geglu, prefer):
    """one row of the file (see the module docstring)"""
    del lib.calls[:]
    _Product.added = None
    error = None
    try:
        ops.linear(x, weight, bias, residual=residual, geglu=geglu, prefer_kernel=prefer)
    except Exception as e:
        error = type(e).__name__
    own_r = residual.data_ptr() if residual is not None else None
    calls = []
    for name, a in lib.calls:
        if name in ("dsc_linear_f16", "dsc_linear_splitk_f16", "dsc_linear_lt_f16"):
            M, ldr, r = a[5], a[9], _ptr(a[3])
            geglu_flag = a[11] if name == "dsc_linear_f16" else 0
            calls.append([name, M, a[6], a[7], a[8], ldr, a[10], geglu_flag, ((ldr >> 32) or M) if r is not None else 0,
                          _ptr(a[0]) == x.data_ptr(), (r == own_r) if r is not None else None])
        elif name == "torch":
            xa, r = a[0], _Product.added
            K = xa.shape[-1]
            calls.append([name, xa.numel() // K, a[1].shape[0], K, r.numel() // r.shape[-1] if r is not None else 0,
                          xa.data_ptr() == x.data_ptr(), (r.data_ptr() == own_r) if r is not None else None])
        else:
            calls.append([name])
    N, K = weight.shape
    M = x.numel() // K
    return [calls, _answer(ops.linear_kernel_covers, M, N, K, x.dtype, geglu), _answer(ops.linear_kernel_can, x, weight, bias, residual),
            _answer(ops.linear_qkv_covers, x, weight, 8), error]


def record_all():
    """{setting: {case id: row}}"""
    table = {}
    for setting, switches in SETTINGS.items():
        with faked(**switches) as lib:
            table[setting] = {cid: record(lib, *operands) for cid, *operands in cases()}
    return table


def load():
    """the committed table; the file holds every row of "default" and, of the other settings, the rows that differ from it"""
    with open(PATH) as f:
        table = json.load(f)
    return {setting: {**table["default"], **rows} for setting, rows in table.items()}


if __name__ == "__main__":
    table = record_all()
    kept = {s: {c: row for c, row in rows.items() if s == "default" or row != table["default"][c]} for s, rows in table.items()}
    with open(PATH, "w") as f:
        f.write("{\n" + ",\n".join(
            json.dumps(s) + ": {\n" + ",\n".join(f" {json.dumps(c)}: {json.dumps(row, separators=(',', ':'))}" for c, row in rows.items()) + "\n}"
            for s, rows in kept.items()) + "\n}\n")
    assert load() == json.loads(json.dumps(table))
    print({s: len(rows) for s, rows in kept.items()})
