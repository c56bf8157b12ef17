"""The one place that resolves a 3x3 convolution's resample mode (ops._conv3x3_geometry) and the "try" entry, without a device:
the CONV_* codes against include/dsc_hip.h, the geometry of every mode, the refusals, conv3x3_try on CPU tensors, and that the
resample argument handed to the library is always one of the named codes."""
import itertools
import os
import re

import pytest
import torch

from diffusionspatialcontrol_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADER_NAMES = {"CONV_UPSAMPLE2X": "DSC_CONV_UPSAMPLE2X", "CONV_STRIDE2": "DSC_CONV_STRIDE2", "CONV_STRIDE2_PAD_BR": "DSC_CONV_STRIDE2_PAD_BR",
                "CONV_UPSAMPLE_SIZE": "DSC_CONV_UPSAMPLE_CEIL"}
# keywords of each mode (on the 5 x 7 image; pad-br on 6 x 8): mode, convolution (H, W), output (oh, ow)
TABLE = [({}, (5, 7), 0, (5, 7), (5, 7)),
         ({"upsample": True}, (5, 7), 1, (10, 14), (10, 14)),
         ({"stride2_ceil": True}, (5, 7), 2, (5, 7), (3, 4)),
         ({"stride2_pad_br": True}, (6, 8), 3, (6, 8), (3, 4)),
         ({"upsample_size": (9, 14)}, (5, 7), 4, (9, 14), (9, 14))]


def _x(hw=(5, 7)):
    return torch.zeros(1, 64, *hw, dtype=torch.float16)


W = torch.zeros(64, 64, 3, 3, dtype=torch.float16)


def test_codes_mirror_the_header():
    with open(os.path.join(ROOT, "include", "dsc_hip.h")) as f:
        defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (DSC_CONV_\w+) (\d+)", f.read(), re.M)}
    assert sorted(defines) == sorted(HEADER_NAMES.values())
    for name, c_name in HEADER_NAMES.items():
        assert getattr(ops, name) == defines[c_name], name
    assert ops.CONV_PLAIN == 0 and 0 not in defines.values()


@pytest.mark.parametrize("kw,hw,mode,conv_hw,out_hw", TABLE)
def test_geometry_table(kw, hw, mode, conv_hw, out_hw):
    assert ops._conv3x3_geometry(_x(hw), **kw) == (mode, conv_hw, out_hw)


def test_geometry_refusals():
    with pytest.raises(ValueError):
        ops._conv3x3_geometry(_x(), stride2=True)                               # the even-sides rule of the older keyword
    assert ops._conv3x3_geometry(_x((6, 8)), stride2=True) == (2, (6, 8), (3, 4))
    assert ops._conv3x3_geometry(_x((6, 8)), stride2=True, stride2_ceil=True)[0] == 2    # two spellings of one mode
    modes = [{"upsample": True}, {"upsample_size": (12, 16)}, {"stride2": True}, {"stride2_ceil": True}, {"stride2_pad_br": True}]
    for a, b in itertools.combinations(modes, 2):
        if {**a, **b} == {"stride2": True, "stride2_ceil": True}:
            continue
        with pytest.raises(ValueError):
            ops._conv3x3_geometry(_x((6, 8)), **a, **b)
        with pytest.raises(ValueError):                                         # ... before the device is asked for
            ops.conv3x3(_x((6, 8)), W, **a, **b)
    for fn in (ops.conv3x3_supported, lambda *a, **kw: ops.conv3x3_gn_rows(*a, 32, **kw), lambda *a, **kw: ops.conv3x3_gn(*a, 32, **kw)):
        with pytest.raises(ValueError):
            fn(_x((6, 8)), W, upsample=True, upsample_size=(12, 16))


def test_conv3x3_try_on_cpu_tensors():
    """a CPU tensor is covered by no kernel: None for every good argument set, ValueError for the bad ones (the sizes of
    test_any_size_host.py::test_upsample_size_argument_refusals, on its 3 x 5 image)"""
    for kw, hw, mode, _, _ in TABLE:
        assert ops.conv3x3_try(_x(hw), W, mode=mode, size=kw.get("upsample_size")) is None
    assert ops.conv3x3_try(_x(), W, None, _x(), out_nchw=True, splits=2) is None
    x = _x((3, 5))
    for good in ((5, 9), (6, 9), (5, 10), (6, 10)):
        assert ops.conv3x3_try(x, W, mode=ops.CONV_UPSAMPLE_SIZE, size=good) is None
    for bad in ((7, 9), (5, 11), (4, 9), (5, 8), (3, 5), (0, 9), (5, 9, 1)):
        with pytest.raises(ValueError):
            ops.conv3x3_try(x, W, mode=ops.CONV_UPSAMPLE_SIZE, size=bad)
    with pytest.raises(ValueError):
        ops.conv3x3_try(x, W, mode=ops.CONV_UPSAMPLE_SIZE)                      # the mode without its size
    for mode in (ops.CONV_PLAIN, ops.CONV_UPSAMPLE2X, ops.CONV_STRIDE2, ops.CONV_STRIDE2_PAD_BR):
        with pytest.raises(ValueError):
            ops.conv3x3_try(x, W, mode=mode, size=(5, 9))                       # a size with another mode
    for mode in (-1, 5, None, "upsample"):
        with pytest.raises(ValueError):
            ops.conv3x3_try(x, W, mode=mode)


class _Code(int):
    """an integer that remembers it came from a named constant"""


class _OnDevice(torch.Tensor):
    """a CPU tensor that claims to be on the GPU: enough for the wrappers to reach the (fake) library"""
    is_cuda = property(lambda self: True)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return {"dsc_conv3x3_supported": 1, "dsc_conv3x3_gn_rows": 2}.get(name, 0)
        return fn


def test_resample_argument_is_always_a_named_code(monkeypatch):
    """with the CONV_* constants replaced by marked integers, every resample argument that reaches dsc_conv3x3_nhwc_f16,
    dsc_conv3x3_gn_nhwc_f16 and dsc_conv3x3_gn_rows is a marked one: no call builds the code from a literal"""
    lib = _FakeLib()
    for name in ("CONV_PLAIN", *HEADER_NAMES):
        monkeypatch.setattr(ops, name, _Code(getattr(ops, name)))
    monkeypatch.setattr(_lib, "load_library", lambda: lib)
    monkeypatch.setattr(ops, "_stream_ptr", lambda t: None)
    x, x68, w = _x().as_subclass(_OnDevice), _x((6, 8)).as_subclass(_OnDevice), W.as_subclass(_OnDevice)
    for kw, hw, mode, _, _ in TABLE:
        xi = x68 if hw == (6, 8) else x
        ops.conv3x3(xi, w, **kw)
        assert ops.conv3x3_try(xi, w, mode=mode, size=kw.get("upsample_size")) is not None
        if mode in (0, 1, 4):
            assert ops.conv3x3_gn_rows(xi, w, 32, **kw) == 2
            ops.conv3x3_gn(xi, w, 32, **kw)
    ops.conv3x3(x68, w, stride2=True)
    position = {"dsc_conv3x3_nhwc_f16": 13, "dsc_conv3x3_gn_nhwc_f16": 15, "dsc_conv3x3_gn_rows": 6}
    seen = {name: set() for name in position}
    for name, args in lib.calls:
        if name in position:
            code = args[position[name]]
            assert isinstance(code, _Code), (name, code)
            seen[name].add(int(code))
    assert seen == {"dsc_conv3x3_nhwc_f16": {0, 1, 2, 3, 4}, "dsc_conv3x3_gn_nhwc_f16": {0, 1, 4}, "dsc_conv3x3_gn_rows": {0, 1, 4}}
