"""The one place that routes a linear (ops._linear_plan), without a device: every case of tests/golden/make_linear_routes.py
replayed through the public ops.linear against the recorded table (entry points, integer arguments, copies, exception types and
the answers of the covers / can predicates, under six settings of the switches), and the declared refusals."""
import pytest
import torch

import make_linear_routes as routes
from diffusionspatialcontrol_amd import ops


@pytest.fixture(scope="module")
def recorded():
    return routes.load()


@pytest.mark.parametrize("setting", list(routes.SETTINGS))
def test_routes_match_the_recording(recorded, setting):
    with routes.faked(**routes.SETTINGS[setting]) as lib:
        got = {cid: routes.record(lib, *operands) for cid, *operands in routes.cases()}
    want = recorded[setting]
    assert sorted(got) == sorted(want)
    wrong = {cid: (row, want[cid]) for cid, row in got.items() if row != want[cid]}
    assert not wrong, (len(wrong), next(iter(wrong.items())))


def test_every_route_is_reached(recorded):
    """each LINEAR_* constant the plan can return, and both ways out of a library route that declines"""
    seen = set()
    for setting, switches in routes.SETTINGS.items():
        with routes.faked(**switches):
            for _, x, w, b, r, geglu, prefer in routes.cases():
                route, fallback = ops._linear_plan(x, w, b, r, geglu, prefer)[:2]
                seen.add((route, fallback if route == ops.LINEAR_LIBRARY else None))
    assert seen == {(ops.LINEAR_KERNEL, None), (ops.LINEAR_SPLITK, None), (ops.LINEAR_TORCH, None),
                    (ops.LINEAR_LIBRARY, ops.LINEAR_KERNEL), (ops.LINEAR_LIBRARY, ops.LINEAR_TORCH)}
    chains = {tuple(c[0] for c in row[0] if c[0] != "dsc_linear_splitk_workspace_bytes") for rows in recorded.values() for row in rows.values()}
    assert chains == {("dsc_linear_f16",), ("dsc_linear_splitk_f16",), ("dsc_linear_lt_f16",), ("dsc_linear_lt_f16", "dsc_geglu"),
                      ("dsc_linear_lt_f16", "dsc_linear_f16"), ("dsc_linear_lt_f16", "torch"), ("dsc_linear_lt_f16", "torch", "dsc_geglu"),
                      ("torch",), ("torch", "dsc_geglu")}


@pytest.mark.parametrize("M,N,K", [(1024, 320, 320), (256, 320, 1920)])
@pytest.mark.parametrize("bias", ["fp32", "2-byte offset"])
def test_a_bias_the_kernels_cannot_read_reaches_none_of_them(M, N, K, bias):
    """the C ABI sees no dtypes and refuses a bias that is not 16-byte aligned: both take the torch route, at the kernel's shape and
    at the split-K one"""
    b = routes.fake(N, dtype=torch.float32) if bias == "fp32" else routes.fake(N + 1)[1:]
    for prefer in (False, True):
        with routes.faked() as lib:
            ops.linear(routes.fake(M, K), routes.fake(N, K), b, prefer_kernel=prefer)
        assert [name for name, _ in lib.calls] == ["torch"]


def test_geglu_with_a_residual_is_refused():
    with routes.faked() as lib:
        with pytest.raises(ValueError):
            ops.linear(routes.fake(128, 320), routes.fake(640, 320), routes.fake(640), residual=routes.fake(128, 320), geglu=True)
    assert not lib.calls


def test_linear_qkv_covers_answers_both_ways(recorded):
    answers = {row[3] for row in recorded["default"].values()}
    assert answers == {True, False}


@pytest.mark.parametrize("shape", [(128, 32), (128, 128), (2, 64, 32), (2, 64, 128)])
@pytest.mark.parametrize("entry", ["linear", "linear_ln", "linear_qkv", "linear_gn", "linear_kernel_can"])
def test_an_x_that_does_not_match_the_weight_is_refused_before_any_launch(entry, shape):
    """x [..., 32] or [..., 128] against weight [N, 64] holds half or twice the elements the launch would read: a RuntimeError
    (what x.reshape(M, K) and F.linear raised) from every entry, with the library on or off, and nothing launched"""
    x, w, b = routes.fake(*shape), routes.fake(192, 64), routes.fake(192)
    call = {"linear": lambda: ops.linear(x, w, b, prefer_kernel=True), "linear_ln": lambda: ops.linear_ln(x, w, b),
            "linear_qkv": lambda: ops.linear_qkv(x.reshape(2, 64, -1), w, b, 1), "linear_kernel_can": lambda: ops.linear_kernel_can(x, w, b, None),
            "linear_gn": lambda: ops.linear_gn(x.reshape(2, 64, -1), w, b, None, 64, 32)}[entry]
    for setting in ("default", "library"):
        with routes.faked(**routes.SETTINGS[setting]) as lib:
            with pytest.raises(RuntimeError):
                call()
        assert not lib.calls


def test_the_residual_is_looked_at_once(monkeypatch):
    """ops._residual_2d runs at most once per ops.linear call, whatever the route"""
    calls = []
    inner = ops._residual_2d
    monkeypatch.setattr(ops, "_residual_2d", lambda *a: calls.append(a) or inner(*a))
    for switches in routes.SETTINGS.values():
        with routes.faked(**switches):
            for _, x, w, b, r, geglu, prefer in routes.cases():
                del calls[:]
                ops.linear(x, w, b, residual=r, geglu=geglu, prefer_kernel=prefer)
                assert len(calls) <= (r is not None)
