"""The sampler step's host side against the table recorded at the parent of the change that gave it one step plan
(tests/golden/make_step_records.py, which says what a row holds): every record the batcher hands its executor and every sampler
launch of the fused loop, for the ten fused samplers, both parameterisations, with and without a rescale.  Floats compare equal or
within 2 ulp of double (another machine's libm may round exp / log / expm1 differently); the mistakes this is here to catch - a
neighbouring call's scalar, a sigma that was or was not rounded to fp16, swapped fields, the wrong terminal triple - are many
orders of magnitude larger."""
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_step_records as gold  # noqa: E402

ULPS = 2          # (with 0 - bit equality - the test passes on the machine that wrote the file)


def _differences(got, want, path, out):
    if isinstance(want, float) and isinstance(got, float):
        if got != want and not abs(got - want) <= ULPS * math.ulp(want):
            out.append(f"{path}: {got!r} != {want!r}")
    elif isinstance(want, list) and isinstance(got, list) and len(got) == len(want):
        for i, (g, w) in enumerate(zip(got, want)):
            _differences(g, w, f"{path}[{i}]", out)
    elif isinstance(want, dict) and isinstance(got, dict) and set(got) == set(want):
        for k in want:
            _differences(got[k], want[k], f"{path}.{k}", out)
    elif type(got) is not type(want) or got != want:
        out.append(f"{path}: {got!r} != {want!r}")


@pytest.fixture(scope="module")
def recorded():
    return gold.load()


def test_the_cases_are_the_recorded_ones(recorded):
    assert [case[0] for case in gold.cases()] == list(recorded)


@pytest.mark.parametrize("half", ["serve", "fused"])
def test_records_equal_the_recorded_table(recorded, half):
    wrong = []
    for cid, fn, args, kw in gold.cases():
        if cid.startswith(half):
            _differences(gold.norm(fn(*args, **kw)), recorded[cid], cid, wrong)
    assert not wrong, f"{len(wrong)} differences, the first: " + "; ".join(wrong[:5])


def test_packing_round_trips():
    rows = {"a": [[{"mode": 0, "sigma": 0.1, "noise": ["noise", "A", 1], "req": "A"}, {"mode": 2, "req": None}], None,
                  {"image": ["image", "A"], "blend_now": True}], "b": {"base": [1.5, -0.0, 1e-10], "hires": []}}
    assert gold.unpack(gold.pack(rows)) == rows
    assert math.copysign(1.0, gold.unpack(gold.pack(rows))["b"]["base"][1]) == -1.0
