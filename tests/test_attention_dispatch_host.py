"""The one place that routes an attention call (attention_modify.attention_plan), without a device: every case of
tests/golden/make_attention_routes.py replayed through the four public processors and scaled_dot_product_attention_regionstate
against the recorded table (entry points, integer arguments, strides, flag words, sigma and pointer forms, library-route markers
and exception types), the routes the plan can return, and its refusals."""
import pytest
import torch

import make_attention_routes as routes
from diffusionspatialcontrol_amd import ops
from diffusionspatialcontrol_amd.modules import attention_modify as am


@pytest.fixture(scope="module")
def recorded():
    return routes.load()


@pytest.fixture(scope="module")
def replayed():
    """(rows, the routes attention_plan returned) over all cases, run once"""
    seen, plan = set(), am.attention_plan

    def logged(**facts):
        route = plan(**facts)
        seen.add(route)
        return route

    am.attention_plan = logged
    try:
        return routes.record_all(), seen
    finally:
        am.attention_plan = plan


def test_routes_match_the_recording(recorded, replayed):
    got = replayed[0]
    assert sorted(got) == sorted(recorded)
    wrong = {cid: (row, recorded[cid]) for cid, row in got.items() if row != recorded[cid]}
    assert not wrong, (len(wrong), next(iter(wrong.items())))


def test_every_route_is_reached(replayed):
    assert replayed[1] == set(am.ROUTES) and len(set(am.ROUTES)) == len(am.ROUTES)


REFUSALS = [
    ("processor S=77 region=dense per_group=True mask=True processor=AttnProcessor", NotImplementedError, "per-group sigma: attention masks"),
    ("processor S=77 region=dense kv=none wf=custom per_group=True", NotImplementedError, "per-group sigma: a custom weight_func"),
    ("processor S=97 region=dense kv=none wf=none mask=True processor=AttnProcessor", NotImplementedError, "attention masks with more than"),
    ("processor S=154 region=dense kv=none wf=none per_group=True", NotImplementedError, "need the chunked prepared-operand kernels"),
    ("processor S=154 region=many kv=packed wf=none per_group=True", NotImplementedError, "need the chunked prepared-operand kernels"),
    ("functional S=77 d=40 is_causal=True", NotImplementedError, "is_causal / dropout"),
    ("functional S=77 d=40 dropout_p=0.1", NotImplementedError, "is_causal / dropout"),
    ("processor S=77 region=dense kv=none per_group=short", ValueError, "per_group_sigma needs a dense"),
    ("processor S=77 region=compressed kv=packed per_group=short", ValueError, "per_group_sigma needs a dense"),
    ("processor S=77 region=dense table_L=128", ValueError, "region table .* does not match"),
    ("processor S=77 region=dense wf=none mask=short processor=AttnProcessor", ValueError, "mask .* does not broadcast"),
    ("IPAdapterAttnProcessor tokens=(4,) masks=list", ValueError, "ip_adapter_mask should be a tensor"),
    ("IPAdapterAttnProcessor tokens=(4,) masks=count", ValueError, "must match number of IP-Adapters"),
    ("IPAdapterAttnProcessor tokens=(4,) rows=plain masks=good", ValueError, "not supported with prepared IP-Adapter rows"),
    ("IPAdapterAttnProcessor tokens=(4,) rows=adapters", ValueError, "the processor holds 1"),
    ("IPAdapterAttnProcessor tokens=(257,) rows=plain", ValueError, "257 image tokens"),
    ("IPAdapterAttnProcessor tokens=(4,) rows=plain d=168", ValueError, "head dim 168"),
    ("processor S=77 region=dense level=128", KeyError, "64"),
    ("IPAdapterAttnProcessor tokens=(4,) rows=dict-miss", KeyError, "64"),
]


@pytest.mark.parametrize("cid,error,text", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_each_refusal_is_seen(recorded, cid, error, text):
    """every NotImplementedError, ValueError and KeyError of the routing, by the case that meets it: recorded, and raised with
    its own message"""
    assert recorded[cid][1] == error.__name__
    run = dict(routes.cases())[cid]
    with routes.faked():
        with pytest.raises(error, match=text):
            run()


def test_the_limits_are_stated_once():
    """the plan and the wrappers read the key and head-dim limits from ops: moving one moves the routes"""
    facts = dict(d=40, dtype=torch.float16, table=True, packed=True)
    assert am.attention_plan(S=ops.XATTN_MAX_KEYS, **facts) == am.attention_plan(S=ops.XATTN_MAX_KEYS_PACKED, **facts) == am.ROUTE_REGION_PACKED
    assert am.attention_plan(S=ops.XATTN_MAX_KEYS_PACKED + 1, **facts) == am.ROUTE_REGION_LONG
    assert ops.attn_kernel_takes(torch.float16, ops.ATTN_MAX_HEAD_DIM) and not ops.attn_kernel_takes(torch.float16, ops.ATTN_MAX_HEAD_DIM + 8)
    assert not ops.attn_kernel_takes(torch.float32, 40) and not ops.attn_head_dim_ok(36)
    assert ops.xattn_kv_packable(ops.XATTN_MAX_KEYS_PACKED, 160) and not ops.xattn_kv_packable(ops.XATTN_MAX_KEYS_PACKED + 1, 160)
    with routes.faked() as lib:         # the fake library states the kernels' rule (region_xattn_packed.hip) on its own
        for S in routes.KEYS:
            for d in routes.HEAD_DIMS:
                assert ops.xattn_kv_packable(S, d) == bool(lib.dsc_xattn_kv_pack_bytes(2, 2, S, d))


def test_the_weight_func_is_probed_once_per_call(monkeypatch):
    calls = []
    inner = am.weight_func_is_default
    monkeypatch.setattr(am, "weight_func_is_default", lambda wf: calls.append(wf) or inner(wf))
    with routes.faked():
        for cid, run in list(routes.cases())[::5]:
            if "wf=none" in cid or "wf=" not in cid:
                continue
            del calls[:]
            routes.record(run)
            assert len(calls) <= 1, cid
