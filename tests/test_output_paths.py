"""Output paths of the attention kernels and the contract of every op that writes into a caller-supplied tensor.

Store paths.  `store_o_block` (csrc/dsc_common.h) writes an attention output block either as 16-byte pieces after a
v_permlane32_swap exchange (`wide`: out pointer 16-byte aligned, strides multiples of 8 halves) or as 8-byte pieces
(out only 8-byte aligned; the packed kernel's debug flag 1024 forces it).  The generic region kernel has its own 8-byte
store.  Each destination below is a view into a sentinel-filled buffer; with the pointer / strides it gives, the path is

    destination                         self_attention / region_xattn_packed     region_xattn (generic)
    fresh (out=None)                    wide                                     8-byte store, 16-byte aligned
    offset: 4 halves into a buffer      narrow (8-byte aligned pointer)          8-byte store, 8-byte aligned
    strided: rows padded by 8 halves    wide, non-contiguous                     8-byte store, non-contiguous
    strided + offset 4 halves           narrow, non-contiguous                   8-byte store, 8-byte aligned
    packed, debug_flags=1024            narrow (forced)                          -
    rows padded by 4 halves             refused by the C entry point (DscLibraryError) before any launch

and every result must equal the fresh run bit for bit, leave every element outside the view at the sentinel, and (the fresh
run) meet the bounds of test_region_xattn_gpu.py / test_self_attention against a high-precision reference.

Destinations.  The wrappers refuse an `out=` (and the sampler kernels' buffers) of the wrong shape, dtype or device before
the library is reached: those tests run against a stub library whose entry points fail the test when called, so a
regression fails there instead of writing out of bounds on the GPU.

GroupNorm partial sums.  attach_gn_partials' contract: every op that writes through `out=` or in place drops the partial
sums riding on its destination.  WRITERS lists those ops; a CPU test keeps the list complete (every public op with an `out`
parameter) and checks, from the source, that each writer calls `_drop_gn_partials` on each destination.
"""
import ast
import inspect
import math
import textwrap

import pytest
import torch

from inputs import attn_inputs
from oracle import region_attention as ra
from test_region_xattn_gpu import ATOL16, ATOL32, tol16

from diffusionspatialcontrol_amd import _lib
from diffusionspatialcontrol_amd import ops as dsc_ops

SENTINEL = 0x7E5A          # an fp16 NaN bit pattern: no kernel stores it
S_KEYS = 77

# every op that writes into a tensor the caller owns -> the parameters naming those tensors
WRITERS = {
    "self_attention": ("out",),
    "region_xattn": ("out",),
    "region_xattn_packed": ("out",),
    "softmax_rows": ("out",),
    "xattn_kv_pack": ("out",),
    "prepare_unet_input": ("x_in",),
    "cfg_dpmpp2m_step": ("x", "old", "x_in"),
}
# helpers that write for them: the sampler kernels' row broadcast destination
HELPER_WRITERS = {"_row_args": ("dst",)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return dsc_ops


# ----------------------------------------------------------------------------- store paths
# (B, H, L, d): d over the head widths of SD 1.5 / SDXL plus the extremes the kernels take; L multiples of 32 and not
SHAPES = [(2, 8, 4000, 40), (2, 8, 1000, 80), (2, 4, 100, 64), (2, 4, 256, 160), (2, 2, 100, 8), (2, 2, 1024, 8)]
# (name, row pad in halves, offset in halves, wide path expected for the store_o_block kernels)
DESTS = [("offset", 0, 4, False), ("strided", 8, 0, True), ("strided_offset", 8, 4, False)]


def _dest(shape, row_dims, pad, shift):
    """(buf, out): `out` a [shape] view of a sentinel-filled flat fp16 buffer whose rows (the last `row_dims` dims) are
    padded by `pad` halves, starting `shift` halves into the buffer; 8 sentinel halves follow the last row"""
    lead, tail = shape[:-row_dims], shape[-row_dims:]
    row = math.prod(tail)
    n = math.prod(lead) * (row + pad)
    buf = torch.full((shift + n + 8,), SENTINEL, dtype=torch.int16, device="cuda").view(torch.float16)
    out = buf[shift:shift + n].view(*lead, row + pad)[..., :row].unflatten(-1, tail)
    return buf, out


def _untouched_outside(buf, out):
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    inside.as_strided(out.shape, out.stride(), out.storage_offset()).fill_(True)
    return bool((buf.view(torch.int16)[~inside] == SENTINEL).all())


def _check_destinations(run, ref, row_dims):
    """run(out) into every destination of DESTS: the fresh result `ref` bit for bit, nothing written outside the view; a row
    stride that is not a multiple of 8 halves is refused before any launch"""
    shape = tuple(ref.shape)
    for name, pad, shift, wide in DESTS:
        buf, out = _dest(shape, row_dims, pad, shift)
        assert (out.data_ptr() % 16 == 0) == wide and out.data_ptr() % 8 == 0 and out.is_contiguous() == (pad == 0), name
        got = run(out)
        assert got.data_ptr() == out.data_ptr(), name
        assert torch.equal(out, ref), (name, (out.float() - ref.float()).abs().max().item())
        assert _untouched_outside(buf, out), name
    buf, out = _dest(shape, row_dims, 4, 0)
    with pytest.raises(_lib.DscLibraryError):
        run(out)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == SENTINEL).all())


def _sdpa_fp64(q, k, v):
    """softmax(q k^T / sqrt(d)) v in fp64 for [B, L, H, d] views -> [B, L, H, d]"""
    qd, kd, vd = (t.double().transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qd @ kd.transpose(-1, -2) / math.sqrt(q.shape[-1]), dim=-1)
    return (p @ vd).transpose(1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,L,d", SHAPES)
def test_self_attention_store_paths(ops, B, H, L, d):
    g = torch.Generator().manual_seed(L * d + H + 7)
    C = H * d
    qkv = torch.randn(B, L, 3 * C, generator=g).half().cuda()
    q, k, v = (qkv[..., i * C:(i + 1) * C].unflatten(-1, (H, d)) for i in range(3))
    ref = ops.self_attention(q, k, v)
    assert ref.data_ptr() % 16 == 0 and ref.is_contiguous()
    err = (ref.double() - _sdpa_fp64(q, k, v)).abs()
    assert err.max().item() < 2e-3 and err.mean().item() < 2e-4, (err.max().item(), err.mean().item())   # test_self_attention
    _check_destinations(lambda out: ops.self_attention(q, k, v, out=out), ref, 2)


def _region_case(Bc, H, L, d, with_region):
    x = attn_inputs(f"store/{Bc}/{H}/{L}/{d}", Bc=Bc, H=H, L=L, S=S_KEYS, d=d)
    q, k, v, w = (torch.from_numpy(x[n]) for n in ("q", "k", "v", "w"))
    return q, k, v, (w if with_region else torch.zeros_like(w))


def _assert_oracle(out_bhld, q, k, v, w, ref16, with_region, sigma):
    """the bounds test_region_xattn_gpu.py holds the kernels to: fp16-rounding mode against the rounding oracle (tol16, mean
    3e-4), the fp32-score mode against the fp32 oracle (ATOL32, mean 4e-4; ATOL16 without a table, as plain SDPA)"""
    exp = ra.region_attention(q, k, v, w, sigma, fp16_rounding=ref16)
    err = (out_bhld.float().cpu() - exp).abs()
    bound = tol16(q, k, w, sigma) if ref16 else (ATOL32 if with_region else ATOL16)
    assert err.max().item() < bound, (err.max().item(), bound)
    assert err.mean().item() < (3e-4 if ref16 else 4e-4), err.mean().item()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["bhld", "blhd"])
@pytest.mark.parametrize("with_region", [True, False])
@pytest.mark.parametrize("ref16", [True, False])
@pytest.mark.parametrize("Bc,H,L,d", SHAPES)
def test_region_xattn_store_paths(ops, Bc, H, L, d, ref16, with_region, layout):
    sigma = 2.0
    q, k, v, w = _region_case(Bc, H, L, d, with_region)
    qd, kd, vd = q.cuda().half(), k.cuda().half(), v.cuda().half()
    if layout == "blhd":
        qd, kd, vd = qd.transpose(1, 2), kd.transpose(1, 2), vd.transpose(1, 2)
    region = w.cuda() if with_region else None

    def run(out):
        return ops.region_xattn(qd, kd, vd, region, sigma, layout=layout, ref_fp16_rounding=ref16, out=out)

    ref = run(None)
    _assert_oracle(ref if layout == "bhld" else ref.transpose(1, 2), q, k, v, w, ref16, with_region, sigma)
    _check_destinations(run, ref, 1 if layout == "bhld" else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("with_region", [True, False])
@pytest.mark.parametrize("ref16", [True, False])
@pytest.mark.parametrize("Bc,H,L,d", SHAPES)
def test_region_xattn_packed_store_paths(ops, Bc, H, L, d, ref16, with_region):
    sigma = 2.0
    q, k, v, w = _region_case(Bc, H, L, d, with_region)
    qd, kd, vd = q.cuda().half(), k.cuda().half(), v.cuda().half()
    packed = ops.xattn_kv_pack(kd, vd, layout="bhld")
    region = ops.compress_region_table(w.cuda()) if with_region else None
    assert region is not None or not with_region
    q4 = qd.transpose(1, 2)

    def run(out, flags=0):
        return ops.region_xattn_packed(q4, packed, S_KEYS, region, sigma, ref_fp16_rounding=ref16, out=out, debug_flags=flags)

    ref = run(None)
    assert ref.data_ptr() % 16 == 0 and ref.is_contiguous()
    assert torch.equal(run(None, 1024), ref)                 # 8-byte pieces forced on the aligned destination
    _assert_oracle(ref.transpose(1, 2), q, k, v, w, ref16, with_region, sigma)
    _check_destinations(run, ref, 2)
    buf, out = _dest(tuple(ref.shape), 2, 8, 0)               # forced narrow path on a strided destination
    run(out, 1024)
    assert torch.equal(out, ref) and _untouched_outside(buf, out)


# ----------------------------------------------------------------------------- destination validation
class _NoLaunchLibrary:
    """stands in for libdsc_hip.so: any entry point reached fails the test (validation must have refused the call)"""

    def __getattr__(self, name):
        def launched(*args, **kwargs):
            pytest.fail(f"kernel launched: {name} reached with a malformed destination")
        return launched


def _h(*shape, device="cuda", dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype, device=device)


def _malformed_calls():
    """id -> (call, exception): each call hands one wrapper one malformed destination"""
    o = dsc_ops
    q4 = _h(2, 64, 2, 8)                           # [B, L, H, d]
    qb = _h(2, 2, 64, 8)                           # [B, H, L, d]
    packed = _h(4096)
    s = _h(8, 64)
    x, eps, old, x_in = _h(2, 4, 8, 8), _h(4, 4, 8, 8), _h(2, 4, 8, 8), _h(4, 4, 8, 8)
    t_buf, sig = _h(4, dtype=torch.float32), _h(1, dtype=torch.float32)
    ragged = _h(2, 4, 8, 16)[..., :8]              # right shape, not contiguous

    def prep(**kw):
        a = dict(x=x, x_in=x_in, t_buf=t_buf, sigma_buf=sig)
        a.update(kw)
        return lambda: o.prepare_unet_input(a["x"], 0.5, 10.0, 1.0, a["x_in"], a["t_buf"], a["sigma_buf"], row=kw.get("row"))

    def step(**kw):
        a = dict(x=x, eps=eps, old=old, x_in=x_in, t_buf=t_buf, sigma_buf=sig)
        a.update(kw)
        return lambda: o.cfg_dpmpp2m_step(a["x"], a["eps"], a["old"], 1.0, 7.5, 0.5, 0.5, 0.0, 1.0, 10.0, 1.0, a["x_in"],
                                          a["t_buf"], a["sigma_buf"], row=kw.get("row"))

    return {
        "self_attention/too_small": (lambda: o.self_attention(q4, q4, q4, out=_h(2, 63, 2, 8)), ValueError),
        "self_attention/head_major": (lambda: o.self_attention(q4, q4, q4, out=_h(2, 2, 64, 8)), ValueError),
        "self_attention/fp32": (lambda: o.self_attention(q4, q4, q4, out=_h(2, 64, 2, 8, dtype=torch.float32)), TypeError),
        "self_attention/cpu": (lambda: o.self_attention(q4, q4, q4, out=_h(2, 64, 2, 8, device="cpu")), ValueError),
        "region_xattn/too_small": (lambda: o.region_xattn(qb, qb, qb, out=_h(2, 2, 32, 8)), ValueError),
        "region_xattn/blhd_given_bhld": (lambda: o.region_xattn(q4, q4, q4, layout="blhd", out=_h(2, 2, 64, 8)), ValueError),
        "region_xattn/fp32": (lambda: o.region_xattn(qb, qb, qb, out=_h(2, 2, 64, 8, dtype=torch.float32)), TypeError),
        "region_xattn/cpu": (lambda: o.region_xattn(qb, qb, qb, out=_h(2, 2, 64, 8, device="cpu")), ValueError),
        "region_xattn_packed/too_small": (lambda: o.region_xattn_packed(q4, packed, 16, out=_h(2, 64, 1, 8)), ValueError),
        "region_xattn_packed/fp32": (lambda: o.region_xattn_packed(q4, packed, 16, out=_h(2, 64, 2, 8, dtype=torch.float32)),
                                     TypeError),
        "region_xattn_packed/cpu": (lambda: o.region_xattn_packed(q4, packed, 16, out=_h(2, 64, 2, 8, device="cpu")), ValueError),
        "softmax_rows/too_few_rows": (lambda: o.softmax_rows(s, out=_h(7, 64)), ValueError),
        "softmax_rows/too_narrow": (lambda: o.softmax_rows(s, out=_h(8, 32)), ValueError),
        "softmax_rows/fp32": (lambda: o.softmax_rows(s, out=_h(8, 64, dtype=torch.float32)), TypeError),
        "softmax_rows/cpu": (lambda: o.softmax_rows(s, out=_h(8, 64, device="cpu")), ValueError),
        "softmax_rows/transposed": (lambda: o.softmax_rows(s, out=_h(64, 8).t()), ValueError),
        "prepare_unet_input/x_fp32": (prep(x=_h(2, 4, 8, 8, dtype=torch.float32)), TypeError),
        "prepare_unet_input/x_not_contiguous": (prep(x=ragged), ValueError),
        "prepare_unet_input/x_in_one_row_short": (prep(x_in=_h(3, 4, 8, 8)), ValueError),
        "prepare_unet_input/x_in_short_rows": (prep(x_in=_h(4, 4, 8, 4)), ValueError),
        "prepare_unet_input/x_in_fp32": (prep(x_in=_h(4, 4, 8, 8, dtype=torch.float32)), TypeError),
        "prepare_unet_input/x_in_not_contiguous": (prep(x_in=_h(4, 4, 8, 16)[..., :8]), ValueError),
        "prepare_unet_input/x_in_cpu": (prep(x_in=_h(4, 4, 8, 8, device="cpu")), _lib.DscLibraryError),
        "prepare_unet_input/t_buf_short": (prep(t_buf=_h(3, dtype=torch.float32)), ValueError),
        "prepare_unet_input/t_buf_fp16": (prep(t_buf=_h(4)), TypeError),
        "prepare_unet_input/sigma_buf_empty": (prep(sigma_buf=_h(0, dtype=torch.float32)), ValueError),
        "prepare_unet_input/sigma_buf_fp16": (prep(sigma_buf=_h(1)), TypeError),
        "prepare_unet_input/row_dst_narrow": (prep(row=(_h(16), _h(2, 8))), ValueError),
        "cfg_dpmpp2m_step/eps_one_image": (step(eps=_h(2, 4, 8, 8)), ValueError),
        "cfg_dpmpp2m_step/eps_fp32": (step(eps=_h(4, 4, 8, 8, dtype=torch.float32)), TypeError),
        "cfg_dpmpp2m_step/eps_not_contiguous": (step(eps=_h(4, 4, 8, 16)[..., :8]), ValueError),
        "cfg_dpmpp2m_step/eps_cpu": (step(eps=_h(4, 4, 8, 8, device="cpu")), _lib.DscLibraryError),
        "cfg_dpmpp2m_step/x_not_contiguous": (step(x=ragged), ValueError),
        "cfg_dpmpp2m_step/old_short": (step(old=_h(2, 4, 8, 4)), ValueError),
        "cfg_dpmpp2m_step/old_other_shape": (step(old=_h(2, 4, 4, 16)), ValueError),
        "cfg_dpmpp2m_step/old_fp32": (step(old=_h(2, 4, 8, 8, dtype=torch.float32)), TypeError),
        "cfg_dpmpp2m_step/x_in_one_row_short": (step(x_in=_h(3, 4, 8, 8)), ValueError),
        "cfg_dpmpp2m_step/t_buf_long": (step(t_buf=_h(5, dtype=torch.float32)), ValueError),
        "cfg_dpmpp2m_step/sigma_buf_fp16": (step(sigma_buf=_h(1)), TypeError),
        "cfg_dpmpp2m_step/row_dst_fp32": (step(row=(_h(16), _h(2, 16, dtype=torch.float32))), ValueError),
    }


MALFORMED = ["self_attention/too_small", "self_attention/head_major", "self_attention/fp32", "self_attention/cpu",
             "region_xattn/too_small", "region_xattn/blhd_given_bhld", "region_xattn/fp32", "region_xattn/cpu",
             "region_xattn_packed/too_small", "region_xattn_packed/fp32", "region_xattn_packed/cpu",
             "softmax_rows/too_few_rows", "softmax_rows/too_narrow", "softmax_rows/fp32", "softmax_rows/cpu",
             "softmax_rows/transposed",
             "prepare_unet_input/x_fp32", "prepare_unet_input/x_not_contiguous", "prepare_unet_input/x_in_one_row_short",
             "prepare_unet_input/x_in_short_rows", "prepare_unet_input/x_in_fp32", "prepare_unet_input/x_in_not_contiguous",
             "prepare_unet_input/x_in_cpu", "prepare_unet_input/t_buf_short", "prepare_unet_input/t_buf_fp16",
             "prepare_unet_input/sigma_buf_empty", "prepare_unet_input/sigma_buf_fp16", "prepare_unet_input/row_dst_narrow",
             "cfg_dpmpp2m_step/eps_one_image", "cfg_dpmpp2m_step/eps_fp32", "cfg_dpmpp2m_step/eps_not_contiguous",
             "cfg_dpmpp2m_step/eps_cpu", "cfg_dpmpp2m_step/x_not_contiguous", "cfg_dpmpp2m_step/old_short",
             "cfg_dpmpp2m_step/old_other_shape", "cfg_dpmpp2m_step/old_fp32", "cfg_dpmpp2m_step/x_in_one_row_short",
             "cfg_dpmpp2m_step/t_buf_long", "cfg_dpmpp2m_step/sigma_buf_fp16", "cfg_dpmpp2m_step/row_dst_fp32"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MALFORMED)
def test_malformed_destination_is_refused_before_any_launch(ops, monkeypatch, case):
    calls = _malformed_calls()
    assert sorted(calls) == sorted(MALFORMED)
    call, exc = calls[case]
    monkeypatch.setattr(_lib, "_LIB", _NoLaunchLibrary())
    with pytest.raises(exc):
        call()


@pytest.mark.gpu
def test_well_formed_destinations_still_launch(ops):
    """the checks accept what the pipeline passes: in-place softmax (vae_decoder.py), a padded-row softmax destination, the
    sampler buffers of the fused loop with a 1-D fp32 t_buf and a longer sigma_buf"""
    g = torch.Generator().manual_seed(3)
    s = (torch.randn(8, 64, generator=g) * 4).half().cuda()
    ref = ops.softmax_rows(s)
    wide = torch.full((8, 72), SENTINEL, dtype=torch.int16, device="cuda").view(torch.float16)
    assert torch.equal(ops.softmax_rows(s, out=wide[:, :64]), ref) and bool((wide[:, 64:].view(torch.int16) == SENTINEL).all())
    assert torch.equal(ops.softmax_rows(s, out=s), ref)
    x = torch.randn(1, 4, 8, 8, generator=g).half().cuda()
    x_in, t_buf, sig = torch.zeros(2, 4, 8, 8, dtype=torch.half, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(3, device="cuda")
    ops.prepare_unet_input(x, 0.5, 10.0, 2.0, x_in, t_buf, sig)
    assert torch.equal(x_in, torch.cat([x, x]) * 0.5) and t_buf.tolist() == [10.0, 10.0] and sig.tolist() == [2.0, 0.0, 0.0]


# ----------------------------------------------------------------------------- GroupNorm partial sums
def _dummy_partials(t):
    return dsc_ops.GnPartials(torch.zeros(4, dtype=torch.float32, device=t.device), 1, 1, 1, 1, 1)


def _writer_call(o, name):
    """(call, destinations) for one writer on small well-formed operands"""
    g = torch.Generator().manual_seed(17)
    r = lambda *shape: (torch.randn(shape, generator=g) * 0.5).half().cuda()  # noqa: E731
    if name == "self_attention":
        q4, out = r(1, 64, 2, 8), r(1, 64, 2, 8)
        return (lambda: o.self_attention(q4, q4, q4, out=out)), [out]
    if name == "region_xattn":
        qb, kb, out = r(1, 2, 64, 8), r(1, 2, 16, 8), r(1, 2, 64, 8)
        return (lambda: o.region_xattn(qb, kb, kb, out=out)), [out]
    if name == "region_xattn_packed":
        q4, kb, out = r(1, 64, 2, 8), r(1, 2, 16, 8), r(1, 64, 2, 8)
        packed = o.xattn_kv_pack(kb, kb, layout="bhld")
        return (lambda: o.region_xattn_packed(q4, packed, 16, out=out)), [out]
    if name == "softmax_rows":
        s, out = r(8, 64), r(8, 64)
        return (lambda: o.softmax_rows(s, out=out)), [out]
    if name == "softmax_rows/in_place":
        s = r(8, 64)
        return (lambda: o.softmax_rows(s, out=s)), [s]
    if name == "xattn_kv_pack":
        kb = r(1, 2, 16, 8)
        out = o.xattn_kv_pack(kb, kb, layout="bhld").zero_()
        return (lambda: o.xattn_kv_pack(kb, kb, layout="bhld", out=out)), [out]
    x, old, eps, x_in = r(1, 4, 8, 8), r(1, 4, 8, 8), r(2, 4, 8, 8), r(2, 4, 8, 8)
    t_buf, sig = torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda")
    src, dst = r(16), r(2, 16)
    if name == "prepare_unet_input":
        return (lambda: o.prepare_unet_input(x, 0.5, 10.0, 1.0, x_in, t_buf, sig, row=(src, dst))), [x_in, dst]
    assert name == "cfg_dpmpp2m_step", name
    return (lambda: o.cfg_dpmpp2m_step(x, eps, old, 1.0, 7.5, 0.5, 0.5, 0.1, 1.0, 10.0, 1.0, x_in, t_buf, sig,
                                       row=(src, dst))), [x, old, x_in, dst]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WRITERS) + ["softmax_rows/in_place"])
def test_writers_drop_groupnorm_partials(ops, name):
    """a raw-pointer write does not bump torch's version counter, so a writer that kept the sums on its destination would hand
    the next GroupNorm statistics of the bytes before the write"""
    call, dests = _writer_call(ops, name)
    for t in dests:
        ops.attach_gn_partials(t, _dummy_partials(t))
        assert ops.gn_partials_of(t) is not None
    before = [t.clone() for t in dests]
    call()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, t) for a, t in zip(before, dests)), "the call wrote nothing"
    for i, t in enumerate(dests):
        assert ops.gn_partials_of(t) is None, (name, i)


def _drop_targets(fn):
    tree = ast.parse(textwrap.dedent(inspect.getsource(fn)))
    return {c.args[0].id for c in ast.walk(tree) if isinstance(c, ast.Call) and getattr(c.func, "id", None) == "_drop_gn_partials"
            and c.args and isinstance(c.args[0], ast.Name)}


def test_every_writer_is_under_the_partials_contract():
    """no GPU: every public op with an `out` parameter is in WRITERS (so test_writers_drop_groupnorm_partials covers it), and
    every writer calls _drop_gn_partials on each destination it writes"""
    public = {n: f for n, f in vars(dsc_ops).items()
              if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == dsc_ops.__name__}
    with_out = {n for n, f in public.items() if "out" in inspect.signature(f).parameters}
    assert "self_attention" in with_out and "softmax_rows" in with_out
    assert with_out <= set(WRITERS), sorted(with_out - set(WRITERS))
    for name, dests in list(WRITERS.items()) + list(HELPER_WRITERS.items()):
        missing = set(dests) - _drop_targets(getattr(dsc_ops, name))
        assert not missing, (name, sorted(missing))
    for name in ("prepare_unet_input", "cfg_dpmpp2m_step"):                    # their row broadcast goes through _row_args
        assert "_row_args(row" in inspect.getsource(getattr(dsc_ops, name)), name
