"""Every product counted once: the GEMM and convolution entry points of include/dsc_hip.h on operands where exactly one output is
correct (tests/exact_inputs.py), compared with `torch.equal` - no tolerance anywhere in this file.

The tolerance tests (|err| <= 1.5e-3 |ref| + 2e-3 on randn operands) and the variant-against-variant comparisons do not see a term
that is lost, doubled or misplaced for a few elements, or a defect every variant shares: tests/test_exact_sums_host.py shows the
shares.  Here the operands are small integers (regime "integer": nothing rounds, and the producers' GroupNorm / LayerNorm statistics
are exact integers too) or the same integers times powers of two (regime "dyadic": the fp32 sum is still exact and the epilogue's one
fp16 rounding, after bias and residual, is the only rounding), so the fp64 reference rounded once is the one correct tensor under
every ring depth, tile shape, split and launch profile.  The cases are exact_inputs.CASES, whose conditions the host file asserts.
An entry that refuses a case is asserted to refuse it.

Pinned: dsc_linear_f16 (with a wrapped residual), _splitk_f16, _qkv_f16 (no LayerNorm fold), _ln_f16 as producer, _gn_f16, _rows_f16,
_lt_f16; dsc_conv3x3_nhwc_f16 in every resample mode, _up2x_pack_f16 + _up2x_nhwc_f16, _gn_nhwc_f16, _fewcin_f16.
Not in scope, because nothing in them is exact: softmax / attention (numeric_ref.staircase_qkv prescribes probabilities there), GEGLU
and the LayerNorm-folded consumer (erf, rsqrt), GroupNorm apply."""
import pytest
import torch

import exact_inputs as E
import guard_band_refs as R
from test_guard_bands_gpu import CL, DSC_ERR_UNSUPPORTED, DSC_OK, GEMM_STAGES, _CONV_KW

pytestmark = pytest.mark.gpu

CONV_RINGS = ((401, 0), (3,), (9, 400), (9, 402))        # dsc_debug_set_conv_ring: the rule's own choice, three stages, nine, nine + loaders


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from diffusionspatialcontrol_amd import _lib
    return _lib.load_library()


@pytest.fixture
def variants(ops, lib):
    """variants(sweep) yields after switching the GEMM launch variant: the measured rule alone, or every dsc_debug_set_gemm_stages
    knob and then the rule under the throughput profile; knob and profile are back after the test, whatever it did"""
    before = ops.tuning_profile()

    def walk(sweep):
        for knob in GEMM_STAGES if sweep else (0,):
            lib.dsc_debug_set_gemm_stages(knob)
            yield knob
        if sweep:
            lib.dsc_debug_set_gemm_stages(0)
            ops.set_tuning_profile("throughput")
            yield "throughput"
            ops.set_tuning_profile(before)
    try:
        yield walk
    finally:
        lib.dsc_debug_set_gemm_stages(0)
        ops.set_tuning_profile(before)


@pytest.fixture
def conv_variants(ops, lib):
    """the same for the convolution: dsc_debug_set_conv_ring settings, then the throughput profile"""
    before = ops.tuning_profile()

    def walk(sweep):
        for ring in CONV_RINGS if sweep else CONV_RINGS[:1]:
            for setting in ring:
                lib.dsc_debug_set_conv_ring(setting)
            yield ring
        if sweep:
            for setting in CONV_RINGS[0]:
                lib.dsc_debug_set_conv_ring(setting)
            ops.set_tuning_profile("throughput")
            yield "throughput"
            ops.set_tuning_profile(before)
    try:
        yield walk
    finally:
        for setting in CONV_RINGS[0]:
            lib.dsc_debug_set_conv_ring(setting)
        ops.set_tuning_profile(before)


def _ids(cases):
    return [c.id for c in cases]


def _device(ref):
    """(the operands, the one correct output) on the GPU, moved once per case"""
    return {k: v.cuda() for k, v in ref.ops.items()}, ref.expected.cuda()


def _empty(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="cuda")


# ============================================================================= GEMM family (gemm.hip, temb.hip, linear_lt.hip)
@pytest.mark.parametrize("case", E.cases("linear"), ids=_ids(E.cases("linear")))
def test_linear_f16(ops, lib, variants, case):
    """dsc_linear_f16: rows on both sides of the 64- and 128-row tile edges, one to four column blocks, 1 / 4 / 11 / 80 K steps (the
    two- and three-stage rings wrap and end mid-ring), with and without bias + residual; a residual of 128 rows under 256 and 384"""
    M, N, K = case.shape
    d, want = _device(E.reference(case))
    ldr = (N | (case.get("res_rows") << 32)) if case.res else 0
    for variant in variants(case.sweep):
        out = _empty(M, N)
        rc = lib.dsc_linear_f16(ops._p(d["x"]), ops._p(d["w"]), ops._p(d.get("bias")), ops._p(d.get("res")), ops._p(out), M, N, K, K, ldr,
                                N, 0, 0, ops._stream_ptr(out))
        assert rc == DSC_OK, variant
        assert torch.equal(out, want), variant


@pytest.mark.parametrize("case", E.cases("splitk"), ids=_ids(E.cases("splitk")))
def test_linear_splitk_f16(ops, lib, variants, case):
    """dsc_linear_splitk_f16 on exactly dsc_linear_splitk_workspace_bytes: 11 K steps in 2, 3 and 4 splits (a shorter last split), 5
    steps asked in 4 splits - two steps each, so three splits run and the last has one"""
    M, N, K = case.shape
    splits = case.get("splits")
    d, want = _device(E.reference(case))
    nbytes = lib.dsc_linear_splitk_workspace_bytes(M, N, K, splits)
    kps = -(-(K // 64) // splits)
    assert nbytes == -(-(K // 64) // kps) * M * N * 4 and (K, splits, nbytes // (M * N * 4)) in ((704, 2, 2), (704, 3, 3), (704, 4, 4), (320, 4, 3))
    for variant in variants(case.sweep):
        out, ws = _empty(M, N), _empty(nbytes, dtype=torch.uint8)
        rc = lib.dsc_linear_splitk_f16(ops._p(d["x"]), ops._p(d["w"]), ops._p(d["bias"]), ops._p(d["res"]), ops._p(out), M, N, K, K, N, N,
                                       splits, ops._p(ws), nbytes, 0, ops._stream_ptr(out))
        assert rc == DSC_OK, variant
        assert torch.equal(out, want), variant


@pytest.mark.parametrize("case", E.cases("qkv"), ids=_ids(E.cases("qkv")))
def test_linear_qkv_f16(ops, lib, variants, case):
    """dsc_linear_qkv_f16 without a LayerNorm fold: q row-major, K / V head-major [2, B, heads, L, d] - every value where
    guard_band_refs.head_major puts it; 130 and 129 rows: images end inside a row tile, the last tile is ragged"""
    B, L, C, heads = case.shape
    M = B * L
    ref = E.reference(case)
    d, _ = _device(ref)
    want_q, want_kv = (t.contiguous().cuda() for t in R.head_major(ref.expected, B, L, heads))
    for variant in variants(case.sweep):
        q, kv = _empty(M, C), _empty(2, B, heads, L, C // heads)
        rc = lib.dsc_linear_qkv_f16(ops._p(d["x"]), ops._p(d["w"]), ops._p(d["bias"]), ops._p(q), ops._p(kv), M, C, C, C, C, heads, L,
                                    None, 0, None, 0.0, 0, ops._stream_ptr(q))
        assert rc == DSC_OK, variant
        assert torch.equal(q, want_q) and torch.equal(kv, want_kv), variant


@pytest.mark.parametrize("case", E.cases("ln"), ids=_ids(E.cases("ln")))
def test_linear_ln_f16_producer(ops, lib, variants, case):
    """dsc_linear_ln_f16 with ln_in null: the output in both regimes and, on integers, ln_out [M, N / 64, 2] equal to the fp64 (sum, sum
    of squares) of every 64-column block of the stored row - 291282 writes two statistics blocks per 128-column tile"""
    M, N, K = case.shape
    ref = E.reference(case)
    d, want = _device(ref)
    want_stats = R.row_block_stats(ref.expected)[0].float().cuda()
    for variant in variants(case.sweep):
        out, stats = _empty(M, N), _empty(M, N // 64, 2, dtype=torch.float32)
        rc = lib.dsc_linear_ln_f16(ops._p(d["x"]), ops._p(d["w"]), ops._p(d["bias"]), ops._p(d["res"]), ops._p(out), M, N, K, K, N, N, 0,
                                   None, 0, None, 0.0, ops._p(stats), 0, ops._stream_ptr(out))
        assert rc == DSC_OK, variant
        assert torch.equal(out, want), variant
        if case.regime == "integer":
            assert torch.equal(stats, want_stats), variant


def _equal_where_written(part, want):
    """the producers' partial sums against group_partials: every slot a producer writes (NaN in `want`: it writes none there)"""
    live = ~torch.isnan(want)
    return torch.equal(part[live], want[live].float())


@pytest.mark.parametrize("case", E.cases("gn"), ids=_ids(E.cases("gn")))
def test_linear_gn_f16(ops, lib, variants, case):
    """dsc_linear_gn_f16: the output and, on integers, gn_part [B, rows, G, 2, 2] in both `which` slots, at the row tile each launch
    variant takes.  A variant whose tile height does not divide the image's rows (128-row tiles under 64 or 192 rows) is refused."""
    B, L, K, N = case.shape
    M, groups = B * L, case.get("groups")
    ref = E.reference(case)
    d, want = _device(ref)
    ran = set()
    for variant in variants(case.sweep):
        rows = lib.dsc_linear_gn_rows(M, N, K, L, groups)
        out, part = _empty(M, N), _empty(B, max(rows, 1), groups, 2, 2, dtype=torch.float32)
        rc = lib.dsc_linear_gn_f16(ops._p(d["x"]), ops._p(d["w"]), ops._p(d["bias"]), ops._p(d["res"]), ops._p(out), M, N, K, K, N, N, L,
                                   ops._p(part), groups, 0, ops._stream_ptr(out))
        if rows == 0:
            assert rc == DSC_ERR_UNSUPPORTED, variant
            continue
        ran.add(L // rows)
        assert rc == DSC_OK and L // rows in (64, 128), variant
        assert torch.equal(out, want), variant
        if case.regime == "integer":
            want_part = E.group_partials(E.stored_rows(case, ref), *E.row_tiles(L, rows), groups).cuda()
            assert _equal_where_written(part, want_part), variant
    assert ran == ({64, 128} if L % 128 == 0 else {64})


@pytest.mark.parametrize("case", E.cases("rows"), ids=_ids(E.cases("rows")))
def test_linear_rows_f16(ops, lib, case):
    """dsc_linear_rows_f16 without SiLU or the sinusoid input: 1, 5 and 8 rows, K of 9 and 129 16-byte chunks over 64 lanes"""
    d, want = _device(E.reference(case))
    assert torch.equal(ops.linear_rows(d["x"], d["w"], d["bias"]), want)


def test_linear_lt_f16(ops, lib):
    """dsc_linear_lt_f16 (bias epilogue, residual as beta C): exact on integers like every fp32-accumulating GEMM; a build without the
    library refuses before any launch"""
    (case,) = E.cases("lt")
    M, N, K = case.shape
    d, want = _device(E.reference(case))
    out = _empty(M, N)
    rc = lib.dsc_linear_lt_f16(ops._p(d["x"]), ops._p(d["w"]), ops._p(d["bias"]), ops._p(d["res"]), ops._p(out), M, N, K, K, N, N, 0,
                               ops._stream_ptr(out))
    if not lib.dsc_has_library_gemm():
        assert rc == DSC_ERR_UNSUPPORTED
        return
    assert rc == DSC_OK and torch.equal(out, want)


# ============================================================================= convolutions (conv3x3.hip, conv_in.hip)
def _conv_operands(d):
    return d["x"].contiguous(memory_format=CL), d["w"].contiguous(memory_format=CL), d.get("res")


@pytest.mark.parametrize("case", E.cases("conv"), ids=_ids(E.cases("conv")))
def test_conv3x3_nhwc_f16(ops, lib, conv_variants, case):
    """dsc_conv3x3_nhwc_f16: one pixel to 24 x 48, both tile widths with ragged sides, ragged last channel tiles, every resample mode
    (odd targets and odd sides), channel-major output, one to twenty channel slices in one to three splits (an uneven one: 2 + 1),
    every epilogue; two shapes under every ring form and the throughput profile"""
    B, Cin, Cout, h, w = case.shape
    mode, splits, nchw = case.get("mode"), case.get("splits"), bool(case.get("nchw"))
    d, want = _device(E.reference(case))
    x, wt, res = _conv_operands(d)
    (H, W), _ = R.conv_geometry(mode, h, w)
    nbytes = lib.dsc_conv3x3_workspace_bytes(B, H, W, Cin, Cout, splits)
    assert splits == 0 or nbytes == (splits > 1) * min(splits, Cin // 64) * B * H * W * Cout * 4       # (0: the cost model's choice)
    for variant in conv_variants(case.sweep):
        out = ops.conv3x3(x, wt, d.get("bias"), residual=res, splits=splits, out_nchw=nchw, **_CONV_KW[mode]((H, W)))
        assert torch.equal(out, want), variant


@pytest.mark.parametrize("case", E.cases("up2x"), ids=_ids(E.cases("up2x")))
def test_conv3x3_up2x_f16(ops, lib, case):
    """dsc_conv3x3_up2x_pack_f16: the packed phase weights equal the fp64 tap sums (sums of up to four values of {-2 .. 2}: exact);
    dsc_conv3x3_up2x_nhwc_f16 equals nearest-2x + 3x3 in fp64, unsplit and in two splits"""
    B, Cin, Cout, h, w = case.shape
    splits = case.get("splits")
    ref = E.reference(case)
    d, want = _device(ref)
    x, wt, _ = _conv_operands(d)
    assert ops.conv3x3_up2x_supported(x, wt)
    packed = ops.conv3x3_up2x_pack(wt)
    assert torch.equal(packed, E.round16(E.up2x_pack64(ref.ops["w"])).cuda()) and torch.equal(packed.double().cpu(), E.up2x_pack64(ref.ops["w"]))
    assert splits == 0 or (lib.dsc_conv3x3_up2x_workspace_bytes(B, h, w, Cin, Cout, splits) > 0) == (splits > 1)
    assert torch.equal(ops.conv3x3_up2x(x, packed, d["bias"], splits=splits), want)


@pytest.mark.parametrize("case", E.cases("conv_gn"), ids=_ids(E.cases("conv_gn")))
def test_conv3x3_gn_nhwc_f16(ops, lib, case):
    """dsc_conv3x3_gn_nhwc_f16: the output and, on integers, gn_part per 8 x 16 pixel tile and group in both `which` slots - ragged
    tiles, an odd upsampled target, groups that cross a channel tile, the per-image add.  8-wide tiles emit none: refused."""
    B, Cin, Cout, h, w = case.shape
    mode, groups = case.get("mode"), case.get("groups")
    ref = E.reference(case)
    d, want = _device(ref)
    x, wt, res = _conv_operands(d)
    (H, W), _ = R.conv_geometry(mode, h, w)
    size = {"upsample_size": (H, W)} if mode == R.UPSAMPLE_CEIL else {}
    rows = lib.dsc_conv3x3_gn_rows(B, H, W, Cin, Cout, groups, mode)
    assert (rows == 0) == (E.conv_tile_width(W) == 8) and ops.conv3x3_gn_rows(x, wt, groups, **size) == rows
    if rows == 0:
        out, part = _empty(B, H, W, Cout), _empty(B, 1, groups, 2, 2, dtype=torch.float32)
        rc = lib.dsc_conv3x3_gn_nhwc_f16(ops._p(x), ops._p(wt), ops._p(d["bias"]), None, 0, None, ops._p(out), B, H, W, Cin, Cout, Cin, 0,
                                         Cout, mode, ops._p(part), groups, 0, ops._stream_ptr(out))
        assert rc == DSC_ERR_UNSUPPORTED
        return
    tile, ntiles = E.pixel_tiles(H, W)
    assert rows == ntiles
    out = ops.conv3x3_gn(x, wt, groups, bias=d["bias"], add=d.get("add"), residual=res, **size)
    assert torch.equal(out, want)
    if case.regime == "integer":
        part = ops.gn_partials_of(out)
        assert part is not None and tuple(part.buf.shape) == (B, rows, groups, 2, 2)
        assert _equal_where_written(part.buf, E.group_partials(E.stored_rows(case, ref), tile, ntiles, groups).cuda())


@pytest.mark.parametrize("case", E.cases("fewcin"), ids=_ids(E.cases("fewcin")))
def test_conv3x3_fewcin_f16(ops, lib, case):
    """dsc_conv3x3_fewcin_f16: 4 and 9 input channels, rows of 7 and 17 pixels (a last block of 8 that hangs over), 8 and 40
    channel groups per pixel"""
    B, Cin, Cout, h, w = case.shape
    d, want = _device(E.reference(case))
    wt = d["w"].reshape(Cout, Cin * 9).t().contiguous()
    assert torch.equal(ops.conv3x3_fewcin(d["x"], wt, d["bias"], Cout), want)
