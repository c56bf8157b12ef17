"""The kernels on activation-like inputs (`-m gpu`): channels tens to hundreds of standard deviations from zero through every
GroupNorm form and LayerNorm, attention logits in the tens through every softmax kernel, a running maximum placed tile by tile
through the two online softmaxes, and every finite fp16 value through GEGLU.  References are fp64 (tests/numeric_ref.py); every
tolerance is a bound the neighbouring test already uses, a stated count of roundings, or twice the floor that the kernel's
documented roundings cost on the same inputs (computed here, capped in tests/test_numeric_stress_host.py).  Each test prints its
figures before it asserts."""
import math

import pytest
import torch

import numeric_ref as nr
from inputs import attn_inputs

pytestmark = pytest.mark.gpu
CL = torch.channels_last
ATOL32 = 6e-3                  # tests/test_region_xattn_gpu.py: attention output against an unrounded oracle, mean <= 4e-4
EMU_MAX, EMU_MEAN = 2e-3, 2e-4   # tests/test_unet_pipeline_gpu.py::test_self_attention: max (times max(1, |ref|max)) and mean


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


def _lib():
    from diffusionspatialcontrol_amd import _lib as lib_mod
    return lib_mod.load_library()


# ============================================================================= 1. GroupNorm away from zero mean
def _gn_check(y, ref, what, check=True):
    mx, mean, bound = nr.gn_errors(y, ref)
    print(f"{what}: max err {mx:.3e} (bound {bound:.3e}), mean err {mean:.3e} (bound {nr.GN_MEAN:.1e})")
    if check:
        assert mx < bound and mean < nr.GN_MEAN, (what, mx, bound, mean)
    return mx, mean


# (2, 64, 24, 24): hw % 8 == 0, the vectorised fp64-accumulating kernels; (1, 40, 5, 7): hw = 35, the scalar kernels
@pytest.mark.parametrize("offset,sigma", nr.OFFSET_SIGMA)
@pytest.mark.parametrize("B,C,h,w,G", [(2, 64, 24, 24, 8), (1, 40, 5, 7, 8)])
def test_groupnorm_nchw_away_from_zero_mean(ops, B, C, h, w, G, offset, sigma):
    """dsc_groupnorm_silu against fp64.  The vectorised statistics kernel sums 128 values per thread in fp32 before fp64 takes
    over; about zero that cost a mean error of 5.0e-4 at (60, 0.25) and 5.3e-4 at (200, 0.7) without SiLU (over the 4e-4 bound),
    about the thread's first value it is 1.2e-4 .. 1.3e-4 at every (offset, sigma).  The scalar kernels are fp64 throughout."""
    x, _, gamma, beta = nr.offset_groupnorm_inputs(B, C, h, w, G, offset, sigma, seed=C + h)
    for act in (True, False):
        ref = nr.groupnorm64(x, G, gamma, beta, 1e-5, act)
        y = ops.groupnorm_silu(x.cuda(), G, gamma.cuda(), beta.cuda(), 1e-5, act)
        _gn_check(y, ref, f"NCHW {B}x{C}x{h}x{w} offset {offset} sigma {sigma} act {act}")


# The launch form each shape selects (run_groupnorm in csrc/groupnorm_nhwc.hip), mode = dsc_debug_set_gn_mode:
#   small     cpg = 8, hw * cpg / 8 = 36 <= 2048 vectors: gn_nhwc_small, one launch, two-pass variance
#   bundle10  cpg = 10, 4 groups per bundle of 5 vectors, hw * 5 = 1280 <= 1536: gn_nhwc_bundle, groups straddle the vectors
#   bundle20  cpg = 20, 2 groups per bundle of 5 vectors: gn_nhwc_bundle
#   slabs     cpg = 10, hw * 5 > 1536: gn_nhwc_stats + gn_nhwc_apply; 32 row chunks of 128 rows per image, 4 channel slabs of 10
#             vectors, 25 row slices: ~5 rows per thread in fp32, the rest in fp64
#   noslabs   mode 10: the same with one slab of 40 vectors, 6 row slices: ~21 rows per thread
#   finalize  mode 4: 256 fine row chunks of 16 rows, the separate finalize launch
NHWC_FORMS = [("small", 2, 64, 6, 6, 8, None), ("bundle10", 2, 320, 16, 16, 32, None), ("bundle20", 2, 640, 16, 16, 32, None),
              ("slabs", 2, 320, 64, 64, 32, None), ("noslabs", 2, 320, 64, 64, 32, 10), ("finalize", 2, 320, 64, 64, 32, 4)]


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("offset,sigma", nr.OFFSET_SIGMA)
@pytest.mark.parametrize("form,B,C,h,w,G,mode", NHWC_FORMS)
def test_groupnorm_nhwc_away_from_zero_mean(ops, form, B, C, h, w, G, mode, offset, sigma, with_add):
    """every launch form of dsc_groupnorm_silu_nhwc against fp64 with the suite's GroupNorm bound at every (offset, sigma).
    With fp32 sums about zero in the statistics pass, the form with the most rows per thread (noslabs, ~21) missed the bound at
    (60, 0.25), (200, 0.7) and (1000, 5) - mean error up to 1.06e-3, max up to 5.1e-2 - while the default slab form (~5 rows per
    thread) stayed inside it with up to twice its present error; with the sums about a pivot all three forms give the same figures,
    mean error 7.3e-5 .. 8.1e-5 at every (offset, sigma)."""
    x, add, gamma, beta = nr.offset_groupnorm_inputs(B, C, h, w, G, offset, sigma, seed=C + h + int(offset), with_add=with_add)
    ref = nr.groupnorm64(x, G, gamma, beta, 1e-5, True, add=add)
    xc = x.cuda().contiguous(memory_format=CL)
    addc = add.cuda() if with_add else None
    lib = _lib()
    try:
        if mode is not None:
            lib.dsc_debug_set_gn_mode(mode)
        y = ops.groupnorm_silu_nhwc(xc, G, gamma.cuda(), beta.cuda(), 1e-5, True, add=addc)
        again = ops.groupnorm_silu_nhwc(xc, G, gamma.cuda(), beta.cuda(), 1e-5, True, add=addc)
    finally:
        lib.dsc_debug_set_gn_mode(11)
        lib.dsc_debug_set_gn_mode(0)
    _gn_check(y, ref, f"NHWC {form} offset {offset} sigma {sigma} add {with_add}")
    assert torch.equal(y, again)
    if form == "slabs":                                       # token-major view: the same bytes
        tok = xc.permute(0, 2, 3, 1).reshape(B, h * w, C)
        y2 = ops.groupnorm_silu_nhwc(tok, G, gamma.cuda(), beta.cuda(), 1e-5, True, add=addc)
        assert torch.equal(y2.reshape(B, h, w, C).permute(0, 3, 1, 2), y)


# (2, 192 + 128, 64, 64): the two-launch form (the statistics pass reads both sources and writes the concatenation; the group of
# channels 190 .. 199 straddles the two sources); (2, 64 + 64, 4, 4): gn_nhwc_small reading through gn_load
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("offset,sigma", nr.OFFSET_SIGMA)
@pytest.mark.parametrize("B,C1,C2,h,w,G", [(2, 192, 128, 64, 64, 32), (2, 64, 64, 4, 4, 8)])
def test_groupnorm_of_concatenation_away_from_zero_mean(ops, B, C1, C2, h, w, G, offset, sigma, with_add):
    C = C1 + C2
    x, add, gamma, beta = nr.offset_groupnorm_inputs(B, C, h, w, G, offset, sigma, seed=C1 + h + int(offset), with_add=with_add)
    ref = nr.groupnorm64(x, G, gamma, beta, 1e-5, True, add=add)
    xc = x.cuda()
    x1, x2 = xc[:, :C1].contiguous(memory_format=CL), xc[:, C1:].contiguous(memory_format=CL)
    addc = add.cuda() if with_add else None
    y, cat = ops.groupnorm_silu_nhwc_cat(x1, x2, G, gamma.cuda(), beta.cuda(), 1e-5, True, add=addc)
    _gn_check(y, ref, f"NHWC cat {C1}+{C2} {h}x{w} offset {offset} sigma {sigma} add {with_add}")
    want_cat = xc.contiguous(memory_format=CL)
    assert torch.equal(cat, want_cat)
    assert torch.equal(y, ops.groupnorm_silu_nhwc(want_cat, G, gamma.cuda(), beta.cuda(), 1e-5, True, add=addc))   # same arithmetic


def _producer_outputs(ops, producer, offset, sigma):
    """(the tensor a statistics-emitting producer stored, channels_last [B, C, h, w], its partial sums, groups): the offsets come in
    through the bias, the spread through the input (unit-variance weights: the output's sigma is the input's)"""
    g = torch.Generator().manual_seed(int(offset) + len(producer))
    groups = 32
    if producer == "linear_gn":                                  # dsc_linear_gn_f16, 1x1 convolution as a token-major GEMM; cpg = 20
        B, L, K, N = 2, 1024, 640, 640
        x = (torch.randn(B, L, K, generator=g) * sigma).half().cuda()
        wt = (torch.randn(N, K, generator=g) / math.sqrt(K)).half().cuda()
        bias = (nr.channel_offsets(N, groups, offset) + torch.randn(N, generator=g) * 0.2 * sigma).half().cuda()
        got = ops.linear_gn(x, wt, bias, None, L, groups)
        assert got is not None
        y, part = got
        return y.reshape(B, 32, 32, N).permute(0, 3, 1, 2), part, groups
    B, cin, cout = 2, 320, 640                                   # dsc_conv3x3_gn_nhwc_f16; cpg = 20 straddles the 64-channel tiles
    src, kw = ((32, 32), {}) if producer == "conv3x3_gn" else ((16, 16), {"upsample_size": (31, 32)})   # resample code 4: odd height
    x = (torch.randn(B, cin, *src, generator=g) * sigma).half().cuda().contiguous(memory_format=CL)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)).half().cuda().contiguous(memory_format=CL)
    bias = (nr.channel_offsets(cout, groups, offset) + torch.randn(cout, generator=g) * 0.2 * sigma).half().cuda()
    assert ops.conv3x3_gn_rows(x, wt, groups, **kw) > 0
    out = ops.conv3x3_gn(x, wt, groups, bias=bias, **kw)
    part = ops.gn_partials_of(out)
    assert part is not None
    return out, part, groups


def _producer_case(ops, producer, offset, sigma, check):
    out, part, groups = _producer_outputs(ops, producer, offset, sigma)
    C = out.shape[1]
    g = torch.Generator().manual_seed(9)
    gamma, beta = (torch.randn(C, generator=g) * 0.5 + 1).half(), (torch.randn(C, generator=g) * 0.3).half()
    grp = out.double().cpu().reshape(out.shape[0], groups, -1)
    ratio = (grp.mean(-1).abs() / grp.std(-1)).max().item()
    ref = nr.groupnorm64(out.cpu(), groups, gamma, beta, 1e-5, False)
    one = ops.groupnorm_apply_nhwc(out, part, groups, gamma.cuda(), beta.cuda(), 1e-5, False)
    two = ops.groupnorm_silu_nhwc(out, groups, gamma.cuda(), beta.cuda(), 1e-5, False)
    print(f"{producer} offset {offset} sigma {sigma}: largest group mean / sigma {ratio:.0f}")
    _gn_check(two, ref, f"  {producer} two-launch GroupNorm of the same tensor")       # makes its own statistics pass: always held
    return _gn_check(one, ref, f"  {producer} one-launch GroupNorm from the producer's partials", check=check)


@pytest.mark.parametrize("offset,sigma", nr.MODERATE)
@pytest.mark.parametrize("producer", ["conv3x3_gn", "linear_gn", "sized_upsample"])
def test_groupnorm_from_producer_statistics_away_from_zero_mean(ops, producer, offset, sigma):
    """dsc_groupnorm_apply_nhwc fed by each producer's fp32 (sum, sum of squares) partials, against fp64 with the suite's GroupNorm
    bound, up to mean / sigma ~ 100 (60 / 0.7 is the regime
    test_groupnorm_epilogue_statistics_with_a_large_channel_offset names)"""
    _producer_case(ops, producer, offset, sigma, check=True)


@pytest.mark.parametrize("offset,sigma", nr.OFFSET_SIGMA[2:])
@pytest.mark.parametrize("producer", ["conv3x3_gn", "linear_gn", "sized_upsample"])
def test_groupnorm_from_producer_statistics_known_limit(ops, producer, offset, sigma):
    """Above mean / sigma ~ 100 the producers' partials are fp32 sums of squares about zero, and their cancellation is the known
    limit of the one-launch form: measured and printed here, NOT asserted (the epilogues are not part of the change that added this
    test; the two-launch GroupNorm of the same tensor is asserted in the helper).  Measured on the MI355X, one-launch max / mean
    error against fp64 (the bound would be 4e-3 * max(1, |ref|max) / 4e-4):

    producer        (offset, sigma)  group mean/sigma   max err    mean err   (two-launch form, same tensor: max / mean)
    conv3x3_gn      (60, 0.25)       244                1.11e-02   2.58e-04   3.77e-03 / 1.48e-04
    conv3x3_gn      (200, 0.7)       290                1.58e-02   4.28e-04   3.73e-03 / 1.48e-04
    conv3x3_gn      (1000, 5)        203                8.91e-03   2.25e-04   3.75e-03 / 1.48e-04
    linear_gn       (60, 0.25)       238                1.03e-02   3.11e-04   3.60e-03 / 1.48e-04
    linear_gn       (200, 0.7)       284                9.80e-03   3.11e-04   3.68e-03 / 1.48e-04
    linear_gn       (1000, 5)        201                7.74e-03   2.52e-04   1.96e-03 / 1.48e-04
    sized_upsample  (60, 0.25)       247                9.66e-03   2.98e-04   3.87e-03 / 1.48e-04
    sized_upsample  (200, 0.7)       294                1.85e-02   3.94e-04   3.01e-03 / 1.47e-04
    sized_upsample  (1000, 5)        205                8.09e-03   2.36e-04   3.81e-03 / 1.48e-04

    |ref|max is 8 - 12 on these inputs, so the max bound (3.4e-2 .. 4.7e-2) holds everywhere; the mean error is two to three times
    that of the two-launch form and crosses 4e-4 at conv3x3_gn (200, 0.7)."""
    _producer_case(ops, producer, offset, sigma, check=False)


@pytest.mark.parametrize("offset,sigma", nr.OFFSET_SIGMA)
@pytest.mark.parametrize("rows,C", [(6, 320), (9, 64), (5, 2560)])
def test_add_layernorm_away_from_zero_mean(ops, rows, C, offset, sigma):
    """dsc_add_layernorm (two-pass variance on the register copy) with whole rows at +-offset, test_add_layernorm's tolerance"""
    g = torch.Generator().manual_seed(rows + C + int(offset))
    x = torch.randn(rows, C, generator=g) * sigma
    x[::2] += offset
    x[1] -= offset
    x = x.half()
    a = (torch.randn(rows, C, generator=g) * 0.5 * sigma).half()
    gamma, beta = (torch.randn(C, generator=g) * 0.3 + 1).half(), (torch.randn(C, generator=g) * 0.2).half()
    s_ref = (x.float() + a.float()).half()
    for a_dev, src in ((a.cuda(), s_ref), (None, x)):
        s, y = ops.add_layernorm(x.cuda(), a_dev, gamma.cuda(), beta.cuda())
        ref = nr.layernorm64(src, gamma, beta)
        err = (y.double().cpu() - ref).abs()
        print(f"add_layernorm {rows}x{C} offset {offset} sigma {sigma} add {a_dev is not None}: max err {err.max().item():.3e}")
        assert torch.equal(s.cpu(), src)
        assert torch.all(err <= 1.5e-3 * ref.abs() + 2e-3), err.max().item()


# ============================================================================= 2. attention at large logits
def _attention_check(out, ref, emu, floor, what):
    """against the emulation: test_self_attention's tolerances (the pre-scale rounding is on both sides, so large logits do not
    loosen it; a wrong rescale or mask shows here).  Against fp64: twice the emulation's own floor on these inputs - the factor 2
    covers the MFMA summation order and the fp16 rounding of the output, which the emulation does not model."""
    o = out.double().cpu()
    e_emu, e_ref = (o - emu).abs(), (o - ref).abs()
    top = max(1.0, ref.abs().max().item())
    print(f"{what}: vs emulation max {e_emu.max().item():.3e} (bound {EMU_MAX * top:.3e}) mean {e_emu.mean().item():.3e}; "
          f"vs fp64 max {e_ref.max().item():.3e} (floor {floor:.3e}, bound {2 * floor:.3e})")
    assert e_emu.max().item() < EMU_MAX * top and e_emu.mean().item() < EMU_MEAN, (what, e_emu.max().item(), e_emu.mean().item())
    assert e_ref.max().item() <= 2.0 * floor, (what, e_ref.max().item(), floor)


# measured on the MI355X, max |out - fp64| at gain 2 / gain 3 (the emulation's floor in brackets); against the emulation the
# maximum stayed between 1.0e-3 and 1.8e-3 everywhere:
#   (1, 2, 128, 128, 40)   2.23e-3 (1.71e-3) / 5.38e-3 (5.29e-3)
#   (1, 2, 96, 200, 64)    2.28e-3 (2.04e-3) / 5.08e-3 (4.91e-3)
#   (1, 2, 64, 130, 80)    1.70e-3 (1.48e-3) / 4.32e-3 (3.96e-3)
#   (1, 1, 64, 257, 160)   2.06e-3 (1.59e-3) / 3.78e-3 (3.65e-3)
#   rotated stagger        2.61e-3 (2.44e-3) / 5.58e-3 (5.60e-3)
#   every forced tiling    - / 5.55e-3 (5.43e-3), the same bits from all eighteen
@pytest.mark.parametrize("gain", nr.ATTN_GAINS)
@pytest.mark.parametrize("B,H,L,S,d,seed", nr.ATTN_CASES)
def test_self_attention_large_logits(ops, B, H, L, S, d, seed, gain):
    q, k, v, ref, emu, floor = nr.attention_case(B, H, L, S, d, gain, seed)
    out = ops.self_attention(q.cuda(), k.cuda(), v.cuda())
    _attention_check(out, ref, emu, floor, f"self_attention B={B} H={H} L={L} S={S} d={d} gain={gain} max|s|={nr.max_logit(q, k):.0f}")


@pytest.mark.parametrize("gain", nr.ATTN_GAINS)
def test_self_attention_large_logits_rotated_stagger(ops, gain):
    """the compact d = 40 image with the rotated stagger (chosen from 256 workgroups of 256 query rows on) at the smallest L at
    which all eight computing waves own rows; four distinct heads laid out over 256 (batch, head) pairs"""
    q, k, v, ref, emu, floor = nr.rotated_case(gain)
    out = ops.self_attention(q.cuda(), k.cuda(), v.cuda())
    _attention_check(out, ref, emu, floor, f"self_attention rotated stagger gain={gain}")


@pytest.mark.parametrize("variant", list(range(1, 19)))
def test_self_attention_large_logits_tiling_variants(ops, variant):
    """every tiling dsc_debug_set_self_attn_variant can force, at one shape (d = 40 reaches all of them, the compact-image ones
    included, so none is skipped) and gain 3"""
    B, H, L, S, d, seed = nr.VARIANT_CASE
    q, k, v, ref, emu, floor = nr.attention_case(B, H, L, S, d, 3, seed)
    lib = _lib()
    lib.dsc_debug_set_self_attn_variant(variant)
    try:
        out = ops.self_attention(q.cuda(), k.cuda(), v.cuda())
    finally:
        lib.dsc_debug_set_self_attn_variant(0)
    _attention_check(out, ref, emu, floor, f"self_attention variant {variant} gain 3")


def _region_case(Bc, H, L, S, d, Bw, seed):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(Bc, H, L, d, generator=g) * 3).half()
    k = (torch.randn(Bc, H, S, d, generator=g) * 3).half()
    v = torch.randn(Bc, H, S, d, generator=g).half()
    w = torch.from_numpy(attn_inputs(f"stress/{Bc}/{H}/{L}/{S}/{d}", Bc=Bc, H=H, L=L, S=S, d=d, Bw=Bw)["w"])
    return q, k, v, w


# generic: dsc_region_xattn_fwd; packed: pre-packed K / V + compressed table, S <= 96 (one chunk); chunked: S = 154 > 96, the
# long-prompt kernels' online softmax over chunks of 96 keys.  The region kernels scale the fp32 scores (no fp16 pre-scale of Q):
# the fp32-score path against the unrounded fp64 oracle at its neighbour's tolerance (tests/test_region_xattn_gpu.py: 6e-3 / 4e-4)
@pytest.mark.parametrize("form,Bc,H,L,S,d,Bw", [("generic", 2, 2, 100, 77, 40, 2), ("packed", 2, 2, 100, 77, 40, 2),
                                                ("chunked", 2, 2, 70, 154, 40, 2), ("chunked", 1, 2, 40, 231, 80, 1)])
def test_region_xattn_large_logits(ops, form, Bc, H, L, S, d, Bw):
    q, k, v, w = _region_case(Bc, H, L, S, d, Bw, seed=L + S)
    sigma = 2.0
    ref = nr.region_attention64(q, k, v, w, sigma)
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    if form == "generic":
        out = ops.region_xattn(qd, kd, vd, w.cuda(), sigma, ref_fp16_rounding=False)
    else:
        packed = ops.xattn_kv_pack(kd, vd, layout="bhld")
        comp = ops.compress_region_table(w.cuda())
        assert comp is not None
        out = ops.region_xattn_packed(qd.transpose(1, 2), packed, S, comp, sigma, ref_fp16_rounding=False).transpose(1, 2)
    err = (out.double().cpu() - ref).abs()
    print(f"region_xattn {form} L={L} S={S} d={d}: max |s| {nr.max_logit(q.transpose(1, 2), k.transpose(1, 2)):.0f}, "
          f"max err {err.max().item():.3e} mean {err.mean().item():.3e}")
    assert err.max().item() < ATOL32 and err.mean().item() < 4e-4, (err.max().item(), err.mean().item())


IP_ROW_SCALE = [0.0, 0.7, 1.0, -0.5]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("L,H,d,T", [(100, 4, 40, 4), (100, 4, 40, 16), (64, 2, 160, 16)])
def test_ip_xattn_add_large_logits(ops, L, H, d, T, masked):
    """dsc_ip_xattn_add_f16 / _masked_f16 at gain 3, tests/test_ip_serving_gpu.py's bound per row: |row_scale| (* max weight) * 6e-3
    + half an fp16 ulp of the largest |result|"""
    B = len(IP_ROW_SCALE)
    g = torch.Generator().manual_seed(L + d + T)
    q = (torch.randn(B, L, H, d, generator=g) * 3).half()
    k = (torch.randn(B, T, H, d, generator=g) * 3).half()
    v = torch.randn(B, T, H, d, generator=g).half()
    io = torch.randn(B, L, H * d, generator=g).half()
    wq = None
    if masked:
        wq = torch.rand(B, L, generator=g)
        wq[:, 16:32] = 0.0                                        # one whole 16-query tile of zeros
        wq[:, 40] = 1.0
        wq = wq.half()
    ref = nr.ip_restated64(q, k, v, io, IP_ROW_SCALE, wq)
    got = ops.ip_xattn_add(q.cuda(), k.cuda(), v.cuda(), torch.tensor(IP_ROW_SCALE, device="cuda"), io.cuda().clone(),
                           q_weight=wq.cuda() if masked else None).double().cpu()
    for b, rs in enumerate(IP_ROW_SCALE):
        top = ref[b].abs().max().item()
        half_ulp = 2.0 ** (math.floor(math.log2(top)) - 10) / 2
        wmax = wq[b].float().abs().max().item() if masked else 1.0
        err = (got[b] - ref[b]).abs().max().item()
        print(f"ip_xattn_add L={L} d={d} T={T} masked={masked} row {b}: max err {err:.3e} (bound {abs(rs) * wmax * ATOL32 + half_ulp:.3e})")
        assert err <= abs(rs) * wmax * ATOL32 + half_ulp, (b, err)
    assert torch.equal(got[0], io[0].double())


# n = 64: softmax_rows_kernel<1>; 1000: <1> with a ragged last vector group; 8200: 1025 vectors -> <8>
@pytest.mark.parametrize("n", [64, 1000, 8200])
def test_softmax_rows_large_logits(ops, n):
    """scores randn * 200 at scale 0.37 (logits of sigma 74), a one-hot row (60 000 against -60 000) and an all-equal row; the
    bound of test_softmax_rows against fp64, row sums within 2e-3 of 1"""
    g = torch.Generator().manual_seed(n)
    s = (torch.randn(6, n, generator=g) * 200).half()
    s[0] = -60000.0
    s[0, n // 3] = 60000.0
    s[1] = 123.0
    ref = nr.softmax64(s, 0.37)
    out = ops.softmax_rows(s.cuda(), scale=0.37).double().cpu()
    err = (out - ref).abs().max().item()
    print(f"softmax_rows n={n}: max err {err:.3e}, max |row sum - 1| {(out.sum(-1) - 1).abs().max().item():.3e}")
    assert torch.isfinite(out).all()
    assert err < 1e-3 * ref.max().item() + 1e-6
    assert (out.sum(-1) - 1).abs().max().item() < 2e-3
    assert out[0, n // 3].item() == 1.0 and out[0].sum().item() == 1.0


# ============================================================================= 3. where the running maximum moves
def _staircase_check(out, q, k, v, what):
    ref = nr.attention64(q, k, v, nr.STAIRCASE_SCALE)
    err = (out.double().cpu() - ref).abs()
    P = 4
    per = [err[0, p_::P].max().item() for p_ in range(min(P, err.shape[1]))]
    print(f"{what}: max err {err.max().item():.3e} mean {err.mean().item():.3e}; per pattern " + " ".join(f"{e:.2e}" for e in per))
    assert torch.isfinite(out).all()
    assert err.max().item() < EMU_MAX * max(1.0, ref.abs().max().item()) and err.mean().item() < EMU_MEAN, (what, per)


# variant 0: the automatic choice (one workgroup of L = 256 rows: two 4-wave or one 8-wave); 2 / 7: eight waves, without and with
# loader waves; 14 / 18: the staggered and rotated-stagger kernels, whose waves run P.V one tile late (d = 40; d = 64 gets the
# generic staggered kernel or falls through to 8 waves + 2 loaders)
@pytest.mark.parametrize("variant", [0, 1, 2, 7, 14, 18])
@pytest.mark.parametrize("S", [129, 191, 256])
@pytest.mark.parametrize("d", [40, 64])
def test_self_attention_running_maximum_patterns(ops, d, S, variant):
    """Prescribed logits (numeric_ref.staircase_qkv), V one-hot per key: the output is the probability row.  Query row i follows
    pattern i % 4, so the 32 rows of one wave disagree about rescaling: a maximum that climbs 9 log2 units per 64-key tile (every
    tile rescales, tau = 8), one that climbs 7.5 above tile 0 and stays (no rescale of its own, P ~ 181 in fp16 summed over all
    later keys), one that sits in tile 0 with every later key 30 below, and one that only appears in the ragged last tile.  Then
    the two quiet patterns alone: after tile 0 no row of any wave asks for a rescale.  fp64 reference, the emulation tolerance."""
    L = 256
    lib = _lib()
    steps = nr.staircase_patterns(S)
    for name, st in (("all four", steps), ("quiet only", [steps[1], steps[2]] * 2)):
        q, k, v, _ = nr.staircase_qkv(L, S, d, st)
        lib.dsc_debug_set_self_attn_variant(variant)
        try:
            out = ops.self_attention(q.cuda(), k.cuda(), v.cuda(), scale=nr.STAIRCASE_SCALE)
        finally:
            lib.dsc_debug_set_self_attn_variant(0)
        _staircase_check(out, q, k, v, f"self_attention d={d} S={S} variant {variant} {name}")


@pytest.mark.parametrize("S", [300, 384])
@pytest.mark.parametrize("d", [40, 64])
def test_region_xattn_chunked_running_maximum_patterns(ops, d, S):
    """the same four patterns over the 96-key chunks of the long-prompt kernels' online softmax (dsc_region_xattn_fwd_packed,
    S > 96, no region table): S = 384 is four whole chunks, S = 300 ends in a ragged chunk of 12 keys"""
    L = 64
    steps = nr.staircase_patterns(S, tile=96)
    for name, st in (("all four", steps), ("quiet only", [steps[1], steps[2]] * 2)):
        q, k, v, _ = nr.staircase_qkv(L, S, d, st, tile=96)
        packed = ops.xattn_kv_pack(k.cuda(), v.cuda(), layout="blhd")
        out = ops.region_xattn_packed(q.cuda(), packed, S, None, scale=nr.STAIRCASE_SCALE, ref_fp16_rounding=False)
        _staircase_check(out, q, k, v, f"region_xattn_packed chunked d={d} S={S} {name}")


# ============================================================================= 4. GEGLU over every fp16 value
def _geglu_bound(hid, gate):
    """|y - hid * gelu64(gate)| for y = fp16(hid * fp16(gelu(gate))): one fp16 rounding of gelu plus twice the approximation bound
    csrc/dsc_common.h states for gelu_erf (1.5e-7 on erfc, times |gate|), carried through the product by |hid|, plus - for
    hid != 1, where the product is not exact - one more rounding at the result"""
    gel = nr.gelu64(gate)
    ref = hid.double() * gel
    g_abs = gate.double().abs().numpy()
    bound = hid.double().abs().numpy() * (nr.ulp16(gel.numpy()) + 3e-7 * g_abs)
    if not torch.all(hid == 1):
        bound = bound + nr.ulp16(ref.numpy())
    return ref, torch.from_numpy(bound)


def _geglu_check(y, hid, gate, what):
    ref, bound = _geglu_bound(hid, gate)
    keep = ref.abs() <= 65000.0                                   # (fp16-overflowing products are not this test's subject)
    err = (y.double().cpu() - ref).abs()
    assert torch.isfinite(y.cpu()[keep]).all(), what
    worst = (err / bound)[keep]
    i = int(torch.argmax(torch.where(keep, err / bound, torch.zeros_like(err))))
    print(f"{what}: {int(keep.sum())} values, worst err / bound {worst.max().item():.3f} at gate {gate[i].item()!r} "
          f"(err {err[i].item():.3e}, bound {bound[i].item():.3e})")
    assert torch.all(err[keep] <= bound[keep]), (what, gate[i].item(), err[i].item(), bound[i].item())


def test_geglu_over_every_finite_fp16_gate(ops):
    """dsc_geglu with gate = all 63 488 finite fp16 values in one row of 63 488 (a multiple of the 8-wide vectors); hid = 1: the
    output is fp16(gelu(gate)); then hid in {-3, 0.1, 7, 1000}"""
    gate = nr.all_finite_fp16()
    for h in (1.0, -3.0, 0.1, 7.0, 1000.0):
        hid = torch.full_like(gate, h)                           # (0.1 as its fp16 value)
        y = ops.geglu(torch.cat([hid, gate]).view(1, -1).cuda()).view(-1)
        _geglu_check(y, hid, gate, f"geglu hid={h}")


def test_linear_geglu_over_every_finite_fp16_gate(ops):
    """the same sweep through the GEMM's fused GEGLU epilogue (dsc_linear_f16, geglu = 1), which its shape rules allow at C = 64:
    x [992, 64] holds the 63 488 values, the weight's gate half is the identity and its hidden half zero with bias `hid`, so the
    fp32 accumulator of gate column j of row m is x[m, j] exactly"""
    gate = nr.all_finite_fp16()
    K = 64
    x = gate.view(-1, K)
    w = torch.zeros(2 * K, K, dtype=torch.float16)
    w[K:] = torch.eye(K, dtype=torch.float16)
    for h in (1.0, 7.0):
        b = torch.zeros(2 * K, dtype=torch.float16)
        b[:K] = h
        y = ops.linear(x.cuda(), w.cuda(), b.cuda(), geglu=True, prefer_kernel=True)
        assert y.shape == (x.shape[0], K)
        _geglu_check(y.reshape(-1), torch.full_like(gate, h), gate, f"linear geglu hid={h}")
