"""tests/exact_inputs.py on the CPU: the conditions under which tests/test_exact_sums_gpu.py may compare with `torch.equal` hold for
every case of its table, the generator and the fp64 references are what they say, and the exact comparison sees what the tolerance
tests pass over.

The last part is the reason for both files.  The matrix kernels are otherwise tested on randn operands against
|err| <= 1.5e-3 |ref| + 2e-3, a bound that is wide next to ONE term of a long sum.  Each mutant below is applied to a plain CPU
emulation of the tiled sum (K steps of 64, channel slices x taps, splits; no kernel is edited).  On the exact operands the comparison
fails for every one; on randn operands (test_linear_kernel's and test_conv3x3_kernel's distributions) this share of the outputs the
mutant changes still passes the old bound (MUTANT_SHARES, recomputed and printed by test_the_detector_detects):

    last K element dropped in the last row                  GEMM  200 x 64, K = 704        8 %
    the K step that reuses ring stage 0 added twice         GEMM  200 x 64, K = 704        1 %
    first channel slice of the last split skipped           conv  192 -> 64, 12 x 12       0 %
    one halo column of an overhanging sub-block read as 0   conv  64 -> 64, 9 x 30         1 %
    two taps swapped at the image border only               conv  64 -> 64, 9 x 30         1 %
    accumulator rounded to fp16 before the residual add     GEMM  200 x 64, K = 704      100 %
"""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E
import guard_band_refs as R

ENTRIES = sorted({c.entry for c in E.CASES})


@pytest.mark.parametrize("entry", ENTRIES)
def test_conditions_hold_for_every_case(entry):
    """check_exact: sum |terms| < 2^24 per output element, the reference on the regime's grid, integer outputs <= 2048 and unrounded,
    dyadic outputs rounded somewhere, every emitted statistic's sum of squares < 2^24"""
    for regime in E.REGIMES:
        for case in E.cases(entry, (regime,)):
            figures = E.check_exact(case)
            assert figures["sum|terms|"] < E.LIMIT and figures["sumsq"] < E.LIMIT


def test_the_table_covers_what_it_names():
    by = {e: E.cases(e) for e in ENTRIES}
    assert set(by) == set(E._SHAPES) and all(by.values())
    lin = {c.shape for c in by["linear"] if c.sweep and not c.opt}
    assert lin == {(M, N, K) for M in (1, 63, 65, 129, 200) for N in (64, 192, 256) for K in (64, 256, 704)}
    assert {(c.shape[2], c.get("splits")) for c in by["splitk"]} == {(704, 2), (704, 3), (704, 4), (320, 4)}
    assert {c.get("mode") for c in by["conv"]} == {R.PLAIN, R.UPSAMPLE2X, R.UPSAMPLE_CEIL, R.STRIDE2, R.STRIDE2_PAD_BR}
    assert {c.shape[2] for c in by["conv"]} >= {4, 40, 72, 100} and {c.shape[1] for c in by["fewcin"]} == {4, 9}
    for entry, cs in by.items():                                           # both regimes, the same cases in each
        if entry != "lt":
            assert {dataclass_key(c) for c in cs if c.regime == "integer"} == {dataclass_key(c) for c in cs if c.regime == "dyadic"}


def dataclass_key(c):
    return (c.entry, c.shape, c.bias, c.res, c.opt)


def test_generator_emits_only_its_stated_values():
    for case in E.CASES[::7] + tuple(E.cases("conv_gn")) + tuple(E.cases("fewcin")):
        o = E.operands(case)
        dy = case.regime == "dyadic"
        K = o["x"].shape[1]
        xe = E._x_exponents(K, case.regime)
        xi = o["x"].double() / torch.pow(2.0, xe).reshape(1, K, *([1] * (o["x"].dim() - 2)))
        assert set(xi.unique().tolist()) <= {-1.0, 0.0, 1.0}, case.id
        assert set((o["w"].double() / 2.0 ** (E.W_EXP if dy else 0)).unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}, case.id
        for name in ("bias", "res", "add"):
            if name in o:
                assert set((o[name].double() / 2.0 ** (E.E_EXP if dy else 0)).unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}, case.id
        assert ("bias" in o) == case.bias and ("res" in o) == case.res and ("add" in o) == bool(case.get("add"))
        assert all(torch.equal(v, E.operands(case)[k]) for k, v in o.items())             # seeded: the same again


def test_no_two_taps_of_a_filter_are_equal():
    """a kernel that multiplies tap t's pixels with tap u's weights gets other numbers, for every filter of every convolution case"""
    for case in (c for c in E.CASES if c.entry in E.CONV_ENTRIES):
        w = E.operands(case)["w"]
        taps = w.reshape(w.shape[0], w.shape[1], 9).permute(0, 2, 1)                      # [Cout, 9, Cin]
        same = (taps[:, :, None, :] == taps[:, None, :, :]).all(-1)
        assert int(same.sum()) == 9 * w.shape[0], case.id
        k = torch.arange(w.shape[1])
        edge = (k % 64 == 0) | (k % 64 == 63) | (k == w.shape[1] - 1)
        assert (w[:, edge] != 0).all() and (E.operands(case)["x"][:, edge] != 0).all(), case.id      # live_edges


@pytest.mark.parametrize("mode", [R.PLAIN, R.UPSAMPLE2X, R.UPSAMPLE_CEIL, R.STRIDE2, R.STRIDE2_PAD_BR])
def test_convolution_reference_agrees_with_torch(mode):
    g = torch.Generator().manual_seed(mode)
    h, w = (6, 8) if mode == R.STRIDE2_PAD_BR else (5, 7)
    x, wt = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64), torch.randn(4, 3, 3, 3, generator=g, dtype=torch.float64)
    (H, W), (oh, ow) = R.conv_geometry(mode, h, w)
    b, add, r = torch.randn(4, generator=g).double(), torch.randn(2, 4, generator=g).double(), torch.randn(2, 4, oh, ow, generator=g).double()
    mine = E.conv_epilogue64(E.conv64(x, wt, mode), b, r, add)
    ref = R.conv3x3(x, wt, b, r, mode, (H, W), add=add, dtype=torch.float64)
    assert mine.shape == ref.shape == (2, 4, oh, ow) and torch.allclose(mine, ref, rtol=0, atol=1e-12)


def test_linear_and_layout_references_agree_with_torch():
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(6, 5, generator=g, dtype=torch.float64), torch.randn(9, 5, generator=g, dtype=torch.float64)
    b, r = torch.randn(9, generator=g, dtype=torch.float64), torch.randn(2, 9, generator=g, dtype=torch.float64)
    y = E.linear64(x, w, b, r)
    assert torch.allclose(y, F.linear(x, w, b) + torch.cat([r, r, r]), rtol=0, atol=1e-12)
    q, kv = R.head_major(y, 2, 3, 3)                                  # B = 2, L = 3, C = 3, three heads of one channel
    for bb in range(2):
        for l in range(3):
            for hd in range(3):
                assert q[bb * 3 + l, hd] == y[bb * 3 + l, hd] and kv[0, bb, hd, l, 0] == y[bb * 3 + l, 3 + hd] and kv[1, bb, hd, l, 0] == y[bb * 3 + l, 6 + hd]
    # the phase weights: nearest 2x + 3x3 == four 2x2 convolutions of the source with the summed taps
    xs, wt = torch.randn(1, 2, 3, 4, generator=g, dtype=torch.float64), torch.randn(3, 2, 3, 3, generator=g, dtype=torch.float64)
    packed, want = E.up2x_pack64(wt), F.conv2d(F.interpolate(xs, scale_factor=2.0, mode="nearest"), wt, padding=1)
    pad = F.pad(xs, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            got = sum(torch.einsum("bchw,oc->bohw", pad[:, :, py + a:py + a + 3, px + b:px + b + 4], packed[2 * py + px, :, 2 * a + b, :])
                      for a in range(2) for b in range(2))
            assert torch.allclose(got, want[:, :, py::2, px::2], rtol=0, atol=1e-12)
    assert torch.equal(E.up2x_pack64(wt.half()).half(), R.up2x_pack(wt.half()))


def test_statistics_references():
    """group_partials against a loop over its definition (gn_partials.h): 48 channels per group in 192 - groups 1 and 2 cross a
    64-channel boundary -, 9 x 30 pixels in 8 x 16 tiles; the tiles of a group add up to guard_band_refs.group_sums"""
    g = torch.Generator().manual_seed(2)
    B, H, W, C, groups = 2, 9, 30, 192, 4
    v = torch.randint(-9, 10, (B, H * W, C), generator=g).double()
    tile, ntiles = E.pixel_tiles(H, W)
    assert ntiles == 4 and tile.reshape(H, W)[8, 16] == 3 and tile.reshape(H, W)[7, 15] == 0
    part = E.group_partials(v, tile, ntiles, groups)
    assert torch.equal(~torch.isnan(part[0, 0, :, 1, 0]), R.straddles(C, groups))
    img = v.reshape(B, H, W, C)
    assert part[1, 3, 1, 0, 0] == img[1, 8:, 16:, 48:64].sum() and part[1, 3, 1, 1, 1] == (img[1, 8:, 16:, 64:96] ** 2).sum()
    assert part[0, 1, 3, 0, 0] == img[0, :8, 16:, 144:].sum()
    assert torch.equal(torch.nan_to_num(part).sum(dim=(1, 3)), R.group_sums(v.reshape(B * H * W, C), B, groups))
    rt, n = E.row_tiles(192, 3)
    assert n == 3 and rt[63] == 0 and rt[64] == 1 and rt[191] == 2


# ============================================================================= the detector detects
def tiled_gemm(x, w, bias, res, *, stages=3, mutant=None, round_acc=False):
    """x @ w.T as the kernels add it up - K steps of 64 in order, step kt in ring stage kt % stages - then + bias + residual, fp64"""
    M, K = x.shape
    acc = torch.zeros(M, w.shape[0], dtype=torch.float64)
    for kt in range(K // 64):
        xs, ws = x[:, kt * 64:(kt + 1) * 64].double().clone(), w[:, kt * 64:(kt + 1) * 64].double()
        if mutant == "last k, last row" and kt == K // 64 - 1:
            xs[M - 1, 63] = 0.0
        acc += xs @ ws.t()
        if mutant == "ring stage 0 twice" and kt == stages:               # the first step that lands in a stage used before
            acc += xs @ ws.t()
    if round_acc:
        acc = E.round16(acc).double()
    return acc + bias.double() + res.double()


def tiled_conv(x, w, bias, res, *, splits=1, mutant=None):
    """the 3x3 / pad 1 convolution as channel slices of 64 (outer, dealt to `splits` in order) x 9 taps (inner), the splits' partial
    sums added in split order, + bias + residual; fp64.  Sub-blocks are 8 x 16 pixels."""
    B, Cin, H, W = x.shape
    nc = Cin // 64
    cps = -(-nc // splits)
    pad = torch.zeros(B, Cin, H + 2, W + 2, dtype=torch.float64)
    pad[:, :, 1:-1, 1:-1] = x.double()
    wd = w.double()
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    total = torch.zeros(B, w.shape[0], H, W, dtype=torch.float64)
    for sp in range(-(-nc // cps)):
        part = torch.zeros_like(total)
        for c in range(sp * cps, min(nc, (sp + 1) * cps)):
            if mutant == "first slice of the last split" and sp == -(-nc // cps) - 1 and c == sp * cps:
                continue
            sl = slice(c * 64, (c + 1) * 64)
            for dy in range(3):
                for dx in range(3):
                    src = pad[:, sl, dy:dy + H, dx:dx + W]
                    term = torch.einsum("bchw,oc->bohw", src, wd[:, sl, dy, dx])
                    if mutant == "halo column" and dx == 0:                # the last sub-block column hangs over the right edge: its
                        ox = (W - 1) // 16 * 16                            # left halo column, read by tap dx = 0 of its first pixels
                        assert W % 16 != 0
                        term[:, :, :8, ox] = 0.0
                    if mutant == "taps swapped at the border" and dy == 1 and dx != 1:
                        other = torch.einsum("bchw,oc->bohw", src, wd[:, sl, 1, 2 - dx])
                        term = torch.where(border, other, term)
                    part += term
        total += part
    return total + bias.double()[None, :, None, None] + res.double()


def _old_bound_share(mutated, true):
    """of the outputs the mutant changes: the share whose fp16 value still lies within the tolerance tests' bound of the reference"""
    hit = mutated != true
    err = (E.round16(mutated).double() - true).abs()
    return float((err <= 1.5e-3 * true.abs() + 2e-3)[hit].float().mean()), int(hit.sum())


MUTANTS = [("gemm", "last k, last row", "integer"), ("gemm", "ring stage 0 twice", "integer"),
           ("conv192", "first slice of the last split", "integer"), ("conv64", "halo column", "integer"),
           ("conv64", "taps swapped at the border", "integer"), ("gemm", "rounded before the residual", "dyadic")]
MUTANT_SHARES = {}


@pytest.mark.parametrize("kind,mutant,regime", MUTANTS, ids=[m[1].replace(" ", "_").replace(",", "") for m in MUTANTS])
def test_the_detector_detects(kind, mutant, regime):
    """every mutant of the module docstring, in the other regime as well where it applies: the emulation without a mutant equals the
    reference (it is a summation order, and the order does not matter), with it the exact comparison fails - on the very element for
    the one-term mutant; and the share of changed outputs that the old bound passes on randn operands, printed, > 0 where the mutant
    moves a single term"""
    g = torch.Generator().manual_seed(len(mutant))
    if kind == "gemm":
        M, N, K = 200, 64, 704
        case = E.Case("linear", regime, (M, N, K), bias=True, res=True)
        rnd = {"x": torch.randn(M, K, generator=g).half(), "w": (torch.randn(N, K, generator=g) / K ** 0.5).half(),
               "bias": (torch.randn(N, generator=g) * 0.2).half(), "res": torch.randn(M, N, generator=g).half()}
        kw = {"round_acc": True} if mutant.startswith("rounded") else {"mutant": mutant}
        run = lambda o, **k: tiled_gemm(o["x"], o["w"], o["bias"], o["res"], **k)
    else:
        B, Cin, Cout, H, W = (1, 192, 64, 12, 12) if kind == "conv192" else (2, 64, 64, 9, 30)
        d = 0.5 if Cin > 64 else 0.75
        case = E.Case("conv", regime, (B, Cin, Cout, H, W), bias=True, res=True, dx=d, dw=d)
        rnd = {"x": torch.randn(B, Cin, H, W, generator=g).half(), "w": (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half(),
               "bias": (torch.randn(Cout, generator=g) * 0.2).half(), "res": torch.randn(B, Cout, H, W, generator=g).half()}
        kw = {"mutant": mutant, "splits": 2 if kind == "conv192" else 1}
        run = lambda o, **k: tiled_conv(o["x"], o["w"], o["bias"], o["res"], **k)
    E.check_exact(case)
    ref = E.reference(case)
    clean = {k: v for k, v in kw.items() if k == "splits"}
    assert torch.equal(run(ref.ops, **clean), ref.out)                                 # the tiled order is the plain sum
    bad = run(ref.ops, **kw)
    assert not torch.equal(E.round16(bad), ref.expected), mutant                       # the exact comparison fails
    if mutant == "last k, last row":
        moved = (ref.ops["x"][-1, -1].double() * ref.ops["w"][:, -1].double()) != 0
        assert moved.any() and torch.equal(E.round16(bad) != ref.expected, torch.cat([torch.zeros(199, 64, dtype=torch.bool), moved[None]]))
    true = run(rnd, **clean)
    share, changed = _old_bound_share(run(rnd, **kw), true)
    MUTANT_SHARES[mutant] = share
    print(f"\n{mutant}: {changed} outputs changed on randn operands, {100 * share:.0f} % of them within 1.5e-3 |ref| + 2e-3")
    if mutant == "last k, last row":
        assert share > 0
