"""Operands on which the GEMM and convolution kernels have exactly one correct output, the fp64 references of those outputs, and the
table of cases that tests/test_exact_sums_host.py (conditions, on the CPU) and tests/test_exact_sums_gpu.py (kernels) both walk.

fp16 operands that are small integers times powers of two multiply and add in fp32 without rounding while the sum of the magnitudes
of the terms of an output stays below 2^24: then ring depth, tile shape, split order, LDS staging and MFMA lane order all give the
same fp32 value, and the fp64 result rounded ONCE to fp16 is the only correct output.  A lost, doubled or misplaced product changes
that value on the element where it happens.  Two regimes, one seeded generator:

    integer   x in {-1, 0, 1}; w, bias, residual and the per-image add in {-2 .. 2}.  Every output is an integer of magnitude
              <= 2048: nothing rounds anywhere, and the producers' statistics (sums and sums of squares of the stored values) are
              exact integers below 2^24 as well.
    dyadic    the same integers scaled: x by 2^-3 - and by 2^9 in every eighth K column / input channel (k % 8 == 1), whose products
              are multiples of 16 -, w by 2^-5, bias / residual / add by 2^-8.  accumulator + bias + residual is still exact in
              fp32, but a multiple of 16 plus a multiple of 2^-8 needs more than the 11 significant bits of fp16 - the accumulator
              alone already does - so the epilogue's one rounding happens, and a kernel that rounds before it adds the residual
              rounds twice and differs.

Nothing here imports the GPU library."""
import dataclasses
import functools
import zlib

import numpy as np
import torch

import guard_band_refs as R

LIMIT = float(1 << 24)               # sums of magnitudes (in units of the regime's grid) stay below this: fp32 adds them exactly
INT_MAX = 2048                       # integer regime: |output| <= 2048 - every such integer is an fp16 value
REGIMES = ("integer", "dyadic")
X_EXP, X_HEAVY_EXP, W_EXP, E_EXP = -3, 9, -5, -8       # dyadic exponents of x, of x's heavy columns, of w, of bias / residual / add
HEAVY_EVERY, HEAVY_AT = 8, 1
GRID = {"integer": 1.0, "dyadic": 2.0 ** (X_EXP + W_EXP)}     # every term of an output is a multiple of this (E_EXP = X_EXP + W_EXP)


@dataclasses.dataclass(frozen=True)
class Case:
    """entry: the C entry point's family; shape: its dimensions (see _SHAPES); opt: sorted (key, value) pairs - mode, splits, groups,
    heads, res_rows, nchw, add; dx / dw: the share of non-zero elements of x and of w; sweep: the GPU test runs the case under every
    launch knob and the throughput profile, not only under the launch rule's own choice"""
    entry: str
    regime: str
    shape: tuple
    bias: bool = False
    res: bool = False
    dx: float = 0.75
    dw: float = 0.75
    opt: tuple = ()
    sweep: bool = False

    def get(self, key, default=0):
        return dict(self.opt).get(key, default)

    @property
    def id(self):
        epi = ("b" if self.bias else "") + ("r" if self.res else "") or "plain"
        opt = "".join(f"-{k}{v}" for k, v in self.opt)
        return f"{self.entry}-{'x'.join(map(str, self.shape))}-{epi}{opt}-{self.regime}"


_SHAPES = {"linear": "M N K", "splitk": "M N K", "ln": "M N K", "lt": "M N K", "rows": "M N K", "qkv": "B L C heads", "gn": "B L K N",
           "conv": "B Cin Cout h w", "up2x": "B Cin Cout h w", "conv_gn": "B Cin Cout h w", "fewcin": "B Cin Cout h w"}
CONV_ENTRIES = ("conv", "up2x", "conv_gn", "fewcin")


# ============================================================================= the generator
def _generator(case, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(repr((case.entry, case.shape, case.opt, case.bias, case.res, salt)).encode()))


def ints(g, shape, kmax, density):
    """int64 tensor: with probability `density` a value of {-kmax .. kmax} without 0 (uniform), else 0"""
    mag = torch.randint(1, kmax + 1, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    keep = torch.rand(shape, generator=g) < density
    return mag * sign * keep


def live_edges(g, v, dim):
    """the same integers with no zero in the first and the last element of every run of 64 along `dim` (K columns, input channels)
    nor in the last one of all: the terms at the edges of a K step, a channel slice and the whole sum exist for every output, so a
    kernel that drops or repeats one of them changes every output it does that to"""
    k = torch.arange(v.shape[dim])
    edge = ((k % 64 == 0) | (k % 64 == 63) | (k == v.shape[dim] - 1)).reshape([-1 if d == dim else 1 for d in range(v.dim())])
    fill = torch.randint(0, 2, v.shape, generator=g) * 2 - 1
    return torch.where(edge & (v == 0), fill, v)


def distinct_taps(w):
    """[Cout, Cin, 3, 3] integers -> the same with two channels per filter overwritten so that no two of its nine taps are equal
    as Cin-vectors: tap t = 3 dy + dx carries the pair (t // 3 - 1, t % 3 - 1) in two neighbouring channels of filter n, inside the
    first slice and off its edges (live_edges).  A kernel that reads a tap's weights for another tap never gets the same numbers."""
    Cout, Cin = w.shape[:2]
    assert Cin >= 4
    n = torch.arange(Cout)
    c = 1 + n % max(min(Cin, 64) - 3, 1)
    for t in range(9):
        w[n, c, t // 3, t % 3] = t // 3 - 1
        w[n, c + 1, t // 3, t % 3] = t % 3 - 1
    return w


def _x_exponents(K, regime):
    """per K column / input channel: the power of two x is scaled by"""
    e = torch.zeros(K, dtype=torch.float64)
    if regime == "dyadic":
        e += X_EXP
        e[HEAVY_AT::HEAVY_EVERY] = X_HEAVY_EXP
    return e


def _scaled(v, exp):
    """integers times 2^exp as fp16 (exact: at most 3 significant bits, exponents inside fp16's normal range)"""
    out = v.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.as_tensor(exp, dtype=torch.float64))
    h = out.half()
    assert torch.equal(h.double(), out)
    return h


def operands(case):
    """dict of fp16 CPU tensors: x, w and, where the case has them, bias, res, add - GEMMs: x [M, K], w [N, K], res [R, N];
    convolutions: x [B, Cin, h, w] (the source image), w [Cout, Cin, 3, 3], res [B, Cout, oh, ow], add [B, Cout]"""
    g = _generator(case)
    dy = case.regime == "dyadic"
    we, ee = (W_EXP, E_EXP) if dy else (0, 0)
    if case.entry in CONV_ENTRIES:
        B, Cin, Cout, h, w = case.shape
        xe = _x_exponents(Cin, case.regime)[None, :, None, None]
        ops = {"x": _scaled(live_edges(g, ints(g, (B, Cin, h, w), 1, case.dx), 1), xe),
               "w": _scaled(distinct_taps(live_edges(g, ints(g, (Cout, Cin, 3, 3), 2, case.dw), 1)), we)}
        _, (oh, ow) = R.conv_geometry(case.get("mode"), h, w)
        if case.entry == "up2x":
            oh, ow = 2 * h, 2 * w
        rshape, N, batch = (B, Cout, oh, ow), Cout, B
    else:
        if case.entry == "qkv":
            B, L, C, _ = case.shape
            M, N, K, batch = B * L, 3 * C, C, B
        elif case.entry == "gn":
            B, L, K, N = case.shape
            M, batch = B * L, B
        else:
            (M, N, K), batch = case.shape, 1
        ops = {"x": _scaled(live_edges(g, ints(g, (M, K), 1, case.dx), 1), _x_exponents(K, case.regime)[None, :]),
               "w": _scaled(live_edges(g, ints(g, (N, K), 2, case.dw), 1), we)}
        rshape = (case.get("res_rows") or M, N)
    if case.bias:
        ops["bias"] = _scaled(ints(g, (N,), 2, 0.75), ee)
    if case.res:
        ops["res"] = _scaled(ints(g, rshape, 2, 0.75), ee)
    if case.get("add"):
        ops["add"] = _scaled(ints(g, (batch, N), 2, 0.75), ee)
    return ops


# ============================================================================= fp64 references
def linear64(x, w, bias=None, res=None):
    """x @ w.T (+ bias) (+ residual row m % R) in fp64, as a plain sum over k"""
    y = torch.einsum("mk,nk->mn", x.double(), w.double())
    if bias is not None:
        y = y + bias.double()
    if res is not None:
        y = y + res.double().repeat(x.shape[0] // res.shape[0], 1)
    return y


def conv64(x, w, mode=R.PLAIN):
    """the nine taps of the 3x3 convolution written out in fp64: x [B, Cin, h, w] is read through the nearest-neighbour doubling
    (source pixel = destination >> 1) in the two upsampling modes - UPSAMPLE_CEIL to the odd target 2s - 1 -, zero outside the image;
    STRIDE2 keeps the even pixels of the stride-1 result, STRIDE2_PAD_BR (zero padding below and right only) the odd ones"""
    x, w = x.double(), w.double()
    (H, W), _ = R.conv_geometry(mode, x.shape[2], x.shape[3])
    if mode in (R.UPSAMPLE2X, R.UPSAMPLE_CEIL):
        x = x[:, :, torch.arange(H) >> 1][:, :, :, torch.arange(W) >> 1]
    pad = torch.zeros(x.shape[0], x.shape[1], H + 2, W + 2, dtype=torch.float64)
    pad[:, :, 1:-1, 1:-1] = x
    y = torch.zeros(x.shape[0], w.shape[0], H, W, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            y += torch.einsum("bchw,oc->bohw", pad[:, :, dy:dy + H, dx:dx + W], w[:, :, dy, dx])
    if mode == R.STRIDE2:
        y = y[:, :, ::2, ::2]
    elif mode == R.STRIDE2_PAD_BR:
        y = y[:, :, 1::2, 1::2]
    return y


def conv_epilogue64(y, bias=None, res=None, add=None):
    if bias is not None:
        y = y + bias.double()[None, :, None, None]
    if add is not None:
        y = y + add.double()[:, :, None, None]
    if res is not None:
        y = y + res.double()
    return y


def up2x_pack64(w):
    """[Cout, Cin, 3, 3] -> [4, Cout, 4, Cin] fp64: the sums of the taps that read one source pixel through the doubling
    (guard_band_refs.PHASE_TAPS), each a sum of one, two or four weights"""
    w = w.double()
    out = torch.zeros(4, w.shape[0], 4, w.shape[1], dtype=torch.float64)
    for (py, a), dys in R.PHASE_TAPS.items():
        for (px, b), dxs in R.PHASE_TAPS.items():
            for dy in dys:
                for dx in dxs:
                    out[2 * py + px, :, 2 * a + b, :] += w[:, :, dy, dx]
    return out


def round16(y):
    """fp64 -> fp16, one rounding to nearest even (numpy converts directly)"""
    return torch.from_numpy(y.contiguous().numpy().astype(np.float16))


def pixel_tiles(H, W):
    """([H W] the 8 x 16 pixel tile of every pixel, the tiles per image) as the convolution numbers them: row-major over the image"""
    per_row = (W + 15) // 16
    ty, tx = torch.arange(H)[:, None] // 8, torch.arange(W)[None, :] // 16
    return (ty * per_row + tx).reshape(-1), ((H + 7) // 8) * per_row


def conv_tile_width(W):
    """the convolution's tile width for an image of W columns (conv3x3.hip tile_width): 16, or 8 where that hangs over less"""
    if W % 16 == 0 or W % 8 == 0:
        return 16 if W % 16 == 0 else 8
    return 16 if (W + 15) // 16 * 16 - W <= (W + 7) // 8 * 8 - W else 8


def row_tiles(L, rows):
    """the same for the GEMM that emits GroupNorm partial sums: `rows` tiles of L / rows consecutive token rows per image"""
    return torch.arange(L) // (L // rows), rows


def group_partials(stored, tile, ntiles, groups):
    """What the producers' epilogues emit (gn_partials.h), restated in fp64: part[b][pt][g][which] = (sum, sum of squares) of the
    stored fp16 values `stored` [B, hw, C] over the pixels of tile pt and the channels of group g that lie in the 64-channel tile
    where g begins (which = 0) or in the next one (which = 1: groups that cross a 64-channel boundary only).  Plain sums about zero,
    no pivot.  NaN marks the slots no producer writes."""
    v = stored.double()
    B, _, C = v.shape
    cpg = C // groups
    part = torch.full((B, ntiles, groups, 2, 2), float("nan"), dtype=torch.float64)
    for g in range(groups):
        c0, c1 = g * cpg, (g + 1) * cpg
        cut = min(c1, (c0 // 64 + 1) * 64)
        for which, (a, b) in enumerate(((c0, cut), (cut, c1))):
            if a < b:
                seg = v[:, :, a:b]
                part[:, :, g, which, 0] = torch.zeros(B, ntiles, dtype=torch.float64).index_add_(1, tile, seg.sum(-1))
                part[:, :, g, which, 1] = torch.zeros(B, ntiles, dtype=torch.float64).index_add_(1, tile, (seg * seg).sum(-1))
    return part


def gn_tilings(case):
    """the (tile, ntiles) pairs the case's GroupNorm partial sums can be emitted at: the convolution's 8 x 16 pixel tiles; for the
    GEMM both tile heights (64 and 128 token rows) that divide the image's rows - the launch knob decides which one runs"""
    if case.entry == "conv_gn":
        _, (oh, ow) = R.conv_geometry(case.get("mode"), case.shape[3], case.shape[4])
        return [pixel_tiles(oh, ow)]
    L = case.shape[1]
    return [row_tiles(L, L // bm) for bm in (64, 128) if L % bm == 0]


@dataclasses.dataclass
class Reference:
    ops: dict          # the operands
    out: torch.Tensor  # fp64: GEMMs [M, N]; convolutions [B, Cout, oh, ow]
    mag: torch.Tensor  # fp64, same shape: the sum of the magnitudes of every term of the element, epilogue included
    expected: torch.Tensor   # round16(out)


@functools.lru_cache(maxsize=4)
def reference(case):
    o = operands(case)
    absd = {k: v.abs() for k, v in o.items()}
    outs = []
    for t in (o, absd):
        if case.entry in CONV_ENTRIES:
            mode = R.UPSAMPLE2X if case.entry == "up2x" else case.get("mode")
            outs.append(conv_epilogue64(conv64(t["x"], t["w"], mode), t.get("bias"), t.get("res"), t.get("add")))
        else:
            outs.append(linear64(t["x"], t["w"], t.get("bias"), t.get("res")))
    return Reference(o, outs[0], outs[1], round16(outs[0]))


def rows_of(ref_out):
    """[B, C, H, W] -> [B, H W, C]"""
    return ref_out.permute(0, 2, 3, 1).reshape(ref_out.shape[0], -1, ref_out.shape[1])


def stored_rows(case, ref):
    """the stored fp16 tensor as [B, pixels or token rows, C] for group_partials"""
    if case.entry == "conv_gn":
        return rows_of(ref.expected)
    B, L, _, N = case.shape
    return ref.expected.reshape(B, L, N)


def check_exact(case):
    """The conditions under which `torch.equal` against reference(case).expected is the right test, asserted for every output
    element and every emitted statistic of the case; returns the figures.  A case that breaks one gets a lower density."""
    ref = reference(case)
    grid = GRID[case.regime]
    units = ref.mag / grid
    assert float(units.max()) < LIMIT, (case.id, float(units.max()))
    assert torch.equal(ref.out / grid, torch.round(ref.out / grid)), case.id           # every term lies on the regime's grid
    rounded = int((ref.expected.double() != ref.out).sum())
    assert torch.isfinite(ref.expected).all(), case.id
    if case.regime == "integer":
        assert float(ref.out.abs().max()) <= INT_MAX and rounded == 0, (case.id, float(ref.out.abs().max()))
    else:
        assert rounded > 0, case.id                                                     # the one rounding does happen
    figures = {"sum|terms|": float(units.max()), "|out|": float(ref.out.abs().max()), "rounded": rounded, "sumsq": 0.0}
    if case.regime == "integer" and case.entry == "ln":
        figures["sumsq"] = float(R.row_block_stats(ref.expected)[0][..., 1].max())
    if case.regime == "integer" and case.entry in ("gn", "conv_gn"):
        for tile, ntiles in gn_tilings(case):
            part = group_partials(stored_rows(case, ref), tile, ntiles, case.get("groups"))
            figures["sumsq"] = max(figures["sumsq"], float(part[..., 1][~torch.isnan(part[..., 1])].max()))
    assert figures["sumsq"] < LIMIT, (case.id, figures["sumsq"])      # sums of squares bound the sums of the same integers
    return figures


# ============================================================================= the case table
def _linear_cases():
    out = []
    for regime in REGIMES:
        for M in (1, 63, 65, 129, 200):
            for N in (64, 192, 256):
                for K in (64, 256, 704):        # 1, 4 and 11 K steps: the 3-ring wraps once / the 2-ring twice; both end mid-ring
                    for epi in (False, True):
                        out.append(Case("linear", regime, (M, N, K), bias=epi, res=epi, sweep=True))
        out.append(Case("linear", regime, (129, 64, 5120), bias=True, res=True, dx=0.125, dw=0.125))          # 80 K steps
        for M in (256, 384):                    # residual row m % 128
            out.append(Case("linear", regime, (M, 192, 256), bias=True, res=True, opt=(("res_rows", 128),), sweep=True))
        # K = 704 = 11 steps: 6 + 5 | 4 + 4 + 3 | 3 + 3 + 3 + 2;  K = 320 = 5 steps asked in 4 splits: 2 + 2 + 1 in three
        for M, N, K, splits in ((70, 128, 704, 2), (70, 128, 704, 3), (129, 64, 704, 4), (70, 64, 320, 4)):
            out.append(Case("splitk", regime, (M, N, K), bias=True, res=True, opt=(("splits", splits),), sweep=True))
        for shape in ((2, 65, 128, 2), (1, 129, 192, 3)):
            out.append(Case("qkv", regime, shape, bias=True, sweep=True))
        for M in (65, 129):
            for N in (192, 256):
                out.append(Case("ln", regime, (M, N, 256), bias=True, res=True, sweep=True))
        # groups inside a 64-column tile | 48 channels per group: groups 1 and 2 cross a tile boundary | 192 rows per image: three
        # 64-row tiles, no whole number of 128-row ones
        for shape, groups in (((2, 64, 64, 64), 8), ((3, 128, 192, 192), 4), ((2, 192, 64, 128), 32)):
            out.append(Case("gn", regime, shape, bias=True, res=True, opt=(("groups", groups),), sweep=True))
        for M in (1, 5, 8):
            for K in (72, 1032):                # 9 and 129 16-byte chunks for 64 lanes: a partly idle wave, a ragged third round
                out.append(Case("rows", regime, (M, 18, K), bias=True))
    out.append(Case("lt", "integer", (128, 128, 256), bias=True, res=True))
    return out


def _conv_cases():
    out = []
    both = {"bias": True, "res": True}
    for regime in REGIMES:
        # (B, Cin, Cout, h, w, splits): one pixel | 8-wide ragged | 16-wide ragged, two channel tiles | 8-wide tiles holding two
        # images' sub-blocks, B odd | 2 slices in 2 splits | 3 in 3 | 3 in 2: 2 + 1 | 20 slices, sparse
        for shape, splits, d in (((1, 64, 64, 1, 1), 0, 0.75), ((1, 64, 64, 5, 7), 0, 0.75), ((3, 64, 128, 9, 30), 0, 0.75),
                                 ((5, 64, 64, 8, 8), 0, 0.75), ((2, 128, 64, 12, 20), 2, 0.5), ((2, 192, 64, 24, 48), 3, 0.5),
                                 ((1, 192, 64, 12, 12), 2, 0.5), ((1, 1280, 64, 8, 8), 0, 0.125)):
            sweep = shape in ((3, 64, 128, 9, 30), (2, 128, 64, 12, 20))
            out.append(Case("conv", regime, shape, dx=d, dw=d, opt=(("splits", splits),), sweep=sweep, **both))
        for shape in ((1, 64, 64, 5, 7), (3, 64, 128, 9, 30)):
            for bias, res in ((True, False), (False, True), (False, False)):
                out.append(Case("conv", regime, shape, bias=bias, res=res))
        for shape in ((2, 64, 40, 5, 7), (2, 64, 72, 9, 30), (2, 64, 100, 5, 7)):      # ragged last channel tile
            out.append(Case("conv", regime, shape, **both))
        for mode in (R.UPSAMPLE2X, R.UPSAMPLE_CEIL, R.STRIDE2, R.STRIDE2_PAD_BR):
            even = mode == R.STRIDE2_PAD_BR
            for (B, Cin, Cout, h, w), splits, d in (((2, 64, 64, 5, 7), 0, 0.75), ((3, 64, 128, 9, 30), 0, 0.75), ((2, 128, 64, 7, 11), 2, 0.5)):
                shape = (B, Cin, Cout, h + h % 2, w + w % 2) if even else (B, Cin, Cout, h, w)
                out.append(Case("conv", regime, shape, dx=d, dw=d, opt=(("mode", mode), ("splits", splits)), **both))
        for shape, res in (((2, 64, 4, 5, 7), False), ((1, 64, 4, 9, 17), True)):       # conv_out: 4 channels, channel-major
            out.append(Case("conv", regime, shape, bias=True, res=res, opt=(("nchw", 1),)))
        for shape, splits, d in (((1, 64, 64, 3, 5), 0, 0.75), ((3, 128, 64, 4, 4), 0, 0.5), ((2, 128, 64, 3, 16), 2, 0.5)):
            out.append(Case("up2x", regime, shape, bias=True, dx=d, dw=d, opt=(("splits", splits),)))
        # 9 x 30 | 8 x 8: the 8-wide tiles emit no statistics, the entry refuses (conv_tile_width) | 8 x 16: one whole tile per image,
        # four channels per group | UPSAMPLE_CEIL 5 x 8 -> 9 x 15 | 48 channels per group: two of four cross a channel tile | add
        for shape, groups, mode, add, res in (((2, 64, 64, 9, 30), 8, R.PLAIN, 0, False), ((3, 64, 128, 8, 8), 32, R.PLAIN, 0, False),
                                              ((3, 64, 128, 8, 16), 32, R.PLAIN, 0, False),
                                              ((2, 64, 64, 5, 8), 8, R.UPSAMPLE_CEIL, 0, True), ((2, 64, 192, 9, 16), 4, R.PLAIN, 0, True),
                                              ((3, 64, 64, 9, 30), 8, R.PLAIN, 1, True)):
            out.append(Case("conv_gn", regime, shape, bias=True, res=res, dx=0.5, dw=0.5, opt=(("add", add), ("groups", groups), ("mode", mode))))
        for shape in ((2, 4, 64, 5, 7), (1, 4, 320, 9, 17), (2, 9, 64, 9, 17), (1, 9, 320, 5, 7)):
            out.append(Case("fewcin", regime, shape, bias=True))
    return out


CASES = tuple(_linear_cases() + _conv_cases())
assert len({c.id for c in CASES}) == len(CASES)


def cases(entry, regimes=REGIMES):
    return [c for c in CASES if c.entry == entry and c.regime in regimes]
