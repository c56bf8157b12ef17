"""The case table of the row-isolation tests: every batched kernel, at the smallest shape at which two images meet in one tile,
wave or launch, with the owner map of every operand and output (tests/isolation.py).

Built on the CPU from seeded generators, with nothing of the GPU library imported: a case's `make_run(ops, lib)` is handed the
library by tests/test_isolation_gpu.py and returns the `run(operands) -> outputs` of `isolation.check_isolated`; the owner maps are
checked for completeness by tests/test_isolation_host.py on a machine without a GPU.  A new batched kernel adds a row here.

Three images everywhere, the victim in the middle (B = 3, j = 1), so that it has a neighbour in memory on both sides; the sampler
entries use four slots.  N, K, groups and heads are those of the smallest case of the entry in tests/test_guard_bands_gpu.py.
"""
from dataclasses import dataclass, field

import torch

import guard_band_refs as R
import isolation as iso
from inputs import attn_inputs

B, J = 3, 1
CL = torch.channels_last


@dataclass
class Case:
    id: str
    family: str
    operands: dict                     # name -> CPU tensor (the logical operand: `run` lays it out for the kernel)
    owners: dict                       # name -> owner map, for every operand and every output
    outputs: tuple                     # the names `run` returns
    make_run: object                   # (ops, lib) -> run
    B: int = B
    j: int = J
    seam_axes: dict = field(default_factory=dict)
    victim_rules: dict = field(default_factory=dict)
    frozen: tuple = ()
    sweep: str = ""                    # the launch knobs tests/test_isolation_gpu.py repeats the case under


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * s for i, s in enumerate(seed)) % (1 << 31))


def _rows(shape, dim=0, n=B):
    return iso.owner_rows(n, tuple(shape), dim)


def _ragged_rows(shape):
    """7 rows: images 0 / 1 / 2 hold rows [0, 2) / [2, 5) / [5, 7) - the victim aligned to neither 4 nor 8"""
    assert shape[0] == 7
    own = torch.tensor([0, 0, 1, 1, 1, 2, 2])
    return own.view(7, *([1] * (len(shape) - 1))).expand(tuple(shape)).contiguous()


def _row_owner(shape):
    return _ragged_rows(shape) if shape[0] == 7 else _rows(shape)


# ============================================================================= GEMM family (gemm.hip)
def _gemm_operands(M, N, K, seed, R_rows=None):
    g = _gen(M, N, K, seed)
    x = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    b = (torch.randn(N, generator=g) * 0.2).half()
    r = torch.randn(R_rows or M, N, generator=g).half()
    return x, w, b, r


def _linear(id, M, N, K, epilogue, geglu=False, R_rows=None, sweep="stages"):
    x, w, b, r = _gemm_operands(M, N, K, 1, R_rows)
    n_out = N // 2 if geglu else N
    operands, owners = {"x": x, "w": w}, {"x": _rows(x.shape), "w": iso.shared(w.shape), "out": _rows((M, n_out))}
    if epilogue or geglu:
        operands["b"], owners["b"] = b, iso.shared(b.shape)
    if epilogue and not geglu:
        operands["r"] = r
        owners["r"] = _rows(r.shape) if R_rows is None else iso.shared(r.shape)      # a wrapped residual is every image's

    def make_run(ops, lib):
        def run(o):
            plan = ops._linear_plan(o["x"], o["w"], o.get("b"), o.get("r"), geglu, True)
            assert plan[0] == ops.LINEAR_KERNEL and plan[5] is None, "linear: not the kernel route"
            return {"out": ops.linear(o["x"], o["w"], o.get("b"), residual=o.get("r"), geglu=geglu, prefer_kernel=True)}
        return run
    return Case(id, "gemm", operands, owners, ("out",), make_run, sweep=sweep)


def _linear_ln_stats(M, N, K):
    """M = 120 lies below the row window of ops.linear_kernel_covers (128 rows): there the entry is called directly, as
    tests/test_guard_bands_gpu.py calls it (it has no other route and raises on refusal); M = 144 is the smallest 3 x 8k rows inside
    the window, where the route question the callers ask is asserted too"""
    a, wo, bo, xres = _gemm_operands(M, N, K, 4)
    xres = (xres.float() * 2 + 0.7).half()
    operands = {"a": a, "w": wo, "b": bo, "xres": xres}
    owners = {"a": _rows(a.shape), "w": iso.shared(wo.shape), "b": iso.shared(bo.shape), "xres": _rows(xres.shape),
              "out": _rows((M, N)), "stats": _rows((M, N // 64, 2))}

    def make_run(ops, lib):
        def run(o):
            assert ops.linear_kernel_can(o["a"], o["w"], o["b"], o["xres"])
            assert M < 128 or ops.linear_kernel_covers(M, N, K, o["a"].dtype), "linear_ln: outside the kernel's window"
            out, stats = ops.linear_ln(o["a"], o["w"], o["b"], residual=o["xres"], ln_stats=True)
            return {"out": out, "stats": stats}
        return run
    return Case(f"linear_ln-stats-M{M}", "gemm", operands, owners, ("out", "stats"), make_run, sweep="profile")


def _linear_ln_folded(M, N):
    g = _gen(M, N, 5)
    s = (torch.randn(M, N, generator=g) * 2 + 0.7).half()
    st = R.row_block_stats(s)[0].float()                                   # what the producer's epilogue emits: [M, N / 64, 2]
    gamma, beta = (torch.randn(N, generator=g) * 0.3 + 1).half(), (torch.randn(N, generator=g) * 0.2).half()
    w, b = (torch.randn(N, N, generator=g) / N ** 0.5).half(), (torch.randn(N, generator=g) * 0.2).half()
    operands = {"s": s, "st": st, "w": w, "b": b, "gamma": gamma, "beta": beta}
    owners = {"s": _rows(s.shape), "st": _rows(st.shape), "out": _rows((M, N)),
              **{n: iso.shared(operands[n].shape) for n in ("w", "b", "gamma", "beta")}}

    def make_run(ops, lib):
        def run(o):
            w2, b2, cvec = ops.fold_layernorm(o["w"], o["b"], o["gamma"], o["beta"])
            assert ops.linear_kernel_can(o["s"], w2, b2, None)
            assert M < 128 or ops.linear_kernel_covers(M, N, N, o["s"].dtype), "linear_ln: outside the kernel's window"
            return {"out": ops.linear_ln(o["s"], w2, b2, ln=(o["st"].contiguous(), cvec, 1e-5))}
        return run
    return Case(f"linear_ln-folded-M{M}", "gemm", operands, owners, ("out",), make_run, sweep="profile")


def _linear_qkv(L, C, H):
    g = _gen(B, L, C, H)
    x = (torch.randn(B, L, C, generator=g) * 1.3 + 0.2).half()
    w = (torch.randn(3 * C, C, generator=g) / C ** 0.5).half()
    b = (torch.randn(3 * C, generator=g) * 0.2).half()
    d = C // H
    operands = {"x": x, "w": w, "b": b}
    owners = {"x": _rows(x.shape), "w": iso.shared(w.shape), "b": iso.shared(b.shape),
              **{n: _rows((B, L, H, d)) for n in ("q", "k", "v")}}

    def make_run(ops, lib):
        def run(o):
            # the entry's own coverage answer includes the row window (128 rows): asserted where the shape lies inside it; the
            # 3 x 40-row case lies below it and goes to the entry directly, which raises on refusal (no other route)
            assert ops.linear_kernel_can(o["x"], o["w"], o["b"], None)
            assert B * L < 128 or ops.linear_qkv_covers(o["x"], o["w"], H), "linear_qkv: not covered"
            q, k, v = ops.linear_qkv(o["x"], o["w"], o["b"], H)
            return {"q": q, "k": k, "v": v}
        return run
    return Case(f"linear_qkv-L{L}", "gemm", operands, owners, ("q", "k", "v"), make_run, sweep="profile")


def _linear_splitk(M, N, K, splits):
    x, w, b, r = _gemm_operands(M, N, K, 7)
    operands = {"x": x, "w": w, "b": b, "r": r}
    owners = {"x": _rows(x.shape), "w": iso.shared(w.shape), "b": iso.shared(b.shape), "r": _rows(r.shape), "out": _rows((M, N))}

    def make_run(ops, lib):
        def run(o):
            assert lib.dsc_linear_splitk_workspace_bytes(M, N, K, splits) > 0
            return {"out": ops.linear_splitk(o["x"], o["w"], o["b"], o["r"], splits=splits)}
        return run
    return Case(f"linear_splitk-K{K}-s{splits}", "gemm", operands, owners, ("out",), make_run, sweep="profile")


def _linear_rows(M, N, K):
    g = _gen(M, N, K)
    x = torch.randn(M, K, generator=g).half()
    w, b = (torch.randn(N, K, generator=g) / K ** 0.5).half(), (torch.randn(N, generator=g) * 0.1).half()
    operands = {"x": x, "w": w, "b": b}
    owners = {"x": _row_owner(x.shape), "w": iso.shared(w.shape), "b": iso.shared(b.shape), "out": _row_owner((M, N))}

    def make_run(ops, lib):
        return lambda o: {"out": ops.linear_rows(o["x"], o["w"], o["b"], silu_out=True)}
    return Case(f"linear_rows-N{N}", "gemm", operands, owners, ("out",), make_run, sweep="profile")


def _linear_lt(M, N, K):
    x, w, b, r = _gemm_operands(M, N, K, 8)
    operands = {"x": x, "w": w, "b": b, "r": r}
    owners = {"x": _rows(x.shape), "w": iso.shared(w.shape), "b": iso.shared(b.shape), "r": _rows(r.shape), "out": _rows((M, N))}

    def make_run(ops, lib):
        def run(o):
            out = torch.empty((M, N), dtype=torch.float16, device=o["x"].device)
            rc = lib.dsc_linear_lt_f16(ops._p(o["x"]), ops._p(o["w"]), ops._p(o["b"]), ops._p(o["r"]), ops._p(out), M, N, K, K, N, N, 0,
                                       ops._stream_ptr(out))
            assert rc == 0, rc
            return {"out": out}
        return run
    return Case("linear_lt", "gemm_lt", operands, owners, ("out",), make_run)


def _linear_gn(L, K, N, groups):
    M = B * L
    x, w, b, r = _gemm_operands(M, N, K, 6)
    assert not bool(R.straddles(N, groups).any())              # slot [g][1] is never written at this N: slot 0 is the output
    operands = {"x": x.reshape(B, L, K), "w": w, "b": b, "r": r.reshape(B, L, N)}
    owners = {"x": _rows((B, L, K)), "w": iso.shared(w.shape), "b": iso.shared(b.shape), "r": _rows((B, L, N)),
              "out": _rows((B, L, N)), "part": _rows((B, 2, groups, 2))}

    def make_run(ops, lib):
        def run(o):
            got = ops.linear_gn(o["x"], o["w"], o["b"], o["r"], L, groups)
            assert got is not None, "linear_gn: the variant refuses the shape"
            y, part = got
            sums = part.buf[..., 0, :]                        # [B, rows, G, 2]: one row per 128-row tile, two per 64-row tile
            assert sums.shape[1] in (1, 2)
            return {"out": y, "part": sums.repeat(1, 2 // sums.shape[1], 1, 1).contiguous()}
        return run
    case = Case("linear_gn", "gemm_gn", operands, owners, ("out", "part"), make_run, sweep="stages_gn")
    case.gn_dims = (M, N, K, L, groups)
    return case


def gemm_cases():
    M = 120                            # 3 x 40 rows: the 64-row tile [0, 64) holds images 0 and 1, the 128-row tile all three
    return [_linear("linear-plain", M, 64, 64, False), _linear("linear-bias-residual", M, 64, 64, True),
            _linear("linear-wrapped-residual", 3 * 128, 192, 64, True, R_rows=128),
            _linear("linear-geglu", M, 128, 64, False, geglu=True, sweep="stages_no64"),
            _linear_ln_stats(M, 192, 64), _linear_ln_folded(M, 192), _linear_qkv(40, 64, 2),
            # 3 x 48 rows: the same seams ([0, 64) holds images 0 and 1, [0, 128) all three) inside the callers' row window
            _linear_ln_stats(144, 192, 64), _linear_ln_folded(144, 192), _linear_qkv(48, 64, 2),
            _linear_splitk(M, 64, 1024, 0), _linear_splitk(M, 128, 512, 3),
            _linear_rows(7, 8, 320), _linear_rows(3, 320, 320), _linear_lt(M, 64, 64), _linear_gn(128, 64, 64, 8)]


# ============================================================================= 3x3 convolution (conv3x3.hip, conv_in.hip)
_CONV_KW = {R.PLAIN: lambda size: {}, R.UPSAMPLE2X: lambda size: {"upsample": True}, R.UPSAMPLE_CEIL: lambda size: {"upsample_size": size},
            R.STRIDE2: lambda size: {"stride2_ceil": True}, R.STRIDE2_PAD_BR: lambda size: {"stride2_pad_br": True}}
_MODE_NAME = {R.PLAIN: "plain", R.UPSAMPLE2X: "upsample", R.UPSAMPLE_CEIL: "upsample-ceil", R.STRIDE2: "stride2", R.STRIDE2_PAD_BR: "stride2-pad-br"}


def _conv_operands(Cin, Cout, h, w, seed):
    g = _gen(B, Cin, Cout, h, w, seed)
    x = torch.randn(B, Cin, h, w, generator=g).half()
    wt = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half()
    b = (torch.randn(Cout, generator=g) * 0.2).half()
    return g, x, wt, b


def _conv(h, w, mode, Cin=64, Cout=64, splits=0, nchw=False, residual=True):
    g, x, wt, b = _conv_operands(Cin, Cout, h, w, mode)
    (H, W), (oh, ow) = R.conv_geometry(mode, h, w)
    operands = {"x": x, "w": wt, "b": b}
    owners = {"x": _rows(x.shape), "w": iso.shared(wt.shape), "b": iso.shared(b.shape), "out": _rows((B, Cout, oh, ow))}
    seams = {"x": 2}
    if residual:
        operands["r"], owners["r"], seams["r"] = torch.randn(B, Cout, oh, ow, generator=g).half(), _rows((B, Cout, oh, ow)), 2

    def make_run(ops, lib):
        def run(o):
            xd, wd = o["x"].contiguous(memory_format=CL), o["w"].contiguous(memory_format=CL)
            assert lib.dsc_conv3x3_supported(B, H, W, Cin, Cout), "conv3x3: shape not covered"
            res = o["r"].contiguous(memory_format=CL) if residual else None
            return {"out": ops.conv3x3(xd, wd, o["b"], residual=res, splits=splits, out_nchw=nchw, **_CONV_KW[mode]((H, W)))}
        return run
    id = f"conv3x3-{_MODE_NAME[mode]}-{h}x{w}" + (f"-splits{splits}" if splits else "") + ("-nchw" if nchw else "")
    return Case(id, "conv", operands, owners, ("out",), make_run, seam_axes=seams, sweep="conv")


def _conv_gn(H, W, Cin, Cout, groups):
    g, x, wt, b = _conv_operands(Cin, Cout, H, W, 9)
    add, r = (torch.randn(B, Cout, generator=g) * 0.5).half(), torch.randn(B, Cout, H, W, generator=g).half()
    gamma, beta = (1 + 0.1 * torch.randn(Cout, generator=g)).half(), (0.1 * torch.randn(Cout, generator=g)).half()
    assert not bool(R.straddles(Cout, groups).any())
    rows = ((H + 7) // 8) * ((W + 15) // 16)
    operands = {"x": x, "w": wt, "b": b, "add": add, "r": r, "gamma": gamma, "beta": beta}
    owners = {"x": _rows(x.shape), "add": _rows(add.shape), "r": _rows(r.shape), "out": _rows((B, Cout, H, W)),
              "part": _rows((B, rows, groups, 2)), "y": _rows((B, Cout, H, W)),
              **{n: iso.shared(operands[n].shape) for n in ("w", "b", "gamma", "beta")}}

    def make_run(ops, lib):
        def run(o):
            xd, wd, rd = (o[n].contiguous(memory_format=CL) for n in ("x", "w", "r"))
            assert ops.conv3x3_gn_rows(xd, wd, groups) == rows, "conv3x3_gn: not covered"
            out = ops.conv3x3_gn(xd, wd, groups, bias=o["b"], add=o["add"], residual=rd)
            part = ops.gn_partials_of(out)
            # groupnorm_apply_nhwc from the producer's partial sums: the consumer of the same launch pair
            y = ops.groupnorm_apply_nhwc(out, part, groups, o["gamma"], o["beta"], 1e-5, True)
            return {"out": out, "part": part.buf[..., 0, :].contiguous(), "y": y}
        return run
    return Case(f"conv3x3_gn+groupnorm_apply-{H}x{W}", "conv", operands, owners, ("out", "part", "y"), make_run,
                seam_axes={"x": 2, "r": 2})


def _conv_up2x(h, w, splits):
    Cin, Cout = (128, 64) if splits else (64, 64)
    _, x, wt, b = _conv_operands(Cin, Cout, h, w, 11)
    operands = {"x": x, "w": wt, "b": b}
    owners = {"x": _rows(x.shape), "w": iso.shared(wt.shape), "b": iso.shared(b.shape), "out": _rows((B, Cout, 2 * h, 2 * w))}

    def make_run(ops, lib):
        def run(o):
            xd, wd = o["x"].contiguous(memory_format=CL), o["w"].contiguous(memory_format=CL)
            assert ops.conv3x3_up2x_supported(xd, wd), "conv3x3_up2x: shape not covered"
            return {"out": ops.conv3x3_up2x(xd, ops.conv3x3_up2x_pack(wd), o["b"], splits=splits)}
        return run
    return Case(f"conv3x3_up2x-{h}x{w}-splits{splits}", "conv", operands, owners, ("out",), make_run, seam_axes={"x": 2}, sweep="conv")


def _conv_fewcin(h, w, Cin=4, Cout=64):
    _, x, wt, b = _conv_operands(Cin, Cout, h, w, 12)
    operands = {"x": x, "w": wt, "b": b}
    owners = {"x": _rows(x.shape), "w": iso.shared(wt.shape), "b": iso.shared(b.shape), "out": _rows((B, Cout, h, w))}

    def make_run(ops, lib):
        def run(o):
            w_t = o["w"].reshape(Cout, Cin * 9).t().contiguous()
            return {"out": ops.conv3x3_fewcin(o["x"], w_t, o["b"], Cout)}
        return run
    return Case(f"conv3x3_fewcin-{h}x{w}", "conv", operands, owners, ("out",), make_run, seam_axes={"x": 2})


def conv_cases():
    out = []
    for h in (8, 12):                  # 8 x 8: one 128-pixel tile holds sub-blocks of two images; 12 x 12: ragged sub-blocks
        out += [_conv(h, h, mode) for mode in (R.PLAIN, R.UPSAMPLE2X, R.UPSAMPLE_CEIL, R.STRIDE2, R.STRIDE2_PAD_BR)]
        out += [_conv(h, h, R.PLAIN, Cin=128, splits=2), _conv(h, h, R.PLAIN, nchw=True, residual=False),
                _conv_up2x(h, h, 0), _conv_up2x(h, h, 2), _conv_fewcin(h, h)]
    # dsc_conv3x3_gn_nhwc_f16 emits statistics from the 16-wide tiles only: 8 x 8 and 12 x 12 take the 8-wide kernel and are refused
    # before any launch (tests/test_guard_bands_gpu.py::test_conv3x3_gn_nhwc_f16), so its seam is at the smallest image it takes
    out.append(_conv_gn(16, 16, 64, 64, 8))
    return out


# ============================================================================= normalisation and row kernels
def _gn_operands(C, hw, seed):
    g = _gen(B, C, hw, seed)
    x = (torch.randn(B, C, hw, generator=g) * 1.7 + 0.6).half()
    gamma, beta = (torch.randn(C, generator=g) * 0.5 + 1).half(), (torch.randn(C, generator=g) * 0.3).half()
    add = (torch.randn(B, C, generator=g) * 0.8).half()
    return x, gamma, beta, add


def _groupnorm_nchw(C, hw, groups):
    x, gamma, beta, _ = _gn_operands(C, hw, 1)
    operands = {"x": x.view(B, C, hw, 1), "gamma": gamma, "beta": beta}
    owners = {"x": _rows((B, C, hw, 1)), "gamma": iso.shared(gamma.shape), "beta": iso.shared(beta.shape), "y": _rows((B, C, hw, 1))}
    return Case("groupnorm_silu-nchw", "norm", operands, owners, ("y",),
                lambda ops, lib: lambda o: {"y": ops.groupnorm_silu(o["x"], groups, o["gamma"], o["beta"], 1e-5, True)},
                seam_axes={"x": 2})


def _groupnorm_nhwc(C, hw, groups, with_add):
    x, gamma, beta, add = _gn_operands(C, hw, 2)
    tok = x.transpose(1, 2).contiguous()
    operands = {"x": tok, "gamma": gamma, "beta": beta}
    owners = {"x": _rows(tok.shape), "gamma": iso.shared(gamma.shape), "beta": iso.shared(beta.shape), "y": _rows(tok.shape)}
    if with_add:
        operands["add"], owners["add"] = add, _rows(add.shape)
    return Case("groupnorm_silu_nhwc" + ("-add" if with_add else ""), "norm", operands, owners, ("y",),
                lambda ops, lib: lambda o: {"y": ops.groupnorm_silu_nhwc(o["x"], groups, o["gamma"], o["beta"], 1e-5, True, add=o.get("add"))},
                sweep="gn")


def _groupnorm_cat(C1, C2, hw, groups):
    C = C1 + C2
    x, gamma, beta, add = _gn_operands(C, hw, 3)
    tok = x.transpose(1, 2).contiguous()
    x1, x2 = tok[..., :C1].contiguous(), tok[..., C1:].contiguous()
    operands = {"x1": x1, "x2": x2, "gamma": gamma, "beta": beta, "add": add}
    owners = {"x1": _rows(x1.shape), "x2": _rows(x2.shape), "add": _rows(add.shape), "gamma": iso.shared(gamma.shape),
              "beta": iso.shared(beta.shape), "y": _rows((B, hw, C)), "cat": _rows((B, hw, C))}

    def make_run(ops, lib):
        img = lambda t: t.reshape(B, hw, 1, t.shape[-1]).permute(0, 3, 1, 2)                 # channels_last [B, c, hw, 1]
        def run(o):
            a, b = img(o["x1"].contiguous()), img(o["x2"].contiguous())
            assert ops.groupnorm_cat_covers(a, b), "groupnorm_silu_nhwc_cat: not covered"
            y, cat = ops.groupnorm_silu_nhwc_cat(a, b, groups, o["gamma"], o["beta"], 1e-5, True, add=o["add"])
            return {"y": R.rows_of(y).reshape(B, hw, C), "cat": R.rows_of(cat).reshape(B, hw, C)}
        return run
    return Case("groupnorm_silu_nhwc_cat", "norm", operands, owners, ("y", "cat"), make_run, sweep="gn_cat")


def _add_layernorm(rows, C, with_a):
    g = _gen(rows, C)
    x, a = (torch.randn(rows, C, generator=g) * 2 + 0.3).half(), torch.randn(rows, C, generator=g).half()
    gamma, beta = (torch.randn(C, generator=g) * 0.3 + 1).half(), (torch.randn(C, generator=g) * 0.2).half()
    own = _row_owner((rows, C))
    operands = {"x": x, "gamma": gamma, "beta": beta}
    owners = {"x": own, "gamma": iso.shared(gamma.shape), "beta": iso.shared(beta.shape), "s": own, "y": own}
    if with_a:
        operands["a"], owners["a"] = a, own

    def make_run(ops, lib):
        def run(o):
            s, y = ops.add_layernorm(o["x"], o.get("a"), o["gamma"], o["beta"])
            return {"s": s, "y": y}
        return run
    return Case(f"add_layernorm-{rows}x{C}" + ("-a" if with_a else ""), "norm", operands, owners, ("s", "y"), make_run)


def _softmax_rows(rows, n):
    s = (torch.randn(rows, n, generator=_gen(rows, n)) * 6).half()
    own = _row_owner((rows, n))
    return Case(f"softmax_rows-{rows}x{n}", "rows", {"s": s}, {"s": own, "out": own}, ("out",),
                lambda ops, lib: lambda o: {"out": ops.softmax_rows(o["s"], scale=0.37)})


def _geglu(rows, n):
    x = (torch.randn(rows, 2 * n, generator=_gen(rows, n, 2)) * 2).half()
    return Case(f"geglu-{rows}x{n}", "rows", {"x": x}, {"x": _row_owner(x.shape), "out": _row_owner((rows, n))}, ("out",),
                lambda ops, lib: lambda o: {"out": ops.geglu(o["x"])})


def _act(rows, n, kind):
    x = (torch.randn(rows, n, generator=_gen(rows, n, 3)) * 3).half()
    own = _row_owner((rows, n))
    return Case(f"act_-{kind}-{rows}x{n}", "rows", {"x": x}, {"x": own, "out": own}, ("out",),
                lambda ops, lib: lambda o: {"out": ops.act_(o["x"].clone(), kind)})


def _add_bias_residual(rows, C):
    g = _gen(rows, C, 4)
    a, b = torch.randn(rows, C, generator=g).half(), torch.randn(rows, C, generator=g).half()
    bias = (torch.randn(C, generator=g) * 0.2).half()
    own = _row_owner((rows, C))
    return Case(f"add_bias_residual-{rows}x{C}", "rows", {"a": a, "b": b, "bias": bias},
                {"a": own, "b": own, "bias": iso.shared(bias.shape), "out": own}, ("out",),
                lambda ops, lib: lambda o: {"out": ops.add_bias_residual(o["a"], o["b"], o["bias"])})


def norm_cases():
    return [_groupnorm_nchw(32, 8, 8), _groupnorm_nhwc(64, 15, 8, False), _groupnorm_nhwc(64, 15, 8, True), _groupnorm_cat(40, 24, 35, 8),
            _add_layernorm(7, 64, True), _add_layernorm(7, 64, False), _add_layernorm(9, 320, True)]


def row_cases():
    # 7 rows of 64: several rows share a wave; one case at the guard-band size
    return [_softmax_rows(7, 64), _softmax_rows(7, 1000), _geglu(7, 64), _geglu(7, 1000), _act(7, 64, "quick_gelu"), _act(7, 64, "gelu"),
            _act(7, 1000, "gelu"), _add_bias_residual(7, 64), _add_bias_residual(7, 320)]


# ============================================================================= attention
H_ATTN = 2


def _fused_views(q, k, v):
    """q / k / v [B, n, H, d] as strided views of one [B, max n, 3 H d] projection: behind image 0's last key lies image 1"""
    Bq, L, H, d = q.shape
    S = k.shape[1]
    buf = torch.zeros(Bq, max(L, S), 3 * H * d, dtype=q.dtype, device=q.device)
    buf[:, :L, :H * d] = q.reshape(Bq, L, H * d)
    buf[:, :S, H * d:2 * H * d] = k.reshape(Bq, S, H * d)
    buf[:, :S, 2 * H * d:] = v.reshape(Bq, S, H * d)
    return (buf[:, :L, :H * d].view(Bq, L, H, d), buf[:, :S, H * d:2 * H * d].view(Bq, S, H, d), buf[:, :S, 2 * H * d:].view(Bq, S, H, d))


def _self_attention(L, S, d, fused, sweep=""):
    g = _gen(L, S, d)
    q, k, v = (torch.randn(B, n, H_ATTN, d, generator=g).half() for n in (L, S, S))
    operands = {"q": q, "k": k, "v": v}
    owners = {"q": _rows(q.shape), "k": _rows(k.shape), "v": _rows(v.shape), "out": _rows(q.shape)}

    def make_run(ops, lib):
        def run(o):
            assert ops.attn_kernel_takes(o["q"].dtype, d)
            qq, kk, vv = _fused_views(o["q"], o["k"], o["v"]) if fused else (o["q"], o["k"], o["v"])
            return {"out": ops.self_attention(qq, kk, vv)}
        return run
    return Case(f"self_attention-L{L}-S{S}-d{d}-" + ("fused" if fused else "compact") + ("-variants" if sweep else ""), "self_attn",
                operands, owners, ("out",), make_run, sweep=sweep)


def _causal_attn(S, d, fused):
    g = _gen(S, d, 77)
    q, k, v = (torch.randn(B, S, H_ATTN, d, generator=g).half() for _ in range(3))
    operands = {"q": q, "k": k, "v": v}
    owners = {n: _rows(q.shape) for n in ("q", "k", "v", "out")}

    def make_run(ops, lib):
        def run(o):
            assert ops.causal_attn_takes(o["q"].dtype, S, d)
            qq, kk, vv = _fused_views(o["q"], o["k"], o["v"]) if fused else (o["q"], o["k"], o["v"])
            return {"out": ops.causal_attn(qq, kk, vv)}
        return run
    return Case(f"causal_attn-S{S}-d{d}-" + ("fused" if fused else "compact"), "text", operands, owners, ("out",), make_run)


def self_attn_cases():
    out = [_self_attention(L, S, d, fused) for d in (40, 64, 80, 160) for (L, S) in ((77, 77), (64, 77), (64, 64)) for fused in (False, True)]
    out += [_self_attention(77, 77, 40, fused, sweep="sa_variants") for fused in (False, True)]
    return out


def _region_inputs(L, S, d):
    x = attn_inputs(f"isolation/{L}/{S}/{d}", Bc=B, H=H_ATTN, L=L, S=S, d=d, Bw=B)
    q, k, v, w = (torch.from_numpy(x[n]) for n in ("q", "k", "v", "w"))
    return q.half(), k.half(), v.half(), w.float()                      # [B, H, L, d], [B, H, S, d], [Bw, L, S]


SIGMAS = (2.0, 0.75, 3.5)              # one per std group = per request


def _region_xattn(L, S, d, layout, ref16):
    q, k, v, w = _region_inputs(L, S, d)
    if layout == "blhd":
        q, k, v = (t.transpose(1, 2).contiguous() for t in (q, k, v))
    sig = torch.tensor(SIGMAS)
    operands = {"q": q, "k": k, "v": v, "w": w, "sigma": sig}
    owners = {"q": _rows(q.shape), "k": _rows(k.shape), "v": _rows(v.shape), "w": iso.shared(w.shape), "sigma": iso.shared(sig.shape),
              "out": _rows(q.shape)}

    def make_run(ops, lib):
        def run(o):
            assert ops.attn_kernel_takes(o["q"].dtype, d) and S <= ops.XATTN_MAX_KEYS
            return {"out": ops.region_xattn(o["q"], o["k"], o["v"], o["w"], o["sigma"], layout=layout, n_std_groups=B,
                                            ref_fp16_rounding=ref16, per_group_sigma=True)}
        return run
    return Case(f"region_xattn-{layout}-L{L}-S{S}-d{d}-" + ("ref16" if ref16 else "fp32"), "region", operands, owners, ("out",), make_run,
                seam_axes={n: 2 if layout == "bhld" else 1 for n in ("q", "k", "v")})


def _region_std(L, S, d, masked):
    q, k, _, _ = _region_inputs(L, S, d)
    operands = {"q": q, "k": k}
    owners = {"q": _rows(q.shape), "k": _rows(k.shape), "std": torch.arange(B)}
    if masked:
        operands["mask"] = torch.randn(L, S, generator=_gen(L, S, 5)) * 0.5
        owners["mask"] = iso.shared((L, S))

    def make_run(ops, lib):
        return lambda o: {"std": ops.region_xattn_std(o["q"], o["k"], n_std_groups=B, mask=o.get("mask"))}
    return Case(f"region_xattn_std-L{L}-S{S}-d{d}" + ("-masked" if masked else ""), "region", operands, owners, ("std",), make_run,
                seam_axes={"q": 2, "k": 2})


def _region_packed(L, S, d):
    ref16 = S <= 96                    # the chunked kernels keep fp32 scores: DSC_FLAG_REF_FP16_ROUNDING is refused there
    q, k, v, w = _region_inputs(L, S, d)
    q, k, v = (t.transpose(1, 2).contiguous() for t in (q, k, v))         # [B, n, H, d]
    sig = torch.tensor(SIGMAS)
    operands = {"q": q, "k": k, "v": v, "w": w, "sigma": sig}
    owners = {"q": _rows(q.shape), "k": _rows(k.shape), "v": _rows(v.shape), "w": iso.shared(w.shape), "sigma": iso.shared(sig.shape),
              "out": _rows(q.shape)}

    def make_run(ops, lib):
        def run(o):
            assert ops.xattn_kv_packable(S, d)
            comp = ops.compress_region_table_for_kernel(o["w"].cpu())
            assert comp is not None, "region table does not compress"
            packed = ops.xattn_kv_pack(o["k"], o["v"])
            return {"out": ops.region_xattn_packed(o["q"], packed, S, (comp[0].to(o["q"].device), comp[1].to(o["q"].device)), o["sigma"],
                                                   n_std_groups=B, ref_fp16_rounding=ref16, per_group_sigma=True)}
        return run
    return Case(f"xattn_kv_pack+region_xattn_packed-L{L}-S{S}-d{d}", "region", operands, owners, ("out",), make_run)


def region_cases():
    out = []
    for d in (40, 64):
        for L in (64, 100):
            out += [_region_xattn(L, 77, d, layout, ref16) for layout in ("bhld", "blhd") for ref16 in (True, False)]
            out += [_region_std(L, 77, d, masked) for masked in (False, True)]
            out += [_region_packed(L, 77, d)]
            # 96 < S: the chunked long-prompt kernels (online softmax over 96-key chunks); dsc_region_xattn_fwd itself stops at 96 keys
            out += [_region_packed(L, 154, d)]
    return out


def _ip_xattn(T, masked, io_frozen):
    """the IP-Adapter term.  Image 2's row_scale is 0: the row returns before it reads K / V and io keeps its bits.  io_frozen: the
    victim's io stays benign, so that what the kernel adds is visible - its queries with weight 0 keep their bits (the contract of
    the masked entry), every other one turns NaN with the victim's q / K / V."""
    L, d = 70, 40
    g = _gen(T, L, d, 9)
    q = torch.randn(B, L, H_ATTN, d, generator=g).half()
    k_ip, v_ip = (torch.randn(B, T, H_ATTN, d, generator=g).half() for _ in range(2))
    io = torch.randn(B, L, H_ATTN * d, generator=g).half()
    rs = torch.tensor([0.6, 1.0, 0.0])
    operands = {"q": q, "k_ip": k_ip, "v_ip": v_ip, "io": io, "row_scale": rs}
    owners = {"q": _rows(q.shape), "k_ip": _rows(k_ip.shape), "v_ip": _rows(v_ip.shape), "io": _rows(io.shape), "row_scale": torch.arange(B),
              "out": _rows(io.shape)}
    frozen = ("row_scale",) + (("io",) if io_frozen else ())
    rules = {}
    if masked:
        wgt = (torch.rand(B, L, generator=g) > 0.4).half() * torch.rand(B, L, generator=g).half()
        wgt[:, 16:32] = 0                                                  # a whole 16-query tile of zeros: not read
        operands["q_weight"], owners["q_weight"] = wgt, _rows(wgt.shape)
        frozen += ("q_weight",)
    if io_frozen:
        def rule(benign, got, mine, wgt=operands.get("q_weight")):
            live = torch.ones(B, L, dtype=torch.bool) if wgt is None else wgt != 0
            live = live.to(got.device)[:, :, None].expand_as(got) & mine
            dead = mine & ~live
            assert bool(torch.isnan(got[live]).all()), "ip_xattn_add: a weighted query of the victim is not NaN"
            assert torch.equal(iso.bits(got)[dead], iso.bits(benign)[dead]), "ip_xattn_add: a query of weight 0 was written"
        rules["out"] = rule

    def make_run(ops, lib):
        def run(o):
            assert ops.attn_kernel_takes(o["q"].dtype, d) and T <= ops.IP_MAX_TOKENS
            before = o["io"].clone()
            out = ops.ip_xattn_add(o["q"], o["k_ip"], o["v_ip"], o["row_scale"], o["io"].clone(), q_weight=o.get("q_weight"))
            assert torch.equal(iso.bits(out[2]), iso.bits(before[2])), "ip_xattn_add: a row of scale 0 changed"
            return {"out": out}
        return run
    return Case(f"ip_xattn_add-T{T}" + ("-masked" if masked else "") + ("-io-benign" if io_frozen else ""), "ip", operands, owners, ("out",),
                make_run, frozen=frozen, victim_rules=rules)


def ip_text_cases():
    out = [_ip_xattn(T, masked, frozen) for T in (4, 16) for masked in (False, True) for frozen in (False, True)]
    return out + [_causal_attn(77, 64, False), _causal_attn(77, 64, True)]


# ============================================================================= sampler steps (sampler.hip)
N_SLOTS, TW = 4, 96
_ROW_MODE = {"S": 0, "J": 1, "I": 2}                                   # ROW_STEP / ROW_JOIN / ROW_IDLE


def _slot_params(i):
    """tests/test_serving_gpu.py's distinct scalars per slot"""
    return {"sigma": 14.6 / (i + 1), "guidance": 7.5 - i, "a": 0.8 - 0.05 * i, "b": 0.2 + 0.03 * i, "c": 0.0 if i == 0 else -0.01 * i,
            "c_in_next": 0.07 * (i + 1), "t_next": 900.0 - 50 * i, "sigma_next": 12.0 / (i + 1)}


def _pair_owner(n, shape):
    """rows {i, n + i} of a [2 n, ...] buffer belong to slot i"""
    own = torch.arange(2 * n) % n
    return own.view(2 * n, *([1] * (len(shape) - 1))).expand(tuple(shape)).contiguous()


def _step_rows(entry, modes, n_dst, chw, stage=None):
    """one per-row sampler step over four slots, the victim in slot 1 (a STEP slot in every mix).  Hostile: the victim's x, old,
    mid, eps rows {1, n_src + 1}, its time-embedding row, noise row, known-region image / noise rows and extra row.  The records
    (scalars, modes, stages), the known-region mask and the slot pointers stay as they are.  t_buf and sigma_groups are made of
    the records alone: they keep their bits whatever the victim holds."""
    n_src = N_SLOTS
    g = _gen(n_dst, chw, len(entry), sum(map(ord, modes)))
    h = lambda *shape: torch.randn(*shape, generator=g).half()            # noqa: E731
    operands = {"x": h(N_SLOTS, chw), "old": h(N_SLOTS, chw), "eps": h(2 * n_src, chw), "temb": h(N_SLOTS, TW)}
    owners = {"x": _rows((N_SLOTS, chw), n=N_SLOTS), "old": _rows((N_SLOTS, chw), n=N_SLOTS), "eps": _pair_owner(n_src, (2 * n_src, chw)),
              "temb": _rows((N_SLOTS, TW), n=N_SLOTS)}
    frozen = ()
    linear = entry in ("linear", "rescale", "cat", "staged")
    if linear:
        operands["noise"], owners["noise"] = h(N_SLOTS, chw), _rows((N_SLOTS, chw), n=N_SLOTS)
    if entry == "known":
        for name in ("k_image", "k_noise"):
            operands[name], owners[name] = h(N_SLOTS, chw), _rows((N_SLOTS, chw), n=N_SLOTS)
        operands["k_mask"], owners["k_mask"] = (torch.rand(N_SLOTS, chw, generator=g) > 0.5).half(), _rows((N_SLOTS, chw), n=N_SLOTS)
        frozen = ("k_mask",)
    eh = 8 * 5
    if entry == "cat":
        operands["extra"], owners["extra"] = h(N_SLOTS, eh), _rows((N_SLOTS, eh), n=N_SLOTS)
    if entry == "staged":
        operands["mid"], owners["mid"] = h(N_SLOTS, chw), _rows((N_SLOTS, chw), n=N_SLOTS)
    row = chw + (eh if entry == "cat" else 0)
    owners.update({"x_out": owners["x"], "old_out": owners["old"], "x_in": _pair_owner(n_dst, (2 * n_dst, row)),
                   "t_buf": _pair_owner(n_dst, (2 * n_dst,)), "sigma_groups": torch.arange(n_dst), "tadd": _pair_owner(n_dst, (2 * n_dst, TW))})
    outputs = ("x_out", "old_out", "x_in", "t_buf", "sigma_groups", "tadd")
    if entry == "staged":
        owners["mid_out"], outputs = owners["mid"], outputs + ("mid_out",)

    def make_run(ops, lib):
        def run(o):
            dev = o["x"].device
            x, old = o["x"].clone(), o["old"].clone()
            mid = o["mid"].clone() if entry == "staged" else None
            recs = []
            for i, m in enumerate(modes):
                r = dict(_slot_params(i), mode=_ROW_MODE[m], temb_row=None if m == "I" else o["temb"][i])
                if linear:
                    r.update(s=0.3 + 0.1 * i, noise=o["noise"][i].clone())          # (a row of its own: 16-byte aligned at any chw)
                if entry == "rescale" and m == "S":
                    r["rescale"] = 0.7
                if entry == "staged" and m == "S":
                    r.update(stage=stage if i == 1 else ops.ROW_STAGE_FULL, m=0.5)
                recs.append(r)
            x_in = torch.full((2 * n_dst, row), 7.0, dtype=torch.float16, device=dev)
            t, sg = torch.full((2 * n_dst,), -1.0, device=dev), torch.full((n_dst,), -1.0, device=dev)
            tadd = torch.zeros(2 * n_dst, TW, dtype=torch.float16, device=dev)
            if entry == "rows":
                ops.cfg_dpmpp2m_step_rows(x, o["eps"], old, n_src, x_in, t, sg, recs, tadd=tadd)
            elif entry == "known":
                known = [None if m == "I" or i == 3 else {"image": o["k_image"][i].clone(), "noise": o["k_noise"][i].clone(), "mask": o["k_mask"][i].clone(),
                                                            "blend_now": i % 2 == 1, "blend_next": True} for i, m in enumerate(modes)]
                ops.cfg_dpmpp2m_step_rows_known(x, o["eps"], old, n_src, x_in, t, sg, recs, known, tadd=tadd)
            elif entry == "linear":
                ops.cfg_linear_step_rows(x, o["eps"], old, n_src, x_in, t, sg, recs, tadd=tadd)
            elif entry == "rescale":
                ops.cfg_linear_step_rows_rescale(x, o["eps"], old, n_src, x_in, t, sg, recs, tadd=tadd)
            elif entry == "cat":
                ops.cfg_linear_step_rows_cat(x, o["eps"], old, n_src, x_in, t, sg, recs, [o["extra"][i].clone() for i in range(N_SLOTS)], tadd=tadd)
            else:
                ops.cfg_staged_step_rows(x, mid, o["eps"], old, n_src, x_in, t, sg, recs, tadd=tadd)
            out = {"x_out": x, "old_out": old, "x_in": x_in, "t_buf": t, "sigma_groups": sg, "tadd": tadd}
            if entry == "staged":
                out["mid_out"] = mid
            return out
        return run
    name = {"rows": "cfg_dpmpp2m_step_rows", "known": "cfg_dpmpp2m_step_rows_known", "linear": "cfg_linear_step_rows",
            "rescale": "cfg_linear_step_rows_rescale", "cat": "cfg_linear_step_rows_cat", "staged": "cfg_staged_step_rows"}[entry]
    id = f"{name}-{modes}-dst{n_dst}-chw{chw}" + ({None: "", 1: "-predict", 2: "-correct"}[stage])
    return Case(id, "sampler", operands, owners, outputs, make_run, B=N_SLOTS, frozen=frozen,
                victim_rules={"t_buf": None, "sigma_groups": None})


def _scalar_step(entry, chw):
    """dsc_prepare_unet_input / dsc_cfg_dpmpp2m_step over four images with the row broadcast (a shared row, benign)"""
    n = N_SLOTS
    g = _gen(chw, len(entry), 31)
    h = lambda *shape: torch.randn(*shape, generator=g).half()            # noqa: E731
    operands = {"x": h(n, chw), "row": h(TW)}
    owners = {"x": _rows((n, chw), n=n), "row": iso.shared((TW,)), "x_in": _pair_owner(n, (2 * n, chw)), "t_buf": _pair_owner(n, (2 * n,)),
              "sigma_buf": iso.shared((1,)), "tadd": iso.shared((2 * n, TW))}
    outputs = ("x_in", "t_buf", "sigma_buf", "tadd")
    if entry == "step":
        operands.update(old=h(n, chw), eps=h(2 * n, chw))
        owners.update(old=_rows((n, chw), n=n), eps=_pair_owner(n, (2 * n, chw)), x_out=owners["x"], old_out=owners["x"])
        outputs += ("x_out", "old_out")

    def make_run(ops, lib):
        def run(o):
            dev = o["x"].device
            x = o["x"].clone()
            x_in = torch.full((2 * n, chw), 7.0, dtype=torch.float16, device=dev)
            t, sg = torch.full((2 * n,), -1.0, device=dev), torch.full((1,), -1.0, device=dev)
            tadd = torch.zeros(2 * n, TW, dtype=torch.float16, device=dev)
            p = _slot_params(1)
            if entry == "prepare":
                ops.prepare_unet_input(x, p["c_in_next"], p["t_next"], p["sigma_next"], x_in, t, sg, row=(o["row"], tadd))
                return {"x_in": x_in, "t_buf": t, "sigma_buf": sg, "tadd": tadd}
            old = o["old"].clone()
            ops.cfg_dpmpp2m_step(x, o["eps"], old, p["sigma"], p["guidance"], p["a"], p["b"], p["c"], p["c_in_next"], p["t_next"],
                                 p["sigma_next"], x_in, t, sg, row=(o["row"], tadd))
            return {"x_in": x_in, "t_buf": t, "sigma_buf": sg, "tadd": tadd, "x_out": x, "old_out": old}
        return run
    name = "prepare_unet_input" if entry == "prepare" else "cfg_dpmpp2m_step"
    return Case(f"{name}-row-broadcast-chw{chw}", "sampler", operands, owners, outputs, make_run, B=n, victim_rules={"t_buf": None})


def sampler_cases():
    out = []
    for entry in ("rows", "known", "linear", "rescale", "cat", "staged"):
        stages = (1, 2) if entry == "staged" else (None,)                 # ROW_STAGE_PREDICT / ROW_STAGE_CORRECT in the victim's slot
        for stage in stages:
            # a JOIN record joins the bucket that runs next: slot 2 of SSJI lies behind a 2-row bucket and the entries refuse it
            # (DSC_ERR_BAD_ARG before any launch), so the 2-row mix joins in slot 0
            for modes, n_dst in (("SSJI", 4), ("SSSS", 4), ("JSSI", 2), ("SSSS", 2)):
                out.append(_step_rows(entry, modes, n_dst, 256, stage))
            if entry in ("rows", "known"):                                # 36 halfs: the 8-byte path; the linear entries take chw % 8 only
                out.append(_step_rows(entry, "SSJI", 4, 36, stage))
    return out + [_scalar_step(e, chw) for e in ("prepare", "step") for chw in (256, 36)]


# ============================================================================= lanes
def _cl_rows(t):
    return t.contiguous(memory_format=CL)


def _equals_benign(what):
    def rule(benign, got, mine):
        assert torch.equal(iso.bits(got)[mine], iso.bits(benign)[mine]), what
    return rule


def _zeros(what):
    def rule(benign, got, mine):
        assert bool((got[mine] == 0).all()), what
    return rule


def _freeu(stage):
    g = _gen(stage, 41)
    hidden, skip = torch.randn(B, 32, 8, 8, generator=g).half(), torch.randn(B, 16, 8, 8, generator=g).half()
    params = torch.tensor([[0.9, 0.2, 1.2, 1.4], [0.6, 0.5, 1.1, 1.3], [0.8, 0.3, 1.5, 1.2]])
    operands = {"hidden": hidden, "skip": skip, "params": params}
    owners = {"hidden": _rows(hidden.shape), "skip": _rows(skip.shape), "params": _rows(params.shape),
              "hidden_out": _rows(hidden.shape), "skip_out": _rows(skip.shape)}

    def make_run(ops, lib):
        def run(o):
            hd, sk = _cl_rows(o["hidden"]).clone(memory_format=torch.preserve_format), _cl_rows(o["skip"]).clone(memory_format=torch.preserve_format)
            assert ops.freeu_covers(hd, sk), "freeu_rows_: not covered"
            ops.freeu_rows_(hd, sk, o["params"], stage)
            return {"hidden_out": hd, "skip_out": sk}
        return run
    return Case(f"freeu_rows_-stage{stage}", "lanes", operands, owners, ("hidden_out", "skip_out"), make_run, frozen=("params",),
                seam_axes={"hidden": 2, "skip": 2})


def _add_rows_gated(in_place, closed):
    """closed: the victim's gate is 0 and its x stays benign - the hostile features behind the closed gate are not read and the
    victim's row keeps x's bits"""
    g = _gen(int(in_place), int(closed), 43)
    x, feat = torch.randn(B, 64, 2, 2, generator=g).half(), torch.randn(B, 64, 2, 2, generator=g).half()
    gate = torch.tensor([1.0, 0.0 if closed else 0.7, 0.5])
    operands = {"x": x, "feat": feat, "gate": gate}
    owners = {"x": _rows(x.shape), "feat": _rows(feat.shape), "gate": torch.arange(B), "out": _rows(x.shape)}

    def make_run(ops, lib):
        def run(o):
            src, ft = _cl_rows(o["x"]).clone(memory_format=torch.preserve_format), _cl_rows(o["feat"])
            assert ops.add_rows_gated_supported(src, ft), "add_rows_gated: not covered"
            out = ops.add_rows_gated(src, ft, o["gate"], out=src if in_place else None)
            if closed:
                assert torch.equal(iso.bits(out[1]), iso.bits(_cl_rows(o["x"])[1])), "add_rows_gated: a row with gate 0 changed"
            return {"out": out}
        return run
    return Case("add_rows_gated" + ("-in-place" if in_place else "") + ("-closed-gate" if closed else ""), "lanes", operands, owners, ("out",),
                make_run, frozen=("gate",) + (("x",) if closed else ()), seam_axes={"x": 2, "feat": 2},
                victim_rules={"out": _equals_benign("a closed gate let the features through")} if closed else {})


def _scatter_add_rows():
    """five lane rows of two nets: lane 0 -> image 0, lane 1 -> the victim, lane 2 idle (dst < 0), lane 3 -> image 2 with every gate
    0, lane 4 -> image 2.  Lanes 1, 2 and 3 hold the victim's features: an idle lane and a lane whose gates are all 0 return before
    they load, so image 2 receives lane 4 alone"""
    g = _gen(47)
    x, feat = torch.randn(B, 64, 2, 2, generator=g).half(), torch.randn(2, 5, 64, 2, 2, generator=g).half()
    gate = torch.tensor([[1.0, 0.7, 0.9, 0.0, 0.6], [0.5, 0.0, 0.4, 0.0, 0.3]])
    dst = torch.tensor([0, 1, -1, 2, 2], dtype=torch.int32)
    lane_owner = torch.tensor([0, 1, 1, 1, 2]).view(1, 5, 1, 1, 1).expand(feat.shape).contiguous()
    operands = {"x": x, "feat": feat, "gate": gate, "dst": dst}
    owners = {"x": _rows(x.shape), "feat": lane_owner, "gate": iso.shared(gate.shape), "dst": iso.shared(dst.shape), "out": _rows(x.shape)}

    def make_run(ops, lib):
        def run(o):
            xd = _cl_rows(o["x"]).clone(memory_format=torch.preserve_format)
            ft = torch.stack([_cl_rows(f) for f in o["feat"]])                  # [A, R] channels-last rows, the nets dense behind one another
            assert ops.scatter_add_rows_supported(xd, ft), "scatter_add_rows: not covered"
            return {"out": ops.scatter_add_rows(xd, ft, o["gate"], o["dst"])}
        return run
    return Case("scatter_add_rows", "lanes", operands, owners, ("out",), make_run, seam_axes={"x": 2, "feat": 3})


def _latent_resample_noise(mode):
    g = _gen(len(mode), 53)
    src, noise = torch.randn(B, 4, 8, 8, generator=g).half(), torch.randn(B, 4, 12, 12, generator=g).half()
    operands = {"src": src, "noise": noise}
    owners = {"src": _rows(src.shape), "noise": _rows(noise.shape), "out": _rows(noise.shape)}
    return Case(f"latent_resample_noise-{mode}", "lanes", operands, owners, ("out",),
                lambda ops, lib: lambda o: {"out": ops.latent_resample_noise(o["src"], (12, 12), mode, noise=o["noise"], sigma0=7.0)},
                seam_axes={"src": 2, "noise": 2})


def _latent_preview(up):
    lat = torch.randn(B, 4, 8, 8, generator=_gen(up, 59)).half()
    operands = {"lat": lat}
    owners = {"lat": _rows(lat.shape), "out": _rows((B, 8 * up, 8 * up, 3))}
    return Case(f"latent_preview-up{up}", "lanes", operands, owners, ("out",),
                lambda ops, lib: lambda o: {"out": ops.latent_preview(o["lat"], [0, 1, 2], up=up)},
                seam_axes={"lat": 2}, victim_rules={"out": _zeros("latent_preview: NaN -> 0")})


def _image_finish():
    img = (torch.randn(B, 3, 8, 16, generator=_gen(61)) * 0.7).half()
    operands = {"img": img}
    owners = {"img": _rows(img.shape), "out": _rows((B, 8, 16, 3))}
    return Case("image_finish-uint8", "lanes", operands, owners, ("out",),
                lambda ops, lib: lambda o: {"out": ops.image_finish(o["img"], "uint8")},
                seam_axes={"img": 2}, victim_rules={"out": _zeros("image_finish: NaN -> 0")})


def _prompt_weight_rows():
    T, C = 77, 64
    g = _gen(67)
    z = torch.randn(2 * B, T, C, generator=g).half()
    mult = 1.0 + 0.3 * torch.randn(B, 2, T, generator=g)
    operands = {"z": z, "mult": mult}
    owners = {"z": _pair_owner(B, z.shape), "mult": iso.shared(mult.shape), "neg": _rows((B, T, C)), "pos": _rows((B, T, C))}

    def make_run(ops, lib):
        def run(o):
            neg = torch.zeros(B, T, C, dtype=torch.float16, device=o["z"].device)
            pos = torch.zeros_like(neg)
            ops.prompt_weight_rows(o["z"], [{"rows": (i, B + i), "mult": o["mult"][i].contiguous(), "out": (neg[i], pos[i])} for i in range(B)])
            return {"neg": neg, "pos": pos}
        return run
    return Case("prompt_weight_rows", "lanes", operands, owners, ("neg", "pos"), make_run)


def _latent_start():
    g = _gen(71)
    moments, eps, noise = torch.randn(B, 8, 8, 8, generator=g).half(), torch.randn(B, 4, 8, 8, generator=g).half(), torch.randn(B, 4, 8, 8, generator=g).half()
    operands = {"moments": moments, "eps": eps, "noise": noise}
    owners = {"moments": _rows(moments.shape), "eps": _rows(eps.shape), "noise": _rows(noise.shape), "start": _rows(eps.shape), "keep": _rows(eps.shape)}

    def make_run(ops, lib):
        def run(o):
            start, keep = torch.zeros_like(o["eps"]), torch.zeros_like(o["eps"])
            ops.latent_start(o["moments"], [{"form": ("add", "add", "scale")[i], "row": i, "eps": o["eps"][i].clone(), "noise": o["noise"][i].clone(),
                                             "scaling": 0.18215, "coef": 7.0 + i, "start": start[i], "keep": keep[i]} for i in range(B)])
            return {"start": start, "keep": keep}
        return run
    return Case("latent_start", "lanes", operands, owners, ("start", "keep"), make_run, seam_axes={n: 2 for n in operands})


def _image_prepare():
    """float pixels and a float mask per row.  The mask output is a compare (`mask < 0.5` at every eighth pixel): a NaN mask gives
    0 or 1, never NaN - the entry's contract; the image outputs propagate"""
    g = _gen(73)
    H = W = 16
    image, mask = torch.rand(B, 3, H, W, generator=g) * 2 - 1, torch.rand(B, H, W, generator=g)
    operands = {"image": image, "mask": mask}
    owners = {"image": _rows(image.shape), "mask": _rows(mask.shape), "out_image": _rows(image.shape), "out_masked": _rows(image.shape),
              "out_mask": _rows((B, 1, H // 8, W // 8))}

    def binary(benign, got, mine):
        assert bool(((got[mine] == 0) | (got[mine] == 1)).all()), "image_prepare: the mask compare gave something else than 0 or 1"

    def make_run(ops, lib):
        def run(o):
            dev = o["image"].device
            oi, om = torch.zeros(B, 3, H, W, dtype=torch.float16, device=dev), torch.zeros(B, 3, H, W, dtype=torch.float16, device=dev)
            ok = torch.zeros(B, 1, H // 8, W // 8, dtype=torch.float16, device=dev)
            ops.image_prepare([{"image": o["image"][i].clone(), "mask": o["mask"][i].clone(), "out_image": oi[i], "out_masked": om[i],
                                "out_mask": ok[i]} for i in range(B)], H, W)
            return {"out_image": oi, "out_masked": om, "out_mask": ok}
        return run
    return Case("image_prepare", "lanes", operands, owners, ("out_image", "out_masked", "out_mask"), make_run,
                seam_axes={"image": 2, "mask": 1}, victim_rules={"out_mask": binary})


def lane_cases():
    return ([_freeu(0), _freeu(1)] + [_add_rows_gated(ip, closed) for ip in (False, True) for closed in (False, True)]
            + [_scatter_add_rows(), _latent_resample_noise("bicubic"), _latent_resample_noise("bilinear"), _latent_preview(1), _latent_preview(2),
               _image_finish(), _prompt_weight_rows(), _latent_start(), _image_prepare()])


# ============================================================================= the table
FAMILIES = ("gemm", "gemm_lt", "gemm_gn", "conv", "norm", "rows", "self_attn", "region", "ip", "text", "sampler", "lanes")


def all_cases():
    return (gemm_cases() + conv_cases() + norm_cases() + row_cases() + self_attn_cases() + region_cases() + ip_text_cases() + sampler_cases() + lane_cases())
