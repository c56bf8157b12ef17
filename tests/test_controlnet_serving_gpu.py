"""ControlNet requests in the continuous batcher on the MI355X (`-m gpu`): dsc_scatter_add_rows_f16 (lane residuals scaled by
device-side gates and added into the batch rows a device-side vector names) against torch's fp16 ops, its skip / capture /
determinism properties and the wrapper's refusals; the ControlNet's `unscaled` keyword and the UNet's `down_block_scattered`
keyword against the eager hook; and the serving batcher with control images on compact lanes against the oracle loop, `txt2img` /
`img2img` and itself."""
import dataclasses
import math

import pytest
import torch

from inputs import FakeTokenizer
from oracle import unet_ref

pytestmark = pytest.mark.gpu
CL = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- the kernel
SHAPES = [(4, 2, 1, 8, 1, 1),           # one 16-byte piece per row
          (4, 2, 1, 64, 2, 2),          # 256 halfs per row: less than one wave of pieces
          (4, 2, 1, 32, 16, 16),
          (6, 4, 2, 320, 19, 19),       # odd, with a ragged last block; two nets
          (2, 2, 1, 1280, 8, 8),
          (16, 2, 1, 320, 64, 64)]      # one real level: the grid cap and the stride


def _stack(ts):
    """[A, R, C, h, w] from A tensors [R, C, h, w]: every net's rows channels-last, the nets dense behind one another"""
    return torch.stack([t.permute(0, 2, 3, 1) for t in ts]).contiguous().permute(0, 1, 4, 2, 3)


def _operands(X, R, A, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(X, C, h, w, generator=g).half().contiguous(memory_format=CL).cuda()
    feat = _stack([torch.randn(R, C, h, w, generator=g).half() for _ in range(A)]).cuda()
    return x, feat


def _permuted(X, R):
    """lane 0 to the last row, lane j to row j - 1"""
    return [X - 1] + list(range(R - 1))


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _f32(v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


def _times(t, g):
    """torch's fp16 `t * g` for a python float g - as torch multiplies every residual of a real model.  torch's elementwise
    multiply has two code paths: whole blocks of 2048 elements run an fp32 multiply whose fp32 result is then converted (the
    contract of dsc_scatter_add_rows_f16), and the block that is left over (a whole tensor, below 2048 elements) runs a bounds-
    checked path in which the compiler folded the conversion into the multiply (v_fma_mixlo_f16: the exact product rounded
    ONCE).  Every residual of SD1.5 is a whole number of such blocks (the smallest, two rows of 1280 x 8 x 8, is 80 of them).
    Measured on one MI355X with g = 0.9: the two roundings disagree by one ulp at 4.2 % of random elements (43669 of 2**20);
    `t * 0.9` follows the single rounding at 8, 256 and 1024 elements and the double rounding at 2048, 4096, 8192, 65536,
    163840 and 2**20, and a 115520-element row (56 blocks + 832) equals neither.  So the operand is multiplied inside a tensor
    of a whole number of 8192-element blocks: the same torch op, on the path it takes for real shapes.  (torch's fp16 add has
    one form: an fp16 sum is exactly rounded either way; measured: no difference in 5.2 M sums.)"""
    n = t.numel()
    pad = torch.zeros(-(-n // 8192) * 8192, dtype=t.dtype, device=t.device)
    pad[:n] = t.reshape(-1)
    return (pad * g)[:n].view(t.shape)


def _model(x, feat, gates, dst):
    """the contract in numpy on the host, independent of torch's kernels: fp32 operations, each rounded to fp32 and then to fp16"""
    import numpy as np
    out = x.cpu().numpy().copy()
    xn, fn = x.cpu().numpy(), feat.cpu().numpy()
    for j, d in enumerate(dst):
        nets = [a for a in range(fn.shape[0]) if gates[a][j] != 0.0]
        if d < 0 or d >= xn.shape[0] or not nets:
            continue
        t = None
        for a in nets:
            p = (fn[a, j].astype(np.float32) * np.float32(gates[a][j])).astype(np.float16)
            t = p if t is None else (t.astype(np.float32) + p.astype(np.float32)).astype(np.float16)
        out[d] = (xn[d].astype(np.float32) + t.astype(np.float32)).astype(np.float16)
    return torch.from_numpy(out)


@pytest.mark.parametrize("X, R, A, C, h, w", SHAPES)
def test_one_net_is_torchs_fp16_multiply_then_add(ops, X, R, A, C, h, w):
    """A = 1 (the first net of the shape): torch.equal to torch's x[d] + feat[j] * g for python floats g (the product as _times
    takes it), and to the numpy model of the contract; rows no lane names untouched"""
    x, feat = _operands(X, R, A, C, h, w, seed=X + C + h)
    feat = feat[:1]
    dst = _permuted(X, R)
    assert ops.scatter_add_rows_supported(x, feat)
    for g in (1.0, 0.9, 0.3, -0.5):
        got = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), feat, _f32([[g] * R]), _i32(dst))
        torch.cuda.synchronize()
        assert got.is_contiguous(memory_format=CL)
        for j, d in enumerate(dst):
            assert torch.equal(got[d], x[d] + _times(feat[0, j], g)), (g, j, d)
        for r in set(range(X)) - set(dst):
            assert torch.equal(got[r], x[r]), (g, r)
        assert torch.equal(got.cpu(), _model(x, feat, [[g] * R], dst)), g
    assert not torch.equal(got[dst[0]], x[dst[0]])


def _chain(x, feat, gates, dst):
    """the contract in torch's fp16 ops: t = f_a0 * g_a0; t = t + f_a * g_a over the further open nets; x[d] + t"""
    out = x.clone(memory_format=torch.preserve_format)
    for j, d in enumerate(dst):
        nets = [a for a in range(feat.shape[0]) if gates[a][j] != 0.0]
        if d < 0 or not nets:
            continue
        t = _times(feat[nets[0], j], gates[nets[0]][j])
        for a in nets[1:]:
            t = t + _times(feat[a, j], gates[a][j])
        out[d] = x[d] + t
    return out


@pytest.mark.parametrize("X, R, A, C, h, w", [SHAPES[3], (4, 2, 2, 64, 2, 2), (5, 3, 3, 32, 16, 16)])
def test_several_nets_are_the_chain_of_separately_rounded_torch_ops(ops, X, R, A, C, h, w):
    x, feat = _operands(X, R, A, C, h, w, seed=3 * X + A)
    dst = _permuted(X, R)
    gates = [[(0.9, 0.4, -0.7)[a] * (1.0, 0.5, 0.3, 1.7)[j % 4] for j in range(R)] for a in range(A)]
    got = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), feat, _f32(gates), _i32(dst))
    torch.cuda.synchronize()
    # the gates the kernel reads are fp32: the torch chain multiplies by the same fp32 values
    g32 = torch.tensor(gates, dtype=torch.float32).tolist()
    assert torch.equal(got, _chain(x, feat, g32, dst))
    assert torch.equal(got.cpu(), _model(x, feat, g32, dst))


def test_idle_lanes_and_closed_gates_read_nothing_and_write_nothing(ops):
    """dst = -1, and all gates 0, over NaN features: the would-be destination keeps its bits; a net whose gate is 0 is not read
    (NaN there) and the result is the one-net call on the other net"""
    X, R, A, C, h, w = 6, 4, 2, 320, 19, 19
    x, feat = _operands(X, R, A, C, h, w, seed=8)
    f = feat.clone()
    f[:, 1] = float("nan")               # lane 1 is idle
    f[:, 2] = float("nan")               # lane 2: every gate 0
    f[0, 3] = float("nan")               # lane 3: net 0 closed
    f[1, 0] = float("nan")               # lane 0: net 1 closed
    dst = [5, -1, 2, 0]
    gates = [[0.9, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.3]]
    got = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), f, _f32(gates), _i32(dst))
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    for r in (1, 2, 3, 4):
        assert torch.equal(got[r], x[r]), r
    one0 = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), feat[:1], _f32([[0.9, 0.0, 0.0, 0.0]]),
                                _i32(dst))
    one1 = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), feat[1:], _f32([[0.0, 0.0, 0.0, 0.3]]),
                                _i32(dst))
    torch.cuda.synchronize()
    assert torch.equal(got[5], one0[5]) and torch.equal(got[0], one1[0])
    assert not torch.equal(got[5], x[5]) and not torch.equal(got[0], x[0])
    # a destination past x is an idle lane too
    same = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), feat, _f32([[1.0] * 4] * 2), _i32([6, 70000, -5, -1]))
    torch.cuda.synchronize()
    assert torch.equal(same, x)


def test_under_graph_capture_the_replay_follows_gate_dst_and_feat(ops):
    """one captured call; gate, dst and feat are overwritten in place and x reset between the replays"""
    X, R, A, C, h, w = 4, 2, 2, 32, 16, 16
    x, feat = _operands(X, R, A, C, h, w, seed=9)
    _, feat2 = _operands(X, R, A, C, h, w, seed=10)
    gate, dst = _f32([[1.0, 0.0], [0.0, 0.0]]), _i32([0, -1])
    buf = x.clone(memory_format=torch.preserve_format)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.scatter_add_rows(buf, feat, gate, dst)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    buf.copy_(x)
    with torch.cuda.graph(g):
        ops.scatter_add_rows(buf, feat, gate, dst)
    for gates2, dst2, f2 in (([[0.5, 0.25], [0.0, -1.0]], [3, 1], feat2), ([[0.0, 0.0], [0.0, 0.0]], [3, 1], feat2),
                             ([[0.0, 2.0], [0.3, 0.0]], [-1, 2], feat)):
        gate.copy_(_f32(gates2))
        dst.copy_(_i32(dst2))
        feat.copy_(f2)
        buf.copy_(x)
        g.replay()
        fresh = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), f2, _f32(gates2), _i32(dst2))
        torch.cuda.synchronize()
        assert torch.equal(buf, fresh), (gates2, dst2)
        assert torch.equal(buf, _chain(x, f2, torch.tensor(gates2, dtype=torch.float32).tolist(), dst2))


def test_determinism_feature_views_and_token_major_rows(ops):
    X, R, A, C, h, w = 6, 4, 2, 320, 19, 19
    x, feat = _operands(X, R, A, C, h, w, seed=11)
    gate, dst = _f32([[1.0, 0.3, 0.0, -1.0], [0.5, 0.0, 0.0, 2.0]]), _i32([5, 0, 3, 2])
    a = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), feat, gate, dst)
    b = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), feat, gate, dst)
    n = C * h * w
    flat = torch.zeros(A * R * n + 64, dtype=torch.float16, device="cuda")
    view = flat[8:8 + A * R * n].view(A, R, h, w, C).permute(0, 1, 4, 2, 3)       # 16 bytes into the buffer
    view.copy_(feat)
    assert view.data_ptr() % 16 == 0 and view.data_ptr() != flat.data_ptr() and ops.scatter_add_rows_supported(x, view)
    c = ops.scatter_add_rows(x.clone(memory_format=torch.preserve_format), view, gate, dst)
    # the same bytes as token-major rows [X, L, C] / [A, R, L, C]
    xt = x.permute(0, 2, 3, 1).reshape(X, h * w, C).clone()
    ft = feat.permute(0, 1, 3, 4, 2).reshape(A, R, h * w, C).contiguous()
    d = ops.scatter_add_rows(xt, ft, gate, dst)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(d.view(X, h, w, C).permute(0, 3, 1, 2), a)


def test_wrapper_refusals_and_dropped_partial_sums(ops):
    from diffusionspatialcontrol_amd import DscLibraryError
    x, feat = _operands(4, 2, 2, 32, 4, 4, seed=12)
    gate, dst = torch.ones(2, 2, device="cuda"), _i32([0, 1])
    assert ops.scatter_add_rows_supported(x, feat)
    small = _operands(2, 1, 1, 4, 3, 3, seed=1)                                    # 36 halfs per row
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.scatter_add_rows(*small, torch.ones(1, 1, device="cuda"), _i32([0]))
    assert not ops.scatter_add_rows_supported(*small)
    with pytest.raises(ValueError, match="channels-last"):
        ops.scatter_add_rows(x, feat.contiguous(), gate, dst)                      # NCHW rows against channels-last x
    assert not ops.scatter_add_rows_supported(x, feat.contiguous())
    with pytest.raises(ValueError, match="channels-last"):
        ops.scatter_add_rows(x, _stack([feat[0], feat[0], feat[1]])[::2], gate, dst)   # the nets not dense behind one another
    with pytest.raises(ValueError, match="trailing shape"):
        ops.scatter_add_rows(x, feat[:, :, :16], gate, dst)
    with pytest.raises(ValueError, match="trailing shape"):
        ops.scatter_add_rows(x, feat[0], gate, dst)                                # no nets dimension
    with pytest.raises(ValueError, match="at most 8"):
        ops.scatter_add_rows(x, _stack([feat[0]] * 9), torch.ones(9, 2, device="cuda"), dst)
    with pytest.raises(TypeError, match="fp16"):
        ops.scatter_add_rows(x.float(), feat, gate, dst)
    with pytest.raises(ValueError, match="gate"):
        ops.scatter_add_rows(x, feat, torch.ones(2, device="cuda"), dst)
    with pytest.raises(ValueError, match="gate"):
        ops.scatter_add_rows(x, feat, gate.half(), dst)
    with pytest.raises(ValueError, match="dst"):
        ops.scatter_add_rows(x, feat, gate, dst.long())
    with pytest.raises(ValueError, match="dst"):
        ops.scatter_add_rows(x, feat, gate, _i32([0, 1, 2]))
    with pytest.raises(DscLibraryError):
        ops.scatter_add_rows(x, feat, gate.cpu(), dst)                             # gate and dst are read on the device
    with pytest.raises(DscLibraryError):
        ops.scatter_add_rows(x, feat, gate, dst.cpu())
    big = torch.zeros(2 * 2 + 4, 4, 4, 32, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="overlaps feat"):
        ops.scatter_add_rows(big[3:7].permute(0, 3, 1, 2), big[:4].view(2, 2, 4, 4, 32).permute(0, 1, 4, 2, 3), gate, dst)
    # x 8 bytes into a buffer: dense rows, but no 16-byte pieces
    flat = torch.zeros(4 * 512 + 16, dtype=torch.float16, device="cuda")
    odd = flat[4:4 + 4 * 512].view(4, 4, 4, 32).permute(0, 3, 1, 2)
    assert odd.data_ptr() % 16 == 8 and not ops.scatter_add_rows_supported(odd, feat)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.scatter_add_rows(odd, feat, gate, dst)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.scatter_add_rows(x, flat[4:4 + 4 * 512].view(2, 2, 4, 4, 32).permute(0, 1, 4, 2, 3), gate, dst)
    # more lane rows than gridDim.y takes
    many = torch.zeros(1, 65536, 8, 1, 1, dtype=torch.float16, device="cuda")
    x8 = torch.zeros(2, 8, 1, 1, dtype=torch.float16, device="cuda")
    assert not ops.scatter_add_rows_supported(x8, many)
    with pytest.raises(ValueError, match="at most 65535"):
        ops.scatter_add_rows(x8, many, torch.zeros(1, 65536, device="cuda"), torch.zeros(65536, dtype=torch.int32, device="cuda"))
    # x over the gates, x over dst: the gate matrix / the dst vector carved out of the memory x lies in
    words = torch.zeros(4 * 256 + 64, dtype=torch.float32, device="cuda")
    xw = words.view(torch.float16)[:4 * 512].view(4, 4, 4, 32).permute(0, 3, 1, 2)
    with pytest.raises(ValueError, match="overlaps gate"):
        ops.scatter_add_rows(xw, feat, words[8:12].view(2, 2), dst)
    ints = torch.zeros(4 * 256 + 64, dtype=torch.int32, device="cuda")
    xi = ints.view(torch.float16)[:4 * 512].view(4, 4, 4, 32).permute(0, 3, 1, 2)
    with pytest.raises(ValueError, match="overlaps dst"):
        ops.scatter_add_rows(xi, feat, gate, ints[1022:1024])
    dst_t = x.clone(memory_format=torch.preserve_format)
    ops.attach_gn_partials(dst_t, ops.GnPartials(torch.zeros(4, 1, 8, 2, 2, device="cuda"), 1, 8, 32, 4, 16))
    assert ops.gn_partials_of(dst_t) is not None
    ops.scatter_add_rows(dst_t, feat, gate, dst)
    assert ops.gn_partials_of(dst_t) is None
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the ControlNet and UNet keywords
def _unet(cfg=None, seed=0):
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(seed)
    return UNet2DConditionModel(cfg or UNetConfig.tiny()).half().cuda().eval()


def _controlnet(cfg, seed=5):
    import test_unet_pipeline_gpu as up
    cn, sd = up._controlnet(cfg, seed=seed)
    return cn.cuda().eval(), sd


@pytest.mark.parametrize("first_attn", [True, False])
def test_unscaled_residuals_scattered_equal_the_eager_hook(ops, first_attn):
    """The ControlNet's `unscaled` outputs times the scale in torch are the default forward's outputs bit for bit (the keyword
    leaves out exactly those launches).  Scattered with an identity dst and every gate at the scale, the UNet's output is
    torch.equal to the eager keywords `down_block_additional_residuals` / `mid_block_additional_residual` handed the residuals
    times the scale as torch multiplies real-size tensors (_times), both WITHOUT `cfg_shared_prefix` (the eager keywords switch
    the shared prefix off; the scatter keyword alone does not): the kernel's chain is that `d * scale` then torch's `s + r`, at
    the same places, and both routes hand the readers tensors without producer statistics.  Against the eager route as
    ControlNetModel.forward scales them the bound is 2e-3 of the range and NOT equality at this toy width: six of its thirteen
    residuals have fewer than 2048 elements, where torch's multiply rounds once (see _times).  The same bound holds with the
    shared prefix on the scatter side, where the first block's launches differ.  All gates 0 over NaN residuals, and every
    lane idle: the bits of the call without the keyword.  One lane on row 1 only: each row equals its own case."""
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNetConfig
    cfg = UNetConfig.tiny() if first_attn else dataclasses.replace(UNetConfig.tiny(), transformer_layers_per_block=(0, 1, 1, 0))
    unet = _unet(cfg)
    cn, _ = _controlnet(cfg)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, 16, 16, generator=g).half().cuda().repeat(2, 1, 1, 1)
    text = torch.randn(2, 77, 64, generator=g).half().cuda()
    cond = torch.rand(1, 3, 128, 128, generator=g).half().cuda().repeat(2, 1, 1, 1)
    t = torch.tensor([300.0, 300.0], device="cuda")
    s = 0.9
    with torch.no_grad():
        down, mid = cn(x, t, text, cond, conditioning_scale=s, return_dict=False)
        raw_down, raw_mid = cn(x, t, text, cond, unscaled=True, return_dict=False)
        for a, b in zip(down + [mid], raw_down + [raw_mid]):
            assert torch.equal(b * s, a) and not torch.equal(b, a)
        feats, fmid = [_stack([d]) for d in raw_down], _stack([raw_mid])
        nan = [f * float("nan") for f in feats]
        swapped, smid = [_stack([d.flip(0)]) for d in raw_down], _stack([raw_mid.flip(0)])
        plain = unet(x, t, text).sample
        stock = unet(x, t, text, down_block_additional_residuals=[d.clone() for d in down],
                     mid_block_additional_residual=mid.clone()).sample
        eager = unet(x, t, text, down_block_additional_residuals=[_times(d, s) for d in raw_down],
                     mid_block_additional_residual=_times(raw_mid, s)).sample
        full = (_f32([[s, s]]), _i32([0, 1]))
        got = unet(x, t, text, down_block_scattered=(feats, fmid) + full).sample
        shared = unet(x, t, text, down_block_scattered=(feats, fmid) + full, cfg_shared_prefix=True).sample
        zero = unet(x, t, text, down_block_scattered=(nan, fmid * float("nan"), _f32([[0.0, 0.0]]), _i32([0, 1]))).sample
        idle = unet(x, t, text, down_block_scattered=(nan, fmid * float("nan"), _f32([[s, s]]), _i32([-1, -1]))).sample
        mixed = unet(x, t, text, down_block_scattered=(swapped, smid, _f32([[s, s]]), _i32([1, -1]))).sample
        with pytest.raises(ValueError, match="mutually exclusive"):
            unet(x, t, text, down_block_scattered=(feats, fmid) + full, mid_block_additional_residual=mid)
        with pytest.raises(ValueError, match="do not fit"):
            unet(x, t, text, down_block_scattered=([feats[0][:, :, :16].contiguous()] + feats[1:], fmid) + full)
    torch.cuda.synchronize()
    rng = eager.float().abs().max().item()
    assert (eager.float() - plain.float()).abs().max().item() > 1e-2 * rng
    assert torch.equal(got, eager)
    assert torch.equal(zero, plain) and torch.equal(idle, plain)
    assert torch.equal(mixed[0], plain[0]) and torch.equal(mixed[1], eager[1])
    d = (shared.float() - eager.float()).abs().max().item()
    d_stock = (got.float() - stock.float()).abs().max().item()
    print(f"first_attn={first_attn}: scatter with the shared CFG prefix vs the eager route {d:.3e}; scatter vs the eager route with "
          f"ControlNetModel.forward's own multiplies {d_stock:.3e} (range {rng:.2f})")
    assert d < 2e-3 * rng and d_stock < 2e-3 * rng


def test_two_nets_scattered_equal_the_multi_controlnet_hook(ops):
    """MultiControlNetModel's `unscaled` outputs scattered with the per-net gates, against the eager keywords handed
    `a * s_a + b * s_b` (the products as torch multiplies real-size tensors, _times): torch.equal without the shared prefix.
    Against the default forward's own residuals (small tensors scaled by torch's single-rounding variant): 2e-3 of the range."""
    from diffusionspatialcontrol_amd.modules.controlnet import MultiControlNetModel
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNetConfig
    cfg = UNetConfig.tiny()
    unet = _unet(cfg)
    multi = MultiControlNetModel([_controlnet(cfg, 5)[0], _controlnet(cfg, 6)[0]])
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 4, 16, 16, generator=g).half().cuda().repeat(2, 1, 1, 1)
    text = torch.randn(2, 77, 64, generator=g).half().cuda()
    conds = [torch.rand(1, 3, 128, 128, generator=g).half().cuda().repeat(2, 1, 1, 1) for _ in range(2)]
    t = torch.tensor([450.0, 450.0], device="cuda")
    with torch.no_grad():
        down, mid = multi(x, t, text, conds, [0.5, 0.4], return_dict=False)
        raw_down, raw_mid = multi(x, t, text, conds, None, unscaled=True, return_dict=False)
        assert len(raw_down) == 2 and len(raw_down[0]) == len(down) == 12 and len(raw_mid) == 2
        feats = [_stack([raw_down[0][k], raw_down[1][k]]) for k in range(12)]
        stock = unet(x, t, text, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
        summed = [_times(a, 0.5) + _times(b, 0.4) for a, b in zip(raw_down[0] + [raw_mid[0]], raw_down[1] + [raw_mid[1]])]
        eager = unet(x, t, text, down_block_additional_residuals=summed[:-1], mid_block_additional_residual=summed[-1]).sample
        got = unet(x, t, text, down_block_scattered=(feats, _stack(raw_mid), _f32([[0.5, 0.5], [0.4, 0.4]]), _i32([0, 1]))).sample
    torch.cuda.synchronize()
    assert torch.equal(got, eager)
    rng = stock.float().abs().max().item()
    assert (got.float() - stock.float()).abs().max().item() < 2e-3 * rng


# ----------------------------------------------------------------------------- the batcher
KARRAS = {"scheduler": "karras"}
STEPS, SCALE, START, END = 5, 0.9, 0.0, 0.6


def _serve_one(b, req, **kw):
    fut = b.submit(dict(req, **kw))
    b.run_until_idle()
    return fut.result().float().cpu()


def _image(seed):
    return torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(seed))


def _latents(seed):
    return torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).half()


def _setup(seed=0):
    import types
    import test_unet_pipeline_gpu as up
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    cfg, unet, sd, text = up._tiny_setup(1, seed=seed)
    state, ids, rs = up._region_state(n_img=1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    base = {"prompt_embeds": text[1:2].cuda(), "negative_prompt_embeds": text[:1].cuda(), "text_input_ids": ids,
            "region_map_state": state, "guidance_scale": 7.5, "sampler_opt": KARRAS}
    common = dict(guidance_scale=7.5, output_type="latent", region_map_state=state, sampler_name="sample_dpmpp_2m",
                  sampler_opt=KARRAS, prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], text_input_ids=ids, width=128,
                  height=128)
    return types.SimpleNamespace(cfg=cfg, sd=sd, text=text, rs=rs, pipe=pipe, base=base, common=common)


@pytest.fixture(scope="module")
def served():
    """one tiny pipeline (the oracle shares its weights): a request served BEFORE setup_controlnet, then the ControlNet (zero
    convolutions re-drawn), a batcher built without the flag and a warm batcher built with it (one bucket of two slots)"""
    tn = _setup()
    tn.req = dict(tn.base, latents=_latents(11).cuda(), num_inference_steps=4)
    tn.before = _serve_one(tn.pipe.serve(128, 128, max_batch=2, buckets=(2,)).warm(), tn.req)
    tn.cn, tn.cn_sd = _controlnet(tn.cfg)
    tn.pipe.setup_controlnet(tn.cn)
    tn.off = tn.pipe.serve(128, 128, max_batch=2, buckets=(2,)).warm()
    tn.b = tn.pipe.serve(128, 128, max_batch=2, buckets=(2,), controlnet=True).warm()
    return tn


def test_flag_off_batcher_is_the_batcher_it_was(served):
    """a batcher built WITHOUT the flag on a pipeline WITH a ControlNet: bit for bit the request served before setup_controlnet,
    and the key is still refused"""
    got = _serve_one(served.off, served.req)
    assert torch.equal(got, served.before), (got - served.before).abs().max().item()
    with pytest.raises(ValueError, match="control_img"):
        served.off.submit(dict(served.req, control_img=_image(10)))
    assert served.off.stats()["control_steps"] == 0 and served.off.stats()["control_gate_updates"] == 0


@pytest.mark.parametrize("kw", [{}, {"control_img": 10, "controlnet_conditioning_scale": 0.0},
                                {"control_img": 10, "control_guidance_start": 0.7, "control_guidance_end": 0.3}])
def test_flag_on_plain_requests_equal_the_flag_off_batcher(served, kw):
    """no control image, scale 0, an empty window: the step with every lane idle computes, bit for bit, what the step without
    the keyword computes - thirteen launches that return before they touch anything, and one copy of the last skip tensor.  At
    this shape (16 pixel rows at the last level; a producer emits GroupNorm statistics from 1024 pixel rows on) no reader of
    the skips or of the mid output takes producer statistics that the adds invalidate.  The ControlNet never runs."""
    kw = dict(kw)
    if "control_img" in kw:
        kw["control_img"] = _image(kw["control_img"])
    s0 = served.b.stats()
    got = _serve_one(served.b, served.req, **kw)
    assert torch.equal(got, served.before), (got - served.before).abs().max().item()
    st = served.b.stats()
    assert st["control_steps"] == s0["control_steps"] and st["control_gate_updates"] == s0["control_gate_updates"]
    assert st["captures_after_warm"] == 0 and served.b._lanes == [None, None]


def _relations(what, got, own, ref, plain):
    """d(served, oracle) < 4e-2 range (the bound of test_controlnet_pipeline_vs_oracle for this path); d(served, oracle)
    <= 2 d(pipeline method, oracle) (the served route is no worse an approximation); the control is live: > 1e-2 range from the
    same request without it.  d(served, pipeline method) is printed, not asserted."""
    rng = ref.abs().max().item()
    d_served, d_own = (got - ref).abs().max().item(), (own - ref).abs().max().item()
    print(f"{what}: d(served, oracle) {d_served:.3e}  d(pipeline method, oracle) {d_own:.3e}  d(served, pipeline method) "
          f"{(got - own).abs().max().item():.3e}  d(served, no control) {(got - plain).abs().max().item():.3e}  range {rng:.2f}")
    assert torch.isfinite(got).all()
    assert d_served < 4e-2 * rng, (d_served, rng)
    assert d_served <= 2 * d_own, (d_served, d_own)
    assert (got - plain).abs().max().item() > 1e-2 * rng


def _oracle_control(cn_sd, ctrl, scales):
    return {"sd": cn_sd, "cond": torch.cat([ctrl.half().float()] * 2), "scale": scales}


CONTROL = dict(controlnet_conditioning_scale=SCALE, control_guidance_start=START, control_guidance_end=END)


def test_control_request_against_the_oracle_and_txt2img(served):
    """5 steps, scale 0.9, window [0, 0.6] (keep 1, 1, 1, 0, 0: three ControlNet replays), built as
    tests/test_unet_pipeline_gpu.py::test_controlnet_pipeline_vs_oracle builds it.  `txt2img`'s captured step rounds the scale to
    fp16 and the batcher does not, so the two are not expected to agree bit for bit (printed, not asserted).
    Measured on one MI355X (one run): d(served, oracle) 1.281e-01, d(txt2img(fused=False), oracle) 1.330e-01, d(served, txt2img)
    1.602e-01, d(served, no control) 1.200e+01, range 56.50."""
    tn, img, lat = served, _image(7), _latents(6)
    req = dict(tn.base, latents=lat.cuda(), num_inference_steps=STEPS)
    s0 = tn.b.stats()
    got = _serve_one(tn.b, req, control_img=img, **CONTROL)
    s1 = tn.b.stats()
    assert s1["control_steps"] - s0["control_steps"] == 3
    assert s1["control_gate_updates"] - s0["control_gate_updates"] == 2                   # the window opens, the window closes
    plain = _serve_one(tn.b, req)
    own = tn.pipe.txt2img(None, num_inference_steps=STEPS, latents=lat.clone(), control_img=img, fused=False, **CONTROL,
                          **tn.common)[0].float().cpu()
    sig = tn.pipe.get_sigmas(STEPS, KARRAS).half().float().cpu()
    keep = [1.0, 1.0, 1.0, 0.0, 0.0]
    ref = unet_ref.denoise_loop(tn.sd, tn.cfg, lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), tn.text.float(), tn.rs,
                                7.5, controlnet=_oracle_control(tn.cn_sd, img, [SCALE * k for k in keep]))
    _relations("txt2img request", got, own, ref, plain)
    assert tn.b.stats()["captures_after_warm"] == 0 and tn.b._lanes == [None, None]


def test_img2img_control_request_against_the_oracle_and_img2img(served):
    """`image` = 4-channel latents, strength 0.6 of 5 steps: 3 model calls on sigmas[2:] (4 sigmas); img2img hands
    preprocess_controlnet len(sigma_sched) = 4, so keep = 1, 1, 0, 0 for the window [0, 0.6]: two ControlNet replays.
    Measured on one MI355X (one run): d(served, oracle) 1.437e-02, d(img2img(fused=False), oracle) 1.856e-02, d(served, img2img)
    1.660e-02, d(served, no control) 1.263e+00, range 5.31."""
    tn, img = served, _image(12)
    lat0 = (_latents(21) * 0.8).half()
    gen = lambda: torch.Generator().manual_seed(33)                                                    # noqa: E731
    req = dict(tn.base, image=lat0.clone().cuda(), strength=0.6, num_inference_steps=STEPS)
    s0 = tn.b.stats()
    got = _serve_one(tn.b, dict(req, generator=gen()), control_img=img, **CONTROL)
    assert tn.b.stats()["control_steps"] - s0["control_steps"] == 2
    plain = _serve_one(tn.b, dict(req, generator=gen()))
    own = tn.pipe.img2img(None, num_inference_steps=STEPS, latents=lat0.clone(), strength=0.6, generator=gen(), control_img=img,
                          fused=False, **CONTROL, **tn.common)[0].float().cpu()
    sig = tn.pipe.get_sigmas(STEPS, KARRAS).half().float().cpu()
    sched = sig[STEPS - min(int(STEPS * 0.6), STEPS):]
    noise = torch.randn(lat0.shape, generator=gen(), dtype=torch.float16).float()
    keep = [1.0 - float(i / len(sched) < START or (i + 1) / len(sched) > END) for i in range(len(sched))]
    assert len(sched) == 4 and keep == [1.0, 1.0, 0.0, 0.0]
    ref = unet_ref.denoise_loop(tn.sd, tn.cfg, lat0.float() + noise * math.sqrt(float(sched[0]) ** 2 + 1), sched.tolist(),
                                tn.text.float(), tn.rs, 7.5, controlnet=_oracle_control(tn.cn_sd, img, [SCALE * k for k in keep]))
    _relations("img2img request", got, own, ref, plain)
    assert tn.b.stats()["captures_after_warm"] == 0


# ----------------------------------------------------------------------------- lanes
@pytest.fixture(scope="module")
def one_lane(served):
    """two slots, buckets 1 and 2, ONE ControlNet lane - on the `served` pipeline"""
    return served.pipe.serve(128, 128, max_batch=2, buckets=(1, 2), controlnet=True, control_slots=1).warm()


def _solo_equal(b, specs, got):
    solo = {n: _serve_one(b, dict(s)) for n, s in specs.items()}
    rng = max(v.abs().max().item() for v in solo.values())
    dist = {n: (got[n] - solo[n]).abs().max().item() for n in specs}
    for n, d in dist.items():
        print(f"request {n}: vs its own solo served run {d:.3e} (range {rng:.2f})")
    for n, d in dist.items():
        assert d < 2e-3 * rng, (n, d, rng)
    return solo, rng


def test_lanes_follow_bucket_switches_and_slots(served, one_lane):
    """A (control) runs alone in bucket 1 (lane rows -> batch rows 0, 1); P (plain) joins: bucket 2, dst becomes 0, 2 - the gate
    vector of the NEW bucket is uploaded once, the ControlNet graph is the one it was.  Then Q (plain) first and B (control)
    second: B sits in slot 1 on lane 0.  Each equals its own solo served run within 2e-3 of the range (the bound of the mixed
    membership tests: both sides run the same kernels, in buckets of different sizes); no capture after warm().
    Measured on one MI355X (one run): 0.0 for all four, range 60.66."""
    b, base = one_lane, served.base
    specs = {"A": dict(base, latents=_latents(41).cuda(), num_inference_steps=4, control_img=_image(51), **CONTROL),
             "P": dict(base, latents=_latents(42).cuda(), num_inference_steps=3, sampler_opt={"scheduler": "exponential"}),
             "Q": dict(base, latents=_latents(43).cuda(), num_inference_steps=2),
             "B": dict(base, latents=_latents(44).cuda(), num_inference_steps=3, guidance_scale=5.0, control_img=_image(54),
                       controlnet_conditioning_scale=0.5)}
    s0 = b.stats()
    futs = {"A": b.submit(dict(specs["A"]))}
    b.step()
    s1 = b.stats()
    assert s1["bucket"] == 1 and s1["control_gate_updates"] == s0["control_gate_updates"] + 1 and b._lanes[0] is b._slots[0]
    futs["P"] = b.submit(dict(specs["P"]))
    b.step()                                             # A's second call (keep[1] of 4: still open), now in bucket 2
    s2 = b.stats()
    assert s2["bucket"] == 2 and s2["control_gate_updates"] == s1["control_gate_updates"] + 1
    assert s2["control_steps"] == s0["control_steps"] + 2
    b.step()                                             # keep[2] = 0 (3 / 4 > 0.6): the window closes, nothing else happens
    s3 = b.stats()
    assert s3["control_gate_updates"] == s2["control_gate_updates"] + 1 and s3["control_steps"] == s2["control_steps"]
    assert s3["refreshes"] == s2["refreshes"]
    b.run_until_idle()
    futs["Q"] = b.submit(dict(specs["Q"]))
    futs["B"] = b.submit(dict(specs["B"]))
    b.step()
    assert b._slots[1] is not None and b._slots[1].lane == 0 and b._lanes[0] is b._slots[1]
    b.run_until_idle()
    assert b.stats()["captures_after_warm"] == 0 and b._lanes == [None]
    got = {n: f.result().float().cpu() for n, f in futs.items()}
    solo, rng = _solo_equal(b, specs, got)
    no_control = _serve_one(b, {k: v for k, v in specs["A"].items() if "control" not in k})
    assert (got["A"] - no_control).abs().max().item() > 1e-2 * rng
    assert b.stats()["captures_after_warm"] == 0


def test_two_control_requests_queue_on_one_lane(served, one_lane):
    """A and B both carry a control image; one lane: B is not admitted while A holds the lane although slot 1 is free, and joins
    when A has left.  Both equal their solo served runs within 2e-3 of the range (measured on one MI355X: 0.0, range 58.66)."""
    b, base = one_lane, served.base
    specs = {"A": dict(base, latents=_latents(61).cuda(), num_inference_steps=2, control_img=_image(71)),
             "B": dict(base, latents=_latents(62).cuda(), num_inference_steps=2, control_img=_image(72),
                       controlnet_conditioning_scale=0.7)}
    futs = {n: b.submit(dict(s)) for n, s in specs.items()}
    b.step()
    assert b._slots[0] is not None and b._slots[1] is None and b.stats()["queued"] == 1
    b.step()
    assert b._slots[1] is None and b.stats()["queued"] == 1
    b.step()                                             # A's last step is applied: it leaves and frees the lane
    assert b._slots == [None, None] and b._lanes == [None] and b.stats()["queued"] == 1
    b.step()
    assert b._slots[0] is not None and b._slots[0].lane == 0 and b.stats()["queued"] == 0
    b.run_until_idle()
    got = {n: f.result().float().cpu() for n, f in futs.items()}
    _solo_equal(b, specs, got)
    assert b.stats()["captures_after_warm"] == 0


# ----------------------------------------------------------------------------- two nets
def test_multi_controlnet_one_net_open_equals_the_single_net_batcher():
    """Three pipelines on the same UNet weights: nets [N0, N1], N0 alone, N1 alone.  Scales [s, 0] with images [a, b] against
    the single-net batcher of N0 with image a at s, and [0, s] against N1 with b: the closed net's rows are never read and the
    chain is the one-net chain.  Bit for bit: the open net's ControlNet graph, the scatter chain and the step are the same
    launches on the same values (measured on one MI355X: 0.0 both ways; net 0 against net 1: 19.0 of a range of 68.3)."""
    multi, one0, one1 = _setup(seed=1), _setup(seed=1), _setup(seed=1)
    n0, n1 = _controlnet(multi.cfg, 15)[0], _controlnet(multi.cfg, 25)[0]
    multi.pipe.setup_controlnet([n0, n1])
    one0.pipe.setup_controlnet(n0)
    one1.pipe.setup_controlnet(n1)
    kw = dict(max_batch=2, buckets=(2,), controlnet=True, control_slots=1)
    bm, b0, b1 = (t.pipe.serve(128, 128, **kw).warm() for t in (multi, one0, one1))
    a, b_, s, lat = _image(81), _image(82), 0.8, _latents(83)
    req = dict(num_inference_steps=3, latents=lat.cuda())
    got0 = _serve_one(bm, dict(multi.base, **req), control_img=[a, b_], controlnet_conditioning_scale=[s, 0.0])
    got1 = _serve_one(bm, dict(multi.base, **req), control_img=[a, b_], controlnet_conditioning_scale=[0.0, s])
    want0 = _serve_one(b0, dict(one0.base, **req), control_img=a, controlnet_conditioning_scale=s)
    want1 = _serve_one(b1, dict(one1.base, **req), control_img=b_, controlnet_conditioning_scale=s)
    rng = want0.abs().max().item()
    d0, d1 = (got0 - want0).abs().max().item(), (got1 - want1).abs().max().item()
    print(f"[s, 0] vs net 0 alone {d0:.3e}; [0, s] vs net 1 alone {d1:.3e}; net 0 vs net 1 {(want0 - want1).abs().max().item():.3e} "
          f"(range {rng:.2f})")
    assert torch.equal(got0, want0) and torch.equal(got1, want1)        # (and so within the 2e-3 of the range asked for)
    assert (want0 - want1).abs().max().item() > 1e-2 * rng
    assert bm.stats()["captures_after_warm"] == 0 and bm.stats()["control_steps"] == 6


def test_two_copies_of_one_net_at_half_scales_satisfy_the_single_net_oracle():
    """a MultiControlNetModel of two copies of one net, one image twice, scales 0.5 and 0.4: the oracle relations of the
    single-net request at 0.9 (0.5 d + 0.4 d, each product and the sum rounded to fp16, against the oracle's fp32 0.9 d).
    Measured on one MI355X (one run): d(served, oracle) 1.219e-01, d(txt2img(fused=False), oracle) 1.473e-01, d(served, txt2img)
    1.719e-01, d(served, no control) 1.731e+01, range 63.31."""
    tn = _setup(seed=2)
    cn, cn_sd = _controlnet(tn.cfg, 35)
    twin, _ = _controlnet(tn.cfg, 35)
    tn.pipe.setup_controlnet([cn, twin])
    b = tn.pipe.serve(128, 128, max_batch=2, buckets=(2,), controlnet=True).warm()
    img, lat = _image(91), _latents(92)
    kw = dict(controlnet_conditioning_scale=[0.5, 0.4], control_guidance_start=START, control_guidance_end=END)
    req = dict(tn.base, latents=lat.cuda(), num_inference_steps=STEPS)
    got = _serve_one(b, req, control_img=[img, img], **kw)
    plain = _serve_one(b, req)
    own = tn.pipe.txt2img(None, num_inference_steps=STEPS, latents=lat.clone(), control_img=[img, img], fused=False, **kw,
                          **tn.common)[0].float().cpu()
    sig = tn.pipe.get_sigmas(STEPS, KARRAS).half().float().cpu()
    ref = unet_ref.denoise_loop(tn.sd, tn.cfg, lat.float() * math.sqrt(float(sig[0]) ** 2 + 1), sig.tolist(), tn.text.float(), tn.rs,
                                7.5, controlnet=_oracle_control(cn_sd, img, [0.9 * k for k in (1.0, 1.0, 1.0, 0.0, 0.0)]))
    _relations("two copies of one net", got, own, ref, plain)
    assert b.stats()["captures_after_warm"] == 0 and b.stats()["control_steps"] == 3
