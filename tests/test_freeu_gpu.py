"""FreeU on the MI355X (`-m gpu`): dsc_freeu_rows_f16 (the half-channel scale and the four-frequency Fourier filter of an up-block
ResNet's two inputs, per batch row, in place, in one launch) against the fp64 closed form and torch's own multiply, its identity
rows, determinism and refusals; `UNet2DConditionModel.enable_freeu` / `forward(freeu_rows=...)` against the fp32 oracle with
torch.fft; the captured step across enable / change / disable; and the serving batcher with per-request values."""
import ctypes

import numpy as np
import pytest
import torch

import freeu_ref as fr
from inputs import FakeTokenizer

pytestmark = pytest.mark.gpu
CL = torch.channels_last
VALUES = (0.9, 0.2, 1.5, 1.6)           # the paper's values for SD 1.x: s1, s2, b1, b2
OTHER = (0.6, 0.4, 1.1, 1.2)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- the kernel
#         B, C_h, C_s, H, W
SHAPES = [(3, 64, 64, 2, 2),
          (2, 64, 64, 4, 4),
          (2, 32, 64, 3, 5),
          (2, 1280, 1280, 8, 8),       # SD1.5 up block 0
          (2, 1280, 640, 16, 16),      # SD1.5 up block 1, last ResNet
          (2, 64, 64, 19, 19),
          (1, 64, 64, 32, 32)]         # more pixels than a workgroup has row slices
GUARD = 64                             # halfs of sentinel in front of and behind each operand


def _guarded(t):
    """t's values in a channels-last tensor that sits inside a sentinel-filled flat buffer -> (tensor, whole buffer)"""
    B, C, H, W = t.shape
    flat = torch.full((t.numel() + 2 * GUARD,), 777.0, dtype=torch.float16)
    flat[GUARD:GUARD + t.numel()] = t.permute(0, 2, 3, 1).reshape(-1).half()
    flat = flat.cuda()
    view = flat[GUARD:GUARD + t.numel()].view(B, H, W, C).permute(0, 3, 1, 2)
    assert view.is_contiguous(memory_format=CL) and view.data_ptr() % 16 == 0
    return view, flat


def _operands(B, C_h, C_s, H, W, seed):
    hidden = fr.activations((B, C_h, H, W), seed).half()
    skip = fr.activations((B, C_s, H, W), seed + 1).half()
    return hidden, skip


def _ordinal(t):
    """fp16 values as integers in which neighbouring values differ by one"""
    i = t.cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _params(rows):
    return torch.tensor(rows, dtype=torch.float32, device="cuda").reshape(-1, 4).contiguous()


@pytest.fixture(scope="module")
def references():
    """the fp64 closed form of each shape's skip tensor, once per (shape, stage), rounded to fp16"""
    cache = {}

    def get(shape, stage, rows):
        key = (shape, stage)
        if key not in cache:
            _, skip = _operands(*shape, seed=sum(shape))
            s = np.array([np.float32(r[stage]) for r in rows], dtype=np.float64)          # the kernel reads fp32 values
            # rounded ONCE, by numpy: torch's float64 -> float16 goes through float32, and that second rounding moves 1.8 % of
            # the elements of the 2 x 2 case (where the result is s * x with a 24-bit s) by an ulp
            cache[key] = torch.from_numpy(fr.closed_form(skip.double().numpy(), s).astype(np.float16))
        return cache[key]
    return get


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("B, C_h, C_s, H, W", SHAPES)
def test_kernel_against_the_closed_form_and_torchs_multiply(ops, references, B, C_h, C_s, H, W, stage):
    """skip: every element within 1 fp16 ulp of the fp64 closed form rounded to fp16, at most 1 % of them different at all (an
    fp32 evaluation of the form on the CPU at 16 x 16 x 64 differs from fp64 on 0.12 % of the elements, each by one ulp: the cap
    leaves eight times that).  The rows' s run from 0.9 down (stage 0) and from the paper's 0.2 up (stage 1); with 0.2 the
    result crosses zero, where an ulp is small: a kernel with fp32 sums was up to 9 ulps off there (0.1 % of the elements
    differed), which is why the kernel sums in fp64.  Measured on one MI355X with fp64 sums: 0 ulp, 0.000 % at every shape.
    hidden: the first half is `fp16(fp32(x) * b)` bit for bit - torch's fp16 `x * b` as the CPU computes it, and
    `(x.float() * b).half()` on the GPU; the second half and the bytes around both operands are untouched.  (torch's own fp16
    `x * b` ON THE GPU is printed, not asserted: on small tensors its kernel rounds the product once, straight to fp16, and
    differs from the CPU's result by one ulp - measured on one MI355X: 0.1 - 0.6 % of the elements at the 64-channel shapes, none
    at the 1280-channel ones.)"""
    shape = (B, C_h, C_s, H, W)
    rows = [(0.9 - 0.1 * r, 0.2 + 0.1 * r, 1.5 + 0.05 * r, 1.6 - 0.05 * r) for r in range(B)]
    hidden0, skip0 = _operands(*shape, seed=sum(shape))
    hidden, hbuf = _guarded(hidden0)
    skip, sbuf = _guarded(skip0)
    params = _params(rows)
    got_h, got_s = ops.freeu_rows_(hidden, skip, params, stage)
    torch.cuda.synchronize()
    assert got_h.data_ptr() == hidden.data_ptr() and got_s.data_ptr() == skip.data_ptr()
    ref = references(shape, stage, rows)
    d = (_ordinal(skip) - _ordinal(ref)).abs()
    frac = (d > 0).float().mean().item()
    print(f"{shape} stage {stage}: worst {int(d.max())} ulp, {100 * frac:.3f} % of the elements differ")
    assert int(d.max()) <= 1 and frac <= 0.01
    assert not torch.equal(skip.cpu(), skip0)
    b = [float(np.float32(r[2 + stage])) for r in rows]                                  # the kernel reads fp32 values
    half = C_h // 2
    want = torch.stack([hidden0[r, :half] * b[r] for r in range(B)])                     # torch's fp16 tensor * python float
    two_ops = torch.stack([(hidden0[r, :half].cuda().float() * b[r]).half() for r in range(B)])
    on_gpu = torch.stack([hidden0[r, :half].cuda() * b[r] for r in range(B)])
    print(f"    hidden: {(hidden[:, :half] != on_gpu).float().mean().item() * 100:.3f} % of the elements differ from torch's fp16 "
          f"multiply as the GPU computes it")
    assert torch.equal(hidden[:, :half].cpu(), want) and torch.equal(hidden[:, :half], two_ops)
    assert torch.equal(hidden[:, half:].cpu(), hidden0[:, half:])
    for buf in (hbuf, sbuf):
        assert (buf[:GUARD] == 777.0).all() and (buf[-GUARD:] == 777.0).all()
    assert torch.equal(params, _params(rows))


def test_rows_of_a_batch_equal_each_row_alone_and_a_second_run(ops):
    """B = 4 with four different (s, b) rows: each row is, bit for bit, that row run alone (B = 1) - and the whole launch run
    again on the same inputs gives the same bits (fixed-order sums, no atomics)"""
    shape = (4, 64, 64, 19, 19)
    rows = [VALUES, OTHER, (0.3, 0.5, 0.8, 2.0), (1.0, 0.7, 1.0, 1.3)]
    hidden0, skip0 = _operands(*shape, seed=11)
    for stage in (0, 1):
        h = hidden0.contiguous(memory_format=CL).cuda()
        s = skip0.contiguous(memory_format=CL).cuda()
        ops.freeu_rows_(h, s, _params(rows), stage)
        h2 = hidden0.contiguous(memory_format=CL).cuda()
        s2 = skip0.contiguous(memory_format=CL).cuda()
        ops.freeu_rows_(h2, s2, _params(rows), stage)
        torch.cuda.synchronize()
        assert torch.equal(h, h2) and torch.equal(s, s2)
        for r in range(4):
            h1 = hidden0[r:r + 1].contiguous(memory_format=CL).cuda()
            s1 = skip0[r:r + 1].contiguous(memory_format=CL).cuda()
            ops.freeu_rows_(h1, s1, _params([rows[r]]), stage)
            torch.cuda.synchronize()
            assert torch.equal(h[r], h1[0]) and torch.equal(s[r], s1[0]), (stage, r)


def test_identity_rows_keep_their_bits_whatever_they_hold(ops):
    """b == 1: the hidden row is neither read nor written; s == 1: the skip row neither - rows full of NaN (an fp16 NaN times 1,
    or summed, would come back as another NaN pattern or spread) keep every bit.  The other rows are filtered as usual."""
    shape = (4, 64, 64, 8, 8)
    hidden0, skip0 = _operands(*shape, seed=5)
    nan = torch.full((64, 8, 8), float("nan")).half().view(torch.int16)
    nan[::2] |= 0x0155                                    # payload bits: a NaN that arithmetic would not reproduce
    nan = nan.view(torch.float16)
    #        s1   s2   b1   b2
    rows = [(1.0, 1.0, 1.0, 1.0), (1.0, 0.5, 1.4, 1.0), (0.5, 1.0, 1.0, 1.4), (0.5, 0.5, 1.4, 1.4)]
    for stage in (0, 1):
        hidden0[0], skip0[0] = nan, nan
        s_id = [r for r in range(4) if rows[r][stage] == 1.0]
        b_id = [r for r in range(4) if rows[r][2 + stage] == 1.0]
        for r in s_id:
            skip0[r] = nan
        for r in b_id:
            hidden0[r] = nan
        h = hidden0.contiguous(memory_format=CL).cuda()
        s = skip0.contiguous(memory_format=CL).cuda()
        ops.freeu_rows_(h, s, _params(rows), stage)
        torch.cuda.synchronize()
        for r in range(4):
            same_s = torch.equal(s[r].cpu().view(torch.int16), skip0[r].view(torch.int16))
            same_h = torch.equal(h[r].cpu().view(torch.int16), hidden0[r].view(torch.int16))
            assert same_s == (r in s_id) and same_h == (r in b_id), (stage, r)
        hidden0, skip0 = _operands(*shape, seed=5)


def test_under_graph_capture_the_replay_reads_the_device_values_of_that_moment(ops):
    shape = (2, 64, 64, 4, 4)
    hidden0, skip0 = _operands(*shape, seed=2)
    h = hidden0.contiguous(memory_format=CL).cuda()
    s = skip0.contiguous(memory_format=CL).cuda()
    params = _params([(1.0,) * 4] * 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.freeu_rows_(h, s, params, 0)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.freeu_rows_(h, s, params, 0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(h.cpu(), hidden0) and torch.equal(s.cpu(), skip0)            # all ones: nothing touched
    params.copy_(_params([VALUES, (1.0,) * 4]))
    g.replay()
    torch.cuda.synchronize()
    eh, es = ops.freeu_eager(hidden0[:1], skip0[:1], VALUES[0], VALUES[2])
    assert torch.equal(h[0].cpu(), eh[0]) and (_ordinal(s[0]) - _ordinal(es[0])).abs().max() <= 1
    assert torch.equal(h[1].cpu(), hidden0[1]) and torch.equal(s[1].cpu(), skip0[1])


def test_every_refusal_returns_its_error_and_launches_nothing(ops):
    from diffusionspatialcontrol_amd import _lib
    lib = _lib.load_library()
    B, C, H, W = 2, 64, 4, 4
    hidden0, skip0 = _operands(B, C, C, H, W, seed=3)
    h = hidden0.contiguous(memory_format=CL).cuda()
    s = skip0.contiguous(memory_format=CL).cuda()
    params = _params([VALUES] * B)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)                                             # noqa: E731
    BAD, UNSUPPORTED = -1, -2                           # DSC_ERR_BAD_ARG, DSC_ERR_UNSUPPORTED (include/dsc_hip.h)

    def call(hp=None, C_h=C, sp=None, C_s=C, B_=B, H_=H, W_=W, pp=None, stage=0):
        return lib.dsc_freeu_rows_f16(p(h) if hp is None else hp, C_h, p(s) if sp is None else sp, C_s, B_, H_, W_,
                                      p(params) if pp is None else pp, stage, None)

    null = ctypes.c_void_p(0)
    cases = {"null hidden": (dict(hp=null), BAD), "null skip": (dict(sp=null), BAD), "null params": (dict(pp=null), BAD),
             "B < 1": (dict(B_=0), BAD), "H < 2": (dict(H_=1), BAD), "W < 2": (dict(W_=1), BAD),
             "C_s % 8": (dict(C_s=60), UNSUPPORTED), "C_h % 16": (dict(C_h=56), UNSUPPORTED),
             "misaligned hidden": (dict(hp=p(h, 2)), UNSUPPORTED), "misaligned skip": (dict(sp=p(s, 8)), UNSUPPORTED),
             "misaligned params": (dict(pp=p(params, 2)), UNSUPPORTED),
             "hidden is skip": (dict(sp=p(h)), BAD), "skip inside hidden": (dict(sp=p(h, 32)), BAD),
             "params inside skip": (dict(pp=p(s, 16)), BAD), "params inside hidden": (dict(pp=p(h, 64)), BAD),
             "stage 2": (dict(stage=2), BAD), "stage -1": (dict(stage=-1), BAD),
             "B above the grid limit": (dict(B_=65536), UNSUPPORTED),
             "H above the table": (dict(H_=ops.FREEU_MAX_SIDE + 1), UNSUPPORTED),
             "W above the table": (dict(W_=ops.FREEU_MAX_SIDE + 1), UNSUPPORTED)}
    assert _lib.load_library().dsc_status_string(BAD) and call() == 0               # (the operands themselves are fine)
    torch.cuda.synchronize()
    after_h, after_s = h.clone(), s.clone()
    for name, (kw, want) in cases.items():
        assert call(**kw) == want, name
    torch.cuda.synchronize()
    assert torch.equal(h, after_h) and torch.equal(s, after_s) and torch.equal(params, _params([VALUES] * B))
    # the wrapper refuses the same things, and what only it can see, before any launch
    with pytest.raises(_lib.DscLibraryError):
        ops.freeu_rows_(h.cpu(), s, params, 0)
    bad = [(h.float(), s, params, 0, TypeError), (h, s[:, :, :3], params, 0, ValueError), (h, s[:1], params, 0, ValueError),
           (h.contiguous(), s, params, 0, ValueError), (h, s, params[:1], 0, ValueError), (h, s, params.double(), 0, ValueError),
           (h, s, params, 2, ValueError), (h, h, params, 0, ValueError), (h[:, :56], s, params, 0, ValueError),
           (h[:, :, :1], s[:, :, :1], params, 0, ValueError)]
    for hh, ss, pp, st, err in bad:
        with pytest.raises(err):
            ops.freeu_rows_(hh, ss, pp, st)
    assert not ops.freeu_covers(h.float(), s) and not ops.freeu_covers(h.contiguous(), s) and ops.freeu_covers(h, s)
    torch.cuda.synchronize()
    assert torch.equal(h, after_h) and torch.equal(s, after_s)


def test_the_op_drops_groupnorm_partials(ops):
    """the contract of every raw-pointer writer in ops: sums a producer attached describe the bytes before the write"""
    hidden0, skip0 = _operands(2, 64, 64, 4, 4, seed=4)
    h = hidden0.contiguous(memory_format=CL).cuda()
    s = skip0.contiguous(memory_format=CL).cuda()
    for t in (h, s):
        ops.attach_gn_partials(t, ops.GnPartials(torch.zeros(4, dtype=torch.float32, device="cuda"), 1, 1, 1, 1, 1))
    assert ops.gn_partials_of(h) is not None and ops.gn_partials_of(s) is not None
    ops.freeu_rows_(h, s, _params([VALUES] * 2), 0)
    assert ops.gn_partials_of(h) is None and ops.gn_partials_of(s) is None


# ----------------------------------------------------------------------------- the UNet
def _tiny(seed=0):
    import test_unet_pipeline_gpu as up
    return up._tiny_setup(1, seed=seed)


def _inputs(h, w):
    g = torch.Generator().manual_seed(5)
    return torch.randn(2, 4, h, w, generator=g).half(), torch.tensor([731.25, 731.25])


@pytest.mark.parametrize("h, w", [(16, 16), (19, 19)])
def test_unet_with_freeu_matches_the_oracle_with_torch_fft(ops, h, w):
    """the tiny fp16 UNet on the kernel route against the same weights in fp32 on the CPU with freeu_eager, at 128 px (up blocks 0 /
    1 at 2 x 2 / 4 x 4) and 152 px (3 x 3 / 5 x 5: odd up-path sides), within test_unet_forward_matches_oracle's bounds"""
    cfg, unet, sd, text = _tiny()
    x, t = _inputs(h, w)
    with torch.no_grad():
        off = unet(x.cuda(), t.cuda(), text.cuda()).sample.float().cpu()
        unet.enable_freeu(*VALUES)
        out = unet(x.cuda(), t.cuda(), text.cuda()).sample.float().cpu()
        rows = unet(x.cuda(), t.cuda(), text.cuda(), freeu_rows=_params([OTHER, (1.0,) * 4])).sample.float().cpu()
        unet.disable_freeu()
        kw = unet(x.cuda(), t.cuda(), text.cuda(), freeu_rows=_params([VALUES] * 2)).sample.float().cpu()
        ones = unet(x.cuda(), t.cuda(), text.cuda(), freeu_rows=_params([(1.0,) * 4] * 2)).sample.float().cpu()
        again = unet(x.cuda(), t.cuda(), text.cuda()).sample.float().cpu()
        ref = fr.freeu_unet_forward(sd, cfg, x.float(), t, text.float(), freeu=VALUES)
        ref_off = fr.freeu_unet_forward(sd, cfg, x.float(), t, text.float())
        ref_rows = fr.freeu_unet_forward(sd, cfg, x.float(), t, text.float(), freeu=torch.tensor([OTHER, (1.0,) * 4]))
    scale = ref.abs().max().item()
    err = (out - ref).abs()
    moved, moved_ref = (out - off).abs().max().item(), (ref - ref_off).abs().max().item()
    print(f"{h}x{w}: max err {err.max().item():.3e}, mean {err.mean().item():.3e}, range {scale:.3f}; FreeU moves the output by "
          f"{moved:.3e} (oracle {moved_ref:.3e})")
    assert err.max().item() < 1e-2 * scale + 1e-3 and err.mean().item() < 2e-3 * scale
    assert moved_ref > 1e-2 * scale and moved > 0.5 * moved_ref
    assert torch.equal(kw, out)                                  # the keyword with the same values in every row: the same bits
    assert torch.equal(ones, off) and torch.equal(again, off)    # rows of ones / disabled: the forward it was, bit for bit
    # the keyword takes precedence over the module-level setting, per row: row 1 (ones) is the plain forward's
    err_rows = (rows - ref_rows).abs()
    assert err_rows.max().item() < 1e-2 * scale + 1e-3 and err_rows.mean().item() < 2e-3 * scale
    assert torch.equal(rows[1], off[1]) and not torch.equal(rows[0], out[0])


def test_b_only_kernel_route_equals_the_eager_route_bit_for_bit(ops):
    """s = 1 leaves the skip tensors alone on both routes and the half-channel scale is torch's own multiply: with DSC_FREEU=0
    (ops.USE_FREEU_KERNEL off: torch.fft and torch's multiply, new tensors) the UNet computes the same bits"""
    cfg, unet, sd, text = _tiny()
    x, t = _inputs(16, 16)
    unet.enable_freeu(1.0, 1.0, 1.5, 1.6)
    try:
        with torch.no_grad():
            kernel = unet(x.cuda(), t.cuda(), text.cuda()).sample
            ops.USE_FREEU_KERNEL = False
            eager = unet(x.cuda(), t.cuda(), text.cuda()).sample
            unet.enable_freeu(*VALUES)
            eager_s = unet(x.cuda(), t.cuda(), text.cuda()).sample
            ops.USE_FREEU_KERNEL = True
            kernel_s = unet(x.cuda(), t.cuda(), text.cuda()).sample
    finally:
        ops.USE_FREEU_KERNEL = True
    assert torch.equal(kernel, eager)
    # with s as well the two routes round the filter differently (fp32 sums against fp32 torch.fft): close, not equal
    rng = kernel_s.float().abs().max().item()
    assert (kernel_s.float() - eager_s.float()).abs().max().item() < 2e-3 * rng


# ----------------------------------------------------------------------------- the captured step
KARRAS = {"scheduler": "karras"}
STEPS = 4


def _setup(seed=0):
    import types
    import test_unet_pipeline_gpu as up
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    cfg, unet, sd, text = up._tiny_setup(1, seed=seed)
    state, ids, rs = up._region_state(n_img=1)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    base = {"prompt_embeds": text[1:2].cuda(), "negative_prompt_embeds": text[:1].cuda(), "text_input_ids": ids,
            "region_map_state": state, "guidance_scale": 7.5, "sampler_opt": KARRAS, "num_inference_steps": STEPS}
    common = dict(guidance_scale=7.5, output_type="latent", region_map_state=state, sampler_name="sample_dpmpp_2m",
                  sampler_opt=KARRAS, prompt_embeds=text[1:2], negative_prompt_embeds=text[:1], text_input_ids=ids, width=128,
                  height=128, num_inference_steps=STEPS)
    return types.SimpleNamespace(cfg=cfg, sd=sd, text=text, pipe=pipe, base=base, common=common)


def _latents(seed, hw=(16, 16)):
    return torch.randn(1, 4, *hw, generator=torch.Generator().manual_seed(seed)).half()


def _txt2img(tn, lat, values=None):
    if values is None:
        tn.pipe.unet.disable_freeu()
    else:
        tn.pipe.unet.enable_freeu(*values)
    return tn.pipe.txt2img(None, fused=True, latents=lat.clone(), **tn.common)[0].float().cpu()


def test_enable_change_disable_across_fused_calls_give_the_bits_of_fresh_pipelines(ops):
    """one pipeline: plain, FreeU on (a second capture), other values (the same capture: the table is refilled in place), off (the
    plain capture again), on again - each call the bits of a fresh pipeline that only ever ran that setting"""
    lat = _latents(11)
    tn = _setup()
    seq = [None, VALUES, OTHER, None, VALUES]
    got = []
    for v in seq:
        got.append(_txt2img(tn, lat, v))
    n_graphs = len(tn.pipe._graphs)
    tn.pipe.unet.disable_freeu()
    fresh = {v: _txt2img(_setup(), lat, v) for v in (None, VALUES, OTHER)}
    for v, g in zip(seq, got):
        assert torch.equal(g, fresh[v]), (v, (g - fresh[v]).abs().max().item())
    rng = fresh[None].abs().max().item()
    assert (fresh[VALUES] - fresh[None]).abs().max().item() > 1e-2 * rng and not torch.equal(fresh[VALUES], fresh[OTHER])
    assert n_graphs == 2                     # the plain step and its twin with the FreeU launches, both kept


# ----------------------------------------------------------------------------- the batcher
def _serve_one(b, req, **kw):
    fut = b.submit(dict(req, **kw))
    b.run_until_idle()
    return fut.result().float().cpu()


@pytest.fixture(scope="module")
def served():
    """one tiny pipeline, a batcher built without the flag and one built with it (one bucket of two slots: slot 1 is idle in a
    solo run), both warm"""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    tn = _setup()
    tn.req = dict(tn.base, latents=_latents(11).cuda())
    tn.off = tn.pipe.serve(128, 128, max_batch=2, buckets=(2,)).warm()
    tn.b = tn.pipe.serve(128, 128, max_batch=2, buckets=(2,), freeu=True).warm()
    return tn


def test_requests_without_the_key_equal_the_flagless_batcher(served):
    """rows of ones: the six launches return before they load anything, and the step computes the bits it computed without them"""
    want = _serve_one(served.off, served.req)
    got = _serve_one(served.b, served.req)
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert served.b.stats()["freeu_updates"] == 0 and served.b.stats()["captures_after_warm"] == 0
    with pytest.raises(ValueError, match="freeu=True"):
        served.off.submit(dict(served.req, freeu=VALUES))


def test_served_request_equals_fused_txt2img_with_the_unet_level_setting(served):
    tn = served
    got = _serve_one(tn.b, tn.req, freeu=VALUES)
    as_dict = _serve_one(tn.b, tn.req, freeu=dict(zip(("s1", "s2", "b1", "b2"), VALUES)))
    plain = _serve_one(tn.b, tn.req)
    try:
        want = _txt2img(tn, _latents(11), VALUES)
    finally:
        tn.pipe.unet.disable_freeu()
    d = (got - want).abs().max().item()
    rng = want.abs().max().item()
    print(f"served with freeu vs txt2img(fused=True) after enable_freeu: {d:.3e}; FreeU moves the result by "
          f"{(got - plain).abs().max().item():.3e} (range {rng:.2f})")
    assert torch.equal(got, want), d
    assert torch.equal(as_dict, got)
    assert (got - plain).abs().max().item() > 1e-2 * rng
    assert tn.b.stats()["captures_after_warm"] == 0


def test_mixed_batch_equals_each_request_alone(served):
    """A (FreeU) and B (none) start together; C (other values) joins the slot A frees while B still runs.  Each equals its own
    solo served run within 2e-3 of the range (the bound of the other serving tests' mixed-membership cases: both sides run the
    same kernels); no capture after warm()"""
    b = served.b
    specs = {"A": dict(served.base, latents=_latents(41).cuda(), num_inference_steps=3, freeu=VALUES),
             "B": dict(served.base, latents=_latents(42).cuda(), num_inference_steps=6, sampler_opt={"scheduler": "exponential"}),
             "C": dict(served.base, latents=_latents(43).cuda(), num_inference_steps=4, guidance_scale=5.0, freeu=OTHER)}
    s0 = b.stats()
    futs = {"A": b.submit(dict(specs["A"])), "B": b.submit(dict(specs["B"]))}
    for _ in range(4):
        b.step()
    assert b._slots[0] is None and b._slots[1] is not None          # A has left, B runs
    futs["C"] = b.submit(dict(specs["C"]))
    b.step()
    assert b._slots[0] is not None and b._slots[0].freeu == OTHER
    b.run_until_idle()
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["joins"] - s0["joins"] == 3, st
    got = {n: f.result().float().cpu() for n, f in futs.items()}
    solo = {n: _serve_one(b, dict(s)) for n, s in specs.items()}
    rng = max(v.abs().max().item() for v in solo.values())
    for n in specs:
        d = (got[n] - solo[n]).abs().max().item()
        print(f"request {n}: vs its own solo served run {d:.3e} (range {rng:.2f})")
        assert d < 2e-3 * rng, (n, d, rng)
    without = _serve_one(b, {k: v for k, v in specs["A"].items() if k != "freeu"})
    assert (got["A"] - without).abs().max().item() > 1e-2 * rng
    flagless = _serve_one(served.off, specs["B"])
    assert (got["B"] - flagless).abs().max().item() < 2e-3 * rng      # B never saw its neighbours' FreeU
    assert b.stats()["captures_after_warm"] == 0


def test_both_passes_of_a_hires_request_carry_it(ops):
    """serve_hires(freeu=True): one chained request == the pair driven by hand with the key on both parts, bit for bit (the
    construction of tests/test_hires_gpu.py::test_chain_equals_its_parts); with the key on one part only the result differs"""
    tn = _setup()
    X, STRENGTH, LAT2 = 1.5, 0.6, (1, 4, 24, 24)
    pair = tn.pipe.serve_hires(128, 128, X, max_batch=2, buckets=(1, 2), freeu=True).warm()
    base = dict(tn.base, num_inference_steps=8)
    lat = _latents(50).cuda()
    noise = torch.randn(LAT2, generator=torch.Generator().manual_seed(51)).half().cuda()
    sig2 = tn.pipe._schedule(8, KARRAS, "cpu", torch.float16).float().tolist()[8 - int(8 * STRENGTH)]

    def run(fut):
        pair.run_until_idle()
        return fut.result()

    chained = run(pair.submit(dict(base, latents=lat, hires_latents=noise, upscale=True, upscale_x=X, upscale_method="bicubic",
                                   upscale_denoising_strength=STRENGTH, freeu=VALUES)))
    assert chained.shape == LAT2 and torch.isfinite(chained).all()

    def by_hand(first_kw, second_kw):
        first = run(pair.submit(dict(base, latents=lat, **first_kw)))
        start = ops.latent_resample_noise(first, LAT2[2:], "bicubic", noise=noise, sigma0=sig2)
        torch.cuda.synchronize()
        return run(pair.hires.submit(dict(base, image=start, latents=torch.zeros_like(noise), strength=STRENGTH, **second_kw)))

    key = {"freeu": VALUES}
    both, first_only, second_only = by_hand(key, key), by_hand(key, {}), by_hand({}, key)
    assert torch.equal(chained, both), (chained.float() - both.float()).abs().max().item()
    assert not torch.equal(chained, first_only) and not torch.equal(chained, second_only)
    st = pair.stats()
    assert st["base"]["captures_after_warm"] == 0 and st["hires"]["captures_after_warm"] == 0
