"""FreeU on the host: `ops.freeu_eager` (torch.fft, fp32) against the fp64 closed form of the four-frequency filter, the
half-channel scale against torch's own multiply, `enable_freeu` / `disable_freeu`, the UNet's FreeU hook on CPU fp32 through the
oracle's forward, the batcher's submit-time checks, and the C-ABI symbol."""
import numpy as np
import pytest
import torch

import freeu_ref as fr
from inputs import FakeTokenizer
from serving_fakes import RecordingExec

from diffusionspatialcontrol_amd import _lib, ops
from diffusionspatialcontrol_amd.modules.serving import ServingBatcher

SIZES = [(2, 2), (2, 4), (3, 5), (4, 4), (9, 10), (16, 16)]
VALUES = (0.9, 0.2, 1.5, 1.6)


@pytest.mark.parametrize("H, W", SIZES + [(8, 8), (12, 12)])
def test_closed_form_is_the_literal_fft_algorithm(H, W):
    """the test's own reference: seven sums and one pass == fft2, fftshift, the centre block times s, and back, in float64"""
    x = fr.activations((2, 3, H, W), seed=H * 31 + W).double().numpy()
    a, b = fr.closed_form(x, 0.2), fr.literal_fft(x, 0.2)
    assert np.abs(a - b).max() < 1e-13 * np.abs(b).max()


@pytest.mark.parametrize("H, W", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_freeu_eager_against_the_closed_form(H, W, dtype):
    """fp32 operands: 1e-5 of the range (torch.fft in fp32 on values of ~10: a few fp32 ulps).  fp16 operands: the same fp32
    computation, rounded once - half an fp16 ulp of the largest value (2 ** (floor(log2 max) - 11)) on top"""
    B, C = 3, 8
    skip = fr.activations((B, C, H, W), seed=H + 7 * W).to(dtype)
    hidden = fr.activations((B, 16, H, W), seed=1).to(dtype)
    s = torch.tensor([0.9, 0.2, 1.0])
    out_h, out_s = ops.freeu_eager(hidden, skip, s, 1.5)
    assert out_s.dtype == dtype and out_s.shape == skip.shape and out_h.dtype == dtype
    ref = fr.closed_form(skip.double().numpy(), s.double().numpy())
    rng = ref.max() - ref.min()
    err = np.abs(out_s.double().numpy() - ref).max()
    bound = 1e-5 * rng + (0.0 if dtype == torch.float32 else 2.0 ** (np.floor(np.log2(np.abs(ref).max())) - 11))
    print(f"{H}x{W} {dtype}: max error {err:.3e}, range {rng:.2f}, bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(out_s[2], skip[2])                      # a row with s == 1 keeps its bits
    assert not torch.equal(out_s[0], skip[0])
    one = ops.freeu_eager(hidden, skip, 0.2, 1.5)[1]           # one number for every row == that number per row
    assert torch.equal(one[1], out_s[1])


def test_at_two_by_two_the_filter_is_s_times_x():
    x = fr.activations((2, 8, 2, 2), seed=3)
    _, out = ops.freeu_eager(torch.zeros(2, 16, 2, 2), x, 0.3, 1.0)
    assert (out - 0.3 * x).abs().max().item() < 1e-5 * (x.max() - x.min()).item()
    assert np.abs(fr.closed_form(x.numpy(), 0.3) - 0.3 * x.double().numpy()).max() < 1e-13


def test_a_side_of_one_is_refused():
    with pytest.raises(ValueError, match="side of 1"):
        ops.freeu_eager(torch.zeros(1, 16, 1, 4), torch.zeros(1, 8, 1, 4), 0.5, 1.2)


@pytest.mark.parametrize("b", [1.5, 1.6, 1.2, 0.7])
def test_hidden_half_scale_is_torchs_fp16_multiply_bit_for_bit(b):
    hidden = fr.activations((2, 32, 5, 3), seed=9).half()
    out, _ = ops.freeu_eager(hidden, torch.zeros(2, 8, 5, 3).half(), 1.0, b)
    assert torch.equal(out[:, :16], hidden[:, :16] * b) and torch.equal(out[:, 16:], hidden[:, 16:])
    assert out.data_ptr() != hidden.data_ptr()
    per_row, _ = ops.freeu_eager(hidden, torch.zeros(2, 8, 5, 3).half(), 1.0, torch.tensor([b, 1.0]))
    assert torch.equal(per_row[0], out[0]) and torch.equal(per_row[1], hidden[1])


def _tiny_unet(seed=0):
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(seed)
    return UNetConfig.tiny(), UNet2DConditionModel(UNetConfig.tiny())


def test_enable_and_disable_set_and_clear_the_block_attributes():
    _, unet = _tiny_unet()
    assert unet.freeu_setting() is None and all(blk.s1 is None for blk in unet.up_blocks)
    unet.enable_freeu(*VALUES)                                   # the reference's names and argument order: s1, s2, b1, b2
    for blk in unet.up_blocks:
        assert (blk.s1, blk.s2, blk.b1, blk.b2) == VALUES
    assert unet.freeu_setting() == VALUES
    unet.enable_freeu(s1=0.6, s2=0.4, b1=1.1, b2=1.2)
    assert unet.freeu_setting() == (0.6, 0.4, 1.1, 1.2)
    unet.disable_freeu()
    for blk in unet.up_blocks:
        assert blk.s1 is None and blk.s2 is None and blk.b1 is None and blk.b2 is None
    assert unet.freeu_setting() is None
    with pytest.raises(ValueError, match="finite"):
        unet.enable_freeu(0.9, float("nan"), 1.5, 1.6)
    assert unet.freeu_setting() is None
    assert "s1" not in unet.state_dict() and not any("freeu" in k for k in unet.state_dict())


def test_the_persistent_table_is_refilled_in_place():
    """what keeps a captured step valid across enable_freeu calls: one table per (rows, device), rewritten, never replaced"""
    _, unet = _tiny_unet()
    unet.enable_freeu(*VALUES)
    tab = unet._freeu_table(4, torch.device("cpu"))
    assert tab.dtype == torch.float32 and tab.shape == (4, 4) and torch.equal(tab, torch.tensor([VALUES] * 4))
    unet.enable_freeu(0.6, 0.4, 1.1, 1.2)
    assert torch.equal(tab, torch.tensor([(0.6, 0.4, 1.1, 1.2)] * 4))
    assert unet._freeu_table(4, torch.device("cpu")) is tab and unet._freeu_table(2, torch.device("cpu")) is not tab
    unet.disable_freeu()
    unet.up_blocks[0].s1, unet.up_blocks[0].s2, unet.up_blocks[0].b1, unet.up_blocks[0].b2 = VALUES      # set by hand
    assert torch.equal(unet._freeu_table(4, torch.device("cpu")), torch.tensor([VALUES] * 4))


@pytest.mark.parametrize("hw", [(16, 16), (19, 19)])
def test_unet_hook_on_cpu_fp32_identity_values_and_real_values(hw):
    """the UNet's FreeU hook (UNet2DConditionModel._freeu) inside the fp32 oracle's forward on the tiny weights (the package's own
    forward runs on the GPU only: tests/test_freeu_gpu.py): values (1, 1, 1, 1) are the disabled forward, bit for bit; the values
    of the paper move the output"""
    cfg, unet = _tiny_unet()
    sd = unet.state_dict()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, *hw, generator=g)
    enc = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    t = torch.tensor([731.25, 731.25])
    with torch.no_grad():
        off = fr.freeu_unet_forward(sd, cfg, x, t, enc)
        ones = fr.freeu_unet_forward(sd, cfg, x, t, enc, freeu=(1.0, 1.0, 1.0, 1.0))
        on = fr.freeu_unet_forward(sd, cfg, x, t, enc, freeu=VALUES)
        mixed = fr.freeu_unet_forward(sd, cfg, x, t, enc, freeu=torch.tensor([VALUES, (1.0, 1.0, 1.0, 1.0)]))
    assert torch.equal(ones, off)
    rng = off.abs().max().item()
    assert (on - off).abs().max().item() > 1e-2 * rng
    assert torch.equal(mixed[1], off[1]) and torch.equal(mixed[0], on[0])


def test_forward_refuses_a_malformed_freeu_rows():
    _, unet = _tiny_unet()
    x, t, enc = torch.zeros(2, 4, 16, 16), torch.zeros(2), torch.zeros(2, 77, 64)
    for bad in (torch.ones(2, 3), torch.ones(3, 4), torch.ones(2, 4, dtype=torch.float64), [[1.0] * 4] * 2):
        with pytest.raises(ValueError, match="freeu_rows"):
            unet(x, t, enc, freeu_rows=bad)


# ----------------------------------------------------------------------------- the batcher's submit-time checks
class _Exec(RecordingExec):
    def set_freeu(self, n, table):
        self._event("set_freeu", n, [list(row) for row in table])


@pytest.fixture()
def pipe():
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    _, unet = _tiny_unet()
    return StableDiffusionPipeline(None, None, FakeTokenizer(), unet.half(), SD15Scheduler())


def _req(name, steps=3, **kw):
    emb = torch.randn(2, 77, 64, generator=torch.Generator().manual_seed(len(name)))
    r = {"name": name, "prompt_embeds": emb[1:2].half(), "negative_prompt_embeds": emb[0:1].half(), "num_inference_steps": steps,
         "guidance_scale": 7.5, "sampler_opt": {"scheduler": "karras"}, "latents": torch.zeros(1, 4, 16, 16).half()}
    r.update(kw)
    return r


@pytest.mark.parametrize("bad", [(0.9, 0.2, 1.5), (0.9, 0.2, 1.5, 1.6, 1.0), (0.9, 0.2, 1.5, float("inf")), (0.9, 0.2, 1.5, float("nan")),
                                 (0.9, "x", 1.5, 1.6), 0.9, {"s1": 0.9, "s2": 0.2, "b1": 1.5}, {"s1": 0.9, "s2": 0.2, "b1": 1.5, "b3": 1.6},
                                 (0.9, 0.2, True, 1.6)])
def test_submit_refuses_a_bad_freeu(pipe, bad):
    b = ServingBatcher(pipe, 128, 128, executor=_Exec(), freeu=True)
    with pytest.raises(ValueError, match="freeu"):
        b.submit(_req("A", freeu=bad))
    assert b.stats()["queued"] == 0 and not b.exec.prepared


def test_submit_takes_a_tuple_or_a_dict_and_the_table_follows_the_members(pipe):
    ex = _Exec()
    b = ServingBatcher(pipe, 128, 128, max_batch=2, buckets=(2,), executor=ex, freeu=True)
    b.submit(_req("A", steps=2, freeu=VALUES))
    b.submit(_req("BB", steps=4, freeu=dict(s1=0.6, s2=0.4, b1=1.1, b2=1.2)))
    b.run_until_idle()
    b.submit(_req("CCC", steps=1))                                       # no key: its rows are ones, nothing is uploaded for it
    b.run_until_idle()
    one, a, bb = [1.0] * 4, list(VALUES), [0.6, 0.4, 1.1, 1.2]
    tables = [e[3] for e in ex.events if e[0] == "set_freeu"]
    assert tables == [[a, bb, a, bb], [one, bb, one, bb], [one] * 4]     # rows {i, n + i}; a slot that empties goes back to ones
    assert b.stats()["freeu_updates"] == 3


def test_the_key_is_refused_without_the_flag(pipe):
    b = ServingBatcher(pipe, 128, 128, executor=_Exec())
    with pytest.raises(ValueError, match=r"freeu=True"):
        b.submit(_req("A", freeu=VALUES))
    assert "freeu_updates" not in b.stats()
    b.submit(_req("A"))
    b.run_until_idle()
    assert not [e for e in b.exec.events if e[0] == "set_freeu"]


@pytest.mark.parametrize("flag", [False, True])
def test_building_a_batcher_is_refused_while_the_unet_level_setting_is_on(pipe, flag):
    pipe.unet.enable_freeu(*VALUES)
    with pytest.raises(ValueError, match=r"disable_freeu"):
        ServingBatcher(pipe, 128, 128, executor=_Exec(), freeu=flag)
    pipe.unet.disable_freeu()
    b = ServingBatcher(pipe, 128, 128, executor=_Exec(), freeu=flag)
    pipe.unet.enable_freeu(*VALUES)                                      # switched on under a live batcher: refused at submit
    with pytest.raises(ValueError, match=r"disable_freeu"):
        b.submit(_req("A"))


def test_step_key_tells_captures_with_and_without_freeu_apart(pipe):
    text = torch.zeros(2, 77, 64, dtype=torch.float16)
    off = pipe._step_key(0, 1, (1, 4, 16, 16), None, text, None, None)
    pipe.unet.enable_freeu(*VALUES)
    on = pipe._step_key(0, 1, (1, 4, 16, 16), None, text, None, None)
    pipe.unet.enable_freeu(0.6, 0.4, 1.1, 1.2)
    assert pipe._step_key(0, 1, (1, 4, 16, 16), None, text, None, None) == on      # values stay out of the key
    pipe.unet.disable_freeu()
    assert pipe._step_key(0, 1, (1, 4, 16, 16), None, text, None, None) == off != on


def test_c_abi_symbol_is_declared_and_bound():
    assert "dsc_freeu_rows_f16" in _lib.declared_symbols() and "dsc_freeu_rows_f16" in _lib._SIGNATURES
    lib = _lib.load_library()
    assert lib.dsc_freeu_rows_f16.restype is not None and len(lib.dsc_freeu_rows_f16.argtypes) == 10
    # the entry refuses before it launches: these return on a machine without a GPU too
    assert lib.dsc_freeu_rows_f16(None, 64, None, 64, 1, 4, 4, None, 0, None) != 0
