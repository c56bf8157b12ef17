"""Finished images in the continuous batcher, the host half: dsc_image_finish's C ABI (exported, declared, bound; its argument
checks run before any GPU call), the constructor's and submit's refusals of the decode lane against a fake executor, and the
torch restatement of the kernel's arithmetic (ops.image_finish_torch, the GPU tests' reference) against the reference chain -
decode_latents' fp16 `(image / 2 + 0.5).clamp(0, 1)`, NHWC float32, numpy_to_pil's `(x * 255).round().astype("uint8")` - over
every fp16 bit pattern that is not a NaN."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from inputs import FakeTokenizer
from serving_fakes import RecordingExec

import diffusionspatialcontrol_amd as dsc
from diffusionspatialcontrol_amd import _lib, build as dsc_build
from diffusionspatialcontrol_amd.modules.serving import ServingBatcher, decode_buckets

S = 77


@pytest.fixture(scope="module")
def lib():
    dsc_build.build(verbose=False)
    return dsc.load_library()


# ----------------------------------------------------------------------------- the C ABI
def test_symbol_is_exported_declared_and_bound(lib):
    assert "dsc_image_finish" in _lib.declared_symbols()
    assert "dsc_image_finish" in _lib._SIGNATURES
    assert hasattr(lib, "dsc_image_finish")
    nm = subprocess.run(["nm", "-D", "--defined-only", dsc.lib_path()], capture_output=True, text=True).stdout
    assert " T dsc_image_finish" in nm
    header = open(_lib.header_path()).read()
    assert re.search(r"#define\s+DSC_IMAGE_U8\s+0\b", header) and re.search(r"#define\s+DSC_IMAGE_F32\s+1\b", header)
    assert "model_k_diffusion.py:291-299" in header and ":533-539" in header          # the reference lines it replaces
    from diffusionspatialcontrol_amd import ops
    assert ops.IMAGE_KINDS["uint8"][0] == 0 and ops.IMAGE_KINDS["float32"][0] == 1


def test_argument_checks_need_no_gpu(lib):
    img, out = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    BAD_ARG, UNSUPPORTED = -1, -2

    def call(img=img, out=out, n=1, H=16, W=24, kind=0):
        return lib.dsc_image_finish(img, out, n, H, W, kind, None)

    assert call(img=None) == BAD_ARG and call(out=None) == BAD_ARG
    assert call(out=img) == BAD_ARG                                  # in place makes no sense: another layout and dtype
    assert call(n=0) == BAD_ARG and call(n=-3) == BAD_ARG
    assert call(H=0) == BAD_ARG and call(W=-8) == BAD_ARG
    assert call(kind=2) == BAD_ARG and call(kind=-1) == BAD_ARG
    for kind in (0, 1):
        assert call(H=12, kind=kind) == UNSUPPORTED and call(W=12, kind=kind) == UNSUPPORTED
        assert call(H=8, W=4, kind=kind) == UNSUPPORTED
    assert call(img=ctypes.c_void_p(0x10008)) == UNSUPPORTED         # 16-byte loads
    assert call(out=ctypes.c_void_p(0x20004), kind=0) == UNSUPPORTED  # 8-byte stores
    assert call(out=ctypes.c_void_p(0x20008), kind=1) == UNSUPPORTED  # 16-byte stores


def test_wrapper_refuses_cpu_tensors():
    from diffusionspatialcontrol_amd import ops
    with pytest.raises(_lib.DscLibraryError, match="GPU only"):
        ops.image_finish(torch.zeros(1, 3, 8, 8, dtype=torch.float16))


# ----------------------------------------------------------------------------- the arithmetic, over every fp16 value
def _all_non_nan_halfs():
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.float16)
    return x[~torch.isnan(x)]


def test_restatement_equals_the_reference_chain_over_all_fp16():
    from diffusionspatialcontrol_amd import ops
    x = _all_non_nan_halfs()
    assert x.numel() == 63490
    per = -(-x.numel() // 3 // 8) * 8                               # a [1, 3, 1, per] image that holds every value once
    img = x.repeat(2)[:3 * per].reshape(1, 3, 1, per).contiguous()
    # the reference, line for line (model_k_diffusion.py decode_latents / numpy_to_pil)
    image = (img / 2 + 0.5).clamp(0, 1)
    ref_f32 = image.cpu().permute(0, 2, 3, 1).float().numpy()
    ref_u8 = (ref_f32 * 255).round().astype("uint8")
    assert np.array_equal(ops.image_finish_torch(img, "float32").numpy(), ref_f32)
    assert np.array_equal(ops.image_finish_torch(img, "uint8").numpy(), ref_u8)
    # the two properties the kernel's uint8 line rests on: the fp32 product with 255 is exact, and 0.5 is its only tie
    h = torch.from_numpy(ref_f32).reshape(-1)
    prod = h * 255.0
    assert torch.equal(prod.double(), h.double() * 255.0)
    ties = h[(prod - torch.floor(prod)) == 0.5]
    assert ties.numel() > 0 and bool((ties == 0.5).all())
    assert int(torch.round(torch.tensor(0.5) * 255.0)) == 128
    assert ref_u8.min() == 0 and ref_u8.max() == 255
    with pytest.raises(ValueError, match="kind"):
        ops.image_finish_torch(img, "int8")


# ----------------------------------------------------------------------------- the batcher's refusals
_NoDeviceExec = RecordingExec         # nothing in these tests reaches a device


def _pipe(with_vae):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKLDecoder, VaeConfig
    torch.manual_seed(0)
    unet = UNet2DConditionModel(UNetConfig.tiny()).half()
    vae = AutoencoderKLDecoder(VaeConfig.tiny()).half() if with_vae else None
    return StableDiffusionPipeline(vae, None, FakeTokenizer(), unet, SD15Scheduler())


@pytest.fixture(scope="module")
def pipe():
    return _pipe(True)


def _req(**kw):
    emb = torch.randn(2, S, 64, generator=torch.Generator().manual_seed(5))
    r = {"prompt_embeds": emb[1:2].half(), "negative_prompt_embeds": emb[0:1].half(), "num_inference_steps": 3,
         "guidance_scale": 7.5, "sampler_opt": {"scheduler": "karras"}, "latents": torch.zeros(1, 4, 16, 16).half()}
    r.update(kw)
    return r


def test_decode_needs_a_vae():
    bare = _pipe(False)
    with pytest.raises(ValueError, match="decode=True.*without a VAE"):
        ServingBatcher(bare, 128, 128, executor=_NoDeviceExec(), decode=True)
    with pytest.raises(ValueError, match="decode=True.*without a VAE"):
        bare.serve_hires(128, 128, 1.5, decode=True)
    with pytest.raises(ValueError, match="decode=True.*without a VAE"):
        bare.serve(128, 128, decode=True)
    ServingBatcher(bare, 128, 128, executor=_NoDeviceExec())                # without the flag a latent-only pipeline serves


@pytest.mark.parametrize("bad", [0, -1, 5, 2.0, True, None])
def test_decode_batch_range(pipe, bad):
    with pytest.raises(ValueError, match="decode_batch"):
        ServingBatcher(pipe, 128, 128, max_batch=4, buckets=(1, 2, 4), executor=_NoDeviceExec(), decode=True, decode_batch=bad)


def test_decode_batch_bounds_are_inclusive_and_buckets(pipe):
    for ok in (1, 4):
        b = ServingBatcher(pipe, 128, 128, max_batch=4, buckets=(1, 2, 4), executor=_NoDeviceExec(), decode=True, decode_batch=ok)
        assert b.decode and b.decode_batch == ok
    assert decode_buckets(1) == (1,) and decode_buckets(2) == (1, 2) and decode_buckets(4) == (1, 2, 4)
    assert decode_buckets(6) == (1, 2, 4, 6) and decode_buckets(8) == (1, 2, 4, 8)


def test_stats_keys_only_with_the_flag(pipe):
    plain = ServingBatcher(pipe, 128, 128, executor=_NoDeviceExec())
    lane = ServingBatcher(pipe, 128, 128, executor=_NoDeviceExec(), decode=True)
    assert not plain.decode and "decodes" not in plain.stats() and "decode_rows" not in plain.stats()
    assert set(lane.stats()) - set(plain.stats()) == {"decodes", "decode_rows"}
    assert lane.stats()["decodes"] == 0 and lane.stats()["decode_rows"] == 0


def test_uint8_needs_the_lane(pipe):
    plain = ServingBatcher(pipe, 128, 128, executor=_NoDeviceExec())
    with pytest.raises(ValueError, match="uint8.*decode=True"):
        plain.submit(_req(output_type="uint8"))
    for ok in ("latent", "np", "pil"):                                       # the flagless batcher takes what it took
        plain.submit(_req(output_type=ok))
    assert plain.stats()["queued"] == 3


def test_unknown_output_type_on_a_decode_batcher(pipe):
    lane = ServingBatcher(pipe, 128, 128, executor=_NoDeviceExec(), decode=True)
    for bad in ("pt", "jpeg", "UINT8", None, 8):
        with pytest.raises(ValueError, match="output_type"):
            lane.submit(_req(output_type=bad))
    assert lane.stats()["queued"] == 0
    for ok in ("latent", "np", "numpy", "uint8"):
        lane.submit(_req(output_type=ok))
    lane.submit(_req())                                                      # the default is still the latent row
    assert lane.stats()["queued"] == 5
