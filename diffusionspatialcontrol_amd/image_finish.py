"""ops.image_finish: the wrapper of dsc_image_finish (csrc/image_finish.hip), the launch that turns the VAE decoder's fp16
channel-major output into the uint8 / float32 [n, H, W, 3] image a served request receives (the decode lane of
modules/serving/), and `image_finish_torch`, the same arithmetic restated in torch for tests and tools."""
import torch

from . import _lib

IMAGE_KINDS = {"uint8": (0, torch.uint8), "float32": (1, torch.float32)}      # DSC_IMAGE_U8 / DSC_IMAGE_F32 (include/dsc_hip.h)


def _ops():
    from . import ops                    # (ops re-exports this module's functions: resolved at call time)
    return ops


def image_finish_torch(img, kind="uint8"):
    """dsc_image_finish's arithmetic on any device, rounding by rounding: fp16 `x * 0.5`, fp16 `+ 0.5`, clamp, NHWC, then
    float32 or `rint(float * 255)` as uint8.  Equal bit for bit to the reference chain (`(image / 2 + 0.5).clamp(0, 1)` on the
    fp16 tensor, `.permute(0, 2, 3, 1).float()`, numpy's `(x * 255).round().astype("uint8")`) for every non-NaN input
    (tests/test_image_serving_host.py walks all of them)."""
    if kind not in IMAGE_KINDS:
        raise ValueError(f"image_finish: kind must be one of {', '.join(IMAGE_KINDS)}, got {kind!r}")
    halved = (img.to(torch.float16).float() * 0.5).to(torch.float16)
    h = (halved.float() + 0.5).to(torch.float16).float().clamp(0.0, 1.0).permute(0, 2, 3, 1).contiguous()
    return h if kind == "float32" else torch.round(h * 255.0).to(torch.uint8)


def image_finish(img, kind="uint8", out=None):
    """img [n, 3, H, W] fp16, contiguous (AutoencoderKLDecoder.decode's output) -> [n, H, W, 3] uint8 (`kind="uint8"`: the bytes
    of the reference's PIL image) or float32 (`kind="float32"`: decode_latents' array), in one launch on the current stream
    (dsc_image_finish).  H and W are multiples of 8.  out: None (a new tensor) or a contiguous tensor of that dtype and shape on
    img's device, written through its raw pointer.  Returns out."""
    ops = _ops()
    ops._require_gpu(img)
    if kind not in IMAGE_KINDS:
        raise ValueError(f"image_finish: kind must be one of {', '.join(IMAGE_KINDS)}, got {kind!r}")
    tag, dtype = IMAGE_KINDS[kind]
    if img.dtype != torch.float16:
        raise TypeError(f"image_finish: img must be fp16, got {img.dtype}")
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[0] < 1:
        raise ValueError(f"image_finish: img must be [n, 3, H, W], got {tuple(img.shape)}")
    if not img.is_contiguous():
        raise ValueError(f"image_finish: img must be contiguous (channel-major), got strides {img.stride()}")
    n, _, H, W = (int(v) for v in img.shape)
    if H < 8 or W < 8 or H % 8 or W % 8:
        raise ValueError(f"image_finish: {H}x{W}: both sides must be multiples of 8 (one lane owns 8 pixels of a row)")
    shape = (n, H, W, 3)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=img.device)
    # written through the raw pointer as a dense [n, H, W, 3] array of `dtype`: anything else would be a foreign or
    # out-of-bounds write, so it is refused before any launch (ops._check_out's rule, for this entry's two dtypes)
    if not torch.is_tensor(out) or out.dtype != dtype:
        raise TypeError(f"image_finish: out must be {dtype} for kind={kind!r}, got {out.dtype if torch.is_tensor(out) else type(out).__name__}")
    if out.device != img.device:
        raise ValueError(f"image_finish: out is on {out.device}, img on {img.device}")
    if tuple(out.shape) != shape:
        raise ValueError(f"image_finish: out has shape {tuple(out.shape)}, the kernel writes {shape}")
    if not out.is_contiguous():
        raise ValueError(f"image_finish: out must be contiguous, got strides {out.stride()}")
    if img.data_ptr() % 16 or out.data_ptr() % (8 if kind == "uint8" else 16):
        raise ValueError("image_finish: img must be 16-byte aligned, out 8-byte (uint8) / 16-byte (float32) aligned")
    rc = _lib.load_library().dsc_image_finish(ops._p(img), ops._p(out), n, H, W, tag, ops._stream_ptr(img))
    _lib.check(rc, "dsc_image_finish")
    return out
