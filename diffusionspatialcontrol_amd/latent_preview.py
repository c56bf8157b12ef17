"""ops.latent_preview: the wrapper of dsc_latent_preview (csrc/latent_preview.hip), the launch that turns up to 16 fp16 latent
rows into approximate uint8 RGB thumbnails (the preview path of modules/serving/), `latent_preview_numpy`, the same arithmetic
restated in numpy float32 for tests and tools, and `LATENT_RGB_SD15`, the default coefficients."""
import ctypes

import numpy as np
import torch

from . import _lib

PREVIEW_MAX_ROWS, PREVIEW_MAX_CHANNELS = 16, 8       # DSC_PREVIEW_MAX_ROWS / DSC_PREVIEW_MAX_CHANNELS (include/dsc_hip.h)
PREVIEW_SCALES = (1, 2, 4, 8)

# k[c][rgb] then bias[rgb]: the widely used linear approximation of the SD 1.x VAE decoder on the sampler's scaled latents
LATENT_RGB_SD15 = ((0.298, 0.207, 0.208), (0.187, 0.286, 0.173), (-0.158, 0.189, 0.264), (-0.184, -0.271, -0.473),
                   (0.0, 0.0, 0.0))


def _ops():
    from . import ops                    # (ops re-exports this module's functions: resolved at call time)
    return ops


def preview_coef(coef, C):
    """`coef` (None: LATENT_RGB_SD15; else C * 3 + 3 numbers in any nesting, k[c][rgb] row-major then bias[rgb]) -> a flat
    float32 array of C * 3 + 3"""
    flat = np.asarray(LATENT_RGB_SD15 if coef is None else coef, dtype=np.float32).reshape(-1)
    if flat.size != 3 * C + 3:
        raise ValueError(f"latent_preview: coef must hold C * 3 + 3 = {3 * C + 3} numbers (k[c][rgb], then bias[rgb]) for C = {C} "
                         f"channels, got {flat.size}")
    return np.ascontiguousarray(flat)


def latent_preview_numpy(lat_rows, coef, up):
    """dsc_latent_preview's arithmetic on the CPU, op by op in float32: lat_rows [n, C, h, w] (fp16 values: a tensor or an array)
    -> np.uint8 [n, h * up, w * up, 3]"""
    if up not in PREVIEW_SCALES:
        raise ValueError(f"latent_preview: up must be one of {PREVIEW_SCALES}, got {up!r}")
    if torch.is_tensor(lat_rows):
        lat_rows = lat_rows.detach().cpu().numpy()
    z = np.asarray(lat_rows).astype(np.float16).astype(np.float32)
    if z.ndim != 4:
        raise ValueError(f"latent_preview: lat_rows must be [n, C, h, w], got {z.shape}")
    n, C, h, w = z.shape
    flat = preview_coef(coef, C)
    k, bias = flat[:3 * C].reshape(C, 3), flat[3 * C:]
    half, one, zero = np.float32(0.5), np.float32(1.0), np.float32(0.0)
    v = np.broadcast_to(bias, (n, h, w, 3)).astype(np.float32)
    for c in range(C):
        v = v + k[c] * z[:, c, :, :, None]                   # one float32 product, one float32 sum
    y = v * half + half
    y = np.where(y > zero, y, zero)                          # (a NaN compares false: 0)
    y = np.where(y < one, y, one)
    out = np.rint(y * np.float32(255.0)).astype(np.uint8)
    return np.ascontiguousarray(out.repeat(up, axis=1).repeat(up, axis=2))


def latent_preview(lat, rows, coef=None, up=1, out=None):
    """lat [R, C, h, w] fp16 on the GPU, every row dense (the row stride may be larger than C * h * w); rows: up to 16 row
    indices, in any order; coef: C * 3 + 3 numbers (None: LATENT_RGB_SD15, for C = 4) -> uint8 [len(rows), h * up, w * up, 3],
    thumbnail j showing row rows[j], in one launch on the current stream (dsc_latent_preview).  up in {1, 2, 4, 8} with
    (w * up) % 8 == 0.  out: None (a new tensor) or a contiguous uint8 tensor of that shape on lat's device, written through its
    raw pointer.  Returns out."""
    ops = _ops()
    ops._require_gpu(lat)
    if lat.dtype != torch.float16:
        raise TypeError(f"latent_preview: lat must be fp16, got {lat.dtype}")
    if lat.dim() != 4 or lat.shape[0] < 1:
        raise ValueError(f"latent_preview: lat must be [R, C, h, w], got {tuple(lat.shape)}")
    R, C, h, w = (int(v) for v in lat.shape)
    if not 1 <= C <= PREVIEW_MAX_CHANNELS:
        raise ValueError(f"latent_preview: 1 to {PREVIEW_MAX_CHANNELS} channels, got {C}")
    if not lat[0].is_contiguous() or (R > 1 and lat.stride(0) < C * h * w):
        raise ValueError(f"latent_preview: every row of lat must be dense [C, h, w], got strides {lat.stride()}")
    if up not in PREVIEW_SCALES:
        raise ValueError(f"latent_preview: up must be one of {PREVIEW_SCALES}, got {up!r}")
    if (w * up) % 8:
        raise ValueError(f"latent_preview: width {w} * up {up} must be a multiple of 8 (one lane owns 8 pixels of an output row)")
    rows = [int(r) for r in rows]
    if not 1 <= len(rows) <= PREVIEW_MAX_ROWS or any(not 0 <= r < R for r in rows):
        raise ValueError(f"latent_preview: rows must be 1 to {PREVIEW_MAX_ROWS} indices in [0, {R}), got {rows}")
    flat = preview_coef(coef, C)
    n, stride = len(rows), int(lat.stride(0)) if R > 1 else C * h * w
    shape = (n, h * up, w * up, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=lat.device)
    # written through the raw pointer as a dense uint8 [n, h * up, w * up, 3] array: anything else would be a foreign or
    # out-of-bounds write, so it is refused before any launch
    if not torch.is_tensor(out) or out.dtype != torch.uint8:
        raise TypeError(f"latent_preview: out must be uint8, got {out.dtype if torch.is_tensor(out) else type(out).__name__}")
    if out.device != lat.device:
        raise ValueError(f"latent_preview: out is on {out.device}, lat on {lat.device}")
    if tuple(out.shape) != shape:
        raise ValueError(f"latent_preview: out has shape {tuple(out.shape)}, the kernel writes {shape}")
    if not out.is_contiguous():
        raise ValueError(f"latent_preview: out must be contiguous, got strides {out.stride()}")
    piece = 8 // up
    if lat.data_ptr() % (2 * piece) or stride % piece or out.data_ptr() % 8:
        raise ValueError(f"latent_preview: lat must be {2 * piece}-byte aligned with a row stride that is a multiple of {piece} "
                         f"halfs (up = {up}), out 8-byte aligned")
    rc = _lib.load_library().dsc_latent_preview(ops._p(lat), stride, (ctypes.c_int * n)(*rows), n, C, h, w,
                                                flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), up, ops._p(out),
                                                ops._stream_ptr(lat))
    _lib.check(rc, "dsc_latent_preview")
    return out
