"""ops.image_prepare / ops.latent_start: the wrappers of dsc_image_prepare and dsc_latent_start_rows (csrc/image_prepare.hip), the
two launches around the VAE encoder's captured graph on the encode lane of the continuous batcher (modules/serving/), and
`image_prepare_torch` / `latent_start_torch`, the literal eager chains they replace, for tests and tools."""
import ctypes

import torch

from . import _lib

MAX_ROWS = 16                                    # DSC_IMAGE_PREPARE_MAX_ROWS (include/dsc_hip.h)
PIXEL_KINDS = {torch.uint8: 0, torch.float32: 1}                 # DSC_PIXELS_U8 / DSC_PIXELS_F32
START_KINDS = {"add": 1, "scale": 2, "none": 3}                  # DSC_START_ADD / _SCALE / _NONE (0: an idle row)
REQUEST_KINDS = ("img2img", "inpaint", "inpaint_max", "masked")  # what a row of the encode lane is, see start_form


def _ops():
    from . import ops                    # (ops re-exports this module's functions: resolved at call time)
    return ops


# ---------------------------------------------------------------------- the eager chains
def image_prepare_torch(image, mask=None, rep=1):
    """The eager chain dsc_image_prepare replaces, on any device.  image: uint8 [H, W, 3] (the bytes of a PIL image) or float32
    [3, H, W] in [-1, 1]; mask: None, uint8 [H, W] or float32 [H, W] -> (fp16 [3, H, W] image, fp16 [3, H, W] masked image or
    None, fp16 [rep, H / 8, W / 8] latent mask or None): `_image_tensor`'s `2.0 * (bytes.float32 / 255.0) - 1.0` and `>= 0.5`,
    inpaiting's `init * (mask < 0.5)`, the VAE's `.to(fp16)` and `F.interpolate(mask, size=(h, w))` (nearest)."""
    if image.dtype == torch.uint8:
        init = 2.0 * (image.to(torch.float32) / 255.0).permute(2, 0, 1) - 1.0
    else:
        init = image.to(torch.float32)
    H, W = (int(v) for v in init.shape[-2:])
    if mask is None:
        return init.to(torch.float16), None, None
    m = mask.to(torch.float32) / 255.0 if mask.dtype == torch.uint8 else mask.to(torch.float32)
    m = (m >= 0.5).float()[None, None]
    masked = (init[None] * (m < 0.5))[0].to(torch.float16)
    small = torch.nn.functional.interpolate(m, size=(H // 8, W // 8)).to(torch.float16)
    return init.to(torch.float16), masked, small[0].expand(rep, H // 8, W // 8).contiguous()


def start_form(kind, sigma0, given_latents=False):
    """which arithmetic a lane row's start latent has, and its scalar, without touching the device -> (form, coef):
    "img2img"     lat + noise * (sig[0] ** 2 + 1) ** 0.5 on the fp16 0-dim tensor: every op of the coefficient rounds to fp16,
                  and the product with a 0-dim fp16 tensor is an fp16 tensor op -> ("add", that fp16 value)
    "inpaint"     add_noise's `image_latents + sigma * noise` with the fp16 0-dim sigma -> ("add", sigma_0)
    "inpaint_max" (or any inpainting request with `latents` given) `noise * (sigma.item() ** 2 + 1) ** 0.5`: a PYTHON float, which
                  torch multiplies into an fp16 tensor as an fp32 scalar -> ("scale", fp32 of the double-precision root)
    "masked"      the masked image of a 9-channel request: no start latent -> ("none", 0)"""
    s = torch.as_tensor(sigma0).detach().to("cpu", torch.float16).reshape(())
    if kind == "masked":
        return "none", 0.0
    if kind == "img2img":
        return "add", float((s ** 2 + 1) ** 0.5)
    if kind == "inpaint_max" or (kind == "inpaint" and given_latents):
        return "scale", float(torch.tensor((s.item() ** 2 + 1) ** 0.5, dtype=torch.float32))
    if kind == "inpaint":
        return "add", float(s)
    raise ValueError(f"latent_start: kind must be one of {', '.join(REQUEST_KINDS)}, got {kind!r}")


def latent_start_torch(moments, eps, noise, scaling, kind, sigma0):
    """The eager chain dsc_latent_start_rows replaces for ONE row, on any device.  moments fp16 [1, 8, h, w]
    (`latent_dist.parameters`), eps / noise fp16 [1, 4, h, w] (noise: None for "masked"), sigma0 the fp16 0-dim first sigma ->
    (latents, start latent or None): DiagonalGaussianDistribution's clamp / exp / sample, `_encode_vae_image`'s product, then
    prepare_image's or prepare_latents_inpating's line for `kind` (REQUEST_KINDS)."""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    lat = scaling * (mean + std * eps)
    if kind == "masked":
        return lat, None
    if kind == "img2img":
        return lat, lat + noise * (sigma0 ** 2 + 1) ** 0.5
    if kind == "inpaint":
        return lat, lat + sigma0 * noise
    if kind == "inpaint_max":
        return lat, noise * (sigma0.item() ** 2 + 1) ** 0.5
    raise ValueError(f"latent_start: kind must be one of {', '.join(REQUEST_KINDS)}, got {kind!r}")


# ---------------------------------------------------------------------- argument checks
def _dense(t, what, dtypes, shape, device, align=16):
    """`t` is read or written through its raw pointer as a dense `shape` array: dtype, shape, contiguity, device and alignment"""
    if not torch.is_tensor(t) or t.dtype not in dtypes:
        names = " / ".join(str(d) for d in dtypes)
        raise TypeError(f"{what} must be {names}, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} has shape {tuple(t.shape)}, the kernel takes {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous, got strides {t.stride()}")
    if t.device != device:
        raise ValueError(f"{what} is on {t.device}, the launch runs on {device}")
    if t.data_ptr() % align:
        raise ValueError(f"{what} must be {align}-byte aligned")


def _device_of(rows, keys, what):
    for row in rows:
        for k in keys:
            if row is not None and torch.is_tensor(row.get(k)):
                _ops()._require_gpu(row[k])
                return row[k].device
    raise ValueError(f"{what}: no row names a tensor")


def image_prepare(rows, H, W):
    """Up to 16 request images -> what `vae.encode` and the sampler step read, in ONE launch on the current stream
    (dsc_image_prepare).  rows: a list with, per row, None (idle: neither read nor written) or a dict of
        image       uint8 [H, W, 3] or float32 [3, H, W] in [-1, 1]
        mask        uint8 [H, W] or float32 [H, W] (optional)
        out_image   fp16 [3, H, W]                 <- the image, rounded once
        out_masked  fp16 [3, H, W]                 <- init * (mask < 0.5), the fp32 product rounded once (needs mask)
        out_mask    fp16 [rep, H / 8, W / 8]       <- the mask binarised at 0.5 at pixel (8 i, 8 j), rep (1 or 4) times (needs mask)
    every destination optional.  All tensors contiguous, on one GPU, 16-byte aligned (out_mask: 2-byte); H and W multiples of 8."""
    if not isinstance(rows, (list, tuple)) or not 1 <= len(rows) <= MAX_ROWS:
        raise ValueError(f"image_prepare: rows must be a list of 1 to {MAX_ROWS} rows, got "
                         f"{len(rows) if isinstance(rows, (list, tuple)) else type(rows).__name__}")
    if isinstance(H, bool) or isinstance(W, bool) or not isinstance(H, int) or not isinstance(W, int) or H < 8 or W < 8 or H % 8 or W % 8:
        raise ValueError(f"image_prepare: {H}x{W}: both sides must be multiples of 8")
    dev = _device_of(rows, ("image", "mask", "out_image", "out_masked", "out_mask"), "image_prepare")
    recs = (_lib.ImagePrepareRow * len(rows))()
    for j, row in enumerate(rows):
        if row is None:
            continue
        unknown = set(row) - {"image", "mask", "out_image", "out_masked", "out_mask"}
        if unknown:
            raise ValueError(f"image_prepare: row {j} has unknown keys {sorted(unknown)}")
        image, mask = row.get("image"), row.get("mask")
        o_img, o_masked, o_mask = row.get("out_image"), row.get("out_masked"), row.get("out_mask")
        rec = recs[j]
        if o_img is not None or o_masked is not None:
            if image is None:
                raise ValueError(f"image_prepare: row {j} asks for an image output without `image`")
            _dense(image, f"image_prepare: row {j}: image", (torch.uint8, torch.float32),
                   (H, W, 3) if torch.is_tensor(image) and image.dtype == torch.uint8 else (3, H, W), dev)
            rec.image, rec.image_kind = image.data_ptr(), PIXEL_KINDS[image.dtype]
        if o_masked is not None or o_mask is not None:
            if mask is None:
                raise ValueError(f"image_prepare: row {j} asks for a mask output without `mask`")
            _dense(mask, f"image_prepare: row {j}: mask", (torch.uint8, torch.float32), (H, W), dev)
            rec.mask, rec.mask_kind = mask.data_ptr(), PIXEL_KINDS[mask.dtype]
        for name, t in (("out_image", o_img), ("out_masked", o_masked)):
            if t is not None:
                _dense(t, f"image_prepare: row {j}: {name}", (torch.float16,), (3, H, W), dev)
                setattr(rec, name, t.data_ptr())
        if o_img is not None and o_masked is not None and o_img.data_ptr() == o_masked.data_ptr():
            raise ValueError(f"image_prepare: row {j}: out_image and out_masked are one tensor")
        if o_mask is not None:
            if not torch.is_tensor(o_mask) or o_mask.dim() != 3 or o_mask.shape[0] not in (1, 4):
                raise ValueError(f"image_prepare: row {j}: out_mask must be [1 or 4, {H // 8}, {W // 8}], got "
                                 f"{tuple(o_mask.shape) if torch.is_tensor(o_mask) else type(o_mask).__name__}")
            _dense(o_mask, f"image_prepare: row {j}: out_mask", (torch.float16,), (int(o_mask.shape[0]), H // 8, W // 8), dev, align=2)
            rec.out_mask, rec.mask_rep = o_mask.data_ptr(), int(o_mask.shape[0])
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load_library().dsc_image_prepare(recs, len(rows), H, W, stream), "dsc_image_prepare")


def latent_start(moments, rows):
    """After the encode, every row of it in ONE launch on the current stream (dsc_latent_start_rows).  moments: fp16
    [m, 8, h, w] contiguous (`vae.encode(x).latent_dist.parameters`).  rows: a list with, per row, None (idle) or a dict of
        form        "add" (start = lat + noise * coef), "scale" (start = noise * coef) or "none" (no start latent): start_form
        row         which row of `moments` it reads
        eps, noise  fp16 [4, h, w]: the posterior draw and the noise (noise: not for "none")
        scaling     the VAE's scaling factor;   coef: the scalar of `form`
        start       fp16 [4, h, w] <- the start latent (not for "none")
        keep        fp16 [4, h, w] <- the latents `scaling * (mean + std * eps)` (optional; "none" needs it)
        keep_noise  fp16 [4, h, w] <- the noise row (optional)
    [4, h, w] may also be given as [1, 4, h, w].  All tensors contiguous, on moments' GPU."""
    ops = _ops()
    ops._require_gpu(moments)
    if moments.dtype != torch.float16:
        raise TypeError(f"latent_start: moments must be fp16, got {moments.dtype}")
    if moments.dim() != 4 or moments.shape[1] != 8 or moments.shape[0] < 1:
        raise ValueError(f"latent_start: moments must be [m, 8, h, w], got {tuple(moments.shape)}")
    if not moments.is_contiguous():
        raise ValueError(f"latent_start: moments must be contiguous, got strides {moments.stride()}")
    if not isinstance(rows, (list, tuple)) or not 1 <= len(rows) <= MAX_ROWS:
        raise ValueError(f"latent_start: rows must be a list of 1 to {MAX_ROWS} rows, got "
                         f"{len(rows) if isinstance(rows, (list, tuple)) else type(rows).__name__}")
    m, _, h, w = (int(v) for v in moments.shape)
    dev = moments.device
    recs = (_lib.LatentStartRow * len(rows))()
    for j, row in enumerate(rows):
        if row is None:
            continue
        unknown = set(row) - {"form", "row", "eps", "noise", "scaling", "coef", "start", "keep", "keep_noise"}
        if unknown:
            raise ValueError(f"latent_start: row {j} has unknown keys {sorted(unknown)}")
        form = row.get("form")
        if form not in START_KINDS:
            raise ValueError(f"latent_start: row {j}: form must be one of {', '.join(START_KINDS)}, got {form!r}")
        k = row.get("row")
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < m:
            raise ValueError(f"latent_start: row {j} reads row {k!r} of moments, which has {m}")
        needed = ("eps",) + (("keep",) if form == "none" else ("noise", "start"))
        if form == "none" and (row.get("noise") is not None or row.get("start") is not None or row.get("keep_noise") is not None):
            raise ValueError(f"latent_start: row {j}: form 'none' takes no noise, start or keep_noise")
        rec = recs[j]
        seen = {}
        for name in ("eps", "noise", "start", "keep", "keep_noise"):
            t = row.get(name)
            if t is None:
                if name in needed:
                    raise ValueError(f"latent_start: row {j} (form {form!r}) needs `{name}`")
                continue
            shape = (1, 4, h, w) if torch.is_tensor(t) and t.dim() == 4 else (4, h, w)
            _dense(t, f"latent_start: row {j}: {name}", (torch.float16,), shape, dev, align=2)
            if name in ("start", "keep", "keep_noise"):
                if t.data_ptr() in seen:
                    raise ValueError(f"latent_start: row {j}: {name} and {seen[t.data_ptr()]} are one tensor")
                seen[t.data_ptr()] = name
            setattr(rec, name, t.data_ptr())
        rec.kind, rec.moments_row = START_KINDS[form], k
        rec.scaling, rec.coef = float(row.get("scaling", 1.0)), float(row.get("coef", 0.0))
    _lib.check(_lib.load_library().dsc_latent_start_rows(ops._p(moments), m, recs, len(rows), h, w, ops._stream_ptr(moments)),
               "dsc_latent_start_rows")
