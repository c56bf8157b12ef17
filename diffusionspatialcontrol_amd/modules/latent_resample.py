"""Tap tables of the hires pass's latent resample (reference model_k_diffusion.py:1179-1191: `F.interpolate` between the passes).

Every mode of `torch.nn.functional.interpolate` the reference's "Hires fix" tab offers - bilinear and bicubic (plain or antialiased),
nearest, nearest-exact, area - is separable and, when enlarging, touches at most four source samples per axis.  `resample_taps`
restates each as a table of (index, weight) x 4 per output coordinate, so ONE kernel (dsc_latent_resample_noise) serves them all
without knowing the mode.  The coordinates are computed in fp32, step by step as torch's kernels compute them
(aten/src/ATen/native/UpSample.h): the fp32 rounding of `scale` decides which sample a nearest mode picks, and the fp32
fraction is what its interpolation weights are made from.

Only n_out >= n_in (the app's factor range is 1.0 .. 2.0).
"""
import functools
import math

import numpy as np
import torch

MODES = ("bilinear", "bicubic", "nearest", "nearest-exact", "area")
_f = np.float32


def hires_target_size(height, width, upscale_x, vae_scale_factor=8):
    """(target_height, target_width) of the hires pass: the reference's expression (:1177-1178), as _hires_pass restates it"""
    return int(height * upscale_x // vae_scale_factor) * 8, int(width * upscale_x // vae_scale_factor) * 8


def _centre(scale, o):
    """scale * (o + 0.5) - 0.5 with ONE rounding: torch's compiled kernels contract the expression into an fma (seen in the
    weights F.interpolate gives a unit impulse: 64 -> 76, output 38)"""
    return _f(np.float64(scale) * np.float64(_f(o) + _f(0.5)) - 0.5)


def _fma(a, b, c):
    """fp32 fused multiply-add: the fp64 product of two fp32 numbers is exact, one rounding of the sum"""
    return _f(np.float64(a) * np.float64(b) + np.float64(c))


# The cubic convolution polynomials of UpSample.h, with the multiply-adds torch's compiled CPU kernels contract into fmas (found
# by comparing, bit for bit, with the weights F.interpolate gives unit impulses; the plain and the antialiased kernels were
# compiled to different contractions).  With these and the tap ORDER below, the fp32 value the kernel rounds to fp16 is the one
# torch rounds, bit for bit, for both bicubic modes - which is what keeps results that nearly cancel within one fp16 spacing.
def _conv1(x, A):                                   # |x| <= 1, plain bicubic
    return _fma(A + _f(2), x, -(A + _f(3))) * x * x + _f(1)


def _conv2(x, A):                                   # 1 < |x| < 2, plain bicubic
    q = _fma(_fma(A, x, -_f(5) * A), x, _f(8) * A)
    return q * x - _f(4) * A


def _conv_aa(x, A):                                 # the antialiased filter
    if x < 1:
        q = (A + _f(2)) * x - (A + _f(3))
        return _fma(q * x, x, _f(1))
    if x < 2:
        q = _fma(A * x - _f(5) * A, x, _f(8) * A)
        return _fma(q, x, -_f(4) * A)
    return _f(0)


def _taps_1d(n_in, n_out, mode, antialias):
    idx = np.zeros((n_out, 4), dtype=np.int32)
    w = np.zeros((n_out, 4), dtype=np.float32)
    scale = _f(n_in) / _f(n_out)                    # area_pixel_compute_scale<float> / compute_scales_value<float>
    for o in range(n_out):
        if mode in ("nearest", "nearest-exact"):
            if n_out == n_in:                       # nearest_idx's shortcuts (the fp32 product is not consulted)
                i = o
            elif mode == "nearest" and n_out == 2 * n_in:
                i = o >> 1
            else:
                off = _f(0.5) if mode == "nearest-exact" else _f(0)
                i = min(int(math.floor((_f(o) + off) * scale)), n_in - 1)
            idx[o], w[o, 0] = i, 1.0
        elif mode == "area":                        # adaptive_avg_pool2d's window: one or two samples when enlarging
            i0 = (o * n_in) // n_out
            i1 = -((-(o + 1) * n_in) // n_out)
            k = i1 - i0
            assert 1 <= k <= 2, (n_in, n_out, o)
            idx[o] = i0
            idx[o, :k] = np.arange(i0, i1)
            w[o, :k] = 1.0 / k
        elif mode == "bilinear" and not antialias:
            c = max(_centre(scale, o), _f(0))
            i0 = int(c)
            lam = min(max(c - _f(i0), _f(0)), _f(1))
            idx[o] = i0
            idx[o, 1] = min(i0 + 1, n_in - 1)
            w[o, 0], w[o, 1] = _f(1) - lam, lam
        elif mode == "bicubic" and not antialias:   # A = -0.75, clamped indices: weights pile onto the border sample
            c = _centre(scale, o)
            i0 = int(math.floor(c))
            t = c - _f(i0)
            A = _f(-0.75)
            x2 = _f(1) - t
            w[o] = (_conv2(t + _f(1), A), _conv1(t, A), _conv1(x2, A), _conv2(x2 + _f(1), A))
            idx[o] = np.clip(np.arange(i0 - 1, i0 + 3), 0, n_in - 1)
            # tap order = evaluation order: the kernel computes fma(v3, w3, fma(v2, w2, fma(v1, w1, v0 * w0))), torch's kernel
            # x0 * c0 + x1 * c1 + ... compiled to fma(x0, c0, x1 * c1) first: the second tap leads
            idx[o, :2], w[o, :2] = idx[o, 1::-1].copy(), w[o, 1::-1].copy()
        else:
            # antialiased (_compute_indices_weights_aa): a triangle of support 1 / a cubic with A = -0.5 of support 2 (the support
            # grows only when shrinking); taps outside the row are dropped and the rest renormalised.  Enlarging, the triangle
            # gives plain bilinear's two taps, from a centre rounded at another point: equal to the last fp32 bits
            A = _f(-0.5)
            center = scale * (_f(o) + _f(0.5))
            support = _f(1) if mode == "bilinear" else _f(2)
            xmin = max(int(center - support + _f(0.5)), 0)
            xsize = min(int(center + support + _f(0.5)), n_in) - xmin
            assert 1 <= xsize <= 4, (n_in, n_out, o)
            ws = []
            for j in range(xsize):
                x = abs(_f(j + xmin) - center + _f(0.5))
                if mode == "bilinear":
                    ws.append(_f(1) - x if x < 1 else _f(0))
                else:
                    ws.append(_conv_aa(x, A))
            total = _f(0)
            for v in ws:
                total = total + v
            idx[o] = xmin
            idx[o, :xsize] = np.arange(xmin, xmin + xsize)
            w[o, :xsize] = [v / total for v in ws]
    return idx, w


@functools.lru_cache(maxsize=None)
def _taps_cached(n_in, n_out, mode, antialias):
    idx, w = _taps_1d(n_in, n_out, mode, antialias)
    assert idx.min() >= 0 and idx.max() < n_in
    return torch.from_numpy(idx), torch.from_numpy(w)


def resample_taps(n_in, n_out, mode, antialias=False):
    """-> (idx int32 [n_out, 4], w float32 [n_out, 4]): per output coordinate along one axis up to four source indices and
    weights; unused taps have weight 0 and a valid index.  Cached per (n_in, n_out, mode, antialias): treat as read-only."""
    n_in, n_out = int(n_in), int(n_out)
    if mode not in MODES:
        raise ValueError(f"resample_taps: unknown mode {mode!r} (one of {', '.join(MODES)})")
    if n_in < 1 or n_out < n_in:
        raise ValueError(f"resample_taps: only enlarging is tabulated (n_out >= n_in >= 1), got {n_in} -> {n_out}")
    antialias = bool(antialias) and mode in ("bilinear", "bicubic")
    return _taps_cached(n_in, n_out, mode, antialias)


_DEVICE_TAPS = {}


def device_taps(n_in, n_out, mode, antialias, device):
    """the table on `device` (uploaded once per key; call it outside graph capture first - ServingBatcher.warm() does)"""
    device = torch.device(device)
    key = (int(n_in), int(n_out), mode, bool(antialias) and mode in ("bilinear", "bicubic"), device.type, device.index)
    hit = _DEVICE_TAPS.get(key)
    if hit is None:
        idx, w = resample_taps(n_in, n_out, mode, antialias)
        hit = (idx.to(device).contiguous(), w.to(device).contiguous())
        _DEVICE_TAPS[key] = hit
    return hit


def noise_scale_f16(sigma0):
    """fp16( (sigma_0 ** 2 + 1) ** 0.5 ) with img2img's own roundings (modules/model_k_diffusion.py: the expression on the fp16
    0-dim `sigma_sched[0]`: the square, the sum and the root each round to fp16), as a Python float, without touching the device"""
    s = torch.as_tensor(sigma0).detach().to("cpu", torch.float16).reshape(())
    return float((s ** 2 + 1) ** 0.5)


def latent_resample_noise(src, size, mode, antialias=False, noise=None, sigma0=None, out=None):
    """The hires pass's start latent in one launch (dsc_latent_resample_noise): `F.interpolate(src.float(), size, mode
    [, antialias]).to(fp16)` and, with `noise` ([n, C, H, W] fp16 unit noise) and `sigma0` (the second pass's first sigma, a
    number), img2img's `+ noise * (sigma0 ** 2 + 1) ** 0.5` with its fp16 roundings.  src [n, C, h, w] fp16 contiguous on the GPU;
    size = (H, W) >= (h, w); mode one of MODES.  The tap tables are cached on the device per size pair."""
    from .. import _lib, ops                       # (ops re-exports this function: no import of it at module level)
    ops._require_gpu(src, noise, out)
    if src.dtype != torch.float16 or src.dim() != 4:
        raise TypeError(f"latent_resample_noise: src must be a 4-D fp16 tensor, got {src.dtype} {tuple(src.shape)}")
    if not src.is_contiguous():
        raise ValueError("latent_resample_noise: src must be contiguous (NCHW rows)")
    n, C, h, w = (int(v) for v in src.shape)
    H, W = (int(v) for v in size)
    if H < h or W < w:
        raise ValueError(f"latent_resample_noise: only enlarging is supported, {(h, w)} -> {(H, W)}")
    if (noise is None) != (sigma0 is None):
        raise ValueError("latent_resample_noise: `noise` and `sigma0` go together")
    shape = (n, C, H, W)
    if noise is not None:
        if noise.dtype != torch.float16:
            raise TypeError(f"latent_resample_noise: noise must be fp16, got {noise.dtype}")
        if noise.device != src.device or tuple(noise.shape) != shape or not noise.is_contiguous():
            raise ValueError(f"latent_resample_noise: noise must be a contiguous {shape} tensor on {src.device}, got "
                             f"{tuple(noise.shape)} on {noise.device}")
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=src.device)
    ops._check_out(out, shape, src, "latent_resample_noise")
    if not out.is_contiguous():
        raise ValueError("latent_resample_noise: out must be contiguous")
    if out.untyped_storage().data_ptr() == src.untyped_storage().data_ptr():
        raise ValueError("latent_resample_noise: out must not share src's storage")
    iy, wy = device_taps(h, H, mode, antialias, src.device)
    ix, wx = device_taps(w, W, mode, antialias, src.device)
    s = noise_scale_f16(sigma0) if noise is not None else 0.0
    ops._drop_gn_partials(out)
    p = ops._p
    rc = _lib.load_library().dsc_latent_resample_noise(p(src), p(noise), p(out), n, C, h, w, H, W, p(iy), p(wy), p(ix), p(wx), s,
                                                       ops._stream_ptr(src))
    _lib.check(rc, "dsc_latent_resample_noise")
    return out
