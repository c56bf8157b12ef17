"""Per-call cost from Python of ops.latent_resample_noise (dsc_latent_resample_noise) beside the eager route it replaces - F.interpolate on an fp32 copy, the conversion back to fp16, the
multiply of the noise and the add (modules/model_k_diffusion.py _hires_pass + img2img) - timed with device events on a warm
device, alternating, at the sizes a served hires request has (one latent row 4 x 64 x 64 and up).  One JSON line per case.

    python tools/mb_latent_resample.py [--iters 2000]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionspatialcontrol_amd import ops  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters                  # us per call, launches back to back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    a = ap.parse_args()
    sigma = 2.37109375
    for n, (h, w), (H, W), mode, aa in [(1, (64, 64), (76, 76), "bicubic", False), (1, (64, 64), (76, 71), "bicubic", False),
                                        (1, (64, 64), (128, 128), "bicubic", False), (1, (64, 64), (76, 76), "bicubic", True),
                                        (1, (64, 64), (76, 76), "bilinear", False), (1, (64, 64), (76, 76), "nearest-exact", False),
                                        (1, (128, 128), (256, 256), "bicubic", False), (8, (64, 64), (76, 76), "bicubic", False)]:
        g = torch.Generator().manual_seed(0)
        src = torch.randn(n, 4, h, w, generator=g).half().cuda()
        noise = torch.randn(n, 4, H, W, generator=g).half().cuda()
        out = torch.empty_like(noise)
        sig16 = torch.tensor(sigma, dtype=torch.float16, device="cuda")
        kw = {"antialias": aa} if mode in ("bilinear", "bicubic") else {}

        def kernel():
            ops.latent_resample_noise(src, (H, W), mode, aa, noise=noise, sigma0=sigma, out=out)

        def eager():
            lat = F.interpolate(src.float(), size=(H, W), mode=mode, **kw).to(src.dtype)
            return lat + noise * (sig16 ** 2 + 1) ** 0.5

        for fn in (kernel, eager):                            # warm-up: code objects, the tap tables, the allocator
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        runs = [(timed(kernel, a.iters), timed(eager, a.iters)) for _ in range(3)]            # alternating
        print(json.dumps({"n": n, "src": [h, w], "dst": [H, W], "mode": mode, "antialias": aa,
                          "op_call_us": [round(k, 2) for k, _ in runs], "eager_route_us": [round(e, 2) for _, e in runs],
                          "note": "us per call from device events over back-to-back calls from Python (the wrapper's host work "
                                  "and launch cost included where they bound the rate); eager = interpolate(fp32 copy) + "
                                  ".to(fp16) + noise * s + add"}), flush=True)


if __name__ == "__main__":
    main()
