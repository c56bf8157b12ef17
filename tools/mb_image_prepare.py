"""Per-call cost from Python and device time of ops.image_prepare (dsc_image_prepare) and ops.latent_start
(dsc_latent_start_rows) beside the eager chains they replace on the device (ops.image_prepare_torch per image - the division,
`2 x - 1`, the permute, the mask's threshold, the product, the nearest interpolation, the conversions to fp16 - and
ops.latent_start_torch per row - DiagonalGaussianDistribution's clamp / exp / sample, the scaling, the start latent), for 1 - 4
rows at 512x512 and 768x768.  Timed with device events on a warm device, alternating: plain keys over back-to-back calls from Python
(bound by the host: a launch costs more than these kernels run), graph_ keys over replays of a graph of 20 calls (device time).
The outputs are compared before anything is timed.  One JSON line per case.

    python tools/mb_image_prepare.py [--iters 1000]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionspatialcontrol_amd import ops  # noqa: E402
from mb_image_finish import graph_timed, timed  # noqa: E402


def _bits(t):
    return t.contiguous().view(torch.int16)


def prepare_case(n, side):
    g = torch.Generator().manual_seed(side + n)
    imgs = [torch.randint(0, 256, (side, side, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(n)]
    masks = [torch.randint(0, 256, (side, side), generator=g, dtype=torch.uint8).cuda() for _ in range(n)]
    x = torch.empty(2 * n, 3, side, side, dtype=torch.float16, device="cuda")
    lm = torch.empty(n, 1, side // 8, side // 8, dtype=torch.float16, device="cuda")
    rows = [{"image": imgs[j], "mask": masks[j], "out_image": x[2 * j], "out_masked": x[2 * j + 1], "out_mask": lm[j]}
            for j in range(n)]
    rows_img = [{"image": imgs[j], "out_image": x[2 * j]} for j in range(n)]

    def eager():
        return [ops.image_prepare_torch(imgs[j], masks[j], 1) for j in range(n)]

    def eager_img():
        return [ops.image_prepare_torch(imgs[j]) for j in range(n)]

    cases = {"kernel_inpaint_us": lambda: ops.image_prepare(rows, side, side),
             "kernel_image_us": lambda: ops.image_prepare(rows_img, side, side),
             "eager_inpaint_us": eager, "eager_image_us": eager_img}
    for fn in cases.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ops.image_prepare(rows, side, side)
    ref = eager()
    same = all(torch.equal(_bits(x[2 * j]), _bits(ref[j][0])) and torch.equal(_bits(x[2 * j + 1]), _bits(ref[j][1])) and
               torch.equal(lm[j], ref[j][2]) for j in range(n))
    read = n * (side * side * 4)
    written = n * (2 * 3 * side * side * 2 + side * side // 64 * 2)
    return cases, same, read + written


def start_case(n, side):
    h = side // 8
    g = torch.Generator().manual_seed(side + 7 * n)
    moments = torch.randn(n, 8, h, h, generator=g).half().cuda()
    eps, noise = (torch.randn(n, 4, h, h, generator=g).half().cuda() for _ in range(2))
    start, keep, keepn = (torch.empty(n, 4, h, h, dtype=torch.float16, device="cuda") for _ in range(3))
    sig0 = torch.tensor(3.3).half().cuda()
    form, coef = ops.start_form("inpaint", sig0)
    rows = [{"form": form, "row": j, "eps": eps[j], "noise": noise[j], "scaling": 0.18215, "coef": coef, "start": start[j],
             "keep": keep[j], "keep_noise": keepn[j]} for j in range(n)]

    def eager():
        out = []
        for j in range(n):
            lat, st = ops.latent_start_torch(moments[j:j + 1], eps[j:j + 1], noise[j:j + 1], 0.18215, "inpaint", sig0)
            out.append((lat[0].clone(), st, noise[j].clone()))                   # (the inline path clones the rows it keeps)
        return out

    cases = {"kernel_us": lambda: ops.latent_start(moments, rows), "eager_us": eager}
    for fn in cases.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    ref = eager()
    same = all(torch.equal(_bits(keep[j]), _bits(ref[j][0])) and torch.equal(_bits(start[j]), _bits(ref[j][1][0])) and
               torch.equal(keepn[j], noise[j]) for j in range(n))
    return cases, same, n * 4 * h * h * 2 * 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    a = ap.parse_args()
    for what, build in (("image_prepare", prepare_case), ("latent_start", start_case)):
        for side in (512, 768):
            for n in (1, 2, 3, 4):
                cases, same, nbytes = build(n, side)
                runs = [{k: timed(fn, a.iters) for k, fn in cases.items()} for _ in range(3)]            # alternating
                graphs = [{k: graph_timed(fn, max(a.iters // 20, 10)) for k, fn in cases.items()} for _ in range(3)]
                first = next(iter(cases))
                best = min(r[first] for r in graphs)
                print(json.dumps({"op": what, "rows": n, "H": side, "W": side, "equal_to_eager": bool(same),
                                  **{k: [round(r[k], 2) for r in runs] for k in cases},
                                  **{"graph_" + k: [round(r[k], 2) for r in graphs] for k in cases},
                                  "bytes": nbytes, first.replace("_us", "_GBps_at_best"): round(nbytes / best / 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
