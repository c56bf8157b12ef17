"""Per-call cost from Python of ops.image_finish (dsc_image_finish) beside the eager chain it replaces on the device -
`(img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()` (decode_latents' tail, modules/model_k_diffusion.py) followed by
`.mul(255).round().to(torch.uint8)` (numpy_to_pil's line) - timed with device events on a warm device, alternating, at the image
sizes a served request has.  The kernel is timed per output kind and for both kinds back to back (what one captured decode of the
lane launches); the eager chain up to the float32 image and up to the bytes.  From Python both sides are bound by the host (a
launch costs more than the kernel runs), so each case is also captured into a graph of 20 calls and the replays timed: device us
per call, the figure the lane's captured decode pays.  The outputs are compared before anything is timed.  One JSON line per case.

    python tools/mb_image_finish.py [--iters 2000]
"""
import argparse
import json
import os
import sys

import torch

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


def graph_timed(fn, iters, calls=20):
    """device us per call: `calls` calls captured into one graph, `iters` replays between two events"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return timed(g.replay, iters) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    a = ap.parse_args()
    for n, side in [(1, 512), (4, 512), (1, 768), (4, 768)]:
        img = (1.5 * torch.randn(n, 3, side, side, generator=torch.Generator().manual_seed(side + n))).half().cuda()
        u8 = torch.empty(n, side, side, 3, dtype=torch.uint8, device="cuda")
        f32 = torch.empty(n, side, side, 3, dtype=torch.float32, device="cuda")

        def eager_f32():
            return (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()

        def eager_u8():
            return eager_f32().mul(255).round().to(torch.uint8)

        cases = {"kernel_uint8_us": lambda: ops.image_finish(img, "uint8", out=u8),
                 "kernel_float32_us": lambda: ops.image_finish(img, "float32", out=f32),
                 "kernel_both_us": lambda: (ops.image_finish(img, "uint8", out=u8), ops.image_finish(img, "float32", out=f32)),
                 "eager_float32_us": eager_f32, "eager_uint8_us": eager_u8}
        for fn in cases.values():                                 # warm-up: code objects, the allocator
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(u8, eager_u8())) and bool(torch.equal(f32, eager_f32().contiguous()))
        runs = [{k: timed(fn, a.iters) for k, fn in cases.items()} for _ in range(3)]            # alternating
        graphs = [{k: graph_timed(fn, max(a.iters // 20, 10)) for k, fn in cases.items()} for _ in range(3)]
        bytes_u8, bytes_f32 = img.numel() * 2 + u8.numel(), img.numel() * 2 + f32.numel() * 4
        best = {k: min(r[k] for r in graphs) for k in cases}
        print(json.dumps({"n": n, "H": side, "W": side, "equal_to_eager": same,
                          **{k: [round(r[k], 2) for r in runs] for k in cases},
                          **{"graph_" + k: [round(r[k], 2) for r in graphs] for k in cases},
                          "kernel_uint8_bytes": bytes_u8, "kernel_float32_bytes": bytes_f32,
                          "kernel_uint8_GBps_at_best": round(bytes_u8 / best["kernel_uint8_us"] / 1e3, 1),
                          "kernel_float32_GBps_at_best": round(bytes_f32 / best["kernel_float32_us"] / 1e3, 1),
                          "note": "us per call from device events, three alternating rounds: plain keys over back-to-back calls from "
                                  "Python (host work and launch cost included: they bound the rate), graph_ keys over replays of a graph of "
                                  "20 calls (device time; GB/s from the fastest of these); bytes = the fp16 input read once + the output "
                                  "written once; the buffers are re-read by every call, so small cases run from the caches"}), flush=True)


if __name__ == "__main__":
    main()
