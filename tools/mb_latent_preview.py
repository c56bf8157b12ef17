"""Per-call cost from Python of ops.latent_preview (dsc_latent_preview) beside the eager chain it replaces on the device - index
the rows, `einsum` with the [C, 3] matrix, add the bias, `/ 2 + 0.5`, clamp, `* 255`, round, cast to uint8 (NHWC) and, for
up > 1, `repeat_interleave` along both image axes - timed with device events on a warm device, alternating, for 1, 4 and 8 rows
of 64 x 64 and 96 x 96 latents at up = 1 and 8.  From Python both sides are bound by the host (a launch costs more than the kernel
runs), so each case is also captured into a graph of 20 calls and the replays timed: device us per call.  The eager chain runs
in float32 without the kernel's pinned rounding, so the outputs are compared to within one grey level before anything is timed
(the bit-exact reference is ops.latent_preview_numpy, on the CPU).  One JSON line per case.

    python tools/mb_latent_preview.py [--iters 2000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionspatialcontrol_amd import ops  # noqa: E402
from mb_image_finish import graph_timed, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    a = ap.parse_args()
    flat = np.asarray(ops.LATENT_RGB_SD15, dtype=np.float32).reshape(-1)
    k, bias = torch.from_numpy(flat[:12].reshape(4, 3)).cuda(), torch.from_numpy(flat[12:]).cuda()
    for side in (64, 96):
        for n in (1, 4, 8):
            for up in (1, 8):
                old = (1.5 * torch.randn(8, 4, side, side, generator=torch.Generator().manual_seed(side + n))).half().cuda()
                rows = list(range(8))[::-1][:n]
                idx = torch.tensor(rows, device="cuda")
                out = torch.empty(n, side * up, side * up, 3, dtype=torch.uint8, device="cuda")

                def eager():
                    v = torch.einsum("nchw,cq->nhwq", old[idx].float(), k) + bias
                    b = (v / 2 + 0.5).clamp(0, 1).mul(255).round().to(torch.uint8)
                    return b if up == 1 else b.repeat_interleave(up, 1).repeat_interleave(up, 2)

                cases = {"kernel_us": lambda: ops.latent_preview(old, rows, flat, up, out=out), "eager_us": eager}
                for fn in cases.values():                             # warm-up: code objects, the allocator
                    for _ in range(50):
                        fn()
                torch.cuda.synchronize()
                exact = bool(np.array_equal(out.cpu().numpy(), ops.latent_preview_numpy(old[idx].cpu(), flat, up)))
                near = int((out.int() - eager().int()).abs().max())
                runs = [{key: timed(fn, a.iters) for key, fn in cases.items()} for _ in range(3)]            # alternating
                graphs = [{key: graph_timed(fn, max(a.iters // 20, 10)) for key, fn in cases.items()} for _ in range(3)]
                moved = n * 4 * side * side * 2 + out.numel()
                print(json.dumps({"rows": n, "h": side, "w": side, "up": up, "equal_to_numpy": exact, "max_levels_from_eager": near,
                                  **{key: [round(r[key], 2) for r in runs] for key in cases},
                                  **{"graph_" + key: [round(r[key], 2) for r in graphs] for key in cases},
                                  "kernel_bytes": moved,
                                  "kernel_GBps_at_best": round(moved / min(r["kernel_us"] for r in graphs) / 1e3, 1),
                                  "note": "us per call from device events, three alternating rounds: plain keys over back-to-back "
                                          "calls from Python (host work and launch cost included), graph_ keys over replays of a "
                                          "graph of 20 calls (device time); bytes = the fp16 rows read once + the thumbnails written "
                                          "once; the eager chain has no blocking copy here, the served path it replaces would add one"}),
                      flush=True)


if __name__ == "__main__":
    main()
