"""ops.add_rows_gated (dsc_add_rows_gated_f16) beside the eager pair it replaces - `v * gate` and `x + extra`, what txt2img's own
captured adapter step runs per down block with one scalar gate - at the four SD1.5 level shapes (320x64x64, 640x32x32,
1280x16x16, 1280x8x8) with 2, 4 and 16 batch rows, gates all on and every other row off.  One JSON line per case.

Every leg is captured into a graph of --calls launches and the graph is replayed (device events around the replays): device time
per call without the wrappers' host work, as the kernel runs inside the batcher's captured step.  The legs alternate, three
rounds; the identical kernel leg is captured twice, and the difference between the twins is the run-to-run spread the other
differences are read against.  Every call reads the same buffers, so what fits the caches is served from them - as in the step,
where x was written by the launch before.

`achieved_gbs` = traffic / the fastest in-place time, traffic = read x + read feat + write out of the rows whose gate is on (an
in-place row with gate 0 moves nothing); `hbm_fraction` is that against --peak-gbs (6300: the achievable HBM rate of one MI355X).

    python tools/mb_add_rows.py [--calls 20] [--replays 50] [--peak-gbs 6300]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionspatialcontrol_amd import ops  # noqa: E402

LEVELS = [(320, 64, 64), (640, 32, 32), (1280, 16, 16), (1280, 8, 8)]
ROWS = (2, 4, 16)


def graph_of(fn, calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g


def timed(g, replays, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (replays * calls)        # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--peak-gbs", type=float, default=6300.0, help="achievable HBM rate the traffic is taken against")
    a = ap.parse_args()
    cl = torch.channels_last
    for C, h, w in LEVELS:
        for rows in ROWS:
            g = torch.Generator().manual_seed(C + rows)
            x = torch.randn(rows, C, h, w, generator=g).half().contiguous(memory_format=cl).cuda()
            feat = (torch.randn(rows // 2, C, h, w, generator=g) * 1e-2).half().contiguous(memory_format=cl).cuda()
            full = torch.cat([feat] * 2).contiguous(memory_format=cl)      # the eager route's CFG-duplicated features
            on = torch.ones(rows, device="cuda")
            alt = on.clone()
            alt[1::2] = 0.0
            scalar = torch.ones((), device="cuda", dtype=torch.float16)    # txt2img's captured step: one scalar gate on the device
            xs = [x.clone(memory_format=torch.preserve_format) for _ in range(3)]
            out = torch.empty_like(x)
            keep = {}

            def in_place(buf, gate):
                return lambda: ops.add_rows_gated(buf, feat, gate, out=buf)

            def out_of_place():
                ops.add_rows_gated(x, feat, on, out=out)

            def eager():
                keep["out"] = x + full * scalar

            legs = {"kernel_in_place_us": in_place(xs[0], on), "kernel_in_place_twin_us": in_place(xs[1], on),
                    "kernel_in_place_every_other_row_off_us": in_place(xs[2], alt), "kernel_out_of_place_us": out_of_place,
                    "eager_pair_us": eager}
            graphs = {k: graph_of(f, a.calls) for k, f in legs.items()}
            for gr in graphs.values():
                timed(gr, 5, a.calls)
            runs = [{k: timed(gr, a.replays, a.calls) for k, gr in graphs.items()} for _ in range(3)]      # alternating legs
            best = {k: min(r[k] for r in runs) for k in legs}
            row_bytes = 2 * C * h * w
            spread = max(abs(r["kernel_in_place_us"] - r["kernel_in_place_twin_us"]) for r in runs)
            line = {"C": C, "h": h, "w": w, "rows": rows, "feat_rows": rows // 2}
            line.update({k: [round(r[k], 2) for r in runs] for k in legs})
            line.update({"twin_spread_us": round(spread, 2),
                         "kernel_over_eager": round(min(best["kernel_in_place_us"], best["kernel_in_place_twin_us"]) / best["eager_pair_us"], 3),
                         "traffic_bytes_all_on": 3 * rows * row_bytes,
                         "achieved_gbs_all_on": round(3 * rows * row_bytes / best["kernel_in_place_us"] / 1e3, 1),
                         "hbm_fraction_all_on": round(3 * rows * row_bytes / best["kernel_in_place_us"] / 1e3 / a.peak_gbs, 3),
                         "traffic_bytes_every_other_row_off": 3 * (rows // 2) * row_bytes,
                         "achieved_gbs_every_other_row_off":
                             round(3 * (rows // 2) * row_bytes / best["kernel_in_place_every_other_row_off_us"] / 1e3, 1),
                         "note": "us per call, device events around graph replays (no host work), three alternating rounds; "
                                 "achieved_gbs from the fastest round; eager = `feat * gate` then `x + extra` (two launches, five "
                                 "tensor passes)"})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
