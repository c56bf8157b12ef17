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

The scatter leg (`--legs scatter`): ops.scatter_add_rows (dsc_scatter_add_rows_f16, the ControlNet residuals of the batcher's
compact lanes) beside the eager route it replaces - per skip tensor a multiply by the per-row scales, a sum over the nets and an
indexed add into the batch rows - at the six distinct SD1.5 skip shapes, 16 batch rows, 8 and 16 lane rows (control_slots 4 and
8), one and two nets, every lane active and every other lane idle.  Same method, one JSON line per case ("leg": "scatter").

    python tools/mb_add_rows.py [--legs gated,scatter] [--calls 20] [--replays 50] [--peak-gbs 6300]
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


SKIPS = [(320, 64, 64), (320, 32, 32), (640, 32, 32), (640, 16, 16), (1280, 16, 16), (1280, 8, 8)]


def scatter_leg(a):
    X = 16
    for C, h, w in SKIPS:
        for R in (8, 16):
            for A in (1, 2):
                g = torch.Generator().manual_seed(C + h + R + A)
                x = torch.randn(X, C, h, w, generator=g).half().contiguous(memory_format=torch.channels_last).cuda()
                feat = (torch.randn(A, R, h, w, C, generator=g) * 1e-2).half().cuda().permute(0, 1, 4, 2, 3)
                lanes = R // 2                                             # lane j: rows j and X / 2 + j, as the batcher maps them
                dst = torch.tensor([j for j in range(lanes)] + [X // 2 + j for j in range(lanes)], dtype=torch.int32).cuda()
                half_dst = dst.clone()
                half_dst[1::2] = -1
                gate = torch.full((A, R), 0.9, device="cuda")
                idx = dst.long()
                gcol = gate.half().view(A, R, 1, 1, 1)
                xs = [x.clone(memory_format=torch.preserve_format) for _ in range(4)]

                def kernel(buf, d):
                    return lambda: ops.scatter_add_rows(buf, feat, gate, d)

                def eager():
                    scaled = feat * gcol
                    xs[3].index_add_(0, idx, scaled.sum(0) if A > 1 else scaled[0])

                legs = {"kernel_us": kernel(xs[0], dst), "kernel_twin_us": kernel(xs[1], dst),
                        "kernel_every_other_lane_idle_us": kernel(xs[2], half_dst), "eager_route_us": eager}
                graphs = {k: graph_of(f, a.calls) for k, f in legs.items()}
                for gr in graphs.values():
                    timed(gr, 5, a.calls)
                runs = [{k: timed(gr, a.replays, a.calls) for k, gr in graphs.items()} for _ in range(3)]
                best = {k: min(r[k] for r in runs) for k in legs}
                row_bytes = 2 * C * h * w
                traffic = (2 + A) * R * row_bytes                          # read x rows, read A feature rows, write x rows
                line = {"leg": "scatter", "C": C, "h": h, "w": w, "batch_rows": X, "lane_rows": R, "nets": A}
                line.update({k: [round(r[k], 2) for r in runs] for k in legs})
                line.update({"twin_spread_us": round(max(abs(r["kernel_us"] - r["kernel_twin_us"]) for r in runs), 2),
                             "kernel_over_eager": round(min(best["kernel_us"], best["kernel_twin_us"]) / best["eager_route_us"], 3),
                             "traffic_bytes": traffic, "achieved_gbs": round(traffic / best["kernel_us"] / 1e3, 1),
                             "hbm_fraction": round(traffic / best["kernel_us"] / 1e3 / a.peak_gbs, 3),
                             "note": "us per call, device events around graph replays, three alternating rounds; eager = `feat * "
                                     "scale` (+ `.sum(0)` over two nets) then `x.index_add_`"})
                print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--peak-gbs", type=float, default=6300.0, help="achievable HBM rate the traffic is taken against")
    ap.add_argument("--legs", default="gated,scatter", help="comma-separated: gated (add_rows_gated), scatter (scatter_add_rows)")
    a = ap.parse_args()
    legs_wanted = set(a.legs.split(","))
    if "scatter" in legs_wanted:
        scatter_leg(a)
    if "gated" not in legs_wanted:
        return
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
