"""ops.ip_xattn_add (dsc_ip_xattn_add_f16) beside the five-op route of `_IPAdapterProcessor._ip_branch` it replaces in the continuous
batcher's step - to_k_ip(tokens), to_v_ip(tokens), ops.region_xattn without a table, an eager multiply and an eager add - at the
four cross-attention levels of SD1.5 at 512 x 512 with 16 batch rows (8 requests) and 4 / 16 image tokens.  One JSON line per case.

Both routes are captured into a graph of --calls launches and the graph is replayed (device events around the replays): the
figures are device time per call without the wrappers' host work, as the kernel runs inside the batcher's captured step.  Every
call reads the same buffers, so what fits the caches (L2 4 MB per XCD, Infinity Cache 256 MB) is served from them - as in the
step, where q and io were written by the two launches before; --sets N rotates over N buffer sets instead (N x the working set).
`bound_fraction` = (6 B L C bytes / kernel time) / --peak-gbs: the q read, the io read and the io write against the HBM peak.

The masked leg (one more line per level, 4 tokens): dsc_ip_xattn_add_masked_f16 with query weights of all ones, of ones on the top
half of the image and zeros below, and of all zeros, beside the unmasked entry on the same inputs (all-ones / unmasked = what the
weights cost a row without a mask; half / all-ones = what skipping all-zero tiles buys) and beside the eager route with a mask:
the five ops above plus IPAdapterMaskProcessor.downsample (a bicubic interpolate, a repeat to [B, L, C]) and a multiply, as
`_ip_branch` runs them in every layer and step.

    python tools/mb_ip_xattn.py [--calls 20] [--replays 50] [--sets 1] [--peak-gbs 8000]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionspatialcontrol_amd import ops  # noqa: E402
from diffusionspatialcontrol_amd.modules.attention_modify import IPAdapterMaskProcessor  # noqa: E402

LEVELS = [(4096, 40), (1024, 80), (256, 160), (64, 160)]        # (L, d) of SD1.5's cross-attention layers, 8 heads
H, ROWS, CTX = 8, 16, 768


def graph_of(fn, calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn(0)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(calls):
            fn(i)
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
    ap.add_argument("--sets", type=int, default=1)
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="HBM peak the traffic bound is taken against")
    a = ap.parse_args()
    for L, d in LEVELS:
        for T in (4, 16):
            C = H * d
            g = torch.Generator().manual_seed(L + T)
            sets = []
            for _ in range(a.sets):
                sets.append({"q": (torch.randn(ROWS, L, H, d, generator=g) * 0.5).half().cuda(),
                             "io": torch.randn(ROWS, L, C, generator=g).half().cuda(),
                             "tok": torch.randn(ROWS, T, CTX, generator=g).half().cuda()})
            wk = (torch.randn(C, CTX, generator=g) * 0.03).half().cuda()
            wv = (torch.randn(C, CTX, generator=g) * 0.03).half().cuda()
            for s in sets:
                s["k"] = (s["tok"] @ wk.t()).view(ROWS, T, H, d).contiguous()
                s["v"] = (s["tok"] @ wv.t()).view(ROWS, T, H, d).contiguous()
            row_scale = torch.full((ROWS,), 1e-3, device="cuda")        # (small: io stays finite over thousands of accumulations)
            half_rows = row_scale.clone()
            half_rows[::2] = 0.0

            def kernel(i, rs=row_scale):
                s = sets[i % len(sets)]
                ops.ip_xattn_add(s["q"], s["k"], s["v"], rs, s["io"])

            def kernel_half(i):
                kernel(i, half_rows)

            def eager(i):
                s = sets[i % len(sets)]
                k4 = torch.nn.functional.linear(s["tok"], wk).view(ROWS, T, H, d)
                v4 = torch.nn.functional.linear(s["tok"], wv).view(ROWS, T, H, d)
                o = ops.region_xattn(s["q"], k4, v4, None, layout="blhd", ref_fp16_rounding=False)
                s["out"] = s["io"] + 1e-3 * o.reshape(ROWS, L, C)

            graphs = [graph_of(f, a.calls) for f in (kernel, kernel_half, eager)]
            for gr in graphs:
                timed(gr, 5, a.calls)
            runs = [[timed(gr, a.replays, a.calls) for gr in graphs] for _ in range(3)]          # alternating
            best = min(r[0] for r in runs)
            traffic = 6.0 * ROWS * L * C
            print(json.dumps({"L": L, "d": d, "heads": H, "rows": ROWS, "tokens": T, "sets": a.sets,
                              "working_set_mb": round(a.sets * traffic * 2 / 3 / 2 ** 20, 1),
                              "kernel_us": [round(r[0], 2) for r in runs], "kernel_half_rows_skipped_us": [round(r[1], 2) for r in runs],
                              "eager_route_us": [round(r[2], 2) for r in runs],
                              "traffic_bytes": int(traffic), "achieved_gbs": round(traffic / best / 1e3, 1),
                              "bound_fraction": round(traffic / best / 1e3 / a.peak_gbs, 3),
                              "note": "us per call, device events around graph replays (no host work); fastest of three runs for "
                                      "achieved_gbs; eager = 2 library GEMMs + region_xattn (no table) + multiply + add"}), flush=True)
            if T != 4:
                continue
            weights = {"ones": torch.ones(ROWS, L, dtype=torch.float16, device="cuda")}
            weights["half"] = weights["ones"].clone()
            weights["half"][:, L // 2:] = 0.0
            weights["zero"] = torch.zeros_like(weights["ones"])
            mask = torch.zeros(1, 512, 512, device="cuda")
            mask[:, :256] = 1.0

            def masked(name):
                def fn(i):
                    s = sets[i % len(sets)]
                    ops.ip_xattn_add(s["q"], s["k"], s["v"], row_scale, s["io"], q_weight=weights[name])
                return fn

            def eager_masked(i):
                s = sets[i % len(sets)]
                k4 = torch.nn.functional.linear(s["tok"], wk).view(ROWS, T, H, d)
                v4 = torch.nn.functional.linear(s["tok"], wv).view(ROWS, T, H, d)
                o = ops.region_xattn(s["q"], k4, v4, None, layout="blhd", ref_fp16_rounding=False).reshape(ROWS, L, C)
                o = o * IPAdapterMaskProcessor.downsample(mask, ROWS, L, C).to(dtype=o.dtype)
                s["out"] = s["io"] + 1e-3 * o

            legs = [kernel, masked("ones"), masked("half"), masked("zero"), eager_masked]
            graphs = [graph_of(f, a.calls) for f in legs]
            for gr in graphs:
                timed(gr, 5, a.calls)
            runs = [[timed(gr, a.replays, a.calls) for gr in graphs] for _ in range(3)]          # alternating
            best = [min(r[j] for r in runs) for j in range(len(legs))]
            print(json.dumps({"leg": "masked", "L": L, "d": d, "heads": H, "rows": ROWS, "tokens": T, "sets": a.sets,
                              "unmasked_us": [round(r[0], 2) for r in runs], "masked_all_ones_us": [round(r[1], 2) for r in runs],
                              "masked_top_half_us": [round(r[2], 2) for r in runs], "masked_all_zero_us": [round(r[3], 2) for r in runs],
                              "eager_route_with_mask_us": [round(r[4], 2) for r in runs],
                              "all_ones_over_unmasked": round(best[1] / best[0], 3), "top_half_over_all_ones": round(best[2] / best[1], 3),
                              "note": "us per call as above, ratios of the fastest of three runs; eager = the five ops + bicubic "
                                      "interpolate + repeat + multiply"}), flush=True)


if __name__ == "__main__":
    main()
