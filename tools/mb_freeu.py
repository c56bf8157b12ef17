"""ops.freeu_rows_ (dsc_freeu_rows_f16) beside ops.freeu_eager (diffusers' algorithm with torch.fft in fp32: fftn, two shifts, a mask
multiply, ifftn, .real, casts, plus the half-channel multiply) at the six FreeU call shapes of the SD1.5 UNet at 512 px - up
block 0: three ResNets at 8x8, hidden 1280, skips 1280 / 1280 / 1280; up block 1: three at 16x16, hidden 1280, skips 1280 / 1280 /
640 - and their 768 px counterparts (12x12, 24x24), with 2 and 16 batch rows (one image and a full batcher).  One JSON line per
case.

The kernel legs are captured into a graph of --calls launches and the graph is replayed (device events around the replays): device
time per call without the wrapper's host work, as the launch runs inside a captured step.  The identical leg is captured twice;
the difference between the twins is the run-to-run spread.  `kernel_every_other_row_identity_us`: every other row holds (1, 1,
1, 1) and is skipped.  The eager leg is NOT captured (FFT plans inside a capture are what the kernel avoids): device events around
--calls direct calls, host launch cost included where the device outruns it - the cost the eager route has in an eager step.
The kernel works in place; the timing values are s = 0.2 and b = 1.0001 (not 1: that row would be skipped), under which repeated
application keeps every value finite.

The step leg (`--step`): the SD1.5 UNet forward at 64x64 latents with 2 and 16 batch rows, captured into a graph - without the
`freeu_rows` keyword, with a table of ones (six launches that return at once) and with the values (0.9, 0.2, 1.5, 1.6) in every
row; ms per forward, three alternating rounds ("leg": "step").

    python tools/mb_freeu.py [--calls 20] [--replays 50] [--step]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionspatialcontrol_amd import ops  # noqa: E402

#        px, stage, C_h, C_s, side
SHAPES = [(512, 0, 1280, 1280, 8), (512, 1, 1280, 1280, 16), (512, 1, 1280, 640, 16),
          (768, 0, 1280, 1280, 12), (768, 1, 1280, 1280, 24), (768, 1, 1280, 640, 24)]
CALLS_PER_STEP = {(0, 1280): 3, (1, 1280): 2, (1, 640): 1}      # how often a step makes the call


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


def timed(run, replays, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(replays):
        run()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (replays * calls)        # us per call


def step_leg(replays):
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    with torch.device("cuda"):
        unet = UNet2DConditionModel(UNetConfig.sd15()).half().eval()
    for rows in (2, 16):
        g = torch.Generator().manual_seed(rows)
        x = torch.randn(rows, 4, 64, 64, generator=g).half().cuda()
        t = torch.full((rows,), 500.0, device="cuda")
        text = torch.randn(rows, 77, 768, generator=g).half().cuda()
        ones = torch.ones(rows, 4, device="cuda")
        vals = torch.tensor([[0.9, 0.2, 1.5, 1.6]] * rows, device="cuda")
        keep = {}

        def forward(table):
            def run():
                with torch.no_grad():
                    keep["out"] = unet(x, t, text, **({} if table is None else {"freeu_rows": table})).sample
            return run

        legs = {"no_keyword_ms": forward(None), "no_keyword_twin_ms": forward(None), "table_of_ones_ms": forward(ones),
                "values_in_every_row_ms": forward(vals)}
        graphs = {k: graph_of(f, 1) for k, f in legs.items()}
        for gr in graphs.values():
            timed(gr.replay, 3, 1)
        runs = [{k: timed(gr.replay, replays, 1) / 1e3 for k, gr in graphs.items()} for _ in range(3)]
        line = {"leg": "step", "unet": "sd15", "latent": "64x64", "rows": rows}
        line.update({k: [round(r[k], 3) for r in runs] for k in legs})
        line["note"] = "ms per captured UNet forward, device events around graph replays, three alternating rounds"
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--step", action="store_true", help="only the step leg: the SD1.5 UNet forward with and without FreeU")
    a = ap.parse_args()
    if a.step:
        step_leg(a.replays)
        return
    cl = torch.channels_last
    for px, stage, C_h, C_s, side in SHAPES:
        for rows in (2, 16):
            g = torch.Generator().manual_seed(C_s + side + rows)
            hidden = (torch.randn(rows, C_h, side, side, generator=g) * 2 + 5).half().contiguous(memory_format=cl).cuda()
            skip = (torch.randn(rows, C_s, side, side, generator=g) * 2 + 5).half().contiguous(memory_format=cl).cuda()
            on = torch.tensor([[0.2, 0.2, 1.0001, 1.0001]] * rows, device="cuda")
            alt = on.clone()
            alt[1::2] = 1.0
            bufs = [(hidden.clone(memory_format=torch.preserve_format), skip.clone(memory_format=torch.preserve_format))
                    for _ in range(3)]
            keep = {}

            def kernel(pair, params):
                return lambda: ops.freeu_rows_(pair[0], pair[1], params, stage)

            def eager():
                keep["out"] = ops.freeu_eager(hidden, skip, on[:, stage], on[:, 2 + stage])

            legs = {"kernel_us": kernel(bufs[0], on), "kernel_twin_us": kernel(bufs[1], on),
                    "kernel_every_other_row_identity_us": kernel(bufs[2], alt)}
            graphs = {k: graph_of(f, a.calls) for k, f in legs.items()}
            for gr in graphs.values():
                timed(gr.replay, 5, a.calls)
            for _ in range(3):
                eager()
            runs = []
            for _ in range(3):                                   # alternating legs
                r = {k: timed(gr.replay, a.replays, a.calls) for k, gr in graphs.items()}
                r["eager_us"] = timed(eager, a.calls, 1)
                runs.append(r)
            best = {k: min(r[k] for r in runs) for k in runs[0]}
            traffic = 2 * 2 * rows * side * side * (C_s + C_h // 2)          # read + write, the skip tensor and half the hidden
            line = {"px": px, "stage": stage, "C_h": C_h, "C_s": C_s, "h": side, "w": side, "rows": rows,
                    "calls_per_step": CALLS_PER_STEP[(stage, C_s)]}
            line.update({k: [round(r[k], 2) for r in runs] for k in runs[0]})
            line.update({"twin_spread_us": round(max(abs(r["kernel_us"] - r["kernel_twin_us"]) for r in runs), 2),
                         "kernel_over_eager": round(min(best["kernel_us"], best["kernel_twin_us"]) / best["eager_us"], 4),
                         "traffic_bytes": traffic, "achieved_gbs": round(traffic / best["kernel_us"] / 1e3, 1),
                         "note": "us per call, three alternating rounds; kernel legs: device events around graph replays; eager leg: "
                                 "device events around direct calls (about ten launches each, not captured)"})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
