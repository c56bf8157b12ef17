"""Device time of ops.prompt_weight_rows (dsc_prompt_weight_rows_f16) in both layouts - ONE workgroup per (request, chunk) group
doing both passes, and several workgroups per group that each redo the sums and store a slice - beside the eager chain it
replaces on the device (ops.prompt_weight_torch per group: the mean, the broadcast multiply, the second mean, the division, the
scaling and the cast, then the copies into the requests' rows), for 1, 2 and 8 groups of [2, 77, 768].  Timed with device events
on a warm device, alternating: plain keys over back-to-back calls from Python (bound by the host), graph_ keys over replays of a
graph of 20 calls (device time, z in the caches as it is behind the encoder).  The outputs are compared with the restatement
before anything is timed.  A last line times one captured replay of a CLIP-L-sized encoder on a [2, 77] CFG pair
(CLIPTextModel.encode_rows, random weights), the work the launch follows on the text lane.  One JSON line per case.

    python tools/mb_prompt_weight.py [--iters 1000]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionspatialcontrol_amd import _lib, ops  # noqa: E402
from mb_image_finish import graph_timed, timed  # noqa: E402

T, C = 77, 768
SLICES = (1, 2, 4, 8, 16)                       # workgroups per group: 1 = the one-workgroup layout


def weight_case(n):
    g = torch.Generator().manual_seed(n)
    z = (torch.randn(2 * n, T, C, generator=g) - 0.11).half().cuda()
    choices = torch.tensor([1.0, 1.1, 1 / 1.1, 1.21, 1.3, 0.5])
    mult = choices[torch.randint(0, 6, (n, 2, T), generator=g)].cuda()
    out = torch.empty(n, 2, T, C, dtype=torch.float16, device="cuda")
    groups = [{"rows": (2 * j, 2 * j + 1), "mult": mult[j], "out": (out[j, 0], out[j, 1])} for j in range(n)]
    lib = _lib.load_library()

    def kernel(slices):
        def run():
            lib.dsc_debug_set_prompt_weight_slices(slices)
            ops.prompt_weight_rows(z, groups)
        return run

    def eager():
        for j in range(n):
            out[j].copy_(ops.prompt_weight_torch(z[2 * j:2 * j + 2], mult[j]))

    cases = {f"kernel_{s}wg_us": kernel(s) for s in SLICES}
    cases["eager_us"] = eager
    same = True
    for s in SLICES:
        out.zero_()
        kernel(s)()
        torch.cuda.synchronize()
        want = [torch.from_numpy(ops.prompt_weight_numpy(z[2 * j:2 * j + 2].cpu().numpy(), mult[j].cpu().numpy())) for j in range(n)]
        same = same and all(torch.equal(out[j].cpu(), want[j]) for j in range(n))
    for fn in cases.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    return cases, same, n * 2 * T * C * 2 * 2


def encoder_case(iters):
    from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel
    cfg = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
               max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407)
    torch.manual_seed(0)
    enc = CLIPTextModel(cfg).half().cuda().eval()
    ids = torch.randint(0, 49406, (2, T), device="cuda")
    runs = [graph_timed(lambda: enc.encode_rows(ids), max(iters // 20, 10), calls=1) for _ in range(3)]
    return {"op": "clip_l_encode_rows", "ids": [2, T], "graph_us": [round(r, 1) for r in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    a = ap.parse_args()
    try:
        for n in (1, 2, 8):
            cases, same, nbytes = weight_case(n)
            runs = [{k: timed(fn, a.iters) for k, fn in cases.items()} for _ in range(3)]                # alternating
            graphs = [{k: graph_timed(fn, max(a.iters // 20, 10)) for k, fn in cases.items()} for _ in range(3)]
            print(json.dumps({"op": "prompt_weight_rows", "groups": n, "T": T, "C": C, "equal_to_restatement": bool(same),
                              **{k: [round(r[k], 2) for r in runs] for k in cases},
                              **{"graph_" + k: [round(r[k], 2) for r in graphs] for k in cases}, "bytes": nbytes}), flush=True)
    finally:
        _lib.load_library().dsc_debug_set_prompt_weight_slices(0)
    print(json.dumps(encoder_case(a.iters)), flush=True)


if __name__ == "__main__":
    main()
