"""The CLIP text encoder on the package's kernels (modules/clip_text.py), three levels, one JSON line each:

  kernel  dsc_causal_attn_f16 at (B = 2, H = 12, S = 77, d = 64) on three views of one fused QKV buffer, beside torch's fp16
          scaled_dot_product_attention(is_causal=True) on the same values: device time per call - both captured into a graph of
          --calls launches, device events around the replays (no host work in the figure);
  layer   one encoder layer of CLIP-L's shape (768 wide, 3072 inner, 12 heads; eight launches) on [2, 77, 768], the same way;
  encode  the 12-layer CLIP-L shape with random weights at n = 2 (one CFG pair) and n = 6: WALL time per call (host clock around
          --encodes calls and one synchronize) of the native module launched eagerly, of its captured encode (enable_graphs)
          and of transformers' CLIPTextModel in fp16 as the library runs it (eager launches, its default attention).

    python tools/mb_clip_text.py [--calls 20] [--replays 50] [--encodes 30]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionspatialcontrol_amd import ops  # noqa: E402
from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel  # noqa: E402

CLIP_L = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
              max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407)


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


def wall(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / n                   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--encodes", type=int, default=30)
    a = ap.parse_args()
    torch.manual_seed(0)
    B, H, S, d = 2, 12, 77, 64
    C = H * d
    qkv = torch.randn(B, S, 3, H, d, device="cuda").half()
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    out = torch.empty(B, S, H, d, dtype=torch.float16, device="cuda")
    qt, kt, vt = (t.transpose(1, 2) for t in (q, k, v))
    graphs = [graph_of(lambda: ops.causal_attn(q, k, v, into=out), a.calls),
              graph_of(lambda: torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, is_causal=True), a.calls)]
    for g in graphs:
        timed(g, 5, a.calls)
    runs = [[timed(g, a.replays, a.calls) for g in graphs] for _ in range(3)]                    # alternating
    print(json.dumps({"level": "kernel", "B": B, "H": H, "S": S, "d": d, "dsc_causal_attn_f16_us": [round(r[0], 2) for r in runs],
                      "torch_sdpa_causal_us": [round(r[1], 2) for r in runs],
                      "note": "device us per call, events around graph replays; q / k / v views of one fused buffer"}), flush=True)

    model = CLIPTextModel(CLIP_L).half().cuda().eval()
    h = torch.randn(2, S, C, device="cuda").half()
    layer = model.encoder.layers[0]
    with torch.no_grad():
        g = graph_of(lambda: model._layer_kernels(layer, h), a.calls)
        timed(g, 5, a.calls)
        print(json.dumps({"level": "layer", "rows": 2 * S, "hidden": C, "launches": 8,
                          "layer_us": [round(timed(g, a.replays, a.calls), 2) for _ in range(3)],
                          "note": "device us per layer, events around graph replays"}), flush=True)

    hf = None
    try:
        import transformers
        cfg = transformers.CLIPTextConfig(**CLIP_L, bos_token_id=49406, pad_token_id=1)
        hf = transformers.CLIPTextModel(cfg).half().cuda().eval()
        model.load_state_dict(hf.state_dict())
    except ImportError:
        pass
    for n in (2, 6):
        ids = torch.randint(0, 49000, (n, S), device="cuda")
        ids[:, -1] = 49407
        legs = {}
        with torch.no_grad():
            model.enable_graphs(False)
            eager = [wall(lambda: model(ids), a.encodes) for _ in range(3)]
            model.enable_graphs(True)
            model(ids)
            captured = [wall(lambda: model(ids), a.encodes) for _ in range(3)]
            if hf is not None:
                legs["transformers_fp16_eager_wall_us"] = [round(wall(lambda: hf(ids), a.encodes), 1) for _ in range(3)]
        print(json.dumps({"level": "encode", "n": n, "S": S, "layers": 12, "hidden": C,
                          "native_eager_wall_us": [round(t, 1) for t in eager], "native_captured_wall_us": [round(t, 1) for t in captured],
                          **legs, "graph_captures": model.graph_captures,
                          "note": "wall us per encode call (host clock, one synchronize after --encodes calls); random weights"}),
              flush=True)


if __name__ == "__main__":
    main()
