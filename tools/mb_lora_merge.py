"""One LoRA rescale over every SD1.5 target: a synthetic rank-32 adapter on all Linear / 1x1-conv weights of the transformer
blocks of an SD1.5-shaped UNet and of a CLIP-L-shaped text encoder (random weights), merged through pipe.load_lora_weights.
Timed on a warm device, alternating, three runs each:
    kernel_device_ms / kernel_wall_ms   pipe.set_lora_scale: the gain upload and ONE dsc_lora_merge_f16 launch over the table -
                                        device events around the call, and a host clock around the call and a synchronise
    eager_device_ms / eager_wall_ms     ops.lora_merge_eager over the same table (the reference's fp32 mm, scale, add, cast per
                                        weight), into scratch destinations
The merged weights of the two routes are compared first (share of elements that differ).  `bytes` is what the kernel has to move:
every touched weight read once and written once, plus the factors.  With --parent DIR (a checkout of the parent commit with its
library built) it then runs `bench.py --gpus 1 --steps 8 --warmup 2` in this tree and in DIR, alternating, three runs each, and
prints each run's headline figures; without it that measurement is reported as not taken.  One JSON line per measurement.

    python tools/mb_lora_merge.py [--iters 20] [--parent DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffusionspatialcontrol_amd import ops  # noqa: E402
from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel  # noqa: E402
from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline  # noqa: E402
from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig  # noqa: E402

RANK = 32
CLIP_L = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
              max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407)


def synthetic_adapter(unet, te):
    g = torch.Generator().manual_seed(0)
    sd = {}
    for prefix, model, keep in (("lora_unet_", unet, lambda n: ".attentions." in n), ("lora_te_text_model_", te, lambda n: True)):
        for n, m in model.named_modules():
            linear = isinstance(m, torch.nn.Linear)
            if not keep(n) or not (linear or (isinstance(m, torch.nn.Conv2d) and tuple(m.kernel_size) == (1, 1))):
                continue
            N, K = m.weight.shape[:2]
            head = prefix + n.replace(".", "_")
            down, up = (0.05 * torch.randn(RANK, K, generator=g)).half(), (0.05 * torch.randn(N, RANK, generator=g)).half()
            sd[head + ".lora_down.weight"] = down if linear else down[:, :, None, None]
            sd[head + ".lora_up.weight"] = up if linear else up[:, :, None, None]
    return sd


def measure(fn, iters):
    """(device ms, wall ms) per call: events around `iters` calls, a host clock around them and the synchronise"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) * 1e3 / iters


def bench_line(tree):
    try:
        out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "2"], cwd=tree,
                             capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        return {"error": "timeout"}
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if out.returncode != 0 or not lines:
        return {"error": out.returncode, "stderr": out.stderr[-400:]}
    res = json.loads(lines[-1])
    return {k: res.get(k) for k in ("value", "unit", "ms_per_step", "status")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, library built, for the bench.py A/B")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    torch.manual_seed(0)
    unet = UNet2DConditionModel(UNetConfig.sd15()).half().cuda()
    te = CLIPTextModel(CLIP_L).half().cuda().eval()
    pipe = StableDiffusionPipeline(None, te, None, unet, SD15Scheduler())
    pipe.load_lora_weights(synthetic_adapter(unet, te), scale=0.8, name="synthetic")
    mgr, st = pipe._lora, pipe.lora_state()
    targets = list(mgr.targets.values())
    assert st["kernel_targets"] == st["targets"], st
    factors = sum(j[2].numel() + j[3].numel() for j in mgr.table.jobs) * 2
    scratch = [torch.empty_like(t.param) for t in targets]
    adapters = [[(l.up, l.down, 0.8) for _, l in mgr._on(t)] for t in targets]

    def eager():
        for dst, t, ad in zip(scratch, targets, adapters):
            ops.lora_merge_eager(dst, t.base, ad)

    eager()
    diff = sum(int((d != t.param).sum()) for d, t in zip(scratch, targets))
    total = sum(t.param.numel() for t in targets)
    scale = [0.8]

    def kernel():
        scale[0] = 1.3 - scale[0]                                          # 0.5 / 0.8 in turn: every call changes the weights
        pipe.set_lora_scale(scale[0])

    for fn in (kernel, eager):
        for _ in range(3):
            fn()
    runs = [{"kernel": measure(kernel, a.iters), "eager": measure(eager, a.iters)} for _ in range(3)]      # alternating
    print(json.dumps({"op": "lora_rescale_sd15", "rank": RANK, "weights": st["targets"], "tiles": int(mgr.table.tiles),
                      "launches_kernel": 1, "elements": total, "bytes": 2 * st["base_bytes"] + factors,
                      "base_bytes": st["base_bytes"], "elements_differing_from_eager": diff,
                      "kernel_device_ms": [round(r["kernel"][0], 3) for r in runs],
                      "kernel_wall_ms": [round(r["kernel"][1], 3) for r in runs],
                      "eager_device_ms": [round(r["eager"][0], 3) for r in runs],
                      "eager_wall_ms": [round(r["eager"][1], 3) for r in runs]}), flush=True)
    del pipe, unet, te, scratch, targets, adapters, mgr
    torch.cuda.empty_cache()
    if a.parent is None:
        print(json.dumps({"op": "bench_ab", "measured": False, "why": "no --parent checkout given"}), flush=True)
        return
    for i in range(3):
        for name, tree in (("this", ROOT), ("parent", os.path.abspath(a.parent))):
            res = bench_line(tree)
            print(json.dumps({"op": "bench_ab", "run": i, "tree": name, "result": res}), flush=True)
            if "error" in res:                                             # a failed run ends the measurement: nothing more on this GPU
                return


if __name__ == "__main__":
    main()
