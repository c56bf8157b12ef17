"""Per-call cost from Python of the convolution forms a latent with odd level sides needs, each beside the route it replaces, timed
with device events on a warm device, alternating.  One JSON line per case.

  stride2   ops.conv3x3(stride2_ceil=True) on odd... and even sides of a 608 x 608 generation's levels, beside the library's
            stride-2 / pad-1 convolution (what Downsample2D.conv ran for odd sides before)
  upsample  ops.conv3x3(upsample_size=skip size) beside ops.conv3x3 on a materialised F.interpolate(size=...)
  conv_in   ops.conv3x3_fewcin at 76 x 76 beside the eager NCHW convolution + layout change
  step      (--step) per-step time of a fused 25-step txt2img at 608 x 608 beside 640 x 640, SD1.5 geometry, random weights

    python tools/mb_conv_resample.py [--iters 500] [--step]
"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionspatialcontrol_amd import ops  # noqa: E402

CL = torch.channels_last


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters                  # us per call, launches back to back


def compare(name, shape, new, old, iters, note):
    for fn in (new, old):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    runs = [(timed(new, iters), timed(old, iters)) for _ in range(3)]                        # alternating
    print(json.dumps({"case": name, "shape": shape, "new_us": [round(a, 2) for a, _ in runs],
                      "replaced_us": [round(b, 2) for _, b in runs], "note": note}), flush=True)


def operands(B, C, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, h, w, generator=g).half().cuda().contiguous(memory_format=CL)
    wt = (torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)).half().cuda().contiguous(memory_format=CL)
    b = (torch.randn(C, generator=g) * 0.2).half().cuda()
    return x, wt, b


def step_times(size, steps=25):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    cfg = UNetConfig.sd15()
    unet = UNet2DConditionModel(cfg).half().cuda()
    pipe = StableDiffusionPipeline(None, None, None, unet, SD15Scheduler())
    emb = torch.randn(1, 77, cfg.cross_attention_dim).half()
    kw = dict(height=size, width=size, num_inference_steps=steps, sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"},
              prompt_embeds=emb, negative_prompt_embeds=emb * 0, output_type="latent", fused=True,
              latents=torch.randn(1, 4, size // 8, size // 8).half())
    pipe.txt2img(None, **kw)                                   # capture
    out = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.txt2img(None, **kw)
        torch.cuda.synchronize()
        out.append(round(1e3 * (time.perf_counter() - t0) / steps, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    for B, C, h, w in [(2, 320, 76, 76), (2, 640, 38, 38), (2, 1280, 19, 19)]:
        x, wt, b = operands(B, C, h, w)
        compare("stride2", [B, C, h, w], lambda: ops.conv3x3(x, wt, b, stride2_ceil=True),
                lambda: F.conv2d(x, wt, b, stride=2, padding=1), a.iters,
                "new = dsc_conv3x3_nhwc_f16 resample 2; replaced = the library's stride-2 / pad-1 convolution, channels_last")
    for B, C, (h, w), dst in [(2, 1280, (10, 10), (19, 19)), (2, 1280, (19, 19), (38, 38)), (2, 640, (38, 38), (76, 76))]:
        x, wt, b = operands(B, C, h, w, seed=1)
        compare("upsample", [B, C, h, w, *dst], lambda: ops.conv3x3(x, wt, b, upsample_size=dst),
                lambda: ops.conv3x3(F.interpolate(x, size=dst, mode="nearest"), wt, b), a.iters,
                "new = resample 4 (gather through dst >> 1); replaced = F.interpolate(size=...) materialised + resample 0")
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(2, 4, 76, 76, generator=g).half().cuda()
    w4 = (torch.randn(320, 4, 3, 3, generator=g) / 6).half().cuda()
    b4 = (torch.randn(320, generator=g) * 0.2).half().cuda()
    w4t = w4.reshape(320, -1).t().contiguous()
    compare("conv_in", [2, 4, 76, 76, 320], lambda: ops.conv3x3_fewcin(lat, w4t, b4, 320),
            lambda: F.conv2d(lat, w4, b4, padding=1).contiguous(memory_format=CL), a.iters,
            "new = dsc_conv3x3_fewcin_f16 (W % 8 != 0); replaced = eager NCHW convolution + layout change")
    if a.step:
        for size in (608, 640):
            print(json.dumps({"case": "step", "size": size, "ms_per_step": step_times(size),
                              "note": "fused 25-step txt2img, SD1.5 geometry, random weights, batch 1 + CFG; wall clock / steps"}), flush=True)


if __name__ == "__main__":
    main()
