"""Continuous-batching serving measurements (modules/serving/) on one GPU; one JSON line per leg.

    python tools/serve_bench.py [--requests 16] [--rates 2,6] [--seed 0] [--mix] [--sampler NAME] [--guidance-rescale PHI]
                                [--hires X] [--ip-adapter [--ip-masks]] [--t2i-adapter] [--controlnet [--control-slots C]]
                                [--images uint8|pil|np [--decode-batch D]] [--previews K [--preview-scale S]] [--inpaint-unet]
                                [--pixels [--encode-batch E] [--inpaint-unet]] [--prompts [--text-batch E]]

Legs (SD1.5-shape UNet with seeded random weights at 512x512, heterogeneous requests: 1/2/4 masks, distinct prompts and
latents, as tests/test_full_size_parity_gpu.py::_requests builds them):
  saturated   8 slots kept full, 25 steps each: images/s of the batcher (one and two batchers in flight) beside
              txt2img_coalesced at k = 8 (one and two in flight) on the same requests in the same process
  staggered   Poisson arrivals at each rate, mixed step counts (20/25/30) and guidance scales (5/7.5): images/s and p50/p95
              request latency of the batcher against one-at-a-time txt2img and lockstep txt2img_coalesced batches of 8
  join        the stall a join puts on the running rows: host ms of a step that admits a request (text K/V refresh, table
              compression and upload) minus that of a plain step, with the GPU time of the refresh
  stats       the batcher's counters; captures after warm() must be 0
  mix         (--mix: this leg and the saturated txt2img figure only) 8 slots kept full with one third each txt2img / img2img at
              strength 0.6 / inpainting at strength 1.0 (4-channel latents as `image`, distinct prompts and masks per request):
              images/s and sampler steps/s beside the same figures of the all-txt2img batch in the same process
  sampler     (--sampler NAME, one of sampling.LINEAR_FAMILY: this leg only) 8 slots kept full, every other request running NAME
              (its step goes through dsc_cfg_linear_step_rows, with a noise table per request) beside the all-DPM++ 2M batch in
              the same process, three alternating runs; then one-at-a-time txt2img with NAME, fused against protocol mode.
              NAME of sampling.TWO_CALL_FAMILY (sample_heun, sample_dpm_2, sample_dpm_2_ancestral, sample_dpmpp_2s_ancestral,
              sample_dpmpp_sde) builds the batcher with two_call=True (its steps go through dsc_cfg_staged_step_rows, two model
              calls each: the leg also prints model calls/s); --two-call alone is that batcher with no such request, and
              --two-call --kernels only the device time of the per-row sampler entries, the staged one included
  rescale     (--guidance-rescale PHI, alone or with --sampler: this leg only) the same leg with `guidance_rescale` = PHI on
              every other request (its step goes through dsc_cfg_linear_step_rows_rescale; DPM++ 2M unless --sampler names
              another), and one-at-a-time txt2img with PHI, fused against protocol mode
  hires       (--hires X: this leg only) a chained pair of batchers (pipe.serve_hires(512, 512, X)) driven by its two threads,
              every other request with `upscale=True, upscale_x=X` (bicubic, strength 0.7): images/s, and the latency of the
              hires requests split by pass (submit -> handed off on the host clock, handed off -> resolved) beside the plain ones
  ip_adapter  (--ip-adapter: this leg only) 8 slots kept full on a batcher built BEFORE an adapter is loaded, then - a 4-token
              adapter with seeded random weights loaded - on an IP-capable batcher, first with no image prompt at all (what every
              step pays for 16 launches that return early), then with an image prompt on every other request; and one-at-a-time
              txt2img(fused=True) with the image prompt
  ip_masks    (--ip-adapter --ip-masks: after the leg above) a batcher built with `ip_masks=True` on a third slot: the same mixed
              requests without any mask (what the weight buffers of ones cost), then with a half-image `ip_adapter_masks` on
              every other image-prompt request, alternating with the IP-capable batcher of the leg above
  t2i_adapter (--t2i-adapter: this leg only) a T2I-Adapter with seeded random weights set up, then two batchers on two slots: one
              built without `t2i_adapter` (the step of a pipeline without the feature) and one built with it.  8 slots kept full,
              three alternating rounds: the plain requests on both (the price of the flag), then every other request with a
              control image at factor 0.5 on the adapter-capable one; and what admission costs: the GPU time of one request's
              adapter forward on the batch's stream (what the next step waits for) and the host time of submit with and without
  controlnet  (--controlnet [--control-slots C, default 4]: this leg only) an SD1.5-size ControlNet with seeded random weights
              set up, then two batchers on two slots: one built without `controlnet` and one built with it on C lanes.  8 slots
              kept full, three alternating rounds: the plain requests on both (the price of the flag: thirteen launches that
              return at once and one copy of the last skip tensor), then every other request with a control image (scale 0.9,
              window [0, 0.6]) on the ControlNet-capable one; and what admission costs: the GPU time of one request's
              conditioning embedding on the batch's stream (it runs when the request is admitted), whether it repeats bit for bit, and
              the host time of submit with and without
  images      (--images uint8|pil|np [--decode-batch D, default 2]: this leg only) an SD1.x-size VAE decoder with seeded random
              weights in the pipeline, then two batchers on two slots: one built without `decode` (image output types run
              latent_to_image inline, in the poll, on the batch's stream) and one built with `decode=True, decode_batch=D` (the
              decode lane).  8 slots kept full, three alternating rounds of four runs: (a) latent output on the flagless batcher,
              (b) that image type on the flagless batcher, (c) that image type on the decode-lane batcher, (d) latent output on
              the decode-lane batcher; images/s and p50 / p95 of `dsc_latency_s` (submit -> resolved) for each; the same four
              legs with each batcher driven by its own thread and mixed step counts (20 / 25 / 30); and the device time of
              one captured decode per lane bucket
  previews    (--previews K [--preview-scale S, default 8]: this leg only) two batchers on two slots: one built without
              `previews` (the step of a batcher without the feature) and one built with `previews=True, preview_scale=S`.  8 slots
              kept full, three alternating rounds of three runs: (a) the plain requests on the flagless batcher, (b) the plain
              requests on the previews batcher (no slot is ever due: the price of the flag), (c) every request with
              `preview_every=K` and a no-op callback; images/s and p50 / p95 latency for each, with the previews launched,
              their rows, the callbacks made and the previews dropped; then (c) with the batcher driven by its own thread
  inpaint_unet (--inpaint-unet: this leg only) a second SD1.5-shape UNet with `in_channels=9` and seeded random weights, and two
              batchers on two slots: the plain one on the 4-channel pipeline, and one built with `inpaint_unet=True` on the
              9-channel pipeline, every request of it an inpainting request (4-channel latents as `image`, its own mask and
              `masked_image_latents`).  8 slots kept full, three alternating rounds: images/s and steps/s of both; then
              one-at-a-time `inpaiting(fused=True)` beside `fused=False` at 512x512 for 25 steps, ms per image, three runs of
              four; then the device time of dsc_cfg_linear_step_rows_cat beside dsc_cfg_linear_step_rows at 8 slots of 64x64
              latents (a captured graph of 100 launches each, three replays)
  freeu       (--freeu: this leg only) two batchers on two slots: one built without `freeu`, one with it.  8 slots kept full, three
              alternating rounds of (a) the flagless batcher, (b) the same requests on the freeu=True batcher (every row's values
              are ones: the six launches per step return at once - the price of the flag), (c) every other request with
              `freeu=(0.9, 0.2, 1.5, 1.6)`; images/s and steps/s for each
  pixels      (--pixels [--encode-batch E, default 2] [--inpaint-unet]: this leg only) an SD1.x-size VAE with seeded random
              weights in the pipeline, then two batchers on two slots: one built without `encode` (pixel inputs are prepared inline
              inside submit, on the batch's stream) and one built with `encode=True, encode_batch=E` (the encode lane).  Every
              request is img2img at strength 0.6 (with --inpaint-unet: an inpainting request of a 9-channel UNet without
              `masked_image_latents`, two encodes each).  8 slots kept full, three alternating rounds of (a) 4-channel latents as
              `image` on the flagless batcher, (b) the same requests with a PIL image (and PIL mask) on the flagless batcher, (c)
              the same on the encode-lane batcher; images/s, p50 / p95 of submit -> resolved and the wall time of `submit` itself
              for each; then the same three legs with each batcher driven by its own thread
  prompts     (--prompts [--text-batch E, default 2]: this leg only) a CLIP-L-size native text encoder with seeded random weights
              in the pipeline, then two batchers on two slots: one built without `text` and one built with `text=True,
              text_batch=E` (the text lane).  The same requests three ways, 8 slots kept full, three alternating rounds: (a)
              embeddings and ids precomputed, (b) `encode_prompt_function` called in the client in front of every submit - the
              path of a flagless batcher -, (c) `prompt` strings on the text-lane batcher; images/s, p50 of submit -> resolved and
              the wall time of the client's work plus `submit` for each; then the same with each batcher driven by its own
              thread, one request at a time on an idle batcher, and the device time of one captured encode per lane bucket
"""
import argparse
import json
import os
import random
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from inputs import FakeTokenizer  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def make_requests(n, seed):
    tok = FakeTokenizer()
    out = []
    for i in range(n):
        regions = (2, 1, 4)[i % 3]
        words = [f"object{r}a object{r}b" for r in range(regions)]
        ids = [49406, 320]
        for w in words:
            ids += tok(w).input_ids
        ids = ids + [49407] * (77 - len(ids))
        pos = np.array([ids], dtype=np.int64)
        state = {}
        for r, w in enumerate(words):
            m = np.full((512, 512), 255, dtype=np.uint8)
            x0, x1 = (r * 8) // regions, ((r + 1) * 8) // regions
            m[128:384, x0 * 64:x1 * 64] = 0
            state[w] = {"map": m, "weight": 0.5, "mask_outsides": 0.0}
        emb = torch.randn(2, 77, 768, generator=torch.Generator().manual_seed(seed * 1000 + 70 + i)).half().cuda()
        lat = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(seed * 1000 + 1000 + i)).half().cuda()
        out.append({"prompt_embeds": emb[1:2], "negative_prompt_embeds": emb[0:1], "text_input_ids": [pos.copy(), pos],
                    "region_map_state": state, "latents": lat})
    return out


def make_mixed(reqs, seed):
    """request i: txt2img / img2img at strength 0.6 / inpainting (i % 3), its own image latents and its own mask"""
    out = []
    for i, r in enumerate(reqs):
        g = torch.Generator().manual_seed(seed * 1000 + 2000 + i)
        img = (torch.randn(1, 4, 64, 64, generator=g) * 0.8).half().cuda()
        if i % 3 == 0:
            out.append(dict(r))
        elif i % 3 == 1:
            out.append(dict(r, image=img, strength=0.6))
        else:
            m = torch.zeros(1, 1, 512, 512)
            x0 = 64 * (i % 7)
            m[..., x0:x0 + 192] = 1.0                       # repaint a 192-pixel column band, elsewhere keep the image
            out.append(dict(r, image=img, mask_image=m, strength=1.0))
    return out


def make_inpaint(reqs, seed):
    """every request an inpainting request of a 9-channel UNet: its own image latents, mask and masked-image latents"""
    out = []
    for i, r in enumerate(reqs):
        g = torch.Generator().manual_seed(seed * 1000 + 6000 + i)
        img = (torch.randn(1, 4, 64, 64, generator=g) * 0.8).half().cuda()
        mil = (torch.randn(1, 4, 64, 64, generator=g) * 0.8).half().cuda()
        m = torch.zeros(1, 1, 512, 512)
        x0 = 64 * (i % 6)
        m[..., x0:x0 + 192] = 1.0                           # repaint a 192-pixel column band
        out.append(dict(r, image=img, mask_image=m, masked_image_latents=mil, strength=1.0))
    return out


def graph_launch_us(fn, launches=100, replays=3):
    """device microseconds per launch of `fn` (one sampler launch): a captured graph of `launches` of them, timed per replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(round(1e3 * e0.elapsed_time(e1) / launches, 3))
    return out


def step_rows_kernel_us(rounds=3):
    """device microseconds per launch of the per-row sampler entries on 8 STEP slots of a 4 x 64 x 64 latent, `rounds`
    alternating figures each -> (slots, extra_halfs, {entry: [us, ...]}).  One slot of the rescale entry has phi > 0 (its row
    belongs to one workgroup), one slot of the known entry a known region with both blends on; the staged entry runs once with
    every slot PREDICT and once with every slot CORRECT"""
    from diffusionspatialcontrol_amd import ops
    n, chw, eh = 8, 4 * 64 * 64, 5 * 64 * 64
    h = lambda *shape: torch.randn(*shape, device="cuda").half()      # noqa: E731
    x, eps, old = h(n, chw), h(2 * n, chw), h(n, chw)
    t, sg = torch.zeros(2 * n, device="cuda"), torch.ones(n, device="cuda")
    x4, x9 = torch.zeros(2 * n, chw, device="cuda").half(), torch.zeros(2 * n, chw + eh, device="cuda").half()
    ex = [h(eh) for _ in range(n)]
    recs = [{"mode": ops.ROW_STEP, "sigma": 2.0, "guidance": 7.5, "a": 1.0, "b": 0.0, "c": 0.0, "c_skip": 1.0, "c_out": -2.0,
             "c_in_next": 0.4, "t_next": 500.0, "sigma_next": 1.5} for _ in range(n)]      # (a = 1, b = c = 0: x stays x)
    resc = [dict(recs[0], rescale=0.7)] + recs[1:]
    known = [{"image": h(chw), "noise": h(chw), "mask": (torch.rand(chw, device="cuda") < 0.5).half(), "blend_now": True,
              "blend_next": True}] + [None] * (n - 1)
    mid = h(n, chw)
    pred = [dict(r, stage=ops.ROW_STAGE_PREDICT) for r in recs]
    corr = [dict(r, stage=ops.ROW_STAGE_CORRECT, m=0.0) for r in recs]
    entries = {"cfg_dpmpp2m_step_rows": lambda: ops.cfg_dpmpp2m_step_rows(x, eps, old, n, x4, t, sg, recs),
               "cfg_dpmpp2m_step_rows_known": lambda: ops.cfg_dpmpp2m_step_rows_known(x, eps, old, n, x4, t, sg, recs, known),
               "cfg_linear_step_rows": lambda: ops.cfg_linear_step_rows(x, eps, old, n, x4, t, sg, recs),
               "cfg_linear_step_rows_rescale": lambda: ops.cfg_linear_step_rows_rescale(x, eps, old, n, x4, t, sg, resc),
               "cfg_linear_step_rows_cat": lambda: ops.cfg_linear_step_rows_cat(x, eps, old, n, x9, t, sg, recs, ex),
               "cfg_staged_step_rows_predict": lambda: ops.cfg_staged_step_rows(x, mid, eps, old, n, x4, t, sg, pred),
               "cfg_staged_step_rows_correct": lambda: ops.cfg_staged_step_rows(x, mid, eps, old, n, x4, t, sg, corr)}
    us = {name: [] for name in entries}
    for _ in range(rounds):
        for name, fn in entries.items():
            us[name] += graph_launch_us(fn, replays=1)
    return n, eh, us


def run_full(b, reqs, kw):
    """(images/s, sampler steps/s) of one batcher with its slots kept full by these requests"""
    torch.cuda.synchronize()
    s0 = b.stats()["steps"]
    t0 = time.perf_counter()
    futs = [b.submit(dict(r, **kw)) for r in reqs]
    b.run_until_idle()
    for f in futs:
        f.result()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return len(reqs) / dt, (b.stats()["steps"] - s0) / dt


def run_full_latency(b, reqs, kw):
    """run_full, also giving the requests' submit -> resolved latencies: (images/s, p50 s, p95 s)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    futs = [b.submit(dict(r, **kw)) for r in reqs]
    b.run_until_idle()
    for f in futs:
        f.result()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lat = [f.dsc_latency_s for f in futs]
    return len(reqs) / dt, pct(lat, 50), pct(lat, 95)


def run_started_latency(b, reqs, kw):
    """run_full_latency with the batcher driven by its own thread (start / stop): (images/s, p50 s, p95 s)"""
    torch.cuda.synchronize()
    b.start()
    t0 = time.perf_counter()
    futs = [b.submit(dict(r, **kw)) for r in reqs]
    for f in futs:
        f.result()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    b.stop()
    lat = [f.dsc_latency_s for f in futs]
    return len(reqs) / dt, pct(lat, 50), pct(lat, 95)


def run_submit_latency(b, reqs, kw, started=False):
    """run_full_latency / run_started_latency, also timing every `submit` call on the caller's thread:
    (images/s, p50 s, p95 s, mean submit ms, max submit ms)"""
    torch.cuda.synchronize()
    if started:
        b.start()
    t0 = time.perf_counter()
    futs, took = [], []
    for r in reqs:
        s0 = time.perf_counter()
        futs.append(b.submit(dict(r, **kw)))
        took.append(1e3 * (time.perf_counter() - s0))
    if started:
        for f in futs:
            f.result()
    else:
        b.run_until_idle()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if started:
        b.stop()
    lat = [f.dsc_latency_s for f in futs]
    return len(reqs) / dt, pct(lat, 50), pct(lat, 95), sum(took) / len(took), max(took)


def run_client_latency(b, reqs, kw, started, client):
    """run_submit_latency with `client(request)` run on the caller's thread in front of every submit and timed with it:
    (images/s, p50 s of submit -> resolved, mean ms and max ms of client + submit)"""
    torch.cuda.synchronize()
    if started:
        b.start()
    t0 = time.perf_counter()
    futs, took = [], []
    for r in reqs:
        s0 = time.perf_counter()
        futs.append(b.submit(dict(client(r), **kw)))
        took.append(1e3 * (time.perf_counter() - s0))
    if started:
        for f in futs:
            f.result()
    else:
        b.run_until_idle()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if started:
        b.stop()
    return len(reqs) / dt, pct([f.dsc_latency_s for f in futs], 50), sum(took) / len(took), max(took)


def make_prompts(reqs):
    """the requests as prompt strings: the region words of make_requests with emphasis around them, a short negative prompt"""
    out = []
    for i, r in enumerate(reqs):
        words = ", ".join(f"({w}:1.{1 + i % 4})" if j % 2 == 0 else f"[{w}]" for j, w in enumerate(r["region_map_state"]))
        out.append({"prompt": f"a photo of {words}, ((sharp)) focus", "negative_prompt": "blurry, (low quality:1.3)",
                    "region_map_state": r["region_map_state"], "latents": r["latents"]})
    return out


def make_pixels(reqs, seed, inpaint):
    """(latent-input requests, the same requests with PIL pixels): img2img at strength 0.6, or (`inpaint`) inpainting requests of
    a 9-channel UNet - latents with `masked_image_latents` against a PIL image and a PIL mask"""
    from PIL import Image
    lat, pix = [], []
    for i, r in enumerate(reqs):
        g = torch.Generator().manual_seed(seed * 1000 + 8000 + i)
        img = (torch.randn(1, 4, 64, 64, generator=g) * 0.8).half().cuda()
        pil = Image.fromarray(torch.randint(96, 160, (512, 512, 3), generator=g, dtype=torch.uint8).numpy())
        if inpaint:
            mil = (torch.randn(1, 4, 64, 64, generator=g) * 0.8).half().cuda()
            m = torch.zeros(512, 512, dtype=torch.uint8)
            x0 = 64 * (i % 6)
            m[:, x0:x0 + 192] = 255
            lat.append(dict(r, image=img, mask_image=m[None, None].float() / 255, masked_image_latents=mil, strength=1.0))
            pix.append(dict(r, image=pil, mask_image=Image.fromarray(m.numpy(), "L"), strength=1.0))
        else:
            lat.append(dict(r, image=img, strength=0.6))
            pix.append(dict(r, image=pil, strength=0.6))
    return lat, pix


def pct(v, p):
    return float(np.percentile(np.array(v), p)) if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=16)
    ap.add_argument("--rates", default="2,6", help="Poisson arrival rates, requests/s")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mix", action="store_true", help="only the mixed txt2img / img2img / inpainting leg")
    ap.add_argument("--sampler", default=None, help="only the saturated leg with every other request on this sampler "
                                                    "(sample_euler, sample_euler_ancestral, sample_dpmpp_2m_sde, sample_lcm; a "
                                                    "two-call sampler - sample_heun, sample_dpm_2, sample_dpm_2_ancestral, "
                                                    "sample_dpmpp_2s_ancestral, sample_dpmpp_sde - builds the batcher with two_call=True)")
    ap.add_argument("--two-call", action="store_true",
                    help="the saturated sampler leg on a batcher built with two_call=True (alone: no request names a two-call "
                         "sampler); --kernels: only the device time of the per-row sampler entries, the staged one included")
    ap.add_argument("--kernels", action="store_true", help="with --two-call: only the per-row sampler entries' device time")
    ap.add_argument("--guidance-rescale", type=float, default=None, metavar="PHI",
                    help="only the saturated leg with guidance_rescale = PHI (in (0, 1]) on every other request")
    ap.add_argument("--hires", type=float, default=None, metavar="X",
                    help="only the hires leg: a chained pair, every other request with upscale_x = X (1.0 .. 2.0)")
    ap.add_argument("--ip-adapter", action="store_true",
                    help="only the IP-Adapter leg: every other request carries an image prompt (random adapter weights, 4 tokens)")
    ap.add_argument("--ip-masks", action="store_true",
                    help="with --ip-adapter: also a mask-capable batcher, every other image-prompt request with a half-image mask")
    ap.add_argument("--t2i-adapter", action="store_true",
                    help="only the T2I-Adapter leg: every other request carries a control image with factor 0.5 (random weights)")
    ap.add_argument("--controlnet", action="store_true",
                    help="only the ControlNet leg: every other request carries a control image (random weights, SD1.5 size)")
    ap.add_argument("--control-slots", type=int, default=4, help="with --controlnet: the ControlNet lanes of the batcher")
    ap.add_argument("--images", choices=("uint8", "pil", "np"), default=None,
                    help="only the finished-images leg: latent output, this image type inline, this image type on the decode lane")
    ap.add_argument("--decode-batch", type=int, default=2, help="with --images: rows per captured decode of the lane")
    ap.add_argument("--previews", type=int, default=None, metavar="K",
                    help="only the previews leg: every request with preview_every = K and a no-op callback")
    ap.add_argument("--preview-scale", type=int, default=8, help="with --previews: the thumbnails' enlargement (1, 2, 4, 8)")
    ap.add_argument("--inpaint-unet", action="store_true",
                    help="only the 9-channel inpainting UNet leg: a batcher built with inpaint_unet=True, every request inpainting")
    ap.add_argument("--pixels", action="store_true",
                    help="only the pixel-input leg: latents as `image`, pixels inline on a flagless batcher, pixels on the encode lane "
                         "(with --inpaint-unet: inpainting requests of a 9-channel UNet)")
    ap.add_argument("--encode-batch", type=int, default=2, help="with --pixels: rows per captured encode of the lane")
    ap.add_argument("--freeu", action="store_true",
                    help="only the FreeU leg: a flagless batcher, a freeu=True batcher without FreeU requests, and the same with "
                         "freeu=(0.9, 0.2, 1.5, 1.6) on every other request")
    ap.add_argument("--prompts", action="store_true",
                    help="only the prompt-string leg: embeddings precomputed, encode_prompt_function in the client before each "
                         "submit, and `prompt` strings on a text=True batcher (a CLIP-L-size native text encoder, random weights)")
    ap.add_argument("--text-batch", type=int, default=2, help="with --prompts: (request, chunk) groups per encode of the lane")
    a = ap.parse_args()
    if a.ip_masks and not a.ip_adapter:
        ap.error("--ip-masks goes with --ip-adapter")
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(0)
    with torch.device("cuda"):
        unet = UNet2DConditionModel(UNetConfig.sd15())
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet.half().eval(), SD15Scheduler())
    opt = {"scheduler": "karras"}
    reqs = make_requests(a.requests, a.seed)
    kw25 = dict(num_inference_steps=25, guidance_scale=7.5, sampler_opt=opt)

    if a.prompts:
        from inputs import FakeClipTokenizer
        from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel
        from diffusionspatialcontrol_amd.modules.encoder_prompt_modify import encode_prompt_function
        torch.manual_seed(a.seed + 17)
        clip = CLIPTextModel(dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                                  num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                                  eos_token_id=49407))
        with torch.no_grad():                             # a trained final LayerNorm has a bias: the restored mean is not ~0
            clip.final_layer_norm.bias.copy_(torch.rand(768) * 0.5 - 0.35)
        pipe.text_encoder, pipe.tokenizer = clip.half().cuda().eval(), FakeClipTokenizer()
        plain = pipe.serve(512, 512, max_batch=8, slot=0).warm()
        lane = pipe.serve(512, 512, max_batch=8, slot=1, text=True, text_batch=a.text_batch).warm()
        texts = make_prompts(reqs)
        given = [dict(t, **lane.encode_text(t["prompt"], t["negative_prompt"])) for t in texts]
        given = [{k: v for k, v in g.items() if k not in ("prompt", "negative_prompt")} for g in given]
        dev = pipe._execution_device

        def in_client(t):
            with torch.no_grad():
                pos, neg, ids = encode_prompt_function(pipe, t["prompt"], dev, 1, True, t["negative_prompt"], long_encode=0)
            return {"prompt_embeds": pos, "negative_prompt_embeds": neg, "text_input_ids": ids,
                    "region_map_state": t["region_map_state"], "latents": t["latents"]}

        legs = (("a_embeds_precomputed", plain, given, lambda r: r), ("b_encode_in_client", plain, texts, in_client),
                ("c_prompt_text_lane", lane, texts, lambda r: r))
        for started, name in ((False, "prompts"), (True, "prompts_driver_thread")):
            for _, b, group, client in legs:              # one untimed pass each (allocator, kernel selection, the eager encoder)
                run_client_latency(b, group[:8], kw25, started, client)
            before = lane.stats()
            runs = []
            for _ in range(3):                            # alternating, so that a drift of the box hits all alike
                runs.append({leg: run_client_latency(b, group, kw25, started, client) for leg, b, group, client in legs})
            after = lane.stats()
            emit(leg=name, requests=len(reqs), steps=25, text_batch=a.text_batch,
                 **{f"{leg}_img_s": [round(r[leg][0], 3) for r in runs] for leg, *_ in legs},
                 **{f"{leg}_p50_s": [round(r[leg][1], 3) for r in runs] for leg, *_ in legs},
                 **{f"{leg}_submit_ms_mean": [round(r[leg][2], 2) for r in runs] for leg, *_ in legs},
                 **{f"{leg}_submit_ms_max": [round(r[leg][3], 2) for r in runs] for leg, *_ in legs},
                 text_encodes=after["text_encodes"] - before["text_encodes"], text_groups=after["text_groups"] - before["text_groups"],
                 captures_after_warm=after["captures_after_warm"],
                 note="three alternating rounds in one process, 8 slots kept full; " +
                      ("each batcher driven by its own thread (start / stop)" if started else
                       "each batcher stepped by the caller's thread (run_until_idle)") +
                      "; latency = submit -> future resolved (dsc_latency_s); submit_ms = wall time of the client's work in front "
                      "of submit (leg b: encode_prompt_function) plus the submit call itself")
        lone = {}
        for leg, b, group, client in legs:                # lone arrivals: one request at a time on an idle batcher
            took = []
            for r in group[:6]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fut = b.submit(dict(client(r), **kw25))
                b.run_until_idle()
                fut.result()
                took.append(time.perf_counter() - t0)
            lone[leg] = round(1e3 * float(np.median(took)), 2)
        emit(leg="prompts_lone_arrival", ms_submit_to_result_median=lone,
             note="one request on an idle batcher, stepped by the caller: client work + submit + 25 steps, median of 6")
        per = {}
        for g, st in lane.exec.text_lane.st.items():      # one captured encode, device time
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(lane.exec.text_lane.stream):
                st["run"]()
                e0.record()
                for _ in range(10):
                    st["run"]()
                e1.record()
            torch.cuda.synchronize()
            per[g] = round(e0.elapsed_time(e1) / 10, 3)
        emit(leg="prompts_encode_replay", encode_graph_gpu_ms_per_bucket=per,
             note="ten back-to-back replays of the encoder's graph on the lane's stream with nothing else running; bucket g "
                  "encodes [2 g, 77] ids")
        emit(leg="stats", flagless=plain.stats(), text_lane=lane.stats())
        return

    if a.pixels:
        from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKL
        serving = pipe
        more = {}
        if a.inpaint_unet:
            import dataclasses
            torch.manual_seed(1)
            with torch.device("cuda"):
                unet9 = UNet2DConditionModel(dataclasses.replace(UNetConfig.sd15(), in_channels=9))
            serving = StableDiffusionPipeline(None, None, FakeTokenizer(), unet9.half().eval(), SD15Scheduler())
            more = {"inpaint_unet": True}
        torch.manual_seed(a.seed + 13)
        with torch.device("cuda"):
            vae = AutoencoderKL()
        serving.vae = vae.half().eval()
        plain = serving.serve(512, 512, max_batch=8, slot=0, **more).warm()
        lane = serving.serve(512, 512, max_batch=8, slot=1, encode=True, encode_batch=a.encode_batch, **more).warm()
        lat_reqs, pix_reqs = make_pixels(reqs, a.seed, a.inpaint_unet)
        legs = (("a_latents_flagless", plain, lat_reqs), ("b_pixels_inline", plain, pix_reqs), ("c_pixels_encode_lane", lane, pix_reqs))
        for started, name in ((False, "pixels"), (True, "pixels_driver_thread")):
            for _, b, group in legs:                      # one untimed pass each (allocator, kernel selection, the inline encoder)
                run_submit_latency(b, group[:8], kw25, started)
            before = lane.stats()
            runs = []
            for _ in range(3):                            # alternating, so that a drift of the box hits all alike
                runs.append({leg: run_submit_latency(b, group, kw25, started) for leg, b, group in legs})
            after = lane.stats()
            emit(leg=name, requests=len(reqs), steps=25, kind="inpaint_unet 1.0" if a.inpaint_unet else "img2img 0.6",
                 encode_batch=a.encode_batch,
                 **{f"{leg}_img_s": [round(r[leg][0], 3) for r in runs] for leg, _, _ in legs},
                 **{f"{leg}_p50_s": [round(r[leg][1], 3) for r in runs] for leg, _, _ in legs},
                 **{f"{leg}_p95_s": [round(r[leg][2], 3) for r in runs] for leg, _, _ in legs},
                 **{f"{leg}_submit_ms_mean": [round(r[leg][3], 2) for r in runs] for leg, _, _ in legs},
                 **{f"{leg}_submit_ms_max": [round(r[leg][4], 2) for r in runs] for leg, _, _ in legs},
                 encodes=after["encodes"] - before["encodes"], encode_rows=after["encode_rows"] - before["encode_rows"],
                 captures_after_warm=after["captures_after_warm"],
                 note="three alternating rounds in one process, 8 slots kept full; " +
                      ("each batcher driven by its own thread (start / stop)" if started else
                       "each batcher stepped by the caller's thread (run_until_idle)") +
                      "; latency = submit -> future resolved (dsc_latency_s); submit_ms = wall time of the submit call itself")
        per = {}
        for m, st in lane.exec.enc_lane.st.items():      # one captured encode, device time
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(lane.exec.enc_lane.stream):
                st["run"]()
                e0.record()
                for _ in range(10):
                    st["run"]()
                e1.record()
            torch.cuda.synchronize()
            per[m] = round(e0.elapsed_time(e1) / 10, 3)
        emit(leg="pixels_encode_replay", encode_graph_gpu_ms_per_bucket=per,
             note="ten back-to-back replays on the lane's stream with nothing else running")
        emit(leg="stats", flagless=plain.stats(), encode_lane=lane.stats())
        return

    if a.freeu:
        plain = pipe.serve(512, 512, max_batch=8, slot=0).warm()
        on = pipe.serve(512, 512, max_batch=8, slot=1, freeu=True).warm()
        every_other = [dict(r, freeu=(0.9, 0.2, 1.5, 1.6)) if i % 2 else r for i, r in enumerate(reqs)]
        for b in (plain, on):                             # one untimed pass each
            run_full(b, reqs[:8], kw25)
        runs = []
        for _ in range(3):                                # alternating, so that a drift of the box hits all three alike
            runs.append((run_full(plain, reqs, kw25), run_full(on, reqs, kw25), run_full(on, every_other, kw25)))
        emit(leg="freeu", requests=len(reqs), steps=25,
             flagless_img_s=[round(t[0][0], 2) for t in runs], flag_no_freeu_requests_img_s=[round(t[1][0], 2) for t in runs],
             flag_every_other_request_img_s=[round(t[2][0], 2) for t in runs],
             flagless_steps_s=[round(t[0][1], 1) for t in runs], flag_no_freeu_requests_steps_s=[round(t[1][1], 1) for t in runs],
             flag_every_other_request_steps_s=[round(t[2][1], 1) for t in runs],
             freeu_updates=on.stats()["freeu_updates"], captures_after_warm=on.stats()["captures_after_warm"],
             note="three alternating rounds in one process, 8 slots kept full; the freeu=True step holds six dsc_freeu_rows_f16 "
                  "launches, which skip rows whose values are (1, 1, 1, 1)")
        emit(leg="stats", flagless=plain.stats(), freeu=on.stats())
        return

    if a.inpaint_unet:
        import dataclasses
        torch.manual_seed(1)
        with torch.device("cuda"):
            unet9 = UNet2DConditionModel(dataclasses.replace(UNetConfig.sd15(), in_channels=9))
        pipe9 = StableDiffusionPipeline(None, None, FakeTokenizer(), unet9.half().eval(), SD15Scheduler())
        plain = pipe.serve(512, 512, max_batch=8, slot=0).warm()
        inp = pipe9.serve(512, 512, max_batch=8, slot=1, inpaint_unet=True).warm()
        ireqs = make_inpaint(reqs, a.seed)
        for b, group in ((plain, reqs[:8]), (inp, ireqs[:8])):      # one untimed pass each
            run_full(b, group, kw25)
        runs = []
        for _ in range(3):                                # alternating, so that a drift of the box hits both alike
            runs.append((run_full(plain, reqs, kw25), run_full(inp, ireqs, kw25)))
        emit(leg="inpaint_unet", requests=len(reqs), steps=25,
             four_channel_txt2img_img_s=[round(t[0][0], 2) for t in runs], four_channel_txt2img_steps_s=[round(t[0][1], 1) for t in runs],
             nine_channel_inpaint_img_s=[round(t[1][0], 2) for t in runs], nine_channel_inpaint_steps_s=[round(t[1][1], 1) for t in runs],
             cat_transitions=inp.stats()["cat_transitions"], captures_after_warm=inp.stats()["captures_after_warm"],
             note="three alternating rounds in one process, two UNets of the same shape but for conv_in (36 against 81 taps)")
        r = ireqs[0]
        one = dict(height=512, width=512, sampler_name="sample_dpmpp_2m", image=r["image"], mask_image=r["mask_image"],
                   masked_image_latents=r["masked_image_latents"], latents=r["latents"], region_map_state=r["region_map_state"],
                   prompt_embeds=r["prompt_embeds"], negative_prompt_embeds=r["negative_prompt_embeds"],
                   text_input_ids=r["text_input_ids"], output_type="latent", **kw25)
        ms = {True: [], False: []}
        for mode in (True, False):
            pipe9.inpaiting(None, fused=mode, **one)
        for _ in range(3):
            for mode in (True, False):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(4):
                    pipe9.inpaiting(None, fused=mode, **one)
                torch.cuda.synchronize()
                ms[mode].append(round(1e3 * (time.perf_counter() - t0) / 4, 2))
        emit(leg="inpaint_unet_one_at_a_time", steps=25, size="512x512", fused_ms_per_image=ms[True], protocol_ms_per_image=ms[False],
             note="inpaiting(fused=True) against fused=False (eager protocol mode) on the 9-channel UNet, three alternating runs of four")
        n, eh, us = step_rows_kernel_us()
        emit(leg="inpaint_unet_kernel", slots=n, latent="4x64x64", extra_halfs=eh, device_us_per_launch=us,
             note="a captured graph of 100 launches per figure, alternating; one slot of the rescale entry has phi > 0 and one of the "
                  "known entry a known region; the cat entry reads 5/4 and writes 10/4 of a latent more")
        emit(leg="stats", four_channel=plain.stats(), nine_channel=inp.stats())
        return

    if a.previews:
        plain = pipe.serve(512, 512, max_batch=8, slot=0).warm()
        live = pipe.serve(512, 512, max_batch=8, slot=1, previews=True, preview_scale=a.preview_scale).warm()
        made = [0]

        def on_preview(step, steps, image):
            made[0] += 1

        asking = dict(kw25, preview_every=a.previews, on_preview=on_preview)
        legs = (("a_flagless", plain, kw25), ("b_previews_none_asked", live, kw25), ("c_previews_every_k", live, asking))
        for _, b, kw in legs:                             # one untimed pass each (allocator, kernel selection, the ring)
            run_full_latency(b, reqs[:8], kw)
        before, made[0] = live.stats(), 0
        runs = []
        for _ in range(3):                                # alternating, so that a drift of the box hits all alike
            runs.append({name: run_full_latency(b, reqs, kw) for name, b, kw in legs})
        after = live.stats()
        counters = ("previews", "preview_rows", "previews_dropped", "preview_callback_errors")
        emit(leg="previews", requests=len(reqs), steps=25, preview_every=a.previews, preview_scale=a.preview_scale,
             **{f"{name}_img_s": [round(r[name][0], 3) for r in runs] for name, _, _ in legs},
             **{f"{name}_p50_s": [round(r[name][1], 3) for r in runs] for name, _, _ in legs},
             **{f"{name}_p95_s": [round(r[name][2], 3) for r in runs] for name, _, _ in legs},
             **{k: after[k] - before[k] for k in counters}, callbacks=made[0], captures_after_warm=after["captures_after_warm"],
             note="three alternating rounds in one process, each batcher stepped by the caller's thread (run_until_idle); the counters "
                  "are those of the three timed (c) runs together")
        run_started_latency(live, reqs[:8], asking)
        before, made[0] = live.stats(), 0
        runs = [run_started_latency(live, reqs, asking) for _ in range(3)]
        after = live.stats()
        emit(leg="previews_driver_thread", requests=len(reqs), steps=25, preview_every=a.previews, preview_scale=a.preview_scale,
             c_previews_every_k_img_s=[round(r[0], 3) for r in runs], c_previews_every_k_p50_s=[round(r[1], 3) for r in runs],
             c_previews_every_k_p95_s=[round(r[2], 3) for r in runs], **{k: after[k] - before[k] for k in counters},
             callbacks=made[0], captures_after_warm=after["captures_after_warm"],
             note="the (c) run with the batcher driven by its own thread (start / stop), three runs")
        emit(leg="stats", flagless=plain.stats(), previews=live.stats())
        return

    if a.images:
        from diffusionspatialcontrol_amd.modules.vae_decoder import AutoencoderKLDecoder
        torch.manual_seed(a.seed + 11)
        with torch.device("cuda"):
            vae = AutoencoderKLDecoder()
        pipe.vae = vae.half().eval()
        plain = pipe.serve(512, 512, max_batch=8, slot=0).warm()
        lane = pipe.serve(512, 512, max_batch=8, slot=1, decode=True, decode_batch=a.decode_batch).warm()
        # the flagless batcher has never heard of "uint8": its nearest inline equivalent is the PIL image (the same bytes)
        inline_type = "pil" if a.images == "uint8" else a.images
        legs = (("a_latent_flagless", plain, "latent"), ("b_image_inline", plain, inline_type),
                ("c_image_decode_lane", lane, a.images), ("d_latent_decode_lane", lane, "latent"))
        for _, b, out_type in legs:                       # one untimed pass each (allocator, kernel selection, the inline decoder)
            run_full_latency(b, reqs[:8], dict(kw25, output_type=out_type))
        before = lane.stats()
        runs = []
        for _ in range(3):                                # alternating, so that a drift of the box hits all alike
            runs.append({name: run_full_latency(b, reqs, dict(kw25, output_type=out_type)) for name, b, out_type in legs})
        after = lane.stats()
        emit(leg="images", requests=len(reqs), steps=25, image_type=a.images, inline_type=inline_type, decode_batch=a.decode_batch,
             **{f"{name}_img_s": [round(r[name][0], 2) for r in runs] for name, _, _ in legs},
             **{f"{name}_p50_s": [round(r[name][1], 3) for r in runs] for name, _, _ in legs},
             **{f"{name}_p95_s": [round(r[name][2], 3) for r in runs] for name, _, _ in legs},
             decodes=after["decodes"] - before["decodes"], decode_rows=after["decode_rows"] - before["decode_rows"],
             captures_after_warm=after["captures_after_warm"],
             note="three alternating rounds in one process, each batcher stepped by the caller's thread (run_until_idle); latency = "
                  "submit -> future resolved (dsc_latency_s), the queueing of requests 9..16 behind the first eight included")
        # the same four legs with each batcher driven by its own thread (start / stop), mixed step counts so that rows leave one
        # or two at a time instead of a wave of eight
        rng = random.Random(a.seed)
        mixed = [dict(r, num_inference_steps=rng.choice((20, 25, 30))) for r in reqs]
        kwm = dict(guidance_scale=7.5, sampler_opt=opt)
        for _, b, out_type in legs:
            run_started_latency(b, mixed[:8], dict(kwm, output_type=out_type))
        runs = []
        for _ in range(3):
            runs.append({name: run_started_latency(b, mixed, dict(kwm, output_type=out_type)) for name, b, out_type in legs})
        emit(leg="images_driver_thread", requests=len(reqs), steps="20 / 25 / 30 mixed", image_type=a.images, inline_type=inline_type,
             decode_batch=a.decode_batch,
             **{f"{name}_img_s": [round(r[name][0], 2) for r in runs] for name, _, _ in legs},
             **{f"{name}_p50_s": [round(r[name][1], 3) for r in runs] for name, _, _ in legs},
             **{f"{name}_p95_s": [round(r[name][2], 3) for r in runs] for name, _, _ in legs},
             captures_after_warm=lane.stats()["captures_after_warm"],
             note="as the `images` leg, but each batcher is driven by its own thread and the requests have mixed step counts")
        per = {}
        for m, st in lane.exec.lane.st.items():          # one captured decode (scale, decoder, both finishes), device time
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(lane.exec.lane.stream):
                st["run"]()
                e0.record()
                for _ in range(10):
                    st["run"]()
                e1.record()
            torch.cuda.synchronize()
            per[m] = round(e0.elapsed_time(e1) / 10, 3)
        emit(leg="images_decode_replay", decode_graph_gpu_ms_per_bucket=per,
             note="ten back-to-back replays on the lane's stream with nothing else running")
        emit(leg="stats", flagless=plain.stats(), decode_lane=lane.stats())
        return

    if a.controlnet:
        from diffusionspatialcontrol_amd.modules.controlnet import ControlNetModel
        torch.manual_seed(a.seed + 9)
        with torch.device("cuda"):
            cn = ControlNetModel(UNetConfig.sd15())
        for conv in list(cn.controlnet_down_blocks) + [cn.controlnet_mid_block, cn.controlnet_cond_embedding.conv_out]:
            torch.nn.init.normal_(conv.weight, 0.0, 0.02)                  # (zero convolutions would make every residual zero)
        pipe.setup_controlnet(cn.half().eval())
        off = pipe.serve(512, 512, max_batch=8, slot=0).warm()
        on = pipe.serve(512, 512, max_batch=8, slot=1, controlnet=True, control_slots=a.control_slots).warm()
        images = [torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(a.seed * 1000 + 5000 + i)) for i in range(len(reqs))]
        mixed = [dict(r, control_img=images[i], controlnet_conditioning_scale=0.9, control_guidance_start=0.0,
                      control_guidance_end=0.6) if i % 2 else dict(r) for i, r in enumerate(reqs)]
        for b, group in ((off, reqs[:8]), (on, reqs[:8]), (on, mixed[:8])):     # one untimed pass each
            run_full(b, group, kw25)
        runs = []
        s_before = on.stats()
        for _ in range(3):                                # alternating, so that a drift of the box hits all alike
            runs.append((run_full(off, reqs, kw25), run_full(on, reqs, kw25), run_full(on, mixed, kw25)))
        s_after = on.stats()
        emit(leg="controlnet", requests=len(reqs), steps=25, control_slots=a.control_slots,
             mix="every other request with a control image, scale 0.9, window [0, 0.6] (15 of 25 model calls)",
             flag_off_plain_img_s=[round(t[0][0], 2) for t in runs], flag_on_plain_img_s=[round(t[1][0], 2) for t in runs],
             flag_on_every_other_with_control_img_s=[round(t[2][0], 2) for t in runs],
             flag_off_plain_steps_s=[round(t[0][1], 1) for t in runs], flag_on_plain_steps_s=[round(t[1][1], 1) for t in runs],
             flag_on_every_other_with_control_steps_s=[round(t[2][1], 1) for t in runs],
             control_steps=s_after["control_steps"] - s_before["control_steps"], steps_in_those_rounds=s_after["steps"] - s_before["steps"],
             control_gate_updates=s_after["control_gate_updates"] - s_before["control_gate_updates"],
             captures_after_warm=on.stats()["captures_after_warm"],
             note="three alternating rounds in one process; the flag-off batcher captures the step of a pipeline without the feature; "
                  "with fewer lanes than control requests the later ones wait in the queue (FIFO)")
        # one ControlNet replay (all 2 c lane rows) and one bucket-8 step, device time
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        with torch.cuda.stream(on.exec.stream):
            e0.record()
            for _ in range(10):
                on.exec.run_control(8)
            e1.record()
            for _ in range(10):
                on.exec.run(8)
            e2.record()
        torch.cuda.synchronize()
        emit(leg="controlnet_replay", control_slots=a.control_slots, lane_rows=2 * a.control_slots,
             controlnet_replay_gpu_ms=round(e0.elapsed_time(e1) / 10, 3), bucket8_step_gpu_ms=round(e1.elapsed_time(e2) / 10, 3),
             note="ten back-to-back replays each on the batch's stream (gather launches included), every lane idle in the step")
        # admission: the conditioning embedding runs on the batch's stream when the request takes its lane; that step waits for it
        host = {"plain": [], "control": []}
        gpu, repeats = [], []
        for i in range(1, 7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = on._prepare(dict(mixed[i], **kw25))
            host["control" if i % 2 else "plain"].append(time.perf_counter() - t0)
            if i % 2:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(on.exec.stream):
                    e0.record()
                    on.exec._control_rows(r)
                    e1.record()
                torch.cuda.synchronize()
                gpu.append(e0.elapsed_time(e1))
                first = [e.clone() for e in r.cemb]
                with torch.cuda.stream(on.exec.stream):
                    on.exec._control_rows(r)
                torch.cuda.synchronize()
                repeats.append(all(torch.equal(a_, b_) for a_, b_ in zip(first, r.cemb)))
        emit(leg="controlnet_admission", conditioning_embedding_gpu_ms=[round(v, 3) for v in gpu],
             embedding_repeats_bit_for_bit=repeats,
             submit_host_ms_plain=[round(1e3 * v, 3) for v in host["plain"]],
             submit_host_ms_with_control=[round(1e3 * v, 3) for v in host["control"]],
             note="gpu: device events around one request's image preparation + conditioning embedding (seven library convolutions and the last one on the package's 3x3 kernel) "
                  "+ layout on the batch's stream; host: the whole of submit's preparation on the caller's thread, launches included")
        emit(leg="stats", flag_off=off.stats(), flag_on=on.stats())
        return

    if a.t2i_adapter:
        from diffusionspatialcontrol_amd.modules import t2i_adapter as t2i
        torch.manual_seed(a.seed + 7)
        with torch.device("cuda"):
            ad = t2i.T2IAdapter(channels=unet.cfg.block_out_channels, num_res_blocks=2)
        t2i.setup_model_t2i_adapter(pipe, ad.half().eval())
        off = pipe.serve(512, 512, max_batch=8, slot=0).warm()
        on = pipe.serve(512, 512, max_batch=8, slot=1, t2i_adapter=True).warm()
        images = [torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(a.seed * 1000 + 4000 + i)) for i in range(len(reqs))]
        mixed = [dict(r, image_t2i_adapter=images[i], adapter_conditioning_scale=0.8, adapter_conditioning_factor=0.5) if i % 2
                 else dict(r) for i, r in enumerate(reqs)]
        for b, group in ((off, reqs[:8]), (on, reqs[:8]), (on, mixed[:8])):     # one untimed pass each
            run_full(b, group, kw25)
        runs = []
        for _ in range(3):                                # alternating, so that a drift of the box hits all alike
            runs.append((run_full(off, reqs, kw25), run_full(on, reqs, kw25), run_full(on, mixed, kw25)))
        emit(leg="t2i_adapter", requests=len(reqs), steps=25, mix="every other request with a control image, scale 0.8, factor 0.5",
             flag_off_plain_img_s=[round(t[0][0], 2) for t in runs], flag_on_plain_img_s=[round(t[1][0], 2) for t in runs],
             flag_on_every_other_with_control_img_s=[round(t[2][0], 2) for t in runs],
             flag_off_plain_steps_s=[round(t[0][1], 1) for t in runs], flag_on_plain_steps_s=[round(t[1][1], 1) for t in runs],
             adapter_gate_updates=on.stats()["adapter_gate_updates"], captures_after_warm=on.stats()["captures_after_warm"],
             note="three alternating rounds in one process; the flag-off batcher captures the step of a pipeline without the feature")
        # admission: the adapter forward runs on the batch's stream at submit; the next step of the batch waits for it
        host = {"plain": [], "control": []}
        gpu = []
        for i in range(1, 7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = on._prepare(dict(mixed[i], **kw25))
            host["control" if i % 2 else "plain"].append(time.perf_counter() - t0)
            if i % 2:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(on.exec.stream):
                    e0.record()
                    on.exec._adapter_rows(r)
                    e1.record()
                torch.cuda.synchronize()
                gpu.append(e0.elapsed_time(e1))
        emit(leg="t2i_adapter_admission", adapter_forward_gpu_ms=[round(v, 3) for v in gpu],
             submit_host_ms_plain=[round(1e3 * v, 3) for v in host["plain"]],
             submit_host_ms_with_control=[round(1e3 * v, 3) for v in host["control"]],
             note="gpu: device events around one request's adapter forward (library convolutions) + scale + layout on the batch's "
                  "stream; host: the whole of submit's preparation on the caller's thread, launches included")
        emit(leg="stats", flag_off=off.stats(), flag_on=on.stats())
        return

    if a.ip_adapter:
        from diffusionspatialcontrol_amd.modules.u_net_condition_modify import Attention
        plain = pipe.serve(512, 512, max_batch=8, slot=0).warm()
        run_full(plain, reqs[:8], kw25)                   # one untimed pass (allocator, kernel selection at every bucket)
        before = [run_full(plain, reqs, kw25) for _ in range(3)]
        g = torch.Generator().manual_seed(a.seed + 5)
        emb_dim, ctx = 1024, 768
        cross = [m for pre in ("down_blocks", "up_blocks", "mid_block") for n, m in unet.named_modules()
                 if isinstance(m, Attention) and m.is_cross_attention and n.startswith(pre)]
        sd = {"image_proj": {"proj.weight": torch.randn(4 * ctx, emb_dim, generator=g) * 0.03, "proj.bias": torch.zeros(4 * ctx),
                             "norm.weight": torch.ones(ctx), "norm.bias": torch.zeros(ctx)}, "ip_adapter": {}}
        for i, m in enumerate(cross):
            sd["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"] = torch.randn(m.inner_dim, ctx, generator=g) * 0.03
            sd["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"] = torch.randn(m.inner_dim, ctx, generator=g) * 0.03
        pipe.load_ip_adapter(sd)
        pipe.set_ip_adapter_scale(0.6)
        embeds = []
        for i in range(len(reqs)):
            e = torch.randn(2, 1, emb_dim, generator=torch.Generator().manual_seed(a.seed * 1000 + 3000 + i)).half().cuda()
            e[0] = 0
            embeds.append([e])
        mixed = [dict(r, ip_adapter_image_embeds=embeds[i]) if i % 2 else dict(r) for i, r in enumerate(reqs)]
        b = pipe.serve(512, 512, max_batch=8, slot=1).warm()
        for group in (reqs[:8], mixed[:8]):
            run_full(b, group, kw25)
        runs = []
        for _ in range(3):                                # alternating, so that a drift of the box hits both alike
            runs.append((run_full(b, reqs, kw25), run_full(b, mixed, kw25)))
        emit(leg="ip_adapter", requests=len(reqs), steps=25, tokens=4, layers=len(cross),
             batcher_without_adapter_img_s=[round(t[0], 2) for t in before],
             ip_capable_no_image_prompt_img_s=[round(t[0], 2) for t, _ in runs],
             ip_capable_every_other_with_image_prompt_img_s=[round(m[0], 2) for _, m in runs],
             captures_after_warm=b.stats()["captures_after_warm"],
             note="the batcher without an adapter ran first (loading the adapter makes it stale), the two IP-capable legs alternate")
        r = reqs[1]
        one = dict(height=512, width=512, sampler_name="sample_dpmpp_2m", latents=r["latents"], region_map_state=r["region_map_state"],
                   prompt_embeds=r["prompt_embeds"], negative_prompt_embeds=r["negative_prompt_embeds"],
                   text_input_ids=r["text_input_ids"], output_type="latent", ip_adapter_image_embeds=embeds[1], fused=True, **kw25)
        pipe.txt2img(None, **one)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(4):
            pipe.txt2img(None, **one)
        torch.cuda.synchronize()
        emit(leg="ip_adapter_one_at_a_time", steps=25, txt2img_fused_with_image_prompt_img_s=round(4 / (time.perf_counter() - t0), 2))
        if a.ip_masks:
            bm = pipe.serve(512, 512, max_batch=8, slot=2, ip_masks=True).warm()
            half = torch.zeros(1, 1, 512, 512, device="cuda")
            half[:, :, :256] = 1.0                            # the adapter acts on the top half of the image
            masked = [dict(r, cross_attention_kwargs={"ip_adapter_masks": half}) if i % 4 == 3 else dict(r) for i, r in enumerate(mixed)]
            for group in (mixed[:8], masked[:8]):
                run_full(bm, group, kw25)
            runs = []
            for _ in range(3):
                runs.append((run_full(b, mixed, kw25), run_full(bm, mixed, kw25), run_full(bm, masked, kw25)))
            emit(leg="ip_masks", requests=len(reqs), steps=25, tokens=4, layers=len(cross),
                 ip_capable_every_other_with_image_prompt_img_s=[round(t[0][0], 2) for t in runs],
                 mask_capable_same_requests_no_mask_img_s=[round(t[1][0], 2) for t in runs],
                 mask_capable_every_other_image_prompt_masked_img_s=[round(t[2][0], 2) for t in runs],
                 captures_after_warm=bm.stats()["captures_after_warm"],
                 note="three alternating runs; the mask is ones on the top half of the image, down-sampled once per request")
        return

    if a.hires is not None:
        pair = pipe.serve_hires(512, 512, a.hires, max_batch=8).warm()
        mixed = [dict(r, upscale=True, upscale_x=a.hires, seed=i) if i % 2 else dict(r) for i, r in enumerate(reqs)]

        def leg():
            pair.start()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            futs = [pair.submit(dict(r, **kw25)) for r in mixed]
            for f in futs:
                f.result()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            pair.stop()
            return len(mixed) / dt, futs
        leg()                                             # one untimed pass (allocator, kernel selection at every bucket)
        rate, futs = leg()
        hi = [f for i, f in enumerate(futs) if i % 2]
        emit(leg="hires", upscale_x=a.hires, target=[pair.hires.height, pair.hires.width], requests=len(mixed), steps=25,
             mix="every other request with the hires pass (bicubic, strength 0.7: 17 steps at the target size)",
             img_s=round(rate, 2), plain_p50_s=pct([f.dsc_latency_s for i, f in enumerate(futs) if not i % 2], 50),
             hires_p50_s=pct([f.dsc_latency_s for f in hi], 50), hires_first_pass_p50_s=pct([f.dsc_first_pass_s for f in hi], 50),
             hires_second_pass_p50_s=pct([f.dsc_latency_s - f.dsc_first_pass_s for f in hi], 50))
        emit(leg="stats", **pair.stats())
        return

    if a.two_call and a.kernels:
        n, eh, us = step_rows_kernel_us()
        emit(leg="step_rows_kernels", slots=n, latent="4x64x64", device_us_per_launch=us,
             note="a captured graph of 100 launches per figure, alternating")
        return

    if a.sampler or a.guidance_rescale is not None or a.two_call:
        from diffusionspatialcontrol_amd.modules import sampling
        staged = a.sampler is not None and sampling.two_call_family(a.sampler) is not None
        flag = {"two_call": True} if staged or a.two_call else {}
        b = pipe.serve(512, 512, max_batch=8, slot=0, **flag).warm()
        keys = {} if a.guidance_rescale is None else {"guidance_rescale": a.guidance_rescale}
        if a.sampler:
            keys["sampler_name"] = a.sampler
        a.sampler = a.sampler or "sample_dpmpp_2m"
        named = [dict(r, seed=i, **keys) if i % 2 else dict(r) for i, r in enumerate(reqs)]
        for group in (reqs[:8], named[:8]):
            run_full(b, group, kw25)
        runs = []
        for _ in range(3):
            runs.append((run_full(b, reqs, kw25), run_full(b, named, kw25)))
        emit(leg="sampler" if a.guidance_rescale is None else "rescale", sampler=a.sampler, guidance_rescale=a.guidance_rescale,
             requests=len(reqs), steps=25, mix="every other request on the named sampler / with the rescale",
             dpmpp_2m_img_s=[round(t[0], 2) for t, _ in runs], mixed_img_s=[round(m[0], 2) for _, m in runs],
             dpmpp_2m_calls_s=[round(t[1], 2) for t, _ in runs], mixed_calls_s=[round(m[1], 2) for _, m in runs],
             two_call=bool(flag), staged_transitions=b.stats().get("staged_transitions"),
             linear_transitions=b.stats()["linear_transitions"], captures_after_warm=b.stats()["captures_after_warm"])
        from diffusionspatialcontrol_amd.modules import samplers_extra_k_diffusion as sx
        fn = sx.sample_lcm if a.sampler.endswith("lcm") else getattr(sampling, a.sampler)
        r = reqs[0]
        one = dict(height=512, width=512, sampler_name=fn, latents=r["latents"], region_map_state=r["region_map_state"],
                   prompt_embeds=r["prompt_embeds"], negative_prompt_embeds=r["negative_prompt_embeds"], eta=1.0,
                   text_input_ids=r["text_input_ids"], output_type="latent", **kw25)
        if a.guidance_rescale is not None:
            one["guidance_rescale"] = a.guidance_rescale
        if staged:
            one["two_call"] = True
        rate = {}
        for mode in (True, False):
            pipe.txt2img(None, fused=mode, **one)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(4):
                pipe.txt2img(None, fused=mode, **one)
            torch.cuda.synchronize()
            rate[mode] = 4 / (time.perf_counter() - t0)
        emit(leg="sampler_one_at_a_time", sampler=a.sampler, guidance_rescale=a.guidance_rescale, steps=25, fused_img_s=round(rate[True], 2),
             protocol_img_s=round(rate[False], 2))
        return

    if a.mix:
        b = pipe.serve(512, 512, max_batch=8, slot=0).warm()
        mixed = make_mixed(reqs, a.seed)
        for group in (reqs[:8], mixed[:8]):               # one untimed pass each (allocator, kernel selection at every bucket)
            run_full(b, group, kw25)
        runs = []
        for _ in range(3):                                # alternating, so that a drift of the box hits both alike
            runs.append((run_full(b, reqs, kw25), run_full(b, mixed, kw25)))
        emit(leg="mix", requests=len(reqs), steps=25, mix="1/3 txt2img, 1/3 img2img strength 0.6 (15 steps), 1/3 inpainting",
             txt2img_img_s=[round(t[0], 2) for t, _ in runs], txt2img_steps_s=[round(t[1], 1) for t, _ in runs],
             mixed_img_s=[round(m[0], 2) for _, m in runs], mixed_steps_s=[round(m[1], 1) for _, m in runs],
             note="steps/s = captured UNet steps of the batch per second; a step of the mixed batch carries one "
                  "dsc_cfg_dpmpp2m_step_rows_known launch instead of the plain one while an inpainting slot steps")
        emit(leg="stats", slot0=b.stats())
        return

    # ---- saturated
    b0 = pipe.serve(512, 512, max_batch=8, slot=0).warm()
    b1 = pipe.serve(512, 512, max_batch=8, slot=1).warm()
    b0.run_until_idle()
    for r in reqs[:8]:                                   # one untimed pass (allocator, kernel selection at every bucket)
        b0.submit(dict(r, **kw25))
    b0.run_until_idle()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    futs = [b0.submit(dict(r, **kw25)) for r in reqs]
    b0.run_until_idle()
    torch.cuda.synchronize()
    serve1 = len(reqs) / (time.perf_counter() - t0)
    half = len(reqs) // 2
    t0 = time.perf_counter()
    b0.start()
    b1.start()
    futs = [b0.submit(dict(r, **kw25)) for r in reqs[:half]] + [b1.submit(dict(r, **kw25)) for r in reqs[half:]]
    for f in futs:
        f.result()
    torch.cuda.synchronize()
    serve2 = len(reqs) / (time.perf_counter() - t0)
    b0.stop()
    b1.stop()
    groups = [reqs[i:i + 8] for i in range(0, len(reqs) - 7, 8)]
    pipe.txt2img_coalesced(groups[0], height=512, width=512, output_type="latent", **kw25)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for g in groups:
        pipe.txt2img_coalesced(g, height=512, width=512, output_type="latent", **kw25)
    torch.cuda.synchronize()
    co1 = 8 * len(groups) / (time.perf_counter() - t0)
    co2 = None
    if len(groups) >= 2:
        pipe.txt2img_coalesced(groups[1], height=512, width=512, output_type="latent", slot=1, **kw25)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ths = [threading.Thread(target=lambda g_, s_: (torch.cuda.set_stream(torch.cuda.Stream()),
                                                        pipe.txt2img_coalesced(g_, height=512, width=512, output_type="latent",
                                                                               slot=s_, **kw25)), args=(g, i % 2))
               for i, g in enumerate(groups[:2])]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        torch.cuda.synchronize()
        co2 = 16 / (time.perf_counter() - t0)
    emit(leg="saturated", requests=len(reqs), steps=25, serve_one_in_flight_img_s=round(serve1, 2),
         serve_two_in_flight_img_s=round(serve2, 2), coalesced_k8_one_in_flight_img_s=round(co1, 2),
         coalesced_k8_two_in_flight_img_s=None if co2 is None else round(co2, 2))

    # ---- staggered arrivals
    rng = random.Random(a.seed)
    mix = [dict(num_inference_steps=rng.choice((20, 25, 30)), guidance_scale=rng.choice((5.0, 7.5)), sampler_opt=opt)
           for _ in reqs]
    single_s = {}
    for steps in (20, 25, 30):                          # one-at-a-time txt2img: service time per step count
        r = reqs[0]
        pipe.txt2img(None, height=512, width=512, sampler_name="sample_dpmpp_2m", latents=r["latents"],
                     region_map_state=r["region_map_state"], prompt_embeds=r["prompt_embeds"],
                     negative_prompt_embeds=r["negative_prompt_embeds"], text_input_ids=r["text_input_ids"],
                     output_type="latent", num_inference_steps=steps, sampler_opt=opt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.txt2img(None, height=512, width=512, sampler_name="sample_dpmpp_2m", latents=r["latents"],
                     region_map_state=r["region_map_state"], prompt_embeds=r["prompt_embeds"],
                     negative_prompt_embeds=r["negative_prompt_embeds"], text_input_ids=r["text_input_ids"],
                     output_type="latent", num_inference_steps=steps, sampler_opt=opt)
        torch.cuda.synchronize()
        single_s[steps] = time.perf_counter() - t0
    co_batch_s = 8 / co1
    for rate in (float(x) for x in a.rates.split(",")):
        gaps = [rng.expovariate(rate) for _ in reqs]
        arrive = list(np.cumsum(gaps))
        b0.start()
        t0 = time.perf_counter()
        futs, sub_t = [], []
        for r, m, at in zip(reqs, mix, arrive):
            dt = t0 + at - time.perf_counter()
            if dt > 0:
                time.sleep(dt)
            sub_t.append(time.perf_counter())
            futs.append(b0.submit(dict(r, **m)))
        lat = [f.result() is not None and f.dsc_latency_s for f in futs]       # submit -> future resolved (step-granular)
        end = time.perf_counter()
        b0.stop()
        # one-at-a-time txt2img (a FIFO queue, service time measured above) and lockstep batches of 8 (a batch starts when
        # 8 requests have arrived and the previous batch is done; all its requests share the batch's 25-step schedule)
        free, sl = 0.0, []
        for at, m in zip(arrive, mix):
            s_ = max(free, at)
            free = s_ + single_s[m["num_inference_steps"]]
            sl.append(free - at)
        free, cl = 0.0, []
        for i in range(0, len(arrive) - 7, 8):
            s_ = max(free, arrive[i + 7])
            free = s_ + co_batch_s
            cl += [free - at for at in arrive[i:i + 8]]
        emit(leg="staggered", rate_req_s=rate, requests=len(reqs), serve_img_s=round(len(reqs) / (end - t0), 2),
             serve_p50_s=pct(lat, 50), serve_p95_s=pct(lat, 95),
             txt2img_serial_p50_s=pct(sl, 50), txt2img_serial_p95_s=pct(sl, 95),
             coalesced_lockstep_p50_s=pct(cl, 50), coalesced_lockstep_p95_s=pct(cl, 95),
             note="txt2img / coalesced latencies are queueing models over service times measured in this process")

    # ---- join cost
    b0.submit(dict(reqs[0], num_inference_steps=30, guidance_scale=7.5, sampler_opt=opt))
    b0.step()
    for _ in range(3):
        b0.step()
    torch.cuda.synchronize()
    plain = []
    for _ in range(5):
        t0 = time.perf_counter()
        b0.step()
        plain.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    join = []
    for r in reqs[1:4]:
        b0.submit(dict(r, num_inference_steps=30, guidance_scale=7.5, sampler_opt=opt))
        t0 = time.perf_counter()
        b0.step()
        join.append(time.perf_counter() - t0)
        b0.step()
    torch.cuda.synchronize()
    members = [b0._slots[i] if i < len(b0._slots) else None for i in range(max(b0.exec.st))]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(b0.exec.stream):
        e0.record()
        b0.exec.refresh(max(b0.exec.st), members)
        e1.record()
    torch.cuda.synchronize()
    b0.run_until_idle()
    emit(leg="join", plain_step_host_ms=round(1e3 * float(np.median(plain)), 3),
         join_step_host_ms=round(1e3 * float(np.median(join)), 3),
         join_stall_host_ms=round(1e3 * (float(np.median(join)) - float(np.median(plain))), 3),
         text_kv_table_refresh_gpu_ms=round(e0.elapsed_time(e1), 3), bucket=max(b0.exec.st))
    emit(leg="stats", slot0=b0.stats(), slot1=b1.stats())


if __name__ == "__main__":
    main()
