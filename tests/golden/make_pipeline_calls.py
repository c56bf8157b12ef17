"""What txt2img, img2img and inpaiting hand to the two denoise cores, recorded without a device: the tiny fp16 UNet pipeline on the
CPU, `_denoise_fused` / `_denoise_protocol` replaced on the instance by functions that record their arguments and return their
`latents`, `_controlnet_hook` / `_adapter_hook` by functions that record theirs, and `get_sigmas` by a literal table (no
transcendental in the schedule).  Only these five names are patched, so the script runs unchanged before and after a change of the
entries.

    python tests/golden/make_pipeline_calls.py      (re)writes tests/golden/pipeline_calls.json

Run it at the commit whose entries are the reference; tests/test_pipeline_calls_host.py replays the same cases through the same
recorder and requires equality with the file.  The committed file was written at a72fa4a ("Route linears in one plan; one operand
check for every GEMM entry"), the parent of the change that folded the three entries into one generation path.

A row is {"cores": [...], "hooks": [...], "cfg", "added_cond_kwargs", "result" | "error"}:
  cores   one [core, positional arguments, keyword arguments] per core call, as passed (a hires case has two), normalised:
          a tensor as [shape, dtype, SHA-1 of its bytes]; a region-state dict per level; the sampler by __name__; weight_func by
          _weight_func_key; a noise sampler by its type name; control_hook by the kinds in its .static (None: no .static);
          preview by its presence; input_hook by the hashes of what it returns for a fixed x at (call index, sigma) =
          (0, 1.5), (1, 1.5) and (1, 0)
  hooks   [name, arguments] of every _controlnet_hook / _adapter_hook call
  cfg, added_cond_kwargs   the pipeline's _do_classifier_free_guidance and _added_cond_kwargs after the call
  result  the returned list, element by element; error: [exception type, message] when the call raises
Every input is seeded or literal, images and masks are given at their final size and hires cases enlarge with "nearest", so every
tensor replays bit-equal (none is recorded rounded)."""
import dataclasses
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from inputs import FakeTokenizer  # noqa: E402

PATH = os.path.join(HERE, "pipeline_calls.json")
SIGMAS = [14.5, 9.0, 5.5, 3.25, 2.0, 1.25, 0.75, 0.5, 0.25, 0.125]          # fp16-exact, descending
S, CTX, SIZE, LAT = 77, 64, 128, 16
PATCHED = ("_denoise_fused", "_denoise_protocol", "_controlnet_hook", "_adapter_hook", "get_sigmas")

_pipes = {}


def pipe(kind):
    """"eps" / "v": the tiny fp16 UNet of tests/test_linear_step_host.py::_pipe; "eps9": the 9-channel one of
    tests/test_inpaint_unet_host.py::_pipe"""
    if kind not in _pipes:
        from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
        from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
        torch.manual_seed(0)
        cfg = dataclasses.replace(UNetConfig.tiny(), in_channels=9) if kind == "eps9" else UNetConfig.tiny()
        sched = SD15Scheduler(prediction_type="v_prediction" if kind == "v" else "epsilon")
        _pipes[kind] = StableDiffusionPipeline(None, None, FakeTokenizer(), UNet2DConditionModel(cfg).half(), sched)
    return _pipes[kind]


def pattern(*shape, period=23, dtype=torch.float16):
    """a literal tensor: values k / 8 - 1.25 for k = i mod period"""
    n = int(np.prod(shape))
    return ((torch.arange(n) % period).float() / 8 - 1.25).reshape(shape).to(dtype)


def masked():
    """a region state of two phrases with one 64-pixel cell each and the ids of a prompt that holds them (tests/golden/inputs.py)"""
    tok = FakeTokenizer()
    words = ["object0a object0b", "object1a object1b"]
    ids = [49406, 320]
    for w in words:
        ids += tok(w).input_ids
    pos = np.array([ids + [49407] * (S - len(ids))], dtype=np.int64)
    state = {}
    for r, w in enumerate(words):
        m = np.full((SIZE, SIZE), 255, dtype=np.uint8)
        m[0:64, r * 64:(r + 1) * 64] = 0
        state[w] = {"map": m, "weight": 0.5 + 0.25 * r, "mask_outsides": 0.25 * r}
    return state, [pos.copy(), pos]


def base(**kw):
    d = dict(prompt_embeds=pattern(1, S, CTX), negative_prompt_embeds=pattern(1, S, CTX, period=19), num_inference_steps=4,
             guidance_scale=7.5, sampler_name="sample_dpmpp_2m", sampler_opt={"scheduler": "karras"}, output_type="latent",
             generator=torch.Generator().manual_seed(7), seed=3)
    d.update(kw)
    return d


def t2i(**kw):
    return base(height=SIZE, width=SIZE, **kw)


def i2i(**kw):
    return base(**dict(dict(latents=pattern(1, 4, LAT, LAT, period=29), height=SIZE, width=SIZE, strength=0.5), **kw))


def inp(**kw):
    mask = torch.zeros(1, 1, SIZE, SIZE)
    mask[:, :, :, 64:] = 1.0
    return base(**dict(dict(image=pattern(1, 4, LAT, LAT, period=29), mask_image=mask, height=SIZE, width=SIZE), **kw))


HIRES = dict(upscale=True, upscale_x=1.5, upscale_method="nearest", upscale_denoising_strength=0.5)
BROWNIAN = {"scheduler": "karras", "brownian_noise": True, "solver_type": "heun"}


def cases():
    """(id, pipeline kind, entry, keyword arguments, _adapter_hook returns a stub) - built afresh on every call: the generators
    are consumed"""
    state, ids = masked()
    ip = [pattern(2, 4, CTX, period=13)]
    mil = pattern(1, 4, LAT, LAT, period=31)
    noise = pattern(4, 1, 4, LAT, LAT, period=37)
    out = [
        ("txt2img", "eps", "txt2img", t2i()),
        ("txt2img fused=True", "eps", "txt2img", t2i(fused=True)),
        ("txt2img fused=False", "eps", "txt2img", t2i(fused=False)),
        ("txt2img guidance 1.0", "eps", "txt2img", t2i(guidance_scale=1.0)),
        ("txt2img guidance 1.0 fused=True", "eps", "txt2img", t2i(guidance_scale=1.0, fused=True)),
        ("txt2img rescale 0.7", "eps", "txt2img", t2i(guidance_rescale=0.7)),
        ("txt2img rescale 0.7 fused=True", "eps", "txt2img", t2i(guidance_rescale=0.7, fused=True)),
        ("txt2img euler", "eps", "txt2img", t2i(sampler_name="sample_euler")),
        ("txt2img euler fused=True eta", "eps", "txt2img", t2i(sampler_name="sample_euler", fused=True, eta=0.5)),
        ("txt2img heun", "eps", "txt2img", t2i(sampler_name="sample_heun")),
        ("txt2img heun fused=True", "eps", "txt2img", t2i(sampler_name="sample_heun", fused=True)),
        ("txt2img sde brownian heun", "eps", "txt2img", t2i(sampler_name="sample_dpmpp_2m_sde", sampler_opt=BROWNIAN)),
        ("txt2img sde brownian heun fused=True", "eps", "txt2img",
         t2i(sampler_name="sample_dpmpp_2m_sde", sampler_opt=BROWNIAN, fused=True, eta=0.75)),
        ("txt2img two images", "eps", "txt2img", t2i(num_images_per_prompt=2)),
        ("txt2img latents given", "eps", "txt2img", t2i(latents=pattern(1, 4, LAT, LAT, period=29))),
        ("txt2img slot=1", "eps", "txt2img", t2i(slot=1)),
        ("txt2img slot=1 fused=False", "eps", "txt2img", t2i(slot=1, fused=False)),
        ("txt2img step_noise", "eps", "txt2img", t2i(sampler_name="sample_euler_ancestral", fused=True, step_noise=noise)),
        ("txt2img previews", "eps", "txt2img", t2i(latent_processing=1)),
        ("txt2img previews fused=True", "eps", "txt2img", t2i(latent_processing=1, fused=True)),
        ("txt2img hires", "eps", "txt2img", t2i(sampler_name_hires="sample_euler", sampler_opt_hires={"scheduler": "exponential"},
                                                latent_upscale_processing=1, **HIRES)),
        ("txt2img hires, same sampler", "eps", "txt2img", t2i(guidance_rescale=0.25, num_images_per_prompt=2, **HIRES)),
        ("txt2img hires previews", "eps", "txt2img", t2i(latent_processing=1, **HIRES)),
        ("txt2img hires previews both", "eps", "txt2img", t2i(latent_processing=1, latent_upscale_processing=1, **HIRES)),
        ("txt2img regions", "eps", "txt2img", t2i(region_map_state=state, text_input_ids=ids)),
        ("txt2img regions two images hires", "eps", "txt2img",
         t2i(region_map_state=state, text_input_ids=ids, num_images_per_prompt=2, **HIRES)),
        ("txt2img ip embeds", "eps", "txt2img", t2i(ip_adapter_image_embeds=ip)),
        ("txt2img ip embeds guidance 1.0", "eps", "txt2img", t2i(ip_adapter_image_embeds=[ip[0][:1]], guidance_scale=1.0)),
        ("txt2img cross_attention_kwargs", "eps", "txt2img", t2i(cross_attention_kwargs={"scale": 0.5})),
        ("txt2img no negative embeds", "eps", "txt2img", t2i(negative_prompt_embeds=None)),
        ("txt2img no prompt", "eps", "txt2img", t2i(prompt_embeds=None, prompt="a photo")),
        ("txt2img v-prediction", "v", "txt2img", t2i()),
        ("txt2img v-prediction fused=True", "v", "txt2img", t2i(fused=True)),
        ("txt2img adapter image, no adapter", "eps", "txt2img", t2i(image_t2i_adapter=torch.zeros(1, 3, SIZE, SIZE), prompt_embeds=None)),
        ("txt2img hook", "eps", "txt2img", t2i(num_inference_steps=6, adapter_conditioning_factor=0.5), True),
        ("txt2img hook fused=True", "eps", "txt2img", t2i(num_inference_steps=6, fused=True), True),

        ("img2img strength 0.5", "eps", "img2img", i2i()),
        ("img2img strength 1.0", "eps", "img2img", i2i(strength=1.0)),
        ("img2img strength 0.3 of 7", "eps", "img2img", i2i(strength=0.3, num_inference_steps=7)),
        ("img2img no size", "eps", "img2img", i2i(height=None, width=None)),
        ("img2img two images of one latent", "eps", "img2img", i2i(num_images_per_prompt=2)),
        ("img2img fused=True", "eps", "img2img", i2i(fused=True)),
        ("img2img fused=False", "eps", "img2img", i2i(fused=False)),
        ("img2img guidance 1.0", "eps", "img2img", i2i(guidance_scale=1.0)),
        ("img2img rescale 0.7", "eps", "img2img", i2i(guidance_rescale=0.7)),
        ("img2img euler", "eps", "img2img", i2i(sampler_name="sample_euler")),
        ("img2img sde brownian heun", "eps", "img2img", i2i(sampler_name="sample_dpmpp_2m_sde", sampler_opt=BROWNIAN)),
        ("img2img sde brownian heun fused=True", "eps", "img2img",
         i2i(sampler_name="sample_dpmpp_2m_sde", sampler_opt=BROWNIAN, fused=True)),
        ("img2img step_noise", "eps", "img2img", i2i(sampler_name="sample_euler_ancestral", fused=True, step_noise=noise[:3])),
        ("img2img previews", "eps", "img2img", i2i(latent_processing=1)),
        ("img2img hires", "eps", "img2img", i2i(sampler_name_hires="sample_euler", latent_upscale_processing=1, **HIRES)),
        ("img2img hires previews", "eps", "img2img", i2i(latent_processing=1, **HIRES)),
        ("img2img regions ip embeds", "eps", "img2img", i2i(region_map_state=state, text_input_ids=ids, ip_adapter_image_embeds=ip)),
        ("img2img v-prediction", "v", "img2img", i2i()),
        ("img2img nothing to start from", "eps", "img2img", i2i(latents=None)),
        ("img2img hook", "eps", "img2img", i2i(num_inference_steps=6), True),
        ("img2img hook fused=True", "eps", "img2img", i2i(num_inference_steps=6, fused=True), True),

        ("inpaiting strength 1.0", "eps", "inpaiting", inp()),
        ("inpaiting strength 0.5", "eps", "inpaiting", inp(strength=0.5)),
        ("inpaiting latents given", "eps", "inpaiting", inp(latents=pattern(1, 4, LAT, LAT, period=17), eta=0.5)),
        ("inpaiting two images", "eps", "inpaiting", inp(num_images_per_prompt=2, strength=0.75)),
        ("inpaiting fused=True, 4 channels", "eps", "inpaiting", inp(fused=True)),
        ("inpaiting fused=False", "eps", "inpaiting", inp(fused=False)),
        ("inpaiting guidance 1.0", "eps", "inpaiting", inp(guidance_scale=1.0)),
        ("inpaiting previews", "eps", "inpaiting", inp(latent_processing=1)),
        ("inpaiting regions ip embeds", "eps", "inpaiting", inp(region_map_state=state, text_input_ids=ids, ip_adapter_image_embeds=ip)),
        ("inpaiting sde brownian heun", "eps", "inpaiting", inp(sampler_name="sample_dpmpp_2m_sde", sampler_opt=BROWNIAN)),
        ("inpaiting upscale", "eps", "inpaiting", inp(upscale=True)),
        ("inpaiting mask crop", "eps", "inpaiting", inp(padding_mask_crop=8)),
        ("inpaiting no mask", "eps", "inpaiting", inp(mask_image=None)),
        ("inpaiting 9 channels", "eps9", "inpaiting", inp(masked_image_latents=mil)),
        ("inpaiting 9 channels fused=True", "eps9", "inpaiting", inp(masked_image_latents=mil, fused=True, eta=0.5)),
        ("inpaiting 9 channels fused=True strength 0.5 two images", "eps9", "inpaiting",
         inp(masked_image_latents=mil, fused=True, strength=0.5, num_images_per_prompt=2, sampler_name="sample_euler_ancestral",
             step_noise=noise[:2], guidance_rescale=0.5)),
        ("inpaiting 9 channels guidance 1.0", "eps9", "inpaiting", inp(masked_image_latents=mil, guidance_scale=1.0)),
        ("inpaiting 9 channels fused=True previews", "eps9", "inpaiting", inp(masked_image_latents=mil, fused=True, latent_processing=1)),
        ("inpaiting 9 channels fused=True odd latent", "eps9", "inpaiting",
         inp(image=pattern(1, 4, 13, 13), mask_image=torch.ones(1, 1, 104, 104), masked_image_latents=pattern(1, 4, 13, 13, period=31),
             height=104, width=104, fused=True)),
        ("inpaiting 9 channels, latents for pixels", "eps9", "inpaiting", inp()),
        ("inpaiting hook", "eps", "inpaiting", inp(num_inference_steps=6, strength=0.5), True),
        ("inpaiting hook fused=True", "eps", "inpaiting", inp(num_inference_steps=6, fused=True), True),
        ("inpaiting 9 channels hook", "eps9", "inpaiting", inp(masked_image_latents=mil, num_inference_steps=6, strength=0.5), True),
        ("inpaiting 9 channels hook fused=True", "eps9", "inpaiting", inp(masked_image_latents=mil, num_inference_steps=6, fused=True), True),
    ]
    return [c if len(c) == 5 else c + (False,) for c in out]


# ----------------------------------------------------------------------------- normalisation
def norm(v):
    if torch.is_tensor(v):
        return [list(v.shape), str(v.dtype), hashlib.sha1(v.detach().contiguous().cpu().numpy().tobytes()).hexdigest()]
    if isinstance(v, np.ndarray):
        return norm(torch.from_numpy(v))
    if isinstance(v, dict):
        return {str(k): norm(e) for k, e in v.items()}
    if isinstance(v, (list, tuple)):
        return [norm(e) for e in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


def _input_hook(hook, latents):
    if hook is None:
        return None
    x = pattern(*latents.shape, period=41).to(latents.dtype)
    return [norm(hook(x.clone(), torch.tensor([s], dtype=latents.dtype), i)) for i, s in ((0, 1.5), (1, 1.5), (1, 0.0))]


def _named(p, name, v, latents):
    if name == "sampler":
        return getattr(v, "__name__", norm(v))
    if name == "weight_func":
        return norm(p._weight_func_key(v))
    if name == "sampler_args" and isinstance(v, dict):
        return {k: type(e).__name__ if k == "noise_sampler" else norm(e) for k, e in v.items()}
    if name == "control_hook" and v is not None:
        st = getattr(v, "static", None)
        return {"static": None if st is None else [part["kind"] for part in st]}
    if name == "preview":
        return v is not None
    if name == "input_hook":
        return _input_hook(v, latents)
    return norm(v)


def record(case):
    """one row of the file (see the module docstring)"""
    _, kind, entry, kwargs, stub_hook = case
    p = pipe(kind)
    cores, hooks = [], []
    real = {name: getattr(type(p), name) for name in PATCHED}

    def core(name):
        params = list(inspect.signature(real[name]).parameters)[1:]

        def fn(*args, **kw):
            latents = args[params.index("latents")]
            cores.append([name, [_named(p, params[i], v, latents) for i, v in enumerate(args)],
                          {k: _named(p, k, v, latents) for k, v in kw.items()}])
            return latents
        return fn

    def hook(name):
        def fn(*args, **kw):
            hooks.append([name, norm(args), norm(kw)])
            if name == "_adapter_hook" and stub_hook:
                stub = lambda latent_model_input, sigma: {}             # noqa: E731
                stub.static = None
                return stub
            return None
        return fn

    def get_sigmas(steps, params):
        return torch.tensor(SIGMAS[:steps] + [0.0])

    patches = {"_denoise_fused": core("_denoise_fused"), "_denoise_protocol": core("_denoise_protocol"),
               "_controlnet_hook": hook("_controlnet_hook"), "_adapter_hook": hook("_adapter_hook"), "get_sigmas": get_sigmas}
    row = {"cores": cores, "hooks": hooks}
    try:
        for name, fn in patches.items():
            setattr(p, name, fn)
        try:
            res = getattr(p, entry)(**kwargs)
            row["result"] = norm(res) if isinstance(res, list) else ["not a list", norm(res)]
        except Exception as e:                       # an answer too
            row["error"] = [type(e).__name__, str(e)]
    finally:
        for name in patches:
            delattr(p, name)
    row["cfg"] = p._do_classifier_free_guidance
    row["added_cond_kwargs"] = norm(p._added_cond_kwargs)
    return row


def record_all():
    """{case id: row}"""
    table = {}
    for case in cases():
        assert case[0] not in table, case[0]
        table[case[0]] = record(case)
    return table


def load():
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    table = record_all()
    with open(PATH, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(c)}: {json.dumps(row, separators=(',', ':'))}" for c, row in table.items()) + "\n}\n")
    assert load() == json.loads(json.dumps(table))
    print(len(table), "cases,", sum("error" in row for row in table.values()), "of them raise")
