"""A request's record (`_Request`, the one class of every batcher) and the submit-time validation of its keys (caller's thread,
host only): functions of (batcher, request, ...) that ServingBatcher._prepare calls in order, on top of one copy of each small check.

Image-conditioned requests.  A request with `image` is img2img (the last `strength` fraction of its schedule, started from
`image_latents + noise * sqrt(sigma_0^2 + 1)`, the pipeline method's line); with `mask_image` too it is inpainting on the 4-channel
UNet: its image latents, noise and mask rows stay on the device while it runs, and the per-row step blends the known region into
the model input of every model call after its first (dsc_cfg_dpmpp2m_step_rows_known, what `inpaiting`'s eager hook does per
call).  That launch replaces the plain one only for transitions in which an inpainting slot steps.

9-channel inpainting UNets.  A batcher built with `inpaint_unet=True` serves the inpainting checkpoints, whose UNet reads
`[latents | mask | masked-image latents]` (reference model_k_diffusion.py:1617-1619): every request of it carries `image` and
`mask_image` (kind "inpaint_unet"), as pixels or as [1, 4, h, w] latents with `masked_image_latents`.  It has no known region to
blend: admission builds `r.extra`, the request's fp16 [5, h, w] row cat([mask, masked-image latents]), and every transition is ONE
dsc_cfg_linear_step_rows_cat launch that writes each member's row, times the coming c_in, behind its latent.  That launch carries
the whole linear family, both parameterisations and the rescale, so the two refusals of `mask_image` above apply to 4-channel
batchers only.

Region masks of image prompts.  A batcher built with `ip_masks=True` takes the reference's
`cross_attention_kwargs={"ip_adapter_masks": [n_adapters, 1, Hm, Wm]}` (app.py:1077-1091; both IP-Adapter processors multiply the
adapter's output by the down-sampled mask, attention_modify.py:371-385 / :676-685).  After down-sampling a mask is one number per
query, so at admission the request's mask is down-sampled ONCE per adapter and cross-attention level of this batcher
(IPAdapterMaskProcessor.downsample, the restatement txt2img's eager route runs per layer and step) and rounded to fp16; the
captured step hands every IP layer a static [rows, L] weight buffer per adapter (ones: no mask) and launches
dsc_ip_xattn_add_masked_f16, which folds the weight into its per-query coefficient and skips 16-query tiles of zeros.  `refresh`
writes a member's weights to rows {i, n + i} (the reference repeats the mask over the batch, unconditional rows included).  A
batcher built without `ip_masks` launches the unmasked entry as before and refuses the key.  A hires request's second pass
down-samples the same mask at the target size's levels.
"""
import torch

from ... import ops
from .. import sampling
from ..attention_modify import weight_func_fused
from ..external_k_diffusion import DiscreteVDDPMDenoiser
from ..latent_resample import MODES as _RESAMPLE_MODES, hires_target_size

MAX_TEXT_KEYS = ops.XATTN_MAX_KEYS_PACKED     # the chunked prepared-operand kernels (ops.region_xattn_packed)
_UNSUPPORTED_KEYS = ("control_img", "image_t2i_adapter")
_IMAGE_TYPES = ("pil", "np", "numpy", "uint8")      # what a batcher built with `decode=True` hands out besides "latent"
_FLAG_HINT = {"image_t2i_adapter": "; a batcher built with `t2i_adapter=True` (pipe.serve(..., t2i_adapter=True)) serves it",
              "control_img": "; a batcher built with `controlnet=True` (pipe.serve(..., controlnet=True)) serves it",
              "freeu": "; a batcher built with `freeu=True` (pipe.serve(..., freeu=True)) serves it"}


class _Request:
    """one request from submit until its future resolves, the same record on every batcher: every field starts at its default here
    (None unless listed), and _prepare assigns only what it computes.  `plan`: its step_plan.StepPlan, one entry per MODEL CALL
    (`i`: the index of the call that runs now); `sig`: the plan's sigmas and the final 0.0.  Fields of a feature stay None on a
    batcher built without it: `extra` (`inpaint_unet=True`: the fp16 [5, h, w] row cat([nearest-downsampled mask, masked-image
    latents]) on the device from admission until it leaves), `freeu` (its (s1, s2, b1, b2)), `enc` / `txt` (its handle on the
    encode / text lane, encode_lane._EncodeHandle / text_lane._TextHandle, from submit until it leaves; None: it does not touch
    the lane - it brings latents / embeddings)"""
    __slots__ = ("rid", "req", "future", "steps", "sig", "sig_dev", "plan", "guidance", "tables",
                 "slot", "i", "lat", "temb", "text", "output_type", "t_submit", "t_done", "kind", "strength", "known",
                 "family", "noise", "rescale", "eta", "hires", "second", "ready", "hnoise", "t_handoff",
                 "ip_embeds", "ip_scale", "ip_rows", "ip_weights", "adapter", "adapter_limit", "adapter_feats",
                 "control", "cgates", "lane", "cemb", "extra", "freeu", "enc", "txt")
    _DEFAULTS = {"steps": 0, "i": 0, "output_type": "latent", "kind": "txt2img", "strength": 1.0, "rescale": 0.0, "eta": 1.0,
                 "second": False, "adapter_limit": 0}

    def __init__(self, **given):
        unknown = set(given) - set(self.__slots__)
        if unknown:
            raise TypeError(f"_Request has no field {sorted(unknown)}")
        for name in self.__slots__:
            setattr(self, name, given.get(name, self._DEFAULTS.get(name)))


# ---------------------------------------------------------------------- one copy of each small check
def finite(v):
    """a python number (no bool) that is neither NaN nor infinite"""
    return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and v not in (float("inf"), float("-inf"))


def per_item(key, v, n, holder, lists=True):
    """request key `key`: a finite number or a list with one finite number per item of `holder` (n of them) -> n floats;
    `lists=False`: the holder is a single model, which takes no list"""
    listed = isinstance(v, (list, tuple))
    if listed and not lists:
        raise ValueError(f"serve: `{key}` is a list, but {holder} is a single model (a list goes with its Multi* form)")
    if listed and len(v) != n:
        raise ValueError(f"serve: `{key}` lists {len(v)} values, {holder} holds {n}")
    vals = list(v) if listed else [v] * n
    if not all(finite(e) for e in vals):
        raise ValueError(f"serve: `{key}` must be a finite number or a list with one finite number per item of {holder}, "
                         f"got {v!r}")
    return [float(e) for e in vals]


def fraction(key, v):
    """request key `key`: a number in [0, 1] -> float"""
    if not finite(v) or not 0.0 <= v <= 1.0:
        raise ValueError(f"serve: `{key}` must be a number in [0, 1], got {v!r}")
    return float(v)


def control_images(key, image, multi, cins, holder, size=None):
    """request key `key`: one PIL image or one floating-point [1, C, H, W] tensor per model of `holder` (`cins`: each model's
    input channels) - a list exactly when the holder is its Multi* form (`multi`), of its length; `size`: the exact (H, W) a
    tensor must have -> the list of images"""
    n, listed = len(cins), isinstance(image, (list, tuple))
    images = list(image) if listed else [image]
    if listed != multi or len(images) != n:
        raise ValueError(f"serve: `{key}` must be " + (f"a list of {n} images ({holder} is a Multi* model)" if multi
                         else f"one image (a list goes with the Multi* form of {holder})") +
                         f", got {f'a list of {len(images)}' if listed else type(image).__name__}")
    for one, cin in zip(images, cins):
        if torch.is_tensor(one):
            ok = one.dim() == 4 and one.shape[0] == 1 and one.shape[1] == cin and torch.is_floating_point(one)
            if not ok or (tuple(one.shape[-2:]) != tuple(size) if size else min(one.shape[2:]) < 1):
                hw = f"{size[0]}, {size[1]}] image in [0, 1] (this batcher's size)" if size else "H, W] image in [0, 1]"
                raise ValueError(f"serve: `{key}` as a tensor must be a floating-point [1, {cin}, {hw}, got {one.dtype} "
                                 f"{list(one.shape)}")
        elif not (hasattr(one, "size") and hasattr(one, "resize") and not hasattr(one, "shape")):
            raise ValueError(f"serve: `{key}` must be a [1, 3, H, W] tensor or a PIL image, got {type(one).__name__}")
    return images


def _spatial_size(image):
    """(height, width) of a tensor (NCHW / CHW / HW), a numpy array (HW / HWC / NCHW) or a PIL image"""
    if torch.is_tensor(image):
        return tuple(int(v) for v in image.shape[-2:])
    if hasattr(image, "size") and not hasattr(image, "shape"):              # PIL: (width, height)
        return (int(image.size[1]), int(image.size[0]))
    shape = tuple(getattr(image, "shape", ()))
    if len(shape) == 3:
        return (int(shape[0]), int(shape[1]))
    return tuple(int(v) for v in shape[-2:])


def _ip_layers(pipe):
    """(attention module, its IP-Adapter processor) of every cross-attention layer in module order; [] without an adapter"""
    from ..attention_modify import _IPAdapterProcessor
    from ..u_net_condition_modify import Attention
    return [(m, m.processor) for m in pipe.unet.modules() if isinstance(m, Attention) and isinstance(m.processor, _IPAdapterProcessor)]


# ---------------------------------------------------------------------- the keys of a request, per feature
def common_request(b, request):
    """the keys every request carries -> (output_type, v_pred, family, guidance_rescale, guidance_scale)"""
    pipe = b.pipe
    out_type = request.get("output_type", "latent")
    if b.decode:
        if out_type not in ("latent",) + _IMAGE_TYPES:
            raise ValueError(f"serve: `output_type` {out_type!r} is not served by a batcher built with `decode=True` (one of: "
                             f"latent, {', '.join(_IMAGE_TYPES)})")
        if out_type == "pil":
            try:
                import PIL.Image  # noqa: F401
            except ImportError as e:
                raise ValueError("serve: `output_type` 'pil' needs Pillow; ask for 'uint8' (the same bytes as an array)") from e
    elif out_type == "uint8":
        raise ValueError("serve: `output_type` 'uint8' is made by the decode lane: build the batcher with `decode=True` "
                         "(pipe.serve(..., decode=True))")
    v_pred = bool(getattr(pipe, "v_prediction", False))
    # the v scalars (step_skip, c_out) come from the denoiser object, the choice of launch from the flag: setup_unet sets
    # both from the scheduler; a flag flipped by hand on an eps-prediction pipeline (tests/test_serving_host.py does that to
    # probe the former v-prediction rejection) would otherwise be served with eps scalars
    if v_pred != isinstance(pipe.k_diffusion_model, DiscreteVDDPMDenoiser):
        raise ValueError("serve: pipe.v_prediction and the denoiser disagree: a v-prediction pipeline needs CompVisVDenoiser's "
                         "scalars (setup_unet builds both from the scheduler's prediction_type; do not set the flag alone)")
    sampler = request.get("sampler_name") or "dpmpp_2m"
    family = sampling.linear_family(sampler)
    if family is None and getattr(b, "two_call", False):
        family = sampling.two_call_family(sampler)
        for k in _UNSUPPORTED_KEYS:
            # (their windows count distinct sigmas seen, which is one per model call only for the one-call samplers)
            if family is not None and request.get(k) is not None:
                raise ValueError(f"serve: `{k}` is not served together with the two-call sampler `sampler_name` {family!r} "
                                 f"(its guidance window counts one model call per step); use txt2img")
    if family is None:
        raise ValueError(f"serve: `sampler_name` {getattr(sampler, '__name__', sampler)!r} has no per-row step (supported: "
                         f"{', '.join(sampling.LINEAR_FAMILY)}; use txt2img)")
    # (a batcher built with `inpaint_unet=True` has no known-region step: its launch carries every sampler, v and the rescale)
    if request.get("mask_image") is not None and not b.inpaint and (family != "dpmpp_2m" or v_pred):
        raise ValueError("serve: `mask_image` (inpainting) runs DPM++ 2M on an eps-prediction model only (the known-region "
                         "step, dsc_cfg_dpmpp2m_step_rows_known); drop `sampler_name` or use inpaiting")
    phi = request.get("guidance_rescale", 0.0)
    phi = fraction("guidance_rescale", 0.0 if phi is None else phi)
    if request.get("mask_image") is not None and not b.inpaint and phi > 0.0:
        raise ValueError("serve: `mask_image` (inpainting) with `guidance_rescale` > 0 is not served (the known-region step "
                         "has no rescale); use inpaiting")
    if (request.get("height", b.height), request.get("width", b.width)) != (b.height, b.width):
        raise ValueError(f"serve: this batcher runs {b.height}x{b.width} images, the request asks for "
                         f"{request.get('height')}x{request.get('width')}")
    # dsc_cfg_linear_step_rows and its rescale form move 8 halfs per lane; refused here, before the request can reach a step
    # that other requests share (DPM++ 2M's own per-row step takes the 4 * odd halfs of a latent with both sides odd)
    if (family != "dpmpp_2m" or v_pred or phi > 0.0) and (4 * (b.height // 8) * (b.width // 8)) % 8 != 0:
        raise ValueError(f"serve: this batcher's {b.height // 8}x{b.width // 8} latent has both sides odd; the linear "
                         f"per-row step (every sampler but DPM++ 2M, v-prediction models, `guidance_rescale` > 0) needs a "
                         f"multiple of 8 halfs per latent: drop `sampler_name` / `guidance_rescale`, or use txt2img")
    g = float(request.get("guidance_scale", 7.5))
    if g <= 1.0:
        raise ValueError("serve: guidance_scale must be > 1 (classifier-free guidance rows u_i / c_i)")
    wf = request.get("weight_func")
    if not weight_func_fused(wf):
        raise ValueError("serve: a custom weight_func is not supported (use txt2img)")
    for k in _UNSUPPORTED_KEYS:
        if request.get(k) is not None and not (b.t2i and k == "image_t2i_adapter") and not (b.cn and k == "control_img"):
            raise ValueError(f"serve: `{k}` (ControlNet / T2I-Adapter) is not supported (use txt2img)" + _FLAG_HINT.get(k, ""))
    if request.get("ip_adapter_image") is not None:
        raise ValueError("serve: `ip_adapter_image` (a raw image) is not supported: encode it once with pipe.encode_image and "
                         "pass `ip_adapter_image_embeds` ([negative; positive] per loaded adapter)")
    return out_type, v_pred, family, phi, g


def preview_request(b, request):
    """submit-time checks of the preview keys -> (preview_every, on_preview); (0, None): no previews"""
    every, call = request.get("preview_every"), request.get("on_preview")
    if every is not None and (isinstance(every, bool) or not isinstance(every, int) or every < 0):
        raise ValueError(f"serve: `preview_every` must be an integer >= 1 (absent, None or 0: no previews), got {every!r}")
    if call is not None and not callable(call):
        raise ValueError(f"serve: `on_preview` must be a callable f(step, steps, image), got {type(call).__name__}")
    if not every:
        return 0, None                                           # (a callback alone is accepted and never called)
    if not b.previews:
        raise ValueError("serve: `preview_every` (live previews) is not supported by this batcher: build it with `previews=True` "
                         "(pipe.serve(..., previews=True))")
    if call is None:
        raise ValueError("serve: `preview_every` needs `on_preview`, a callable f(step, steps, image)")
    return every, call


def check_freeu_off(pipe):
    """a batcher's steps take FreeU per request (`freeu=True`) or not at all: the UNet-level setting would enter every capture made
    from here on, for every row"""
    setting = getattr(getattr(pipe, "unet", None), "freeu_setting", None)
    if setting is not None and setting() is not None:
        raise ValueError("serve: the UNet-level FreeU setting is on (unet.enable_freeu); a batcher takes FreeU per request: call "
                         "unet.disable_freeu(), build the batcher with `freeu=True` and pass `freeu=(s1, s2, b1, b2)` in the requests")


def freeu_request(b, request):
    """submit-time check of `freeu` -> (s1, s2, b1, b2) as four finite floats, or None (absent)"""
    v = request.get("freeu")
    if v is None:
        return None
    if not getattr(b, "freeu", False):
        raise ValueError("serve: `freeu` (FreeU per request) is not supported by this batcher" + _FLAG_HINT["freeu"])
    try:
        return ops.freeu_values(v)
    except ValueError as e:
        raise ValueError(f"serve: `freeu` must be four finite numbers (s1, s2, b1, b2) or a dict with those names: {e}") from None


def text_request(b, request):
    """the prompt embeddings -> (negative, positive), [1, S, ctx] each at this batcher's text length"""
    pos, neg = request.get("prompt_embeds"), request.get("negative_prompt_embeds")
    if pos is None or neg is None:
        raise ValueError("serve: a request needs prompt_embeds and negative_prompt_embeds ([1, S, ctx] each)")
    if pos.dim() != 3 or pos.shape[0] != 1 or neg.shape != pos.shape:
        raise ValueError("serve: prompt_embeds / negative_prompt_embeds must both be [1, S, ctx]")
    if pos.shape[1] > MAX_TEXT_KEYS:
        raise ValueError(f"serve: {pos.shape[1]} text keys; the batcher's kernels take at most {MAX_TEXT_KEYS} (use txt2img)")
    if pos.shape[1] != b.text_len:
        raise ValueError(f"serve: this batcher runs {b.text_len} text keys, the request has {pos.shape[1]}")
    return neg, pos


def prompt_request(b, request):
    """submit-time checks of `prompt` / `negative_prompt` on a batcher built with `text=True` -> the request's handle on the text
    lane (host work only: parsing, chunking, padding to the batcher's chunk count), or None when it carries no `prompt` (it then
    brings its embeddings: text_request)"""
    from . import text_lane
    prompt = request.get("prompt")
    if prompt is None:
        return None
    for key in ("prompt_embeds", "negative_prompt_embeds", "text_input_ids"):
        if request.get(key) is not None:
            raise ValueError(f"serve: `prompt` and `{key}` are given together; a request brings its prompt as strings (the text "
                             f"lane encodes them and makes the ids) or as embeddings, not both")
    negative = request.get("negative_prompt")
    negative = "" if negative is None else negative
    if not isinstance(prompt, str) or not isinstance(negative, str):
        raise ValueError(f"serve: `prompt` / `negative_prompt` are one string each (one image per request), got "
                         f"{type(prompt).__name__} / {type(negative).__name__}")
    long_encode = request.get("long_encode", 0)
    if long_encode != 0:                                         # (encode_prompt_function's own test: False is 0)
        raise ValueError(f"serve: `long_encode` {long_encode!r} is not served: the text lane runs the default branch of "
                         f"encode_prompt_function (long_encode = 0); encode in the client and pass the embeddings")
    if "clip_skip" in request and text_lane.effective_skip(request["clip_skip"]) != text_lane.effective_skip(b.clip_skip):
        raise ValueError(f"serve: `clip_skip` {request['clip_skip']!r} differs from this batcher's ({b.clip_skip!r}): the lane's "
                         f"captured encoder ends at one layer (build a batcher with pipe.serve(..., text=True, clip_skip=...))")
    return text_lane.prompt_chunks(b._parser, negative, prompt, b.text_len // text_lane.CHUNK, b.text_len)


def adapter_request(b, request):
    """submit-time checks of the T2I-Adapter keys -> {"image", "scale", "factor"} or None (no control image, or nothing to
    add: every scale 0 / factor 0)"""
    image = request.get("image_t2i_adapter")
    if not b.t2i:
        return None                                              # (the key itself is refused with the other unsupported keys)
    from ..t2i_adapter import MultiAdapter
    if getattr(b.pipe, "adapter", None) is not b._adapter:
        raise RuntimeError("serve: the pipeline's T2I-Adapter changed since this batcher was built (setup_model_t2i_adapter): "
                           "build a new one with pipe.serve(..., t2i_adapter=True)")
    multi = isinstance(b._adapter, MultiAdapter)
    n = b._adapter.num_adapter if multi else 1
    scale, factor = request.get("adapter_conditioning_scale", 1.0), request.get("adapter_conditioning_factor", 1.0)
    scale = per_item("adapter_conditioning_scale", 1.0 if scale is None else scale, n, "pipe.adapter", lists=multi)
    factor = fraction("adapter_conditioning_factor", 1.0 if factor is None else factor)
    if image is None:
        return None
    if request.get("upscale"):
        raise ValueError("serve: `image_t2i_adapter` with `upscale` (a control image in the hires pass) is not served yet; use "
                         "txt2img")
    cin = (b._adapter.adapters[0] if multi else b._adapter).config.in_channels
    images = control_images("image_t2i_adapter", image, multi, [cin] * n, "pipe.adapter", size=(b.height, b.width))
    if factor == 0.0 or all(v == 0.0 for v in scale):
        return None                                              # nothing to add: no adapter forward, the rows stay skipped
    return {"image": images if multi else images[0], "scale": scale if multi else scale[0], "factor": factor}


def control_request(b, request, second=False):
    """submit-time checks of the ControlNet keys -> {"image": [one per net], "scale", "start", "end": one float per net} or
    None (no control image).  Whether any model call carries it is decided once the schedule is known (_prepare)."""
    image = request.get("control_img")
    if not b.cn:
        return None                                              # (the key itself is refused with the other unsupported keys)
    from ..controlnet import MultiControlNetModel
    if getattr(b.pipe, "controlnet", None) is not b._controlnet:
        raise RuntimeError("serve: the pipeline's ControlNet changed since this batcher was built (setup_controlnet): build a "
                           "new one with pipe.serve(..., controlnet=True)")
    nets = b._control_nets()
    per_net = {}
    for key, default in (("controlnet_conditioning_scale", 1.0), ("control_guidance_start", 0.0), ("control_guidance_end", 1.0)):
        v = request.get(key)
        per_net[key] = per_item(key, default if v is None else v, len(nets), "pipe.controlnet")
    if image is None:
        return None
    if request.get("upscale") or second or b._hires is not None:
        raise ValueError("serve: `control_img` with `upscale` / on a chained hires pair (a ControlNet in the hires pass) is not "
                         "served yet; use txt2img")
    if request.get("mask_image") is not None:
        raise ValueError("serve: `control_img` with `mask_image` (a ControlNet with inpainting) is not served yet; use inpaiting")
    images = control_images("control_img", image, isinstance(b._controlnet, MultiControlNetModel),
                            [int(net.controlnet_cond_embedding.conv_in.in_channels) for net in nets], "pipe.controlnet")
    return {"image": images, "scale": per_net["controlnet_conditioning_scale"], "start": per_net["control_guidance_start"],
            "end": per_net["control_guidance_end"]}


def check_ip_current(b):
    """the captured steps were built for the IP-Adapter processors of construction time (their to_k_ip / to_v_ip, the static
    buffers' layout): a batcher that has seen load_ip_adapter / unload_ip_adapter since is stale"""
    now = _ip_layers(b.pipe)
    proj = getattr(b.pipe.unet, "encoder_hid_proj", None) if now else None
    if len(now) != len(b._ip) or any(a[1] is not c[1] for a, c in zip(now, b._ip)) or proj is not b._ip_proj:
        raise RuntimeError("serve: the pipeline's IP-Adapter processors changed since this batcher was built (load_ip_adapter / "
                           "unload_ip_adapter): its captured steps are stale - build a new one with pipe.serve(...)")


def ip_request(b, request):
    """submit-time checks of the image-prompt keys -> (embeds or None, one scale per loaded adapter; all 0 without embeds)"""
    n = len(b._ip_tokens)
    embeds, scale = request.get("ip_adapter_image_embeds"), request.get("ip_adapter_scale")
    if scale is None:
        scale = [float(v) for v in b._ip[0][1].scale] if n else []
    scale = per_item("ip_adapter_scale", scale, n, "the pipeline's loaded IP-Adapters")
    if embeds is None:
        return None, [0.0] * n
    if n == 0:
        raise ValueError("serve: `ip_adapter_image_embeds` on a pipeline without an IP-Adapter (pipe.load_ip_adapter first, then "
                         "build the batcher)")
    if not isinstance(embeds, (list, tuple)) or len(embeds) != n:
        got = len(embeds) if isinstance(embeds, (list, tuple)) else type(embeds).__name__
        raise ValueError(f"serve: `ip_adapter_image_embeds` must be a list with one tensor per loaded IP-Adapter ({n}), got {got}")
    for a, (e, t) in enumerate(zip(embeds, b._ip_tokens)):
        if not torch.is_tensor(e) or e.dim() < 3 or e.shape[0] != 2:
            raise ValueError(f"serve: `ip_adapter_image_embeds[{a}]` must be [negative; positive] along dim 0 ([2, 1, ...], what "
                             f"txt2img takes), got {list(e.shape) if torch.is_tensor(e) else type(e).__name__}")
        if e.shape[1] != 1:
            raise ValueError(f"serve: `ip_adapter_image_embeds[{a}]` holds {e.shape[1]} images = {e.shape[1] * t} image tokens, "
                             f"adapter {a} has {t} tokens per request in the batcher (one image; use txt2img for more)")
    if all(v == 0.0 for v in scale):
        return None, scale                                      # nothing to add: no projection work, the rows stay skipped
    return list(embeds), scale


def ip_masks_of(b, request):
    """submit-time checks of `ip_adapter_masks` (cross_attention_kwargs) -> the [n_adapters, 1, Hm, Wm] tensor or None"""
    kw = request.get("cross_attention_kwargs")
    masks = kw.get("ip_adapter_masks") if isinstance(kw, dict) else None
    if masks is None:
        return None
    if not b.ip_masks:
        raise ValueError("serve: `ip_adapter_masks` (cross_attention_kwargs) are not supported by this batcher: build it with "
                         "`ip_masks=True` (pipe.serve(..., ip_masks=True)), or use txt2img")
    n = len(b._ip_tokens)
    if not torch.is_tensor(masks) or masks.ndim != 4 or masks.shape[1] != 1:
        raise ValueError(f"serve: `ip_adapter_masks` must be a tensor of shape [num_ip_adapter, 1, height, width], got "
                         f"{list(masks.shape) if torch.is_tensor(masks) else type(masks).__name__}")
    if masks.shape[0] != n:
        raise ValueError(f"serve: `ip_adapter_masks` holds {masks.shape[0]} masks, the pipeline has {n} IP-Adapter(s) loaded")
    if not torch.is_floating_point(masks) or masks.shape[2] < 1 or masks.shape[3] < 1 or not bool(torch.isfinite(masks).all()):
        raise ValueError("serve: `ip_adapter_masks` must hold finite floating-point values")
    return masks


def ip_mask_weights(b, masks):
    """once per request: per adapter {L: [L] fp16}, its mask down-sampled to every cross-attention level of THIS batcher as
    the processors' eager route does per layer and step (IPAdapterMaskProcessor.downsample in the mask's own dtype, then the
    query dtype: attention_modify.py:373-376 + :381 / :672-675 + :681)"""
    from ..attention_modify import IPAdapterMaskProcessor
    return [{L: IPAdapterMaskProcessor.downsample(masks[a], 1, L, 1)[0, :, 0].to(torch.float16) for L in b.levels()}
            for a in range(masks.shape[0])]


def hires_request(b, request):
    """a request with `upscale=True` on a chained pair: the checks of the hires keys -> the (first pass, second pass) request
    dicts; each is then validated like any request, by its own batcher"""
    hi = b._hires
    if hi is None:
        raise ValueError("serve: `upscale` (the hires pass) needs a chained pair of batchers (pipe.serve_hires, or chain_hires "
                         "on two batchers); this one is not chained (or use the pipeline methods)")
    if request.get("mask_image") is not None:
        raise ValueError("serve: `mask_image` with `upscale` is not supported (inpaiting refuses the hires pass too)")
    x = request.get("upscale_x", 2.0)
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not x > 0:
        raise ValueError(f"serve: `upscale_x` must be a positive number, got {x!r}")
    th, tw = hires_target_size(b.height, b.width, x, b.pipe.vae_scale_factor)
    if th < b.height or tw < b.width:
        raise ValueError(f"serve: `upscale_x` {x} shrinks {b.height}x{b.width} to {th}x{tw}; only enlarging is served "
                         "(use txt2img / img2img with upscale=True)")
    if (th, tw) != (hi.height, hi.width):
        raise ValueError(f"serve: `upscale_x` {x} asks for a {th}x{tw} hires pass, the chained batcher runs "
                         f"{hi.height}x{hi.width}")
    method = request.get("upscale_method", "bicubic")
    if method not in _RESAMPLE_MODES:
        raise ValueError(f"serve: `upscale_method` {method!r} is not one of {', '.join(_RESAMPLE_MODES)}")
    name2 = request.get("sampler_name_hires") or request.get("sampler_name") or "dpmpp_2m"
    if sampling.linear_family(name2) is None:
        raise ValueError(f"serve: `sampler_name_hires` {getattr(name2, '__name__', name2)!r} has no per-row step (supported: "
                         f"{', '.join(sampling.LINEAR_FAMILY)}; use txt2img)")
    if b.ip_masks and not hi.ip_masks and ip_masks_of(b, request) is not None:
        raise ValueError("serve: `ip_adapter_masks` with `upscale`: the chained hires batcher was built without `ip_masks=True` "
                         "(pipe.serve_hires(..., ip_masks=True) builds both with it)")
    noise = request.get("hires_latents")
    want = (1, 4, th // 8, tw // 8)
    if noise is not None and (not torch.is_tensor(noise) or tuple(noise.shape) != want):
        raise ValueError(f"serve: `hires_latents` (the unit noise of the hires pass) must be a {list(want)} tensor, got "
                         f"{list(noise.shape) if torch.is_tensor(noise) else type(noise).__name__}")
    drop = ("upscale", "image", "strength", "latents", "step_noise", "height", "width", "output_type")
    first = {k: v for k, v in request.items() if k not in ("upscale", "output_type")}
    second = {k: v for k, v in request.items() if k not in drop}
    second.update(sampler_name=name2, sampler_opt=request.get("sampler_opt_hires") or request.get("sampler_opt") or {},
                  strength=request.get("upscale_denoising_strength", 0.7), output_type=request.get("output_type", "latent"))
    if "region_map_state_hires" in request:
        second["region_map_state"] = request["region_map_state_hires"]
    return first, second


def image_request(b, r):
    """kind / strength of the request and the submit-time rejections of the image keys -> first index of its schedule"""
    req, pipe = r.req, b.pipe
    image, mask = req.get("image"), req.get("mask_image")
    if req.get("padding_mask_crop") is not None:
        raise ValueError("serve: `padding_mask_crop` is not supported (use inpaiting)")
    if b.inpaint and (image is None or mask is None):
        raise ValueError("serve: a batcher built with `inpaint_unet=True` serves inpainting requests only - every request needs "
                         "`image` and `mask_image` (an inpainting UNet has no txt2img)")
    if r.second:                             # the hires pass: img2img from the latent the hand-off writes
        r.kind = "img2img"
        r.strength = float(req.get("strength", 0.7))
        keep = min(int(r.steps * r.strength), r.steps) if 0.0 < r.strength <= 1.0 else 0               # :637-638
        if keep < 1:
            raise ValueError(f"serve: `upscale_denoising_strength` {r.strength} leaves none of the {r.steps} steps of the "
                             "hires pass (it must be in (0, 1])")
        return max(r.steps - keep, 0)
    if image is None:
        if mask is not None:
            raise ValueError("serve: `mask_image` needs `image`")
        if req.get("strength") is not None:
            raise ValueError("serve: `strength` needs `image` (txt2img starts from pure noise)")
        return 0
    # "inpaint_unet": the 9-channel UNet reads the mask and the masked image as input channels - no known region, no blend
    r.kind = "img2img" if mask is None else "inpaint_unet" if b.inpaint else "inpaint"
    r.strength = float(req.get("strength", 1.0))
    if not 0.0 < r.strength <= 1.0:
        raise ValueError(f"serve: `strength` must be in (0, 1], got {r.strength}")
    keep = min(int(r.steps * r.strength), r.steps)                                           # :637-638
    if keep < 1:
        raise ValueError(f"serve: `strength` {r.strength} leaves none of the {r.steps} steps")
    h, w = b.height // 8, b.width // 8
    size = _spatial_size(image)
    latents_in = torch.is_tensor(image) and image.dim() == 4 and image.shape[1] == 4
    if latents_in:
        if tuple(image.shape) != (1, 4, h, w):
            raise ValueError(f"serve: `image` latents {tuple(image.shape)}, this batcher needs {(1, 4, h, w)}")
    else:
        if size != (b.height, b.width) or (torch.is_tensor(image) and (image.dim() != 4 or image.shape[0] != 1)):
            raise ValueError(f"serve: `image` is {size}, this batcher runs one {b.height}x{b.width} image per request")
        if pipe.vae is None or not hasattr(pipe.vae, "encode"):
            raise ValueError("serve: `image` given as pixels needs a VAE with an encoder; pass [1, 4, h, w] latents")
    if b.inpaint:
        mil = req.get("masked_image_latents")
        if mil is None and latents_in:
            raise ValueError(f"serve: `image` given as latents needs `masked_image_latents` ([1, 4, {h}, {w}]: the masked image "
                             "cannot be built from latents); pass pixels, or both")
        if mil is not None and (not torch.is_tensor(mil) or tuple(mil.shape) != (1, 4, h, w)):
            raise ValueError(f"serve: `masked_image_latents` must be a {[1, 4, h, w]} tensor, got "
                             f"{list(mil.shape) if torch.is_tensor(mil) else type(mil).__name__}")
    if mask is not None:
        if pipe.unet.config.in_channels != 4 and not b.inpaint:
            raise ValueError("serve: `mask_image` on a 9-channel inpainting UNet is not supported by this batcher (use inpaiting, "
                             "or build the batcher with pipe.serve(..., inpaint_unet=True))")
        if _spatial_size(mask) not in ((b.height, b.width), (h, w)):
            raise ValueError(f"serve: `mask_image` is {_spatial_size(mask)}, this batcher needs {b.height}x{b.width} "
                             f"(or the latent size {h}x{w})")
    return max(r.steps - keep, 0)
