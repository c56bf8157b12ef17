"""k-diffusion text-to-image pipeline for the MI355X hot path - counterpart of reference
`source/modules/model_k_diffusion.py` (`ModelWrapper` :85-98, `StableDiffusionPipeline` :101-, `setup_unet`
:138-141, `get_scheduler` :143-146, `get_sigmas` :848-882, `prepare_latents` :428-456, `txt2img` :943-1231).

Scope (SURVEY.md 8a rows a6-a10, 8f and the callers around them): `txt2img` (:943-1231), `img2img` (:543-846), `inpaiting`
(:1365-1760; 4- and 9-channel UNets), hires upscale, ControlNet (`setup_controlnet` / `preprocess_controlnet`, :348-427),
T2I-Adapter, IP-Adapter (embeddings or raw images through `encode_image`), prompt strings through
`encoder_prompt_modify.encode_prompt_function` (all three `long_encode` branches), every sampler `app.py:170-220` lists, eps-
and v-prediction.  Latent previews (`latent_processing == 1`) return the list of per-model-call estimates as the reference does.
Not built (NotImplementedError): mask cropping, LoRA scaling of the text encoder, textual inversion.  `output_type="latent"` (an extra of this build) returns the final latents.

Two execution modes produce the same numbers:
  * protocol mode (`fused=False`): the reference's control flow - a `model_fn(x, sigma)` closure handed to
    `sampler(model_fn, latents, sigmas=...)` (:1175), any sampler callable.  The closure's body is graph-backed where nothing
    but (x, sigma) changes per call: one launch writes the static inputs, ONE replay of the captured UNet (+ ControlNet /
    adapter) step, one launch does CFG + eps -> denoised; otherwise (v-prediction, IP-Adapter embeddings, CFG rescale, 9-channel
    inpainting) it is the reference's eager sequence - duplicate the latent, attach `region_prompt`, `CompVisDenoiser` ->
    `ModelWrapper.apply_model` -> UNet, combine CFG (:1091-1171).
  * fused mode (`fused=True`, default for `sample_dpmpp_2m`): the UNet forward of one step is captured ONCE into a
    HIP graph over static buffers (sigma and the timestep are device scalars, so the same graph serves all 25
    steps); between replays ONE HIP launch (dsc_cfg_dpmpp2m_step) does CFG combine + eps->denoised + the DPM++ 2M
    update + the next step's `cat([x]*2) * c_in`.  No device->host sync inside the loop (the reference has two
    per step: `sigma.item()` :1115 and the sampler's `sigmas[i+1] == 0` test).
Batches of B > 1 images use the reference's row layout [u_0..u_{B-1}, c_0..c_{B-1}] (:1021,1097) with one std group
per image (`n_std_groups = B`), which is what B separate reference calls compute (the reference itself cannot batch:
external_k_diffusion.py:109-114 broadcasts c_in[B] against input[2B]).
"""
import contextlib
import gc
import importlib
import inspect
import os
import threading
import time
import weakref
from typing import List, Optional, Union

import torch

from .. import _lib, ops
from . import sampling
from .encode_region_map_function import encode_region_map
from .step_plan import step_plan, step_record
from .attention_modify import weight_func_fused
from .external_k_diffusion import CompVisDenoiser, CompVisVDenoiser


class ModelWrapper:
    def __init__(self, model, alphas_cumprod):
        self.model = model
        self.alphas_cumprod = alphas_cumprod

    def apply_model(self, *args, **kwargs):
        if len(args) == 3:
            encoder_hidden_states = args[-1]
            args = args[:2]
        if kwargs.get("cond", None) is not None:
            encoder_hidden_states = kwargs.pop("cond")
        return self.model(*args, encoder_hidden_states=encoder_hidden_states, **kwargs).sample


class SD15Scheduler:
    """Stand-in for the diffusers scheduler object the reference pipeline reads `alphas_cumprod` and
    `config.prediction_type` from (:138-141): scaled_linear betas 0.00085 -> 0.012, 1000 steps (SD1.5)."""

    def __init__(self, beta_start=0.00085, beta_end=0.012, num_train_timesteps=1000, prediction_type="epsilon"):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.config = type("Cfg", (), {"prediction_type": prediction_type})()


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """reference :71-82 (arXiv 2305.08891 sec. 3.4)"""
    dims = list(range(1, noise_pred_text.ndim))
    factor = noise_pred_text.std(dim=dims, keepdim=True) / noise_cfg.std(dim=dims, keepdim=True)
    return guidance_rescale * (noise_cfg * factor) + (1 - guidance_rescale) * noise_cfg


_CAPTURE_LOCK = threading.RLock()


@contextlib.contextmanager
def _capture_without_gc():
    """Around a stream capture.  A cyclic collection that starts INSIDE a capture finalizes whatever dead cycles exist at that
    moment - a dropped ServingBatcher and its executor refer to each other and hold CUDAGraphs, a stream, events and graph-pool
    memory - and releasing those while a global-mode capture is open aborted the process (seen in a batcher's capture after
    other batchers had been dropped; which collection lands inside a capture depends only on allocation counts).
    torch.cuda.graph used to collect before every capture and no longer does (torch >= 2.9, force_cudagraph_gc): collect here,
    outside the capture, and keep the collector off until the capture has ended."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


class StableDiffusionPipeline:
    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler, feature_extractor=None, image_encoder=None):
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.unet, self.scheduler = unet, scheduler
        self.feature_extractor, self.image_encoder = feature_extractor, image_encoder
        self.controlnet = None
        self.adapter = None                                  # T2I-Adapter, set by modules.t2i_adapter.setup_model_t2i_adapter
        self.vae_scale_factor = 8 if vae is None else 2 ** (len(vae.config.block_out_channels) - 1)
        self._do_classifier_free_guidance = True
        self._graphs = {}
        self._added_cond_kwargs = None
        self.weights_epoch = 0                               # counts the LoRA changes; a serving batcher serves the epoch it was built at
        self._batchers = weakref.WeakSet()                   # the ServingBatchers built on this pipeline (modules/serving/batcher.py)
        self._lora = None                                    # modules.lora.LoraManager, from the first load_lora_weights on
        self.setup_unet(self.unet)

    # ------------------------------------------------------------------ reference surface
    @property
    def device(self):
        return self.unet.device

    @property
    def _execution_device(self):
        return self.unet.device

    @property
    def do_classifier_free_guidance(self):
        return self._do_classifier_free_guidance

    def to(self, device):
        self.unet.to(device)
        self.k_diffusion_model.to(device)
        return self

    def setup_unet(self, unet):
        self.unet = unet
        model = ModelWrapper(unet, self.scheduler.alphas_cumprod)
        self.v_prediction = getattr(self.scheduler.config, "prediction_type", "epsilon") == "v_prediction"      # :138-141
        self.k_diffusion_model = CompVisVDenoiser(model) if self.v_prediction else CompVisDenoiser(model)
        self.k_diffusion_model.to(unet.device)
        self._graphs = {}
        self._drop_text_kv()

    def get_scheduler(self, scheduler_type: str):
        """reference :143-146 resolves the name in `k_diffusion.sampling`; here in the build's own sampling module"""
        return getattr(importlib.import_module(sampling.__name__), scheduler_type)

    def setup_controlnet(self, controlnet):
        """reference :348-353"""
        from .controlnet import MultiControlNetModel
        if isinstance(controlnet, (list, tuple)):
            controlnet = MultiControlNetModel(controlnet)
        self.controlnet = controlnet

    def prepare_image(self, image, width, height, batch_size, num_images_per_prompt, device, dtype,
                      do_classifier_free_guidance=False, guess_mode=False):
        """reference :483-515: the control image in [0, 1] (no normalisation) at (height, width), duplicated for CFG"""
        if not isinstance(image, torch.Tensor):
            image = (self._image_tensor(image, height, width) + 1.0) / 2.0
        elif tuple(image.shape[-2:]) != (height, width):
            image = torch.nn.functional.interpolate(image.float(), size=(height, width), mode="bilinear")
        image = image.to(device=device, dtype=dtype)
        if do_classifier_free_guidance and not guess_mode:
            image = torch.cat([image] * 2)
        return image

    def preprocess_controlnet(self, controlnet_conditioning_scale, control_guidance_start, control_guidance_end, image, width,
                              height, num_inference_steps, batch_size, num_images_per_prompt):
        """reference :355-427: (control image(s), keep schedule, guess_mode, conditioning scale(s))"""
        from .controlnet import ControlNetModel, MultiControlNetModel
        controlnet = self.controlnet
        multi = isinstance(controlnet, MultiControlNetModel)
        if not isinstance(control_guidance_start, list) and isinstance(control_guidance_end, list):
            control_guidance_start = len(control_guidance_end) * [control_guidance_start]
        elif not isinstance(control_guidance_end, list) and isinstance(control_guidance_start, list):
            control_guidance_end = len(control_guidance_start) * [control_guidance_end]
        elif not isinstance(control_guidance_start, list) and not isinstance(control_guidance_end, list):
            mult = len(controlnet.nets) if multi else 1
            control_guidance_start, control_guidance_end = mult * [control_guidance_start], mult * [control_guidance_end]
        if multi and isinstance(controlnet_conditioning_scale, float):
            controlnet_conditioning_scale = [controlnet_conditioning_scale] * len(controlnet.nets)
        first = controlnet.nets[0] if multi else controlnet
        guess_mode = bool(first.config.global_pool_conditions)
        prep = lambda im: self.prepare_image(im, width, height, batch_size, num_images_per_prompt, self._execution_device,  # noqa: E731
                                             controlnet.dtype, self.do_classifier_free_guidance, guess_mode)
        if multi:
            image = [prep(im) for im in image]
        elif isinstance(controlnet, ControlNetModel):
            image = prep(image)
        else:
            raise TypeError("setup_controlnet() takes a ControlNetModel or a list of them")
        keep = []
        for i in range(num_inference_steps):
            keeps = [1.0 - float(i / num_inference_steps < s or (i + 1) / num_inference_steps > e)
                     for s, e in zip(control_guidance_start, control_guidance_end)]
            keep.append(keeps if multi else keeps[0])
        return image, keep, guess_mode, controlnet_conditioning_scale

    def _controlnet_hook(self, control_img, controlnet_conditioning_scale, control_guidance_start, control_guidance_end,
                         width, height, n_steps, n_img, num_images_per_prompt, text):
        """The per-call ControlNet evaluation of the reference's model_fn (:1118-1152) as a function
        (latent_model_input, sigma) -> UNet keyword arguments; None when no ControlNet is set up."""
        if self.controlnet is None:
            return None
        if control_img is None:
            raise ValueError("a ControlNet is set up (setup_controlnet): pass control_img")
        scale = 1.0 if controlnet_conditioning_scale is None else controlnet_conditioning_scale
        start = 0.0 if control_guidance_start is None else control_guidance_start
        end = 1.0 if control_guidance_end is None else control_guidance_end
        img, keep, guess_mode, scale = self.preprocess_controlnet(scale, start, end, control_img, width, height, n_steps,
                                                                  n_img, num_images_per_prompt)
        seen = []
        kdm = self.k_diffusion_model
        cfg = self.do_classifier_free_guidance

        def schedule(key):
            """conditioning scale(s) of the model call at sigma `key`: one control step per DISTINCT sigma, in call order"""
            if key not in seen:                                 # (:1119-1123)
                seen.append(key)
            k = keep[min(len(seen) - 1, len(keep) - 1)]
            if isinstance(k, list):
                return [c * s_ for c, s_ in zip(scale, k)]
            return (scale[0] if isinstance(scale, list) else scale) * k

        def hook(latent_model_input, sigma):
            cond_scale = schedule(float(sigma[0]))
            down, mid = self.controlnet(latent_model_input / ((sigma[0] ** 2 + 1) ** 0.5), kdm.sigma_to_t(sigma),
                                        encoder_hidden_states=text, controlnet_cond=img, conditioning_scale=cond_scale,
                                        guess_mode=guess_mode, return_dict=False)
            if guess_mode and cfg:                              # inferred for the conditional rows only (:1143-1148)
                down = [torch.cat([torch.zeros_like(d), d]) for d in down]
                mid = torch.cat([torch.zeros_like(mid), mid])
            return {"down_block_additional_residuals": down, "mid_block_additional_residual": mid}
        hook.static = None if guess_mode else {"kind": "controlnet", "image": img, "schedule": schedule}
        return hook

    def _adapter_hook(self, image_t2i_adapter, adapter_conditioning_scale, adapter_conditioning_factor, width, height,
                      steps_denoising, num_images_per_prompt):
        """T2I-Adapter (reference :700-703, :722-731): the adapter's features are computed once; every model call during the
        first int(steps_denoising * factor) distinct sigmas hands clones of them to the UNet as
        `down_intrablock_additional_residuals`.  None when no adapter image is given."""
        if image_t2i_adapter is None:
            return None
        if getattr(self, "adapter", None) is None:
            raise ValueError("image_t2i_adapter needs an adapter: modules.t2i_adapter.setup_model_t2i_adapter(pipe, adapter)")
        from .t2i_adapter import preprocessing_t2i_adapter
        state = preprocessing_t2i_adapter(self, image_t2i_adapter, width, height, adapter_conditioning_scale, num_images_per_prompt)
        seen = []
        limit = int(steps_denoising * adapter_conditioning_factor)

        def schedule(key):
            use = len(seen) < limit
            if key not in seen:
                seen.append(key)
            return use

        def hook(latent_model_input, sigma):
            return {"down_intrablock_additional_residuals": [v.clone() for v in state]} if schedule(float(sigma[0])) else {}
        hook.static = {"kind": "adapter", "state": state, "schedule": schedule}
        return hook

    @staticmethod
    def _merge_hooks(*hooks):
        hooks = [h for h in hooks if h is not None]
        if not hooks:
            return None

        def merged(latent_model_input, sigma):
            out = {}
            for h in hooks:
                out.update(h(latent_model_input, sigma))
            return out
        statics = [getattr(h, "static", None) for h in hooks]
        merged.static = None if any(st_ is None for st_ in statics) else statics
        return merged

    def get_sigmas(self, steps, params):
        """reference :848-882"""
        discard = params.get("discard_next_to_last_sigma", False)
        steps += 1 if discard else 0
        named = {"karras": sampling.get_sigmas_karras, "exponential": sampling.get_sigmas_exponential,
                 "polyexponential": sampling.get_sigmas_polyexponential}
        if params.get("scheduler", None) in named:
            # sigma_min / sigma_max are constants of the model: read once (a device->host copy synchronises, and a
            # synchronisation per generation keeps the host from preparing generation i+1 under generation i's replays);
            # the 26-entry schedule is computed on the host
            kdm = self.k_diffusion_model
            rng = getattr(self, "_sigma_range", None)
            if rng is None or rng[0] is not kdm:
                rng = self._sigma_range = (kdm, kdm.sigmas[0].item(), kdm.sigmas[-1].item())
            sigmas = named[params["scheduler"]](n=steps, sigma_min=rng[1], sigma_max=rng[2], device="cpu")
        else:
            sigmas = self.k_diffusion_model.get_sigmas(steps)
        if discard:
            sigmas = torch.cat([sigmas[:-2], sigmas[-1:]])
        return sigmas

    def _schedule(self, steps, params, device, dtype):
        """get_sigmas() cast to the model dtype on the device (reference :1027-1029: fp16 rounding is part of the schedule).
        A host-computed schedule is rounded on the host (round-to-nearest-even, as the device cast), uploaded from pinned
        memory without blocking, and carries the rounded values as host floats (`_dsc_host`) for the fused loop."""
        s = self.get_sigmas(steps, params)
        device = torch.device(device)
        if s.is_cuda or device.type != "cuda":
            return s.to(device, dtype=dtype)
        h = s.to(dtype=dtype)
        d = h.pin_memory().to(device, non_blocking=True)
        d._dsc_host = h.float().tolist()
        return d

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        shape = (batch_size, num_channels_latents, height // 8, width // 8)
        if latents is None:
            gdev = generator.device if generator is not None else device
            latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
        else:
            latents = latents.to(device)
        return latents

    def get_sampler_extra_args_t2i(self, sigmas, eta, steps, sampler_opt, latents, seed, func):
        params = inspect.signature(func).parameters
        extra = {}
        if "eta" in params:
            extra["eta"] = eta
        if "sigma_min" in params:
            extra["sigma_min"], extra["sigma_max"] = sigmas[0].item(), sigmas[-1].item()
        if "n" in params:
            extra["n"] = steps
        else:
            extra["sigmas"] = sigmas
        if sampler_opt.get("brownian_noise", False):
            extra["noise_sampler"] = self.create_noise_sampler(latents, sigmas, steps, seed)
        if sampler_opt.get("solver_type", None) == "heun":
            extra["solver_type"] = "heun"
        return extra

    def create_noise_sampler(self, x, sigmas, p, seed):
        """reference :884-890 (BrownianTreeNoiseSampler seeded per generation; see sampling.BrownianTreeNoiseSampler for
        what the torchsde-free counterpart keeps of it)"""
        sigma_min, sigma_max = sigmas[sigmas > 0].min(), sigmas.max()
        return sampling.BrownianTreeNoiseSampler(x, sigma_min, sigma_max, seed=seed)

    @torch.no_grad()
    def decode_latents(self, latents):
        """reference :291-299: 1/scaling_factor, vae.decode, /2 + 0.5, clamp, NHWC float32 numpy"""
        latents = latents.to(self.device, dtype=self.vae.dtype)
        latents = 1 / self.vae.config.scaling_factor * latents
        image = self.vae.decode(latents).sample
        image = (image / 2 + 0.5).clamp(0, 1)
        return image.cpu().permute(0, 2, 3, 1).float().numpy()

    @staticmethod
    def numpy_to_pil(images):
        from PIL import Image
        if images.ndim == 3:
            images = images[None, ...]
        images = (images * 255).round().astype("uint8")
        return [Image.fromarray(im) for im in images]

    def latent_to_image(self, latents, output_type):
        """reference :533-539; output_type 'latent' (this build's extra) returns the latents untouched"""
        if output_type == "latent":
            return latents
        if self.vae is None:
            raise NotImplementedError("no VAE was given to the pipeline: pass output_type='latent' or construct it with a "
                                      "modules.vae_decoder.AutoencoderKLDecoder")
        image = self.decode_latents(latents)
        if output_type == "pil":
            image = self.numpy_to_pil(image)
        if len(image) > 1:
            return image
        return image[0]

    # ---- IP-Adapter surface (reference ip_adapter.py:48-292, state-dict form)
    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder=None, weight_name=None,
                        image_encoder_folder=None, **kwargs):
        """ip_adapter.py:48-239 restricted to what works offline: `pretrained_model_name_or_path_or_dict` must be a
        state dict {"image_proj": ..., "ip_adapter": ...} or a list of them; the CLIP image encoder is not loaded
        (pass `ip_adapter_image_embeds` to txt2img, as the reference's own warning at :219-222 suggests)."""
        sds = pretrained_model_name_or_path_or_dict
        if not isinstance(sds, list):
            sds = [sds]
        for sd in sds:
            if not isinstance(sd, dict) or sorted(sd.keys()) != ["image_proj", "ip_adapter"]:
                raise ValueError("Required keys are (`image_proj` and `ip_adapter`) missing from the state dict.")   # :191-192
        self._graphs = {}
        return self.unet._load_ip_adapter_weights(sds, low_cpu_mem_usage=False)

    def set_ip_adapter_scale(self, scale):
        """ip_adapter.py:242-264"""
        from .attention_modify import IPAdapterAttnProcessor, IPAdapterAttnProcessor2_0
        for proc in self.unet.attn_processors.values():
            if isinstance(proc, (IPAdapterAttnProcessor, IPAdapterAttnProcessor2_0)):
                sc = scale if isinstance(scale, list) else [scale] * len(proc.scale)
                if len(proc.scale) != len(sc):
                    raise ValueError(f"`scale` should be a list of same length as the number if ip-adapters "
                                     f"Expected {len(proc.scale)} but got {len(sc)}.")
                proc.scale = sc
        self._graphs = {}                            # the scales are baked into a captured step

    def unload_ip_adapter(self):
        """ip_adapter.py:266-292: drops the image projection and restores plain processors.  (The reference's
        has-SDPA test is inverted and installs `AttnProcessor`; both classes compute the same function)"""
        from .attention_modify import AttnProcessor
        self.unet.encoder_hid_proj = None
        self.unet.config["encoder_hid_dim_type"] = None
        self.unet.set_attn_processor(AttnProcessor())
        self._graphs = {}

    # ---- LoRA surface (reference app.py:532-597 `load_lora_control_pipeline`; modules/lora.py)
    def load_lora_weights(self, state_dict_or_safetensors_path, scale=1.0, name=None, use_alpha=False):
        """Merge a kohya-format LoRA (a state dict or a .safetensors path) into the UNet and the text encoder at `scale`, the
        reference's `lora_scale`; `use_alpha=False` skips the file's `.alpha` keys as the reference does, True multiplies by
        alpha / rank.  Several adapters may be loaded (`name`: default the file's stem / "lora<n>").  Captured steps are dropped
        and `weights_epoch` advances; a ServingBatcher built before the call refuses to go on.  -> the adapter's name"""
        from .lora import LoraManager
        if self._lora is None:
            self._lora = LoraManager(self)
        return self._lora.load(state_dict_or_safetensors_path, scale=scale, name=name, use_alpha=use_alpha)

    def set_lora_scale(self, scale):
        """a float for every loaded adapter, or {name: scale}: all touched weights are recomputed from their pristine copies"""
        if self._lora is None:
            raise ValueError("set_lora_scale: no LoRA is loaded")
        self._lora.set_scale(scale)

    def unload_lora_weights(self, name=None):
        """drop one adapter, or all: weights no adapter touches any more get their original bits back; after the last adapter
        the pristine copies and the packed operands are freed"""
        if self._lora is not None:
            self._lora.unload(name)

    def lora_state(self):
        """{"adapters": {name: {scale, use_alpha, layers, rank}}, "targets", "kernel_targets", "base_bytes", "weights_epoch"}"""
        from .lora import LoraManager
        return (self._lora or LoraManager(self)).state()

    def encode_image(self, image, device, num_images_per_prompt, output_hidden_states=None):
        """reference :148-170: CLIP image embeddings (or penultimate hidden states) of the IP-Adapter image and their
        unconditional counterpart; `image_encoder` is any transformers-style CLIPVisionModelWithProjection, `feature_extractor`
        its image processor"""
        if self.image_encoder is None:
            raise NotImplementedError("ip_adapter_image needs the pipeline's image_encoder (a CLIP vision model with "
                                      "projection) and feature_extractor; or pass ip_adapter_image_embeds")
        dtype = next(self.image_encoder.parameters()).dtype
        if not isinstance(image, torch.Tensor):
            image = self.feature_extractor(image, return_tensors="pt").pixel_values
        image = image.to(device=device, dtype=dtype)
        if output_hidden_states:
            pos = self.image_encoder(image, output_hidden_states=True).hidden_states[-2]
            neg = self.image_encoder(torch.zeros_like(image), output_hidden_states=True).hidden_states[-2]
            return pos.repeat_interleave(num_images_per_prompt, dim=0), neg.repeat_interleave(num_images_per_prompt, dim=0)
        emb = self.image_encoder(image).image_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        return emb, torch.zeros_like(emb)

    def prepare_ip_adapter_image_embeds(self, ip_adapter_image, ip_adapter_image_embeds, device, num_images_per_prompt,
                                        do_classifier_free_guidance):
        """Reference :173-222, pre-computed-embeddings branch (:203-221): each list entry holds [negative; positive]
        along dim 0 when CFG is on; both halves are repeated per image and re-concatenated."""
        if ip_adapter_image_embeds is None:                                                       # :176-201
            if not isinstance(ip_adapter_image, list):
                ip_adapter_image = [ip_adapter_image]
            layers = self.unet.encoder_hid_proj.image_projection_layers
            if len(ip_adapter_image) != len(layers):
                raise ValueError(f"`ip_adapter_image` must have same length as the number of IP Adapters. Got "
                                 f"{len(ip_adapter_image)} images and {len(layers)} IP Adapters.")
            from .u_net_condition_modify import ImageProjection
            out = []
            for img, layer in zip(ip_adapter_image, layers):
                hidden = not isinstance(layer, ImageProjection)            # Plus-style projections take hidden states
                pos, neg = self.encode_image(img, device, 1, hidden)
                pos = torch.stack([pos] * num_images_per_prompt, dim=0)
                neg = torch.stack([neg] * num_images_per_prompt, dim=0)
                if do_classifier_free_guidance:
                    pos = torch.cat([neg, pos]).to(device)
                out.append(pos)
            return out
        out = []
        for e in ip_adapter_image_embeds:
            ones = [1] * (e.dim() - 1)
            if do_classifier_free_guidance:
                neg, pos = e.chunk(2)
                e = torch.cat([neg.repeat(num_images_per_prompt, *ones), pos.repeat(num_images_per_prompt, *ones)])
            else:
                e = e.repeat(num_images_per_prompt, *ones)
            out.append(e)
        return out

    # ------------------------------------------------------------------ txt2img
    @torch.no_grad()
    def txt2img(self, prompt: Union[str, List[str], None] = None, height: int = 512, width: int = 512,
                num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None, eta: float = 0.0,
                generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None,
                output_type: Optional[str] = "pil", callback_steps: Optional[int] = 1, upscale=False, upscale_x: float = 2.0,
                upscale_method: str = "bicubic", upscale_antialias: bool = False, upscale_denoising_strength: float = 0.7,
                region_map_state=None, sampler_name="", sampler_opt={}, sampler_name_hires="", sampler_opt_hires={},
                start_time=-1, timeout=180,
                latent_processing=0, weight_func=lambda w, sigma, qk: w * sigma * qk.std(), seed=0,
                ip_adapter_image=None, control_img=None, controlnet_conditioning_scale=None, control_guidance_start=None,
                control_guidance_end=None, image_t2i_adapter=None, adapter_conditioning_scale=1.0,
                adapter_conditioning_factor: float = 1.0, guidance_rescale: float = 0.0,
                cross_attention_kwargs=None, clip_skip=None, long_encode=0, num_images_per_prompt=1,
                ip_adapter_image_embeds=None,
                # build-specific inputs (the prompt encoders are a "next" row):
                prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                text_input_ids=None, fused: Optional[bool] = None, slot: int = 0, step_noise: Optional[torch.Tensor] = None,
                two_call: bool = False, **unsupported):
        """reference :943-1231.  What is txt2img's own stands here; the rest is the shared path below (_text_and_schedule,
        _conditioning, _denoise_and_finish)."""
        a = dict(locals())                       # this call's arguments by name, as given: what the shared path reads
        if image_t2i_adapter is not None:        # (before any prompt work)
            if getattr(self, "adapter", None) is None:
                raise ValueError("image_t2i_adapter needs an adapter: modules.t2i_adapter.setup_model_t2i_adapter(pipe, adapter)")
            from .t2i_adapter import default_height_width
            height, width = default_height_width(self, height, width, image_t2i_adapter)              # :990-991
        sampler, text, text_input_ids, n_img, sigmas = self._text_and_schedule(a)
        latents = self.prepare_latents(n_img, self.unet.config.in_channels, height, width, text.dtype, self._execution_device,
                                       generator, latents)           # the only generator draw of the call
        latents = latents * (sigmas[0] ** 2 + 1) ** 0.5                                                      # :1043
        cond = self._conditioning(a, text, text_input_ids, n_img, sigmas, width, height, num_inference_steps)
        return self._denoise_and_finish(a, sampler, latents, sigmas, text, n_img, cond, height, width, num_inference_steps, eta,
                                        fused_by_default=True, protocol_kw={"slot": slot}, fused_kw={"slot": slot})

    def serve(self, height: int = 512, width: int = 512, max_batch: int = 8, slot: int = 0, buckets=(1, 2, 4, 8), text_len: int = 77,
              ip_masks: bool = False, t2i_adapter: bool = False, controlnet: bool = False, control_slots=None,
              decode: bool = False, decode_batch: int = 2, previews: bool = False, preview_scale: int = 8, preview_coef=None,
              preview_ring: int = 8, inpaint_unet: bool = False, freeu: bool = False, encode: bool = False, encode_batch: int = 2,
              two_call: bool = False, text: bool = False, text_batch: int = 2, clip_skip=None):
        """Continuous-batching server (modules/serving/): requests join a running batch at any step boundary, each at its own
        point of its own schedule, and leave when done.  Returns a `ServingBatcher` (submit / step / run_until_idle / start / stop /
        stats / warm).  `ip_masks=True` (IP-Adapters loaded): requests may carry the reference's
        `cross_attention_kwargs={"ip_adapter_masks": ...}`, the region mask of each image prompt.  `t2i_adapter=True` (an adapter
        set up with setup_model_t2i_adapter): requests may carry `image_t2i_adapter` / `adapter_conditioning_scale` /
        `adapter_conditioning_factor`.  `controlnet=True` (a ControlNet set up with setup_controlnet; not together with
        `t2i_adapter`): requests may carry `control_img` / `controlnet_conditioning_scale` / `control_guidance_start` /
        `control_guidance_end`; the ControlNet runs on `control_slots` compact lanes (default: max_batch), so a request without a
        control image does not pay for its neighbours'.  `decode=True` (a pipeline with a VAE decoder): requests may ask for
        finished images - `output_type` "pil", "np" (float32 [H, W, 3]) or "uint8" (np.uint8 [H, W, 3]) - which a decode lane
        on a second stream produces beside the step, up to `decode_batch` (in [1, max_batch]) rows per captured decode; without
        it image output types run `latent_to_image` inline, as before, and "uint8" is refused.  `previews=True`: requests may
        carry `preview_every=k` and `on_preview=f`; after every k-th of a request's steps but the last, `f(step, steps, image)`
        receives an approximate np.uint8 [h * preview_scale, w * preview_scale, 3] thumbnail of its denoised estimate (h, w: the
        latent's sides; `preview_scale` in {1, 2, 4, 8} with a thumbnail width that is a multiple of 8; `preview_coef`: C * 3 + 3
        numbers, the latent-to-RGB matrix k[c][rgb] then a bias, default ops.LATENT_RGB_SD15) made by one launch beside the step
        and copied out on a second stream through a ring of `preview_ring` pinned buffers; a preview that finds the ring full
        is dropped, never waited for.  `inpaint_unet=True` (a 9-channel inpainting UNet; not together with `controlnet` /
        `t2i_adapter`): every request is an inpainting request (`image`, `mask_image`, optional `masked_image_latents` /
        `strength`) with any served sampler, v-prediction and `guidance_rescale`; every step writes the request's mask and
        masked-image latents behind its latent row (dsc_cfg_linear_step_rows_cat).  `freeu=True`: requests may carry
        `freeu=(s1, s2, b1, b2)` (or a dict with those names), FreeU per request: the captured steps hold the six FreeU launches
        (dsc_freeu_rows_f16), which read each row's values from a table and leave rows without the key as they are; it combines
        with every other flag.  `encode=True` (a pipeline whose VAE has an encoder, in fp16 on the GPU): requests whose `image` /
        `mask_image` are pixels are encoded on an encode lane - a second stream with one captured `vae.encode` per bucket, up to
        `encode_batch` (in [1, max_batch]) rows per encode, between one dsc_image_prepare and one dsc_latent_start_rows launch -
        beside the step: `submit` does host work and the request's draws only, and the request is admitted when its encode has
        completed; without it pixel inputs are prepared inline inside `submit`, as before.  `two_call=True` (not together with
        `inpaint_unet`): requests may name a sampler of sampling.TWO_CALL_FAMILY (Heun, DPM2, DPM2 a, DPM++ 2S a, DPM++ SDE) with
        `eta` / `s_noise` / `seed` / `step_noise` (one row per model call, sampling.call_noise_table); such a request advances by
        one model call per transition, two per sampler step (dsc_cfg_staged_step_rows), beside requests of the one-call samplers;
        not with `control_img` / `image_t2i_adapter`.  `text=True` (pipe.text_encoder is modules.clip_text.CLIPTextModel in fp16
        on the GPU, `text_len` a multiple of 77): requests may carry `prompt` / `negative_prompt` strings in place of the
        embeddings and ids; a text lane - a stream with one captured encoder per bucket, up to `text_batch` (request, chunk)
        groups per encode, and one dsc_prompt_weight_rows_f16 launch behind it - serves encode_prompt_function's default branch
        beside the step (`clip_skip`: the batcher's, fixed at construction), `submit` does host work only, and
        `batcher.encode_text(prompt, negative_prompt)` returns the embeddings synchronously.  Any batcher is refused while the
        UNet-level setting (unet.enable_freeu) is on."""
        from .serving import ServingBatcher
        kw = dict(previews=True, preview_scale=preview_scale, preview_coef=preview_coef, preview_ring=preview_ring) if previews else {}
        if inpaint_unet:                         # (a batcher built without the flag is constructed exactly as before)
            kw["inpaint_unet"] = True
        if freeu:
            kw["freeu"] = True
        if encode:
            kw.update(encode=True, encode_batch=encode_batch)
        if two_call:
            kw["two_call"] = True
        if text:
            kw.update(text=True, text_batch=text_batch, clip_skip=clip_skip)
        return ServingBatcher(self, height, width, max_batch=max_batch, slot=slot, buckets=buckets, text_len=text_len,
                              ip_masks=ip_masks, t2i_adapter=t2i_adapter, controlnet=controlnet, control_slots=control_slots,
                              decode=decode, decode_batch=decode_batch, **kw)

    def serve_hires(self, height: int = 512, width: int = 512, upscale_x: float = 1.25, max_batch: int = 8, buckets=(1, 2, 4, 8),
                    text_len: int = 77, slots=(0, 1), ip_masks: bool = False, decode: bool = False, decode_batch: int = 2,
                    previews: bool = False, preview_scale: int = 8, preview_coef=None, preview_ring: int = 8,
                    inpaint_unet: bool = False, freeu: bool = False, encode: bool = False, encode_batch: int = 2,
                    two_call: bool = False, text: bool = False, text_batch: int = 2, clip_skip=None):
        """Continuous-batching server for requests with a hires pass (reference :1176-1228): a batcher at `height` x `width`
        chained to one at the target size of `upscale_x` (_hires_pass's expression), on two workspace slots.  A request with
        `upscale=True` runs its first pass on the one, is enlarged and re-noised on the device (dsc_latent_resample_noise) and
        finishes on the other; requests without it are served at the base size as by `serve`.  Returns a `HiresPair` with the
        batcher's surface (submit / step / run_until_idle / start / stop / stats / warm).  `ip_masks=True` builds both batchers for
        `ip_adapter_masks` (see `serve`); the second pass down-samples a request's mask at its own levels.  `decode=True` gives
        each batcher a decode lane at its own image size (see `serve`): a request without `upscale` finishes on the base batcher.
        `previews=True` gives both batchers the preview path (see `serve`): each pass of a request with `upscale` counts its own
        steps, and the second pass previews at its own size.  `freeu=True` builds both batchers for per-request FreeU (see
        `serve`): both passes of a request get its values.  `encode=True` gives the encode lane (see `serve`) to the base-size batcher
        only: the second pass starts from the hand-off's latent, never from pixels.  `text=True` gives the text lane (see `serve`)
        to the base-size batcher only: a request with `prompt` and `upscale` is encoded once, and its second pass shares the
        first's text rows and ids (which also serve `region_map_state_hires`)."""
        from .latent_resample import hires_target_size
        from .serving import HiresPair, ServingBatcher
        if two_call:
            raise ValueError("serve_hires: `two_call=True` is not served (the two-call samplers run on a batcher built with "
                             "pipe.serve(..., two_call=True))")
        if inpaint_unet:
            raise ValueError("serve_hires: `inpaint_unet=True` is not served (inpaiting refuses the hires pass too); build the "
                             "batcher with pipe.serve(..., inpaint_unet=True)")
        th, tw = hires_target_size(height, width, upscale_x, self.vae_scale_factor)
        if th < height or tw < width:
            raise ValueError(f"serve_hires: upscale_x {upscale_x} shrinks {height}x{width} to {th}x{tw}; only enlarging is served "
                             "(use txt2img / img2img with upscale=True)")
        if len(slots) != 2:
            raise ValueError("serve_hires: `slots` names two workspace slots, one per batcher")
        # REMAINING ITEM: the UNet now hands the skip connection's size to each upsampler (the reference's `upsample_size`,
        # u_net_condition_modify.py:1116-1300) and runs any latent size: txt2img(upscale=True, upscale_x=1.2), serve(608, 608) and a
        # HiresPair built by hand from a 512 and a 608 batcher all work.  This guard is stale and stays only because an existing
        # test pins its ValueError (tests/test_hires_host.py, the 1.2 case); removing the six lines below together with that
        # assertion is the follow-up.  Until then the app's default factor 1.2 is served through a hand-built pair.
        m = 2 ** (len(self.unet.down_blocks) - 1)
        if (th // 8) % m or (tw // 8) % m:
            raise ValueError(f"serve_hires: a {th}x{tw} hires pass has {th // 8}x{tw // 8} latents; this package's UNet does not yet "
                             f"forward the skip sizes to its upsamplers (the reference's `upsample_size`), so latents must be "
                             f"multiples of {m} (txt2img(upscale=True) has the same limit).  Choose an upscale_x whose target is a "
                             f"multiple of {8 * m} pixels, e.g. 1.25 or 1.5 at 512")
        kw = dict(max_batch=max_batch, buckets=buckets, text_len=text_len, ip_masks=ip_masks)
        if decode:                               # (a pair built without the flag is constructed exactly as before)
            kw.update(decode=True, decode_batch=decode_batch)
        if previews:
            kw.update(previews=True, preview_scale=preview_scale, preview_coef=preview_coef, preview_ring=preview_ring)
        if freeu:
            kw["freeu"] = True
        base_kw = dict(kw, encode=True, encode_batch=encode_batch) if encode else kw
        if text:
            base_kw = dict(base_kw, text=True, text_batch=text_batch, clip_skip=clip_skip)
        return HiresPair(ServingBatcher(self, height, width, slot=slots[0], **base_kw), ServingBatcher(self, th, tw, slot=slots[1], **kw))

    def txt2img_coalesced(self, requests, height: int = 512, width: int = 512, num_inference_steps: int = 50,
                          guidance_scale: float = 7.5, sampler_opt=None, output_type: Optional[str] = "latent",
                          weight_func=lambda w, sigma, qk: w * sigma * qk.std(), cross_attention_kwargs=None,
                          start_time=-1, timeout=180, slot: int = 0):
        """k CONCURRENT batch-1 requests - each with its own prompt rows, region masks and start latent - denoised together by ONE
        captured UNet step per sigma (serving mode; the reference serialises requests: Gradio `queue()`, app.py:3063, one latent
        per `txt2img` call).  What the requests must share is what the step itself shares: image size, step count / schedule
        (DPM++ 2M, `sampler_opt`), guidance scale.

        Every request keeps the arithmetic of its own one-image call: the rows are laid out `[u_0..u_{k-1}, c_0..c_{k-1}]`
        (model_k_diffusion.py:1021,1097), request i's std group is rows {i, k + i} (`n_std_groups = k`: the std of
        attention_modify.py:96 taken over ONE image's rows), its region tables ride on exactly those two rows
        (quirk q1: both carry the cond table), and nothing else in the UNet couples rows - so image i equals the result of
        `txt2img(**requests[i])` to launch-geometry rounding (tests/test_full_size_parity_gpu.py::
        test_coalesced_requests_equal_their_single_runs), while every kernel of the step runs on k times the rows.

        requests: list of dicts with `prompt_embeds` [1, S, ctx], `negative_prompt_embeds` [1, S, ctx], `text_input_ids`
        ([negative ids, positive ids] or None), `region_map_state` (the UI's {phrase: {map, weight, mask_outsides}} or None) and
        `latents` [1, 4, h/8, w/8] (or `generator`).  Returns the list of per-request outputs (`latent_to_image`)."""
        k = len(requests)
        if k < 1:
            raise ValueError("txt2img_coalesced: no requests")
        if guidance_scale <= 1.0 or self.v_prediction:
            raise NotImplementedError("coalesced requests run the fused classifier-free-guidance loop (guidance_scale > 1, eps-prediction)")
        device = self._execution_device
        self._do_classifier_free_guidance = True
        self._added_cond_kwargs = None
        dt = self.unet.dtype
        neg = torch.cat([r["negative_prompt_embeds"] for r in requests]).to(device=device, dtype=dt)
        pos = torch.cat([r["prompt_embeds"] for r in requests]).to(device=device, dtype=dt)
        if neg.shape != pos.shape or pos.shape[0] != k:
            raise ValueError("txt2img_coalesced: one [1, S, ctx] prompt / negative prompt pair per request, equal S")
        text = torch.cat([neg, pos])                                                                         # [u_0.., c_0..]
        sigmas = self._schedule(num_inference_steps, sampler_opt or {}, device, dt)
        lats = []
        for r in requests:
            lats.append(self.prepare_latents(1, self.unet.config.in_channels, height, width, dt, device, r.get("generator"),
                                             r.get("latents")))
        latents = torch.cat(lats) * (sigmas[0] ** 2 + 1) ** 0.5                                              # :1043
        # per-request tables {L: [2, L, S]} (rows u, c) -> {L: [2k, L, S]} in the batch's row order
        per = [encode_region_map(self, r.get("region_map_state"), width=width, height=height, num_images_per_prompt=1,
                                 text_ids=r.get("text_input_ids") or [None, None]) for r in requests]
        region_state = self._coalesce_region_tables(per)
        latents = self._denoise_fused(latents, sigmas, text, region_state, weight_func, guidance_scale, k,
                                      {} if cross_attention_kwargs is None else cross_attention_kwargs, start_time, timeout, slot=slot)
        return [self.latent_to_image(latents[i:i + 1], output_type) for i in range(k)]

    @staticmethod
    def _coalesce_region_tables(per):
        """per-request tables [{L: [2, L, S]} (rows uncond, cond) or a non-dict] -> ONE {L: [2k, L, S]} in the batch's row order
        [u_0..u_{k-1}, c_0..c_{k-1}]: the kernels read table row b for batch row b (repeat_interleave(w, H) of
        attention_modify.py:97-99 with Bw == Bc).  A request without masks rides along with zero tables (quirk q2: the region
        path with a zero bias is the plain one); no request with masks -> the first request's non-dict state (region path off)."""
        has = [isinstance(t, dict) and bool(t) for t in per]
        if not any(has):
            return per[0]
        ref = per[has.index(True)]
        per = [t if h else {L: torch.zeros_like(w) for L, w in ref.items()} for t, h in zip(per, has)]
        for t in per:
            if sorted(t) != sorted(ref) or any(t[L].shape != ref[L].shape or t[L].shape[0] != 2 for L in ref):
                raise ValueError("txt2img_coalesced: the requests' region tables differ in levels / shape (same image size and prompt length needed)")
        return {L: torch.cat([t[L][0:1] for t in per] + [t[L][1:2] for t in per]) for L in ref}

    def get_sampler_extra_args_i2i(self, sigmas, steps, sampler_opt, latents, seed, func):
        """reference :916-941"""
        params = inspect.signature(func).parameters
        extra = {}
        if "sigma_min" in params:
            extra["sigma_min"] = sigmas[-2]              # the last sigma is zero, which DPM fast / adaptive do not allow
        if "sigma_max" in params:
            extra["sigma_max"] = sigmas[0]
        if "n" in params:
            extra["n"] = len(sigmas) - 1
        if "sigma_sched" in params:
            extra["sigma_sched"] = sigmas
        if "sigmas" in params:
            extra["sigmas"] = sigmas
        if sampler_opt.get("brownian_noise", False):
            extra["noise_sampler"] = self.create_noise_sampler(latents, sigmas, steps, seed)
        if sampler_opt.get("solver_type", None) == "heun":
            extra["solver_type"] = "heun"
        return extra

    # ---- image-side helpers of img2img / inpainting
    def preprocess(self, image):
        """reference :458-481 (`[-1, 1]` NCHW float tensor; PIL images are resized down to a multiple of 8, lanczos)"""
        if isinstance(image, torch.Tensor):
            return image
        import numpy as np
        import PIL.Image
        if isinstance(image, PIL.Image.Image):
            image = [image]
        if isinstance(image[0], PIL.Image.Image):
            w, h = image[0].size
            w, h = (v - v % 8 for v in (w, h))
            arr = np.concatenate([np.array(i.convert("RGB").resize((w, h), resample=PIL.Image.LANCZOS))[None] for i in image])
            return torch.from_numpy(2.0 * (arr.astype(np.float32) / 255.0).transpose(0, 3, 1, 2) - 1.0)
        return torch.cat(list(image), dim=0)

    def _image_tensor(self, image, height, width, mask=False):
        """What the reference's VaeImageProcessor.preprocess calls (:1447-1449, :1480-1482) amount to for tensors, numpy
        arrays and PIL images: NCHW float32 at (height, width); images in [-1, 1], masks one channel binarised at 0.5"""
        import numpy as np
        if not isinstance(image, torch.Tensor):
            import PIL.Image
            if isinstance(image, PIL.Image.Image):
                image = image.convert("L" if mask else "RGB").resize((width, height), resample=PIL.Image.LANCZOS)
                image = np.array(image).astype(np.float32) / 255.0
            arr = np.asarray(image, dtype=np.float32)             # numpy: HW, HWC or NCHW, values in [0, 1]
            image = torch.from_numpy(arr)
            if arr.ndim == 2:
                image = image[None, None]
            elif arr.ndim == 3:
                image = image.permute(2, 0, 1)[None]
            if not mask:
                image = 2.0 * image - 1.0
        image = image.float()
        if image.ndim == 3:
            image = image[None]
        if mask:
            if image.shape[1] != 1:
                image = image.mean(dim=1, keepdim=True)
            image = (image >= 0.5).float()
        if tuple(image.shape[-2:]) != (height, width):
            image = torch.nn.functional.interpolate(image, size=(height, width), mode="nearest" if mask else "bilinear")
        return image

    def _encode_vae_image(self, image, generator):
        """reference :1234-1246: sample the posterior, times the scaling factor"""
        if self.vae is None or not hasattr(self.vae, "encode"):
            raise NotImplementedError("img2img / inpainting from pixels needs a VAE with an encoder "
                                      "(modules.vae_decoder.AutoencoderKL); pass 4-channel latents instead")
        image = image.to(self.vae.device, dtype=self.vae.dtype)
        return self.vae.config.scaling_factor * self.vae.encode(image).latent_dist.sample(generator)

    def _encode_text_rows(self, prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, text_input_ids,
                          num_images_per_prompt, clip_skip, long_encode, device):
        """(text rows [u.., c..] in the UNet dtype, token ids, number of images) - reference :1006-1023"""
        cfg = self.do_classifier_free_guidance
        if prompt_embeds is None:
            if prompt is None or self.tokenizer is None or self.text_encoder is None:
                raise NotImplementedError("pass prompt_embeds / negative_prompt_embeds / text_input_ids, or construct the "
                                          "pipeline with a tokenizer and a CLIP text encoder and pass `prompt`")
            from .encoder_prompt_modify import encode_prompt_function
            prompt_embeds, negative_prompt_embeds, text_input_ids = encode_prompt_function(
                self, prompt, device, 1, cfg, negative_prompt, clip_skip=clip_skip, long_encode=long_encode)
        n_img = prompt_embeds.shape[0] * num_images_per_prompt
        text = prompt_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        if cfg:
            if negative_prompt_embeds is None:
                raise ValueError("classifier-free guidance needs negative_prompt_embeds")
            text = torch.cat([negative_prompt_embeds.repeat_interleave(num_images_per_prompt, dim=0), text])
        if text_input_ids is None:
            text_input_ids = [None, None]
        return text.to(device=device, dtype=self.unet.dtype), text_input_ids, n_img

    @staticmethod
    def _randn_like_ref(shape, generator, device, dtype):
        """diffusers randn_tensor: drawn on the generator's device, moved to `device`"""
        gdev = generator.device if generator is not None else device
        return torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)

    def _hires_pass(self, latents, height, width, upscale_x, upscale_method, upscale_antialias, **img2img_kwargs):
        """reference :1176-1228 (txt2img), :789-838 (img2img), :1705-1757 (inpaiting): interpolate the final latents by
        `upscale_x` and run img2img on them at `upscale_denoising_strength`"""
        f = self.vae_scale_factor
        target_height = int(height * upscale_x // f) * 8
        target_width = int(width * upscale_x // f) * 8
        latents = torch.nn.functional.interpolate(latents.float(), size=(int(target_height // f), int(target_width // f)),
                                                  mode=upscale_method,
                                                  **({"antialias": upscale_antialias} if upscale_method in ("bilinear", "bicubic") else {})
                                                  ).to(latents.dtype)
        return self.img2img(latents=latents, width=int(target_width), height=int(target_height), **img2img_kwargs)

    @torch.no_grad()
    def img2img(self, prompt=None, num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None,
                generator: Optional[torch.Generator] = None, image=None, output_type: Optional[str] = "pil", latents=None,
                strength=1.0, region_map_state=None, sampler_name="", sampler_opt={}, start_time=-1, timeout=180,
                scale_ratio=8.0, latent_processing=0, weight_func=lambda w, sigma, qk: w * sigma * qk.std(), upscale=False,
                upscale_x: float = 2.0, upscale_method: str = "bicubic", upscale_antialias: bool = False,
                upscale_denoising_strength: float = 0.7, sampler_name_hires="", sampler_opt_hires={},
                width=None, height=None, seed=0, ip_adapter_image=None, control_img=None,
                controlnet_conditioning_scale=None, control_guidance_start=None, control_guidance_end=None,
                image_t2i_adapter=None, adapter_conditioning_scale=1.0, adapter_conditioning_factor: float = 1.0,
                guidance_rescale: float = 0.0, cross_attention_kwargs=None, clip_skip=None, long_encode=0,
                num_images_per_prompt=1, ip_adapter_image_embeds=None,
                prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                text_input_ids=None, fused: Optional[bool] = None, step_noise: Optional[torch.Tensor] = None,
                two_call: bool = False, **unsupported):
        """reference :543-846: encode the image (or take `latents`), keep the last `strength` fraction of the schedule, add
        noise, denoise.  Reproduces the reference's start: `latents + noise * sqrt(sigma_0^2 + 1)` (:647 - sic, not
        `noise * sigma_0`).  Generator draws: the VAE posterior sample, then the noise; the image is encoded before the prompt."""
        a = dict(locals())                       # this call's arguments by name, as given: what the shared path reads
        if image is not None:
            image = self.preprocess(image)
            latents = self._encode_vae_image(image, generator)                                       # :600-606
        if latents is None:
            raise ValueError("img2img needs `image` or `latents`")
        if height is None:
            height = int(latents.shape[-2]) * 8
        if width is None:
            width = int(latents.shape[-1]) * 8
        device = self._execution_device
        latents = latents.to(device, dtype=self.unet.dtype)
        sampler, text, text_input_ids, n_img, sigmas = self._text_and_schedule(a)
        if latents.shape[0] != n_img:
            latents = latents.repeat(n_img // latents.shape[0], 1, 1, 1)
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)                # :637-638
        sigma_sched = sigmas[max(num_inference_steps - init_timestep, 0):]
        noise = self._randn_like_ref(latents.shape, generator, device, text.dtype)
        latents = latents + noise * (sigma_sched[0] ** 2 + 1) ** 0.5                                 # :647
        cond = self._conditioning(a, text, text_input_ids, n_img, sigma_sched, width, height, len(sigma_sched))
        return self._denoise_and_finish(a, sampler, latents, sigma_sched, text, n_img, cond, height, width, len(sigma_sched), None,
                                        fused_by_default=True)

    def _sigma_to_alpha_sigma_t(self, sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)                                                      # :1293-1297
        return alpha_t, sigma * alpha_t

    def add_noise(self, init_latents_proper, noise, sigma):
        if isinstance(sigma, torch.Tensor) and sigma.numel() > 1:                                    # :1299-1304
            sigma = sigma.sort(descending=True)[0][0].item()
        return init_latents_proper + sigma * noise

    def prepare_latents_inpating(self, batch_size, num_channels_latents, height, width, dtype, device, generator,
                                 latents=None, image=None, sigma=None, is_strength_max=True, return_noise=False,
                                 return_image_latents=False):
        """reference :1306-1362 (same spelling)"""
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if (image is None or sigma is None) and not is_strength_max:
            raise ValueError("Since strength < 1. initial latents are to be initialised as a combination of Image + Noise."
                             "However, either the image or the noise sigma has not been provided.")
        image_latents = None
        if return_image_latents or (latents is None and not is_strength_max):
            image = image.to(device=device, dtype=dtype)
            image_latents = image if image.shape[1] == 4 else self._encode_vae_image(image, generator).to(device, dtype)
            image_latents = image_latents.repeat(batch_size // image_latents.shape[0], 1, 1, 1)
        if latents is None:
            noise = self._randn_like_ref(shape, generator, device, dtype)
            latents = noise if is_strength_max else self.add_noise(image_latents, noise, sigma)
            latents = latents * (sigma.item() ** 2 + 1) ** 0.5 if is_strength_max else latents
        else:
            noise = latents.to(device)
            latents = noise * (sigma.item() ** 2 + 1) ** 0.5
        out = (latents,)
        if return_noise:
            out += (noise,)
        if return_image_latents:
            out += (image_latents,)
        return out

    @torch.no_grad()
    def inpaiting(self, prompt=None, height: int = 512, width: int = 512, num_inference_steps: int = 50,
                  guidance_scale: float = 7.5, negative_prompt=None, eta: float = 0.0,
                  generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None,
                  output_type: Optional[str] = "pil", callback_steps: Optional[int] = 1, upscale=False,
                  region_map_state=None, sampler_name="", sampler_opt={}, start_time=-1, timeout=180,
                  latent_processing=0, weight_func=lambda w, sigma, qk: w * sigma * qk.std(), seed=0,
                  ip_adapter_image=None, control_img=None, controlnet_conditioning_scale=None, control_guidance_start=None,
                  control_guidance_end=None, image_t2i_adapter=None, adapter_conditioning_scale=1.0,
                  adapter_conditioning_factor: float = 1.0, image=None, mask_image=None,
                  masked_image_latents=None, padding_mask_crop=None, strength: float = 1.0, guidance_rescale: float = 0.0,
                  cross_attention_kwargs=None, clip_skip=None, long_encode=0, num_images_per_prompt=1,
                  ip_adapter_image_embeds=None,
                  prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                  text_input_ids=None, fused: Optional[bool] = None, step_noise: Optional[torch.Tensor] = None, **unsupported):
        """reference :1365-1760 (method name as spelled there).  4-channel UNet: the known region `image_latents + sigma * noise` is
        re-imposed on the model input before every model call after the first (:1599-1612).  9-channel UNet (the inpainting
        checkpoints): mask and masked-image latents are concatenated to the duplicated latent (:1617-1619) - eager protocol mode,
        or with fused=True the captured 9-channel step and one dsc_cfg_linear_step_rows_cat launch per step (_denoise_fused with
        `extra`: every sampler of sampling.LINEAR_FAMILY, v-prediction, guidance_rescale; step_noise as in img2img).  Generator
        draws: everything inside prepare_latents_inpating, then the masked-image encode."""
        a = dict(locals())                       # this call's arguments by name, as given: what the shared path reads
        if upscale or padding_mask_crop is not None:             # (the refusals come before anything else)
            raise NotImplementedError("hires upscale after inpainting and mask cropping are outside the denoising hot path "
                                      "built here")
        num_channels_unet = self.unet.config.in_channels
        if num_channels_unet not in (4, 9):
            raise ValueError(f"The unet {self.unet.__class__} should have either 4 or 9 input channels, not {num_channels_unet}.")
        if image is None or mask_image is None:
            raise ValueError("inpaiting needs `image` and `mask_image`")
        device = self._execution_device
        sampler, text, text_input_ids, n_img, sigmas = self._text_and_schedule(a)
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)                # :1432-1438
        sigmas = sigmas[max(num_inference_steps - init_timestep, 0):] if 0 <= strength < 1.0 else sigmas
        is_strength_max = strength == 1.0
        init_image = self._image_tensor(image, height, width) if not (isinstance(image, torch.Tensor) and image.shape[1] == 4) \
            else image.float()
        latents, noise_inp, image_latents = self.prepare_latents_inpating(
            n_img, 4, height, width, text.dtype, device, generator, latents, image=init_image, sigma=sigmas[0],
            is_strength_max=is_strength_max, return_noise=True, return_image_latents=True)           # :1459-1478
        mask = self._image_tensor(mask_image, height, width, mask=True)
        extra_input = None
        if num_channels_unet == 9:                               # :1253-1290, :1617-1619: [latents | mask | masked-image latents]
            if masked_image_latents is None:
                if init_image.shape[1] == 4:
                    raise ValueError("the 9-channel UNet needs pixels (or masked_image_latents) to build the masked image")
                masked = init_image * (mask < 0.5)
                masked_image_latents = self._encode_vae_image(masked, generator)
            mil = masked_image_latents.to(device=device, dtype=text.dtype)
            if mil.shape[0] < n_img:
                mil = mil.repeat(n_img // mil.shape[0], 1, 1, 1)
        mask = torch.nn.functional.interpolate(mask, size=(height // self.vae_scale_factor, width // self.vae_scale_factor))
        mask = mask.to(device=device, dtype=text.dtype)                                              # :1253-1257
        if mask.shape[0] < n_img:
            mask = mask.repeat(n_img // mask.shape[0], 1, 1, 1)
        if num_channels_unet == 9:
            rows = 2 if self.do_classifier_free_guidance else 1
            extra_input = torch.cat([torch.cat([mask] * rows), torch.cat([mil] * rows)], dim=1)
        sig_last = float(sigmas[-1])

        def keep_known_region(x, sigma, call_index):                                                 # :1599-1612
            if call_index == 0 or num_channels_unet != 4:
                return x
            s = float(sigma[0])
            known = image_latents
            if s > sig_last:
                alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(s)
                known = alpha_t * image_latents + sigma_t * noise_inp
            rate = (s ** 2 + 1) ** 0.5
            return ((1 - mask) * known + mask * x / rate) * rate

        cond = self._conditioning(a, text, text_input_ids, n_img, sigmas, width, height, num_inference_steps)
        fused_kw = None
        if fused:
            if num_channels_unet != 9:
                raise NotImplementedError("inpaiting(fused=True) runs the 9-channel inpainting UNets; the known-region blend of a "
                                          "4-channel UNet has no fused loop: run it with fused=False")
            if latents.shape[-2] * latents.shape[-1] % 8 != 0:
                raise NotImplementedError(f"inpaiting(fused=True): the 9-channel input row must stay 16-byte aligned, which needs a "
                                          f"latent of h * w % 8 == 0, got {list(latents.shape[-2:])}; run it with fused=False")
            fused_kw = {"extra": torch.cat([mask, mil], dim=1)}
        return self._denoise_and_finish(a, sampler, latents, sigmas, text, n_img, cond, height, width, num_inference_steps, eta,
                                        fused_by_default=False, fused_kw=fused_kw,
                                        protocol_kw={"input_hook": keep_known_region, "extra_input": extra_input})

    # ------------------------------------------------------------------ the generation path the three entries share
    # Each entry keeps what is its own - its refusals, how the start latent is made (and with it the order of the generator's
    # draws) and the strength cut of the schedule - and runs the rest here, in the reference's order:
    #   _text_and_schedule -> [the entry's latents] -> _conditioning -> _denoise_and_finish.
    # Where the entries differ on purpose (they mirror the reference), the difference is a parameter of these three methods and
    # is written down at that parameter.  `a` is the entry's own `dict(locals())`, taken before it changes anything: the
    # arguments as the caller gave them, by name.
    def _text_and_schedule(self, a):
        """-> (sampler, text rows, token ids, number of images, schedule).  Sets `_do_classifier_free_guidance` first: the text
        rows, the region tables and the hooks read it when they are built.  The prompt is encoded here, i.e. before every
        generator draw of txt2img and inpaiting and after img2img's image encode (:600-606)."""
        sampler = self.get_scheduler(a["sampler_name"]) if isinstance(a["sampler_name"], str) else a["sampler_name"]
        device = self._execution_device
        self._do_classifier_free_guidance = a["guidance_scale"] > 1.0
        text, text_input_ids, n_img = self._encode_text_rows(
            a["prompt"], a["negative_prompt"], a["prompt_embeds"], a["negative_prompt_embeds"], a["text_input_ids"],
            a["num_images_per_prompt"], a["clip_skip"], a["long_encode"], device)
        # sigmas are cast to the model dtype on the device (:1027-1029): fp16 rounding is part of the schedule
        return sampler, text, text_input_ids, n_img, self._schedule(a["num_inference_steps"], a["sampler_opt"], device, text.dtype)

    def _conditioning(self, a, text, text_input_ids, n_img, sigmas, width, height, steps):
        """-> (region_state, cross_attention_kwargs, control_hook): the region tables (:1050), the IP-Adapter embeds in
        `self._added_cond_kwargs` (:1069-1082; reset on every call) and the ControlNet / T2I-Adapter hooks, merged.
        sigmas: the schedule the entry will run, i.e. after img2img's and inpaiting's strength cut.  The T2I-Adapter hook counts
        its steps as len(sigmas) in every entry (:1086-1089, :700-703, :1588-1591).
        steps: what the ControlNet hook spreads its guidance window over - `num_inference_steps` in txt2img (:1060-1061) and
        inpaiting (:1577-1578), cut or not; len(sigmas) in img2img (:675-676)."""
        device, n_per = self._execution_device, a["num_images_per_prompt"]
        region_state = encode_region_map(self, a["region_map_state"], width=width, height=height, num_images_per_prompt=n_per,
                                         text_ids=text_input_ids)
        self._added_cond_kwargs = None
        if a["ip_adapter_image"] is not None or a["ip_adapter_image_embeds"] is not None:
            embeds = self.prepare_ip_adapter_image_embeds(a["ip_adapter_image"], a["ip_adapter_image_embeds"], device, n_per,
                                                          self.do_classifier_free_guidance)
            self._added_cond_kwargs = {"image_embeds": [e.to(device=device, dtype=text.dtype) for e in embeds]}
        control_hook = self._merge_hooks(
            self._controlnet_hook(a["control_img"], a["controlnet_conditioning_scale"], a["control_guidance_start"],
                                  a["control_guidance_end"], width, height, steps, n_img, n_per, text),
            self._adapter_hook(a["image_t2i_adapter"], a["adapter_conditioning_scale"], a["adapter_conditioning_factor"], width,
                               height, len(sigmas), n_per))
        return region_state, {} if a["cross_attention_kwargs"] is None else a["cross_attention_kwargs"], control_hook

    def _denoise_and_finish(self, a, sampler, latents, sigmas, text, n_img, cond, height, width, steps, eta, fused_by_default,
                            protocol_kw=None, fused_kw=None):
        """Choose the core, run it, and return what the entry returns.
        steps, eta: what the sampler's arguments are built from.  txt2img and inpaiting: `num_inference_steps` and the caller's
        eta, in both modes (protocol mode leaves the arguments to _denoise_protocol: get_sampler_extra_args_t2i).  img2img: len(sigmas)
        and eta None - the fused loop then keeps the sampler's own default, and protocol mode gets the arguments of
        get_sampler_extra_args_i2i (:916-941), which takes no eta (the core is handed 0.0).
        fused_by_default: what `fused=None` means.  True (txt2img, img2img): the fused loop where it is the cheaper equal - DPM++ 2M,
        guidance on and not rescaled, eps-prediction, no hook, no previews.  False (inpaiting): protocol mode.
        protocol_kw / fused_kw: what only this entry hands the cores - txt2img its `slot` (to both), inpaiting `input_hook` and
        `extra_input` (protocol) or `extra` (fused)."""
        region_state, cross_attention_kwargs, control_hook = cond
        output_type, sampler_opt, seed, step_noise = a["output_type"], a["sampler_opt"], a["seed"], a["step_noise"]
        guidance_scale, guidance_rescale, weight_func = a["guidance_scale"], a["guidance_rescale"], a["weight_func"]
        latent_processing, preview = a["latent_processing"], None
        if latent_processing == 1:                               # :1083-1084, :696-697, :1584-1585: previews of every model call's estimate
            latents_process = [self.latent_to_image(latents, output_type)]
            preview = (latents_process, output_type)
        fused = a["fused"]
        if fused is None:
            fused = fused_by_default and sampler is sampling.sample_dpmpp_2m and guidance_rescale == 0.0 \
                and self.do_classifier_free_guidance and not self.v_prediction and control_hook is None and preview is None
        if fused:
            if control_hook is not None or preview is not None:
                raise NotImplementedError("ControlNet / T2I-Adapter / latent previews run in protocol mode (fused=False)")
            latents = self._denoise_fused(latents, sigmas, text, region_state, weight_func, guidance_scale, n_img,
                                          cross_attention_kwargs, a["start_time"], a["timeout"], sampler=sampler,
                                          sampler_args=self._fused_sampler_args(sampler, sigmas, eta, steps, sampler_opt, latents,
                                                                                seed, step_noise),
                                          step_noise=step_noise, guidance_rescale=guidance_rescale,
                                          **({"two_call": True} if a.get("two_call") else {}), **(fused_kw or {}))
        else:
            protocol_kw = dict(protocol_kw or {})
            if eta is None:
                protocol_kw["sampler_args"] = self.get_sampler_extra_args_i2i(sigmas, steps, sampler_opt, latents, seed, sampler)
            latents = self._denoise_protocol(sampler, latents, sigmas, text, region_state, weight_func, guidance_scale,
                                             guidance_rescale, n_img, cross_attention_kwargs, 0.0 if eta is None else eta, steps,
                                             sampler_opt, seed, a["start_time"], a["timeout"], control_hook=control_hook,
                                             preview=preview, **protocol_kw)
        if a["upscale"]:                                         # :1176-1228, :789-838 (inpaiting refuses it on entry)
            hires = dict(strength=a["upscale_denoising_strength"], sampler_name=a["sampler_name_hires"] or a["sampler_name"],
                         sampler_opt=a["sampler_opt_hires"] or sampler_opt,
                         latent_processing=a["unsupported"].get("latent_upscale_processing", False),
                         **{k: a[k] for k in self._HIRES_SAME})
            res = self._hires_pass(latents, height, width, a["upscale_x"], a["upscale_method"], a["upscale_antialias"], **hires)
            return latents_process + res if preview is not None else res
        if preview is not None:                                  # :1229-1230, :841-842, :1759-1760 (the list ends with the last model call's estimate)
            return latents_process
        return [self.latent_to_image(latents, output_type)]

    # what the hires pass (img2img on the enlarged latents) is given unchanged, as the caller gave it
    _HIRES_SAME = ("prompt", "num_inference_steps", "guidance_scale", "negative_prompt", "generator", "region_map_state", "seed",
                   "control_img", "controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end",
                   "image_t2i_adapter", "adapter_conditioning_scale", "adapter_conditioning_factor", "guidance_rescale",
                   "cross_attention_kwargs", "clip_skip", "long_encode", "num_images_per_prompt", "weight_func",
                   "ip_adapter_image_embeds", "prompt_embeds", "negative_prompt_embeds", "text_input_ids", "output_type",
                   "start_time", "timeout")

    # ---- what the two cores share
    @staticmethod
    def _check_timeout(start_time, timeout):
        """before every model call and every fused step (reference :1094-1095, :707-708, :1596-1597)"""
        if start_time > 0 and timeout > 0:
            assert (time.time() - start_time) < timeout, "inference process timed out"

    def _step_key(self, slot, n_img, in_shape, region_state, text, weight_func, ip_key):
        """the key of a captured step: shapes only (and what the capture bakes in), see _build_or_refresh_step"""
        levels = tuple(sorted((int(L), tuple(w.shape)) for L, w in region_state.items())) \
            if isinstance(region_state, dict) else None
        # ("freeu", on): whether the capture holds the UNet's FreeU launches (unet.enable_freeu) - the VALUES are data the launches
        # read from the UNet's persistent table, so changing them keeps the capture; enabling builds a second one beside the
        # plain step's, and disabling finds the plain one again (_build_or_refresh_step keeps one of each per slot)
        freeu = ("freeu", getattr(self.unet, "freeu_setting", lambda: None)() is not None)
        return (("slot", slot), n_img, in_shape, levels, tuple(text.shape), text.dtype, self._weight_func_key(weight_func), ip_key,
                freeu)

    @staticmethod
    def _record_done(st, device):
        """the event a later generation on the same static buffers waits for (_build_or_refresh_step)"""
        done = st.get("done")
        if done is None:
            done = st["done"] = torch.cuda.Event()
        done.record(torch.cuda.current_stream(device))

    # ---- protocol mode: the reference's model_fn closure (:1091-1171) + sampler call (:1172-1175)
    def _denoise_protocol(self, sampler, latents, sigmas, text, region_state, weight_func, guidance_scale,
                          guidance_rescale, n_img, cross_attention_kwargs, eta, steps, sampler_opt, seed, start_time,
                          timeout, sampler_args=None, input_hook=None, control_hook=None, extra_input=None, preview=None,
                          slot=0):
        """sampler_args: the keyword arguments for `sampler` when the caller built them itself (img2img's
        get_sampler_extra_args_i2i); input_hook(x, sigma, call_index) -> x: applied to the model input (inpainting's
        re-imposition of the known region, reference :1599-1612); extra_input [rows, c, h, w]: channels concatenated to the
        duplicated latent before the denoiser (the 9-channel inpainting UNet's mask + masked-image latents, :1617-1619 - the
        denoiser's c_in then scales them too, as in the reference); preview = (list, output_type): every model call appends the
        image of its denoised estimate (`latent_processing == 1`, :1169-1170)"""
        cfg = self.do_classifier_free_guidance
        kdm = self.k_diffusion_model
        calls = [0]

        def enter(x, sigma):
            """how both model_fn below begin: the timeout, the caller's input_hook, the call counter -> the model input"""
            self._check_timeout(start_time, timeout)
            if input_hook is not None:
                x = input_hook(x, sigma, calls[0])
            calls[0] += 1
            return x

        def sample(model_fn):
            extra = sampler_args if sampler_args is not None else \
                self.get_sampler_extra_args_t2i(sigmas, eta, steps, sampler_opt, latents, seed, sampler)
            return sampler(model_fn, latents, **extra)

        # Graph-backed model calls: when nothing has to enter the UNet per call besides (x, sigma) - no ControlNet / adapter
        # residuals, eps-prediction, CFG without rescale, fp16 - the sampler's model call is: one launch that writes the
        # static inputs, ONE replay of the captured UNet step (the fused mode's graph), one launch for CFG + eps -> denoised.
        # Every sampler then runs at graph speed; only its own update arithmetic stays eager.
        control = None if control_hook is None else getattr(control_hook, "static", None)
        use_graph = (ops.PROTOCOL_GRAPH and (control_hook is None or control is not None) and cfg and guidance_rescale == 0.0
                     and not self.v_prediction and latents.is_cuda and text.dtype == torch.float16 and extra_input is None
                     and self._added_cond_kwargs is None and latents.numel() // latents.shape[0] % 4 == 0)
        if use_graph:
            ckey = None if control is None else tuple(
                ("cn", id(self.controlnet), tuple(tuple(i.shape) for i in (p["image"] if isinstance(p["image"], list) else [p["image"]])))
                if p["kind"] == "controlnet" else ("ad", tuple(tuple(v.shape) for v in p["state"])) for p in control)
            key = self._step_key(slot, n_img, tuple(latents.shape), region_state, text, weight_func, None) \
                + (() if ckey is None else (ckey,))
            _lib.check(_lib.load_library().dsc_set_workspace_slot(slot), "dsc_set_workspace_slot")    # see _denoise_fused
            st = self._static_step(key, n_img, tuple(latents.shape), text, region_state, weight_func, cross_attention_kwargs,
                                   control=control)
            scratch = torch.zeros_like(latents, dtype=text.dtype)

            def set_control(s):
                for part in control or []:
                    v = part["schedule"](s)
                    if part["kind"] == "controlnet":
                        for buf, val in zip(st["cn"]["scale"], v if isinstance(v, list) else [v]):
                            buf.fill_(float(val))
                    else:
                        st["ad"]["gate"].fill_(1.0 if v else 0.0)

            def model_fn(x, sigma):
                x = enter(x, sigma)
                s = float(sigma[0])                              # the host needs sigma for (c_in, t): one sync per model call
                c_in, _, t = kdm.step_scalars(s)
                d = x.to(text.dtype).contiguous().clone()
                row = None
                if st["tadd"] is not None:                       # any sigma may be asked for: this call's embedding rows, now
                    row = (self.unet.temb_add_table(torch.tensor([t], dtype=torch.float32, device=d.device))[0], st["tadd"])
                ops.prepare_unet_input(d, c_in, t, s, st["x_in"], st["t"], st["sigma"], row=row)
                set_control(s)
                st["run"]()
                # a = 0, b = 1, c = 0: d <- D = x - sigma (eps_u + g (eps_c - eps_u)); the "next input" it also writes is unused
                ops.cfg_dpmpp2m_step(d, st["eps"], scratch, s, guidance_scale, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0,
                                     st["x_in"], st["t"], st["sigma"])
                if preview is not None:
                    preview[0].append(self.latent_to_image(d, preview[1]))
                return d.to(x.dtype)

            out = sample(model_fn)
            self._record_done(st, latents.device)
            return out
        if slot:
            raise NotImplementedError("generation slots need the graph-backed model call (eps-prediction, CFG without rescale, "
                                      "fp16, no per-call UNet inputs)")

        def model_fn(x, sigma):
            x = enter(x, sigma)
            latent_model_input = torch.cat([x] * 2) if cfg else x
            if extra_input is not None:
                latent_model_input = torch.cat([latent_model_input, extra_input.to(latent_model_input.dtype)], dim=1)
            cross_attention_kwargs["region_prompt"] = {
                "region_state": region_state, "sigma": sigma[0], "weight_func": weight_func, "n_std_groups": n_img}
            if latent_model_input.dtype != text.dtype:
                latent_model_input = latent_model_input.to(text.dtype)
            # CompVisDenoiser.forward broadcasts sigma[B] against 2B rows (external_k_diffusion.py:109-114), which
            # only works for B == 1 in the reference; repeat sigma per row so that B > 1 works too
            sig_rows = torch.cat([sigma] * 2) if cfg else sigma
            extra_kw = {} if self._added_cond_kwargs is None else {"added_cond_kwargs": self._added_cond_kwargs}
            if control_hook is not None:
                extra_kw.update(control_hook(latent_model_input, sig_rows))
            noise_pred = kdm(latent_model_input, sig_rows, cond=text, cross_attention_kwargs=cross_attention_kwargs,
                             **extra_kw)
            if cfg:
                u, c = noise_pred.chunk(2)
                noise_pred = u + guidance_scale * (c - u)
                if guidance_rescale > 0.0:
                    noise_pred = rescale_noise_cfg(noise_pred, c, guidance_rescale=guidance_rescale)
            if preview is not None:
                preview[0].append(self.latent_to_image(noise_pred, preview[1]))
            return noise_pred

        return sample(model_fn)

    # ---- fused mode
    def _control_buffers(self, control, st=None):
        """Static buffers of the ControlNet / T2I-Adapter parts of a captured step (control = the hooks' static
        descriptions): conditioning embeddings computed ONCE per generation, per-call scales / gates as 0-dim device tensors
        the model call fills before each replay.  With `st` given the existing buffers are refreshed in place."""
        from .controlnet import MultiControlNetModel
        out = {"cn": None, "ad": None} if st is None else st
        for part in control or []:
            if part["kind"] == "controlnet":
                multi = isinstance(self.controlnet, MultiControlNetModel)
                nets = list(self.controlnet.nets) if multi else [self.controlnet]
                imgs = part["image"] if multi else [part["image"]]
                embs = [n.conditioning_embedding(im) for n, im in zip(nets, imgs)]
                if st is None:
                    dev, dt = embs[0].device, embs[0].dtype
                    out["cn"] = {"emb": [e.clone() for e in embs], "img": [im.clone() for im in imgs], "multi": multi,
                                 "scale": [torch.zeros((), device=dev, dtype=dt) for _ in nets]}
                else:
                    for dst, src in zip(st["cn"]["emb"], embs):
                        dst.copy_(src)
            else:
                if st is None:
                    out["ad"] = {"state": [v.clone() for v in part["state"]],
                                 "gate": torch.zeros((), device=part["state"][0].device, dtype=part["state"][0].dtype)}
                else:
                    for dst, src in zip(st["ad"]["state"], part["state"]):
                        dst.copy_(src)
        return out

    def _static_step(self, key, *args, **kwargs):
        """_build_or_refresh_step, with first-time creation (warm-up launches + stream capture) serialised across host
        threads: a capture must not overlap another thread's allocations.  Generation slots should still be created one
        after the other before they run concurrently - a running slot's thread allocates too."""
        if key in self._graphs:
            return self._build_or_refresh_step(key, *args, **kwargs)
        with _CAPTURE_LOCK:
            return self._build_or_refresh_step(key, *args, **kwargs)

    def _build_or_refresh_step(self, key, n_img, lat_shape, text, region_state, weight_func, cross_attention_kwargs, control=None,
                               n_std_groups=None):
        """Static buffers + the captured UNet step.  The graph is keyed by SHAPES only: a new generation with other
        text / other region masks updates the static buffers in place (text, its packed K/V, the compressed region
        tables) and replays the same graph."""
        st = self._graphs.get(key)
        comp_cpu = self._compress_tables(region_state)
        ack = self._added_cond_kwargs
        # Which tables does the captured step READ?  The prepared-operand kernels read the compressed (ids, rows) buffers;
        # every other route (a table with more than 32 distinct rows, a custom weight_func, prompts beyond the chunked
        # kernels) reads the DENSE table - so the graph must be given a static device copy that each generation refreshes in
        # place, never the first generation's own tensors (a later generation with the same shapes would replay old masks).
        need_dense = isinstance(region_state, dict) and bool(region_state) and (
            comp_cpu is None or self._weight_func_key(weight_func) != "default" or text.shape[1] > ops.XATTN_MAX_KEYS_PACKED
            or not self._all_cross_attention_packable())         # (beyond the chunked prepared-operand kernels)
        if (st is not None and (st["compressed"] is None) == (comp_cpu is None)
                and (st["dense"] is None) == (not need_dense) and st["profile"] == ops.tuning_profile()):
            done = st.get("done")
            if done is not None:         # the slot's buffers may last have been driven from another stream
                torch.cuda.current_stream(text.device).wait_event(done)
            if ack is not None:
                for dst, src in zip(st["image_embeds"], ack["image_embeds"]):
                    dst.copy_(src)
            st["text"].copy_(text)
            self._refresh_text_kv(st["text"])
            self._upload_tables(st, comp_cpu, region_state)
            self._control_buffers(control, st)
            return st
        dev, dt = text.device, text.dtype
        rows = 2 * n_img
        st = {
            "x_in": torch.zeros((rows,) + lat_shape[1:], device=dev, dtype=dt),
            "t": torch.zeros(rows, device=dev, dtype=torch.float32),
            # the captured step reads element 0 (a lockstep batch has one sigma); the per-row sampler step
            # (ops.cfg_linear_step_rows) writes every image's own entry of the same buffer
            "sigma_rows": torch.ones(n_img, device=dev, dtype=torch.float32),
            "text": text.clone(),
            "compressed": None, "dense": None,
            "weight_func": weight_func,          # kept alive: the key holds its id
            "profile": ops.tuning_profile(),     # the launch rules baked into the capture (ops.set_tuning_profile)
            # the time-embedding projections of all ResNet blocks for the step about to run: written by the sampler kernels
            # (a row of the per-schedule table, _denoise_fused) instead of being recomputed by three launches inside every step
            "tadd": (torch.zeros((rows, self.unet.temb_width()), device=dev, dtype=dt)
                     if ops.USE_TEMB_HOIST and hasattr(self.unet, "temb_add_table") and dt == torch.float16 else None),
            "temb_tab": None, "temb_key": None,
            "image_embeds": None if ack is None else [e.clone() for e in ack["image_embeds"]],
        }
        st["sigma"] = st["sigma_rows"][:1]
        if comp_cpu is not None:
            st["compressed"] = {L: (ids.to(dev), rws.to(dev)) for L, (ids, rws) in comp_cpu.items()}
        if need_dense:
            st["dense"] = {L: w.to(device=dev, dtype=torch.float32).contiguous().clone() for L, w in region_state.items()}
        st.update(self._control_buffers(control))
        self._refresh_text_kv(st["text"])
        kw = dict(cross_attention_kwargs)
        # without a dense copy the dict only supplies the level keys / shapes: no kernel of the captured step reads it
        # "compressed": False = the tables are static buffers refreshed in place: the processors must read them densely and
        # must not derive (and bake into the capture) a compressed form from the values they hold during the capture
        kw["region_prompt"] = {"region_state": st["dense"] if need_dense else region_state,
                               "compressed": st["compressed"] if st["compressed"] is not None else (False if need_dense else None),
                               "sigma": st["sigma"], "weight_func": weight_func,
                               "n_std_groups": n_img if n_std_groups is None else n_std_groups}

        ukw = {} if ack is None else {"added_cond_kwargs": {"image_embeds": st["image_embeds"]}}

        def step():
            extra = dict(ukw)
            if st["cn"] is not None:                # ControlNet on the same scaled input and timestep as the UNet (:1134-1142)
                cn = st["cn"]
                one = not cn["multi"]
                down, mid = self.controlnet(st["x_in"], st["t"], encoder_hidden_states=st["text"],
                                            controlnet_cond=cn["img"][0] if one else cn["img"],
                                            conditioning_scale=cn["scale"][0] if one else cn["scale"], guess_mode=False,
                                            return_dict=False, cond_embedding=cn["emb"][0] if one else cn["emb"])
                extra.update({"down_block_additional_residuals": down, "mid_block_additional_residual": mid})
            if st["ad"] is not None:                # T2I-Adapter features, gated per call (0 = the reference passes none)
                extra["down_intrablock_additional_residuals"] = [v * st["ad"]["gate"] for v in st["ad"]["state"]]
            if st["tadd"] is not None:
                extra["temb_adds"] = st["tadd"]
            if ops.USE_CFG_SHARED_PREFIX and st["cn"] is None and st["ad"] is None and hasattr(self.unet, "temb_add_table"):
                extra["cfg_shared_prefix"] = True    # x_in = [x; x] (ops.prepare_unet_input / cfg_dpmpp2m_step), one timestep
            return self.unet(st["x_in"], st["t"], encoder_hidden_states=st["text"], cross_attention_kwargs=kw, **extra).sample

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):                   # warm-up: workspaces, MIOpen / hipBLASLt kernel selection
                st["eps"] = step()
        torch.cuda.current_stream(dev).wait_stream(side)
        if not ops.GRAPHS_ENABLED:
            st["run"] = lambda: st.__setitem__("eps", step())
        else:
            g = torch.cuda.CUDAGraph()
            with _capture_without_gc(), torch.cuda.graph(g):
                st["eps"] = step()
            st["graph"] = g
            st["run"] = g.replay
        # keep one captured step per generation slot (and one more with the FreeU launches, once FreeU has been enabled)
        tag = (self._slot_of(key), ("freeu", True) in key)
        self._graphs = {k: v for k, v in self._graphs.items() if (self._slot_of(k), ("freeu", True) in k) != tag}
        self._graphs[key] = st
        return st

    def _all_cross_attention_packable(self):
        """every cross-attention layer's head dim has a packed text K/V image (_refresh_text_kv), i.e. runs the
        prepared-operand kernels that read the compressed table"""
        from .u_net_condition_modify import Attention
        for m in self.unet.modules():
            if isinstance(m, Attention) and m.is_cross_attention:
                if not ops.xattn_kv_packable(1, m.to_q.weight.shape[0] // m.heads):      # the head dim alone: whatever the keys
                    return False
        return True

    @staticmethod
    def _weight_func_key(weight_func):
        """"default" for anything that behaves as `w * sigma * qk.std()`; otherwise by VALUE where that is safe - (code object,
        closure cell contents, defaults) when every captured value is an immutable scalar (int / float / bool / str / None or a
        tuple of those), so that app.py's fresh lambda per request (app.py:1004) re-uses the captured step instead of paying two
        warm-up steps and a capture under the capture lock per request - and by object identity otherwise: a captured MUTABLE
        object hashes by identity, two closures over it would share one captured step whose baked-in scalars go stale when the
        object changes, and the key would keep the object alive as long as the graph cache."""
        if weight_func_fused(weight_func):
            return "default"

        def immutable(v):
            return v is None or type(v) in (int, float, bool, str) or (type(v) is tuple and all(immutable(e) for e in v))

        code = getattr(weight_func, "__code__", None)
        if code is not None:
            try:
                cells = tuple(c.cell_contents for c in (getattr(weight_func, "__closure__", None) or ()))
                defaults = getattr(weight_func, "__defaults__", None) or ()
                kwdefaults = tuple(sorted((getattr(weight_func, "__kwdefaults__", None) or {}).items()))
                if all(immutable(v) for v in cells) and all(immutable(v) for v in defaults) and all(immutable(v) for _, v in kwdefaults):
                    return ("wf", code, cells, defaults, kwdefaults)
            except ValueError:                                       # empty cell
                pass
        return id(weight_func)

    @staticmethod
    def _slot_of(key):
        return key[0][1] if isinstance(key[0], tuple) and key[0][:1] == ("slot",) else 0

    @staticmethod
    def _compress_tables(region_state):
        """{L: (ids, rows padded to 32)} on the CPU, or None when there is no table / a level is not compressible
        (then the dense tables are used and the graph is re-captured per generation)."""
        if not isinstance(region_state, dict) or not region_state:
            return None
        out = {}
        for L, w in region_state.items():
            c = ops.compress_region_table_for_kernel(w.float().cpu() if w.is_cuda else w.float(), pad_rows=True)
            if c is None:
                return None
            out[L] = c
        return out

    @staticmethod
    def _upload_tables(st, comp_cpu, region_state):
        if st["dense"] is not None:              # the dense tables the captured step reads: refreshed in place
            for L, dst in st["dense"].items():
                src = region_state[L]
                dst.copy_(src.pin_memory() if not src.is_cuda else src, non_blocking=True)
        if comp_cpu is None:
            return
        for L, (ids, rws) in comp_cpu.items():
            dst_ids, dst_rows = st["compressed"][L]
            # pinned staging: a copy from pageable memory waits for the stream, i.e. for the previous generation
            dst_ids.copy_(ids.pin_memory() if dst_ids.is_cuda else ids, non_blocking=True)
            dst_rows.copy_(rws.pin_memory() if dst_rows.is_cuda else rws, non_blocking=True)

    def _refresh_text_kv(self, text):
        """K/V projections of the text for every cross-attention layer, once per generation (they are step-invariant;
        the reference recomputes them in all 16 layers x 25 steps).  Written IN PLACE into the buffers the captured
        graph reads."""
        from .u_net_condition_modify import Attention
        for m in self.unet.modules():
            if isinstance(m, Attention) and m.is_cross_attention:
                if text.is_cuda and text.dtype == torch.float16 and type(m.to_k) is torch.nn.Linear and m.to_k.bias is None:
                    # the package's own GEMM (as every linear of the step): the same bits in every process / on every rank
                    k = ops.linear(text, m.to_k.weight, prefer_kernel=True)
                    v = ops.linear(text, m.to_v.weight, prefer_kernel=True)
                else:
                    k, v = m.to_k(text), m.to_v(text)
                B, S, C = k.shape
                d = C // m.heads
                # one entry per static text buffer (= per captured step: a generation slot's, and its twin with the FreeU launches
                # once FreeU has been enabled); the newest few are kept, and every entry a serving batcher pinned (its bucket graphs
                # read those buffers for as long as the batcher lives, modules/serving/)
                slots = m.__dict__.setdefault("kv_caches", [])
                c = next((e for e in slots if e["src"] is text and e["k"].shape == k.shape), None)
                if c is not None:
                    c["k"].copy_(k)
                    c["v"].copy_(v)
                else:
                    c = {"src": text, "k": k, "v": v, "packed": None}
                    others = [e for e in slots if e["src"] is not text]
                    slots[:] = [e for e in others if e.get("pin")] + [e for e in others if not e.get("pin")][-7:] + [c]
                m.kv_cache = c
                # MFMA-fragment image of K / V^T for the fused kernel (rewritten in place: captured graphs keep reading it)
                if ops.xattn_kv_packable(S, d):                  # long prompts: one image per chunk of ops.XATTN_MAX_KEYS keys
                    c["packed"] = ops.xattn_kv_pack(c["k"].view(B, S, m.heads, d), c["v"].view(B, S, m.heads, d),
                                                    out=c.get("packed"))

    def _drop_text_kv(self):
        from .u_net_condition_modify import Attention
        for m in self.unet.modules():
            if isinstance(m, Attention):
                m.kv_cache = None
                m.__dict__.pop("kv_caches", None)

    def _fused_sampler_args(self, sampler, sigmas, eta, steps, sampler_opt, latents, seed, step_noise):
        """what protocol mode hands `sampler` besides the schedule (get_sampler_extra_args_t2i / _i2i), for the fused loop:
        eta (None: the sampler's own default, as img2img passes none), the solver type and the Brownian noise sampler of
        `sampler_opt` - the latter only when the loop has to build the noise table itself"""
        args = {"solver_type": "heun" if sampler_opt.get("solver_type", None) == "heun" else "midpoint"}
        if eta is not None:
            args["eta"] = eta
        if step_noise is None and sampler_opt.get("brownian_noise", False) \
                and (sampling.linear_family(sampler) in ("euler_ancestral", "dpmpp_2m_sde", "lcm")
                     or sampling.two_call_family(sampler) in ("dpm_2_ancestral", "dpmpp_2s_ancestral", "dpmpp_sde")):
            args["noise_sampler"] = self.create_noise_sampler(latents, sigmas, steps, seed)
        return args

    @staticmethod
    def _check_step_noise(noise, steps, x):
        """the noise table of a fused / served generation: [steps, 1 or n, *latent] -> dense, x's dtype, on x's device"""
        want = (steps,) + tuple(x.shape)
        if not torch.is_tensor(noise) or noise.dim() != len(want) or tuple(noise.shape[2:]) != want[2:] \
                or noise.shape[0] != steps or noise.shape[1] not in (1, x.shape[0]):
            raise ValueError(f"step_noise must be a [{steps}, 1 or {x.shape[0]}, {', '.join(str(v) for v in x.shape[1:])}] tensor, "
                             f"got {tuple(noise.shape) if torch.is_tensor(noise) else type(noise).__name__}")
        return noise.to(device=x.device, dtype=x.dtype).contiguous()

    def _rows_fused_loop(self, st, x, old, plan, noise, tab, guidance_scale, n_img, start_time, timeout, rescale=0.0, extras=None):
        """the fused loop's steps through the per-row kernels: one model call and one launch per entry of `plan`, one record per
        image, all on the same call of the same plan.  A two-call plan launches dsc_cfg_staged_step_rows (the step's intermediate
        point in `mid`), any other dsc_cfg_linear_step_rows; rescale > 0: every record carries it (the wrappers then issue the
        rescale launch); extras: the images' extra input channels of a 9-channel UNet (ops.cfg_linear_step_rows_cat writes them
        behind each latent row)"""
        mid = torch.zeros_like(x) if plan.two_call else None
        for k, call in enumerate(plan):
            self._check_timeout(start_time, timeout)
            st["run"]()
            after = (1.0, 0.0, 1e-10, None)                          # (c_in, t, sigma, time-embedding row) of the coming call
            if k + 1 < len(plan):
                nxt = plan[k + 1]
                after = (nxt.c_in, nxt.t, max(nxt.sigma, 1e-10), None if tab is None else tab[k + 1])
            recs = [step_record(plan, call, guidance_scale, rescale,
                                None if noise is None or call.s == 0.0 else noise[k, j if noise.shape[1] > 1 else 0], *after)
                    for j in range(n_img)]
            if plan.two_call:
                ops.cfg_staged_step_rows(x, mid, st["eps"], old, n_img, st["x_in"], st["t"], st["sigma_rows"], recs, tadd=st["tadd"])
            elif extras is not None:
                ops.cfg_linear_step_rows_cat(x, st["eps"], old, n_img, st["x_in"], st["t"], st["sigma_rows"], recs, extras,
                                             tadd=st["tadd"])
            else:
                ops.cfg_linear_step_rows(x, st["eps"], old, n_img, st["x_in"], st["t"], st["sigma_rows"], recs, tadd=st["tadd"])

    def _denoise_fused(self, latents, sigmas, text, region_state, weight_func, guidance_scale, n_img,
                       cross_attention_kwargs, start_time, timeout, slot=0, sampler=None, sampler_args=None, step_noise=None,
                       guidance_rescale=0.0, extra=None, two_call=False):
        """sampler: None (DPM++ 2M) or one of sampling.LINEAR_FAMILY's functions - with two_call=True also one of
        sampling.TWO_CALL_FAMILY's: one model call and one dsc_cfg_staged_step_rows launch per entry of sampling.call_plan, the
        step's intermediate point kept in `mid` beside `old`; step_noise then has one row per model call
        (sampling.call_noise_table); not with `extra`.  DPM++ 2M on an eps-prediction model is one
        dsc_cfg_dpmpp2m_step per step; every other member, and every v-prediction model, one dsc_cfg_linear_step_rows with a
        record per image.  step_noise: the noise table [steps, 1 or n_img, c, h, w] (default: sampling.step_noise_table).
        guidance_rescale (phi, arXiv 2305.08891 sec. 3.4) > 0: every family member, DPM++ 2M on an eps model included, takes the
        per-row path and its records carry phi - the statistics of rescale_noise_cfg are taken inside the sampler launch
        (dsc_cfg_linear_step_rows_rescale), on the denoised estimate as protocol mode's model_fn does.
        extra: fp16 [n_img, c, h, w], the step-invariant channels a UNet with in_channels = 4 + c reads beside the latent (the
        9-channel inpainting checkpoints, reference :1617-1619).  The static step's x_in then has 4 + c channels, every sampler
        takes the per-row path (DPM++ 2M on an eps model too: its records are that sampler's bits) and every launch, the first
        input's JOIN records included, is dsc_cfg_linear_step_rows_cat, which scales the extra channels by the coming c_in."""
        guidance_rescale = float(guidance_rescale)
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"fused=True: guidance_rescale must be in [0, 1], got {guidance_rescale}")
        family = "dpmpp_2m" if sampler is None else sampling.linear_family(sampler)
        staged = family is None and two_call and sampling.two_call_family(sampler) is not None
        if staged:
            family = sampling.two_call_family(sampler)
            if extra is not None:
                raise NotImplementedError(f"fused=True: the two-call sampler {family!r} has no step for a UNet with extra input "
                                          "channels (dsc_cfg_staged_step_rows takes no CAT form); run it with fused=False")
        if family is None:
            raise NotImplementedError(f"fused=True: sampler {getattr(sampler, '__name__', sampler)!r} has no fused step "
                                      f"(supported: {', '.join(sampling.LINEAR_FAMILY)}); run it with fused=False")
        rows_path = staged or family != "dpmpp_2m" or self.v_prediction or guidance_rescale > 0.0 or extra is not None
        if rows_path and n_img > ops.ROW_STEP_MAX_SLOTS:
            raise NotImplementedError(f"fused=True: the per-row sampler step takes at most {ops.ROW_STEP_MAX_SLOTS} images per "
                                      f"batch, got {n_img}; run it with fused=False")
        # the lockstep kernel's wrapper refuses CPU / non-fp16 tensors itself, deep inside the loop; the per-row path builds
        # records and a noise table first, so it says so here (tests/test_host_logic.py probes a v-prediction pipeline's fused
        # path with no tensors at all and expects this error class)
        if rows_path and not (torch.is_tensor(latents) and latents.is_cuda and text.dtype == torch.float16):
            raise NotImplementedError("fused=True: the per-row sampler step (dsc_cfg_linear_step_rows: every sampler but DPM++ 2M, "
                                      "v-prediction models, and guidance_rescale) runs fp16 latents on the GPU; run it with "
                                      "fused=False")
        # dsc_cfg_linear_step_rows and its rescale form move 8 halfs per lane; a latent with both sides odd (152 x 152 pixels:
        # 4 * 19 * 19 = 1444 halfs) runs DPM++ 2M's own step only, which also takes rows of 4 * odd halfs
        if rows_path and latents[0].numel() % 8 != 0:
            raise NotImplementedError(f"fused=True: the per-row sampler step (dsc_cfg_linear_step_rows: every sampler but DPM++ "
                                      f"2M, v-prediction models, and guidance_rescale) needs a latent of a multiple of 8 halfs, "
                                      f"got {list(latents.shape[1:])} (both sides odd); run it with fused=False")
        if self.v_prediction and not self.k_diffusion_model.pass_kwargs:
            region_state, cross_attention_kwargs = None, {}          # CompVisVDenoiser.get_v forwards (x, t, cond) only
        prof = os.environ.get("DSC_PROFILE_HOST") == "1"
        if prof:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        kdm = self.k_diffusion_model
        sig = getattr(sigmas, "_dsc_host", None)                     # host copy made where the schedule was built, or
        if sig is None:
            sig = sigmas.detach().float().cpu().tolist()             # one device->host transfer before the loop
        sargs = dict(sampler_args or {})
        noise_sampler = sargs.pop("noise_sampler", None)
        # one entry per model call; on the lockstep path (DPM++ 2M's own kernel) only its sigma, (a, b, c) and model scalars are read
        plan = step_plan(kdm, family, sig, latents.dtype, eta=sargs.get("eta"), s_noise=sargs.get("s_noise"),
                         solver_type=sargs.get("solver_type"), needs_linear=rows_path)
        ack = getattr(self, "_added_cond_kwargs", None)
        ip_key = None if ack is None else (tuple(tuple(e.shape) for e in ack["image_embeds"]),
                                           id(getattr(self.unet, "encoder_hid_proj", None)))
        # a callable that behaves as the default `w * sigma * qk.std()` (app.py:1004 builds a fresh lambda per request) runs
        # the fused kernels whatever object it is; any other callable is baked into the captured step, so the key is the
        # OBJECT (two closures of one code object may capture different values) and the step keeps it alive
        in_shape = tuple(latents.shape)                              # of the static step's x_in (per CFG half)
        extras = None
        if extra is not None:
            if tuple(extra.shape[2:]) != in_shape[2:] or extra.shape[0] != n_img or extra[0].numel() % 8 != 0:
                raise ValueError(f"fused=True: extra input channels {tuple(extra.shape)} do not fit latents {in_shape} "
                                 "(one row of a multiple of 8 halfs per image)")
            extra = extra.to(device=latents.device, dtype=latents.dtype).contiguous()
            extras = [extra[j] for j in range(n_img)]
            in_shape = (n_img, in_shape[1] + extra.shape[1]) + in_shape[2:]
        key = self._step_key(slot, n_img, in_shape, region_state, text, weight_func, ip_key)
        if latents.is_cuda:
            # generation slots: each keeps its own static buffers, captured step, packed K/V and library-GEMM workspace, so
            # two generations can be in flight on two streams (one host thread per slot)
            _lib.check(_lib.load_library().dsc_set_workspace_slot(slot), "dsc_set_workspace_slot")
        st = self._static_step(key, n_img, in_shape, text, region_state, weight_func, cross_attention_kwargs)
        x = latents.contiguous().clone()
        old = torch.zeros_like(x)
        if prof:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        c_in, t = plan[0].c_in, plan[0].t
        tab = None
        if st["tadd"] is not None:
            # the schedule's timesteps are known here: every step's embedding rows in one table (kept while the schedule repeats)
            tkey = (tuple(call.sigma for call in plan), self.unet.temb_signature())   # the schedule AND the weights the table bakes in
            if st["temb_key"] != tkey:
                st["temb_tab"] = self.unet.temb_add_table(torch.tensor([call.t for call in plan], dtype=torch.float32, device=x.device))
                st["temb_key"] = tkey
            tab = st["temb_tab"]
        if extras is not None:
            # the first model input: JOIN records (dsc_prepare_unet_input's line per row, plus the extra channels), no source bucket
            join = {"mode": ops.ROW_JOIN, "c_in_next": c_in, "t_next": t, "sigma_next": sig[0], "temb_row": None if tab is None else tab[0]}
            ops.cfg_linear_step_rows_cat(x, None, old, 0, st["x_in"], st["t"], st["sigma_rows"], [join] * n_img, extras, tadd=st["tadd"])
        else:
            ops.prepare_unet_input(x, c_in, t, sig[0], st["x_in"], st["t"], st["sigma"], row=None if tab is None else (tab[0], st["tadd"]))
        if rows_path:
            noise = None
            if plan.noisy:
                noise = step_noise
                if noise is None:
                    table = sampling.call_noise_table if plan.two_call else sampling.step_noise_table
                    noise = table(family, x, sigmas, eta=sargs.get("eta", 1.0), noise_sampler=noise_sampler)
                noise = self._check_step_noise(noise, len(plan), x)
            self._rows_fused_loop(st, x, old, plan, noise, tab, guidance_scale, n_img, start_time, timeout,
                                  rescale=guidance_rescale, extras=extras)
        for i, call in enumerate(() if rows_path else plan):        # DPM++ 2M's own lockstep kernel (sampling.dpmpp_2m_coefficients)
            self._check_timeout(start_time, timeout)
            st["run"]()
            c_in_n, t_n, nxt = (plan[i + 1].c_in, plan[i + 1].t, plan[i + 1].sigma) if i + 1 < len(plan) else (1.0, 0.0, 0.0)
            # x <- a*x + b*D + c*D_old with D = x - sigma*(eps_u + g*(eps_c - eps_u)); also writes next x_in/t/sigma
            ops.cfg_dpmpp2m_step(x, st["eps"], old, call.sigma, guidance_scale, call.a, call.b, call.c, c_in_n, t_n, max(nxt, 1e-10),
                                 st["x_in"], st["t"], st["sigma"],
                                 row=(tab[i + 1], st["tadd"]) if tab is not None and i + 1 < len(plan) else None)
        if x.is_cuda:
            self._record_done(st, x.device)
        if prof:
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print(f"[dsc host profile] setup (tables, text K/V, graph) {1e3 * (t1 - t0):.1f} ms, "
                  f"{len(plan)}-call loop {1e3 * (t2 - t1):.1f} ms", flush=True)
        return x
