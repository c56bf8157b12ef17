"""The host side of the continuous batcher: `ServingBatcher` (construction, the public interface, the scheduling of every step
against a replaceable device executor) and `HiresPair`.  The package docstring has slots, buckets and the step.

Samplers and parameterisation.  A request names its sampler (`sampler_name`: one of sampling.LINEAR_FAMILY - Euler, Euler a,
DPM++ 2M (default), DPM++ 2M SDE, LCM - by name or as the callable) with `eta` / `s_noise` / `solver_type`; the noise of all its
steps is one table on the device from submit until it leaves (`step_noise`, or sampling.step_noise_table from `seed` /
`generator`), and its record for step j points at row j.  A transition in which every stepping slot is DPM++ 2M on an
eps-prediction model launches dsc_cfg_dpmpp2m_step_rows as before; any other launches dsc_cfg_linear_step_rows for all slots
(DPM++ 2M slots ride in it with the same bits).  On a v-prediction pipeline every slot carries CompVisVDenoiser's scalars (and,
with `pass_kwargs = False`, zero region tables: the reference's v-prediction path never sees the region prompt).  The
known-region launch of inpainting carries DPM++ 2M records only, so an inpainting request and a request of another sampler never
share a batch: the later one waits in the queue until the others have left.

Two-call samplers.  On a batcher built with `two_call=True` a request may also name a sampler of sampling.TWO_CALL_FAMILY (Heun,
DPM2, DPM2 a, DPM++ 2S a, DPM++ SDE): two model calls per sampler step.  A request's `plan` (step_plan.py, the fused loop's too)
holds one entry per MODEL CALL whatever its sampler - here sampling.call_plan's - `r.i` is the index of the model call that runs
now, and every transition applies one call: PREDICT writes the step's intermediate point into the slot's row of `exec.mid` and
leaves x alone, CORRECT reads it back (dsc_cfg_staged_step_rows).  A transition in which some slot carries such a stage launches that entry for
all slots - the one-call members ride in it as FULL records with the bits they have otherwise - and any other transition the
launch it had.  Not with ControlNet / T2I-Adapter requests (their windows count one model call per step), inpainting or
`inpaint_unet`.

Guidance rescale.  A request may carry `guidance_rescale` (phi in [0, 1], arXiv 2305.08891 sec. 3.4; the usual companion of
v-prediction models).  Its STEP records carry `rescale` and, DPM++ 2M on an eps-prediction model included, (c_skip, c_out); a
transition in which such a slot steps launches dsc_cfg_linear_step_rows_rescale for all slots (ops.cfg_linear_step_rows picks it
from the records), every other transition the launch it had.  Inpainting with rescale is refused at submit.

Hires requests.  A batcher is built for one image size, so the reference's "Hires fix" (generate at the base size, enlarge the
final latents, img2img at the target size; model_k_diffusion.py:1176-1228) runs on a chained PAIR of batchers on two workspace
slots (`pipe.serve_hires`, or `base.chain_hires(hi)`).  A request with `upscale=True` is validated and prepared for BOTH passes at
submit (the second pass with its own sampler, schedule tail, coefficients, time-embedding table, region tables at the target
size and noise).  When it leaves the first batcher, ONE launch of dsc_latent_resample_noise on that batcher's stream reads its
final row of x and writes the second pass's start latent (the enlarged row + noise * fp16 sqrt(sigma_0^2 + 1), img2img's line)
into a tensor of the second-pass record; an event is recorded, the record joins the second batcher's queue, and that batcher's
stream waits on the event before it loads the row.  Only the first batcher ever takes the second's lock (no cycle); the caller's
one Future resolves with the second pass's output.  No host synchronisation between the passes.

The region tables of a batch are compressed to at most 32 distinct rows per level (the prepared-operand kernels' LDS table): a
request whose admission would push the union of the active requests' rows past that waits in the queue (FIFO) until a slot frees.
"""
import collections
import concurrent.futures
import threading
import time

import torch

from ... import ops
from .. import sampling
from ..encode_region_map_function import encode_region_map
from ..step_plan import step_plan, step_record
from . import requests, text_lane
from .encode_lane import _EncodeHandle, encode_roles
from .executor import _GraphExecutor, step_launch
from .requests import MAX_TEXT_KEYS, _Request, _ip_layers


def _conv_out_hw(conv, h, w):
    """(h, w) of `conv`'s output on an h x w input, from the module's own kernel size, padding and stride"""
    return tuple((v + 2 * conv.padding[i] - conv.kernel_size[i]) // conv.stride[i] + 1 for i, v in enumerate((h, w)))


class ServingBatcher:
    """See the package docstring.  `executor` is the device side (default: the captured-graph executor on the pipeline's GPU);
    the scheduling here is host logic only."""

    def __init__(self, pipe, height, width, max_batch=8, slot=0, buckets=(1, 2, 4, 8), text_len=77, executor=None, ip_masks=False,
                 t2i_adapter=False, controlnet=False, control_slots=None, decode=False, decode_batch=2, previews=False,
                 preview_scale=8, preview_coef=None, preview_ring=8, inpaint_unet=False, freeu=False, encode=False, encode_batch=2,
                 two_call=False, text=False, text_batch=2, clip_skip=None):
        requests.check_freeu_off(pipe)
        buckets = tuple(sorted(set(int(b) for b in buckets)))
        if not buckets or buckets[0] < 1 or buckets[-1] < max_batch:
            raise ValueError(f"serve: buckets {buckets} must cover max_batch={max_batch}")
        if max_batch > ops.ROW_STEP_MAX_SLOTS:
            raise ValueError(f"serve: at most {ops.ROW_STEP_MAX_SLOTS} slots (dsc_cfg_dpmpp2m_step_rows)")
        if text_len > MAX_TEXT_KEYS:
            raise ValueError(f"serve: at most {MAX_TEXT_KEYS} text keys")
        self.pipe, self.height, self.width = pipe, int(height), int(width)
        self.max_batch, self.slot, self.buckets, self.text_len = int(max_batch), int(slot), buckets, int(text_len)
        self._lock = threading.RLock()
        self._wake = threading.Condition(self._lock)
        self._queue = collections.deque()
        self._slots = [None] * self.max_batch
        self._done = []                        # (request, handle) whose final row copy is in flight
        self._n = None                         # bucket whose eps is pending (None: nothing ran yet / the batch drained)
        self._members = {}                     # bucket -> per-slot request ids its static buffers were last refreshed for
        self._gates = {}                       # bucket -> the adapter gate vector last uploaded for it (absent: zeros, as captured)
        self._next_id = 0
        self._stats = collections.Counter(captures=0, joins=0, leaves=0, bucket_switches=0, steps=0, refreshes=0,
                                          linear_transitions=0, handoffs=0, adapter_gate_updates=0, control_steps=0,
                                          control_gate_updates=0)
        self._hires = None                     # the chained batcher of the hires pass (chain_hires)
        # requests may carry `freeu`: the step holds the FreeU launches, which read (s1, s2, b1, b2) per row from a table (executor.py)
        self.freeu = bool(freeu)
        self._freeu_rows = {}                  # bucket -> the table last uploaded for it (absent: ones, as captured)
        if self.freeu:
            self._stats["freeu_updates"] = 0
        # a 9-channel inpainting UNet: every request is an inpainting request, and every transition writes each member's mask and
        # masked-image latents behind its latent row (dsc_cfg_linear_step_rows_cat; package docstring)
        self.inpaint = bool(inpaint_unet)
        if self.inpaint and two_call:
            raise ValueError("serve: `two_call=True` and `inpaint_unet=True` are not served together (the staged step has no "
                             "form with extra input channels)")
        if self.inpaint:
            self._inpaint_setup(controlnet, t2i_adapter)
        # requests may name a sampler of sampling.TWO_CALL_FAMILY: two transitions per sampler step, the intermediate point in a
        # third state row (dsc_cfg_staged_step_rows)
        self.two_call = bool(two_call)
        if self.two_call:
            self._stats["staged_transitions"] = 0
        # requests may ask for images ("pil" / "np" / "uint8"): a decode lane beside the step finishes them (decode_lane.py)
        self.decode = bool(decode)
        self.decode_batch = 0
        if self.decode:
            if getattr(pipe, "vae", None) is None:
                raise ValueError("serve: `decode=True` on a pipeline without a VAE (construct it with a "
                                 "modules.vae_decoder.AutoencoderKLDecoder, or serve latents)")
            if isinstance(decode_batch, bool) or not isinstance(decode_batch, int) or not 1 <= decode_batch <= self.max_batch:
                raise ValueError(f"serve: `decode_batch` must be an integer in [1, max_batch = {self.max_batch}], got {decode_batch!r}")
            self.decode_batch = decode_batch
            self._stats["decodes"] = self._stats["decode_rows"] = 0
        # pixel inputs (`image` / `mask_image` as pixels) are encoded on an encode lane beside the step (encode_lane.py)
        self.encode = bool(encode)
        self.encode_batch = 0
        if self.encode:
            if getattr(pipe, "vae", None) is None or not hasattr(pipe.vae, "encode"):
                raise ValueError("serve: `encode=True` on a pipeline without a VAE encoder (construct it with a "
                                 "modules.vae_decoder.AutoencoderKL, or pass [1, 4, h, w] latents as `image`)")
            if isinstance(encode_batch, bool) or not isinstance(encode_batch, int) or not 1 <= encode_batch <= self.max_batch:
                raise ValueError(f"serve: `encode_batch` must be an integer in [1, max_batch = {self.max_batch}], got {encode_batch!r}")
            self.encode_batch = encode_batch
            self._stats["encodes"] = self._stats["encode_rows"] = 0
        # requests may carry `prompt` / `negative_prompt` strings: a text lane beside the step encodes them (text_lane.py)
        self.text_on = bool(text)
        self.text_batch, self.clip_skip, self._parser = 0, None, None
        if self.text_on:
            if isinstance(text_batch, bool) or not isinstance(text_batch, int) or not 1 <= text_batch <= ops.PROMPT_WEIGHT_MAX_GROUPS:
                raise ValueError(f"serve: `text_batch` must be an integer in [1, {ops.PROMPT_WEIGHT_MAX_GROUPS}] (the groups of one "
                                 f"dsc_prompt_weight_rows_f16 launch), got {text_batch!r}")
            self._parser = text_lane.check_pipeline(pipe, pipe.unet.config.cross_attention_dim, self.text_len, clip_skip)
            self.text_batch, self.clip_skip = text_batch, clip_skip
            self._stats["text_encodes"] = self._stats["text_groups"] = 0
        # requests may carry `preview_every` / `on_preview`: thumbnails of the denoised estimate leave beside the step
        # (preview_lane.py)
        self.previews = bool(previews)
        self.preview_scale, self.preview_coef, self.preview_ring = 0, None, 0
        self._preview_queue = collections.deque()   # (handle, [(state, step, steps)] in row order) of queued previews, oldest first
        self._preview_of = {}                  # request -> its _PreviewState (only requests that asked), until it resolves / hands off
        if self.previews:
            self._preview_setup(preview_scale, preview_coef, preview_ring)
        self._warm_captures = None
        self._thread = None
        self._stop = False
        # the weights this batcher's captured steps hold (derived copies included): a LoRA change on the pipeline retires it
        self._weights_epoch = getattr(pipe, "weights_epoch", 0)
        if hasattr(pipe, "_batchers"):
            pipe._batchers.add(self)                    # load / set / unload refuse while one of these runs its own thread
        # the IP-Adapters this batcher's step is built for (load_ip_adapter): the processors, the image projection, tokens per adapter
        self._ip = _ip_layers(pipe)
        self._ip_proj = getattr(pipe.unet, "encoder_hid_proj", None) if self._ip else None
        self._ip_tokens = [int(t) for t in self._ip[0][1].num_tokens] if self._ip else []
        if any(t > ops.IP_MAX_TOKENS for t in self._ip_tokens):
            raise ValueError(f"serve: a loaded IP-Adapter has {max(self._ip_tokens)} image tokens; the batcher's image-token attention "
                             f"(dsc_ip_xattn_add_f16) takes at most {ops.IP_MAX_TOKENS} (ops.IP_MAX_TOKENS) - the 257-token Full "
                             f"projection runs through txt2img(ip_adapter_image_embeds=...)")
        # requests may carry `ip_adapter_masks`: the step hands per-query weights to the masked entry (requests.py)
        self.ip_masks = bool(ip_masks)
        if self.ip_masks and not self._ip:
            raise ValueError("serve: `ip_masks=True` on a pipeline without an IP-Adapter (pipe.load_ip_adapter first, then build the "
                             "batcher)")
        # requests may carry `image_t2i_adapter`: the step hands the UNet per-slot features and a per-row gate (executor.py)
        self.t2i = bool(t2i_adapter)
        if controlnet and self.t2i:
            raise ValueError("serve: `controlnet=True` and `t2i_adapter=True` are not served together yet (build one batcher for each)")
        self._adapter = getattr(pipe, "adapter", None) if self.t2i else None
        self._adapter_shapes = self._adapter_setup() if self.t2i else None
        # requests may carry `control_img`: a compact ControlNet batch of `control_slots` lanes runs beside the step, and the
        # step scatters its residuals into the rows of the requests that hold a lane (executor.py)
        self.cn = bool(controlnet)
        self._controlnet = getattr(pipe, "controlnet", None) if self.cn else None
        self.control_slots = (self.max_batch if control_slots is None else int(control_slots)) if self.cn else 0
        self._control_shapes = self._controlnet_setup() if self.cn else None
        self._lanes = [None] * self.control_slots     # lane -> the request that holds it
        self._cstate = {}                      # bucket -> (dst, gather, gates) last uploaded for it (absent: as captured)
        self.exec = executor if executor is not None else _GraphExecutor(self)

    def _inpaint_setup(self, controlnet, t2i_adapter):
        """`inpaint_unet=True` against the UNet and this batcher's size, at construction"""
        c = int(self.pipe.unet.config.in_channels)
        if c != 9:
            raise ValueError(f"serve: `inpaint_unet=True` serves the 9-channel inpainting UNets ([latents | mask | masked-image "
                             f"latents]); this pipeline's UNet has in_channels = {c}")
        if controlnet or t2i_adapter:
            raise ValueError("serve: `inpaint_unet=True` and `controlnet=True` / `t2i_adapter=True` are not served together yet")
        h, w = self.height // 8, self.width // 8
        if (h * w) % 8 != 0:
            raise ValueError(f"serve: `inpaint_unet=True`: this batcher's {h}x{w} latent has h * w % 8 != 0; the 9-channel input "
                             "row (4 + 5 maps of h * w halfs) must stay 16-byte aligned (use inpaiting)")
        self._stats["cat_transitions"] = 0

    def _preview_setup(self, scale, coef, ring):
        """the preview arguments against this batcher's latent, at construction"""
        from ...latent_preview import preview_coef
        from .preview_lane import preview_scales_for
        # (the latent a preview reads has 4 channels whatever else an inpainting UNet's input carries)
        C, w = 4 if self.inpaint else int(self.pipe.unet.config.in_channels), self.width // 8
        if self.max_batch > ops.PREVIEW_MAX_ROWS or C > ops.PREVIEW_MAX_CHANNELS:
            raise ValueError(f"serve: `previews=True` takes at most {ops.PREVIEW_MAX_ROWS} slots and {ops.PREVIEW_MAX_CHANNELS} latent "
                             f"channels (dsc_latent_preview), got max_batch = {self.max_batch}, {C} channels")
        works = preview_scales_for(w)
        if isinstance(scale, bool) or not isinstance(scale, int) or scale not in works:
            raise ValueError(f"serve: `preview_scale` {scale!r} does not work at a latent width of {w}: the thumbnail's width "
                             f"(latent width * scale) must be a multiple of 8; at this size use one of {', '.join(map(str, works))}")
        if isinstance(ring, bool) or not isinstance(ring, int) or ring < 1:
            raise ValueError(f"serve: `preview_ring` must be an integer >= 1, got {ring!r}")
        self.preview_scale, self.preview_ring = scale, ring
        self.preview_coef = preview_coef(coef, C)                # (None: LATENT_RGB_SD15; a wrong count is refused here)
        for key in ("previews", "preview_rows", "previews_dropped", "preview_callback_errors"):
            self._stats[key] = 0

    def _adapter_setup(self):
        """the adapter against the UNet, at construction -> [(C_k, h_k, w_k)] of the feature each down block adds: as many maps
        as down blocks, the UNet's channels, and the size of the tensor the add lands on.  Both sides are computed from their own
        modules' parameters (the adapter's PixelUnshuffle and pooling, the UNet's stride-2 convolutions), not assumed equal."""
        from ..t2i_adapter import MultiAdapter
        pipe, ad = self.pipe, self._adapter
        if ad is None:
            raise ValueError("serve: `t2i_adapter=True` on a pipeline without a T2I-Adapter "
                             "(modules.t2i_adapter.setup_model_t2i_adapter(pipe, adapter) first, then build the batcher)")
        unet = pipe.unet
        # the UNet: block k adds after its last attention (before its downsampler) or, without attention, after the whole block
        h, w = self.height // 8, self.width // 8
        want = []
        for c, blk in zip(unet.config.block_out_channels, unet.down_blocks):
            size = (h, w)
            if hasattr(blk, "downsamplers"):
                h, w = _conv_out_hw(blk.downsamplers[0].conv, h, w)
                if not blk.has_attn:
                    size = (h, w)
            want.append((int(c), int(size[0]), int(size[1])))
        for a, one in enumerate(ad.adapters if isinstance(ad, MultiAdapter) else [ad]):
            full = getattr(one, "adapter", None)
            if full is None or not hasattr(full, "body") or not hasattr(full, "unshuffle"):
                raise ValueError(f"serve: `t2i_adapter=True`: adapter {a} is not a full_adapter T2IAdapter (the type the batcher serves)")
            f = int(full.unshuffle.downscale_factor)
            if self.height % f or self.width % f:
                raise ValueError(f"serve: `t2i_adapter=True`: {self.height}x{self.width} is not a multiple of the adapter's "
                                 f"downscale factor {f}")
            ah, aw = self.height // f, self.width // f
            got = []
            for blk in full.body:
                pool = blk.downsample
                if pool is not None:
                    k_, s_ = int(pool.kernel_size), int(pool.stride)
                    ah, aw = ((-(-(v - k_) // s_) if pool.ceil_mode else (v - k_) // s_) + 1 for v in (ah, aw))
                got.append((int(blk.resnets[-1].block2.out_channels), int(ah), int(aw)))
            if len(got) != len(want):
                raise ValueError(f"serve: `t2i_adapter=True`: adapter {a} gives {len(got)} feature maps, the UNet has {len(want)} "
                                 f"down blocks")
            if got != want:
                raise ValueError(f"serve: `t2i_adapter=True`: adapter {a}'s feature maps (C, h, w) {got} do not match what the "
                                 f"UNet's down blocks add to at {self.height}x{self.width}: {want}")
        return want

    def _control_nets(self):
        from ..controlnet import MultiControlNetModel
        cn = self._controlnet
        return list(cn.nets) if isinstance(cn, MultiControlNetModel) else [cn]

    @staticmethod
    def _skip_shapes(model, h, w):
        """[(C, h, w)] of the skip tensors an encoder half (the UNet's, a ControlNet's) collects at an h x w latent, the mid
        block's output last - from the module's own convolutions (conv_in, every ResNet's conv2, the stride-2 downsamplers)"""
        shapes = [(int(model.conv_in.out_channels), int(h), int(w))]
        for blk in model.down_blocks:
            for res in blk.resnets:
                shapes.append((int(res.conv2.out_channels), int(h), int(w)))
            if hasattr(blk, "downsamplers"):
                conv = blk.downsamplers[0].conv
                h, w = _conv_out_hw(conv, h, w)
                shapes.append((int(conv.out_channels), int(h), int(w)))
        return shapes + [(int(model.mid_block.resnets[-1].conv2.out_channels), int(h), int(w))]

    def _controlnet_setup(self):
        """the ControlNet against the UNet, at construction -> [(C, h, w)] of every skip tensor and of the mid block's output,
        the tensors its residuals are added to.  Both sides are computed from their own modules, not assumed equal."""
        from ..controlnet import ControlNetModel
        if self._controlnet is None:
            raise ValueError("serve: `controlnet=True` on a pipeline without a ControlNet (pipe.setup_controlnet(controlnet) first, "
                             "then build the batcher)")
        if not 1 <= self.control_slots <= self.max_batch:
            raise ValueError(f"serve: `control_slots` must be in [1, max_batch = {self.max_batch}], got {self.control_slots}")
        nets = self._control_nets()
        from ... import scatter_add
        if len(nets) > scatter_add.MAX_NETS:
            raise ValueError(f"serve: `controlnet=True`: {len(nets)} ControlNets; the step's scatter-add takes at most "
                             f"{scatter_add.MAX_NETS}")
        want = self._skip_shapes(self.pipe.unet, self.height // 8, self.width // 8)
        for a, net in enumerate(nets):
            if not isinstance(net, ControlNetModel):
                raise ValueError(f"serve: `controlnet=True`: net {a} is a {type(net).__name__}, not a ControlNetModel")
            if net.config.global_pool_conditions:
                raise ValueError(f"serve: `controlnet=True`: net {a} is a guess-mode ControlNet (global_pool_conditions), which the "
                                 "batcher does not serve (use txt2img)")
            got = self._skip_shapes(net, self.height // 8, self.width // 8)
            if got != want:
                raise ValueError(f"serve: `controlnet=True`: net {a}'s residuals (C, h, w) {got} do not match the UNet's skip tensors "
                                 f"and mid output at {self.height}x{self.width}: {want}")
        return want

    # ------------------------------------------------------------------ public interface
    def _check_weights(self):
        now = getattr(self.pipe, "weights_epoch", 0)
        if now != self._weights_epoch:
            raise RuntimeError(f"serve: the pipeline's weights changed since this batcher was built (LoRA load / set_lora_scale / "
                               f"unload: weights_epoch {self._weights_epoch} -> {now}); its captured steps hold the old weights - "
                               f"build a new batcher")

    def warm(self):
        """capture every bucket's step now (otherwise each is captured on first use)"""
        self._check_weights()
        with self._lock:
            if self.t2i:
                self.exec.warm_adapter()             # the adapter's convolutions pay their first-call cost here, not at a join
            if self.cn:
                self._ensure_control()               # the ControlNet graph first: every bucket's step reads its residual buffers
                self.exec.warm_control()
            for n in self.buckets:
                self._ensure(n)
            if self.decode:
                self._ensure_decode()                # the lane's stream, static buffers, graphs and pinned ring
            if self.encode:
                self._ensure_encode()                # the encode lane's stream, static buffers, graphs, staging and pinned ring
            if self.previews:
                self.exec.ensure_preview()           # the preview stream and its ring of device / pinned buffers
            if self.text_on:
                self._ensure_text()                  # the text lane's stream, static buffers, graphs and the empty chunk's rows
            self._warm_captures = self._stats["captures"]
        return self

    def chain_hires(self, hi):
        """requests with `upscale=True` run their second pass on `hi`, a batcher of the target size on another workspace slot
        (executor.py); `hi` keeps serving ordinary requests of its size.  Returns self."""
        if not isinstance(hi, ServingBatcher):
            raise TypeError("serve: chain_hires takes the ServingBatcher of the hires pass")
        if self.inpaint or hi.inpaint:
            raise ValueError("serve: a batcher built with `inpaint_unet=True` is not chained (inpaiting refuses the hires pass too)")
        if hi is self:
            raise ValueError("serve: a batcher cannot be chained to itself (the hires pass runs at another image size)")
        if hi.slot == self.slot:
            raise ValueError(f"serve: both batchers of a hires pair sit on workspace slot {self.slot}; give the second its own")
        if hi.pipe is not self.pipe:
            raise ValueError("serve: both batchers of a hires pair serve the same pipeline")
        if hi.height < self.height or hi.width < self.width:
            raise ValueError(f"serve: the hires batcher runs {hi.height}x{hi.width}, smaller than this one's "
                             f"{self.height}x{self.width} (only enlarging is served)")
        if self.text_on and hi.text_len != self.text_len:
            raise ValueError(f"serve: `text=True` on a hires pair: the second pass shares the first's text rows, but the batchers "
                             f"run {self.text_len} and {hi.text_len} text keys")
        with self._lock:
            self._hires = hi
        return self

    def submit(self, request):
        """request: txt2img_coalesced's request dict plus its own `num_inference_steps` (default 25), `sampler_opt` (the
        schedule: karras / exponential / ...), `guidance_scale` (> 1, default 7.5) and `latents` / `generator`; optional
        `output_type` ("latent", default, or what latent_to_image takes; on a batcher built with `decode=True`: "latent", "pil",
        "np" / "numpy" - float32 [H, W, 3] - or "uint8" - np.uint8 [H, W, 3], the bytes of the PIL image), `sampler_name`
        (sampling.LINEAR_FAMILY, default DPM++ 2M) with `eta` / `s_noise` / `solver_type`, `step_noise` ([steps, 1, 4, h, w]: the noise of every step;
        default: drawn as the sampler itself would, from `seed` / `generator`) and `guidance_rescale` (in [0, 1], default 0; not
        with `mask_image`).  On a pipeline with IP-Adapters loaded: `ip_adapter_image_embeds` (a list with one tensor per loaded
        adapter, each [negative; positive] along dim 0 with ONE image per half - what txt2img takes, see encode_image; absent /
        None: the request runs without an image prompt beside those that have one) and `ip_adapter_scale` (a float, or a list
        with one entry per adapter; default: the processors' scale at submit time, so set_ip_adapter_scale needs no capture); on a
        batcher built with `ip_masks=True` also `cross_attention_kwargs={"ip_adapter_masks": t}`, t [n_adapters, 1, Hm, Wm]: each
        adapter's term is multiplied by its mask, down-sampled per level as the reference does (ignored without an image prompt).
        On a chained pair (chain_hires) `upscale=True` adds the hires pass: `upscale_x` (2.0), `upscale_method`
        ("bicubic"), `upscale_antialias`, `upscale_denoising_strength` (0.7), `sampler_name_hires`, `sampler_opt_hires` (default:
        the first pass's), `hires_latents` ([1, 4, H/8, W/8] unit noise of the second pass; default: drawn from `generator` after
        the first pass's draws) and `region_map_state_hires` (default: `region_map_state`; None: no region condition in the second
        pass).  On a batcher built with `t2i_adapter=True`: `image_t2i_adapter` (a [1, 3, H, W] tensor in [0, 1] of this
        batcher's size or a PIL image; a list with one per adapter when pipe.adapter is a MultiAdapter), `adapter_conditioning_scale`
        (default 1.0; a list for a MultiAdapter) and `adapter_conditioning_factor` (in [0, 1], default 1.0: the fraction of the
        request's steps that carry the control) - the pipeline methods' own keys; not with `upscale`.  On a batcher built with
        `controlnet=True`: `control_img` (a PIL image or a [1, 3, H, W] tensor in [0, 1]; a list with one per net when
        pipe.controlnet is a MultiControlNetModel), `controlnet_conditioning_scale` (default 1.0), `control_guidance_start` (0.0)
        and `control_guidance_end` (1.0) (numbers, or lists with one entry per net) - the pipeline methods' own keys; not with
        `upscale` or `mask_image`.  On a batcher built with `inpaint_unet=True` every request carries `image` (pixels, which needs
        a VAE encoder, or [1, 4, h, w] latents together with `masked_image_latents` [1, 4, h, w]) and `mask_image`, optionally
        `strength`; `sampler_name`, v-prediction and `guidance_rescale` combine with them.
        On a batcher built with `previews=True`: `preview_every` (an int k >= 1; absent, None or 0: no
        previews) and `on_preview` (a callable f(step, steps, image)): after every k-th of the request's steps but the last, f
        receives the count of steps applied, the steps of this pass and an np.uint8 [h * scale, w * scale, 3] thumbnail of the
        denoised estimate (preview_lane.py); f runs on the thread that steps the batcher.
        On a batcher built with `encode=True`: `image` / `mask_image` given as pixels (a PIL image, a numpy array or a tensor, of
        this batcher's size) are encoded on the encode lane (encode_lane.py): submit normalises them on the host and makes the
        request's draws, and the request joins the batch once its encode has completed; its result has the bits the inline path
        gives at the same encode batch size.
        On a batcher built with `two_call=True`: `sampler_name` may be one of sampling.TWO_CALL_FAMILY (sample_heun, sample_dpm_2,
        sample_dpm_2_ancestral, sample_dpmpp_2s_ancestral, sample_dpmpp_sde) with `eta` / `s_noise` / `seed` / `generator`;
        `step_noise` then has one row per MODEL CALL (sampling.call_noise_table) and `preview_every` counts sampler steps; not
        with `control_img` / `image_t2i_adapter` / `mask_image`.
        On a batcher built with `text=True`: `prompt` (a string) and optionally `negative_prompt` (absent / None: "") in place of
        `prompt_embeds` / `negative_prompt_embeds` / `text_input_ids` - the default branch of encode_prompt_function (emphasis
        syntax, 77-token chunks up to this batcher's text_len, `BREAK`) runs on the text lane (text_lane.py): submit parses and
        chunks on the host, and the request joins the batch once its encode has completed; `region_map_state` needs nothing else
        (the lane makes the ids); `long_encode` other than 0 and a `clip_skip` other than the batcher's are refused.
        Returns a Future of the final output."""
        self._check_weights()
        r = self._prepare(request)
        with self._lock:
            r.rid = self._next_id
            self._next_id += 1
            self._queue.append(r)
            self._wake.notify_all()
        return r.future

    def step(self):
        """advance every active request by one sigma (admitting queued requests into free slots first); False when idle"""
        self._check_weights()
        with self._lock:
            self.exec.bind_thread()
            self._poll()
            ran = self._step_locked()
            self._poll()
            return ran

    def run_until_idle(self):
        """step until the queue is empty and every request has finished, then wait for the last rows and resolve their futures"""
        while self.step():
            pass
        with self._lock:
            self._poll(wait=True)

    def start(self):
        """drive the batcher from a background thread (one per batcher; two batchers on two slots = two batches in flight)"""
        with self._lock:
            if self._thread is not None:
                return self
            self._stop = False
            self._thread = threading.Thread(target=self._drive, name=f"dsc-serve-{self.slot}", daemon=True)
            self._thread.start()
        return self

    def stop(self):
        """stop the driver thread after the step it is in (queued and active requests stay where they are)"""
        with self._lock:
            self._stop = True
            self._wake.notify_all()
            t = self._thread
        if t is not None:
            t.join()
        with self._lock:
            self._thread = None
            self._poll(wait=True)

    def stats(self):
        with self._lock:
            s = dict(self._stats)
            s["captures_after_warm"] = None if self._warm_captures is None else s["captures"] - self._warm_captures
            s["queued"] = len(self._queue)
            s["active"] = sum(r is not None for r in self._slots)
            s["bucket"] = self._n
            return s

    # ------------------------------------------------------------------ request preparation (caller's thread)
    def encode_text(self, prompt, negative_prompt=None):
        """(a batcher built with `text=True`) the embeddings a request with these strings would run with, synchronously, through
        the lane's own path at bucket 1 -> {"prompt_embeds", "negative_prompt_embeds": fp16 [1, S, C] on the GPU, "text_input_ids":
        [negative, positive] id arrays [1, S]}: what `submit` takes in place of the strings, for clients that cache embeddings"""
        if not self.text_on:
            raise ValueError("serve: encode_text needs a batcher built with `text=True` (pipe.serve(..., text=True))")
        holder = _Request(req={"prompt": prompt, "negative_prompt": negative_prompt})
        holder.txt = requests.prompt_request(self, holder.req)
        if holder.txt is None:
            raise ValueError("serve: encode_text takes `prompt` as a string")
        with self._lock:
            self.exec.bind_thread()
            self._ensure_text()
            self.exec.prepare_text(holder)
            encodes, groups = self.exec.dispatch_texts([holder], batch=1)
            self._stats["text_encodes"] += encodes
            self._stats["text_groups"] += groups
            self.exec.text_wait(holder)
        return {"prompt_embeds": holder.text[1], "negative_prompt_embeds": holder.text[0], "text_input_ids": holder.txt.np_ids}

    def _prepare(self, request, second=False, device=True, text_from=None):
        """validate a request (requests.py) and build its record; `second`: the record of a hires request's second pass on
        this batcher (its start latent comes from the hand-off); `device=False` leaves the device half (_prepare_device) to the
        caller; `text_from`: the first-pass record of a hires pair whose text rows and ids this second pass shares (text lane)"""
        pipe = self.pipe
        if not isinstance(request, dict):
            raise TypeError("serve: a request is a dict (txt2img_coalesced's request + num_inference_steps / sampler_opt / "
                            "guidance_scale)")
        requests.check_ip_current(self)
        requests.check_freeu_off(self.pipe)
        freeu = requests.freeu_request(self, request)
        adapter = requests.adapter_request(self, request)
        control = requests.control_request(self, request, second)
        if request.get("upscale") and not second:
            return self._prepare_hires_pair(request)
        out_type, v_pred, family, phi, g = requests.common_request(self, request)
        ip_masks = requests.ip_masks_of(self, request)
        ip_embeds, ip_scale = requests.ip_request(self, request)
        # masks without an image prompt (or with every scale 0) have nothing to weigh: accepted and ignored
        ip_weights = requests.ip_mask_weights(self, ip_masks) if ip_embeds is not None and ip_masks is not None else None
        txt, shared = None, None if text_from is None else text_from.txt
        if shared is None and self.text_on:
            txt = requests.prompt_request(self, request)
        # (a prompt request's rows are allocated by the device half; a shared second pass receives its first pass's)
        text = requests.text_request(self, request) if txt is None and shared is None else None
        every, on_preview = requests.preview_request(self, request)
        steps = int(request.get("num_inference_steps", 25))
        if steps < 1:
            raise ValueError("serve: num_inference_steps must be >= 1")
        r = _Request(req=request, future=concurrent.futures.Future(), steps=steps, second=second, ip_embeds=ip_embeds,
                     ip_scale=ip_scale, ip_weights=ip_weights, adapter=adapter, control=control, guidance=g, output_type=out_type,
                     family=family, rescale=phi, eta=float(request.get("eta", 1.0)), text=text, freeu=freeu, txt=txt)
        t_start = requests.image_request(self, r)
        if self.encode:                              # its rows on the encode lane; None: the request does not touch it
            roles = encode_roles(self, r)
            r.enc = _EncodeHandle(roles) if roles else None
        dev, dt = self.exec.device, self.exec.dtype
        r.sig_dev = pipe._schedule(r.steps, request.get("sampler_opt") or {}, dev, dt)      # txt2img's schedule, fp16-rounded
        sig = getattr(r.sig_dev, "_dsc_host", None)
        r.sig = sig if sig is not None else r.sig_dev.detach().float().cpu().tolist()
        if t_start:                                                  # img2img / inpaiting keep the schedule's tail (:637-647)
            r.sig, r.sig_dev = r.sig[t_start:], r.sig_dev[t_start:]
        if r.adapter is not None:
            # the window: what the pipeline method of this kind of request passes to _adapter_hook as `steps_denoising` is the
            # length of the sigma schedule the sampler walks, final sigma included - len(sigmas) for txt2img
            # (model_k_diffusion.py:530), len(sigma_sched) = len(sigmas[t_start:]) for img2img (:839), len(sigmas) after the
            # `sigmas[t_start:]` of :940 for inpainting (:994) - and r.sig is that schedule for all three.  Every sampler served
            # here makes one model call per step at a distinct sigma, so the hook's count of distinct sigmas seen is the step index
            r.adapter_limit = int(len(r.sig) * r.adapter["factor"])
            if r.adapter_limit < 1:
                r.adapter = None                                     # no model call carries it: no adapter forward, no rows
        if r.control is not None:
            # the step count the pipeline method of this kind of request hands preprocess_controlnet: num_inference_steps in
            # txt2img (model_k_diffusion.py:527), len(sigma_sched) - the truncated schedule, final sigma included - in img2img
            # (:838).  Every served sampler makes one model call per step at a distinct sigma, so _controlnet_hook's count of
            # distinct sigmas seen is the call index
            n_keep = r.steps if r.kind == "txt2img" else len(r.sig)
            r.cgates = self.control_gates(n_keep, len(r.sig) - 1, r.control["scale"], r.control["start"], r.control["end"])
            if all(g == 0.0 for call in r.cgates for g in call):
                r.control, r.cgates = None, None                     # no model call carries it: no lane, no embedding
        # one entry per MODEL CALL from here on (r.i: the index of the model call that runs now).  needs_linear: with a rescale (or
        # a v-prediction model) DPM++ 2M needs the linear family's launch, its (1, -sigma) spelled out like any other member's
        try:
            r.plan = step_plan(pipe.k_diffusion_model, family, r.sig, dt, eta=r.eta, s_noise=float(request.get("s_noise", 1.0)),
                               solver_type=request.get("solver_type"), needs_linear=v_pred or phi > 0.0)
        except ValueError as e:
            raise ValueError(f"serve: {e}") from None
        r.sig = [call.sigma for call in r.plan] + [0.0]
        table = request.get("step_noise")
        if table is not None:
            want = (len(r.plan), 1, 4, self.height // 8, self.width // 8)
            if not torch.is_tensor(table) or tuple(table.shape) != want:
                raise ValueError(f"serve: `step_noise` must be a {list(want)} tensor (one unit-noise row per step), got "
                                 f"{list(table.shape) if torch.is_tensor(table) else type(table).__name__}")
        ids = request.get("text_input_ids") or [None, None]
        if txt is not None or shared is not None:    # a prompt request: the lane's parser made the ids of both texts
            ids = (txt or shared).np_ids
        tabs = encode_region_map(pipe, request.get("region_map_state"), width=self.width, height=self.height,
                                 num_images_per_prompt=1, text_ids=ids)
        r.tables = self._request_tables(tabs)
        if not self._tables_fit([r]):
            raise ValueError(f"serve: the request's region tables (with the zero row of an idle slot) hold more than "
                             f"{ops.MAX_REGION_ROWS} distinct rows at some level; run it through txt2img")
        r.t_submit = time.perf_counter()
        if device:
            self._prepare_device(r)
        if every:                                    # (last: a request refused above leaves nothing behind)
            from .preview_lane import _PreviewState
            self._preview_of[r] = _PreviewState(every, on_preview)
        return r

    def _adapter_gates(self, n, members):
        """the gate vector of bucket n for the model call about to run: 1.0 at rows {i, n + i} of a member whose call index
        (r.i, counted in its own schedule) is inside its adapter window, 0.0 for every other row"""
        gates = [0.0] * (2 * n)
        for i, r in enumerate(members):
            if r is not None and r.adapter is not None and r.i < r.adapter_limit:
                gates[i] = gates[n + i] = 1.0
        return gates

    @staticmethod
    def _freeu_table(n, members):
        """the FreeU table of bucket n, [2 n][4]: a member's (s1, s2, b1, b2) at rows {i, n + i}; ones (the launches leave such a
        row as it is) for idle slots and members without `freeu`"""
        table = [[1.0] * 4 for _ in range(2 * n)]
        for i, r in enumerate(members):
            if r is not None and r.freeu is not None:
                table[i] = table[n + i] = list(r.freeu)
        return table

    @staticmethod
    def control_keep(n_steps, starts, ends):
        """preprocess_controlnet's keep schedule (reference :417-424) for one start / end per net: [n_steps][nets] of 1.0 / 0.0"""
        return [[1.0 - float(i / n_steps < s or (i + 1) / n_steps > e) for s, e in zip(starts, ends)] for i in range(n_steps)]

    @classmethod
    def control_gates(cls, n_steps, n_calls, scales, starts, ends):
        """the gates of a request's model calls, [n_calls][nets]: call k carries `scale * keep[min(k, len(keep) - 1)]` per net -
        _controlnet_hook's `schedule`, python floats, unrounded (the reference multiplies the residuals by that float)"""
        keep = cls.control_keep(n_steps, starts, ends)
        return [[s * k for s, k in zip(scales, keep[min(call, len(keep) - 1)])] for call in range(n_calls)]

    def _control_vectors(self, n, members):
        """(dst, gather, gates) of bucket n for the model call about to run.  Lane j is ControlNet rows j (unconditional) and
        c + j (conditional); held by the member in slot i it maps to batch rows i and n + i: dst [2 c] (idle: -1), gather [2 c]
        (the rows of the bucket's input the lane rows are read from; idle: row 0, whose values are computed and never used),
        gates [nets][2 c] (the member's gates of the call its own schedule is at: r.i; idle: 0)"""
        c, nets = self.control_slots, len(self._control_nets())
        dst, gather, gates = [-1] * (2 * c), [0] * (2 * c), [[0.0] * (2 * c) for _ in range(nets)]
        for i, r in enumerate(members):
            if r is None or r.control is None:
                continue
            j = r.lane
            assert j is not None and self._lanes[j] is r, f"serve: slot {i}'s request holds no lane"
            dst[j], dst[c + j] = gather[j], gather[c + j] = i, n + i
            if r.i < len(r.cgates):
                for a in range(nets):
                    gates[a][j] = gates[a][c + j] = float(r.cgates[r.i][a])
        active = [d for d in dst if d >= 0]
        # the scatter-add's invariant (ops.scatter_add_rows): no two active lane rows name one batch row
        assert len(set(active)) == len(active) and all(d < 2 * n for d in active), f"serve: lane rows share a batch row: {dst}"
        return dst, gather, gates

    def _prepare_device(self, r):
        """the device half of _prepare, in the order the pipeline's one generator is consumed: start latent, then step noise"""
        if r.second:
            self.exec.prepare_hires(r)
        elif r.kind == "txt2img":
            self.exec.prepare(r)
        elif self.encode and r.enc is not None:
            self.exec.prepare_encode(r)              # host pixels and draws only: the lane encodes it beside the step
        else:
            self.exec.prepare_image(r)
        if r.plan.noisy:
            self.exec.prepare_noise(r, r.eta)

    def _prepare_hires_pair(self, request):
        """a request with `upscale=True`: both passes validated first, then prepared (first pass, then second: the order in which
        txt2img / img2img and _hires_pass draw from the request's generator) -> the first-pass record, its `.hires` the second's"""
        first, second = requests.hires_request(self, request)
        hi = self._hires
        r = self._prepare(first, device=False)
        r2 = None
        try:
            r2 = hi._prepare(second, second=True, device=False, text_from=r)
            r2.future, r2.t_submit = r.future, r.t_submit
            r.hires = r2
            self._prepare_device(r)
            if r.txt is not None:
                r2.text = r.text                     # one encode serves both passes
            hi._prepare_device(r2)
        except BaseException:                        # (a refused request leaves no preview state behind)
            self._preview_of.pop(r, None)
            hi._preview_of.pop(r2, None)
            raise
        if r in self._preview_of:                    # (its future also waits for the first pass's queued previews, _poll)
            hi._preview_of[r2].first = self._preview_of[r]
        return r


    def levels(self):
        """{L: S} of the region tables at this image size (one level per down block, encode_region_map_function.py)"""
        out = {}
        sr = 8
        for _ in self.pipe.unet.down_blocks:
            w_r, h_r = -(-self.width // sr), -(-self.height // sr)
            out[w_r * h_r] = self.text_len
            sr *= 2
        return out

    def _request_tables(self, tabs):
        lv = self.levels()
        if getattr(self.pipe, "v_prediction", False) and not self.pipe.k_diffusion_model.pass_kwargs:
            tabs = None                                             # CompVisVDenoiser.get_v drops the region prompt
        if not isinstance(tabs, dict) or not tabs:                  # no masks: the region path with zero tables (quirk q2)
            return {L: torch.zeros(2, L, S) for L, S in lv.items()}
        if sorted(tabs) != sorted(lv) or any(tuple(w.shape) != (2, L, lv[L]) for L, w in tabs.items()):
            raise ValueError("serve: the request's region tables do not match this batcher's image size / text length")
        return {L: w.float().cpu() for L, w in tabs.items()}

    # ------------------------------------------------------------------ scheduling (host)
    def _bucket_for(self, top):
        return next(b for b in self.buckets if b > top)

    def _tables_fit(self, members):
        """the union of these requests' table rows compresses at every level (<= 32 distinct rows, zero rows of IDLE slots in)"""
        for L in self.levels():
            rows = [r.tables[L].reshape(-1, r.tables[L].shape[-1]) for r in members]
            rows.append(torch.zeros(1, self.text_len))
            if ops.compress_region_table(torch.cat(rows)[None]) is None:
                return False
        return True

    @staticmethod
    def _launch_compatible(head, members):
        """One launch serves every stepping slot of a transition, and the known-region launch (inpainting) carries DPM++ 2M /
        eps-prediction records only: it has no c_skip / c_out / noise fields.  So an inpainting request and a request of another
        sampler never share a batch - whichever comes second waits at the head of the queue (FIFO) until the others have left."""
        if head.kind == "inpaint":
            return not any(r.plan.linear for r in members)
        if head.plan.linear:
            return all(r.kind != "inpaint" for r in members)
        return True

    def _step_locked(self):
        """one step, as phases in the order the device sees them: (encode) send queued pixel inputs to the lane, admit, build the
        records, ensure the next bucket and load the joins, ONE transition launch, (previews) the launch for the slots that are
        due, let the finished leave, advance, refresh / upload / run the next bucket, flush decodes"""
        slots = self._slots
        stepping = [r for r in slots if r is not None and r.i < len(r.plan) and self._n is not None]
        if self.encode:
            self._dispatch_encodes()
        if self.text_on:
            self._dispatch_texts()
        joins = self._admit()
        if not stepping and not joins and self._queue and (self.encode or self.text_on):
            # nothing steps and the head is still encoding: wait for its event(s) instead of reporting idle with a request queued
            head = self._queue[0]
            on_encode = self.encode and head.enc is not None
            on_text = self.text_on and head.txt is not None
            if on_encode:
                self.exec.encode_wait(head)
            if on_text:
                self.exec.text_wait(head)
            if on_encode or on_text:
                joins = self._admit()
        if not stepping and not joins:
            return False
        # who leaves after this transition: a request whose last step is the one being applied now
        leaving = [r for r in stepping if r.i + 1 == len(r.plan)]
        staying = [r for r in slots if r is not None and r not in leaving]
        n_src = self._n or 0
        n_dst = self._bucket_for(max(r.slot for r in staying)) if staying else None
        nd = n_dst if n_dst is not None else self.buckets[0]
        recs, known = self._records(max(n_src, nd), stepping, joins, leaving)
        self._load_joins(n_dst, joins)
        if self.inpaint:
            self._transition_cat(n_src, nd, recs)
        else:
            self._transition(n_src, nd, recs, known)
        if self.previews:
            self._preview(stepping, leaving)         # reads `old` of the step just applied, before the next transition
        self._leave(leaving)
        for r in stepping:
            r.i += 1
        if n_dst is not None:
            self._run_bucket(n_dst)
        self._n = n_dst
        if self.decode and any(r.output_type != "latent" for r in leaving):
            # after the next step is queued: the lane's stream waits on the clones' events only, so the decode runs beside it
            self._ensure_decode()
            decodes, rows = self.exec.flush_decodes()
            self._stats["decodes"] += decodes
            self._stats["decode_rows"] += rows
        return True

    def _admit(self):
        """admissions: FIFO, lowest free slot, while the union of the tables still compresses -> the requests that join"""
        slots, joins = self._slots, []
        while self._queue:
            free = next((i for i, r in enumerate(slots) if r is None), None)
            if free is None:
                break
            head = self._queue[0]
            if not self._tables_fit([r for r in slots if r is not None] + [head]):
                break
            if not self._launch_compatible(head, [r for r in slots if r is not None]):
                break
            if self.encode and head.enc is not None and not self.exec.encode_ready(head):
                break                                # still encoding: it waits although a slot is free, and nobody overtakes it
            if self.text_on and head.txt is not None and not self.exec.text_ready(head):
                break                                # its prompt is still on the text lane: the same rule
            if head.control is not None:
                # a ControlNet lane, the lowest free one, kept until the request leaves; with none free the request waits at the
                # head of the queue although a slot is free (FIFO, the rule of _launch_compatible)
                lane = next((j for j, holder in enumerate(self._lanes) if holder is None), None)
                if lane is None:
                    break
                head.lane = lane
                self._lanes[lane] = head
            self._queue.popleft()
            head.slot, head.i = free, 0
            slots[free] = head
            joins.append(head)
        return joins

    def _dispatch_encodes(self):
        """queued requests whose pixel inputs have not been sent to the encode lane go there now, in FIFO order"""
        todo = [r for r in self._queue if r.enc is not None and r.enc.sent < r.enc.rows]
        if todo:
            self._ensure_encode()
            encodes, rows = self.exec.dispatch_encodes(todo)
            self._stats["encodes"] += encodes
            self._stats["encode_rows"] += rows

    def _dispatch_texts(self):
        """queued prompt requests whose groups have not been sent to the text lane go there now, in FIFO order"""
        todo = [r for r in self._queue if r.txt is not None and r.txt.sent < r.txt.real]
        if todo:
            self._ensure_text()
            encodes, groups = self.exec.dispatch_texts(todo)
            self._stats["text_encodes"] += encodes
            self._stats["text_groups"] += groups

    def _records(self, n_slots, stepping, joins, leaving):
        """the per-slot records of this transition's launch and, per slot, the known-region record of an inpainting slot that
        steps (None for every other slot)"""
        slots, recs = self._slots, []
        for i in range(n_slots):
            r = slots[i] if i < len(slots) else None
            if r is not None and r in stepping:
                call = r.plan[r.i]
                noise = self.exec.noise_row(r, r.i) if r.plan.linear and call.s != 0.0 else None
                if r in leaving:
                    j, after = None, (0.0, 0.0, 1.0, None)
                else:
                    j = r.i + 1
                    after = (r.plan[j].c_in, r.plan[j].t, max(r.plan[j].sigma, 1e-10), self.exec.temb_row(r, j))
                rec = step_record(r.plan, call, r.guidance, r.rescale, noise, *after)
                rec.update(req=r, step=r.i, next_step=j)
            elif r is not None and r in joins:
                rec = {"mode": ops.ROW_JOIN, "c_in_next": r.plan[0].c_in, "t_next": r.plan[0].t, "sigma_next": r.sig[0],
                       "temb_row": self.exec.temb_row(r, 0), "req": r, "step": None, "next_step": 0}
            else:
                rec = {"mode": ops.ROW_IDLE, "t_next": 0.0, "sigma_next": 1.0, "temb_row": None, "req": None}
            recs.append(rec)
        # known region of inpainting slots that step now: the model call of request step k >= 1 saw a blended input, and the
        # coming call is blended unless the request leaves (a JOIN is a request's first call: never blended)
        known = [None] * n_slots
        for i, rec in enumerate(recs):
            r = rec["req"]
            if rec["mode"] == ops.ROW_STEP and r.known is not None:
                known[i] = dict(r.known, blend_now=r.i >= 1, blend_next=r not in leaving)
        return recs, known

    def _load_joins(self, n_dst, joins):
        if n_dst is not None:
            self._ensure(n_dst)
        for r in joins:
            self.exec.load_latent(r)
            if r.control is not None:
                self.exec.load_lane(r)               # its text rows and conditioning embedding(s) into the lane's rows
        self._stats["joins"] += len(joins)

    def _transition(self, n_src, n_dst, recs, known):
        """the ONE launch of this step; executor.step_launch names it from the records"""
        kind = step_launch(recs, known)
        if kind == "known" and step_launch(recs) in ("linear", "staged"):
            raise RuntimeError("serve: an inpainting slot and a slot of another sampler step together (admission check bypassed)")
        if kind == "known":
            self.exec.transition(n_src, n_dst, recs, known)
        else:                                        # (no inpainting slot steps: an executor without known regions serves it)
            self.exec.transition(n_src, n_dst, recs)
        if kind == "linear":                         # a slot steps another sampler / a v-prediction model / with a rescale
            self._stats["linear_transitions"] += 1
        if kind == "staged":                         # a slot is inside a two-call sampler's step
            self._stats["staged_transitions"] += 1

    def _transition_cat(self, n_src, n_dst, recs):
        """the ONE launch of a step on a batcher built with `inpaint_unet=True`: always dsc_cfg_linear_step_rows_cat, with one
        entry of extra input channels per slot - a member's row (its mask and masked-image latents), None for an idle slot"""
        extras = [None if rec["req"] is None else rec["req"].extra for rec in recs]
        self.exec.transition(n_src, n_dst, recs, extras=extras)
        self._stats["cat_transitions"] += 1

    def _preview(self, stepping, leaving):
        """the slots whose request is due a preview after the step just applied (every preview_every-th of its steps, never its
        last) go to ONE launch; with no free ring entry it is skipped and counted - the step does not wait"""
        asked = self._preview_of

        def done(r):                                 # sampler steps applied once this transition has run, or None inside a step
            return r.plan[r.i].step + 1 if r.plan[r.i].ends_step else None

        due = [r for r in stepping if r in asked and done(r) and done(r) % asked[r].every == 0 and r not in leaving]
        if not due:
            return
        self.exec.ensure_preview()
        h = self.exec.preview([r.slot for r in due])
        if h is None:
            self._stats["previews_dropped"] += 1
            return
        for r in due:
            asked[r].out += 1
        self._preview_queue.append((h, [(asked[r], done(r), r.plan[-1].step + 1) for r in due]))
        self._stats["previews"] += 1
        self._stats["preview_rows"] += len(due)

    def _deliver_previews(self, wait=False):
        """completed previews to their callbacks, oldest first (one request's previews arrive in step order): the row is copied
        out of the pinned buffer, then `on_preview(step, steps, image)` runs here; what it raises is counted, never passed on"""
        while self._preview_queue and (wait or self.exec.preview_ready(self._preview_queue[0][0])):
            h, rows = self._preview_queue.popleft()
            for j, (state, step, steps) in enumerate(rows):
                image = self.exec.preview_image(h, j)
                state.out -= 1
                try:
                    state.call(step, steps, image)
                except Exception:                    # noqa: BLE001 - a client's callback must not disturb the batch
                    self._stats["preview_callback_errors"] += 1

    def _leave(self, leaving):
        """hand-off / finish of the requests whose last step was just applied, and the release of what they held"""
        for r in leaving:
            self._slots[r.slot] = None
            if r.hires is not None:
                self._hand_off(r)
            elif self.decode and r.output_type != "latent":
                self._done.append((r, self.exec.finish_image(r)))       # the row is cloned now and goes to the lane below
            else:
                self._done.append((r, self.exec.finish(r)))
            r.hnoise = None                          # (a second-pass record: its start noise was read before it joined)
            r.known = None                           # its image / noise / mask rows go back to the allocator (stream-ordered)
            r.extra = None                           # ... and its mask + masked-image latents row (inpaint_unet)
            r.noise = None                           # ... and its noise table
            r.enc = None                             # ... and its draws and host pixels (encode)
            r.txt = None                             # ... and its pinned ids and multipliers (text)
            r.adapter_feats = None                   # ... and its adapter features
            if r.lane is not None:                   # ... and its ControlNet lane goes to whoever waits for one
                self._lanes[r.lane] = None
                r.lane, r.cemb = None, None
            self._stats["leaves"] += 1

    def _run_bucket(self, n_dst):
        """bucket n_dst's static buffers brought up to date for the model call about to run (each only when it changed), then
        the ControlNet graph when some gate is open, then the bucket's step"""
        slots = self._slots
        rows = [slots[i] if i < len(slots) else None for i in range(n_dst)]      # (a bucket may exceed max_batch)
        members = tuple(None if r is None else r.rid for r in rows)
        if self._members.get(n_dst) != members:
            self.exec.refresh(n_dst, rows)
            self._members[n_dst] = members
            self._stats["refreshes"] += 1
        if self._n is not None and n_dst != self._n:
            self._stats["bucket_switches"] += 1
        if self.t2i:
            # (after r.i moved on: r.i is the index of the model call that runs now.)  Only a changed vector is uploaded, and
            # a window that closes changes nothing else: no text, K/V or table work
            gates = self._adapter_gates(n_dst, rows)
            if self._gates.get(n_dst, [0.0] * (2 * n_dst)) != gates:
                self.exec.set_adapter_gates(n_dst, gates)
                self._gates[n_dst] = gates
                self._stats["adapter_gate_updates"] += 1
        if self.freeu:
            # the values are a member's for its whole stay: the table changes with the membership only
            table = self._freeu_table(n_dst, rows)
            if self._freeu_rows.get(n_dst, [[1.0] * 4] * (2 * n_dst)) != table:
                self.exec.set_freeu(n_dst, table)
                self._freeu_rows[n_dst] = table
                self._stats["freeu_updates"] += 1
        if self.cn:
            # (after r.i moved on, as above.)  Each of the three is uploaded only when it differs from what the bucket holds;
            # the ControlNet itself runs only when some member's gate is open in the coming call
            dst, gather, gates = self._control_vectors(n_dst, rows)
            was = self._cstate.get(n_dst, ([-1] * len(dst), [0] * len(gather), [[0.0] * len(dst) for _ in gates]))
            if (dst, gather, gates) != was:
                self.exec.set_control(n_dst, dst if dst != was[0] else None, gather if gather != was[1] else None,
                                      gates if gates != was[2] else None)
                self._cstate[n_dst] = (dst, gather, gates)
                if gates != was[2]:
                    self._stats["control_gate_updates"] += 1
            if any(g != 0.0 for per in gates for g in per):
                self.exec.run_control(n_dst)
                self._stats["control_steps"] += 1
        self.exec.run(n_dst)
        self._stats["steps"] += 1

    def _hand_off(self, r):
        """r leaves this batcher for its hires pass: the resample + noise launch on this batcher's stream, then the second-pass
        record joins the chained batcher's queue (the only place one batcher takes another's lock)"""
        hi, r2 = self._hires, r.hires
        self._preview_of.pop(r, None)                # (its queued previews keep their state; the second pass's future waits for them)
        r2.ready = self.exec.hand_off(r, r2)
        r2.t_handoff = time.perf_counter()
        r.future.dsc_first_pass_s = r2.t_handoff - r.t_submit    # submit -> handed off (host clock), for measurement tools
        r.hires = None
        self._stats["handoffs"] += 1
        with hi._lock:
            r2.rid = hi._next_id
            hi._next_id += 1
            hi._queue.append(r2)
            hi._wake.notify_all()

    def _ensure(self, n):
        if self.cn:
            self._ensure_control()
        if self.exec.ensure(n):
            self._stats["captures"] += 1

    def _ensure_control(self):
        if self.exec.ensure_control():
            self._stats["captures"] += 1

    def _ensure_decode(self):
        self._stats["captures"] += self.exec.ensure_decode()

    def _ensure_encode(self):
        self._stats["captures"] += self.exec.ensure_encode()

    def _ensure_text(self):
        self._stats["captures"] += self.exec.ensure_text()

    def _poll(self, wait=False):
        """resolve the futures of requests whose final row copy has completed (in completion order); on a previews batcher the
        completed previews are delivered first, and a future is held back while previews of its request are still queued (of a
        hires request's second pass: of its first pass too, which the other batcher's poll delivers)"""
        if self.previews:
            self._deliver_previews(wait)
        keep = []
        for r, h in self._done:
            state = self._preview_of.get(r) if self.previews else None
            held = state is not None and (state.out > 0 or (state.first is not None and state.first.out > 0 and not wait))
            if not held and (wait or self.exec.ready(h)):
                if state is not None:
                    del self._preview_of[r]
                out = self.exec.result(r, h)
                r.t_done = time.perf_counter()
                r.future.dsc_latency_s = r.t_done - r.t_submit        # submit -> resolved, for measurement tools
                if not r.future.done():
                    r.future.set_result(out)
            else:
                keep.append((r, h))
        self._done = keep

    def _drive(self):
        self.exec.bind_thread()
        while True:
            with self._lock:
                if self._stop:
                    return
                self._poll()
                if self._step_locked():
                    # bound how far the host runs ahead of the GPU (a join lands within a few steps, not after every
                    # step already queued): wait for the step before last, never for the one just queued
                    self.exec.throttle()
                elif self._done or self._preview_queue:
                    self._wake.wait(0.0005)              # rows in flight: look again soon
                else:
                    self._wake.wait()

class HiresPair:
    """Two chained batchers (pipe.serve_hires): `base` at the request's size, `hires` at the target size, with the batcher's own
    public surface.  Requests go to `base`; those with `upscale=True` continue on `hires` (which also takes ordinary requests of
    its size through `pair.hires.submit`)."""

    def __init__(self, base, hires):
        self.base, self.hires = base.chain_hires(hires), hires

    def warm(self):
        self.base.warm()
        self.hires.warm()
        if hasattr(self.base.exec, "warm_hand_off"):
            self.base.exec.warm_hand_off(self.hires.exec)
        return self

    def submit(self, request):
        return self.base.submit(request)

    def step(self):
        """advance both batchers by one step each; False when both are idle"""
        a = self.base.step()
        b = self.hires.step()
        return a or b

    def run_until_idle(self):
        while self.step():
            pass
        self.base.run_until_idle()
        self.hires.run_until_idle()

    def start(self):
        self.base.start()
        self.hires.start()
        return self

    def stop(self):
        self.base.stop()
        self.hires.stop()

    def stats(self):
        b = self.base.stats()
        return {"base": b, "hires": self.hires.stats(), "handoffs": b["handoffs"]}
