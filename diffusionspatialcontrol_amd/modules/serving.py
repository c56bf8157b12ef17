"""Continuous batching for serving: requests join a running batch at any step boundary and leave when done.

`txt2img_coalesced` runs k requests in lockstep (one schedule, one guidance scale, all start together).  Here every request
keeps its own schedule, step count and guidance scale; what the batch shares is one captured UNet step per bucket.

Slots and buckets.  A request takes the lowest free slot i (< max_batch) and keeps it until it finishes.  Slot i is latent row i
of the batcher's x / old buffers and rows {i, n + i} of the UNet input of every bucket n > i ([u_0..u_{n-1}, c_0..c_{n-1}], the
layout of txt2img_coalesced), i.e. std group i (`n_std_groups = n`).  Each step runs the captured graph of the smallest bucket
that covers the highest occupied slot; empty slots below it are IDLE rows (zero input, zero text, zero tables).  Every bucket is
captured once (`warm()`); joins, leaves and bucket switches only refresh static buffers in place (text rows, their packed K/V,
the compressed region tables).

Per step: ONE launch of the per-row sampler step takes the eps of the bucket that just ran and writes the next bucket's input -
per slot its own sigma, guidance, DPM++ 2M coefficients (c = 0 on a request's first step), time-embedding row (of its own
`temb_add_table`) and sigma of its std group (read by the region cross-attention under DSC_FLAG_SIGMA_PER_GROUP) - then the
next bucket's graph replays.  No host<->device synchronisation per step: a request's completion is a CUDA event recorded after
the copy of its final latent row, and futures resolve when those events are seen complete.

Image-conditioned requests.  A request with `image` is img2img (the last `strength` fraction of its schedule, started from
`image_latents + noise * sqrt(sigma_0^2 + 1)`, the pipeline method's line); with `mask_image` too it is inpainting on the 4-channel
UNet: its image latents, noise and mask rows stay on the device while it runs, and the per-row step blends the known region into
the model input of every model call after its first (dsc_cfg_dpmpp2m_step_rows_known, what `inpaiting`'s eager hook does per
call).  That launch replaces the plain one only for transitions in which an inpainting slot steps.

Samplers and parameterisation.  A request names its sampler (`sampler_name`: one of sampling.LINEAR_FAMILY - Euler, Euler a,
DPM++ 2M (default), DPM++ 2M SDE, LCM - by name or as the callable) with `eta` / `s_noise` / `solver_type`; the noise of all its
steps is one table on the device from submit until it leaves (`step_noise`, or sampling.step_noise_table from `seed` /
`generator`), and its record for step j points at row j.  A transition in which every stepping slot is DPM++ 2M on an
eps-prediction model launches dsc_cfg_dpmpp2m_step_rows as before; any other launches dsc_cfg_linear_step_rows for all slots
(DPM++ 2M slots ride in it with the same bits).  On a v-prediction pipeline every slot carries CompVisVDenoiser's scalars (and,
with `pass_kwargs = False`, zero region tables: the reference's v-prediction path never sees the region prompt).  The
known-region launch of inpainting carries DPM++ 2M records only, so an inpainting request and a request of another sampler never
share a batch: the later one waits in the queue until the others have left.

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

Image prompts.  On a pipeline with IP-Adapters loaded (load_ip_adapter) the batcher's step carries, per cross-attention layer and
adapter, to_k_ip / to_v_ip of every batch row's image tokens and one scale per row: a request with `ip_adapter_image_embeds` has
its image tokens projected (unet.encoder_hid_proj) and pushed through every layer's to_k_ip / to_v_ip ONCE, at admission, into
a flat row pair; `refresh` copies a member's pair into rows {i, n + i} of the bucket's static buffer (one per adapter; each
layer's k_ip / v_ip are views into it) and writes its `ip_adapter_scale` into the bucket's row_scale vector.  In the captured
step every IP-Adapter processor runs the stock text branch and then ONE launch per adapter of dsc_ip_xattn_add_f16, which reads
row_scale on the device: idle slots and requests without an image prompt carry scale 0, their workgroups return at once and
their rows are bit for bit those of a batcher without an adapter; joins, leaves and a changed scale need no capture.  The
sampler launches do not know about any of it, so every request kind, sampler and guidance rescale combines with an image prompt.

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

T2I-Adapter.  A batcher built with `t2i_adapter=True` on a pipeline with an adapter (setup_model_t2i_adapter) takes the pipeline's
own `image_t2i_adapter` / `adapter_conditioning_scale` / `adapter_conditioning_factor`.  The adapter network runs ONCE per
request, at admission (preprocessing_t2i_adapter's line for one image, without the CFG duplication: features times scale in
fp16), and the request holds its four feature maps until it leaves.  Every bucket owns one static feature buffer
[n, C_k, h_k, w_k] per down block and one fp32 gate vector [2 n]; the captured step hands both to the UNet as
`down_intrablock_gated`, which adds `gate[r] * feats[k][r % n]` where the reference adds its residuals
(u_net_condition_modify.py:1194-1230), one launch of dsc_add_rows_gated_f16 per down block.  `refresh` copies a member's
features into its slot row on a membership change; the gate of rows {i, n + i} is 1 while the member's model call k (counted in
its own schedule) satisfies k < int(steps_denoising * factor) - _adapter_hook's window - and 0 otherwise, for idle slots and
for members without a control image: those rows keep their bits and their feature rows are never read.  The gate vector is
uploaded only when it changes; a window that closes costs that one small copy and no refresh.  The sampler launches do not know
about any of it.  A batcher built without the flag captures the step it captured before and refuses the key.

ControlNet.  A batcher built with `controlnet=True, control_slots=c` on a pipeline with a ControlNet (setup_controlnet) takes the
pipeline's own `control_img` / `controlnet_conditioning_scale` / `control_guidance_start` / `control_guidance_end`.  The ControlNet
does not run over the batch: a request with a control image takes the lowest free of c LANES at admission (lane j = rows j and
c + j of the ControlNet's own batch) and keeps it until it leaves; with none free it waits at the head of the queue (FIFO).  One
captured ControlNet graph per batcher reads static lane buffers (x, t, the text rows, one conditioning embedding per net - computed
once per request at admission) and writes every zero convolution's UNSCALED output into static buffers.  Every bucket owns a dst
vector [2 c] (the lane of the member in slot i -> batch rows i and n + i; idle: -1), a gather vector and an fp32 gate matrix
[nets, 2 c]; its captured step hands them to the UNet as `down_block_scattered`, one launch of dsc_scatter_add_rows_f16 per skip
tensor and one for the mid block's output, where the reference adds its residuals (u_net_condition_modify.py:1236-1245, 1269-1270).
Per model call with an open gate: the lane rows of the bucket's input and timesteps are gathered, the ControlNet graph replays,
then the bucket's graph; with no gate open the ControlNet is skipped.  The gate of a request's model call k is
`scale * keep[min(k, len(keep) - 1)]` (preprocess_controlnet's keep for the step count the pipeline method passes); all gates 0 is a
plain request (no lane).  A batcher built without the flag captures the step it captured before and refuses the key.

Finished images.  A batcher built with `decode=True, decode_batch=d` on a pipeline with a VAE decoder hands out images without
stopping the step for them.  A request whose `output_type` is "pil", "np" or "uint8" leaves as before (its final row is cloned on
the batcher's stream); at the end of that transition the cloned rows go, up to d at a time, to the DECODE LANE: a second stream
with, per decode bucket (1, d and the powers of two between), a static input, static uint8 and float32 [m, H, W, 3] outputs and ONE
captured graph - `1 / scaling_factor * z`, `vae.decode`, and dsc_image_finish once per output kind (decode_latents' clamp, NHWC
permute and float conversion, numpy_to_pil's rounding to bytes, on the device).  The lane's stream waits on the clones' events,
copies the rows into the static input (rows of a padded bucket that hold no request are zeros), replays the graph, copies each
request's row of the kind it asked for into a slot of a small ring of pinned host buffers (non-blocking) and records an event.
The lane has no thread: the thread that steps the batcher queues its work, and the poll that resolves latent rows resolves
images too - `ready` queries the lane's event, `result` copies the row out of the pinned slot (which frees it) and, for "pil",
wraps it.  No GPU work, allocation or stream synchronisation happens under the lock after `warm()`; only a full ring makes the
dispatcher wait, for the oldest decode.  "latent" requests never touch the lane, and a batcher built without the flag has no lane,
no second stream and the inline `latent_to_image` path it had ("uint8", which that path does not know, is refused at submit).

The region tables of a batch are compressed to at most 32 distinct rows per level (the prepared-operand kernels' LDS table): a
request whose admission would push the union of the active requests' rows past that waits in the queue (FIFO) until a slot frees.
"""
import collections
import concurrent.futures
import threading
import time

import torch

from .. import _lib, ops
from . import sampling
from .latent_resample import MODES as _RESAMPLE_MODES, device_taps, hires_target_size
from .attention_modify import weight_func_is_default
from .encode_region_map_function import encode_region_map
from .external_k_diffusion import DiscreteVDDPMDenoiser

_EMBED_LOCK = threading.Lock()       # around the process-wide deterministic switch in _GraphExecutor._control_embedding
MAX_TEXT_KEYS = 384                  # the chunked prepared-operand kernels (ops.region_xattn_packed)
_UNSUPPORTED_KEYS = ("control_img", "image_t2i_adapter")
_IMAGE_TYPES = ("pil", "np", "numpy", "uint8")      # what a batcher built with `decode=True` hands out besides "latent"
_DECODE_RING = 4                     # pinned host slots of the decode lane: decodes whose rows have not been collected yet
_FLAG_HINT = {"image_t2i_adapter": "; a batcher built with `t2i_adapter=True` (pipe.serve(..., t2i_adapter=True)) serves it",
             "control_img": "; a batcher built with `controlnet=True` (pipe.serve(..., controlnet=True)) serves it"}


def _ip_layers(pipe):
    """(attention module, its IP-Adapter processor) of every cross-attention layer in module order; [] without an adapter"""
    from .attention_modify import _IPAdapterProcessor
    from .u_net_condition_modify import Attention
    return [(m, m.processor) for m in pipe.unet.modules() if isinstance(m, Attention) and isinstance(m.processor, _IPAdapterProcessor)]


def decode_buckets(decode_batch):
    """the batch sizes the decode lane captures: 1, decode_batch and the powers of two between"""
    out, m = {1, int(decode_batch)}, 2
    while m < decode_batch:
        out.add(m)
        m *= 2
    return tuple(sorted(out))


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


class _Request:
    __slots__ = ("rid", "req", "future", "steps", "sig", "sig_dev", "coeffs", "scal", "guidance", "tables",
                 "slot", "i", "lat", "temb", "text", "output_type", "t_submit", "t_done", "kind", "strength", "known",
                 "family", "snoise", "skipout", "noise", "rescale", "eta", "hires", "second", "ready", "hnoise", "t_handoff",
                 "ip_embeds", "ip_scale", "ip_rows", "ip_weights", "adapter", "adapter_limit", "adapter_feats",
                 "control", "cgates", "lane", "cemb")


class ServingBatcher:
    """See the module docstring.  `executor` is the device side (default: the captured-graph executor on the pipeline's GPU);
    the scheduling here is host logic only."""

    def __init__(self, pipe, height, width, max_batch=8, slot=0, buckets=(1, 2, 4, 8), text_len=77, executor=None, ip_masks=False,
                 t2i_adapter=False, controlnet=False, control_slots=None, decode=False, decode_batch=2):
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
        # requests may ask for images ("pil" / "np" / "uint8"): a decode lane beside the step finishes them (module docstring)
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
        self._warm_captures = None
        self._thread = None
        self._stop = False
        # the IP-Adapters this batcher's step is built for (load_ip_adapter): the processors, the image projection, tokens per adapter
        self._ip = _ip_layers(pipe)
        self._ip_proj = getattr(pipe.unet, "encoder_hid_proj", None) if self._ip else None
        self._ip_tokens = [int(t) for t in self._ip[0][1].num_tokens] if self._ip else []
        if any(t > ops.IP_MAX_TOKENS for t in self._ip_tokens):
            raise ValueError(f"serve: a loaded IP-Adapter has {max(self._ip_tokens)} image tokens; the batcher's image-token attention "
                             f"(dsc_ip_xattn_add_f16) takes at most {ops.IP_MAX_TOKENS} (ops.IP_MAX_TOKENS) - the 257-token Full "
                             f"projection runs through txt2img(ip_adapter_image_embeds=...)")
        # requests may carry `ip_adapter_masks`: the step hands per-query weights to the masked entry (see the module docstring)
        self.ip_masks = bool(ip_masks)
        if self.ip_masks and not self._ip:
            raise ValueError("serve: `ip_masks=True` on a pipeline without an IP-Adapter (pipe.load_ip_adapter first, then build the "
                             "batcher)")
        # requests may carry `image_t2i_adapter`: the step hands the UNet per-slot features and a per-row gate (module docstring)
        self.t2i = bool(t2i_adapter)
        if controlnet and self.t2i:
            raise ValueError("serve: `controlnet=True` and `t2i_adapter=True` are not served together yet (build one batcher for each)")
        self._adapter = getattr(pipe, "adapter", None) if self.t2i else None
        self._adapter_shapes = self._adapter_setup() if self.t2i else None
        # requests may carry `control_img`: a compact ControlNet batch of `control_slots` lanes runs beside the step, and the
        # step scatters its residuals into the rows of the requests that hold a lane (module docstring)
        self.cn = bool(controlnet)
        self._controlnet = getattr(pipe, "controlnet", None) if self.cn else None
        self.control_slots = (self.max_batch if control_slots is None else int(control_slots)) if self.cn else 0
        self._control_shapes = self._controlnet_setup() if self.cn else None
        self._lanes = [None] * self.control_slots     # lane -> the request that holds it
        self._cstate = {}                      # bucket -> (dst, gather, gates) last uploaded for it (absent: as captured)
        self.exec = executor if executor is not None else _GraphExecutor(self)

    def _adapter_setup(self):
        """the adapter against the UNet, at construction -> [(C_k, h_k, w_k)] of the feature each down block adds: as many maps
        as down blocks, the UNet's channels, and the size of the tensor the add lands on.  Both sides are computed from their own
        modules' parameters (the adapter's PixelUnshuffle and pooling, the UNet's stride-2 convolutions), not assumed equal."""
        from .t2i_adapter import MultiAdapter
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
                conv = blk.downsamplers[0].conv
                h, w = ((v + 2 * conv.padding[i] - conv.kernel_size[i]) // conv.stride[i] + 1 for i, v in enumerate((h, w)))
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
        from .controlnet import MultiControlNetModel
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
                h, w = ((v + 2 * conv.padding[i] - conv.kernel_size[i]) // conv.stride[i] + 1 for i, v in enumerate((h, w)))
                shapes.append((int(conv.out_channels), int(h), int(w)))
        return shapes + [(int(model.mid_block.resnets[-1].conv2.out_channels), int(h), int(w))]

    def _controlnet_setup(self):
        """the ControlNet against the UNet, at construction -> [(C, h, w)] of every skip tensor and of the mid block's output,
        the tensors its residuals are added to.  Both sides are computed from their own modules, not assumed equal."""
        from .controlnet import ControlNetModel
        if self._controlnet is None:
            raise ValueError("serve: `controlnet=True` on a pipeline without a ControlNet (pipe.setup_controlnet(controlnet) first, "
                             "then build the batcher)")
        if not 1 <= self.control_slots <= self.max_batch:
            raise ValueError(f"serve: `control_slots` must be in [1, max_batch = {self.max_batch}], got {self.control_slots}")
        nets = self._control_nets()
        from .. import scatter_add
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
    def warm(self):
        """capture every bucket's step now (otherwise each is captured on first use)"""
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
            self._warm_captures = self._stats["captures"]
        return self

    def chain_hires(self, hi):
        """requests with `upscale=True` run their second pass on `hi`, a batcher of the target size on another workspace slot
        (see the module docstring); `hi` keeps serving ordinary requests of its size.  Returns self."""
        if not isinstance(hi, ServingBatcher):
            raise TypeError("serve: chain_hires takes the ServingBatcher of the hires pass")
        if hi is self:
            raise ValueError("serve: a batcher cannot be chained to itself (the hires pass runs at another image size)")
        if hi.slot == self.slot:
            raise ValueError(f"serve: both batchers of a hires pair sit on workspace slot {self.slot}; give the second its own")
        if hi.pipe is not self.pipe:
            raise ValueError("serve: both batchers of a hires pair serve the same pipeline")
        if hi.height < self.height or hi.width < self.width:
            raise ValueError(f"serve: the hires batcher runs {hi.height}x{hi.width}, smaller than this one's "
                             f"{self.height}x{self.width} (only enlarging is served)")
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
        `upscale` or `mask_image`.  Returns a Future of the final output."""
        r = self._prepare(request)
        with self._lock:
            r.rid = self._next_id
            self._next_id += 1
            self._queue.append(r)
            self._wake.notify_all()
        return r.future

    def step(self):
        """advance every active request by one sigma (admitting queued requests into free slots first); False when idle"""
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
    def _prepare(self, request, second=False, device=True):
        """validate a request and build its record; `second`: the record of a hires request's second pass on this batcher (its
        start latent comes from the hand-off); `device=False` leaves the device half (_prepare_device) to the caller"""
        pipe = self.pipe
        if not isinstance(request, dict):
            raise TypeError("serve: a request is a dict (txt2img_coalesced's request + num_inference_steps / sampler_opt / "
                            "guidance_scale)")
        self._check_ip_current()
        adapter = self._adapter_request(request)
        control = self._control_request(request, second)
        if request.get("upscale") and not second:
            return self._prepare_hires_pair(request)
        out_type = request.get("output_type", "latent")
        if self.decode:
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
        if family is None:
            raise ValueError(f"serve: `sampler_name` {getattr(sampler, '__name__', sampler)!r} has no per-row step (supported: "
                             f"{', '.join(sampling.LINEAR_FAMILY)}; use txt2img)")
        if request.get("mask_image") is not None and (family != "dpmpp_2m" or v_pred):
            raise ValueError("serve: `mask_image` (inpainting) runs DPM++ 2M on an eps-prediction model only (the known-region "
                             "step, dsc_cfg_dpmpp2m_step_rows_known); drop `sampler_name` or use inpaiting")
        phi = request.get("guidance_rescale", 0.0)
        if phi is None:
            phi = 0.0
        if isinstance(phi, bool) or not isinstance(phi, (int, float)) or not 0.0 <= phi <= 1.0:      # (NaN fails the range)
            raise ValueError(f"serve: `guidance_rescale` must be a number in [0, 1], got {phi!r}")
        phi = float(phi)
        if request.get("mask_image") is not None and phi > 0.0:
            raise ValueError("serve: `mask_image` (inpainting) with `guidance_rescale` > 0 is not served (the known-region step "
                             "has no rescale); use inpaiting")
        if (request.get("height", self.height), request.get("width", self.width)) != (self.height, self.width):
            raise ValueError(f"serve: this batcher runs {self.height}x{self.width} images, the request asks for "
                             f"{request.get('height')}x{request.get('width')}")
        # dsc_cfg_linear_step_rows and its rescale form move 8 halfs per lane; refused here, before the request can reach a step
        # that other requests share (DPM++ 2M's own per-row step takes the 4 * odd halfs of a latent with both sides odd)
        if (family != "dpmpp_2m" or v_pred or phi > 0.0) and (4 * (self.height // 8) * (self.width // 8)) % 8 != 0:
            raise ValueError(f"serve: this batcher's {self.height // 8}x{self.width // 8} latent has both sides odd; the linear "
                             f"per-row step (every sampler but DPM++ 2M, v-prediction models, `guidance_rescale` > 0) needs a "
                             f"multiple of 8 halfs per latent: drop `sampler_name` / `guidance_rescale`, or use txt2img")
        g = float(request.get("guidance_scale", 7.5))
        if g <= 1.0:
            raise ValueError("serve: guidance_scale must be > 1 (classifier-free guidance rows u_i / c_i)")
        wf = request.get("weight_func")
        if wf is not None and not weight_func_is_default(wf):
            raise ValueError("serve: a custom weight_func is not supported (use txt2img)")
        for k in _UNSUPPORTED_KEYS:
            if request.get(k) is not None and not (self.t2i and k == "image_t2i_adapter") and not (self.cn and k == "control_img"):
                raise ValueError(f"serve: `{k}` (ControlNet / T2I-Adapter) is not supported (use txt2img)" + _FLAG_HINT.get(k, ""))
        if request.get("ip_adapter_image") is not None:
            raise ValueError("serve: `ip_adapter_image` (a raw image) is not supported: encode it once with pipe.encode_image and "
                             "pass `ip_adapter_image_embeds` ([negative; positive] per loaded adapter)")
        ip_masks = self._ip_masks_of(request)
        ip_embeds, ip_scale = self._ip_request(request)
        # masks without an image prompt (or with every scale 0) have nothing to weigh: accepted and ignored
        ip_weights = self._ip_mask_weights(ip_masks) if ip_embeds is not None and ip_masks is not None else None
        pos, neg = request.get("prompt_embeds"), request.get("negative_prompt_embeds")
        if pos is None or neg is None:
            raise ValueError("serve: a request needs prompt_embeds and negative_prompt_embeds ([1, S, ctx] each)")
        if pos.dim() != 3 or pos.shape[0] != 1 or neg.shape != pos.shape:
            raise ValueError("serve: prompt_embeds / negative_prompt_embeds must both be [1, S, ctx]")
        if pos.shape[1] > MAX_TEXT_KEYS:
            raise ValueError(f"serve: {pos.shape[1]} text keys; the batcher's kernels take at most {MAX_TEXT_KEYS} (use txt2img)")
        if pos.shape[1] != self.text_len:
            raise ValueError(f"serve: this batcher runs {self.text_len} text keys, the request has {pos.shape[1]}")
        r = _Request()
        r.req = request
        r.future = concurrent.futures.Future()
        r.steps = int(request.get("num_inference_steps", 25))
        if r.steps < 1:
            raise ValueError("serve: num_inference_steps must be >= 1")
        r.second, r.hires, r.ready, r.hnoise, r.t_handoff = second, None, None, None, None
        r.ip_embeds, r.ip_scale, r.ip_rows, r.ip_weights = ip_embeds, ip_scale, None, ip_weights
        r.adapter, r.adapter_limit, r.adapter_feats = adapter, 0, None
        r.control, r.cgates, r.lane, r.cemb = control, None, None, None
        t_start = self._image_request(r)
        r.guidance = g
        r.output_type = out_type
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
        r.family = family
        r.rescale = phi
        eta = r.eta = float(request.get("eta", 1.0))
        args = {}
        if family in ("euler_ancestral", "dpmpp_2m_sde"):
            args.update(eta=eta, s_noise=float(request.get("s_noise", 1.0)))
        if family == "dpmpp_2m_sde":
            args["solver_type"] = request.get("solver_type") or "midpoint"
            if args["solver_type"] not in ("midpoint", "heun"):
                raise ValueError(f"serve: `solver_type` must be 'midpoint' or 'heun', got {args['solver_type']!r}")
        abcs = sampling.linear_step_coefficients(family, r.sig, **args)
        r.coeffs = [c4[:3] for c4 in abcs]
        r.snoise = [c4[3] for c4 in abcs]
        kdm = pipe.k_diffusion_model
        r.scal = []
        # None: DPM++ 2M's own launch serves the request (c_skip = 1, c_out = -sigma); with a rescale it needs the linear family's
        # launch, so its (1, -sigma) are spelled out like any other member's
        r.skipout = [] if family != "dpmpp_2m" or v_pred or phi > 0.0 else None
        for s_ in r.sig[:len(r.coeffs)]:
            c_in, c_out, t = kdm.step_scalars(s_)
            r.scal.append((c_in, float(t)))
            if r.skipout is not None:
                r.skipout.append((kdm.step_skip(s_), c_out))
        r.noise = None
        table = request.get("step_noise")
        if table is not None:
            want = (len(r.coeffs), 1, 4, self.height // 8, self.width // 8)
            if not torch.is_tensor(table) or tuple(table.shape) != want:
                raise ValueError(f"serve: `step_noise` must be a {list(want)} tensor (one unit-noise row per step), got "
                                 f"{list(table.shape) if torch.is_tensor(table) else type(table).__name__}")
        ids = request.get("text_input_ids") or [None, None]
        tabs = encode_region_map(pipe, request.get("region_map_state"), width=self.width, height=self.height,
                                 num_images_per_prompt=1, text_ids=ids)
        r.tables = self._request_tables(tabs)
        if not self._tables_fit([r]):
            raise ValueError(f"serve: the request's region tables (with the zero row of an idle slot) hold more than "
                             f"{ops.MAX_REGION_ROWS} distinct rows at some level; run it through txt2img")
        r.slot, r.i, r.t_done = None, 0, None
        r.text = (neg, pos)
        r.t_submit = time.perf_counter()
        if device:
            self._prepare_device(r)
        return r

    def _adapter_request(self, request):
        """submit-time checks of the T2I-Adapter keys -> {"image", "scale", "factor"} or None (no control image, or nothing to
        add: every scale 0 / factor 0)"""
        image = request.get("image_t2i_adapter")
        if not self.t2i:
            return None                                              # (the key itself is refused with the other unsupported keys)
        from .t2i_adapter import MultiAdapter
        if getattr(self.pipe, "adapter", None) is not self._adapter:
            raise RuntimeError("serve: the pipeline's T2I-Adapter changed since this batcher was built (setup_model_t2i_adapter): "
                               "build a new one with pipe.serve(..., t2i_adapter=True)")
        multi = isinstance(self._adapter, MultiAdapter)
        n = self._adapter.num_adapter if multi else 1
        scale, factor = request.get("adapter_conditioning_scale", 1.0), request.get("adapter_conditioning_factor", 1.0)
        scale = 1.0 if scale is None else scale
        factor = 1.0 if factor is None else factor

        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and v not in (float("inf"), float("-inf"))

        if isinstance(scale, (list, tuple)):
            if not multi:
                raise ValueError("serve: `adapter_conditioning_scale` is a list, but pipe.adapter is one adapter (a list goes with a "
                                 "MultiAdapter)")
            if len(scale) != n:
                raise ValueError(f"serve: `adapter_conditioning_scale` lists {len(scale)} scales, pipe.adapter holds {n} adapters")
            if not all(number(v) for v in scale):
                raise ValueError(f"serve: `adapter_conditioning_scale` must hold finite numbers, got {list(scale)!r}")
            scale = [float(v) for v in scale]
        elif not number(scale):
            raise ValueError(f"serve: `adapter_conditioning_scale` must be a finite number (or a list of them for a MultiAdapter), "
                             f"got {scale!r}")
        else:
            scale = float(scale)
        if not number(factor) or not 0.0 <= factor <= 1.0:
            raise ValueError(f"serve: `adapter_conditioning_factor` must be a number in [0, 1], got {factor!r}")
        if image is None:
            return None
        if request.get("upscale"):
            raise ValueError("serve: `image_t2i_adapter` with `upscale` (a control image in the hires pass) is not served yet; use "
                             "txt2img")
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        if isinstance(image, (list, tuple)) != multi or len(images) != n:
            raise ValueError(f"serve: `image_t2i_adapter` must be " + (f"a list of {n} images (pipe.adapter is a MultiAdapter)" if multi
                             else "one image (a list goes with a MultiAdapter)") +
                             f", got {f'a list of {len(images)}' if isinstance(image, (list, tuple)) else type(image).__name__}")
        for one in images:
            if torch.is_tensor(one):
                cin = (self._adapter.adapters[0] if multi else self._adapter).config.in_channels
                if one.dim() != 4 or one.shape[0] != 1 or one.shape[1] != cin or not torch.is_floating_point(one) \
                        or tuple(one.shape[-2:]) != (self.height, self.width):
                    raise ValueError(f"serve: `image_t2i_adapter` as a tensor must be a floating-point [1, {cin}, {self.height}, "
                                     f"{self.width}] image in [0, 1] (this batcher's size), got {one.dtype} {list(one.shape)}")
            elif not (hasattr(one, "size") and hasattr(one, "resize") and not hasattr(one, "shape")):
                raise ValueError(f"serve: `image_t2i_adapter` must be a [1, 3, H, W] tensor or a PIL image, got {type(one).__name__}")
        if factor == 0.0 or all(v == 0.0 for v in (scale if isinstance(scale, list) else [scale])):
            return None                                              # nothing to add: no adapter forward, the rows stay skipped
        return {"image": images if multi else images[0], "scale": scale, "factor": float(factor)}

    def _adapter_gates(self, n, members):
        """the gate vector of bucket n for the model call about to run: 1.0 at rows {i, n + i} of a member whose call index
        (r.i, counted in its own schedule) is inside its adapter window, 0.0 for every other row"""
        gates = [0.0] * (2 * n)
        for i, r in enumerate(members):
            if r is not None and r.adapter is not None and r.i < r.adapter_limit:
                gates[i] = gates[n + i] = 1.0
        return gates

    def _control_request(self, request, second=False):
        """submit-time checks of the ControlNet keys -> {"image": [one per net], "scale", "start", "end": one float per net} or
        None (no control image).  Whether any model call carries it is decided once the schedule is known (_prepare)."""
        image = request.get("control_img")
        if not self.cn:
            return None                                              # (the key itself is refused with the other unsupported keys)
        from .controlnet import MultiControlNetModel
        if getattr(self.pipe, "controlnet", None) is not self._controlnet:
            raise RuntimeError("serve: the pipeline's ControlNet changed since this batcher was built (setup_controlnet): build a "
                               "new one with pipe.serve(..., controlnet=True)")
        multi = isinstance(self._controlnet, MultiControlNetModel)
        n = len(self._control_nets())

        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and v not in (float("inf"), float("-inf"))

        per_net = {}
        for key, default in (("controlnet_conditioning_scale", 1.0), ("control_guidance_start", 0.0), ("control_guidance_end", 1.0)):
            v = request.get(key)
            v = default if v is None else v
            if isinstance(v, (list, tuple)):
                if len(v) != n:
                    raise ValueError(f"serve: `{key}` lists {len(v)} values, pipe.controlnet holds {n} net(s)")
                if not all(number(e) for e in v):
                    raise ValueError(f"serve: `{key}` must hold finite numbers, got {list(v)!r}")
                per_net[key] = [float(e) for e in v]
            elif not number(v):
                raise ValueError(f"serve: `{key}` must be a finite number (or a list with one per net), got {v!r}")
            else:
                per_net[key] = [float(v)] * n
        if image is None:
            return None
        if request.get("upscale") or second or self._hires is not None:
            raise ValueError("serve: `control_img` with `upscale` / on a chained hires pair (a ControlNet in the hires pass) is not "
                             "served yet; use txt2img")
        if request.get("mask_image") is not None:
            raise ValueError("serve: `control_img` with `mask_image` (a ControlNet with inpainting) is not served yet; use inpaiting")
        images = list(image) if isinstance(image, (list, tuple)) else [image]
        if isinstance(image, (list, tuple)) != multi or len(images) != n:
            raise ValueError("serve: `control_img` must be " + (f"a list of {n} images (pipe.controlnet is a MultiControlNetModel)"
                             if multi else "one image (a list goes with a MultiControlNetModel)") +
                             f", got {f'a list of {len(images)}' if isinstance(image, (list, tuple)) else type(image).__name__}")
        for one, net in zip(images, self._control_nets()):
            if torch.is_tensor(one):
                cin = int(net.controlnet_cond_embedding.conv_in.in_channels)
                if one.dim() != 4 or one.shape[0] != 1 or one.shape[1] != cin or not torch.is_floating_point(one) \
                        or one.shape[2] < 1 or one.shape[3] < 1:
                    raise ValueError(f"serve: `control_img` as a tensor must be a floating-point [1, {cin}, H, W] image in [0, 1], got "
                                     f"{one.dtype} {list(one.shape)}")
            elif not (hasattr(one, "size") and hasattr(one, "resize") and not hasattr(one, "shape")):
                raise ValueError(f"serve: `control_img` must be a [1, 3, H, W] tensor or a PIL image, got {type(one).__name__}")
        return {"image": images, "scale": per_net["controlnet_conditioning_scale"], "start": per_net["control_guidance_start"],
                "end": per_net["control_guidance_end"]}

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

    def _check_ip_current(self):
        """the captured steps were built for the IP-Adapter processors of construction time (their to_k_ip / to_v_ip, the static
        buffers' layout): a batcher that has seen load_ip_adapter / unload_ip_adapter since is stale"""
        now = _ip_layers(self.pipe)
        proj = getattr(self.pipe.unet, "encoder_hid_proj", None) if now else None
        if len(now) != len(self._ip) or any(a[1] is not b[1] for a, b in zip(now, self._ip)) or proj is not self._ip_proj:
            raise RuntimeError("serve: the pipeline's IP-Adapter processors changed since this batcher was built (load_ip_adapter / "
                               "unload_ip_adapter): its captured steps are stale - build a new one with pipe.serve(...)")

    def _ip_request(self, request):
        """submit-time checks of the image-prompt keys -> (embeds or None, one scale per loaded adapter; all 0 without embeds)"""
        n = len(self._ip_tokens)
        embeds, scale = request.get("ip_adapter_image_embeds"), request.get("ip_adapter_scale")
        if scale is None:
            scale = [float(v) for v in self._ip[0][1].scale] if n else []
        elif isinstance(scale, (list, tuple)):
            if len(scale) != n:
                raise ValueError(f"serve: `ip_adapter_scale` lists {len(scale)} scales, the pipeline has {n} IP-Adapter(s) loaded")
            scale = list(scale)
        else:
            scale = [scale] * n
        for v in scale:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float("inf"), float("-inf")):
                raise ValueError(f"serve: `ip_adapter_scale` must be a finite number or a list of them, got {v!r}")
        scale = [float(v) for v in scale]
        if embeds is None:
            return None, [0.0] * n
        if n == 0:
            raise ValueError("serve: `ip_adapter_image_embeds` on a pipeline without an IP-Adapter (pipe.load_ip_adapter first, then "
                             "build the batcher)")
        if not isinstance(embeds, (list, tuple)) or len(embeds) != n:
            got = len(embeds) if isinstance(embeds, (list, tuple)) else type(embeds).__name__
            raise ValueError(f"serve: `ip_adapter_image_embeds` must be a list with one tensor per loaded IP-Adapter ({n}), got {got}")
        for a, (e, t) in enumerate(zip(embeds, self._ip_tokens)):
            if not torch.is_tensor(e) or e.dim() < 3 or e.shape[0] != 2:
                raise ValueError(f"serve: `ip_adapter_image_embeds[{a}]` must be [negative; positive] along dim 0 ([2, 1, ...], what "
                                 f"txt2img takes), got {list(e.shape) if torch.is_tensor(e) else type(e).__name__}")
            if e.shape[1] != 1:
                raise ValueError(f"serve: `ip_adapter_image_embeds[{a}]` holds {e.shape[1]} images = {e.shape[1] * t} image tokens, "
                                 f"adapter {a} has {t} tokens per request in the batcher (one image; use txt2img for more)")
        if all(v == 0.0 for v in scale):
            return None, scale                                      # nothing to add: no projection work, the rows stay skipped
        return list(embeds), scale

    def _ip_masks_of(self, request):
        """submit-time checks of `ip_adapter_masks` (cross_attention_kwargs) -> the [n_adapters, 1, Hm, Wm] tensor or None"""
        kw = request.get("cross_attention_kwargs")
        masks = kw.get("ip_adapter_masks") if isinstance(kw, dict) else None
        if masks is None:
            return None
        if not self.ip_masks:
            raise ValueError("serve: `ip_adapter_masks` (cross_attention_kwargs) are not supported by this batcher: build it with "
                             "`ip_masks=True` (pipe.serve(..., ip_masks=True)), or use txt2img")
        n = len(self._ip_tokens)
        if not torch.is_tensor(masks) or masks.ndim != 4 or masks.shape[1] != 1:
            raise ValueError(f"serve: `ip_adapter_masks` must be a tensor of shape [num_ip_adapter, 1, height, width], got "
                             f"{list(masks.shape) if torch.is_tensor(masks) else type(masks).__name__}")
        if masks.shape[0] != n:
            raise ValueError(f"serve: `ip_adapter_masks` holds {masks.shape[0]} masks, the pipeline has {n} IP-Adapter(s) loaded")
        if not torch.is_floating_point(masks) or masks.shape[2] < 1 or masks.shape[3] < 1 or not bool(torch.isfinite(masks).all()):
            raise ValueError("serve: `ip_adapter_masks` must hold finite floating-point values")
        return masks

    def _ip_mask_weights(self, masks):
        """once per request: per adapter {L: [L] fp16}, its mask down-sampled to every cross-attention level of THIS batcher as
        the processors' eager route does per layer and step (IPAdapterMaskProcessor.downsample in the mask's own dtype, then the
        query dtype: attention_modify.py:373-376 + :381 / :672-675 + :681)"""
        from .attention_modify import IPAdapterMaskProcessor
        return [{L: IPAdapterMaskProcessor.downsample(masks[a], 1, L, 1)[0, :, 0].to(torch.float16) for L in self.levels()}
                for a in range(masks.shape[0])]

    def _prepare_device(self, r):
        """the device half of _prepare, in the order the pipeline's one generator is consumed: start latent, then step noise"""
        if r.second:
            self.exec.prepare_hires(r)
        elif r.kind == "txt2img":
            self.exec.prepare(r)
        else:
            self.exec.prepare_image(r)
        if any(v != 0.0 for v in r.snoise):
            self.exec.prepare_noise(r, r.eta)

    def _prepare_hires_pair(self, request):
        """a request with `upscale=True`: both passes validated first, then prepared (first pass, then second: the order in which
        txt2img / img2img and _hires_pass draw from the request's generator) -> the first-pass record, its `.hires` the second's"""
        hi = self._hires
        if hi is None:
            raise ValueError("serve: `upscale` (the hires pass) needs a chained pair of batchers (pipe.serve_hires, or chain_hires "
                             "on two batchers); this one is not chained (or use the pipeline methods)")
        if request.get("mask_image") is not None:
            raise ValueError("serve: `mask_image` with `upscale` is not supported (inpaiting refuses the hires pass too)")
        x = request.get("upscale_x", 2.0)
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not x > 0:
            raise ValueError(f"serve: `upscale_x` must be a positive number, got {x!r}")
        th, tw = hires_target_size(self.height, self.width, x, self.pipe.vae_scale_factor)
        if th < self.height or tw < self.width:
            raise ValueError(f"serve: `upscale_x` {x} shrinks {self.height}x{self.width} to {th}x{tw}; only enlarging is served "
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
        if self.ip_masks and not hi.ip_masks and self._ip_masks_of(request) is not None:
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
        r = self._prepare(first, device=False)
        r2 = hi._prepare(second, second=True, device=False)
        r2.future, r2.t_submit = r.future, r.t_submit
        r.hires = r2
        self._prepare_device(r)
        hi._prepare_device(r2)
        return r

    def _image_request(self, r):
        """kind / strength of the request and the submit-time rejections of the image keys -> first index of its schedule"""
        req, pipe = r.req, self.pipe
        image, mask = req.get("image"), req.get("mask_image")
        r.kind, r.strength, r.known = "txt2img", 1.0, None
        if req.get("padding_mask_crop") is not None:
            raise ValueError("serve: `padding_mask_crop` is not supported (use inpaiting)")
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
        r.kind = "img2img" if mask is None else "inpaint"
        r.strength = float(req.get("strength", 1.0))
        if not 0.0 < r.strength <= 1.0:
            raise ValueError(f"serve: `strength` must be in (0, 1], got {r.strength}")
        keep = min(int(r.steps * r.strength), r.steps)                                           # :637-638
        if keep < 1:
            raise ValueError(f"serve: `strength` {r.strength} leaves none of the {r.steps} steps")
        h, w = self.height // 8, self.width // 8
        size = _spatial_size(image)
        latents_in = torch.is_tensor(image) and image.dim() == 4 and image.shape[1] == 4
        if latents_in:
            if tuple(image.shape) != (1, 4, h, w):
                raise ValueError(f"serve: `image` latents {tuple(image.shape)}, this batcher needs {(1, 4, h, w)}")
        else:
            if size != (self.height, self.width) or (torch.is_tensor(image) and (image.dim() != 4 or image.shape[0] != 1)):
                raise ValueError(f"serve: `image` is {size}, this batcher runs one {self.height}x{self.width} image per request")
            if pipe.vae is None or not hasattr(pipe.vae, "encode"):
                raise ValueError("serve: `image` given as pixels needs a VAE with an encoder; pass [1, 4, h, w] latents")
        if mask is not None:
            if pipe.unet.config.in_channels != 4:
                raise ValueError("serve: `mask_image` on a 9-channel inpainting UNet is not supported (use inpaiting)")
            if _spatial_size(mask) not in ((self.height, self.width), (h, w)):
                raise ValueError(f"serve: `mask_image` is {_spatial_size(mask)}, this batcher needs {self.height}x{self.width} "
                                 f"(or the latent size {h}x{w})")
        return max(r.steps - keep, 0)

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
            return all(r.skipout is None for r in members)
        if head.skipout is not None:
            return all(r.kind != "inpaint" for r in members)
        return True

    def _step_locked(self):
        slots = self._slots
        active = [r for r in slots if r is not None]
        stepping = [r for r in active if r.i < len(r.coeffs) and self._n is not None]
        # admissions: FIFO, lowest free slot, while the union of the tables still compresses
        joins = []
        while self._queue:
            free = next((i for i, r in enumerate(slots) if r is None), None)
            if free is None:
                break
            head = self._queue[0]
            if not self._tables_fit([r for r in slots if r is not None] + [head]):
                break
            if not self._launch_compatible(head, [r for r in slots if r is not None]):
                break
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
        if not stepping and not joins:
            return False
        # who leaves after this transition: a request whose last step is the one being applied now
        leaving = [r for r in stepping if r.i + 1 == len(r.coeffs)]
        staying = [r for r in slots if r is not None and r not in leaving]
        n_src = self._n or 0
        n_dst = self._bucket_for(max(r.slot for r in staying)) if staying else None
        nd = n_dst if n_dst is not None else self.buckets[0]
        n_slots = max(n_src, nd)
        recs = []
        for i in range(n_slots):
            r = slots[i] if i < len(slots) else None
            if r is not None and r in stepping:
                a, b, c = r.coeffs[r.i]
                rec = {"mode": ops.ROW_STEP, "sigma": r.sig[r.i], "guidance": r.guidance, "a": a, "b": b, "c": c}
                if r.skipout is not None:
                    rec.update(c_skip=r.skipout[r.i][0], c_out=r.skipout[r.i][1], s=r.snoise[r.i],
                               noise=self.exec.noise_row(r, r.i) if r.snoise[r.i] != 0.0 else None)
                    if r.rescale > 0.0:
                        rec["rescale"] = r.rescale
                if r in leaving:
                    rec.update(c_in_next=0.0, t_next=0.0, sigma_next=1.0, temb_row=None, req=r, step=r.i, next_step=None)
                else:
                    j = r.i + 1
                    rec.update(c_in_next=r.scal[j][0], t_next=r.scal[j][1], sigma_next=max(r.sig[j], 1e-10),
                               temb_row=self.exec.temb_row(r, j), req=r, step=r.i, next_step=j)
            elif r is not None and r in joins:
                rec = {"mode": ops.ROW_JOIN, "c_in_next": r.scal[0][0], "t_next": r.scal[0][1], "sigma_next": r.sig[0],
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
        if n_dst is not None:
            self._ensure(n_dst)
        for r in joins:
            self.exec.load_latent(r)
            if r.control is not None:
                self.exec.load_lane(r)               # its text rows and conditioning embedding(s) into the lane's rows
        self._stats["joins"] += len(joins)
        if any(k is not None for k in known):
            if any(rec["mode"] == ops.ROW_STEP and rec["req"].skipout is not None for rec in recs):
                raise RuntimeError("serve: an inpainting slot and a slot of another sampler step together (admission check bypassed)")
            self.exec.transition_known(n_src, nd, recs, known)
        elif any(rec["mode"] == ops.ROW_STEP and rec["req"].skipout is not None for rec in recs):
            self.exec.transition_linear(n_src, nd, recs)           # a slot steps another sampler / a v-prediction model
            self._stats["linear_transitions"] += 1
        else:
            self.exec.transition(n_src, nd, recs)
        for r in leaving:
            slots[r.slot] = None
            if r.hires is not None:
                self._hand_off(r)
            elif self.decode and r.output_type != "latent":
                self._done.append((r, self.exec.finish_image(r)))       # the row is cloned now and goes to the lane below
            else:
                self._done.append((r, self.exec.finish(r)))
            r.hnoise = None                          # (a second-pass record: its start noise was read before it joined)
            r.known = None                           # its image / noise / mask rows go back to the allocator (stream-ordered)
            r.noise = None                           # ... and its noise table
            r.adapter_feats = None                   # ... and its adapter features
            if r.lane is not None:                   # ... and its ControlNet lane goes to whoever waits for one
                self._lanes[r.lane] = None
                r.lane, r.cemb = None, None
            self._stats["leaves"] += 1
        for r in stepping:
            r.i += 1
        if n_dst is not None:
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
        self._n = n_dst
        if self.decode and any(r.output_type != "latent" for r in leaving):
            # after the next step is queued: the lane's stream waits on the clones' events only, so the decode runs beside it
            self._ensure_decode()
            decodes, rows = self.exec.flush_decodes()
            self._stats["decodes"] += decodes
            self._stats["decode_rows"] += rows
        return True

    def _hand_off(self, r):
        """r leaves this batcher for its hires pass: the resample + noise launch on this batcher's stream, then the second-pass
        record joins the chained batcher's queue (the only place one batcher takes another's lock)"""
        hi, r2 = self._hires, r.hires
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

    def _poll(self, wait=False):
        """resolve the futures of requests whose final row copy has completed (in completion order)"""
        keep = []
        for r, h in self._done:
            if wait or self.exec.ready(h):
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
                elif self._done:
                    self._wake.wait(0.0005)              # rows in flight: look again soon
                else:
                    self._wake.wait()


class _GraphExecutor:
    """The device side on the pipeline's GPU: per-bucket static buffers + captured UNet step, the per-row sampler launch,
    per-request start latents / time-embedding tables / output rows and completion events."""

    def __init__(self, batcher):
        self.b = batcher
        pipe = batcher.pipe
        self.pipe = pipe
        unet = pipe.unet
        self.device = pipe._execution_device
        self.dtype = unet.dtype
        if self.device.type != "cuda" or self.dtype != torch.float16:
            raise NotImplementedError("serve: the batcher runs fp16 on the GPU")
        if not (ops.USE_TEMB_HOIST and hasattr(unet, "temb_add_table")):
            raise NotImplementedError("serve: needs the UNet's per-step time-embedding tables (temb_add_table)")
        if not pipe._all_cross_attention_packable():
            raise NotImplementedError("serve: every cross-attention head dim must run the prepared-operand kernels "
                                      "(d % 8 == 0, d <= 160)")
        c = unet.config.in_channels
        self.lat_shape = (c, batcher.height // 8, batcher.width // 8)
        self.ctx = unet.config.cross_attention_dim
        self.tw = unet.temb_width()
        mb = max(batcher.max_batch, batcher.buckets[-1])
        self.stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.stream(self.stream):
            self.x = torch.zeros((mb,) + self.lat_shape, device=self.device, dtype=self.dtype)
            self.old = torch.zeros_like(self.x)
        self.st = {}
        self._inflight = collections.deque()
        # IP-Adapters: per adapter the layout of one flat row [sum over layers of (k_ip | v_ip), T * C_layer halfs each]
        self.ip_layers = list(batcher._ip)
        self.ip_tokens = list(batcher._ip_tokens)
        self.ip_offsets, self.ip_width = [], []
        for T in self.ip_tokens:
            offs, w = [], 0
            for _, proc in self.ip_layers:
                offs.append(w)
                w += 2 * T * proc.hidden_size
            self.ip_offsets.append(offs)
            self.ip_width.append(w)
        # (controlnet) the lane buffers, the captured ControlNet graph and its residual buffers: one per batcher (ensure_control)
        self.cn_nets = batcher._control_nets() if batcher.cn else []
        self.cn = None
        # (decode) the lane that finishes images beside the step; its stream and buffers are built by ensure_decode
        self.lane = _DecodeLane(self, batcher.decode_batch) if getattr(batcher, "decode", False) else None

    def bind_thread(self):
        _lib.check(_lib.load_library().dsc_set_workspace_slot(self.b.slot), "dsc_set_workspace_slot")

    def throttle(self, ahead=2):
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self._inflight.append(ev)
        while len(self._inflight) > ahead:
            self._inflight.popleft().synchronize()

    # ---- per request
    def prepare(self, r):
        pipe, dev, dt = self.pipe, self.device, self.dtype
        req = r.req
        self.stream.wait_stream(torch.cuda.current_stream(dev))      # the caller's tensors were made on its own stream
        with torch.cuda.stream(self.stream):
            lat = pipe.prepare_latents(1, self.lat_shape[0], self.b.height, self.b.width, dt, dev, req.get("generator"),
                                       req.get("latents"))
            if tuple(lat.shape) != (1,) + self.lat_shape:
                raise ValueError(f"serve: latents {tuple(lat.shape)}, this batcher needs {(1,) + self.lat_shape}")
            r.lat = lat * (r.sig_dev[0] ** 2 + 1) ** 0.5                                       # txt2img's op (:1043)
            self._tables_and_text(r)

    def _tables_and_text(self, r):
        dev, dt = self.device, self.dtype
        ts = [t for _, t in r.scal]
        r.temb = self.pipe.unet.temb_add_table(torch.tensor(ts, dtype=torch.float32, device=dev))
        neg, pos = r.text
        r.text = (neg.to(device=dev, dtype=dt), pos.to(device=dev, dtype=dt))
        if r.ip_embeds is not None:
            self._ip_request_rows(r)
            if r.ip_weights is not None:                 # on the device, in memory of this stream, until the request leaves
                r.ip_weights = [{L: w.to(dev).clone() for L, w in per.items()} for per in r.ip_weights]
        if r.adapter is not None:
            self._adapter_rows(r)

    @torch.no_grad()
    def _control_embedding(self, net, image):
        """one net's conditioning embedding of one prepared [1, 3, H, W] image, channels-last [1, C0, h, w] - the eight
        convolutions of ControlNetConditioningEmbedding.forward WITHOUT ControlNetModel's one-entry cache (`txt2img` on another
        thread owns that).  The library's default algorithm for the LAST convolution (256 channels in, one image) adds partial
        sums in an order that changes from call to call (8 distinct results in 8 calls), and a served request would differ from
        its own repeat by 3e-3 of its range after a few steps through a ControlNet: that convolution runs on the package's own
        3x3 kernel (dsc_conv3x3_nhwc_f16, a fixed summation order).  Where the kernel does not cover its shape, the library is
        asked for a deterministic algorithm through torch's process-wide `torch.backends.cudnn.deterministic` for that one
        call; _EMBED_LOCK keeps two batchers from restoring each other's value, and a library convolution another thread
        launches inside that window is asked for a deterministic algorithm too (other last bits, never other validity)."""
        ce = net.controlnet_cond_embedding
        h = torch.nn.functional.silu(ce.conv_in(image.to(net.dtype).contiguous()))
        for blk in ce.blocks:
            h = torch.nn.functional.silu(blk(h))
        h = h.contiguous(memory_format=torch.channels_last)
        emb = ops.conv3x3_try(h, ce.conv_out.weight.contiguous(memory_format=torch.channels_last), ce.conv_out.bias)
        if emb is None:
            with _EMBED_LOCK:
                was = torch.backends.cudnn.deterministic
                torch.backends.cudnn.deterministic = True
                try:
                    emb = ce.conv_out(h)
                finally:
                    torch.backends.cudnn.deterministic = was
        return emb.to(self.dtype).contiguous(memory_format=torch.channels_last)

    @torch.no_grad()
    def _control_rows(self, r):
        """once per request, when it is admitted (load_lane): its control image(s) as the pipeline prepares them (prepare_image,
        without the CFG duplication: both lane rows read the one embedding) and each net's conditioning embedding, held until the
        request leaves; a request that waits for a lane holds nothing on the device for it"""
        b, pipe = self.b, self.pipe
        want = (1,) + b._control_shapes[0]
        r.cemb = []
        for net, image in zip(self.cn_nets, r.control["image"]):
            img = pipe.prepare_image(image, b.width, b.height, 1, 1, self.device, net.dtype, do_classifier_free_guidance=False)
            emb = self._control_embedding(net, img)
            if tuple(emb.shape) != want:
                raise ValueError(f"serve: `control_img` gives a conditioning embedding {tuple(emb.shape)}, this batcher's ControlNet "
                                 f"step takes {want}")
            r.cemb.append(emb)

    @torch.no_grad()
    def warm_control(self):
        """one conditioning embedding of a blank image per net (the convolution library's first-call cost, outside any request)"""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            for net in self.cn_nets:
                cin = int(net.controlnet_cond_embedding.conv_in.in_channels)
                self._control_embedding(net, torch.zeros(1, cin, self.b.height, self.b.width, device=self.device))

    def ensure_control(self):
        """lane buffers + the captured ControlNet graph of this batcher; True when this call captured it"""
        if self.cn is not None:
            return False
        from .model_k_diffusion import _CAPTURE_LOCK
        with _CAPTURE_LOCK:
            self.bind_thread()
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            self._capture_control()
        return True

    @torch.no_grad()
    def _capture_control(self):
        """The ControlNet(s) over the 2 c lane rows, captured once: reads the static lane buffers (x, t, text and one conditioning
        embedding per net), writes every zero convolution's UNSCALED output into static buffers stacked over the nets - what the
        buckets' steps scatter into their rows (ops.scatter_add_rows).  It does not depend on the bucket.  The nets get the text
        rows and no region prompt, as in _controlnet_hook."""
        dev, dt, b = self.device, self.dtype, self.b
        c, nets = b.control_slots, self.cn_nets
        rows, A = 2 * c, len(nets)
        shapes = b._control_shapes

        def stacked(shp):        # [A, 2 c, C, h, w], every net's rows channels-last, the nets dense behind one another
            return torch.zeros((A, rows, shp[1], shp[2], shp[0]), device=dev, dtype=dt).permute(0, 1, 4, 2, 3)

        with torch.cuda.stream(self.stream):
            cn = {"x": torch.zeros((rows,) + self.lat_shape, device=dev, dtype=dt),
                  "t": torch.zeros(rows, device=dev, dtype=torch.float32),
                  "text": torch.zeros((rows, b.text_len, self.ctx), device=dev, dtype=dt),
                  "emb": [torch.zeros((rows, shapes[0][1], shapes[0][2], shapes[0][0]), device=dev, dtype=dt).permute(0, 3, 1, 2)
                          for _ in nets],
                  "down": [stacked(shp) for shp in shapes[:-1]], "mid": stacked(shapes[-1])}
            for net in nets:
                net._to_channels_last_once()

        def step():
            for a, net in enumerate(nets):
                down, mid = net(cn["x"], cn["t"], encoder_hidden_states=cn["text"], controlnet_cond=None, return_dict=False,
                                cond_embedding=cn["emb"][a], unscaled=True)
                for buf, d in zip(cn["down"] + [cn["mid"]], down + [mid]):
                    buf[a].copy_(d)

        side = self.stream
        with torch.cuda.stream(side):
            for _ in range(2):                       # warm-up: workspaces, kernel selection
                step()
        if ops.GRAPHS_ENABLED:
            torch.cuda.current_stream(dev).wait_stream(side)
            from .model_k_diffusion import _capture_without_gc
            g = torch.cuda.CUDAGraph()
            with _capture_without_gc(), torch.cuda.graph(g):
                step()
            side.wait_stream(torch.cuda.current_stream(dev))
            cn["graph"] = g
            cn["run"] = g.replay
        else:
            cn["run"] = step
        self.cn = cn

    def load_lane(self, r):
        """a request took lane r.lane: its conditioning embedding(s) are computed (once per request, on this stream) and go,
        with its text rows, into ControlNet rows {lane, c + lane}"""
        c, j, cn = self.b.control_slots, r.lane, self.cn
        with torch.cuda.stream(self.stream):
            self._control_rows(r)
            cn["text"][j].copy_(r.text[0][0])
            cn["text"][c + j].copy_(r.text[1][0])
            for buf, emb in zip(cn["emb"], r.cemb):
                buf[j].copy_(emb[0])
                buf[c + j].copy_(emb[0])

    def set_control(self, n, dst, gather, gates):
        """bucket n's dst / gather / gate vectors <- these values (None: unchanged); pinned, non-blocking"""
        ct = self.st[n]["control"]
        with torch.cuda.stream(self.stream):
            if dst is not None:
                ct["dst"].copy_(torch.tensor(dst, dtype=torch.int32).pin_memory(), non_blocking=True)
            if gather is not None:
                ct["gather"].copy_(torch.tensor(gather, dtype=torch.int64).pin_memory(), non_blocking=True)
            if gates is not None:
                ct["gate"].copy_(torch.tensor(gates, dtype=torch.float32).pin_memory(), non_blocking=True)

    def run_control(self, n):
        """the lane rows of bucket n's input and timesteps into the lane buffers (two static-shape launches), then the ControlNet
        graph: its residual buffers are what bucket n's step, replayed next on this stream, scatters"""
        st, cn = self.st[n], self.cn
        with torch.cuda.stream(self.stream):
            torch.index_select(st["x_in"], 0, st["control"]["gather"], out=cn["x"])
            torch.index_select(st["t"], 0, st["control"]["gather"], out=cn["t"])
            cn["run"]()

    @torch.no_grad()
    def _adapter_rows(self, r):
        """once per request: the adapter network on its control image(s), features times scale in the adapter's dtype
        (t2i_adapter.adapter_features: preprocessing_t2i_adapter's lines before the CFG duplication), channels-last"""
        from .t2i_adapter import adapter_features
        feats = adapter_features(self.pipe, r.adapter["image"], self.b.width, self.b.height, r.adapter["scale"])
        got = [tuple(int(v) for v in f.shape) for f in feats]
        want = [(1,) + s for s in self.b._adapter_shapes]
        if got != want:
            raise ValueError(f"serve: `image_t2i_adapter` gives feature maps {got}, this batcher's step takes {want}")
        r.adapter_feats = [f.to(device=self.device, dtype=self.dtype).contiguous(memory_format=torch.channels_last) for f in feats]

    @torch.no_grad()
    def warm_adapter(self):
        """one adapter forward on a blank image (the convolution library's first-call cost, outside any request)"""
        from .t2i_adapter import MultiAdapter, adapter_features
        ad = self.b._adapter
        multi = isinstance(ad, MultiAdapter)
        cin = (ad.adapters[0] if multi else ad).config.in_channels
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            blank = torch.zeros(1, cin, self.b.height, self.b.width)
            adapter_features(self.pipe, [blank] * ad.num_adapter if multi else blank, self.b.width, self.b.height,
                             [1.0] * ad.num_adapter if multi else 1.0)

    def set_adapter_gates(self, n, gates):
        """the bucket's gate vector (read by the captured dsc_add_rows_gated_f16 launches) <- these 2 n values"""
        with torch.cuda.stream(self.stream):
            self.st[n]["adapter"]["gate"].copy_(torch.tensor(gates, dtype=torch.float32).pin_memory(), non_blocking=True)

    @torch.no_grad()
    def _ip_request_rows(self, r):
        """once per request: its image tokens (unet.encoder_hid_proj on its own [2, ...] embeds: txt2img's call shape) through
        every layer's to_k_ip / to_v_ip, packed into one flat [2, width] row pair per adapter (uncond, cond)"""
        dev, dt = self.device, self.dtype
        tokens = self.pipe.unet.encoder_hid_proj([e.to(device=dev, dtype=dt) for e in r.ip_embeds])
        r.ip_rows = []
        for a, T in enumerate(self.ip_tokens):
            tok = tokens[a]
            if tuple(tok.shape) != (2, T, self.ctx):
                raise ValueError(f"serve: `ip_adapter_image_embeds[{a}]` projects to {tuple(tok.shape)} image tokens, adapter {a} "
                                 f"takes {(2, T, self.ctx)}")
            row = torch.empty(2, self.ip_width[a], device=dev, dtype=dt)
            for (_, proc), off in zip(self.ip_layers, self.ip_offsets[a]):
                n = T * proc.hidden_size
                row[:, off:off + n] = proc.to_k_ip[a](tok).reshape(2, n)
                row[:, off + n:off + 2 * n] = proc.to_v_ip[a](tok).reshape(2, n)
            r.ip_rows.append(row)

    def prepare_image(self, r):
        """img2img / inpainting: the start latent of the pipeline method, line for line, on the truncated schedule; for
        inpainting also the image latents, noise and mask rows the per-row step blends from"""
        pipe, dev, dt = self.pipe, self.device, self.dtype
        req, H, W = r.req, self.b.height, self.b.width
        gen, image = req.get("generator"), req["image"]
        latents_in = torch.is_tensor(image) and image.shape[1] == 4
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            if r.kind == "img2img":
                lat = image if latents_in else pipe._encode_vae_image(pipe._image_tensor(image, H, W), gen)     # :600-606
                lat = lat.to(dev, dtype=dt)
                noise = req.get("latents")
                noise = pipe._randn_like_ref(lat.shape, gen, dev, dt) if noise is None else noise.to(dev, dtype=dt)
                if noise.shape != lat.shape:
                    raise ValueError(f"serve: latents (the noise) {tuple(noise.shape)}, this batcher needs {tuple(lat.shape)}")
                r.lat = lat + noise * (r.sig_dev[0] ** 2 + 1) ** 0.5                                                 # :647
            else:
                init = image.float() if latents_in else pipe._image_tensor(image, H, W)
                r.lat, noise, img_lat = pipe.prepare_latents_inpating(
                    1, 4, H, W, dt, dev, gen, req.get("latents"), image=init, sigma=r.sig_dev[0],
                    is_strength_max=r.strength == 1.0, return_noise=True, return_image_latents=True)            # :1459-1478
                mask = pipe._image_tensor(req["mask_image"], H, W, mask=True)
                mask = torch.nn.functional.interpolate(mask, size=self.lat_shape[1:]).to(device=dev, dtype=dt)    # :1253-1257
                # rows of the batcher's own (allocated on its stream, alive until the request leaves)
                r.known = {"image": img_lat[0].to(dt).clone().contiguous(), "noise": noise[0].to(dt).clone().contiguous(),
                           "mask": mask[0].expand(self.lat_shape).contiguous()}
            if tuple(r.lat.shape) != (1,) + self.lat_shape:
                raise ValueError(f"serve: start latent {tuple(r.lat.shape)}, this batcher needs {(1,) + self.lat_shape}")
            r.lat = r.lat.to(dt)
            self._tables_and_text(r)

    def prepare_noise(self, r, eta):
        """the request's noise table on the device, [steps, 1, c, h, w]: `step_noise`, or the draws its sampler would make"""
        req, dev, dt = r.req, self.device, self.dtype
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            table = req.get("step_noise")
            if table is None:
                like = torch.empty((1,) + self.lat_shape, device=dev, dtype=dt)
                ns = None
                if r.family == "dpmpp_2m_sde":
                    if req.get("seed") is not None:              # protocol mode's `brownian_noise` sampler, seeded per request
                        ns = self.pipe.create_noise_sampler(like, r.sig_dev, len(r.coeffs), int(req["seed"]))
                elif req.get("generator") is not None:
                    gen = req["generator"]
                    ns = lambda *_: torch.randn(like.shape, generator=gen, device=gen.device, dtype=dt).to(dev)   # noqa: E731
                table = sampling.step_noise_table(r.family, like, r.sig_dev, eta=eta, noise_sampler=ns)
            r.noise = table.to(device=dev, dtype=dt).contiguous()

    def prepare_hires(self, r):
        """second pass of a hires request (this executor is the target-size batcher's): its unit noise and the tensor the
        hand-off writes its start latent into, both alive until the request leaves"""
        req, dev, dt = r.req, self.device, self.dtype
        shape = (1,) + self.lat_shape
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            noise = req.get("hires_latents")
            noise = self.pipe._randn_like_ref(shape, req.get("generator"), dev, dt) if noise is None else noise.to(dev, dtype=dt)
            # both are allocated on THIS (the second) batcher's stream and used once by the first batcher's stream in hand_off,
            # ordered by events only (no record_stream): that is safe because they are freed only when the request leaves this
            # batcher, after this stream has waited on the hand-off's event - keep that lifetime
            r.hnoise = noise.contiguous()
            r.lat = torch.empty(shape, device=dev, dtype=dt)
            self._tables_and_text(r)
            r.ready = torch.cuda.Event()
            r.ready.record(self.stream)              # the first batcher's stream waits for these allocations and copies

    def hand_off(self, r, r2):
        """one launch on THIS (the first) batcher's stream: x[r.slot] enlarged + r2's noise * fp16 sqrt(sigma_0^2 + 1) -> r2.lat;
        returns the event the second batcher's stream waits on before it loads the row"""
        req = r2.req
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(r2.ready)
            ops.latent_resample_noise(self.x[r.slot:r.slot + 1], r2.lat.shape[-2:], req.get("upscale_method", "bicubic"),
                                      bool(req.get("upscale_antialias", False)), noise=r2.hnoise, sigma0=r2.sig[0], out=r2.lat)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return ev

    def warm_hand_off(self, hi_exec):
        """every mode's tap tables for this pair of sizes on the device now (otherwise on a mode's first hand-off)"""
        (h, w), (H, W) = self.lat_shape[1:], hi_exec.lat_shape[1:]
        for mode in _RESAMPLE_MODES:
            for aa in ((False, True) if mode in ("bilinear", "bicubic") else (False,)):
                device_taps(h, H, mode, aa, self.device)
                device_taps(w, W, mode, aa, self.device)

    def noise_row(self, r, j):
        return r.noise[j, 0]

    def temb_row(self, r, j):
        return r.temb[j]

    def load_latent(self, r):
        with torch.cuda.stream(self.stream):
            if r.ready is not None:                  # a hires second pass: its start latent is written on another stream
                self.stream.wait_event(r.ready)
            self.x[r.slot].copy_(r.lat[0])

    def finish(self, r):
        with torch.cuda.stream(self.stream):
            out = self.x[r.slot:r.slot + 1].clone()
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return out, ev

    def finish_image(self, r):
        """finish() for a request that leaves a decode batcher with an image `output_type`: the same clone and event, wrapped in
        the handle the lane resolves; the row waits in the lane's pending list until flush_decodes"""
        out, ev = self.finish(r)
        h = _LaneHandle(out, ev, r.output_type)
        self.lane.pending.append(h)
        return h

    def ensure_decode(self):
        """the decode lane's stream, per-bucket static buffers and graphs, pinned ring -> how many graphs this call captured"""
        return self.lane.ensure()

    def flush_decodes(self):
        """the pending rows to the lane, up to decode_batch at a time -> (decodes queued, rows in them)"""
        return self.lane.dispatch()

    def ready(self, h):
        if isinstance(h, _LaneHandle):
            return self.lane.ready(h)
        return h[1].query()

    def result(self, r, h):
        if isinstance(h, _LaneHandle):
            return self.lane.result(h)
        out, ev = h
        ev.synchronize()
        if r.output_type == "latent":
            return out
        with torch.cuda.stream(self.stream):
            return self.pipe.latent_to_image(out, r.output_type)

    # ---- per bucket
    def ensure(self, n):
        """static buffers + captured step of bucket n; True when this call captured it"""
        if n in self.st:
            return False
        from .model_k_diffusion import _CAPTURE_LOCK
        with _CAPTURE_LOCK:
            self.bind_thread()
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            self._capture(n)
        return True

    def _capture(self, n):
        pipe, dev, dt = self.pipe, self.device, self.dtype
        rows = 2 * n
        S = self.b.text_len
        with torch.cuda.stream(self.stream):
            st = {"x_in": torch.zeros((rows,) + self.lat_shape, device=dev, dtype=dt),
                  "t": torch.zeros(rows, device=dev, dtype=torch.float32),
                  "sigma": torch.ones(n, device=dev, dtype=torch.float32),
                  "text": torch.zeros((rows, S, self.ctx), device=dev, dtype=dt),
                  "tadd": torch.zeros((rows, self.tw), device=dev, dtype=dt)}
            zero = {L: torch.zeros(rows, L, S_) for L, S_ in self.b.levels().items()}
            comp = pipe._compress_tables(zero)
            st["compressed"] = {L: (ids.to(dev), rws.to(dev)) for L, (ids, rws) in comp.items()}
            st["dense"] = None
            pipe._refresh_text_kv(st["text"])
            self._pin_kv()
            # one flat buffer and one row_scale vector per adapter; scale 0 (idle / no image prompt): the row's contents are never read
            st["ip"] = [{"buf": torch.zeros(rows, w, device=dev, dtype=dt), "scale": torch.zeros(rows, device=dev, dtype=torch.float32)}
                        for w in self.ip_width]
            # (ip_masks) per adapter and level the weight of every query of every row: ones until a masked member is refreshed in
            st["ipw"] = [{L: torch.ones(rows, L, device=dev, dtype=dt) for L in self.b.levels()} for _ in self.ip_width] \
                if self.b.ip_masks else None
            # (t2i_adapter) one feature row per slot and down block, one gate per batch row: all gates 0 until a member's window
            # opens, and a row whose gate is 0 is never read
            st["adapter"] = {"feats": [torch.empty((n,) + shp, device=dev, dtype=dt).contiguous(memory_format=torch.channels_last).zero_()
                                       for shp in self.b._adapter_shapes],
                             "gate": torch.zeros(rows, device=dev, dtype=torch.float32)} if self.b.t2i else None
            # (controlnet) which batch row each ControlNet lane row lands on (-1: idle), which row of x_in / t it is read from, and
            # one gate per net and lane row: all idle / closed until a member that holds a lane is inside its window
            lanes = 2 * self.b.control_slots
            st["control"] = {"dst": torch.full((lanes,), -1, device=dev, dtype=torch.int32),
                             "gather": torch.zeros(lanes, device=dev, dtype=torch.int64),
                             "gate": torch.zeros((len(self.cn_nets), lanes), device=dev, dtype=torch.float32)} if self.b.cn else None
        kw = {"region_prompt": {"region_state": zero, "compressed": st["compressed"], "sigma": st["sigma"], "weight_func": None,
                                "n_std_groups": n, "sigma_per_group": True}}
        if self.ip_layers:
            ip_rows = {}
            for j, (_, proc) in enumerate(self.ip_layers):
                per = []
                for a, T in enumerate(self.ip_tokens):
                    off, m, buf = self.ip_offsets[a][j], T * proc.hidden_size, st["ip"][a]["buf"]
                    row = (buf[:, off:off + m].unflatten(-1, (T, proc.hidden_size)),
                           buf[:, off + m:off + 2 * m].unflatten(-1, (T, proc.hidden_size)), st["ip"][a]["scale"])
                    per.append(row + (st["ipw"][a],) if st["ipw"] is not None else row)
                ip_rows[proc] = per
            kw["region_prompt"]["ip_rows"] = ip_rows
        unet = pipe.unet
        # a batcher built without `t2i_adapter` calls the UNet exactly as it did before the keyword existed
        gated = {"down_intrablock_gated": (st["adapter"]["feats"], st["adapter"]["gate"])} if st["adapter"] is not None else {}
        if st["control"] is not None:                # ... or the `controlnet` flag (the two are not built together)
            gated = {"down_block_scattered": (self.cn["down"], self.cn["mid"], st["control"]["gate"], st["control"]["dst"])}

        def step():
            return unet(st["x_in"], st["t"], encoder_hidden_states=st["text"], cross_attention_kwargs=kw,
                        temb_adds=st["tadd"], cfg_shared_prefix=ops.USE_CFG_SHARED_PREFIX, **gated).sample

        side = self.stream
        with torch.cuda.stream(side):
            for _ in range(2):                       # warm-up: workspaces, kernel selection
                st["eps"] = step()
        if ops.GRAPHS_ENABLED:
            torch.cuda.current_stream(dev).wait_stream(side)
            from .model_k_diffusion import _capture_without_gc
            g = torch.cuda.CUDAGraph()
            with _capture_without_gc(), torch.cuda.graph(g):
                st["eps"] = step()
            side.wait_stream(torch.cuda.current_stream(dev))
            st["graph"] = g

            def run():
                g.replay()
        else:
            def run():
                pipe._refresh_text_kv(st["text"])
                st["eps"] = step()
        st["run"] = run
        self.st[n] = st

    def _pin_kv(self):
        from .u_net_condition_modify import Attention
        for m in self.pipe.unet.modules():
            if isinstance(m, Attention) and m.is_cross_attention and getattr(m, "kv_cache", None) is not None:
                m.kv_cache["pin"] = True

    @staticmethod
    def ip_row_scales(n, members, a):
        """row_scale of adapter a for bucket n: a member's `ip_adapter_scale` at rows {i, n + i} (uncond, cond); 0 for idle slots
        and members without an image prompt - those rows of the buffer are never read"""
        scales = [0.0] * (2 * n)
        for i, r in enumerate(members):
            if r is not None and r.ip_embeds is not None:
                scales[i] = scales[n + i] = float(r.ip_scale[a])
        return scales

    @staticmethod
    def ip_row_weights(n, members, a, L, device=None):
        """[2 n, L] fp16 query weights of adapter a at level L for bucket n: a masked member's down-sampled mask at rows
        {i, n + i} (the reference repeats the mask over the batch, unconditional rows included); ones for idle slots, members
        without a mask and members without an image prompt (whose rows are skipped by their scale 0 anyway)"""
        out = torch.ones(2 * n, L, dtype=torch.float16, device=device)
        for i, r in enumerate(members):
            if r is not None and r.ip_embeds is not None and r.ip_weights is not None:
                out[i] = out[n + i] = r.ip_weights[a][L]
        return out

    def refresh(self, n, members):
        """text rows, their packed K/V, the compressed tables, (IP-Adapters) the image-token rows and scales and (T2I-Adapter) the
        feature rows of bucket n for these slot members (None = IDLE)"""
        st = self.st[n]
        S = self.b.text_len
        with torch.cuda.stream(self.stream):
            text = st["text"]
            dense = {}
            for L in self.b.levels():
                dense[L] = torch.zeros(2 * n, L, S)
            for i, r in enumerate(members):
                if r is None:
                    text[i].zero_()
                    text[n + i].zero_()
                    continue
                text[i].copy_(r.text[0][0])
                text[n + i].copy_(r.text[1][0])
                for L, w in r.tables.items():
                    dense[L][i] = w[0]
                    dense[L][n + i] = w[1]
            for a, ip in enumerate(st["ip"]):
                scales = self.ip_row_scales(n, members, a)
                for i, r in enumerate(members):
                    if scales[i] != 0.0:
                        ip["buf"][i].copy_(r.ip_rows[a][0])
                        ip["buf"][n + i].copy_(r.ip_rows[a][1])
                ip["scale"].copy_(torch.tensor(scales, dtype=torch.float32).pin_memory(), non_blocking=True)
                if st["ipw"] is not None:
                    for L, buf in st["ipw"][a].items():
                        buf.copy_(self.ip_row_weights(n, members, a, L, device=self.device))
            if st["adapter"] is not None:                # members without a control image are skipped: their rows are never read
                for i, r in enumerate(members):
                    if r is not None and r.adapter_feats is not None:
                        for buf, f in zip(st["adapter"]["feats"], r.adapter_feats):
                            buf[i].copy_(f[0])
            self.pipe._refresh_text_kv(text)
            comp = self.pipe._compress_tables(dense)
            if comp is None:
                raise RuntimeError("serve: the admitted requests' tables do not compress (admission check bypassed)")
            self.pipe._upload_tables(st, comp, dense)

    def transition(self, n_src, n_dst, recs):
        st_d = self.st.get(n_dst)
        if st_d is None:
            self.ensure(n_dst)
            st_d = self.st[n_dst]
        eps = self.st[n_src]["eps"] if n_src else None
        with torch.cuda.stream(self.stream):
            ops.cfg_dpmpp2m_step_rows(self.x, eps, self.old, n_src, st_d["x_in"], st_d["t"], st_d["sigma"], recs,
                                      tadd=st_d["tadd"])

    def transition_linear(self, n_src, n_dst, recs):
        """transition() for a step in which a slot steps a sampler other than DPM++ 2M, or a v-prediction model: the same ONE
        launch through dsc_cfg_linear_step_rows (records without c_skip / c_out are DPM++ 2M's: same bits), or through
        dsc_cfg_linear_step_rows_rescale when a stepping record carries `rescale` (the wrapper chooses)"""
        st_d = self.st.get(n_dst)
        if st_d is None:
            self.ensure(n_dst)
            st_d = self.st[n_dst]
        eps = self.st[n_src]["eps"] if n_src else None
        with torch.cuda.stream(self.stream):
            ops.cfg_linear_step_rows(self.x, eps, self.old, n_src, st_d["x_in"], st_d["t"], st_d["sigma"], recs, tadd=st_d["tadd"])

    def transition_known(self, n_src, n_dst, recs, known):
        """transition() for a step in which an inpainting slot steps: the same ONE launch, with the known-region records"""
        st_d = self.st.get(n_dst)
        if st_d is None:
            self.ensure(n_dst)
            st_d = self.st[n_dst]
        eps = self.st[n_src]["eps"] if n_src else None
        with torch.cuda.stream(self.stream):
            ops.cfg_dpmpp2m_step_rows_known(self.x, eps, self.old, n_src, st_d["x_in"], st_d["t"], st_d["sigma"], recs, known,
                                            tadd=st_d["tadd"])

    def run(self, n):
        with torch.cuda.stream(self.stream):
            self.st[n]["run"]()


class _LaneHandle:
    """one image request between leaving the batch and its resolved future: the cloned latent row and its event, then (once
    queued) the lane entry and row index its image lands in, then the value"""
    __slots__ = ("row", "cloned", "output_type", "kind", "entry", "index", "value")

    def __init__(self, row, cloned, output_type):
        self.row, self.cloned, self.output_type = row, cloned, output_type
        self.kind = "uint8" if output_type in ("pil", "uint8") else "float32"
        self.entry, self.index, self.value = None, None, None


class _DecodeLane:
    """The decode lane of a batcher built with `decode=True` (module docstring): device side only, driven by the thread that
    steps the batcher, under the batcher's lock."""

    def __init__(self, ex, decode_batch):
        self.ex, self.device = ex, ex.device
        self.vae = ex.pipe.vae
        p = next(self.vae.parameters())
        if p.dtype != torch.float16 or p.device != self.device:
            raise NotImplementedError(f"serve: `decode=True` needs the VAE in fp16 on the pipeline's GPU ({self.device}), got "
                                      f"{p.dtype} on {p.device}")
        self.decode_batch = int(decode_batch)
        self.buckets = decode_buckets(self.decode_batch)
        self.stream = None
        self.st = {}                           # decode bucket -> static input, outputs and the captured graph
        self.ring, self.free = None, []        # pinned host slots {"uint8", "float32"}: [decode_batch, H, W, 3] each
        self.inflight = collections.deque()    # queued decodes whose rows have not all been collected, oldest first
        self.pending = []                      # handles of rows cloned in this transition, not queued yet

    def ensure(self):
        if self.st:
            return 0
        from .model_k_diffusion import _CAPTURE_LOCK
        with _CAPTURE_LOCK:
            self.ex.bind_thread()
            self.stream = torch.cuda.Stream(device=self.device)
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            for m in self.buckets:
                self._capture(m)
            H, W = self.st[self.buckets[0]]["uint8"].shape[1:3]
            self.ring = [{"uint8": torch.empty((self.decode_batch, H, W, 3), dtype=torch.uint8).pin_memory(),
                          "float32": torch.empty((self.decode_batch, H, W, 3), dtype=torch.float32).pin_memory()}
                         for _ in range(_DECODE_RING)]
            self.free = list(range(_DECODE_RING))
        return len(self.buckets)

    @torch.no_grad()
    def _capture(self, m):
        """bucket m's static buffers and ONE graph: decode_latents' `1 / scaling_factor * latents` and `vae.decode(...).sample`,
        then dsc_image_finish once per output kind.  Same order as _GraphExecutor._capture: two eager runs on the lane's stream,
        the capture, replays on the lane's stream."""
        dev, vae = self.device, self.vae
        inv = 1 / vae.config.scaling_factor
        with torch.cuda.stream(self.stream):
            st = {"z": torch.zeros((m,) + self.ex.lat_shape, device=dev, dtype=torch.float16)}

        def decode():
            img = vae.decode(inv * st["z"]).sample
            return img if img.is_contiguous() else img.contiguous()

        with torch.cuda.stream(self.stream):
            shape = tuple(decode().shape)
            if len(shape) != 4 or shape[:2] != (m, 3) or shape[2] % 8 or shape[3] % 8:
                raise NotImplementedError(f"serve: `decode=True`: the VAE decodes {(m,) + self.ex.lat_shape} to {shape}; the lane "
                                          f"finishes [m, 3, H, W] images with sides that are multiples of 8 (dsc_image_finish)")
            st["uint8"] = torch.zeros((m, shape[2], shape[3], 3), device=dev, dtype=torch.uint8)
            st["float32"] = torch.zeros((m, shape[2], shape[3], 3), device=dev, dtype=torch.float32)

        def run():
            img = decode()
            ops.image_finish(img, "uint8", out=st["uint8"])
            ops.image_finish(img, "float32", out=st["float32"])

        side = self.stream
        with torch.cuda.stream(side):
            for _ in range(2):                       # warm-up: workspaces, kernel selection, the decoder's derived weights
                run()
        if ops.GRAPHS_ENABLED:
            torch.cuda.current_stream(dev).wait_stream(side)
            from .model_k_diffusion import _capture_without_gc
            g = torch.cuda.CUDAGraph()
            with _capture_without_gc(), torch.cuda.graph(g):
                run()
            side.wait_stream(torch.cuda.current_stream(dev))
            st["graph"] = g
            st["run"] = g.replay
        else:
            st["run"] = run
        self.st[m] = st

    def dispatch(self):
        decodes = rows = 0
        while self.pending:
            chunk, self.pending = self.pending[:self.decode_batch], self.pending[self.decode_batch:]
            self._queue(chunk)
            decodes, rows = decodes + 1, rows + len(chunk)
        return decodes, rows

    @torch.no_grad()
    def _queue(self, chunk):
        """one decode of these rows: wait for their clones, fill the static input, replay, copy each request's row of its kind
        into a pinned slot, record the event the poll queries"""
        m = next(b for b in self.buckets if b >= len(chunk))
        st = self.st[m]
        if not self.free:                            # every pinned slot holds rows nobody has collected: wait for the oldest
            for h in list(self.inflight[0]["handles"]):
                if h.value is None:
                    h.value = self._take(h)
        slot = self.free.pop()
        with torch.cuda.stream(self.stream):
            for i, h in enumerate(chunk):
                self.stream.wait_event(h.cloned)
                st["z"][i].copy_(h.row[0])
            if len(chunk) < m:
                st["z"][len(chunk):].zero_()
            st["run"]()
            for i, h in enumerate(chunk):
                self.ring[slot][h.kind][i].copy_(st[h.kind][i], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        entry = {"ev": ev, "slot": slot, "handles": list(chunk), "left": len(chunk)}
        for i, h in enumerate(chunk):
            h.entry, h.index = entry, i
        self.inflight.append(entry)

    def ready(self, h):
        return h.value is not None or (h.entry is not None and h.entry["ev"].query())

    def _take(self, h):
        """the value of a queued handle, copied out of its pinned slot (waits for the decode when it has not completed); the last
        row taken frees the slot, and the cloned latent row is dropped - its decode has completed"""
        entry = h.entry
        entry["ev"].synchronize()
        arr = self.ring[entry["slot"]][h.kind][h.index].numpy().copy()
        h.row = None
        entry["left"] -= 1
        if entry["left"] == 0:
            self.inflight.remove(entry)
            self.free.append(entry["slot"])
        if h.output_type == "pil":
            from PIL import Image
            return Image.fromarray(arr)
        return arr

    def result(self, h):
        if h.value is None:
            if h.entry is None:                      # (asked for before the transition that cloned it has flushed)
                self.dispatch()
            h.value = self._take(h)
        return h.value


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
