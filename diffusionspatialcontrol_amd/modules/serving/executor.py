"""The device side of the batcher on the pipeline's GPU (`_GraphExecutor`), the one capture sequence every captured graph of the
batcher goes through, and `step_launch`, the one place that decides which per-row sampler launch serves a transition.

Image prompts.  On a pipeline with IP-Adapters loaded (load_ip_adapter) the batcher's step carries, per cross-attention layer and
adapter, to_k_ip / to_v_ip of every batch row's image tokens and one scale per row: a request with `ip_adapter_image_embeds` has
its image tokens projected (unet.encoder_hid_proj) and pushed through every layer's to_k_ip / to_v_ip ONCE, at admission, into
a flat row pair; `refresh` copies a member's pair into rows {i, n + i} of the bucket's static buffer (one per adapter; each
layer's k_ip / v_ip are views into it) and writes its `ip_adapter_scale` into the bucket's row_scale vector.  In the captured
step every IP-Adapter processor runs the stock text branch and then ONE launch per adapter of dsc_ip_xattn_add_f16, which reads
row_scale on the device: idle slots and requests without an image prompt carry scale 0, their workgroups return at once and
their rows are bit for bit those of a batcher without an adapter; joins, leaves and a changed scale need no capture.  The
sampler launches do not know about any of it, so every request kind, sampler and guidance rescale combines with an image prompt.

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
"""
import collections
import contextlib
import threading

import torch

from ... import _lib, ops
from .. import sampling
from ..latent_resample import MODES as _RESAMPLE_MODES, device_taps
from .decode_lane import _DecodeLane, _LaneHandle
from .encode_lane import _EncodeLane
from .preview_lane import _PreviewLane
from .text_lane import _TextLane

_EMBED_LOCK = threading.Lock()       # around the process-wide deterministic switch in _GraphExecutor._control_embedding
_STEP_ROWS = {"rows": "cfg_dpmpp2m_step_rows", "linear": "cfg_linear_step_rows", "known": "cfg_dpmpp2m_step_rows_known",
              "cat": "cfg_linear_step_rows_cat", "staged": "cfg_staged_step_rows"}     # in ops


def step_launch(recs, known=None, extras=None):
    """which ONE launch of the per-row sampler step serves a transition with these records:
    "cat"    - the batcher serves a 9-channel inpainting UNet (`extras` is a list, one entry per slot - every transition of a
               batcher built with `inpaint_unet=True`): dsc_cfg_linear_step_rows_cat, which carries every sampler, both
               parameterisations and the rescale, and writes the extra input channels behind each latent row;
    "known"  - an inpainting slot steps (some entry of `known` is a record): dsc_cfg_dpmpp2m_step_rows_known;
    "staged" - a slot is inside a step of a two-call sampler (a STEP record carries a `stage` other than FULL; a batcher built
               with `two_call=True`): dsc_cfg_staged_step_rows, which takes the intermediate-point buffer; every other slot rides in
               it as a FULL record with the bits of "linear" (the rescale included);
    "linear" - a slot steps another sampler, a v-prediction model or with a guidance rescale (a STEP record carries c_skip /
               c_out): dsc_cfg_linear_step_rows, whose wrapper picks the rescale entry from the records (records without
               c_skip / c_out are DPM++ 2M's: same bits);
    "rows"   - every stepping slot is DPM++ 2M on an eps-prediction model (and IDLE / JOIN-only transitions):
               dsc_cfg_dpmpp2m_step_rows."""
    if extras is not None:
        return "cat"
    if known is not None and any(k is not None for k in known):
        return "known"
    if any(rec["mode"] == ops.ROW_STEP and rec.get("stage", ops.ROW_STAGE_FULL) != ops.ROW_STAGE_FULL for rec in recs):
        return "staged"
    if any(rec["mode"] == ops.ROW_STEP and "c_skip" in rec for rec in recs):
        return "linear"
    return "rows"


@contextlib.contextmanager
def _capturing(ex, stream=None):
    """what every capture site holds while it builds static buffers and captures: the process-wide capture lock, this thread
    bound to the batcher's workspace slot, and `stream` (None: a new one) waiting for the caller's -> the stream"""
    from ..model_k_diffusion import _CAPTURE_LOCK
    with _CAPTURE_LOCK:
        ex.bind_thread()
        if stream is None:
            stream = torch.cuda.Stream(device=ex.device)
        stream.wait_stream(torch.cuda.current_stream(ex.device))
        yield stream


def _capture_graph(run, stream, device):
    """two eager runs of `run` on `stream` (warm-up: workspaces, kernel selection), then its capture -> (graph, graph.replay);
    with ops.GRAPHS_ENABLED off nothing is captured -> (None, run)"""
    with torch.cuda.stream(stream):
        for _ in range(2):
            run()
    if not ops.GRAPHS_ENABLED:
        return None, run
    torch.cuda.current_stream(device).wait_stream(stream)
    from ..model_k_diffusion import _capture_without_gc
    g = torch.cuda.CUDAGraph()
    with _capture_without_gc(), torch.cuda.graph(g):
        run()
    stream.wait_stream(torch.cuda.current_stream(device))
    return g, g.replay


def _upload(buf, values, dtype):
    """static device buffer <- these host values, through pinned memory, non-blocking (on the current stream)"""
    buf.copy_(torch.tensor(values, dtype=dtype).pin_memory(), non_blocking=True)


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
                                      f"(a multiple of 8, at most {ops.ATTN_MAX_HEAD_DIM})")
        c = unet.config.in_channels
        # lat_shape: a request's latent (x / old, noise, outputs); in_shape: a row of the bucket's model input - the same, but
        # [latents | mask | masked-image latents] on a batcher built with `inpaint_unet=True` (reference :1617-1619)
        self.in_shape = (c, batcher.height // 8, batcher.width // 8)
        self.lat_shape = (4,) + self.in_shape[1:] if getattr(batcher, "inpaint", False) else self.in_shape
        self.ctx = unet.config.cross_attention_dim
        self.tw = unet.temb_width()
        mb = max(batcher.max_batch, batcher.buckets[-1])
        self.stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.stream(self.stream):
            self.x = torch.zeros((mb,) + self.lat_shape, device=self.device, dtype=self.dtype)
            self.old = torch.zeros_like(self.x)
            # (two_call) the intermediate point of a two-call sampler's step, a row per slot beside x / old
            self.mid = torch.zeros_like(self.x) if getattr(batcher, "two_call", False) else None
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
        # (encode) the lane that encodes pixel inputs beside the step; its stream and buffers are built by ensure_encode
        self.enc_lane = _EncodeLane(self, batcher.encode_batch) if getattr(batcher, "encode", False) else None
        # (text) the lane that encodes prompt strings beside the step; its stream and buffers are built by ensure_text
        self.text_lane = _TextLane(self, batcher.text_batch, batcher.clip_skip) if getattr(batcher, "text_on", False) else None
        # (previews) the path that turns rows of `old` into thumbnails beside the step; its stream and ring are built by ensure_preview
        self.previews = _PreviewLane(self, batcher.preview_scale, batcher.preview_coef, batcher.preview_ring) \
            if getattr(batcher, "previews", False) else None

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
        ts = [call.t for call in r.plan]
        r.temb = self.pipe.unet.temb_add_table(torch.tensor(ts, dtype=torch.float32, device=dev))
        if r.text is None:                               # a prompt request: the text lane writes its rows beside the step
            self.text_lane.prepare(r)
        else:
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
        with _capturing(self, self.stream):
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

        cn["graph"], cn["run"] = _capture_graph(step, self.stream, dev)
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
            for key, values, dtype in (("dst", dst, torch.int32), ("gather", gather, torch.int64), ("gate", gates, torch.float32)):
                if values is not None:
                    _upload(ct[key], values, dtype)

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
        from ..t2i_adapter import adapter_features
        feats = adapter_features(self.pipe, r.adapter["image"], self.b.width, self.b.height, r.adapter["scale"])
        got = [tuple(int(v) for v in f.shape) for f in feats]
        want = [(1,) + s for s in self.b._adapter_shapes]
        if got != want:
            raise ValueError(f"serve: `image_t2i_adapter` gives feature maps {got}, this batcher's step takes {want}")
        r.adapter_feats = [f.to(device=self.device, dtype=self.dtype).contiguous(memory_format=torch.channels_last) for f in feats]

    @torch.no_grad()
    def warm_adapter(self):
        """one adapter forward on a blank image (the convolution library's first-call cost, outside any request)"""
        from ..t2i_adapter import MultiAdapter, adapter_features
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
            _upload(self.st[n]["adapter"]["gate"], gates, torch.float32)

    def set_freeu(self, n, table):
        """the bucket's FreeU table (read by the captured dsc_freeu_rows_f16 launches) <- these [2 n][4] values"""
        with torch.cuda.stream(self.stream):
            _upload(self.st[n]["freeu"], table, torch.float32)

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
            if r.kind == "inpaint_unet":
                self._prepare_inpaint_unet(r, image, latents_in)
            elif r.kind == "img2img":
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

    def _prepare_inpaint_unet(self, r, image, latents_in):
        """a request of a batcher built with `inpaint_unet=True`, as `inpaiting` prepares it for a 9-channel UNet and in its order
        (start latent, mask, masked-image latents): r.lat, and r.extra - the fp16 [5, h, w] row cat([nearest-downsampled mask,
        masked_image_latents]) (reference :1253-1290) the sampler launch scales and writes behind the latent, built once, on
        this stream, and held until the request leaves"""
        pipe, dev, dt = self.pipe, self.device, self.dtype
        req, H, W = r.req, self.b.height, self.b.width
        gen = req.get("generator")
        init = image.float() if latents_in else pipe._image_tensor(image, H, W)
        r.lat = pipe.prepare_latents_inpating(1, 4, H, W, dt, dev, gen, req.get("latents"), image=init, sigma=r.sig_dev[0],
                                              is_strength_max=r.strength == 1.0, return_noise=True,
                                              return_image_latents=True)[0]                              # :1459-1478
        mask = pipe._image_tensor(req["mask_image"], H, W, mask=True)
        mil = req.get("masked_image_latents")
        if mil is None:
            mil = pipe._encode_vae_image(init * (mask < 0.5), gen)
        mil = mil.to(device=dev, dtype=dt)
        mask = torch.nn.functional.interpolate(mask, size=self.lat_shape[1:]).to(device=dev, dtype=dt)    # :1253-1257
        if tuple(mil.shape) != (1,) + self.lat_shape:
            raise ValueError(f"serve: masked-image latents {tuple(mil.shape)}, this batcher needs {(1,) + self.lat_shape}")
        r.extra = torch.cat([mask[0], mil[0]], dim=0).contiguous()

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
                        ns = self.pipe.create_noise_sampler(like, r.sig_dev, len(r.plan), int(req["seed"]))
                elif req.get("generator") is not None:
                    gen = req["generator"]
                    ns = lambda *_: torch.randn(like.shape, generator=gen, device=gen.device, dtype=dt).to(dev)   # noqa: E731
                if r.plan.two_call:                                  # a two-call sampler: one row per model call
                    if r.family == "dpmpp_sde":
                        ns = None if req.get("seed") is None else \
                            self.pipe.create_noise_sampler(like, r.sig_dev, r.steps, int(req["seed"]))
                    table = sampling.call_noise_table(r.family, like, r.sig_dev, eta=eta, noise_sampler=ns)
                else:
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
            if r.enc is not None:                    # a pixel input: its rows are written on the lane's stream
                self.stream.wait_event(r.enc.ev)
            if r.txt is not None:                    # a prompt: its text rows are written on the lane's stream
                self.stream.wait_event(r.txt.ev)
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

    def prepare_encode(self, r):
        """submit's half of a pixel-input request on a batcher built with `encode=True`: host pixels, draws, allocations"""
        self.enc_lane.prepare(r)

    def ensure_encode(self):
        """the encode lane's stream, per-bucket static buffers and graphs, staging and pinned ring -> how many graphs this call
        captured"""
        return self.enc_lane.ensure()

    def dispatch_encodes(self, requests):
        """these queued requests' rows to the lane, up to encode_batch per encode -> (encodes queued, rows in them)"""
        return self.enc_lane.dispatch(requests)

    def encode_ready(self, r):
        self.enc_lane.reclaim()
        return self.enc_lane.ready(r)

    def encode_wait(self, r):
        self.enc_lane.wait(r)

    def prepare_text(self, r):
        """the device half of a holder of prompt strings outside a request (batcher.encode_text): its rows and pinned ids"""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            self.text_lane.prepare(r)

    def ensure_text(self):
        """the text lane's stream, per-bucket static buffers and graphs, the empty chunk's rows -> how many graphs this call
        captured"""
        return self.text_lane.ensure()

    def dispatch_texts(self, requests, batch=None):
        """these queued requests' groups to the lane, up to text_batch (`batch`) per encode -> (encodes queued, groups in them)"""
        return self.text_lane.dispatch(requests, batch)

    def text_ready(self, r):
        return self.text_lane.ready(r)

    def text_wait(self, r):
        self.text_lane.wait(r)

    def ensure_preview(self):
        """the preview path's stream and its ring of device / pinned buffers (preview_lane.py)"""
        self.previews.ensure()

    def preview(self, slots):
        """one launch of dsc_latent_preview on these slots' rows of `old`, now - after the transition that wrote them, before the
        next - and their copy to pinned memory on the preview stream -> a handle, or None when every ring entry is in use"""
        return self.previews.launch(slots)

    def preview_ready(self, h):
        return self.previews.ready(h)

    def preview_image(self, h, j):
        """thumbnail j (the order of `slots`) of a queued preview: np.uint8 [h * scale, w * scale, 3], the caller's own"""
        return self.previews.image(h, j)

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
        with _capturing(self, self.stream):
            self._capture(n)
        return True

    def _capture(self, n):
        pipe, dev, dt = self.pipe, self.device, self.dtype
        rows = 2 * n
        S = self.b.text_len
        with torch.cuda.stream(self.stream):
            st = {"x_in": torch.zeros((rows,) + self.in_shape, device=dev, dtype=dt),
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
            # (freeu) (s1, s2, b1, b2) per batch row: ones until a member with `freeu` is refreshed in, and a row of ones is
            # neither read nor written by the FreeU launches
            st["freeu"] = torch.ones((rows, 4), device=dev, dtype=torch.float32) if getattr(self.b, "freeu", False) else None
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

        if st["freeu"] is not None:                  # a batcher built without `freeu` calls the UNet exactly as it did before
            gated = dict(gated, freeu_rows=st["freeu"])

        def step():                                  # (every run binds the eps the next transition reads)
            st["eps"] = unet(st["x_in"], st["t"], encoder_hidden_states=st["text"], cross_attention_kwargs=kw,
                             temb_adds=st["tadd"], cfg_shared_prefix=ops.USE_CFG_SHARED_PREFIX, **gated).sample

        def eager():                                 # without graphs nothing replays the text K/V's producers: run them too
            pipe._refresh_text_kv(st["text"])
            step()

        st["graph"], replay = _capture_graph(step, self.stream, dev)
        st["run"] = replay if st["graph"] is not None else eager
        self.st[n] = st

    def _pin_kv(self):
        from ..u_net_condition_modify import Attention
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
                _upload(ip["scale"], scales, torch.float32)
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

    def transition(self, n_src, n_dst, recs, known=None, extras=None):
        """ONE launch of the per-row sampler step - the one step_launch names for these records - takes the eps of bucket
        n_src and writes bucket n_dst's input; `known`: per slot the known-region record of an inpainting slot that steps;
        `extras` (a batcher built with `inpaint_unet=True`): per slot the member's extra input channels, None for an idle slot"""
        kind = step_launch(recs, known, extras)
        st_d = self.st.get(n_dst)
        if st_d is None:
            self.ensure(n_dst)
            st_d = self.st[n_dst]
        eps = self.st[n_src]["eps"] if n_src else None
        args = (self.x,) + ((self.mid,) if kind == "staged" else ()) + \
            (eps, self.old, n_src, st_d["x_in"], st_d["t"], st_d["sigma"], recs) + \
            ((known,) if kind == "known" else (extras,) if kind == "cat" else ())
        with torch.cuda.stream(self.stream):
            getattr(ops, _STEP_ROWS[kind])(*args, tadd=st_d["tadd"])

    def run(self, n):
        with torch.cuda.stream(self.stream):
            self.st[n]["run"]()

