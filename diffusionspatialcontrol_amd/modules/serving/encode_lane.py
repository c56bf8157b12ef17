"""The encode lane of a batcher built with `encode=True`: the input-side twin of the decode lane (decode_lane.py).

Pixel inputs.  On a flagless batcher a request whose `image` / `mask_image` are pixels is prepared inside `submit`, eagerly, on the
stream that replays the captured step (executor.prepare_image): a blocking upload, an eager `vae.encode` per image and a chain of
small torch ops.  A batcher built with `encode=True, encode_batch=e` on a pipeline whose VAE has an encoder moves that work to the
ENCODE LANE: a second stream with, per encode bucket (1, e and the powers of two between), a static fp16 input [m, 3, H, W], static
moments [m, 8, h, w] and ONE captured graph of `vae.encode`, a device staging buffer and a small ring of pinned host buffers.

A lane ROW is one encode: an img2img or 4-channel inpainting request takes one, a request of an `inpaint_unet=True` batcher two
(the image and the masked image), or one when it brings `masked_image_latents`.

`submit` (the caller's thread; `prepare`) does host work and the request's draws only: image and mask are normalised on the host
(a PIL image to its bytes; anything else through `_image_tensor`, whose numpy rule takes array values as they are, to float32),
the request's random draws are made where the inline path makes them and in its order (posterior, noise, posterior of the masked
image, then the step-noise table) and uploaded, the tensors the request keeps (`r.lat`, `r.known`, `r.extra`) are allocated, and an
event is recorded.  No `vae.encode`, no upload of pixels and neither kernel below runs there.

The thread that steps the batcher dispatches queued requests that have not been encoded, in FIFO order, up to e rows per encode:
the images are copied into a pinned slot and uploaded (non-blocking), ONE dsc_image_prepare fills the static input (and each
request's latent mask), the bucket's graph replays (rows of a padded bucket that hold no request are zeros), ONE
dsc_latent_start_rows writes every row's latents / start latent / kept rows, and an event is recorded.  The batcher admits the head
of its queue only when its event has completed; the lane has no thread.  Only a full ring makes the dispatcher wait, for the
oldest encode.  Requests whose `image` is latents, txt2img requests and the second pass of a hires pair never touch the lane, and a
batcher built without the flag has no lane, no second stream and the inline path it had.  The inline path also keeps the requests
the lane would serve with other bits or a blocking copy: an `image` / `mask_image` that is a tensor on a GPU already (the lane's
upload starts on the host), and an inpainting request whose given `latents` are not fp16 (prepare_latents_inpating multiplies
them in their own dtype).
"""
import collections

import torch

from ... import ops
from .decode_lane import decode_buckets as encode_buckets    # (the encode and text lanes capture the same batch sizes)

_ENCODE_RING = 4                     # pinned host slots of the encode lane: encodes whose uploads may still be in flight


def encode_roles(batcher, r):
    """the lane rows of a prepared request record on this batcher, in the order they are encoded: () when it does not touch the
    lane (no flag, txt2img, the second pass of a hires pair, `image` given as latents, pixels that sit on a GPU already, given
    inpainting `latents` that are not fp16: the inline path serves those), else ("image",) or ("image", "masked")"""
    if not getattr(batcher, "encode", False) or r.second or r.kind == "txt2img":
        return ()
    image, given = r.req.get("image"), r.req.get("latents")
    if torch.is_tensor(image) and image.dim() == 4 and image.shape[1] == 4:
        return ()
    if any(torch.is_tensor(t) and t.is_cuda for t in (image, r.req.get("mask_image"))):
        return ()
    if r.kind != "img2img" and torch.is_tensor(given) and given.dtype != torch.float16:
        return ()
    if r.kind == "inpaint_unet" and r.req.get("masked_image_latents") is None:
        return ("image", "masked")
    return ("image",)


class _EncodeHandle:
    """one pixel-input request between submit and admission: its lane rows (host), then what `prepare` leaves (the normalised
    image / mask on the host, the draws on the device and their event), then the event of the encode that holds its last row"""
    __slots__ = ("roles", "sent", "image", "mask", "eps", "noise", "eps_masked", "form", "coef", "drawn", "ev")

    def __init__(self, roles):
        self.roles, self.sent = tuple(roles), 0
        self.image = self.mask = self.eps = self.noise = self.eps_masked = self.form = self.coef = self.drawn = self.ev = None

    @property
    def rows(self):
        return len(self.roles)


class _EncodeLane:
    """The encode lane of a batcher built with `encode=True` (module docstring): device side only.  `prepare` runs on the
    caller's thread; everything else on the thread that steps the batcher, under the batcher's lock."""

    def __init__(self, ex, encode_batch):
        self.ex, self.device = ex, ex.device
        self.vae = ex.pipe.vae
        p = next(self.vae.parameters())
        if p.dtype != torch.float16 or p.device != self.device:
            raise NotImplementedError(f"serve: `encode=True` needs the VAE in fp16 on the pipeline's GPU ({self.device}), got "
                                      f"{p.dtype} on {p.device}")
        self.encode_batch = int(encode_batch)
        self.buckets = encode_buckets(self.encode_batch)
        self.H, self.W = ex.b.height, ex.b.width
        self.lat = (4,) + tuple(ex.lat_shape[1:])
        self.stream = None
        self.st = {}                           # encode bucket -> static input, static moments and the captured graph
        self.dev = None                        # device staging {"image", "mask"}: uint8 [encode_batch, bytes of a float32 image / mask]
        self.ring, self.free = None, []        # pinned host slots of the same two shapes
        self.inflight = collections.deque()    # queued encodes whose pinned slot is still theirs, oldest first

    # ------------------------------------------------------------------ the caller's thread
    def _host_pixels(self, image, mask):
        """`image` (mask=False) or `mask_image` as the kernel reads it, on the host: a PIL image -> its bytes, uint8 [H, W, 3] /
        [H, W] (`_image_tensor`'s convert + resize; the division by 255 is the kernel's); anything else -> `_image_tensor` on the
        host, float32 [3, H, W] in [-1, 1] / [H, W] of zeros and ones"""
        import numpy as np
        import PIL.Image
        if isinstance(image, PIL.Image.Image):
            image = image.convert("L" if mask else "RGB").resize((self.W, self.H), resample=PIL.Image.LANCZOS)
            return torch.from_numpy(np.array(image))
        t = self.ex.pipe._image_tensor(image, self.H, self.W, mask=mask)
        if tuple(t.shape) != (1, 1 if mask else 3, self.H, self.W):
            raise ValueError(f"serve: `{'mask_image' if mask else 'image'}` prepares to {tuple(t.shape)}, this batcher encodes one "
                             f"{(1 if mask else 3, self.H, self.W)} image per request")
        return (t[0, 0] if mask else t[0]).contiguous()

    @torch.no_grad()
    def prepare(self, r):
        """submit's half: host pixels, the draws in the inline path's order, the tensors the request keeps, an event"""
        ex, dev, dt = self.ex, self.device, self.ex.dtype
        pipe, req, enc = ex.pipe, r.req, r.enc
        gen = req.get("generator")
        shape = (1,) + self.lat
        enc.image = self._host_pixels(req["image"], False)
        if r.kind != "img2img":
            enc.mask = self._host_pixels(req["mask_image"], True)
        given = req.get("latents")
        kind = "img2img" if r.kind == "img2img" else "inpaint_max" if r.strength == 1.0 else "inpaint"
        enc.form, enc.coef = ops.start_form(kind, r.sig[0], given_latents=given is not None)
        ex.stream.wait_stream(torch.cuda.current_stream(dev))        # the caller's tensors were made on its own stream
        with torch.cuda.stream(ex.stream):
            enc.eps = pipe._randn_like_ref(shape, gen, dev, dt).contiguous()             # DiagonalGaussianDistribution.sample
            noise = pipe._randn_like_ref(shape, gen, dev, dt) if given is None else given.to(dev, dtype=dt)
            if tuple(noise.shape) != shape:
                raise ValueError(f"serve: latents (the noise) {tuple(noise.shape)}, this batcher needs {shape}")
            enc.noise = noise.contiguous()
            r.lat = torch.empty(shape, device=dev, dtype=dt)
            if r.kind == "inpaint":
                r.known = {name: torch.empty(self.lat, device=dev, dtype=dt) for name in ("image", "noise", "mask")}
            elif r.kind == "inpaint_unet":
                r.extra = torch.empty((5,) + self.lat[1:], device=dev, dtype=dt)
                mil = req.get("masked_image_latents")
                if mil is None:
                    enc.eps_masked = pipe._randn_like_ref(shape, gen, dev, dt).contiguous()
                else:
                    r.extra[1:].copy_(mil.to(device=dev, dtype=dt)[0])
            ex._tables_and_text(r)
            enc.drawn = torch.cuda.Event()
            enc.drawn.record(ex.stream)

    # ------------------------------------------------------------------ the stepping thread
    def ensure(self):
        if self.st:
            return 0
        from .executor import _capturing
        with _capturing(self.ex) as self.stream:     # (a stream of the lane's own, made under the capture lock)
            for m in self.buckets:
                self._capture(m)
            e, px = self.encode_batch, self.H * self.W
            with torch.cuda.stream(self.stream):
                self.dev = {"image": torch.zeros((e, px * 12), device=self.device, dtype=torch.uint8),
                            "mask": torch.zeros((e, px * 4), device=self.device, dtype=torch.uint8)}
            self.ring = [{"image": torch.empty((e, px * 12), dtype=torch.uint8).pin_memory(),
                          "mask": torch.empty((e, px * 4), dtype=torch.uint8).pin_memory()} for _ in range(_ENCODE_RING)]
            self.free = list(range(_ENCODE_RING))
        return len(self.buckets)

    @torch.no_grad()
    def _capture(self, m):
        """bucket m's static buffers and ONE graph: `vae.encode(x).latent_dist.parameters` into the static moments.  Same order
        as the batcher's step (executor._capture_graph): two eager runs on the lane's stream, the capture, replays on it."""
        from .executor import _capture_graph
        dev, vae = self.device, self.vae
        with torch.cuda.stream(self.stream):
            st = {"x": torch.zeros((m, 3, self.H, self.W), device=dev, dtype=torch.float16)}
            shape = tuple(vae.encode(st["x"]).latent_dist.parameters.shape)
            want = (m, 8) + self.lat[1:]
            if shape != want:
                raise NotImplementedError(f"serve: `encode=True`: the VAE encodes {tuple(st['x'].shape)} to moments {shape}; the "
                                          f"lane's rows are {want} (mean | logvar of this batcher's latent)")
            st["moments"] = torch.zeros(want, device=dev, dtype=torch.float16)

        def run():
            st["moments"].copy_(vae.encode(st["x"]).latent_dist.parameters)

        # (the warm-up runs also build the encoder's derived weights)
        st["graph"], st["run"] = _capture_graph(run, self.stream, dev)
        self.st[m] = st

    def dispatch(self, requests):
        """these requests' rows that have not been sent, FIFO, up to encode_batch per encode -> (encodes queued, rows in them)"""
        rows = [(r, k) for r in requests for k in range(r.enc.sent, r.enc.rows)]
        encodes = 0
        for at in range(0, len(rows), self.encode_batch):
            self._queue(rows[at:at + self.encode_batch])
            encodes += 1
        return encodes, len(rows)

    def reclaim(self):
        """pinned slots of completed encodes go back to the free list"""
        while self.inflight and self.inflight[0]["ev"].query():
            self.free.append(self.inflight.popleft()["slot"])

    def _stage(self, slot, k, name, host):
        """host pixels -> row k of the pinned slot -> row k of the device staging buffer (non-blocking) -> its typed view there"""
        flat = host.reshape(-1)
        n = flat.numel() * flat.element_size()
        pin = self.ring[slot][name][k][:n]
        (pin if host.dtype == torch.uint8 else pin.view(host.dtype)).copy_(flat)
        on = self.dev[name][k][:n]
        on.copy_(pin, non_blocking=True)
        return (on if host.dtype == torch.uint8 else on.view(host.dtype)).view(host.shape)

    @torch.no_grad()
    def _queue(self, chunk):
        """one encode of these (request, row index) pairs: upload their pixels, ONE dsc_image_prepare, the bucket's replay, ONE
        dsc_latent_start_rows, the event admission queries"""
        m = next(b for b in self.buckets if b >= len(chunk))
        st = self.st[m]
        self.reclaim()
        if not self.free:                            # every pinned slot is in use: wait for the oldest encode
            self.inflight[0]["ev"].synchronize()
            self.reclaim()
        slot = self.free.pop()
        scaling = float(self.vae.config.scaling_factor)
        members = []                                 # the distinct requests of this chunk, in order
        for r, _ in chunk:
            if not members or members[-1] is not r:
                members.append(r)
        with torch.cuda.stream(self.stream):
            prep, start = [], []
            for k, r in enumerate(members):
                enc = r.enc
                at = {enc.roles[j]: i for i, (q, j) in enumerate(chunk) if q is r}        # role -> row of the static input
                self.stream.wait_event(enc.drawn)
                row = {"image": self._stage(slot, k, "image", enc.image)}
                if "image" in at:
                    row["out_image"] = st["x"][at["image"]]
                if "masked" in at:
                    row["out_masked"] = st["x"][at["masked"]]
                if "image" in at and enc.mask is not None:                               # the latent mask goes with the first row
                    row["out_mask"] = r.known["mask"] if r.kind == "inpaint" else r.extra[:1]
                if "out_masked" in row or "out_mask" in row:
                    row["mask"] = self._stage(slot, k, "mask", enc.mask)
                prep.append(row)
                if "image" in at:
                    known = r.known if r.kind == "inpaint" else None
                    start.append({"form": enc.form, "row": at["image"], "eps": enc.eps, "noise": enc.noise, "scaling": scaling,
                                  "coef": enc.coef, "start": r.lat, "keep": None if known is None else known["image"],
                                  "keep_noise": None if known is None else known["noise"]})
                if "masked" in at:
                    start.append({"form": "none", "row": at["masked"], "eps": enc.eps_masked, "scaling": scaling,
                                  "keep": r.extra[1:]})
            if len(chunk) < m:
                st["x"][len(chunk):].zero_()
            ops.image_prepare(prep, self.H, self.W)
            st["run"]()
            ops.latent_start(st["moments"], start)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.inflight.append({"ev": ev, "slot": slot})
        for r, j in chunk:
            r.enc.sent = j + 1
            if r.enc.sent == r.enc.rows:
                r.enc.ev = ev

    def ready(self, r):
        return r.enc.ev is not None and r.enc.ev.query()

    def wait(self, r):
        r.enc.ev.synchronize()
