"""The decode lane of a batcher built with `decode=True`: device side only, driven by the thread that steps the batcher.

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
"""
import collections

import torch

from ... import ops

_DECODE_RING = 4                     # pinned host slots of the decode lane: decodes whose rows have not been collected yet


def decode_buckets(decode_batch):
    """the batch sizes a lane captures: 1, its batch size and the powers of two between"""
    out, m = {1, int(decode_batch)}, 2
    while m < decode_batch:
        out.add(m)
        m *= 2
    return tuple(sorted(out))


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
        from .executor import _capturing
        with _capturing(self.ex) as self.stream:     # (a stream of the lane's own, made under the capture lock)
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
        then dsc_image_finish once per output kind.  Same order as the batcher's step (executor._capture_graph): two eager runs
        on the lane's stream, the capture, replays on the lane's stream."""
        from .executor import _capture_graph
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

        # (the warm-up runs also build the decoder's derived weights)
        st["graph"], st["run"] = _capture_graph(run, self.stream, dev)
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
