"""The preview path of a batcher built with `previews=True`: device side only, driven by the thread that steps the batcher.

Live previews.  Every per-row step entry ends with `old = D`, the fp16 denoised estimate of the step just applied, so
`exec.old[slot]` holds what a preview of that slot should show until the next transition overwrites it.  A request that carries
`preview_every=k` and `on_preview=f` gets `f(step, steps, image)` after every k-th of its steps but the last (`step` counts the
steps applied so far, 1-based, of `steps` in this pass; the last step's result is the future's value).  Right after a transition
the slots that are due go to `preview(slots)`:
  - a free entry of a ring of `preview_ring` pairs is taken - a device buffer uint8 [max_batch, h * scale, w * scale, 3] and a
    pinned host buffer of the same shape, both allocated at `warm()` / the first step, with two events each;
  - ONE launch of dsc_latent_preview on the batcher's stream reads the due rows of `old` (ordered before the next transition,
    which runs on that stream) and writes the thumbnails - a C x 3 linear map of the latent, `/ 2 + 0.5`, clamp, bytes,
    nearest-neighbour enlargement by `preview_scale`;
  - the entry's first event is recorded there; the PREVIEW STREAM waits on it, copies device -> pinned without blocking and
    records the entry's second event, which the poll queries.
Previews are lossy: with no free entry the preview is skipped (counted in stats()["previews_dropped"], per skipped launch) - the
step never waits for a preview.  The poll delivers completed previews oldest first, before it resolves futures: a row is copied
out of the pinned buffer (the callee owns the array), the entry is freed when its last row is taken, and the callback runs on the
polling thread, under the batcher's lock - it should return quickly.  The launch sits outside every captured graph; after
`warm()` there is no allocation and no stream synchronisation on this path.  A batcher built without the flag has no lane and no
second stream, calls none of this and refuses the keys.
"""
import torch

from ... import ops
from ...latent_preview import preview_coef


def preview_scales_for(w_latent):
    """the `preview_scale` values that work at this latent width: one lane of dsc_latent_preview owns 8 pixels of an output row"""
    return tuple(s for s in ops.PREVIEW_SCALES if (w_latent * s) % 8 == 0)


class _PreviewState:
    """the host side of one request's previews on one batcher, from submit until its future resolves (ServingBatcher._preview_of):
    `every` / `call` are its keys, `out` counts its queued previews that have not been delivered, `first` is, for the second pass
    of a hires request, the state of its first pass on the other batcher - whose queued previews its future waits for too"""
    __slots__ = ("every", "call", "out", "first")

    def __init__(self, every, call):
        self.every, self.call, self.out, self.first = every, call, 0, None


class _PreviewHandle:
    """one queued preview launch: its ring entry and how many of its rows have not been taken yet"""
    __slots__ = ("entry", "left")

    def __init__(self, entry, left):
        self.entry, self.left = entry, left


class _PreviewLane:
    """The preview path of a batcher built with `previews=True` (module docstring), under the batcher's lock."""

    def __init__(self, ex, scale, coef, ring):
        self.ex, self.device = ex, ex.device
        self.scale, self.n_ring = int(scale), int(ring)
        self.coef = preview_coef(coef, ex.lat_shape[0])         # (refuses a coefficient count that does not match the latent)
        self.stream = None
        self.ring, self.free = None, []                         # entries: {"dev", "host", "launched", "copied"}

    def ensure(self):
        if self.ring is not None:
            return
        from .executor import _capturing
        _, h, w = self.ex.lat_shape
        shape = (max(self.ex.b.max_batch, 1), h * self.scale, w * self.scale, 3)
        with _capturing(self.ex) as self.stream:                # (a stream of the lane's own, made under the capture lock)
            with torch.cuda.stream(self.stream):
                self.ring = [{"dev": torch.zeros(shape, dtype=torch.uint8, device=self.device),
                              "host": torch.zeros(shape, dtype=torch.uint8).pin_memory(),
                              "launched": torch.cuda.Event(), "copied": torch.cuda.Event()} for _ in range(self.n_ring)]
            self.ex.stream.wait_stream(self.stream)             # the buffers exist before the batcher's stream writes them
        self.free = list(range(self.n_ring))

    @torch.no_grad()
    def launch(self, slots):
        """thumbnails of these slots' rows of `old`, in this order -> the handle the poll queries, or None (no free entry: skipped)"""
        if not self.free:
            return None
        entry = self.ring[self.free.pop()]
        n = len(slots)
        with torch.cuda.stream(self.ex.stream):
            ops.latent_preview(self.ex.old, slots, self.coef, self.scale, out=entry["dev"][:n])
            entry["launched"].record(self.ex.stream)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(entry["launched"])
            entry["host"][:n].copy_(entry["dev"][:n], non_blocking=True)
            entry["copied"].record(self.stream)
        return _PreviewHandle(entry, n)

    def ready(self, h):
        return h.entry["copied"].query()

    def image(self, h, j):
        """thumbnail j of a queued preview as an array the caller owns (waits for the copy when it has not completed); the last
        row taken frees the entry"""
        h.entry["copied"].synchronize()
        arr = h.entry["host"][j].numpy().copy()
        h.left -= 1
        if h.left == 0:
            self.free.append(next(i for i, e in enumerate(self.ring) if e is h.entry))
        return arr
