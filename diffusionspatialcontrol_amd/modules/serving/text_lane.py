"""The text lane of a batcher built with `text=True`: prompt strings in `submit`, the twin of the encode lane (encode_lane.py).

A batcher without the flag takes ready-made `prompt_embeds` / `negative_prompt_embeds` (and `text_input_ids` for the region
encoder): every client runs `encode_prompt_function` itself - an eager text-encoder call and a chain of small torch ops per
77-token chunk, on its own stream.  A batcher built with `text=True, text_batch=e, clip_skip=s` on a pipeline whose text encoder
is the package's CLIPTextModel (modules/clip_text.py, fp16, on the kernel route) also takes `prompt` / `negative_prompt` strings
and serves the default branch of `encode_prompt_function` (`long_encode == 0`, the emphasis parser of prompt_parser.py) on the
TEXT LANE: a stream with, per bucket g (1, e and the powers of two between), a static ids buffer [2 g, 77], a static multiplier
buffer [g, 2, 77] and ONE captured graph of the encoder (single stream, no parallel branches; with clip_skip > 1 the final
LayerNorm of the earlier hidden state is part of it).

A lane GROUP is one (request, chunk): the chunk's negative and positive row, two rows of the encoder's batch.  A batcher of
`text_len = 77 K` keys gives every request K chunks: `process_texts([negative, prompt])` chunks both texts, the shorter is
padded with empty chunks as the reference does, and more than K chunks are refused.  Chunks behind the longer text's last one
hold the empty chunk in BOTH rows; their weighted encoding is the same for every request, so the lane computes it once when it
is built (through its own bucket-1 path) and copies it into such a chunk's place: only a request's own chunks are groups.

`submit` (the caller's thread; `prompt_chunks`, `prepare`) does host work only: parsing, chunking, the ids for the region encoder,
the request's two [1, S, C] rows (allocated, not written) and the ids / multipliers in pinned memory.  The thread that steps the
batcher dispatches queued requests whose groups have not been sent, in FIFO order, up to e groups per encode: non-blocking
uploads into the bucket's static buffers (rows without a group hold the empty chunk's ids), the graph's replay, ONE
dsc_prompt_weight_rows_f16 launch that writes every group's two slices into its request's rows, one event.  The batcher admits
the head of its queue only when that event has completed; the lane has no thread.  The second pass of a hires pair shares the
first's rows and ids.  A batcher built without the flag has no lane, no stream and the refusals it had.
"""
import numpy as np
import torch

from ... import ops
from .encode_lane import encode_buckets

CHUNK = 77                                    # BOS + 75 + EOS: one call of the encoder


def effective_skip(clip_skip):
    """`clip_skip` as the parser reads it: None, 0 and 1 are the last hidden state"""
    if clip_skip is None:
        return 1
    if isinstance(clip_skip, bool) or not isinstance(clip_skip, int) or clip_skip < 0:
        raise ValueError(f"serve: `clip_skip` must be None or an integer >= 0, got {clip_skip!r}")
    return max(clip_skip, 1)


def check_pipeline(pipe, ctx, text_len, clip_skip):
    """`text=True` against the pipeline, at construction -> the parser the batcher chunks prompts with (host only)"""
    from ..clip_text import CLIPTextModel
    from ..prompt_parser import FrozenCLIPEmbedderWithCustomWords
    enc = getattr(pipe, "text_encoder", None)
    if not isinstance(enc, CLIPTextModel):
        raise NotImplementedError(f"serve: `text=True` needs the package's CLIPTextModel (modules.clip_text) as pipe.text_encoder, "
                                  f"got {type(enc).__name__}")
    dev = pipe._execution_device
    if enc.dtype != torch.float16 or enc.device != dev:
        raise NotImplementedError(f"serve: `text=True` needs the text encoder in fp16 on the pipeline's GPU ({dev}), got "
                                  f"{enc.dtype} on {enc.device}")
    if not enc.kernel_route(2, CHUNK):
        raise NotImplementedError(f"serve: `text=True`: the text encoder does not run [2, {CHUNK}] ids on the package's kernels "
                                  "(CLIPTextModel.kernel_route: head dim 64, hidden and intermediate sizes multiples of 64)")
    if int(enc.config.hidden_size) != int(ctx):
        raise NotImplementedError(f"serve: `text=True`: the text encoder's hidden_size {enc.config.hidden_size} is not the UNet's "
                                  f"cross_attention_dim {ctx}")
    if text_len % CHUNK != 0:
        raise NotImplementedError(f"serve: `text=True`: text_len {text_len} is not a multiple of {CHUNK} (one encoder call per "
                                  f"{CHUNK}-token chunk)")
    if effective_skip(clip_skip) > int(enc.config.num_hidden_layers) + 1:
        raise NotImplementedError(f"serve: `text=True`: clip_skip {clip_skip} reaches behind the encoder's "
                                  f"{enc.config.num_hidden_layers} layers")
    tok = getattr(pipe, "tokenizer", None)
    if not (callable(tok) and hasattr(tok, "get_vocab") and hasattr(tok, "bos_token_id") and hasattr(tok, "eos_token_id")):
        raise NotImplementedError("serve: `text=True` needs pipe.tokenizer with the surface FrozenCLIPEmbedderWithCustomWords "
                                  "uses (callable on a list of texts, get_vocab, bos_token_id, eos_token_id)")
    return FrozenCLIPEmbedderWithCustomWords(tok, enc, clip_skip)


class _TextHandle:
    """one prompt request between submit and admission: its own chunks' ids [real, 2, 77] (int64) and multipliers (float32) on
    the host (pinned by `prepare`), the [1, 77 K] id arrays of both texts, how many groups were sent, then the event of the
    encode that holds its last group"""
    __slots__ = ("ids", "mult", "np_ids", "real", "chunks", "sent", "alloc", "ev")

    def __init__(self, ids, mult, np_ids, chunks):
        self.ids, self.mult, self.np_ids = ids, mult, np_ids
        self.real, self.chunks, self.sent = int(ids.shape[0]), int(chunks), 0
        self.alloc = self.ev = None


def prompt_chunks(parser, negative, prompt, chunks, text_len):
    """[negative, prompt] -> the handle of a request on a batcher of `chunks` chunks: FrozenCLIPEmbedderWithCustomWords.forward's
    rows (both texts chunked, the shorter padded with empty chunks), padded with empty chunks up to `chunks`"""
    batch, _ = parser.process_texts([negative, prompt])
    real = max(len(c) for c in batch)
    if real > chunks:
        raise ValueError(f"serve: the prompt has {real} chunks of {CHUNK} tokens, this batcher's text_len = {text_len} holds "
                         f"{chunks} (build it with text_len = {CHUNK * real}, or shorten the prompt)")
    empty = parser.empty_chunk()
    rows = [[c[k] if k < len(c) else empty for c in batch] for k in range(chunks)]
    ids = np.array([[c.tokens for c in row] for row in rows], dtype=np.int64)              # [chunks, 2, 77]
    mult = np.array([[c.multipliers for c in row] for row in rows[:real]], dtype=np.float32)
    np_ids = [np.hstack(list(ids[:, j]))[None] for j in range(2)]                         # [1, 77 chunks] per text
    return _TextHandle(torch.from_numpy(ids[:real].copy()), torch.from_numpy(mult), np_ids, chunks)


class _TextLane:
    """The text lane of a batcher built with `text=True` (module docstring): device side only.  `prepare` runs on the caller's
    thread; everything else on the thread that steps the batcher, under the batcher's lock."""

    def __init__(self, ex, text_batch, clip_skip):
        self.ex, self.device = ex, ex.device
        self.enc = ex.pipe.text_encoder
        self.text_batch = int(text_batch)
        self.clip_skip = None if effective_skip(clip_skip) == 1 else int(clip_skip)
        self.buckets = encode_buckets(self.text_batch)
        self.S, self.C = ex.b.text_len, ex.ctx
        self.stream = None
        self.st = {}                           # bucket -> static ids, static multipliers, live groups and the captured graph
        self.empty_ids = None                  # [77] the empty chunk's ids on the device
        self.empty = None                      # (negative, positive) [77, C]: the weighted encoding of a chunk empty in both rows
        self.encodes = self.groups = 0

    # ------------------------------------------------------------------ the caller's thread
    @torch.no_grad()
    def prepare(self, r):
        """submit's device half, on the executor's stream: the request's two rows (not written) and its ids / multipliers pinned"""
        h = r.txt
        r.text = tuple(torch.empty((1, self.S, self.C), device=self.device, dtype=torch.float16) for _ in range(2))
        h.ids, h.mult = h.ids.pin_memory(), h.mult.pin_memory()
        h.alloc = torch.cuda.Event()
        h.alloc.record(self.ex.stream)

    # ------------------------------------------------------------------ the stepping thread
    def ensure(self):
        if self.st:
            return 0
        from .executor import _capturing
        empty = self.ex.b._parser.empty_chunk()
        with _capturing(self.ex) as self.stream:     # (a stream of the lane's own, made under the capture lock)
            with torch.cuda.stream(self.stream):
                self.empty_ids = torch.tensor(empty.tokens, dtype=torch.int64, device=self.device)
            for g in self.buckets:
                self._capture(g)
            with torch.cuda.stream(self.stream), torch.no_grad():
                # a chunk that is empty in both rows, through the lane's own bucket-1 path (bucket 1 holds its ids and ones)
                st = self.st[1]
                self.empty = tuple(torch.empty((CHUNK, self.C), device=self.device, dtype=torch.float16) for _ in range(2))
                st["run"]()
                ops.prompt_weight_rows(st["z"], [{"rows": (0, 1), "mult": st["mult"][0], "out": self.empty}])
        return len(self.buckets)

    @torch.no_grad()
    def _capture(self, g):
        """bucket g's static buffers and ONE graph of the encoder on its ids.  Same order as the batcher's step
        (executor._capture_graph): two eager runs on the lane's stream, the capture, replays on it."""
        from .executor import _capture_graph
        with torch.cuda.stream(self.stream):
            st = {"ids": self.empty_ids.repeat(2 * g, 1), "live": 0,
                  "mult": torch.ones((g, 2, CHUNK), device=self.device, dtype=torch.float32)}

        def run():                                   # (every run binds the rows the weighting launch reads)
            st["z"] = self.enc.encode_rows(st["ids"], self.clip_skip)

        st["graph"], st["run"] = _capture_graph(run, self.stream, self.device)
        if tuple(st["z"].shape) != (2 * g, CHUNK, self.C):
            raise NotImplementedError(f"serve: `text=True`: the encoder gives {tuple(st['z'].shape)} for [{2 * g}, {CHUNK}] ids")
        self.st[g] = st

    def dispatch(self, requests, batch=None):
        """these requests' groups that have not been sent, FIFO, up to text_batch (`batch`) per encode -> (encodes queued, groups
        in them); the chunks behind a request's last group receive the empty chunk's rows here"""
        batch = self.text_batch if batch is None else int(batch)
        with torch.cuda.stream(self.stream):
            for r in requests:
                if r.txt.sent == 0 and r.txt.real < r.txt.chunks:
                    self.stream.wait_event(r.txt.alloc)
                    for k in range(r.txt.real, r.txt.chunks):
                        for j in range(2):
                            r.text[j][0, CHUNK * k:CHUNK * (k + 1)].copy_(self.empty[j])
        groups = [(r, k) for r in requests for k in range(r.txt.sent, r.txt.real)]
        encodes = 0
        for at in range(0, len(groups), batch):
            self._queue(groups[at:at + batch])
            encodes += 1
        self.encodes += encodes
        self.groups += len(groups)
        return encodes, len(groups)

    @torch.no_grad()
    def _queue(self, chunk):
        """one encode of these (request, chunk index) groups: upload their ids and multipliers, the bucket's replay, ONE
        dsc_prompt_weight_rows_f16, the event admission queries"""
        g = next(b for b in self.buckets if b >= len(chunk))
        st = self.st[g]
        with torch.cuda.stream(self.stream):
            for j, (r, k) in enumerate(chunk):
                self.stream.wait_event(r.txt.alloc)
                st["ids"][2 * j:2 * j + 2].copy_(r.txt.ids[k], non_blocking=True)
                st["mult"][j].copy_(r.txt.mult[k], non_blocking=True)
            if len(chunk) < st["live"]:              # rows a former encode used and this one does not: the empty chunk again
                st["ids"][2 * len(chunk):2 * st["live"]].copy_(self.empty_ids.expand(2 * (st["live"] - len(chunk)), CHUNK))
            st["live"] = len(chunk)
            st["run"]()
            recs = [{"rows": (2 * j, 2 * j + 1), "mult": st["mult"][j],
                     "out": tuple(r.text[i][0, CHUNK * k:CHUNK * (k + 1)] for i in range(2))} for j, (r, k) in enumerate(chunk)]
            ops.prompt_weight_rows(st["z"], recs)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        for r, k in chunk:
            r.txt.sent = k + 1
            if r.txt.sent == r.txt.real:
                r.txt.ev = ev

    def ready(self, r):
        return r.txt.ev is not None and r.txt.ev.query()

    def wait(self, r):
        r.txt.ev.synchronize()
