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

The seam is host scheduling against a replaceable device executor:
  batcher.py      ServingBatcher (construction, the public interface, the phases of a step) and HiresPair; samplers, guidance
                  rescale, hires pairs, the region-table budget
  requests.py     the request record (one class, `_Request`, on every batcher: a feature's fields stay None where it is off) and
                  the submit-time validation of every request key; image-conditioned requests, region masks of image prompts
  ../step_plan.py a request's `plan`, one entry per model call, and the STEP record of an entry - shared with the pipeline's
                  fused loop, so a served request's records are those of its own fused txt2img
  executor.py     _GraphExecutor, the capture sequence, step_launch (which launch serves a transition); image prompts,
                  T2I-Adapter, ControlNet
  decode_lane.py  the decode lane that finishes images beside the step
  encode_lane.py  the encode lane that encodes pixel inputs beside the step
  preview_lane.py the preview path: thumbnails of running requests' denoised estimates, beside the step
  text_lane.py    the text lane that encodes prompt strings beside the step
"""
# every name that is imported from `modules.serving`
from .batcher import HiresPair, ServingBatcher
from .decode_lane import decode_buckets
from .encode_lane import encode_buckets, encode_roles
from .executor import _GraphExecutor, step_launch
from .requests import MAX_TEXT_KEYS, _ip_layers
