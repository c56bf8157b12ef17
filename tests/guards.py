"""Guard bands: buffers whose every element outside the part a kernel may touch holds a sentinel bit pattern.

A kernel's destination, a strided operand or a scratch buffer is a VIEW into a larger flat buffer that these helpers fill with
a NaN bit pattern no kernel produces.  After the launch `untouched` says whether every element outside the view still holds
those bits: a store one row, pixel or chunk past the end lands in the fence (and fails the test) instead of in a neighbouring
allocation of torch's caching allocator, where no test would see it.  Inputs are laid out the same way (`poisoned`): the gaps
between their rows and the elements around them are NaN, so a read past a row's K or Cin, past row M - 1 or past the last
pixel turns a stored value into NaN if it reaches one.  The fences are sized so that an error of the code under test stays
inside the buffer: tests built on them never hand a launch a buffer smaller than it needs.

A plain module (no fixtures, no conftest): tests/test_guards_host.py exercises it on CPU tensors, the *_gpu.py files on the device.
"""
import torch

# one sentinel per element type: NaNs with a payload no kernel stores (canonical NaNs are 0x7E00 / 0x7FC00000 / 0x7FF8000000000000)
SENTINEL_F16 = 0x7E5A                      # as in test_output_paths.py
SENTINEL_F32 = 0x7FC5A5A5
SENTINEL_F64 = 0x7FF8A5A57FF8A5A5          # a NaN as one fp64 AND as two fp32 words: scratch that holds both kinds stays NaN
SENTINEL_U8 = 0xA5
_BITS = {torch.float16: (torch.int16, SENTINEL_F16), torch.float32: (torch.int32, SENTINEL_F32),
         torch.float64: (torch.int64, SENTINEL_F64), torch.uint8: (torch.uint8, SENTINEL_U8)}
TILE_ROWS = 128                            # one full kernel tile: 128 GEMM rows, 8 x 16 convolution pixels


def bits(t):
    """the elements of `t` as integers of the same width (a view: same memory)"""
    return t.view(_BITS[t.dtype][0])


def sentinel(dtype):
    """the sentinel of `dtype` as the integer `bits()` compares equal to (all of them are positive in their signed width)"""
    return _BITS[dtype][1]


def filled(n, dtype, device="cuda"):
    """a flat buffer of n elements, every one the sentinel of `dtype`"""
    bt, _ = _BITS[dtype]
    return torch.full((n,), sentinel(dtype), dtype=bt, device=device).view(dtype)


def _check_layout(rows, row_len, ld, dtype, lead, tail_rows):
    if rows < 1 or row_len < 1 or ld < row_len or tail_rows < 0 or lead < 0:
        raise ValueError(f"fenced: rows {rows}, row_len {row_len}, ld {ld}, lead {lead}, tail_rows {tail_rows}")
    if (lead * dtype.itemsize) % 16 != 0:
        raise ValueError(f"fenced: a lead of {lead} {dtype} elements breaks the view's 16-byte alignment (8 halves, 4 floats)")


def fenced(rows, row_len, ld=None, dtype=torch.float16, lead=64, tail_rows=TILE_ROWS, device="cuda"):
    """(buf, view): `buf` a flat sentinel-filled buffer, `view` a [rows, row_len] view of it with row stride ld >= row_len that
    starts `lead` elements in (16-byte aligned) and is followed by at least tail_rows * ld sentinel elements - the gap of the
    last row included, so that a tile's worth of overhanging rows stays inside `buf`"""
    ld = row_len if ld is None else ld
    _check_layout(rows, row_len, ld, dtype, lead, tail_rows)
    buf = filled(lead + (rows + tail_rows) * ld + 8, dtype, device)
    view = buf[lead:lead + rows * ld].view(rows, ld)[:, :row_len]
    assert view.data_ptr() % 16 == 0
    return buf, view


def untouched(buf, view):
    """True when every element of `buf` outside `view` (any strided view of buf: 1-D to 4-D, the ld - row_len gap of every row
    counts as outside) still holds the sentinel bits"""
    if view.dtype != buf.dtype or view.untyped_storage().data_ptr() != buf.untyped_storage().data_ptr():
        raise ValueError("untouched: view is not a view of buf")
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    inside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(True)
    return bool((bits(buf)[~inside] == sentinel(buf.dtype)).all())


def all_sentinel(buf):
    """True when no element of `buf` was written at all (a call that must refuse before any launch)"""
    return bool((bits(buf) == sentinel(buf.dtype)).all())


def poisoned(t, ld=None, lead=64, tail_rows=TILE_ROWS):
    """(buf, view) as `fenced`, with `view` holding a bit-identical copy of the 2-D tensor `t` (fp16 / fp32 / fp64) and NaN in
    every row gap, before the first row and after the last one; the NaNs are the sentinels, so `untouched` also shows that
    the kernel wrote nothing into its operand"""
    if t.dim() != 2:
        raise ValueError("poisoned: a [rows, row_len] tensor (reshape pixels / tokens to rows first)")
    buf, view = fenced(t.shape[0], t.shape[1], ld, t.dtype, lead, tail_rows, t.device)
    bits(view).copy_(bits(t))
    return buf, view


def exact_scratch(nbytes, align=16, fill=torch.float32, device="cuda"):
    """(buf, ws): `ws` a workspace of EXACTLY nbytes (as a 1-D tensor of `fill` elements, its address a multiple of `align` and
    - to hold a kernel to the alignment it asks for - of no larger power of two) inside `buf`, which fences it on both sides
    with at least max(4096, nbytes) bytes; all of buf, ws included, starts as the NaN sentinel of `fill`"""
    size = fill.itemsize
    if nbytes <= 0 or nbytes % size or align % size or align & (align - 1):
        raise ValueError(f"exact_scratch: {nbytes} bytes at {align} in {fill} elements")
    n, fence = nbytes // size, (max(4096, nbytes) + 2 * align) // size
    buf = filled(2 * fence + n, fill, device)
    start = fence
    while (buf.data_ptr() + start * size) % (2 * align) != align:      # a multiple of align, an odd one
        start += 1
    ws = buf[start:start + n]
    assert ws.data_ptr() % align == 0 and ws.numel() * size == nbytes
    return buf, ws
