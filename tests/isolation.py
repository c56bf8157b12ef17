"""Row isolation: what one request holds never changes the bits of another request in the same launch.

The continuous batcher puts unrelated requests into one launch of every kernel.  A request that diverges (fp16 `inf` / NaN latents)
must stay alone with it.  Masking by a multiply (`0 * NaN`), a seam select that is off by one, an LDS pad that is not zeroed and a
wave-wide reduction over packed rows are all invisible while every neighbour is finite; with hostile VALUES in the neighbouring
image `torch.equal` on bit views finds them, and no tolerance is needed.

An op case supplies

    run(operands) -> outputs      dicts name -> tensor; `run` leaves its operands as they are (an in-place op works on a copy
                                  and returns it as an output)
    owners                        for every operand and every output an integer tensor of the same shape: the image (request)
                                  each element belongs to, -1 for shared elements (weights, tables, scalars)
    j                             the victim: the image whose elements are overwritten

`check_isolated` (a) runs the benign operands twice and requires equal bits, so that a non-deterministic route is never reported
as a leak, (b) runs once per hostile pattern at the same shapes, strides and launch knobs, (c) requires every output element not
owned by j to hold the bits of the benign run, under every pattern, and (d) under `nan` requires every output element owned by j
to be NaN - a kernel that turns garbage into plausible numbers hides a diverged request from its user - unless the case names
another contract for that output (`victim_rules`).  The contracts the case table asserts instead of "all NaN":

    image_finish, latent_preview      NaN -> 0 (the bytes of a picture)
    image_prepare's mask output       a compare: 0 or 1 whatever the mask holds
    ip_xattn_add                      with the victim's io kept benign: queries of weight 0 are not written and keep their bits
    add_rows_gated, closed gate       with the victim's x kept benign: the row keeps x's bits, the features are not read
    t_buf, sigma_groups               made of by-value records alone: the benign bits (a `None` rule)

Hostile values go into floating-point operands only (activations and state): never into index tensors, gates, records or tables
the host reads, so no hostile value is ever an address.

A plain module (no fixtures, no conftest, nothing of the GPU library): tests/test_isolation_host.py runs it on CPU restatements,
tests/test_isolation_gpu.py on the kernels.
"""
import torch

PATTERNS = ("nan", "inf", "max", "seam")
F16_MAX = 65504.0
_INT_OF = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


class Leak(AssertionError):
    """an output element of another image changed with the victim's data"""


class Swallowed(AssertionError):
    """an output element of the victim is not NaN although every element the victim owns is"""


class Unrepeatable(AssertionError):
    """two runs on the same benign operands gave different bits"""


def bits(t):
    """the elements of `t` as integers of the same width (integer and bool tensors as they are)"""
    t = t.contiguous()
    return t.view(_INT_OF[t.dtype]) if t.dtype in _INT_OF else t


def owner_rows(B, shape, dim=0, per_image=None):
    """an owner map of `shape` whose index along `dim` names the image: index i belongs to image i // per_image
    (per_image = shape[dim] // B by default: B equal runs of rows)"""
    n = shape[dim]
    per_image = n // B if per_image is None else per_image
    if per_image * B != n:
        raise ValueError(f"owner_rows: {n} rows are not {B} images of {per_image}")
    view = [1] * len(shape)
    view[dim] = n
    return (torch.arange(n) // per_image).view(view).expand(shape).contiguous()


def shared(shape):
    """the owner map of a tensor every image reads (weights, bias, tables): -1 everywhere"""
    return torch.full(tuple(shape), -1, dtype=torch.int64)


def check_owner_map(name, t, owner, B, j, must_own):
    """every element has an owner in [0, B) or is shared; with must_own the victim owns something"""
    if tuple(owner.shape) != tuple(t.shape):
        raise ValueError(f"{name}: owner map {tuple(owner.shape)} for a tensor {tuple(t.shape)}")
    if owner.dtype not in (torch.int64, torch.int32) or int(owner.min()) < -1 or int(owner.max()) >= B:
        raise ValueError(f"{name}: owners must be integers in [-1, {B})")
    if must_own and not bool((owner == j).any()):
        raise ValueError(f"{name}: the victim {j} owns nothing of it")


def seam_mask(owner, j, axis):
    """the victim's elements in its first and last row along `axis`: those next to images j - 1 and j + 1"""
    mine = owner == j
    if not bool(mine.any()):
        return mine
    other = [d for d in range(owner.dim()) if d != axis]
    along = mine.any(dim=other) if other else mine
    idx = torch.nonzero(along).flatten()
    edge = torch.zeros_like(along)
    edge[idx[0]] = True
    edge[idx[-1]] = True
    view = [1] * owner.dim()
    view[axis] = owner.shape[axis]
    return mine & edge.view(view)


def default_seam_axis(owner, j):
    """dimension 0 where the victim holds several rows of it ([M, K] rows), else dimension 1 ([B, L, C] tokens).  An operand with
    ONE flat row per image ([slots, chw] latents, [B, C] embedding rows) has no row, pixel row or token inside an image: its seam
    is then the first and last ELEMENT of the victim's row - the two elements that lie next to images j - 1 and j + 1 in memory"""
    mine = owner == j
    if owner.dim() < 2:
        return 0
    rows = mine.reshape(owner.shape[0], -1).any(1)
    return 0 if int(rows.sum()) > 1 else 1


def hostile(t, owner, j, pattern, axis=None):
    """a copy of `t` with the elements image j owns overwritten by `pattern`"""
    if pattern not in PATTERNS:
        raise ValueError(f"pattern {pattern!r}: one of {PATTERNS}")
    owner = owner.to(t.device)
    out = t.clone()
    mine = owner == j
    if pattern == "seam":
        out[seam_mask(owner, j, default_seam_axis(owner, j) if axis is None else axis)] = float("nan")
    elif pattern == "max":
        n = int(mine.sum())
        sign = 1.0 - 2.0 * (torch.arange(n, device=t.device) % 2).to(t.dtype)
        out[mine] = sign * F16_MAX
    else:
        out[mine] = float(pattern)
    return out


def is_activation(t, owner):
    """an operand hostile data may touch: floating point, with elements that belong to single images"""
    return t.is_floating_point() and bool((owner >= 0).any())


def _first_difference(a, b, where):
    idx = torch.nonzero((bits(a) != bits(b)) & where.to(a.device))
    return int(idx.shape[0]), tuple(idx[0].tolist())


def check_isolated(run, operands, owners, j, *, B=None, seam_axes=None, victim_rules=None, patterns=PATTERNS, frozen=()):
    """(a) - (d) of the module docstring; returns {pattern: outputs} with "benign" among the keys.

    seam_axes      {operand: dimension whose first / last index of the victim is the seam}; default_seam_axis otherwise
    victim_rules   {output: rule(benign, got, mine)} replaces "all NaN" for that output under the `nan` pattern: a contract of
                   its own, asserted by the rule; None as the rule: the output does not depend on the victim's values at all
                   (it comes from by-value records) and keeps its benign bits
    frozen         operands that stay benign although the victim owns elements of them (gates, rows the host reads)
    """
    seam_axes, victim_rules = seam_axes or {}, victim_rules or {}
    if B is None:
        B = 1 + max(int(o.max()) for o in owners.values())
    touched = [n for n, t in operands.items() if n not in frozen and is_activation(t, owners[n])]
    for name, t in operands.items():
        check_owner_map(name, t, owners[name], B, j, must_own=name in touched)
    if not touched:
        raise ValueError("no operand for hostile data")
    first = run({n: t.clone() for n, t in operands.items()})
    again = run({n: t.clone() for n, t in operands.items()})
    for name, out in first.items():
        if name not in owners:
            raise ValueError(f"output {name}: no owner map")
        check_owner_map(name, out, owners[name], B, j, must_own=False)
        if not torch.equal(bits(out), bits(again[name])):
            raise Unrepeatable(f"{name}: two benign runs differ - not a case for bit comparison")
    results = {"benign": first}
    for pattern in patterns:
        ops_h = {n: hostile(t, owners[n], j, pattern, seam_axes.get(n)) if n in touched else t.clone() for n, t in operands.items()}
        got = run(ops_h)
        results[pattern] = got
        for name, out in got.items():
            others = owners[name] != j
            if not torch.equal(bits(out)[others.to(out.device)], bits(first[name])[others.to(out.device)]):
                count, at = _first_difference(out, first[name], others)
                raise Leak(f"{pattern}: output {name}: {count} elements of other images changed, first at {at} "
                           f"(owner {int(owners[name][at])}): {first[name][at].item()} -> {out[at].item()}")
            if pattern != "nan":
                continue
            mine = (owners[name] == j).to(out.device)
            if name in victim_rules:
                rule = victim_rules[name]
                if rule is None:
                    if not torch.equal(bits(out), bits(first[name])):
                        raise Leak(f"nan: output {name} is made of records alone and changed")
                else:
                    rule(first[name], out, mine)
            elif not bool(torch.isnan(out[mine]).all()):
                finite = int((~torch.isnan(out[mine])).sum())
                raise Swallowed(f"nan: output {name}: {finite} of the victim's {int(mine.sum())} elements are not NaN")
    return results
