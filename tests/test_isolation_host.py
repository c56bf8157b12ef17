"""tests/isolation.py on the CPU: the detector passes a correct restatement of a GEMM, a 3x3 convolution, a softmax attention and a
GroupNorm under all four hostile patterns, catches four deliberate leaks (no kernel is edited: each mutant is a torch restatement
of a way a batched kernel can go wrong while every neighbour is finite), and the owner maps of every case of
tests/isolation_cases.py cover their tensors exactly.

    mutant                                                   benign neighbours            caught by
    keys of other images masked by `p * 0`, not a select     the correct bits             Leak under nan / inf / seam
    convolution padded from the next image's first row       wrong only at the seam rows  Leak under every pattern
    GroupNorm pivot reduced over the packed buffer           within rounding              Leak under nan / inf
    saturating store through fmax / fmin (drops a NaN)       the correct bits             Swallowed under nan
"""
import pytest
import torch
import torch.nn.functional as F

import isolation as iso
import isolation_cases as IC

B, J = 3, 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------- restatements: correct, and one mutant each
def gemm(o, saturate=False):
    acc = o["x"].float() @ o["w"].float().t() + o["r"].float()
    if saturate:                       # mutant: a "saturating" fp16 store - fmax / fmin return the other operand for a NaN
        big = torch.tensor(iso.F16_MAX)
        acc = torch.fmin(torch.fmax(acc, -big), big)
    return {"out": acc.half()}


def gemm_case():
    g = _gen(1)
    M, N, K = 3 * 5, 8, 16
    o = {"x": torch.randn(M, K, generator=g).half(), "w": (torch.randn(N, K, generator=g) / 4).half(), "r": torch.randn(M, N, generator=g).half()}
    own = {"x": iso.owner_rows(B, (M, K)), "w": iso.shared((N, K)), "r": iso.owner_rows(B, (M, N)), "out": iso.owner_rows(B, (M, N))}
    return o, own


def conv(o, pad_from_neighbour=False):
    x, w = o["x"].float(), o["w"].float()
    if not pad_from_neighbour:
        return {"out": F.conv2d(x, w, padding=1).half()}
    # mutant: the images stacked into one tall image - the row below image b's last row is image b + 1's first, not padding
    Bn, C, H, W = x.shape
    tall = x.permute(1, 0, 2, 3).reshape(1, C, Bn * H, W)
    y = F.conv2d(tall, w, padding=1).reshape(w.shape[0], Bn, H, W).permute(1, 0, 2, 3)
    return {"out": y.half()}


def conv_case():
    g = _gen(2)
    o = {"x": torch.randn(B, 4, 5, 6, generator=g).half(), "w": (torch.randn(3, 4, 3, 3, generator=g) / 6).half()}
    own = {"x": iso.owner_rows(B, (B, 4, 5, 6)), "w": iso.shared((3, 4, 3, 3)), "out": iso.owner_rows(B, (B, 3, 5, 6))}
    return o, own, {"x": 2}


def attention(o, mask_by_multiply=False):
    q, k, v = o["q"].float(), o["k"].float(), o["v"].float()             # [B, L, d], [B, S, d]
    Bn, L, d = q.shape
    S = k.shape[1]
    if not mask_by_multiply:
        p = torch.softmax(q @ k.transpose(1, 2) / d ** 0.5, dim=-1)
        return {"out": (p @ v).half()}
    # mutant: one score tile over the packed keys of every image, foreign keys masked out by a 0 / 1 multiply
    kk, vv = k.reshape(Bn * S, d), v.reshape(Bn * S, d)
    s = q.reshape(Bn * L, d) @ kk.t() / d ** 0.5
    mine = (torch.arange(Bn * L)[:, None] // L == torch.arange(Bn * S)[None, :] // S).float()
    m = torch.where(mine.bool(), s, torch.full_like(s, -1e30)).max(dim=-1, keepdim=True).values
    e = torch.exp(torch.clamp(s - m, max=0.0)) * mine
    p = e / e.sum(-1, keepdim=True)
    return {"out": (p @ (vv * 1.0)).reshape(Bn, L, d).half()}


def attention_case():
    g = _gen(3)
    L, S, d = 6, 5, 8
    o = {"q": torch.randn(B, L, d, generator=g).half(), "k": torch.randn(B, S, d, generator=g).half(), "v": torch.randn(B, S, d, generator=g).half()}
    own = {"q": iso.owner_rows(B, (B, L, d)), "k": iso.owner_rows(B, (B, S, d)), "v": iso.owner_rows(B, (B, S, d)),
           "out": iso.owner_rows(B, (B, L, d))}
    return o, own


def groupnorm(o, packed_pivot=False):
    x = o["x"].float()                                                     # [B, G, n]: one row per (image, group)
    # shifted statistics: var = E[(x - p)^2] - E[x - p]^2 for any pivot p.  Correct: the row's own first element.
    # mutant: the mean of the whole buffer of packed rows - a wave-wide reduction where a per-row one was meant
    p = x.mean() if packed_pivot else x[..., :1]
    c = x - p
    mean_c = c.mean(-1, keepdim=True)
    var = (c * c).mean(-1, keepdim=True) - mean_c * mean_c
    return {"out": ((c - mean_c) * torch.rsqrt(var + 1e-5)).half(), "stats": torch.cat([mean_c + p, var], dim=-1)}


def groupnorm_case():
    o = {"x": (torch.randn(B, 4, 24, generator=_gen(4)) * 1.5 + 0.5).half()}
    own = {"x": iso.owner_rows(B, (B, 4, 24)), "out": iso.owner_rows(B, (B, 4, 24)), "stats": iso.owner_rows(B, (B, 4, 2))}
    return o, own


# ----------------------------------------------------------------------------- the detector
def test_correct_restatements_pass_all_four_patterns():
    o, own = gemm_case()
    assert set(iso.check_isolated(gemm, o, own, J)) == {"benign", *iso.PATTERNS}
    o, own, seams = conv_case()
    iso.check_isolated(conv, o, own, J, seam_axes=seams)
    o, own = attention_case()
    iso.check_isolated(attention, o, own, J)
    o, own = groupnorm_case()
    iso.check_isolated(groupnorm, o, own, J)


def _patterns_caught(run, o, own, kind, **kw):
    caught = set()
    for pattern in iso.PATTERNS:
        try:
            iso.check_isolated(run, o, own, J, patterns=(pattern,), **kw)
        except (iso.Leak, iso.Swallowed) as e:
            if isinstance(e, kind):
                caught.add(pattern)
    return caught


def test_masking_by_a_multiply_is_caught():
    o, own = attention_case()
    mutant = lambda ops: attention(ops, mask_by_multiply=True)
    # with finite neighbours the mutant is the correct kernel, to rounding: no tolerance test sees it
    assert (mutant(o)["out"].float() - attention(o)["out"].float()).abs().max().item() < 2e-3
    assert _patterns_caught(mutant, o, own, iso.Leak) >= {"nan", "inf", "seam"}
    with pytest.raises(iso.Leak, match="other images changed"):
        iso.check_isolated(mutant, o, own, J)


def test_padding_from_the_next_image_is_caught():
    o, own, seams = conv_case()
    mutant = lambda ops: conv(ops, pad_from_neighbour=True)
    good, bad = conv(o)["out"], mutant(o)["out"]
    assert torch.equal(good[:, :, 1:-1], bad[:, :, 1:-1]) and not torch.equal(good, bad)      # wrong at the seam rows only
    assert _patterns_caught(mutant, o, own, iso.Leak, seam_axes=seams) == set(iso.PATTERNS)
    # the seam pattern alone localises it: rows 4 of image 0 and 0 of image 2, nothing else
    got = conv({**o, "x": iso.hostile(o["x"], own["x"], J, "seam", 2)}, pad_from_neighbour=True)["out"]
    changed = (iso.bits(got) != iso.bits(bad)).any(dim=1).any(dim=-1)                          # [B, H]
    assert changed[0].tolist() == [False] * 4 + [True] and changed[2].tolist() == [True] + [False] * 4


def test_a_reduction_over_packed_rows_is_caught():
    o, own = groupnorm_case()
    mutant = lambda ops: groupnorm(ops, packed_pivot=True)
    assert (mutant(o)["out"].float() - groupnorm(o)["out"].float()).abs().max().item() < 2e-3
    assert _patterns_caught(mutant, o, own, iso.Leak) >= {"nan", "inf"}
    with pytest.raises(iso.Leak, match="nan: output"):
        iso.check_isolated(mutant, o, own, J)


def test_a_maximum_that_drops_a_nan_is_caught():
    o, own = gemm_case()
    mutant = lambda ops: gemm(ops, saturate=True)
    assert torch.equal(mutant(o)["out"], gemm(o)["out"])                   # benign: the same bits
    assert _patterns_caught(mutant, o, own, iso.Leak) == set()             # it leaks nothing ...
    assert _patterns_caught(mutant, o, own, iso.Swallowed) == {"nan"}      # ... and hides the diverged request from its user
    with pytest.raises(iso.Swallowed, match="are not NaN"):
        iso.check_isolated(mutant, o, own, J)


def test_a_non_deterministic_route_is_not_reported_as_a_leak():
    o, own = gemm_case()
    calls = []

    def flaky(ops):
        calls.append(1)
        out = gemm(ops)["out"]
        out[0, 0] += len(calls) % 2
        return {"out": out}
    with pytest.raises(iso.Unrepeatable):
        iso.check_isolated(flaky, o, own, J)


def test_patterns_and_contract_rules():
    o, own = gemm_case()
    x, ox = o["x"], own["x"]
    mine = ox == J
    for pattern in ("nan", "inf", "max", "seam"):
        h = iso.hostile(x, ox, J, pattern)
        assert torch.equal(h[~mine], x[~mine]), pattern                    # nobody else's element moves
    assert bool(torch.isnan(iso.hostile(x, ox, J, "nan")[mine]).all()) and bool((iso.hostile(x, ox, J, "inf")[mine] == float("inf")).all())
    mx = iso.hostile(x, ox, J, "max")[mine]
    assert set(mx.tolist()) == {iso.F16_MAX, -iso.F16_MAX} and bool((mx[0::2] == iso.F16_MAX).all()) and bool((mx[1::2] == -iso.F16_MAX).all())
    seam = torch.isnan(iso.hostile(x, ox, J, "seam"))
    assert seam[5].all() and seam[9].all() and int(seam.sum()) == 2 * x.shape[1]     # rows 5 and 9: the first and last of image 1
    # an integer operand, a shared one and a frozen one are never touched
    o2 = {**o, "ids": torch.arange(15)}
    own2 = {**own, "ids": iso.owner_rows(B, (15,))}
    seen = []

    def spy(ops):
        seen.append({n: t.clone() for n, t in ops.items()})
        return gemm(ops)
    iso.check_isolated(spy, o2, own2, J, frozen=("r",))
    assert all(torch.equal(s["ids"], o2["ids"]) and torch.equal(s["w"], o["w"]) and torch.equal(s["r"], o["r"]) for s in seen)
    assert len(seen) == 2 + len(iso.PATTERNS)
    # a contract rule replaces "all NaN" for its output; a None rule means "made of records alone: the benign bits"
    zeroing = lambda ops: {"out": torch.nan_to_num(gemm(ops)["out"], nan=0.0)}
    with pytest.raises(iso.Swallowed):
        iso.check_isolated(zeroing, o, own, J)

    def rule(benign, got, mask):
        assert bool((got[mask] == 0).all())
    iso.check_isolated(zeroing, o, own, J, victim_rules={"out": rule})
    with pytest.raises(iso.Leak, match="records alone"):
        iso.check_isolated(gemm, o, own, J, victim_rules={"out": None})
    # a missing or misshapen owner map is an error of the case, not a pass
    with pytest.raises(ValueError):
        iso.check_isolated(gemm, o, {**own, "x": own["x"][:, :4]}, J)
    with pytest.raises(ValueError):
        iso.check_isolated(gemm, o, {k: v for k, v in own.items() if k != "out"}, J)
    with pytest.raises(ValueError):
        iso.check_isolated(gemm, o, {**own, "x": iso.shared(x.shape), "r": iso.shared(o["r"].shape)}, J)


# ----------------------------------------------------------------------------- the GPU cases' owner maps
ALL = IC.all_cases()


def test_case_ids_are_unique_and_every_family_is_there():
    ids = [c.id for c in ALL]
    assert len(ids) == len(set(ids))
    assert {c.family for c in ALL} >= set(IC.FAMILIES)


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_owner_maps_cover_their_tensors(case):
    """every operand has an owner map of its shape with owners in [0, B) or shared; the victim owns something in every activation,
    and holds a neighbour on both sides; every output has a map; frozen operands and rules name tensors that exist"""
    assert 0 < case.j < case.B - 1
    assert set(case.owners) == set(case.operands) | set(case.outputs), set(case.owners) ^ (set(case.operands) | set(case.outputs))
    touched = 0
    for name, t in case.operands.items():
        own = case.owners[name]
        act = name not in case.frozen and iso.is_activation(t, own)
        iso.check_owner_map(name, t, own, case.B, case.j, must_own=act)
        touched += act
        if act:
            assert {case.j - 1, case.j + 1} <= set(own.unique().tolist()), name      # a neighbour on both sides
            axis = case.seam_axes.get(name, iso.default_seam_axis(own, case.j))
            seam = iso.seam_mask(own, case.j, axis)
            assert bool(seam.any()) and bool((own[seam] == case.j).all()), name
    assert touched >= 1
    for name in case.outputs:                                  # (an output may be shared: a broadcast row, one scalar for all)
        own = case.owners[name]
        assert int(own.min()) >= -1 and int(own.max()) < case.B and bool((own != case.j).any()), name
        assert bool((own == case.j).any()) or bool((own == -1).all()), name
    assert any(bool((case.owners[n] == case.j).any()) for n in case.outputs)
    assert set(case.frozen) <= set(case.operands) and set(case.victim_rules) <= set(case.outputs) and set(case.seam_axes) <= set(case.operands)
