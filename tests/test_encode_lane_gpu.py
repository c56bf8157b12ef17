"""Pixel inputs on the encode lane of the continuous batcher on the MI355X (`-m gpu`): dsc_image_prepare and
dsc_latent_start_rows against the eager chains they replace (ops.image_prepare_torch / ops.latent_start_torch, on the device) bit
for bit - every byte, every fp16 logvar, the edges of their launches, idle rows - and the lane of `pipe.serve(..., encode=True)`
against the flagless batcher's inline path, the eager encoder and the fp32 oracle (oracle/vae_ref.py)."""
import numpy as np
import pytest
import torch

from test_inpaint_unet_gpu import nine  # noqa: F401  (the tiny 9-channel pipeline with a tiny VAE)
from test_serving_img_gpu import tiny  # noqa: F401  (the tiny 4-channel pipeline with a tiny VAE)

pytestmark = pytest.mark.gpu
SIZE, STEPS = 128, 5
POISON = 7.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from diffusionspatialcontrol_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------- dsc_image_prepare
def _prepare(ops, images, masks, reps):
    """one launch over these rows (a mask of None: the image only) -> per row (image, masked, latent mask), with the rows'
    destinations cut from poisoned buffers one row longer than needed (the extra row must stay poison)"""
    n = len(images)
    H, W = (images[0].shape[0], images[0].shape[1]) if images[0].dtype == torch.uint8 else images[0].shape[1:]
    out_i = torch.full((n + 1, 3, H, W), POISON, dtype=torch.float16, device="cuda")
    out_m = torch.full((n + 1, 3, H, W), POISON, dtype=torch.float16, device="cuda")
    out_l = torch.full((n + 1, 4, H // 8, W // 8), POISON, dtype=torch.float16, device="cuda")
    rows = []
    for j in range(n):
        row = {"image": images[j].cuda(), "out_image": out_i[j]}
        if masks[j] is not None:
            row.update(mask=masks[j].cuda(), out_masked=out_m[j], out_mask=out_l[j, :reps[j]])
        rows.append(row)
    ops.image_prepare(rows, int(H), int(W))
    torch.cuda.synchronize()
    for buf in (out_i, out_m, out_l):
        assert (buf[n] == POISON).all()
    got = []
    for j in range(n):
        if masks[j] is None:
            assert (out_m[j] == POISON).all() and (out_l[j] == POISON).all()
            got.append((out_i[j], None, None))
        else:
            assert (out_l[j, reps[j]:] == POISON).all()
            got.append((out_i[j], out_m[j], out_l[j, :reps[j]]))
    return got


def _same(ops, got, image, mask, rep, what):
    ref = ops.image_prepare_torch(image.cuda(), None if mask is None else mask.cuda(), rep)
    for name, g, r in zip(("image", "masked", "latent mask"), got, ref):
        assert (g is None) == (r is None), (what, name)
        if g is not None:
            assert g.shape == r.shape and torch.equal(_bits(g), _bits(r)), (what, name)


def test_image_prepare_every_byte(ops):
    """every byte value in every channel and as a mask value (at every pixel: the masked image; at the sampled pixels (8 i, 8 j):
    the latent mask), and float masks at 0.5 and its two fp32 neighbours"""
    H, W = 8, 2048
    p = torch.arange(H * W)
    img = torch.stack([(p + 85 * c) % 256 for c in range(3)], dim=1).to(torch.uint8).view(H, W, 3)
    every = (p % 256).to(torch.uint8).view(H, W)                                # each value under pixels of every sign
    sampled = (p // 8 % 256).to(torch.uint8).view(H, W)                         # pixel (0, 8 j) holds byte j
    for c in range(3):
        assert img[..., c].unique().numel() == 256
    got = _prepare(ops, [img, img], [every, sampled], [4, 1])
    _same(ops, got[0], img, every, 4, "every")
    _same(ops, got[1], img, sampled, 1, "sampled")
    lm = got[1][2][0, 0].cpu()                                                  # latent row 0: bytes 0..255
    assert lm.tolist() == [0.0] * 128 + [1.0] * 128                             # the flip is between 127 and 128
    masked = got[0][1].cpu()
    kept = (every < 128)[None].expand(3, H, W)
    assert torch.equal(_bits(masked[kept]), _bits(got[0][0].cpu()[kept])) and (masked[~kept] == 0).all()
    assert (_bits(masked[~kept]) == -32768).any() and (_bits(masked[~kept]) == 0).any()     # both signs of zero
    edge = torch.tensor([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))])
    fmask = edge[(p // 8) % 3].view(H, W).contiguous()
    fimg = (torch.rand(3, H, W, generator=_gen(1)) * 2 - 1)
    gotf = _prepare(ops, [fimg], [fmask], [1])
    _same(ops, gotf[0], fimg, fmask, 1, "float edges")
    assert gotf[0][2][0, 0, :3].tolist() == [1.0, 0.0, 1.0]


def _masks(H, W, kind):
    """float32 [H, W] masks whose content shows a wrong gather: ones only at the sampled pixels (8 i, 8 j), zeros only there, ones
    only one pixel off (8 i + 1, 8 j), and a random one"""
    m = torch.zeros(H, W)
    if kind == "on":
        m[::8, ::8] = 1.0
    elif kind == "off":
        m = torch.ones(H, W)
        m[::8, ::8] = 0.0
    elif kind == "beside":
        m[1::8, ::8] = 1.0
    else:
        m = torch.rand(H, W, generator=_gen(H * W))
    return m


@pytest.mark.parametrize("bytes_in", [True, False])
@pytest.mark.parametrize("H, W", [(8, 8), (8, 24), (24, 16), (40, 8)])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_image_prepare_shapes(ops, n, H, W, bytes_in):
    """both input kinds at sizes of one piece, rows that are no multiple of a piece, several latent rows; per row another rep /
    no mask at all; the comparison is on the bits (a repainted negative pixel is -0.0)"""
    for kind in ("on", "off", "beside", "random"):
        images, masks, reps = [], [], []
        for j in range(n):
            g = _gen(100 * n + 10 * j + H)
            if bytes_in:
                images.append(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8))
                m = _masks(H, W, kind)
                masks.append((m * 255).to(torch.uint8) if kind != "random" else torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8))
            else:
                images.append(torch.rand(3, H, W, generator=g) * 2 - 1)
                masks.append(_masks(H, W, kind))
            reps.append(4 if j % 2 == 0 else 1)
        if n == 3:
            masks[2] = None                                                     # a row that asks for its image only
        got = _prepare(ops, images, masks, reps)
        for j in range(n):
            _same(ops, got[j], images[j], masks[j], reps[j], (kind, j))
        lm = got[0][2].cpu()
        if kind == "on":
            assert (lm == 1).all()
        elif kind in ("off", "beside"):
            assert (lm == 0).all()
        if kind == "off":                                                       # everything but the sampled pixels is repainted
            assert (_bits(got[0][1].cpu()) == -32768).any()


def test_image_prepare_idle_rows(ops):
    """a row of None and a row whose destinations are all absent are neither read nor written"""
    H, W = 16, 24
    img = torch.randint(0, 256, (H, W, 3), generator=_gen(2), dtype=torch.uint8).cuda()
    mask = torch.randint(0, 256, (H, W), generator=_gen(3), dtype=torch.uint8).cuda()
    out = torch.full((4, 3, H, W), POISON, dtype=torch.float16, device="cuda")
    lm = torch.full((4, 1, H // 8, W // 8), POISON, dtype=torch.float16, device="cuda")
    rows = [None, {"image": img, "mask": mask, "out_masked": out[1], "out_mask": lm[1]}, {"image": img, "mask": mask}, None]
    ops.image_prepare(rows, H, W)
    torch.cuda.synchronize()
    ref = ops.image_prepare_torch(img, mask, 1)
    assert torch.equal(_bits(out[1]), _bits(ref[1])) and torch.equal(lm[1], ref[2])
    for j in (0, 2, 3):
        assert (out[j] == POISON).all() and (lm[j] == POISON).all()
    ops.image_prepare([{"image": img, "mask": mask}], H, W)                     # nobody asks for anything: no launch, no error


def test_image_prepare_refusals(ops):
    ok = torch.zeros(16, 16, 3, dtype=torch.uint8, device="cuda")
    okf = torch.zeros(3, 16, 16, device="cuda")
    mask = torch.zeros(16, 16, dtype=torch.uint8, device="cuda")
    out = torch.zeros(3, 16, 16, dtype=torch.float16, device="cuda")
    lm = torch.zeros(4, 2, 2, dtype=torch.float16, device="cuda")
    bad = [
        (ValueError, [{"image": ok, "out_image": out}], 16, 12),                                   # a side that is no multiple of 8
        (ValueError, [{"image": ok, "out_image": out}] * 17, 16, 16),                              # more than 16 rows
        (ValueError, [], 16, 16),
        (ValueError, [{"image": ok[:8], "out_image": out}], 16, 16),                               # wrong shape
        (ValueError, [{"image": okf.permute(0, 2, 1), "out_image": out}], 16, 16),                 # not contiguous
        (TypeError, [{"image": ok.to(torch.int32), "out_image": out}], 16, 16),                    # wrong dtype
        (TypeError, [{"image": ok, "out_image": out.float()}], 16, 16),
        (ValueError, [{"image": ok, "out_image": out.cpu()}], 16, 16),                             # another device
        (ValueError, [{"image": ok, "out_masked": out}], 16, 16),                                  # a mask output without a mask
        (ValueError, [{"mask": mask, "out_image": out}], 16, 16),                                  # an image output without an image
        (ValueError, [{"image": ok, "mask": mask[:8], "out_masked": out}], 16, 16),
        (ValueError, [{"image": ok, "mask": mask, "out_mask": lm[:2]}], 16, 16),                   # rep is 1 or 4
        (ValueError, [{"image": ok, "mask": mask, "out_mask": torch.zeros(1, 2, 4, dtype=torch.float16, device="cuda")}], 16, 16),
        (ValueError, [{"image": ok, "mask": mask, "out_image": out, "out_masked": out}], 16, 16),  # one destination twice
        (ValueError, [{"image": ok, "out_image": out, "gamma": 2.2}], 16, 16),
    ]
    for error, rows, H, W in bad:
        with pytest.raises(error, match="image_prepare"):
            ops.image_prepare(rows, H, W)
    from diffusionspatialcontrol_amd import _lib
    with pytest.raises(_lib.DscLibraryError):
        ops.image_prepare([{"image": ok.cpu(), "out_image": out.cpu()}], 16, 16)                   # no CPU fallback
    torch.cuda.synchronize()
    assert not out.any() and not lm.any()


# ----------------------------------------------------------------------------- dsc_latent_start_rows
def _start_rows(ops, moments, specs, scaling, sig0):
    """one launch over `specs` - per row None or (kind, moments row, eps, noise, keep?, keep_noise?) - with destinations cut from
    poisoned buffers -> (start, keep, keep_noise) buffers [n + 1, 4, h, w]"""
    n, shape = len(specs), (4,) + tuple(moments.shape[2:])
    bufs = [torch.full((n + 1,) + shape, POISON, dtype=torch.float16, device="cuda") for _ in range(3)]
    rows = []
    for j, spec in enumerate(specs):
        if spec is None:
            rows.append(None)
            continue
        kind, k, eps, noise, keep, keep_noise = spec
        form, coef = ops.start_form(kind, sig0)
        row = {"form": form, "row": k, "eps": eps, "scaling": scaling, "coef": coef}
        if kind != "masked":
            row.update(noise=noise, start=bufs[0][j])
        if keep:
            row["keep"] = bufs[1][j]
        if keep_noise:
            row["keep_noise"] = bufs[2][j]
        rows.append(row)
    ops.latent_start(moments, rows)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("misaligned", [False, True])
def test_latent_start_every_logvar(ops, misaligned):
    """every fp16 bit pattern of logvar that is not a NaN (63490 of them, both infinities in), crossed with a handful of mean /
    eps values, against the eager chain on the device, bit for bit: decides whether the device's expf rounds as torch's half exp.
    `misaligned`: the posterior draw sits 2 bytes off a 16-byte boundary, so the sweep runs the element path's copy of the arithmetic"""
    pats = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16)
    pats = pats[~torch.isnan(pats)]
    assert pats.numel() == 65536 - 2046 and torch.isinf(pats).sum() == 2
    vals = torch.tensor([0.0, -0.0, 65504.0, -1.5, 0.37], dtype=torch.float16)
    pairs = [(a, b) for a in range(5) for b in range(5)]
    total = pats.numel() * len(pairs)
    w = -(-total // 4)
    w += -w % 2                                                                  # (4 w a multiple of 8: whole vectors)
    mean, logvar, eps = (torch.zeros(4 * w, dtype=torch.float16) for _ in range(3))
    for i, (a, b) in enumerate(pairs):
        sl = slice(i * pats.numel(), (i + 1) * pats.numel())
        mean[sl], logvar[sl], eps[sl] = vals[a], pats, vals[b]
    moments = torch.cat([mean.view(1, 4, 1, w), logvar.view(1, 4, 1, w)], dim=1).cuda()
    if misaligned:
        eps = torch.cat([eps[:1], eps, eps[:7]]).cuda()[1:1 + 4 * w].view(1, 4, 1, w)
        assert eps.data_ptr() % 16 == 2
    else:
        eps = eps.view(1, 4, 1, w).cuda()
    noise = torch.randn(1, 4, 1, w, generator=_gen(6)).half().cuda()
    sig0 = torch.tensor(2.7).half().cuda()
    scaling = 0.18215
    ref_lat, ref_start = ops.latent_start_torch(moments, eps, noise, scaling, "img2img", sig0)
    start, keep, _ = _start_rows(ops, moments, [("img2img", 0, eps, noise, True, False)], scaling, sig0)
    assert not torch.isnan(ref_lat).any()
    bad = (_bits(keep[0]) != _bits(ref_lat[0])).sum().item()
    print(f"latent_start over every logvar: {bad} of {total} latents differ from the eager chain")
    assert bad == 0
    assert torch.equal(_bits(start[0]), _bits(ref_start[0]))
    assert (start[1] == POISON).all() and (keep[1] == POISON).all()


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("h, w", [(1, 1), (3, 5), (16, 16)])
def test_latent_start_kinds_and_shapes(ops, h, w, misaligned):
    """every kind in one launch with an idle row between them, at 4, 60 and 1024 halfs per row (a single tail, a row that is no
    multiple of 8 halfs, whole vectors) and, `misaligned`, with sources 2 bytes off a 16-byte boundary (the element path)"""
    g = _gen(h * w)
    moments = (torch.randn(4, 8, h, w, generator=g) * 1.5).half().cuda()

    def draw():
        if not misaligned:
            return torch.randn(1, 4, h, w, generator=g).half().cuda()
        flat = torch.randn(8 + 4 * h * w, generator=g).half().cuda()
        return flat[1:1 + 4 * h * w].view(4, h, w)

    sig0 = torch.tensor(5.1).half().cuda()
    scaling = 0.18215
    specs = [("img2img", 2, draw(), draw(), False, False), None, ("inpaint", 0, draw(), draw(), True, True),
             ("inpaint_max", 3, draw(), draw(), True, False), ("masked", 1, draw(), None, True, False)]
    start, keep, keep_noise = _start_rows(ops, moments, specs, scaling, sig0)
    for j, spec in enumerate(specs):
        if spec is None:
            assert (start[j] == POISON).all() and (keep[j] == POISON).all() and (keep_noise[j] == POISON).all()
            continue
        kind, k, eps, noise, kp, kn = spec
        lat, st = ops.latent_start_torch(moments[k:k + 1], eps.reshape(1, 4, h, w),
                                         None if noise is None else noise.reshape(1, 4, h, w), scaling, kind, sig0)
        if st is None:
            assert (start[j] == POISON).all()
        else:
            assert torch.equal(_bits(start[j]), _bits(st[0])), (kind, "start")
        assert torch.equal(_bits(keep[j]), _bits(lat[0])) if kp else (keep[j] == POISON).all(), (kind, "keep")
        assert torch.equal(keep_noise[j], noise.reshape(4, h, w)) if kn else (keep_noise[j] == POISON).all(), (kind, "noise")
    for buf in (start, keep, keep_noise):
        assert (buf[len(specs)] == POISON).all()


def test_latent_start_refusals(ops):
    mom = torch.zeros(2, 8, 4, 4, dtype=torch.float16, device="cuda")
    t = lambda: torch.zeros(4, 4, 4, dtype=torch.float16, device="cuda")       # noqa: E731
    eps, noise, start, keep = t(), t(), t(), t()
    ok = {"form": "add", "row": 0, "eps": eps, "noise": noise, "scaling": 0.18215, "coef": 1.0, "start": start}
    with pytest.raises(TypeError, match="latent_start"):
        ops.latent_start(mom.float(), [ok])
    for moments in (mom[:, :4], mom.permute(0, 1, 3, 2)[:, :, :, ::2]):
        with pytest.raises(ValueError, match="latent_start"):
            ops.latent_start(moments, [ok])
    bad = [[], [ok] * 17, [dict(ok, row=2)], [dict(ok, row=-1)], [dict(ok, row=True)], [dict(ok, form="img2img")],
           [dict(ok, eps=None)], [dict(ok, noise=None)], [dict(ok, start=None)], [dict(ok, eps=eps[:2])],
           [dict(ok, start=start.cpu())], [dict(ok, keep=start)], [dict(ok, keep=keep, keep_noise=keep)],
           [{"form": "none", "row": 0, "eps": eps}], [{"form": "none", "row": 0, "eps": eps, "keep": keep, "noise": noise}],
           [dict(ok, eps=torch.zeros(4, 4, 8, dtype=torch.float16, device="cuda")[..., ::2])], [dict(ok, sigma=1.0)]]
    for rows in bad:
        with pytest.raises(ValueError, match="latent_start"):
            ops.latent_start(mom, rows)
    with pytest.raises(TypeError, match="latent_start"):
        ops.latent_start(mom, [dict(ok, noise=noise.float())])
    from diffusionspatialcontrol_amd import _lib
    with pytest.raises(_lib.DscLibraryError):
        ops.latent_start(mom.cpu(), [ok])                                        # no CPU fallback
    torch.cuda.synchronize()
    assert not start.any() and not keep.any()


# ----------------------------------------------------------------------------- the lane
def _serve(pipe, **kw):
    return pipe.serve(SIZE, SIZE, max_batch=2, buckets=(1, 2), **kw).warm()


def _staggered(b, reqs):
    """four requests on two slots, joining at different steps (tests/test_image_serving_gpu.py's schedule) -> their results"""
    futs = [b.submit(reqs[0])]
    b.step()
    futs.append(b.submit(reqs[1]))
    b.step()
    b.step()
    futs.append(b.submit(reqs[2]))
    futs.append(b.submit(reqs[3]))
    b.run_until_idle()
    return [f.result(timeout=0) for f in futs]


def _pixels(i):
    """request i's image in another form each: a PIL image, an np.uint8 array (`_image_tensor`'s numpy rule takes array values as
    they are, so it holds zeros and ones), a float tensor in [-1, 1], a PIL image again"""
    from PIL import Image
    g = _gen(500 + i)
    if i % 2 == 0:
        return Image.fromarray(torch.randint(0, 256, (SIZE, SIZE, 3), generator=g, dtype=torch.uint8).numpy())
    if i == 1:
        return torch.randint(0, 2, (SIZE, SIZE, 3), generator=g, dtype=torch.uint8).numpy()
    return torch.rand(1, 3, SIZE, SIZE, generator=g) * 2 - 1


def _mask(i):
    """request i's mask in another form each: a float tensor, a PIL image of every grey level, a numpy float array"""
    from PIL import Image
    m = torch.zeros(SIZE, SIZE)
    m[16 * i:16 * i + 64, 24:104] = 1.0
    if i % 3 == 0:
        return m[None, None]
    if i % 3 == 1:
        ramp = torch.arange(SIZE * SIZE).view(SIZE, SIZE) % 256
        return Image.fromarray(torch.where(m > 0, ramp, 0 * ramp).to(torch.uint8).numpy(), "L")
    return m.numpy()


def _lane_requests(env, case):
    """the four requests of `case`, built anew on every call: each brings its own seeded CPU generator"""
    reqs = []
    for i in range(4):
        r = dict(env.base, image=_pixels(i), num_inference_steps=STEPS + i % 2, generator=_gen(900 + i))
        if case["mask"]:
            r["mask_image"] = _mask(i)
        if case["strength"] is not None:
            r["strength"] = case["strength"]
        if case.get("mil"):
            r["masked_image_latents"] = (torch.randn(1, 4, 16, 16, generator=_gen(700 + i)) * 0.7).half()
        if i == 3 and not case.get("mil"):
            r["latents"] = torch.randn(1, 4, 16, 16, generator=_gen(800)).half()       # the noise given, not drawn
        reqs.append(r)
    return reqs


CASES = {"img2img 0.6": dict(mask=False, strength=0.6, rows=1),
         "inpaint 1.0": dict(mask=True, strength=1.0, rows=1),
         "inpaint 0.6": dict(mask=True, strength=0.6, rows=1),
         "inpaint_unet": dict(mask=True, strength=None, rows=2, nine=True),
         "inpaint_unet 0.6 + masked_image_latents": dict(mask=True, strength=0.6, rows=1, nine=True, mil=True)}


@pytest.mark.parametrize("name", list(CASES))
def test_lane_equals_inline_at_encode_batch_1(ops, tiny, nine, name):    # noqa: F811
    """pixels in (PIL, np.uint8, float tensor), seeded CPU generators: the lane batcher's results are the flagless batcher's, bit
    for bit; nothing is captured after warm(), the counters count lane rows, and the lane ends empty"""
    case = CASES[name]
    env = nine if case.get("nine") else tiny
    kw = {"inpaint_unet": True} if case.get("nine") else {}
    inline = _staggered(_serve(env.pipe, **kw), _lane_requests(env, case))
    b = _serve(env.pipe, encode=True, encode_batch=1, **kw)
    got = _staggered(b, _lane_requests(env, case))
    st = b.stats()
    assert st["captures_after_warm"] == 0 and st["leaves"] == 4, st
    assert st["encodes"] == 4 * case["rows"] and st["encode_rows"] == 4 * case["rows"], st
    for i, (g, ref) in enumerate(zip(got, inline)):
        assert torch.isfinite(ref).all() and g.shape == (1, 4, 16, 16)
        assert torch.equal(g, ref), (name, i, (g.float() - ref.float()).abs().max().item())
    assert not torch.equal(got[0], got[2])
    lane = b.exec.enc_lane
    torch.cuda.synchronize()
    lane.reclaim()
    assert not lane.inflight and len(lane.free) == len(lane.ring) and st["queued"] == 0 and st["active"] == 0


def test_two_requests_that_arrive_together_share_one_encode(ops, tiny):    # noqa: F811
    """their start latents are ops.latent_start applied to the eager `vae.encode` of the same two-row batch, bit for bit; and the
    lane's moments stay inside the encoder's bound against the fp32 oracle on the same weights (test_unet_pipeline_gpu.py,
    test_vae_encoder_matches_oracle: 2e-2 of the range max, 3e-3 mean), printed beside the inline path's"""
    from oracle import vae_ref
    pipe = tiny.pipe
    vae = pipe.vae
    images = [torch.rand(1, 3, SIZE, SIZE, generator=_gen(40 + i)) * 2 - 1 for i in range(2)]
    b = _serve(pipe, encode=True, encode_batch=2)
    futs = [b.submit(dict(tiny.base, image=images[i].clone(), strength=0.6, num_inference_steps=STEPS, generator=_gen(60 + i)))
            for i in range(2)]
    records = list(b._queue)
    assert b.step()
    st = b.stats()
    assert st["encodes"] == 1 and st["encode_rows"] == 2 and st["active"] == 2, st
    torch.cuda.synchronize()
    x = torch.cat(images).half().cuda()
    with torch.no_grad():
        moments = vae.encode(x).latent_dist.parameters.contiguous()
    lane_moments = b.exec.enc_lane.st[2]["moments"].clone()
    assert torch.equal(lane_moments, moments)
    rows, want = [], torch.empty(2, 4, 16, 16, dtype=torch.float16, device="cuda")
    for i, r in enumerate(records):
        g = _gen(60 + i)
        eps = torch.randn(1, 4, 16, 16, generator=g, dtype=torch.float16).cuda()
        noise = torch.randn(1, 4, 16, 16, generator=g, dtype=torch.float16).cuda()
        form, coef = ops.start_form("img2img", r.sig[0])
        rows.append({"form": form, "row": i, "eps": eps, "noise": noise, "scaling": vae.config.scaling_factor, "coef": coef,
                     "start": want[i]})
    ops.latent_start(moments, rows)
    torch.cuda.synchronize()
    for i, r in enumerate(records):
        assert torch.equal(r.lat[0], want[i]), i
    sd = {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    with torch.no_grad():
        ref = vae_ref.vae_encode_moments(sd, x.float().cpu(), groups=vae.cfg.norm_num_groups)
        inline = torch.cat([vae.encode(x[i:i + 1]).latent_dist.parameters for i in range(2)]).float().cpu()
    scale = ref.abs().max().item()
    figures = {}
    for what, out in (("lane", lane_moments.float().cpu()), ("inline", inline)):
        figures[what] = ((out - ref).abs().max().item() / scale, (out - ref).abs().mean().item() / scale)
        print(f"encoder moments vs the fp32 oracle, {what}: max {figures[what][0]:.3e}, mean {figures[what][1]:.3e} of the range")
    assert figures["lane"][0] < 2e-2 and figures["lane"][1] < 3e-3, figures
    b.run_until_idle()
    assert all(torch.isfinite(f.result(timeout=0)).all() for f in futs) and b.stats()["captures_after_warm"] == 0


def test_driver_thread_resolves_pixel_requests(tiny):    # noqa: F811
    b = _serve(tiny.pipe, encode=True, encode_batch=2).start()
    try:
        futs = [b.submit(dict(tiny.base, image=_pixels(i), mask_image=_mask(i), strength=0.6, num_inference_steps=STEPS,
                              generator=_gen(70 + i))) for i in range(3)]
        outs = [f.result(timeout=120) for f in futs]
    finally:
        b.stop()
    st = b.stats()
    assert all(o.shape == (1, 4, 16, 16) and torch.isfinite(o).all() for o in outs)
    assert st["encode_rows"] == 3 and st["queued"] == 0 and st["active"] == 0 and st["captures_after_warm"] == 0, st


def test_latent_inputs_never_touch_the_lane(tiny):    # noqa: F811
    def reqs():
        return [dict(tiny.base, image=tiny.lat0.clone(), strength=0.6, num_inference_steps=STEPS, generator=_gen(33)),
                dict(tiny.base, num_inference_steps=STEPS, latents=torch.randn(1, 4, 16, 16, generator=_gen(34)).half()),
                dict(tiny.base, image=tiny.lat0.clone(), mask_image=tiny.mask, num_inference_steps=STEPS, generator=_gen(35)),
                # pixels that sit on the GPU already: the lane's upload starts on the host, so the inline path keeps them
                dict(tiny.base, image=_pixels(3).cuda(), strength=0.4, num_inference_steps=STEPS, generator=_gen(36))]
    inline = _staggered(_serve(tiny.pipe), reqs())
    b = _serve(tiny.pipe, encode=True, encode_batch=2)
    got = _staggered(b, reqs())
    st = b.stats()
    assert st["encodes"] == 0 and st["encode_rows"] == 0 and st["captures_after_warm"] == 0, st
    for i, (g, ref) in enumerate(zip(got, inline)):
        assert torch.equal(g, ref), i


def test_hires_pair_encodes_on_the_base_batcher_only(tiny):    # noqa: F811
    def run(**kw):
        pair = tiny.pipe.serve_hires(SIZE, SIZE, 1.5, max_batch=2, buckets=(1, 2), **kw).warm()
        fut = pair.submit(dict(tiny.base, image=_pixels(2), strength=0.6, num_inference_steps=STEPS, generator=_gen(81),
                               upscale=True, upscale_x=1.5, upscale_denoising_strength=0.5))
        pair.run_until_idle()
        return pair, fut.result(timeout=0)
    plain, ref = run()
    pair, got = run(encode=True, encode_batch=1)
    st = pair.stats()
    assert pair.base.encode and not pair.hires.encode and pair.hires.exec.enc_lane is None
    assert st["base"]["encodes"] == 1 and st["base"]["encode_rows"] == 1 and "encodes" not in st["hires"], st
    assert "encodes" not in plain.stats()["base"]
    assert st["handoffs"] == 1 and st["base"]["captures_after_warm"] == 0 and st["hires"]["captures_after_warm"] == 0
    assert got.shape == (1, 4, 24, 24) and torch.equal(got, ref)


def test_flagless_batcher_serves_pixels_as_before(tiny):    # noqa: F811
    """two runs of the inline path on this tree agree bit for bit, and the flagless batcher has no lane"""
    outs = []
    for _ in range(2):
        b = _serve(tiny.pipe)
        fut = b.submit(dict(tiny.base, image=_pixels(0), mask_image=_mask(0), strength=0.6, num_inference_steps=STEPS,
                            generator=_gen(91)))
        b.run_until_idle()
        outs.append(fut.result(timeout=0))
        assert b.exec.enc_lane is None and not b.encode and "encodes" not in b.stats()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
