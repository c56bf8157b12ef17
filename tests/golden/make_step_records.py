"""The host side of the sampler step, recorded without a device: every record the serving batcher hands its executor, and every
sampler launch `_denoise_fused` makes, for the ten fused samplers on the tiny fp16 UNet pipelines (eps and v-prediction) over a
literal fp16-exact schedule.

    python tests/golden/make_step_records.py      (re)writes tests/golden/step_records.json

Run it at the commit whose records are the reference; tests/test_step_records_host.py replays the same cases through the same
recorder and requires equality with the file (floats: equal, or within 2 ulp of double - another machine's libm may round exp /
log / expm1 differently).  The committed file was written at 5dab441 ("Serve prompt strings on a text lane: captured CLIP,
weighting kernel"), the parent of the change that gave a request one record class and one step plan shared with the fused loop.

Only names that exist unchanged before and after are patched, so the script runs on both trees: `get_sigmas`, `_static_step` and
`_record_done` on the pipeline instance, `temb_add_table` on its UNet, `_lib.load_library`, and the five sampler entries of `ops`
(prepare_unet_input, cfg_dpmpp2m_step, cfg_linear_step_rows, cfg_linear_step_rows_cat, cfg_staged_step_rows).

Batcher half ("serve ..." cases): a ServingBatcher on tests/serving_fakes.py::RecordingExec; a row is the executor's `calls` in
full, [launch name, n_src, n_dst, records, known, extras] per transition - every key of every record (`req` by request name, the
noise / temb rows as the fake executor names them).  A hires pair is {"base": calls, "hires": calls}.
Fused half ("fused ..." cases): `_denoise_fused` itself on CPU tensors that claim to be on the GPU, its static step replaced by
CPU buffers with a no-op `run`; a row is [[op name, positional arguments, keyword arguments], records] per call of the five
entries (the records' place among the arguments is marked "records"; None for an entry without records) and ["temb_add_table",
timesteps] for the table of time-embedding rows.  A static buffer is recorded by its name, any other tensor as "T<k>" in order of
first appearance (x, old, mid), a noise row as ["noise", call, image] and an extra-channel row as ["extra", image] (both read
back from the literal values of the tables handed in), a time-embedding row as ["temb", call].

The file is {"floats": [float.hex(), ...], "nodes": [...], "cases": {id: row}}: a float anywhere is "#<k>", an index into
"floats"; a list or dict that does not fit in 8 characters is "@<k>", an index into "nodes" (most occur many times), and a record
(a dict with "mode") is the node {"k": its sorted keys, "v": their values}."""
import dataclasses
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from inputs import FakeTokenizer  # noqa: E402
from serving_fakes import RecordingExec  # noqa: E402

from diffusionspatialcontrol_amd import _lib, ops  # noqa: E402
from diffusionspatialcontrol_amd.modules import samplers_extra_k_diffusion as sx  # noqa: E402
from diffusionspatialcontrol_amd.modules import sampling  # noqa: E402
from diffusionspatialcontrol_amd.modules.serving import HiresPair, ServingBatcher, step_launch  # noqa: E402

PATH = os.path.join(HERE, "step_records.json")
SIGMAS = [14.5, 9.0, 5.5, 3.25, 2.0, 1.25, 0.75, 0.5, 0.25, 0.125]          # fp16-exact, descending
S, CTX, SIZE, LAT = 77, 64, 128, 16
FUNCS = {"euler": sampling.sample_euler, "euler_ancestral": sampling.sample_euler_ancestral, "dpmpp_2m": sampling.sample_dpmpp_2m,
         "dpmpp_2m_sde": sampling.sample_dpmpp_2m_sde, "lcm": sx.sample_lcm, "heun": sampling.sample_heun,
         "dpm_2": sampling.sample_dpm_2, "dpm_2_ancestral": sampling.sample_dpm_2_ancestral,
         "dpmpp_2s_ancestral": sampling.sample_dpmpp_2s_ancestral, "dpmpp_sde": sampling.sample_dpmpp_sde}
READS_ETA = ("euler_ancestral", "dpmpp_2m_sde", "dpm_2_ancestral", "dpmpp_2s_ancestral", "dpmpp_sde")


def variants():
    """(id, family, sampler keys) - eta 0 and 1 where the family reads it (with s_noise 1.1 beside eta 1), both solver types of
    DPM++ 2M SDE"""
    for fam in FUNCS:
        if fam not in READS_ETA:
            yield fam, fam, {}
            continue
        for solver in (("midpoint", "heun") if fam == "dpmpp_2m_sde" else (None,)):
            for eta in (0.0, 1.0):
                kw = {"eta": eta, "s_noise": 1.1 if eta else 1.0}
                if solver is not None:
                    kw["solver_type"] = solver
                yield f"{fam} eta={eta:g}" + (f" {solver}" if solver else ""), fam, kw


_pipes = {}


def pipe(kind):
    """"eps" / "v": the tiny fp16 UNet of tests/test_linear_step_host.py::_pipe; "eps9": the 9-channel one of
    tests/test_inpaint_unet_host.py::_pipe - each with a literal schedule (no transcendental in it)"""
    if kind not in _pipes:
        from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
        from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
        torch.manual_seed(0)
        cfg = dataclasses.replace(UNetConfig.tiny(), in_channels=9) if kind == "eps9" else UNetConfig.tiny()
        sched = SD15Scheduler(prediction_type="v_prediction" if kind == "v" else "epsilon")
        p = StableDiffusionPipeline(None, None, FakeTokenizer(), UNet2DConditionModel(cfg).half(), sched)
        p.get_sigmas = lambda steps, params: torch.tensor(SIGMAS[:steps] + [0.0])
        _pipes[kind] = p
    return _pipes[kind]


# ----------------------------------------------------------------------------- normalisation
def norm(v):
    if isinstance(v, dict):
        return {str(k): norm(e) for k, e in v.items()}
    if isinstance(v, (list, tuple)):
        return [norm(e) for e in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if hasattr(v, "req") and isinstance(v.req, dict):              # a request record
        return v.req.get("name")
    raise TypeError(f"nothing to record for a {type(v).__name__}")


# ----------------------------------------------------------------------------- the batcher half
class GoldenExec(RecordingExec):
    """RecordingExec that keeps every transition in full, the `extras` of a batcher built with `inpaint_unet=True` included"""

    def prepare_image(self, r):
        super().prepare_image(r)
        if r.kind == "inpaint_unet":
            r.extra = ("extra", r.req.get("name"))

    def transition(self, n_src, n_dst, recs, known=None, extras=None):
        self.calls.append(norm([step_launch(recs, known, extras), n_src, n_dst, recs, known, extras]))


def req(name, steps=4, **kw):
    emb = torch.zeros(1, S, CTX, dtype=torch.float16)
    r = {"name": name, "prompt_embeds": emb, "negative_prompt_embeds": emb, "num_inference_steps": steps, "guidance_scale": 7.5,
         "sampler_opt": {"scheduler": "karras"}, "latents": torch.zeros(1, 4, LAT, LAT, dtype=torch.float16)}
    r.update(kw)
    return r


def batcher(kind="eps", size=SIZE, name=None, **kw):
    kw = dict(dict(max_batch=2, buckets=(1, 2)), **kw)
    return ServingBatcher(pipe(kind), size, size, executor=GoldenExec(name), **kw)


def serve_alone(kind, fam, steps, **keys):
    b = batcher(kind, two_call=fam in sampling.TWO_CALL_FAMILY)
    b.submit(req("A", steps, sampler_name=FUNCS[fam].__name__, **keys))
    b.run_until_idle()
    return b.exec.calls


def serve_mixed():
    """Heun (4 steps: 7 model calls) alone for two calls, then DPM++ 2M (2 steps) and Euler a (3 steps) join and leave before it:
    joins, leaves, the bucket up to 4 and back to 1"""
    b = batcher(two_call=True, max_batch=4, buckets=(1, 2, 4))
    b.submit(req("H", 4, sampler_name="sample_heun", guidance_scale=5.0))
    b.step()
    b.step()
    b.submit(req("M", 2))
    b.submit(req("E", 3, sampler_name="sample_euler_ancestral", eta=0.8, s_noise=1.05, guidance_rescale=0.5))
    b.run_until_idle()
    stats = b.stats()
    assert stats["joins"] == stats["leaves"] == 3 and stats["bucket_switches"] >= 2 and stats["staged_transitions"] > 0
    return b.exec.calls


def serve_known():
    """a 4-channel inpainting request (the `known` launch) beside a plain DPM++ 2M request"""
    b = batcher()
    lat, mask = torch.zeros(1, 4, LAT, LAT, dtype=torch.float16), torch.ones(1, 1, SIZE, SIZE)
    b.submit(req("I", 3, image=lat, mask_image=mask))
    b.submit(req("M", 4))
    b.run_until_idle()
    assert any(c[0] == "known" for c in b.exec.calls)
    return b.exec.calls


def serve_cat():
    """a batcher built with `inpaint_unet=True` (the `cat` launch): Euler a with a rescale beside DPM++ 2M at strength 0.5"""
    b = batcher("eps9", inpaint_unet=True)
    keys = dict(image=torch.zeros(1, 4, LAT, LAT, dtype=torch.float16), mask_image=torch.ones(1, 1, SIZE, SIZE),
                masked_image_latents=torch.ones(1, 4, LAT, LAT, dtype=torch.float16))
    b.submit(req("E", 3, sampler_name="sample_euler_ancestral", guidance_rescale=0.5, **keys))
    b.submit(req("M", 4, strength=0.5, **keys))
    b.run_until_idle()
    assert all(c[0] == "cat" for c in b.exec.calls)
    return b.exec.calls


def serve_hires():
    """a hires pair: the first pass on DPM++ 2M, the second (4 steps at strength 0.5) on Euler a"""
    base, hi = batcher(name="base", slot=0), batcher(size=192, name="hires", slot=1)
    pair = HiresPair(base, hi)
    pair.submit(req("U", 4, upscale=True, upscale_x=1.5, upscale_denoising_strength=0.5, sampler_name_hires="sample_euler_ancestral",
                    guidance_rescale=0.7))
    pair.run_until_idle()
    assert hi.exec.calls
    return {"base": base.exec.calls, "hires": hi.exec.calls}


# ----------------------------------------------------------------------------- the fused-loop half
class OnDevice(torch.Tensor):
    """a CPU tensor that claims to be on the GPU: enough for _denoise_fused to take its per-row path"""
    is_cuda = property(lambda self: True)


class FakeLib:
    def __getattr__(self, name):
        return lambda *args: 0


def table(n_calls, n_img, channels=4):
    """a literal noise table [n_calls, n_img, channels, LAT, LAT]: row (i, j) holds the value 8 i + j"""
    v = (8 * torch.arange(n_calls)[:, None] + torch.arange(n_img)[None, :]).to(torch.float16)
    return v[:, :, None, None, None].expand(n_calls, n_img, channels, LAT, LAT).contiguous()


def fused(kind, fam, steps, n_img, noise_images=1, sampler_args=None, rescale=0.0, extra=False, tadd=True):
    """one _denoise_fused call -> [op name, arguments] of every recorded call"""
    p = pipe(kind)
    calls, labels, keep = [], {}, []
    st = {name: torch.zeros(1) for name in ("eps", "x_in", "t", "sigma", "sigma_rows")}
    st["tadd"] = torch.zeros(1) if tadd else None
    for name, t in st.items():
        labels[id(t)] = name
    st.update(run=lambda: None, temb_key=None, temb_tab=None)

    def arg(v, key=None):
        if torch.is_tensor(v):
            if key == "noise":
                return ["noise", int(v.flatten()[0]) // 8, int(v.flatten()[0]) % 8]
            if key == "extras":
                return ["extra", int(v.flatten()[0])]
            if id(v) not in labels:
                labels[id(v)] = f"T{sum(1 for name in labels.values() if name.startswith('T') and name[1:].isdigit())}"
                keep.append(v)
            return labels[id(v)]
        if isinstance(v, dict):
            return {k: arg(e, k) for k, e in v.items()}
        if isinstance(v, (list, tuple)):
            return [arg(e, key) for e in v]
        return norm(v)

    def op(name, params):
        def fn(*args, **kw):
            recs = [v for v in args if isinstance(v, list) and v and isinstance(v[0], dict)]
            calls.append([[name, ["records" if recs and v is recs[0] else arg(v, params[i] if i < len(params) else None)
                                  for i, v in enumerate(args)], {k: arg(v, k) for k, v in kw.items()}], arg(recs[0]) if recs else None])
        return fn

    def temb_add_table(ts):
        calls.append(["temb_add_table", [float(v) for v in ts.tolist()]])
        return [("temb", k) for k in range(len(ts))]

    positional = {"prepare_unet_input": (), "cfg_dpmpp2m_step": (), "cfg_linear_step_rows": (),
                  "cfg_linear_step_rows_cat": (None,) * 8 + ("extras",), "cfg_staged_step_rows": ()}
    patches = [(ops, name, op(name, params)) for name, params in positional.items()]
    patches += [(_lib, "load_library", lambda: FakeLib()), (p, "_static_step", lambda *a, **kw: st),
                (p, "_record_done", lambda st_, device: None), (p.unet, "temb_add_table", temb_add_table)]
    saved = [(obj, name, obj.__dict__.get(name)) for obj, name, _ in patches]
    sig = SIGMAS[:steps] + [0.0]
    n_calls = len(sampling.call_plan(fam, sig)) if fam in sampling.TWO_CALL_FAMILY else steps
    x = torch.zeros(n_img, 4, LAT, LAT, dtype=torch.float16).as_subclass(OnDevice)
    ex = None
    if extra:
        ex = (1 + torch.arange(n_img)).to(torch.float16)[:, None, None, None].expand(n_img, 5, LAT, LAT).contiguous().as_subclass(OnDevice)
    try:
        for obj, name, value in patches:
            setattr(obj, name, value)
        p._denoise_fused(x, torch.tensor(sig, dtype=torch.float16), torch.zeros(2 * n_img, S, CTX, dtype=torch.float16), None, None, 7.5,
                         n_img, {}, 0, 0, slot=0, sampler=None if fam is None else FUNCS[fam], sampler_args=sampler_args,
                         step_noise=table(n_calls, noise_images), guidance_rescale=rescale, extra=ex, two_call=True)
    finally:
        for obj, name, value in saved:
            if isinstance(obj, type(ops)):
                setattr(obj, name, value)
            else:
                delattr(obj, name)
    return calls


# ----------------------------------------------------------------------------- the cases
def cases():
    """(id, function, arguments); txt2img runs 3 and 4 steps, img2img at strength 0.5 the 2-step tail of 4 and the 1-step tail
    of 3"""
    for vid, fam, kw in variants():
        for kind in ("eps", "v"):
            for rescale in (0.0, 0.7):
                for steps in (3, 4):
                    for image in (False, True):
                        keys = dict(kw, guidance_rescale=rescale)
                        if image:
                            keys.update(image=torch.zeros(1, 4, LAT, LAT, dtype=torch.float16), strength=0.5)
                        yield (f"serve {vid} {kind} rescale={rescale:g} steps={steps} {'img2img' if image else 'txt2img'}",
                               serve_alone, (kind, fam, steps), keys)
    yield "serve mixed two_call batch", serve_mixed, (), {}
    yield "serve inpainting, 4 channels (known)", serve_known, (), {}
    yield "serve inpaint_unet (cat)", serve_cat, (), {}
    yield "serve hires pair", serve_hires, (), {}
    for vid, fam, kw in variants():
        args = {k: v for k, v in kw.items() if k != "s_noise"}          # (what _fused_sampler_args hands over: eta, solver_type)
        args.setdefault("solver_type", "midpoint")
        for kind in ("eps", "v"):
            for rescale in (0.0, 0.7):
                for n_img, noise_images in ((1, 1), (2, 1), (2, 2)):
                    yield (f"fused {vid} {kind} rescale={rescale:g} n_img={n_img} noise_images={noise_images}", fused,
                           (kind, fam, 3, n_img), dict(noise_images=noise_images, sampler_args=args, rescale=rescale))
    yield "fused default sampler, no sampler_args", fused, ("eps", None, 4, 1), {}
    yield "fused euler_ancestral, eta not given", fused, ("eps", "euler_ancestral", 4, 2), dict(sampler_args={"solver_type": "midpoint"})
    yield "fused dpmpp_sde, eta not given", fused, ("v", "dpmpp_sde", 4, 1), dict(sampler_args={"solver_type": "midpoint"})
    yield "fused dpmpp_2m no temb table", fused, ("eps", "dpmpp_2m", 3, 1), dict(tadd=False)
    yield "fused heun no temb table", fused, ("eps", "heun", 3, 1), dict(tadd=False)
    yield "fused dpmpp_2m extra=", fused, ("eps", "dpmpp_2m", 3, 2), dict(extra=True)
    yield "fused euler_ancestral extra= rescale", fused, ("eps", "euler_ancestral", 3, 2), dict(extra=True, rescale=0.5, noise_images=2)


def record_all():
    """{case id: row}, floats as they are"""
    out = {}
    for cid, fn, args, kw in cases():
        assert cid not in out, cid
        out[cid] = fn(*args, **kw)
    return out


# ----------------------------------------------------------------------------- the file
def pack(rows):
    floats, nodes = {}, {}

    def intern(v):
        text = json.dumps(v, separators=(",", ":"))
        return v if len(text) <= 8 else f"@{nodes.setdefault(text, len(nodes))}"

    def enc(v):
        if isinstance(v, float):
            return f"#{floats.setdefault(v.hex(), len(floats))}"
        if isinstance(v, list):
            return intern([enc(e) for e in v])
        if isinstance(v, dict) and "mode" in v:                     # a record: its key set is one node, its values another
            keys = sorted(v)
            return intern({"k": intern(keys), "v": [enc(v[k]) for k in keys]})
        if isinstance(v, dict):
            assert set(v) != {"k", "v"}, v
            return intern({k: enc(e) for k, e in v.items()})
        assert not (isinstance(v, str) and v[:1] in "#@"), v
        return v

    cases_ = {cid: enc(row) for cid, row in rows.items()}
    return {"floats": list(floats), "nodes": [json.loads(n) for n in nodes], "cases": cases_}


def unpack(packed):
    floats, nodes, done = [float.fromhex(h) for h in packed["floats"]], packed["nodes"], {}

    def dec(v):
        if isinstance(v, str) and v[:1] == "#":
            return floats[int(v[1:])]
        if isinstance(v, str) and v[:1] == "@":
            if v not in done:
                done[v] = dec(nodes[int(v[1:])])
            return done[v]
        if isinstance(v, list):
            return [dec(e) for e in v]
        if isinstance(v, dict) and set(v) == {"k", "v"}:
            return dict(zip(dec(v["k"]), dec(v["v"])))
        if isinstance(v, dict):
            return {k: dec(e) for k, e in v.items()}
        return v

    return {cid: dec(row) for cid, row in packed["cases"].items()}


def load():
    with open(PATH) as f:
        return unpack(json.load(f))


if __name__ == "__main__":
    rows = record_all()
    packed = pack(rows)
    with open(PATH, "w") as f:
        f.write('{"floats": ' + json.dumps(packed["floats"], separators=(",", ":")) + ',\n"nodes": [\n' +
                ",\n".join(json.dumps(n, separators=(",", ":")) for n in packed["nodes"]) + '\n],\n"cases": {\n' +
                ",\n".join(f"{json.dumps(c)}: {json.dumps(row)}" for c, row in packed["cases"].items()) + "\n}}\n")
    assert load() == json.loads(json.dumps(rows))
    print(len(rows), "cases,", len(packed["floats"]), "floats,", len(packed["nodes"]), "nodes,", os.path.getsize(PATH), "bytes")
