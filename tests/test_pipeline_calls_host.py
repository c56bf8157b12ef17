"""The generation path txt2img, img2img and inpaiting share (model_k_diffusion: _text_and_schedule, _conditioning,
_denoise_and_finish), without a device: every case of tests/golden/make_pipeline_calls.py replayed through the public entries
against the table recorded before the three entries were folded - which core runs, every argument it is handed, what the hooks
are built with, the pipeline's state afterwards and what comes back, or the exception - and the one-site rules of the file."""
import inspect
import json

import pytest

import make_pipeline_calls as calls
from diffusionspatialcontrol_amd.modules import model_k_diffusion as mkd


@pytest.fixture(scope="module")
def recorded():
    return calls.load()


def test_the_cases_are_the_recorded_ones(recorded):
    assert [c[0] for c in calls.cases()] == list(recorded)


@pytest.mark.parametrize("cid", [c[0] for c in calls.cases()])
def test_entry_matches_the_recording(recorded, cid):
    case = next(c for c in calls.cases() if c[0] == cid)
    got = json.loads(json.dumps(calls.record(case)))
    assert got == recorded[cid]


def test_recorder_leaves_the_pipeline_as_it_was():
    p = calls.pipe("eps")
    calls.record(next(c for c in calls.cases() if c[0] == "txt2img"))
    assert not any(name in vars(p) for name in calls.PATCHED)


def test_the_recording_reaches_every_way_through(recorded):
    """both cores from every entry, the hires chain into both, each refusal, and the hooks' step counts of all three entries"""
    seen = {(cid.split()[0], core[0]) for cid, row in recorded.items() for core in row["cores"][:1]}
    assert seen == {(e, c) for e in ("txt2img", "img2img", "inpaiting") for c in ("_denoise_fused", "_denoise_protocol")}
    assert {tuple(core[0] for core in row["cores"]) for row in recorded.values() if len(row["cores"]) == 2} == {
        (a, b) for a in ("_denoise_fused", "_denoise_protocol") for b in ("_denoise_fused", "_denoise_protocol")}
    errors = {row["error"][1][:32] for row in recorded.values() if "error" in row}
    assert len(errors) == 10, errors
    steps = {cid: [h[1][6] if h[0] == "_controlnet_hook" else h[1][5] for h in recorded[cid]["hooks"]]
             for cid in ("txt2img hook", "img2img hook", "inpaiting hook")}
    assert steps == {"txt2img hook": [6, 7], "img2img hook": [4, 4], "inpaiting hook": [6, 4]}       # (n, n + 1), (cut, cut), (n, cut)


def test_each_shared_piece_has_one_site():
    src = inspect.getsource(mkd)
    code = [line.split("#")[0] for line in src.split("\n")]
    count = lambda needle: sum(needle in line for line in code)                            # noqa: E731
    assert count("hires = dict(") == 1
    assert count("self._merge_hooks(") == 1 and count("self.prepare_ip_adapter_image_embeds(") == 1
    assert count("if latent_processing == 1") == 1
    assert count('"inference process timed out"') == 1
    assert count("self._denoise_protocol(") == 1 and count("self._denoise_fused(") == 2
    assert count("encode_prompt_function(") == 1 and "encode_prompt_function" not in inspect.getsource(mkd.StableDiffusionPipeline.txt2img)
