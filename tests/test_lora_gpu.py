"""LoRA merge on the MI355X (`-m gpu`): dsc_lora_merge_f16 through its C-ABI wrapper at the smallest shapes with each edge - against
fp64 under the bound tests/test_lora_host.py shows for the eager fp32 route, exactly on integer / dyadic operands, with gains of
0 over NaN and inf, inside guard bands - and the pipeline surface: captured steps, derived weights and the text encoder's fused
QKV follow a load, a rescale and an unload bit for bit; a serving batcher built before a change refuses to go on.  Every figure
is printed before it is asserted."""
import pytest
import torch
from torch import nn

import guards
import lora_cases as lc
from inputs import FakeTokenizer

from diffusionspatialcontrol_amd import ops
from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _merge(base, adapters, dst=None):
    """one job through ops.lora_merge_ -> dst on the CPU"""
    job, gains = lc.kernel_job(base, adapters, DEV, dst=dst)
    ops.lora_merge_([job], gains)
    return job[0].cpu()


# ----------------------------------------------------------------------------- the kernel through the C ABI
@pytest.mark.parametrize("N,K", lc.SHAPES)
def test_kernel_meets_the_fp32_bound_against_fp64(N, K):
    """every rank set at this shape, rows built so that base + delta cancels included: no element outside
    ulp16(exact) / 2 + (R_pad + 4) 2^-24 (|base| + |gain| sum |up| |down|)"""
    for j, ranks in enumerate(lc.RANK_SETS):
        base, adapters = lc.case(N, K, ranks, seed=100 * lc.SHAPES.index((N, K)) + j)
        got = _merge(base, adapters)
        bad, ulps, share = lc.violations(got, base, adapters)
        e_bad, e_ulps, e_share = lc.violations(ops.lora_merge_eager(torch.empty_like(base), base, adapters), base, adapters)
        print(f"[{N}, {K}] ranks {ranks}: kernel {bad} outside the bound, worst {ulps:.2f} ulp, {100 * share:.2f} % differ from fp64 "
              f"rounded once | eager fp32 {e_bad} outside, worst {e_ulps:.2f} ulp, {100 * e_share:.2f} % differ")
        assert torch.isfinite(got).all()
        assert bad == 0, (N, K, ranks, bad, ulps)


def test_jobs_of_one_launch_equal_the_same_jobs_alone():
    """five jobs of different shapes and ranks in one table: each job's bits are those of the job launched alone, and of the
    same table launched again"""
    cases = [lc.case(N, K, lc.RANK_SETS[(i + 2) % len(lc.RANK_SETS)], seed=500 + i) for i, (N, K) in enumerate(lc.SHAPES)]
    alone = [_merge(base, adapters) for base, adapters in cases]
    jobs, gains = zip(*(lc.kernel_job(base, adapters, DEV) for base, adapters in cases))
    table = ops.LoraMergeTable(list(jobs))
    assert table.tiles == sum(-(-N // 64) * -(-K // 64) for N, K in lc.SHAPES) and len({j[2].shape[1] for j in jobs}) >= 3
    for _ in range(2):
        for j in jobs:
            j[0].fill_(float("nan"))
        ops.lora_merge_(table, list(gains))
        for i, (j, a) in enumerate(zip(jobs, alone)):
            assert torch.equal(j[0].cpu(), a), (i, lc.SHAPES[i])


@pytest.mark.parametrize("N,K", lc.SHAPES)
def test_exact_operands_give_fp64_rounded_once(N, K):
    """integer / dyadic operands: every fp32 sum is exact, so the result is the fp64 value rounded once to fp16 (ties to even) -
    a product counted twice, dropped or taken from a neighbouring row / column / segment changes it"""
    for ranks in lc.RANK_SETS:
        base, adapters = lc.exact_case(N, K, ranks, seed=N + K + sum(ranks))
        want = lc.exact64(base, adapters).half()
        got = _merge(base, adapters)
        assert torch.equal(got, want), (N, K, ranks, int((got != want).sum()))
        assert not torch.equal(want, base)


def test_gains_of_zero_skip_their_segments():
    N, K = 40, 72
    base, adapters = lc.case(N, K, (32, 4), seed=900, cancel=False)
    (u0, d0, g0), (u1, d1, g1) = adapters
    nan_up, inf_down = torch.full_like(u0, float("nan")), torch.full_like(d0, float("inf"))
    # all gains 0, NaN and inf in every factor: dst is base bit for bit
    got = _merge(base, [(nan_up, inf_down, 0.0), (torch.full_like(u1, float("inf")), torch.full_like(d1, float("nan")), 0.0)])
    assert torch.equal(got, base)
    assert torch.equal(_merge(base, [(u0, d0, -0.0), (u1, d1, 0.0)]), base)
    # one adapter's gain 0 (its factors poisoned) gives the other adapter alone, either way round
    assert torch.equal(_merge(base, [(nan_up, inf_down, 0.0), (u1, d1, g1)]), _merge(base, [(u1, d1, g1)]))
    assert torch.equal(_merge(base, [(u0, d0, g0), (torch.full_like(u1, float("nan")), d1, 0.0)]), _merge(base, [(u0, d0, g0)]))
    assert not torch.equal(_merge(base, [(u0, d0, g0)]), base)


@pytest.mark.parametrize("N,K", [(8, 8), (40, 72), (33, 136), (130, 264)])
def test_guard_bands_around_dst_and_base(N, K):
    """dst inside a fenced buffer with a row stride larger than K, at the shapes whose last row tile and last column tile are
    partial: nothing outside dst is written, base is unchanged, and the bits are those of a dense destination"""
    base, adapters = lc.case(N, K, (32, 4), seed=700 + N)
    dense = _merge(base, adapters)
    buf, view = guards.fenced(N, K, ld=K + 24)
    base_buf, base_view = guards.poisoned(base.to(DEV).reshape(1, N * K), lead=64, tail_rows=1)      # dense [N, K], fenced both ends
    (dst, _, up, down), gains = lc.kernel_job(base, adapters, DEV, dst=view)
    up_buf, up_view = guards.poisoned(up.reshape(1, -1), tail_rows=1)
    down_buf, down_view = guards.poisoned(down.reshape(1, -1), tail_rows=1)
    version = buf._version
    ops.lora_merge_([(view, base_view.view(N, K), up_view.view(N, -1), down_view.view(-1, K))], gains)
    torch.cuda.synchronize()
    assert guards.untouched(buf, view)
    assert guards.untouched(base_buf, base_view) and torch.equal(base_view.view(N, K).cpu(), base)
    assert guards.untouched(up_buf, up_view) and guards.untouched(down_buf, down_view)
    assert torch.equal(view.cpu(), dense)                                  # NaN fences around every operand reached no sum
    assert buf._version > version                                          # the written tensor's version counter moved


def test_wrapper_refuses_what_the_entry_does_not_take():
    base, adapters = lc.case(16, 16, (4,), seed=1)
    (dst, b, up, down), gains = lc.kernel_job(base, adapters, DEV)
    with pytest.raises(ValueError):
        ops.lora_merge_([(dst, b, up, down)], gains + [1.0])
    with pytest.raises(TypeError):
        ops.lora_merge_([(dst.float(), b, up, down)], gains)
    with pytest.raises(ValueError):
        ops.lora_merge_([(dst, b, up[:, :16].contiguous(), down[:16].contiguous())], gains)        # rank not padded
    with pytest.raises(Exception, match="dsc_lora_merge_plan"):
        ops.lora_merge_([(b, b, up, down)], gains)                                                 # dst aliases base
    assert ops.lora_merge_takes(dst, [4, 32]) and not ops.lora_merge_takes(dst, [128, 128, 1])
    assert not ops.lora_merge_takes(torch.zeros(16, 12, dtype=torch.float16, device=DEV), [4])      # 24-byte rows
    assert not ops.lora_merge_takes(dst.float(), [4]) and not ops.lora_merge_takes(dst.cpu(), [4])


# ----------------------------------------------------------------------------- the pipeline
def _tiny_pipe(seed=0, text_encoder=None):
    from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
    from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig
    torch.manual_seed(seed)
    cfg = UNetConfig.tiny()
    unet = UNet2DConditionModel(cfg).half().to(DEV)
    return cfg, StableDiffusionPipeline(None, text_encoder, FakeTokenizer(), unet, SD15Scheduler())


def _twin(pipe):
    """a fresh pipeline whose parameters are set to `pipe`'s present (merged) values: no cache, no capture of its own yet"""
    cfg, fresh = _tiny_pipe(99)
    fresh.unet.load_state_dict({k: v.clone() for k, v in pipe.unet.state_dict().items()})
    return fresh


def _targets(unet):
    return [n for n, m in unet.named_modules() if ".attentions." in n or "time_emb" in n
            if isinstance(m, nn.Linear) or (isinstance(m, nn.Conv2d) and tuple(m.kernel_size) == (1, 1))]


def _lora(model, names, prefix, rank, seed):
    g = torch.Generator().manual_seed(seed)
    mods = dict(model.named_modules())
    sd = {}
    for n in names:
        N, K = mods[n].weight.shape[:2]
        head = prefix + n.replace(".", "_")
        conv = mods[n].weight.dim() == 4
        down, up = (0.2 * torch.randn(rank, K, generator=g)).half(), (0.2 * torch.randn(N, rank, generator=g)).half()
        sd[head + ".lora_down.weight"] = down[:, :, None, None] if conv else down
        sd[head + ".lora_up.weight"] = up[:, :, None, None] if conv else up
    return sd


def _generate(pipe, cfg):
    emb = torch.randn(2, 77, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(5)).half()
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(6)).half()
    return pipe.txt2img(None, height=128, width=128, num_inference_steps=3, sampler_name="sample_dpmpp_2m",
                        sampler_opt={"scheduler": "karras"}, prompt_embeds=emb[1:2], negative_prompt_embeds=emb[0:1],
                        output_type="latent", latents=lat)[0].float().cpu()


def test_pipeline_load_rescale_unload_keep_captures_and_derived_weights_current():
    """generate (captures a step, builds the fused QKV, LN-folded weights and the temb table), load, generate: the bits of a
    fresh pipeline on the merged weights - a stale derived weight or a stale capture fails here; likewise after a rescale;
    after the unload, the first generation's bits"""
    cfg, pipe = _tiny_pipe(3)
    original = {n: p.detach().clone() for n, p in pipe.unet.named_parameters()}
    first = _generate(pipe, cfg)
    assert torch.equal(first, _generate(pipe, cfg)) and pipe._graphs
    targets = _targets(pipe.unet)
    sd = _lora(pipe.unet, targets, "lora_unet_", rank=8, seed=21)
    pipe.load_lora_weights(sd, scale=0.8, name="style")
    st = pipe.lora_state()
    print(f"{st['targets']} touched weights, {st['kernel_targets']} on the kernel route, {st['base_bytes']} bytes of bases")
    assert st["targets"] == len(targets) == st["kernel_targets"] and pipe.weights_epoch == 1 and not pipe._graphs
    # the merged weights are the reference's within the kernel's bound
    mods = dict(pipe.unet.named_modules())
    for n in targets[:8]:
        head = "lora_unet_" + n.replace(".", "_")
        ad = [(sd[head + ".lora_up.weight"].flatten(1), sd[head + ".lora_down.weight"].flatten(1), 0.8)]
        bad, ulps, _ = lc.violations(mods[n].weight.detach().flatten(1).cpu(), original[n + ".weight"].flatten(1).cpu(), ad)
        assert bad == 0, (n, ulps)
    merged = _generate(pipe, cfg)
    print(f"LoRA at 0.8 moves the latents by {(merged - first).abs().max().item():.3e}")
    assert not torch.equal(merged, first)
    assert torch.equal(merged, _generate(_twin(pipe), cfg))
    pipe.set_lora_scale(0.5)
    half = _generate(pipe, cfg)
    cfg2, again = _tiny_pipe(3)                                            # a fresh load at 0.5 on the same weights
    again.load_lora_weights(sd, scale=0.5)
    assert pipe.weights_epoch == 2 and not torch.equal(half, merged)
    assert torch.equal(half, _generate(again, cfg2)) and torch.equal(half, _generate(_twin(pipe), cfg))
    pipe.unload_lora_weights()
    assert all(torch.equal(original[n], p) for n, p in pipe.unet.named_parameters())
    assert pipe.weights_epoch == 3 and torch.equal(_generate(pipe, cfg), first)
    assert pipe.lora_state()["base_bytes"] == 0


CLIP_CFG = dict(vocab_size=99, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
                max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2)


def test_text_encoder_round_trip_with_captured_graphs():
    torch.manual_seed(8)
    te = CLIPTextModel(CLIP_CFG).half().to(DEV).eval().enable_graphs(True)
    cfg, pipe = _tiny_pipe(4, text_encoder=te)
    ids = torch.randint(3, 99, (2, 77), generator=torch.Generator().manual_seed(4)).to(DEV)
    assert te.kernel_route(2, 77)
    first = te(ids)[0].cpu()
    captures = te.graph_captures
    assert captures == 1 and torch.equal(te(ids)[0].cpu(), first) and te.graph_captures == 1
    names = [n for n, m in te.named_modules() if isinstance(m, nn.Linear)]
    assert len(names) == 12
    sd = _lora(te, names, "lora_te_text_model_", rank=4, seed=31)
    pipe.load_lora_weights(sd, scale=0.8)
    assert pipe.lora_state()["kernel_targets"] == 12
    merged = te(ids)[0].cpu()
    assert te.graph_captures > captures and not torch.equal(merged, first)
    fresh = CLIPTextModel(CLIP_CFG).half().to(DEV).eval()                  # a freshly merged encoder, eager launches
    fresh.load_state_dict(te.state_dict())
    assert torch.equal(merged, fresh(ids)[0].cpu())
    pipe.set_lora_scale(0.5)
    fresh.load_state_dict(te.state_dict())
    assert torch.equal(te(ids)[0].cpu(), fresh(ids)[0].cpu()) and not torch.equal(te(ids)[0].cpu(), merged)
    pipe.unload_lora_weights()
    assert torch.equal(te(ids)[0].cpu(), first)


def test_serving_batcher_is_retired_by_a_change_and_a_new_one_serves_the_merged_model():
    cfg, pipe = _tiny_pipe(5)
    emb = torch.randn(2, 77, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(7)).half().to(DEV)
    req = {"prompt_embeds": emb[1:2], "negative_prompt_embeds": emb[0:1], "num_inference_steps": 3, "guidance_scale": 7.5,
           "sampler_opt": {"scheduler": "karras"},
           "latents": torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(8)).half().to(DEV)}
    old = pipe.serve(128, 128, max_batch=2, buckets=(1, 2))
    f0 = old.submit(dict(req))
    old.run_until_idle()
    plain = f0.result().float().cpu()
    pipe.load_lora_weights(_lora(pipe.unet, _targets(pipe.unet), "lora_unet_", rank=8, seed=41), scale=0.8)
    for call in (lambda: old.submit(dict(req)), old.step, old.warm):
        with pytest.raises(RuntimeError, match="weights changed.*build a new batcher"):
            call()
    new = pipe.serve(128, 128, max_batch=2, buckets=(1, 2))
    f1 = new.submit(dict(req))
    new.run_until_idle()
    got = f1.result().float().cpu()
    twin = _twin(pipe)                                                     # the pre-merged pipeline, its own batcher
    ref = twin.serve(128, 128, max_batch=2, buckets=(1, 2))
    f2 = ref.submit(dict(req))
    ref.run_until_idle()
    assert not torch.equal(got, plain) and torch.equal(got, f2.result().float().cpu())
