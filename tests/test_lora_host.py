"""LoRA adapters on the host (modules/lora.py, ops.lora_merge_eager, the C entry's argument checks, the batcher guard): key
resolution against the tiny UNet and a tiny CLIPTextModel, every refusal with its key, `use_alpha` both ways, the packer, load /
rescale / unload on a CPU pipeline against plain torch statements, and the GPU test's error bound shown on the eager fp32 route.

The UNet has no CPU forward (the hot path is HIP only), so the CPU pipeline checks compare every parameter bit for bit with the
plain-torch merge and run the fp32 oracle's UNet on both state dicts; tests/test_lora_gpu.py compares `txt2img` outputs."""
import ctypes

import pytest
import torch
from torch import nn

import lora_cases as lc
from inputs import FakeTokenizer
from serving_fakes import RecordingExec

from diffusionspatialcontrol_amd import _lib, ops
from diffusionspatialcontrol_amd.modules import lora
from diffusionspatialcontrol_amd.modules.clip_text import CLIPTextModel
from diffusionspatialcontrol_amd.modules.model_k_diffusion import SD15Scheduler, StableDiffusionPipeline
from diffusionspatialcontrol_amd.modules.serving import ServingBatcher
from diffusionspatialcontrol_amd.modules.u_net_condition_modify import UNet2DConditionModel, UNetConfig

CLIP_CFG = dict(vocab_size=99, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
                max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2)
# one module of every kind a kohya file targets in the UNet (diffusers names) ...
UNET_KINDS = ["down_blocks.0.attentions.0.proj_in", "down_blocks.0.attentions.0.proj_out",
              "down_blocks.1.attentions.1.transformer_blocks.0.attn1.to_q", "mid_block.attentions.0.transformer_blocks.0.attn1.to_k",
              "up_blocks.1.attentions.2.transformer_blocks.0.attn1.to_v", "up_blocks.3.attentions.0.transformer_blocks.0.attn1.to_out.0",
              "down_blocks.2.attentions.0.transformer_blocks.0.attn2.to_q", "down_blocks.2.attentions.0.transformer_blocks.0.attn2.to_k",
              "down_blocks.2.attentions.0.transformer_blocks.0.attn2.to_v", "down_blocks.2.attentions.0.transformer_blocks.0.attn2.to_out.0",
              "up_blocks.2.attentions.1.transformer_blocks.0.ff.net.0.proj", "up_blocks.2.attentions.1.transformer_blocks.0.ff.net.2"]
# ... and in the text encoder
TE_KINDS = ["encoder.layers.0.self_attn.q_proj", "encoder.layers.0.self_attn.k_proj", "encoder.layers.1.self_attn.v_proj",
            "encoder.layers.1.self_attn.out_proj", "encoder.layers.0.mlp.fc1", "encoder.layers.1.mlp.fc2"]


def _unet(dtype=torch.float32, seed=0):
    torch.manual_seed(seed)
    return UNet2DConditionModel(UNetConfig.tiny()).to(dtype)


def _pair(module, rank, gen, dtype=torch.float16):
    """(down, up) tensors of one target, as [., ., 1, 1] when the target is a convolution"""
    N, K = module.weight.shape[:2]
    down, up = (0.1 * torch.randn(rank, K, generator=gen)).to(dtype), (0.1 * torch.randn(N, rank, generator=gen)).to(dtype)
    if isinstance(module, nn.Conv2d):
        down, up = down[:, :, None, None], up[:, :, None, None]
    return down, up


def _state_dict(model, names, prefix, rank=4, seed=1, alpha=None, dtype=torch.float16):
    gen = torch.Generator().manual_seed(seed)
    mods = dict(model.named_modules())
    sd = {}
    for n in names:
        head = prefix + n.replace(".", "_")
        sd[head + ".lora_down.weight"], sd[head + ".lora_up.weight"] = _pair(mods[n], rank, gen, dtype=dtype)
        if alpha is not None:
            sd[head + ".alpha"] = torch.tensor(float(alpha))
    return sd


def _all_targets(unet):
    return [n for n, m in unet.named_modules() if ".attentions." in n and
            (isinstance(m, nn.Linear) or (isinstance(m, nn.Conv2d) and tuple(m.kernel_size) == (1, 1)))]


# ----------------------------------------------------------------------------- key resolution
def test_every_unet_target_kind_resolves():
    unet = _unet()
    mods = dict(unet.named_modules())
    sd = _state_dict(unet, UNET_KINDS, "lora_unet_", alpha=2.0)
    layers = lora.resolve(sd, unet)
    assert len(layers) == len(UNET_KINDS)
    for n, l in zip(UNET_KINDS, layers):
        assert l.module is mods[n], n
        assert l.key == "lora_unet_" + n.replace(".", "_") + ".lora_down.weight"
        assert l.rank == 4 and l.alpha == 2.0
        assert tuple(l.up.shape) == (l.module.weight.shape[0], 4) and tuple(l.down.shape) == (4, l.module.weight.shape[1])
    every = _all_targets(unet)
    assert len(every) > 100 and len(lora.resolve(_state_dict(unet, every, "lora_unet_"), unet)) == len(every)


def test_text_encoder_targets_resolve_with_and_without_text_model():
    unet, te = _unet(), CLIPTextModel(CLIP_CFG)
    mods = dict(te.named_modules())
    sd = _state_dict(te, TE_KINDS, "lora_te_text_model_")                 # the kohya spelling: CLIPTextModel strips text_model_
    for n, l in zip(TE_KINDS, lora.resolve(sd, unet, te)):
        assert l.module is mods[n], n

    class HF(nn.Module):                                                   # a transformers 4.x encoder: .text_model owns the layers
        def __init__(self):
            super().__init__()
            self.text_model = CLIPTextModel(CLIP_CFG)
    hf = HF()
    hmods = dict(hf.named_modules())
    for n, l in zip(TE_KINDS, lora.resolve(sd, unet, hf)):                 # resolved WITH the prefix
        assert l.module is hmods["text_model." + n], n
    for n, l in zip(TE_KINDS, lora.resolve(_state_dict(te, TE_KINDS, "lora_te_"), unet, hf)):      # ... and without it
        assert l.module is hmods["text_model." + n], n
    with pytest.raises(ValueError, match="lora_te_text_model_encoder_layers_0_self_attn_q_proj.lora_down.weight"):
        lora.resolve(sd, unet, None)                                       # no text encoder on the pipeline


def test_every_refusal_names_its_key():
    unet = _unet()
    mods = dict(unet.named_modules())
    gen = torch.Generator().manual_seed(3)
    q = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
    head = "lora_unet_" + q.replace(".", "_")
    down, up = _pair(mods[q], 4, gen)
    good = {head + ".lora_down.weight": down, head + ".lora_up.weight": up}
    before = {n: p.detach().clone() for n, p in unet.named_parameters()}
    pipe = StableDiffusionPipeline(None, None, None, unet, SD15Scheduler())

    def refused(sd, key):
        with pytest.raises(ValueError) as e:
            pipe.load_lora_weights(dict(good, **sd) if sd is not None else None)
        assert key in str(e.value), (key, str(e.value))

    refused({"lora_unet_down_blocks_9_nothing.lora_down.weight": down, "lora_unet_down_blocks_9_nothing.lora_up.weight": up},
            "lora_unet_down_blocks_9_nothing.lora_down.weight")                                    # unknown target
    k = "lora_unet_" + UNET_KINDS[3].replace(".", "_")
    refused({k + ".lora_up.weight": up}, k + ".lora_up.weight")                                    # up without down
    refused({k + ".lora_down.weight": down}, k + ".lora_down.weight")                              # down without up
    refused({k + ".alpha": torch.tensor(1.0)}, k + ".alpha")                                       # alpha alone
    c = "down_blocks.0.resnets.0.conv1"                                                            # LoCon: a 3x3 down weight
    ck = "lora_unet_" + c.replace(".", "_")
    refused({ck + ".lora_down.weight": torch.zeros(4, 32, 3, 3).half(), ck + ".lora_up.weight": torch.zeros(32, 4, 1, 1).half()},
            ck + ".lora_down.weight")
    refused({ck + ".lora_down.weight": torch.zeros(4, 32, 1, 1).half(), ck + ".lora_up.weight": torch.zeros(32, 4, 1, 1).half()},
            ck + ".lora_down.weight")                                                              # a 1x1 pair on a 3x3 convolution
    refused({k + ".lora_down.weight": down, k + ".lora_up.weight": torch.zeros(32, 5).half()}, k + ".lora_down.weight")   # ranks
    refused({k + ".lora_down.weight": torch.zeros(4, 24).half(), k + ".lora_up.weight": up}, k + ".lora_down.weight")     # shape
    refused({k + ".hada_w1_a": down}, k + ".hada_w1_a")                                            # LoHa
    refused({k + ".dora_scale": down}, k + ".dora_scale")                                          # DoRA
    refused({"unet.down_blocks.0.attentions.0.to_q.lora_A.weight": down}, "lora_A")                # a PEFT key
    big = torch.zeros(257, 32).half(), torch.zeros(32, 257).half()                                 # the rank cap
    refused({head + ".lora_down.weight": big[0], head + ".lora_up.weight": big[1]}, head + ".lora_down.weight")
    with pytest.raises(ValueError, match="pickle"):
        pipe.load_lora_weights("adapter.ckpt")
    # nothing was merged partially: `good` came first in every dict
    assert pipe.weights_epoch == 0 and pipe.lora_state()["targets"] == 0
    assert all(torch.equal(before[n], p) for n, p in unet.named_parameters())


# ----------------------------------------------------------------------------- arithmetic
def test_default_is_the_reference_formula_and_use_alpha_scales_by_alpha_over_rank():
    """use_alpha=False: `W += scale * up @ down` in fp32, the .alpha key skipped (app.py:548, :583-590); True: times alpha / rank"""
    unet = _unet(torch.float16)
    names = UNET_KINDS
    sd = _state_dict(unet, names, "lora_unet_", rank=4, alpha=2.0)
    mods = dict(unet.named_modules())
    orig = {n: mods[n].weight.detach().clone() for n in names}

    def reference(scale):
        out = {}
        for n in names:
            head = "lora_unet_" + n.replace(".", "_")
            up, down = sd[head + ".lora_up.weight"], sd[head + ".lora_down.weight"]
            w = orig[n].clone()
            if w.dim() == 4:                                               # the reference's two branches, written out
                w += scale * torch.mm(up.squeeze(3).squeeze(2).to(torch.float32),
                                      down.squeeze(3).squeeze(2).to(torch.float32)).unsqueeze(2).unsqueeze(3)
            else:
                w += scale * torch.mm(up.to(torch.float32), down.to(torch.float32))
            out[n] = w
        return out

    pipe = StableDiffusionPipeline(None, None, None, unet, SD15Scheduler())
    pipe.load_lora_weights(sd, scale=0.8)
    ref = reference(0.8)
    assert all(torch.equal(mods[n].weight, ref[n]) for n in names)
    assert not any(torch.equal(mods[n].weight, orig[n]) for n in names)
    pipe.unload_lora_weights()
    pipe.load_lora_weights(sd, scale=0.8, use_alpha=True)                  # alpha / rank = 0.5
    ref = reference(0.4)
    assert all(torch.equal(mods[n].weight, ref[n]) for n in names)
    assert pipe.lora_state()["adapters"]["lora0"] == {"scale": 0.8, "use_alpha": True, "layers": len(names), "rank": 4}


def test_packer_pads_each_adapter_to_segments_and_gains_follow_the_owner():
    g = torch.Generator().manual_seed(5)
    N, K = 24, 16
    ads = [(torch.randn(N, r, generator=g), torch.randn(r, K, generator=g)) for r in (4, 33, 32)]     # fp32 in: rounded to fp16
    up, down, owner = ops.lora_pack_adapters(ads, N, K)
    assert up.dtype == down.dtype == torch.float16 and tuple(up.shape) == (N, 128) and tuple(down.shape) == (128, K)
    assert owner == [0, 1, 1, 2] and ops.LORA_SEGMENT == 32 and ops.LORA_MAX_RANK == 256
    col = 0
    for (u, d), rp in zip(ads, (32, 64, 32)):
        r = u.shape[1]
        assert torch.equal(up[:, col:col + r], u.half()) and torch.equal(down[col:col + r], d.half())
        assert not up[:, col + r:col + rp].any() and not down[col + r:col + rp].any()                  # zero columns / rows
        col += rp
    assert [ops.lora_padded_rank(r) for r in (1, 32, 33, 256)] == [32, 32, 64, 256]
    with pytest.raises(ValueError):
        ops.lora_pack_adapters([(torch.zeros(N, 4), torch.zeros(5, K))], N, K)
    # the gains of a table: one per segment, the owner's scale (times alpha / rank when asked)
    l = lora.Layer("k", None, ads[0][0], ads[0][1], 2.0, 4)
    assert lora.layer_gain(l, 0.8, False) == 0.8 and lora.layer_gain(l, 0.8, True) == 0.8 * 2.0 / 4
    assert lora.layer_gain(l._replace(alpha=None), 0.8, True) == 0.8


def test_kernel_limits_are_stated_once_and_mirrored():
    w = torch.zeros(16, 16, dtype=torch.float16)
    assert not ops.lora_merge_takes(w, [4])                                # CPU
    assert not ops.lora_merge_takes(w.float(), [4])
    with open(_lib.header_path()) as f:
        head = f.read()
    assert f"#define DSC_LORA_SEGMENT  {ops.LORA_SEGMENT}" in head and f"#define DSC_LORA_MAX_RANK {ops.LORA_MAX_RANK}" in head
    with pytest.raises(_lib.DscLibraryError):
        ops.lora_merge_([(w, w.clone(), torch.zeros(16, 32).half(), torch.zeros(32, 16).half())], [1.0])     # no CPU kernel route


def test_entry_validates_on_the_host_without_a_gpu():
    lib = _lib.load_library()
    BAD, UNSUPPORTED = -1, -2

    def job(**kw):
        j = _lib.LoraJob()
        j.base, j.dst, j.up, j.down, j.gain = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
        j.N, j.K, j.R, j.tile0, j.ld_dst = 40, 72, 32, 0, 72
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def plan(*jobs):
        arr = (_lib.LoraJob * len(jobs))(*jobs)
        return lib.dsc_lora_merge_plan(arr, len(jobs)), arr

    assert plan(job())[0] == 2                                             # 1 row tile x 2 column tiles of 64 x 64
    total, arr = plan(job(), job(N=130, K=264, ld_dst=272), job(N=8, K=8, ld_dst=8))
    assert total == 2 + 3 * 5 + 1 and [j.tile0 for j in arr] == [0, 2, 17]
    assert lib.dsc_lora_merge_plan(None, 1) == BAD and plan(job())[1] is not None and lib.dsc_lora_merge_plan(arr, 0) == BAD
    for field in ("base", "dst", "up", "down", "gain"):
        assert plan(job(**{field: None}))[0] == BAD, field
    assert plan(job(N=0))[0] == BAD and plan(job(R=0))[0] == BAD and plan(job(ld_dst=64))[0] == BAD
    assert plan(job(base=0x200000))[0] == BAD                               # dst aliases base
    assert plan(job(up=0x200000 + 72 * 2 * 39))[0] == BAD                   # ... the last row of dst
    assert plan(job(down=0x200000 - 32 * 72 * 2 + 16))[0] == BAD and plan(job(gain=0x200010))[0] == BAD
    assert plan(job(K=76, ld_dst=76))[0] == UNSUPPORTED                    # rows of 16 bytes
    assert plan(job(ld_dst=76))[0] == UNSUPPORTED
    assert plan(job(R=48))[0] == UNSUPPORTED and plan(job(R=288))[0] == UNSUPPORTED and plan(job(R=256))[0] == 2
    assert plan(job(dst=0x200008))[0] == UNSUPPORTED and plan(job(gain=0x500002))[0] == UNSUPPORTED
    dev = ctypes.c_void_p(0x600000)
    _, one = plan(job())
    assert lib.dsc_lora_merge_f16(None, dev, 1, 0, None) == BAD and lib.dsc_lora_merge_f16(one, None, 1, 0, None) == BAD
    assert lib.dsc_lora_merge_f16(one, dev, 0, 0, None) == BAD
    assert lib.dsc_lora_merge_f16(one, dev, 1, 1, None) == UNSUPPORTED      # fp16 only
    one[0].tile0 = 5
    assert lib.dsc_lora_merge_f16(one, dev, 1, 0, None) == BAD              # not the plan's numbering
    one[0].tile0, one[0].N = 0, 0
    assert lib.dsc_lora_merge_f16(one, dev, 1, 0, None) == BAD


def test_eager_route_meets_the_gpu_tests_bound():
    """the bound tests/test_lora_gpu.py holds the kernel to, on the same inputs, for the reference's fp32 arithmetic: no
    element outside it, although rows built to cancel are several fp16 ulps off (a bare 1-ulp bound would be wrong)"""
    worst = 0.0
    for i, (N, K) in enumerate(lc.SHAPES):
        for j, ranks in enumerate(lc.RANK_SETS):
            base, adapters = lc.case(N, K, ranks, seed=100 * i + j)
            got = ops.lora_merge_eager(torch.empty_like(base), base, adapters)
            bad, ulps, _ = lc.violations(got, base, adapters)
            worst = max(worst, ulps)
            assert bad == 0, (N, K, ranks, bad, ulps)
    print(f"eager fp32 route: largest error {worst:.2f} fp16 ulps of the exact value (rows built to cancel), 0 outside the bound")
    assert worst > 1.0                                                     # the cancelling rows do what they were built for
    # the exact cases are exact on this route too: fp64 rounded once
    base, adapters = lc.exact_case(33, 136, (32, 4), seed=7)
    assert torch.equal(ops.lora_merge_eager(torch.empty_like(base), base, adapters), lc.exact64(base, adapters).half())
    # a gain of 0 is skipped, not multiplied
    up, down, _ = adapters[0]
    poisoned = [(torch.full_like(up, float("nan")), torch.full_like(down, float("inf")), 0.0), adapters[1]]
    assert torch.equal(ops.lora_merge_eager(torch.empty_like(base), base, poisoned),
                       ops.lora_merge_eager(torch.empty_like(base), base, adapters[1:]))
    assert lc.ulp16(torch.tensor([1.0, 1.5, 2.0, 0.0, 2.0 ** -20, -3.0], dtype=torch.float64)).tolist() == \
        [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9]


# ----------------------------------------------------------------------------- pipeline on the CPU
def _plain_merge(orig, sds_scales):
    """{name: weight} merged by plain torch statements from the original weights: fp32 mm, scale, add, cast"""
    out = {}
    for n, w in orig.items():
        total = torch.zeros(w.shape[0], w.shape[1], dtype=torch.float32)
        for sd, scale in sds_scales:
            head = "lora_unet_" + n.replace(".", "_")
            if head + ".lora_up.weight" in sd and scale != 0:
                total = total + scale * torch.mm(sd[head + ".lora_up.weight"].float().flatten(1), sd[head + ".lora_down.weight"].float().flatten(1))
        out[n] = (w.float() + total.reshape(w.shape)).to(w.dtype)
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_load_rescale_unload_on_a_cpu_pipeline(dtype):
    from oracle import unet_ref
    unet = _unet(dtype)
    cfg = UNetConfig.tiny()
    pipe = StableDiffusionPipeline(None, None, None, unet, SD15Scheduler())
    mods = dict(unet.named_modules())
    every = _all_targets(unet)
    a = _state_dict(unet, every, "lora_unet_", rank=4, seed=11, dtype=dtype)
    b = _state_dict(unet, UNET_KINDS, "lora_unet_", rank=33, seed=12, dtype=dtype)
    original = {n: p.detach().clone() for n, p in unet.named_parameters()}
    orig_w = {n: mods[n].weight.detach().clone() for n in every}
    versions = {n: mods[n].weight._version for n in every}

    def matches(sds_scales):
        want = _plain_merge(orig_w, sds_scales)
        return all(torch.equal(mods[n].weight, want[n]) for n in every)

    pipe._graphs = {"stale": object()}
    assert pipe.weights_epoch == 0 and pipe.load_lora_weights(a, scale=0.8, name="a") == "a"
    assert pipe.weights_epoch == 1 and pipe._graphs == {} and matches([(a, 0.8)])
    assert all(mods[n].weight._version > versions[n] for n in every)      # what the derived-weight caches key on
    st = pipe.lora_state()
    assert st["targets"] == len(every) and st["kernel_targets"] == 0
    assert st["base_bytes"] == sum(w.numel() * w.element_size() for w in orig_w.values())
    # the merged pipeline computes what a UNet with plainly merged weights computes (fp32 oracle on both state dicts)
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(1))
    text = torch.randn(2, 77, cfg.cross_attention_dim, generator=torch.Generator().manual_seed(2))
    t = torch.tensor([500.0, 500.0])
    merged_sd = {k: v.float() for k, v in unet.state_dict().items()}
    plain_sd = {k: v.float() for k, v in original.items()}
    plain_sd.update({n + ".weight": w.float() for n, w in _plain_merge(orig_w, [(a, 0.8)]).items()})
    assert torch.equal(unet_ref.unet_forward(merged_sd, cfg, x, t, text), unet_ref.unet_forward(plain_sd, cfg, x, t, text))
    assert not torch.equal(unet_ref.unet_forward(merged_sd, cfg, x, t, text),
                           unet_ref.unet_forward({k: v.float() for k, v in original.items()}, cfg, x, t, text))

    pipe.set_lora_scale(0.5)
    assert pipe.weights_epoch == 2 and matches([(a, 0.5)])
    pipe.load_lora_weights(b, scale=-1.25, name="b")                      # a second adapter on some of the weights
    assert pipe.weights_epoch == 3 and matches([(a, 0.5), (b, -1.25)])
    pipe.set_lora_scale({"b": 0.25})
    assert pipe.weights_epoch == 4 and matches([(a, 0.5), (b, 0.25)])
    pipe.set_lora_scale({"a": 0.0})                                       # a gain of 0 leaves b alone on the shared weights
    assert matches([(b, 0.25)]) and sorted(pipe.lora_state()["adapters"]) == ["a", "b"]
    with pytest.raises(ValueError, match="'c'"):
        pipe.set_lora_scale({"c": 1.0})
    with pytest.raises(ValueError, match="'a'"):
        pipe.load_lora_weights(a, name="a")
    with pytest.raises(ValueError, match="'c'"):
        pipe.unload_lora_weights("c")
    epoch = pipe.weights_epoch
    pipe.unload_lora_weights("a")                                         # weights only `a` touched get their bits back
    assert pipe.weights_epoch == epoch + 1 and matches([(b, 0.25)]) and pipe.lora_state()["targets"] == len(UNET_KINDS)
    pipe.unload_lora_weights()
    assert pipe.weights_epoch == epoch + 2
    assert all(torch.equal(original[n], p) for n, p in unet.named_parameters())
    st = pipe.lora_state()
    assert st["adapters"] == {} and st["targets"] == 0 and st["base_bytes"] == 0 and pipe._lora.table is None
    with pytest.raises(ValueError):
        pipe.set_lora_scale(1.0)


def test_safetensors_file_and_text_encoder_round_trip(tmp_path):
    from safetensors.torch import save_file
    unet, te = _unet(), CLIPTextModel(CLIP_CFG)
    pipe = StableDiffusionPipeline(None, te, FakeTokenizer(), unet, SD15Scheduler())
    sd = dict(_state_dict(unet, UNET_KINDS[:3], "lora_unet_", dtype=torch.float32),
              **_state_dict(te, TE_KINDS, "lora_te_text_model_", dtype=torch.float32, alpha=1.0))
    path = tmp_path / "style.safetensors"
    save_file(sd, str(path))
    ids = torch.randint(3, 99, (2, 77), generator=torch.Generator().manual_seed(4))
    before = te(ids)[0]
    original = {n: p.detach().clone() for n, p in te.named_parameters()}
    assert pipe.load_lora_weights(str(path), scale=1.5) == "style"         # the file's stem
    mods = dict(te.named_modules())
    for n in TE_KINDS:
        head = "lora_te_text_model_" + n.replace(".", "_")
        want = original[n + ".weight"] + 1.5 * torch.mm(sd[head + ".lora_up.weight"], sd[head + ".lora_down.weight"])
        assert torch.equal(mods[n].weight, want), n
    merged = te(ids)[0]                                                    # the fused QKV copies follow the version counter
    fresh = CLIPTextModel(CLIP_CFG)
    fresh.load_state_dict(te.state_dict())
    assert not torch.equal(merged, before) and torch.equal(merged, fresh(ids)[0])
    pipe.unload_lora_weights("style")
    assert all(torch.equal(original[n], p) for n, p in te.named_parameters()) and torch.equal(te(ids)[0], before)


# ----------------------------------------------------------------------------- serving guard
def test_batcher_built_before_a_change_refuses_and_a_running_one_blocks_the_change():
    unet = _unet(torch.float16)
    pipe = StableDiffusionPipeline(None, None, FakeTokenizer(), unet, SD15Scheduler())
    sd = _state_dict(unet, UNET_KINDS, "lora_unet_")
    emb = torch.randn(2, 77, 64, generator=torch.Generator().manual_seed(0)).half()
    req = {"prompt_embeds": emb[1:2], "negative_prompt_embeds": emb[0:1], "num_inference_steps": 2,
           "sampler_opt": {"scheduler": "karras"}, "latents": torch.zeros(1, 4, 16, 16).half()}
    old = ServingBatcher(pipe, 128, 128, executor=RecordingExec())
    fut = old.submit(dict(req))
    assert old.step()
    pipe.load_lora_weights(sd, scale=0.5)
    for call in (lambda: old.submit(dict(req)), old.step, old.warm):
        with pytest.raises(RuntimeError, match="weights changed.*build a new batcher"):
            call()
    assert not fut.done()
    new = ServingBatcher(pipe, 128, 128, executor=RecordingExec())         # built after the change: serves as usual
    f2 = new.submit(dict(req))
    new.run_until_idle()
    assert f2.done()
    new.start()                                                            # its own thread: load / set / unload refuse
    try:
        epoch = pipe.weights_epoch
        for call in (lambda: pipe.set_lora_scale(1.0), lambda: pipe.unload_lora_weights(),
                     lambda: pipe.load_lora_weights(sd, name="again")):
            with pytest.raises(RuntimeError, match="running its own thread"):
                call()
        assert pipe.weights_epoch == epoch and sorted(pipe.lora_state()["adapters"]) == ["lora0"]
    finally:
        new.stop()
    pipe.set_lora_scale(1.0)                                               # stopped: allowed, and `new` is retired too
    with pytest.raises(RuntimeError, match="weights changed"):
        new.step()
