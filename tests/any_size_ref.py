"""Reference pieces for latents whose sides are not multiples of the UNet's overall factor (tests/test_any_size_*.py).

`oracle/unet_ref.py::unet_forward` doubles at every upsampler; the reference UNet hands each upsampler the size of the skip tensor
its result meets (`upsample_size`).  `sized_unet_forward` restates unet_forward from unet_ref's own pieces and differs from it in
one expression: `F.interpolate(x, size=skips[-1].shape[2:], mode="nearest")`.  At sizes that divide the two are the same function
(tests/test_any_size_host.py pins torch.equal at 16 x 16)."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import unet_ref


def sized_unet_forward(sd, cfg, sample, timestep, enc, region_prompt=None, n_std_groups=1, down_residuals=None, mid_residual=None,
                       intrablock=None):
    sd = {k: v.float() for k, v in sd.items()}
    ch, heads_l, G, eps = cfg.block_out_channels, cfg.num_attention_heads, cfg.norm_num_groups, cfg.norm_eps
    enc = enc.float()
    temb, skips, x = unet_ref._encoder_half(sd, cfg, sample, timestep, enc, region_prompt, n_std_groups, intrablock=intrablock)
    if down_residuals is not None:
        skips = [s_ + r for s_, r in zip(skips, down_residuals)]
    if mid_residual is not None:
        x = x + mid_residual
    rev_heads = list(reversed(heads_l))
    for i in range(len(ch)):
        j = 0
        while f"up_blocks.{i}.resnets.{j}.norm1.weight" in sd:
            x = unet_ref._resnet(sd, f"up_blocks.{i}.resnets.{j}", torch.cat([x, skips.pop()], dim=1), temb, G, eps)
            if f"up_blocks.{i}.attentions.{j}.norm.weight" in sd:
                x = unet_ref._transformer(sd, f"up_blocks.{i}.attentions.{j}", x, enc, rev_heads[i], G, region_prompt, n_std_groups)
            j += 1
        if f"up_blocks.{i}.upsamplers.0.conv.weight" in sd:
            x = unet_ref._conv(sd, f"up_blocks.{i}.upsamplers.0.conv", F.interpolate(x, size=skips[-1].shape[2:], mode="nearest"))
    return unet_ref._conv(sd, "conv_out", F.silu(unet_ref._gn(sd, "conv_norm_out", x, G, eps)))


@contextlib.contextmanager
def _sized_forward_installed():
    """unet_ref.denoise_loop looks `unet_forward` up in its module at call time: the sized restatement stands in for the call"""
    saved = unet_ref.unet_forward
    unet_ref.unet_forward = sized_unet_forward
    try:
        yield
    finally:
        unet_ref.unet_forward = saved


def sized_denoise_loop(*args, **kwargs):
    """unet_ref.denoise_loop, every line of it, around sized_unet_forward"""
    with _sized_forward_installed():
        return unet_ref.denoise_loop(*args, **kwargs)


def skip_sizes(h, w, downsamplings):
    """(the sizes of the levels on the way down, the size each upsampler is asked for on the way up): a stride-2 / pad-1
    convolution turns side n into ceil(n / 2); upsampler k (from the lowest level) meets the skip tensors of level k + 1 from
    the bottom"""
    levels = [(h, w)]
    for _ in range(downsamplings):
        h, w = (h + 1) // 2, (w + 1) // 2
        levels.append((h, w))
    return levels, list(reversed(levels[:-1]))
