"""CPU: the three forward weight builders that the padded and the unpadded conv Functions share (autograd.padded_conv1x1_weights,
engine.convt_weights, engine.conv3x3_weights) against the permute / reshape expressions written out here: without a pad exactly that
tensor, with a pad that tensor in the real block and exact zeros around it; one cache entry per (module, dtype, pad) that a weight
write rebuilds; and check_group_size in its two modes."""
import pytest
import torch
import torch.nn as nn

from uniception_amd import autograd, engine
from uniception_amd._lib import UcHipError

DTYPES = (torch.bfloat16, torch.float32)


def _is_block_in_zeros(w, block):
    "w holds `block` in its leading rows / columns and exact zeros elsewhere"
    r, c = block.shape
    rest = w.clone()
    rest[:r, :c] = 0
    return torch.equal(w[:r, :c], block) and not rest.any()


def _padded_bias(b, bias, n):
    return b.dtype == torch.float32 and b.shape == (n,) and torch.equal(b[:bias.numel()], bias.detach()) and not b[bias.numel():].any()


@pytest.mark.parametrize("dt", DTYPES)
def test_conv1x1_builder(dt):
    torch.manual_seed(0)
    conv = nn.Conv2d(16, 5, 1)
    want = conv.weight.detach().reshape(5, -1).to(dt)
    w, b = autograd.padded_conv1x1_weights(conv, dt, 8)
    assert w.dtype == dt and w.shape == (8, 16) and w.is_contiguous() and _is_block_in_zeros(w, want)
    assert _padded_bias(b, conv.bias, 8)
    conv8 = nn.Conv2d(16, 8, 1)
    w, b = autograd.padded_conv1x1_weights(conv8, dt, 8)
    assert torch.equal(w, conv8.weight.detach().reshape(8, -1).to(dt)) and torch.equal(b, conv8.bias.detach())


@pytest.mark.parametrize("dt", DTYPES)
def test_conv_transpose_builder(dt):
    torch.manual_seed(1)
    ct = nn.ConvTranspose2d(10, 8, 2, 2)
    want = ct.weight.detach().permute(2, 3, 1, 0).reshape(2 * 2 * 8, 10).to(dt).contiguous()
    w, b = engine.convt_weights(ct, dt)
    assert w.dtype == dt and w.is_contiguous() and torch.equal(w, want)
    assert b.dtype == torch.float32 and torch.equal(b, ct.bias.detach().repeat(4))
    assert engine.convt_weights(ct, dt, 10)[0] is w                      # the default pad IS in_channels: one cache entry
    wp, bp = engine.convt_weights(ct, dt, 64)
    assert wp.dtype == dt and wp.shape == (32, 64) and wp.is_contiguous() and _is_block_in_zeros(wp, want)
    assert torch.equal(bp, b)
    assert engine.convt_weights(nn.ConvTranspose2d(10, 8, 2, 2, bias=False), dt, 64)[1] is None


@pytest.mark.parametrize("dt", DTYPES)
def test_conv3x3_builder(dt):
    torch.manual_seed(2)
    conv = nn.Conv2d(6, 5, 3, padding=1)
    want = conv.weight.detach().permute(0, 2, 3, 1).reshape(5, -1).to(dt).contiguous()
    w, b = engine.conv3x3_weights(conv, dt)
    assert w.dtype == dt and w.is_contiguous() and torch.equal(w, want)
    assert b.dtype == torch.float32 and torch.equal(b, conv.bias.detach())
    assert engine.conv3x3_weights(conv, dt, 6, 5)[0] is w
    wp, bp = engine.conv3x3_weights(conv, dt, cin_pad=8, cout_pad=8)
    assert wp.dtype == dt and wp.shape == (8, 72) and wp.is_contiguous()
    w4 = wp.view(8, 3, 3, 8)
    assert torch.equal(w4[:5, :, :, :6], want.view(5, 3, 3, 6))
    assert not w4[5:].any() and not w4[:, :, :, 6:].any()
    assert _padded_bias(bp, conv.bias, 8)
    assert engine.conv3x3_weights(nn.Conv2d(6, 5, 3, padding=1, bias=False), dt)[1] is None


@pytest.mark.parametrize("module, build", [
    (nn.Conv2d(16, 5, 1), lambda m: autograd.padded_conv1x1_weights(m, torch.bfloat16, 8)),
    (nn.ConvTranspose2d(10, 8, 2, 2), lambda m: engine.convt_weights(m, torch.bfloat16, 64)),
    (nn.Conv2d(6, 5, 3, padding=1), lambda m: engine.conv3x3_weights(m, torch.bfloat16, 8, 8))], ids=["c1", "ct", "c3"])
def test_builders_cache_per_weight_version(module, build):
    w, b = build(module)
    again = build(module)
    assert again[0] is w and again[1] is b
    with torch.no_grad():
        module.weight.mul_(2.0)                                          # advances the version counter
    w2 = build(module)[0]
    assert w2 is not w and torch.equal(w2.float(), 2.0 * w.float())      # (doubling commutes with the rounding to bf16)


def test_check_group_size():
    for group4 in (False, True):
        with pytest.raises(UcHipError, match=r"blk: 100 channels in 32 groups: channels per group \(3\.125\) must be a multiple of 8"):
            autograd.check_group_size(100, 32, "blk", group4=group4)
    with pytest.raises(UcHipError, match=r"channels per group \(4\) must be a multiple of 8 \(uc_group_norm_nhwc\)"):
        autograd.check_group_size(128, 32)
    autograd.check_group_size(128, 32, group4=True)
    with pytest.raises(UcHipError, match=r"must be a multiple of 8 or 4 \(uc_group_norm_silu_nhwc\)"):
        autograd.check_group_size(48, 4, group4=True)
    autograd.check_group_size(256, 32)
