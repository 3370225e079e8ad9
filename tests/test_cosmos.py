"""CPU: the Cosmos encoder / decoder head mirror the reference's interface (constructor signatures, state_dict layout: the fixture was
written from the real reference classes), the float64 formulas the GPU tests check the kernels against agree with torch.nn.functional,
unsupported options are refused before any tensor is touched, and the new entry points check their arguments before any launch."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cosmos_formulas as cf
from tests.golden.cosmos_cases import CASES, MODULE_OF, keys_of, signature
from tests.helpers import GOLDEN_DIR, rel_l2

P = 4096        # a 16-byte aligned address that is never dereferenced


def _rand(shape, seed, mean=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) + mean


def _cls(kind):
    return getattr(importlib.import_module(f"uniception_amd.models.{MODULE_OF[kind]}"), kind)


@pytest.mark.parametrize("name", list(CASES))
def test_signature_and_state_dict_equal_the_reference(name, capsys):
    G = np.load(os.path.join(GOLDEN_DIR, "cosmos.npz"))
    kind, kw, _ = CASES[name]
    with capsys.disabled():
        model = _cls(kind)(**kw)
    assert signature(_cls(kind)) == str(G[f"{name}/signature"])
    assert keys_of(model) == str(G[f"{name}/keys"])
    assert [k for k, _ in model.named_parameters()] == str(G[f"{name}/p_names"]).split("\n")
    n = len(model.state_dict())
    assert n == {"enc_p8": 88, "enc_p16": 90, "single_p8": 110, "feature_p16": 228, "feature_skip": 222}[name]
    # the patcher's buffers exist and are not persistent
    patchers = [m for m in model.modules() if type(m).__name__ in ("Patcher", "UnPatcher")]
    assert patchers and all("wavelets" in dict(m.named_buffers()) and not m.state_dict() for m in patchers)


def test_encoder_is_registered_with_its_normalization():
    from uniception_amd.models.encoders import ENCODER_CONFIGS, IMAGE_NORMALIZATION_DICT, CosmosEncoder, encoder_factory
    assert ENCODER_CONFIGS["cosmos"]["class"] is CosmosEncoder
    norm = IMAGE_NORMALIZATION_DICT["cosmos"]
    assert norm.mean.tolist() == [0.0, 0.0, 0.0] and norm.std.tolist() == [0.5, 0.5, 0.5]
    enc = encoder_factory("cosmos", name="c", patch_size=16)
    assert enc.patch_size == 16 and enc.data_norm_type == "cosmos" and enc.encoder.num_downsamples == 2
    from uniception_amd.models.prediction_heads import COSMOS_LATENT_CHANNELS
    assert COSMOS_LATENT_CHANNELS == 16


# ---- the formulas against torch.nn.functional ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W", [(1, 3, 4, 4), (2, 3, 8, 12), (1, 3, 36, 20)])
def test_haar_formula_is_the_grouped_wavelet_convolution(B, C, H, W):
    x = _rand((B, C, H, W), 1 + H)
    a = 0.5 ** 0.5
    lo, hi = torch.tensor([a, a], dtype=torch.float64), torch.tensor([a, -a], dtype=torch.float64)

    def dwt(t):        # low / high pass along the width, then along the height, sub-bands [ll | lh | hl | hh], rescaled by 1 / 2
        g = t.shape[1]
        wl, wh = lo.view(1, 1, 1, 2).repeat(g, 1, 1, 1), hi.view(1, 1, 1, 2).repeat(g, 1, 1, 1)
        hl_, hh_ = lo.view(1, 1, 2, 1).repeat(g, 1, 1, 1), hi.view(1, 1, 2, 1).repeat(g, 1, 1, 1)
        tl, th = F.conv2d(t, wl, groups=g, stride=(1, 2)), F.conv2d(t, wh, groups=g, stride=(1, 2))
        return torch.cat([F.conv2d(tl, hl_, groups=g, stride=(2, 1)), F.conv2d(tl, hh_, groups=g, stride=(2, 1)),
                          F.conv2d(th, hl_, groups=g, stride=(2, 1)), F.conv2d(th, hh_, groups=g, stride=(2, 1))], dim=1) / 2
    want = dwt(dwt(x))
    got = cf.haar_patch(x)
    assert got.shape == (B, 16 * C, H // 4, W // 4) and rel_l2(got, want) < 1e-14
    assert rel_l2(cf.haar_unpatch(got), x) < 1e-14                      # the inverse round-trips
    y = _rand(tuple(got.shape), 2 + H)                                   # the adjoint of the patcher is the inverse / 16
    assert abs(float((got * y).sum() - (x * cf.haar_unpatch(y) / 16).sum())) < 1e-12 * float(got.norm() * y.norm())


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 8), (2, 4, 6, 16), (1, 10, 6, 8)])
def test_downsample_formula_is_pad_right_bottom_and_stride_two(B, H, W, C):
    x = _rand((B, H, W, C), 3 + H)
    w, b = _rand((12, C, 3, 3), 4 + H), _rand((12,), 5 + H)
    want = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1)), w, b, stride=2).permute(0, 2, 3, 1)
    assert rel_l2(cf.down2_conv(x, w, b), want) < 1e-14
    rows = cf.down2_rows(x).reshape(B, H // 2, W // 2, 3, 3, C)
    # the last output row / column reads the zero pad, not the next row's first pixel
    assert float(rows[:, -1, :, 2].abs().max()) == 0.0 and float(rows[:, :, -1, :, 2].abs().max()) == 0.0
    assert torch.equal(rows[:, -1, 0, 1, 0], x[:, H - 1, 0])
    d = _rand((B * (H // 2) * (W // 2), 9 * C), 6 + H)
    lhs, rhs = float((cf.down2_rows(x) * d).sum()), float((x * cf.down2_rows_adjoint(d, B, H, W)).sum())
    assert abs(lhs - rhs) < 1e-12 * float(x.norm() * d.norm())


@pytest.mark.parametrize("B,H,W,C,G", [(2, 4, 5, 64, 8), (1, 2, 3, 128, 32), (1, 7, 5, 32, 4)])
def test_group_norm_silu_formula_and_its_backward(B, H, W, C, G):
    eps = 1e-6
    x = _rand((B, H, W, C), 7 + C, 0.5).requires_grad_(True)
    gamma, beta = (1 + 0.1 * _rand((C,), 8 + C)).requires_grad_(True), (0.1 * _rand((C,), 9 + C)).requires_grad_(True)
    dy = _rand((B, H, W, C), 10 + C)
    want = F.silu(F.group_norm(x.permute(0, 3, 1, 2), G, gamma, beta, eps)).permute(0, 2, 3, 1)
    want.backward(dy)
    y, mean, rstd = cf.group_norm_silu(x.detach(), gamma.detach(), beta.detach(), G, eps)
    dx, dg, db = cf.group_norm_silu_bwd(dy, x.detach(), gamma.detach(), beta.detach(), G, eps)
    assert rel_l2(y, want.detach()) < 1e-13 and mean.shape == rstd.shape == (B, G)
    assert rel_l2(dx, x.grad) < 1e-12 and rel_l2(dg, gamma.grad) < 1e-12 and rel_l2(db, beta.grad) < 1e-12


def test_upsample_and_softmax_formulas():
    x = _rand((2, 3, 5, 8), 11)
    want = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(cf.upsample2(x), want)
    g = _rand((2, 6, 10, 8), 12)
    assert abs(float((want * g).sum() - (x * cf.upsample2_adjoint(g)).sum())) < 1e-12 * float(want.norm() * g.norm())
    for rows, N in ((3, 1), (5, 12), (7, 1000)):
        s = (4 * _rand((rows, N), 13 + N)).requires_grad_(True)
        scale = 512 ** -0.5
        p = F.softmax(s * scale, dim=1)
        dp = _rand((rows, N), 14 + N)
        p.backward(dp)
        got = cf.softmax_rows(s.detach(), scale)
        assert rel_l2(got, p.detach()) < 1e-14 and float((got.sum(1) - 1).abs().max()) < 1e-14
        assert float((cf.softmax_rows_bwd(got, dp, scale) - s.grad).norm()) <= 1e-13 * max(float(s.grad.norm()), 1e-30) + 1e-30
    qkv = _rand((2 * 6, 3 * 16), 15)
    q, k, v = (qkv[:, i * 16:(i + 1) * 16].reshape(2, 6, 16) for i in range(3))
    want = F.scaled_dot_product_attention(q, k, v, scale=0.3).reshape(12, 16)
    assert rel_l2(cf.wide_attention(qkv, 2, 6, 0.3), want) < 1e-13


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
class _Untouchable:
    "stands in for a tensor: any attribute access fails the test"

    def __getattr__(self, name):
        raise AssertionError(f"the input was touched ({name}) before the unsupported option was refused")


def test_unsupported_options_are_refused_before_any_tensor_is_touched(capsys):
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.encoders import CosmosEncoder
    from uniception_amd.models.libs.cosmos_tokenizer.modules import ContinuousFormulation, DecoderType, EncoderType
    from uniception_amd.models.libs.cosmos_tokenizer.modules.layers2d import Decoder, Encoder, ResnetBlock
    from uniception_amd.models.libs.cosmos_tokenizer.modules.patching import Patcher, UnPatcher
    from uniception_amd.models.prediction_heads import CosmosFeature, CosmosSingleChannel
    assert EncoderType.Default.value is Encoder and DecoderType.Default.value is Decoder
    assert {m.name for m in ContinuousFormulation} == {"AE", "VAE"}
    with capsys.disabled():
        vae = CosmosEncoder(name="c")
    vae.distribution = ContinuousFormulation.VAE.value()
    with pytest.raises(UcHipError, match="formulation GaussianDistribution has no HIP path"):
        vae.encode(_Untouchable())
    with pytest.raises(UcHipError, match="patch_method='rearrange'"):
        Patcher(4, "rearrange").forward_nhwc(_Untouchable(), torch.float32)
    with pytest.raises(UcHipError, match="patch_size=2"):
        UnPatcher(2, "haar").forward_nhwc(_Untouchable(), 3)
    enc = CosmosEncoder(name="c")
    enc.encoder.patcher.patch_method = "rearrange"
    with pytest.raises(UcHipError, match="rearrange"):
        enc.encode(_Untouchable())
    enc = CosmosEncoder(name="c")
    enc.encoder = torch.nn.Identity()
    with pytest.raises(UcHipError, match="encoder type Identity has no HIP path"):
        enc.encode(_Untouchable())
    dec = CosmosSingleChannel(8)
    dec.decoder = torch.nn.Identity()
    with pytest.raises(UcHipError, match="decoder type Identity has no HIP path"):
        dec(_Untouchable())
    with pytest.raises(UcHipError, match="dropout=0.1 has no HIP path"):
        ResnetBlock(in_channels=256, dropout=0.1)(_Untouchable())
    with pytest.raises(UcHipError, match="channels per group .3. must be a multiple of 8 or 4"):
        ResnetBlock(in_channels=96, dropout=0.0)(_Untouchable())
    head = CosmosFeature(32, 2, 8, skip_linear=True)
    assert not hasattr(head, "linear") and len(head.cosmos_decoders) == 2
    with pytest.raises(AssertionError, match="patch_size must be 8 or 16"):
        CosmosFeature(32, 2, 4)


def test_product_path_fails_loudly_without_gpu():
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.prediction_heads import CosmosSingleChannel
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(UcHipError, match="HIP device only"):
        CosmosSingleChannel(8)(torch.zeros(1, 16, 2, 2))


# ---- argument checks of the new entry points (decided on the host; the pointers are never dereferenced) ----------------------------
def _lib_no_gpu():
    from uniception_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present: a wrongly accepted argument would launch on invalid pointers")
    return _lib.load()


def _rejects(lib, fn, args, needle):
    status = getattr(lib, fn)(*args)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith(fn + ":") and needle in msg, (fn, args, status, msg)


@pytest.mark.parametrize("fn", ["uc_haar_patch", "uc_haar_unpatch"])
def test_haar_arguments_are_checked_before_any_launch(fn):
    lib = _lib_no_gpu()
    patch = fn == "uc_haar_patch"

    def args(img=P, rows=P, dtype=1, B=2, C=3, H=8, W=12, ld=64, scale=1.0):
        return (img, rows, dtype, B, C, H, W, ld, scale, None) if patch else (rows, dtype, img, B, C, H, W, ld, scale, None)
    for kw, needle in ((dict(img=None), "null pointer"), (dict(rows=None), "null pointer"), (dict(dtype=3), "unsupported dtype 3"),
                       (dict(B=0), "bad shape"), (dict(H=6), "multiples of 4"), (dict(W=10), "multiples of 4"), (dict(ld=40), "at least 16 C = 48"),
                       (dict(ld=52), "multiple of 8"), (dict(scale=0.0), "non-zero"), (dict(img=P + 4), "16-byte aligned")):
        _rejects(lib, fn, args(**kw), needle)


def test_group_norm_silu_arguments_are_checked_before_any_launch():
    lib = _lib_no_gpu()
    base = dict(x=P, y=P, gamma=P, beta=P, mean=P, rstd=P, ws=P, dtype=1, B=2, H=5, W=7, C=64, G=2, eps=1e-6)
    for kw, needle in ((dict(C=64, G=3), "C (64) is not a multiple of G (3)"), (dict(C=48, G=4), "channels per group (12) must be a multiple of 8 (or 4)"),
                       (dict(dtype=3), "unsupported dtype 3"), (dict(beta=None), "null pointer"), (dict(eps=0.0), "eps must be positive"),
                       (dict(x=P + 8), "16-byte aligned"), (dict(C=12, G=3), "C=12 G=3 (C must be a multiple of 8)")):
        a = dict(base, **kw)
        _rejects(lib, "uc_group_norm_silu_nhwc", (a["x"], a["y"], a["gamma"], a["beta"], a["mean"], a["rstd"], a["ws"], a["dtype"], a["B"],
                                                  a["H"], a["W"], a["C"], a["G"], a["eps"], None), needle)
    for kw, needle in ((dict(beta=None), "null pointer"), (dict(dx=None), "null pointer"), (dict(C=48, G=4), "(or 4)"),
                       (dict(dtype=-1), "unsupported dtype -1"), (dict(beta=P + 4), "beta must be 16-byte aligned"),
                       (dict(C=12, G=3), "C=12 G=3 (C must be a multiple of 8)")):
        a = dict(dict(dy=P, x=P, mean=P, rstd=P, gamma=P, beta=P, dx=P, dgamma=P, dbeta=P, ws=P, dtype=1, B=2, H=5, W=7, C=64, G=2), **kw)
        _rejects(lib, "uc_group_norm_silu_nhwc_bwd", (a["dy"], a["x"], a["mean"], a["rstd"], a["gamma"], a["beta"], a["dx"], a["dgamma"],
                                                      a["dbeta"], a["ws"], a["dtype"], a["B"], a["H"], a["W"], a["C"], a["G"], None), needle)
    # groups of four channels: a workspace for the SiLU entry points only; the plain GroupNorm's rule is unchanged
    assert lib.uc_group_norm_silu_nhwc_ws_bytes(2, 8, 8, 128, 32) > 0 and lib.uc_group_norm_silu_nhwc_bwd_ws_bytes(2, 8, 8, 128, 32) > 0
    assert lib.uc_group_norm_nhwc_ws_bytes(2, 8, 8, 128, 32) == 0 and lib.uc_group_norm_nhwc_bwd_ws_bytes(2, 8, 8, 128, 32) == 0
    assert lib.uc_group_norm_silu_nhwc_ws_bytes(2, 8, 8, 256, 32) == lib.uc_group_norm_nhwc_ws_bytes(2, 8, 8, 256, 32) > 0
    assert lib.uc_group_norm_silu_nhwc_ws_bytes(2, 8, 8, 48, 4) == 0
    # groups of four with an odd G: C % 8 == 4, no work item of 8 channels fits; none of the four sizes a workspace for it
    for fn in ("uc_group_norm_nhwc_ws_bytes", "uc_group_norm_silu_nhwc_ws_bytes", "uc_group_norm_nhwc_bwd_ws_bytes", "uc_group_norm_silu_nhwc_bwd_ws_bytes"):
        assert getattr(lib, fn)(2, 5, 7, 12, 3) == 0, fn
    assert lib.uc_group_norm_silu_nhwc_ws_bytes(2, 5, 7, 8, 2) > 0 and lib.uc_group_norm_silu_nhwc_bwd_ws_bytes(2, 5, 7, 8, 2) > 0


@pytest.mark.parametrize("fn", ["uc_down2_gather", "uc_down2_gather_bwd", "uc_upsample2_nhwc", "uc_upsample2_nhwc_bwd"])
def test_gather_and_upsample_arguments_are_checked_before_any_launch(fn):
    lib = _lib_no_gpu()
    cases = [(dict(a=None), "null pointer"), (dict(b=None), "null pointer"), (dict(dtype=7), "unsupported dtype 7"), (dict(C=12), "C must be a multiple of 8"),
             (dict(H=0), "bad shape"), (dict(a=P + 4), "16-byte aligned")]
    if "down2" in fn:
        cases += [(dict(H=5), "must be even"), (dict(W=7), "must be even")]
    for kw, needle in cases:
        a = dict(dict(a=P, b=P, dtype=0, B=1, H=4, W=6, C=8), **kw)
        _rejects(lib, fn, (a["a"], a["b"], a["dtype"], a["B"], a["H"], a["W"], a["C"], None), needle)


def test_softmax_arguments_are_checked_before_any_launch():
    lib = _lib_no_gpu()
    for kw, needle in ((dict(S=None), "null pointer"), (dict(Pm=None), "null pointer"), (dict(dtype=5), "unsupported dtype 5"), (dict(rows=0), "bad shape"),
                       (dict(N=0), "bad shape"), (dict(lds=8), "must be at least N=12"), (dict(ldp=11), "must be at least N=12"),
                       (dict(scale=float("nan")), "scale is NaN"), (dict(S=P + 2), "misaligned")):
        a = dict(dict(S=P, Pm=P, dtype=1, lds=16, ldp=16, rows=5, N=12, scale=0.5), **kw)
        _rejects(lib, "uc_softmax_rows", (a["S"], a["lds"], a["Pm"], a["dtype"], a["ldp"], a["rows"], a["N"], a["scale"], None), needle)
        b = dict(dict(a, dP=P, dS=P), **{{"S": "dP"}.get(k, k): v for k, v in kw.items()})
        _rejects(lib, "uc_softmax_rows_bwd", (b["Pm"], b["dP"], b["lds"], b["dS"], b["dtype"], b["ldp"], b["rows"], b["N"], b["scale"], None), needle)
