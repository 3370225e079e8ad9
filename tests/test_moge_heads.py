"""CPU: the MoGe convolutional head (MoGeConvFeature, ResidualConvBlock), MLPFeature and the channels-last kernels behind them
(GroupNorm, replicate pad / crop, half-pixel resize) are declared, bound, exported and checked before any launch; the modules carry
the reference's state_dict keys, shapes and constructor signatures (tests/golden/moge_heads.npz, written by
tests/golden/make_golden_moge_heads.py from the real reference classes)."""
import importlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.golden.moge_heads_cases import CASES, MODULE_OF, fill, keys_of, signature
from tests.helpers import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("uc_group_norm_nhwc", "uc_group_norm_nhwc_ws_bytes", "uc_group_norm_nhwc_bwd", "uc_group_norm_nhwc_bwd_ws_bytes",
       "uc_replicate_pad_nhwc", "uc_replicate_pad_nhwc_bwd", "uc_crop_add_nhwc", "uc_crop_embed_nhwc", "uc_resize_bilinear_nhwc",
       "uc_resize_bilinear_nhwc_bwd")
P = 4096      # a pointer that is never dereferenced: every call that receives it here is rejected before any launch


def _lib_or_build():
    from uniception_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib, _lib.load()


def _gold():
    return np.load(os.path.join(GOLDEN_DIR, "moge_heads.npz"))


def _cls(kind):
    return getattr(importlib.import_module(f"uniception_amd.models.prediction_heads.{MODULE_OF[kind]}"), kind)


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uc_hip.h")).read(), flags=re.S)
    _lib, lib = _lib_or_build()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/uc_hip.h"
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.uc_abi_version() >= 19
    from uniception_amd import autograd, ops
    for fn in ("group_norm_nhwc", "group_norm_nhwc_bwd", "replicate_pad_nhwc", "replicate_pad_nhwc_bwd", "crop_add_nhwc", "crop_embed_nhwc",
               "resize_bilinear_nhwc", "resize_bilinear_nhwc_bwd"):
        assert callable(getattr(ops, fn))
    for fn in ("group_norm", "conv3x3_replicate", "resize_bilinear", "sum_linear", "mlp"):
        assert callable(getattr(autograd, fn))


def test_module_paths_and_exports():
    from uniception_amd.models import prediction_heads as PH
    from uniception_amd.models.prediction_heads.mlp_feature import MLPFeature
    from uniception_amd.models.prediction_heads.moge_conv import MoGeConvFeature, ResidualConvBlock, normalized_view_plane_uv
    assert (PH.MoGeConvFeature, PH.ResidualConvBlock, PH.MLPFeature, PH.normalized_view_plane_uv) == \
        (MoGeConvFeature, ResidualConvBlock, MLPFeature, normalized_view_plane_uv)
    assert PH.PredictionHeadLayeredInput is not None and PH.PixelTaskOutput is not None


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    kind, kw, _, _ = CASES[name]
    assert keys_of(_cls(kind)(**kw)).split("\n") == str(_gold()[f"{name}/keys"]).split("\n")


@pytest.mark.parametrize("name", list(CASES))
def test_constructor_signature_equals_the_reference(name):
    kind = CASES[name][0]
    assert signature(_cls(kind)).split("\n") == str(_gold()[f"{name}/signature"]).split("\n")


@pytest.mark.parametrize("name", list(CASES))
def test_load_state_dict_strict_round_trips(name):
    kind, kw, _, _ = CASES[name]
    a, b = _cls(kind)(**kw), _cls(kind)(**kw)
    fill(a)
    res = b.load_state_dict(a.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, u), (_, v) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(u, v), k


def test_transposed_convolution_taps_are_equal_after_construction():
    kind, kw, _, _ = CASES["moge_small_p14"]
    m = _cls(kind)(**kw)
    for block in m.upsample_blocks:
        w = block[0][0].weight
        assert tuple(w.shape[2:]) == (2, 2)
        assert torch.equal(w, w[:, :, :1, :1].expand_as(w))


def test_normalized_view_plane_uv_equals_its_formula():
    from uniception_amd.models.prediction_heads import normalized_view_plane_uv
    w, h, a = 5, 3, 70 / 42
    uv = normalized_view_plane_uv(width=w, height=h, aspect_ratio=a, dtype=torch.float64)
    assert tuple(uv.shape) == (h, w, 2)
    sx, sy = a / (1 + a * a) ** 0.5, 1 / (1 + a * a) ** 0.5
    for i in range(h):
        for j in range(w):
            u = -sx * (w - 1) / w + 2 * sx * (w - 1) / w * j / (w - 1)
            v = -sy * (h - 1) / h + 2 * sy * (h - 1) / h * i / (h - 1)
            assert abs(float(uv[i, j, 0]) - u) < 1e-12 and abs(float(uv[i, j, 1]) - v) < 1e-12
    assert torch.equal(normalized_view_plane_uv(4, 4), normalized_view_plane_uv(4, 4, aspect_ratio=1.0))


class _Untouchable:
    "stands in for a feature tensor: any use of it fails the test"
    def __getattr__(self, name):
        raise AssertionError(f"the input tensor was touched ({name}) before the unsupported argument was reported")


def test_documented_errors_are_raised_before_any_tensor_is_touched():
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.prediction_heads import MLPFeature, PredictionHeadInput, ResidualConvBlock
    with pytest.raises(UcHipError, match="activation='silu'"):
        ResidualConvBlock(32, activation="silu")(_Untouchable())
    with pytest.raises(UcHipError, match="padding_mode='zeros'"):
        ResidualConvBlock(32, padding_mode="zeros")(_Untouchable())
    with pytest.raises(UcHipError, match="channels per group .* must be a multiple of 8"):
        ResidualConvBlock(20, 20, 32)(_Untouchable())           # GroupNorm(1, 20): 20 channels per group
    with pytest.raises(UcHipError, match="channels per group .* must be a multiple of 8"):
        ResidualConvBlock(32, 32, 72)(_Untouchable())           # GroupNorm(72 // 32 = 2, 72): 36 channels per group
    with pytest.raises(ValueError, match="Unsupported activation"):
        ResidualConvBlock(32, activation="tanh")

    class X:
        shape = (1, 16, 2, 2)
        def __getattr__(self, name):
            raise AssertionError(f"the input tensor was touched ({name})")
    with pytest.raises(UcHipError, match="act_layer=ReLU"):
        MLPFeature(16, patch_size=2, output_dim=1, act_layer=nn.ReLU)(PredictionHeadInput(last_feature=X()))


def test_heads_have_no_cpu_fallback():
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.prediction_heads import MLPFeature, PredictionHeadInput, ResidualConvBlock
    with pytest.raises(UcHipError, match="HIP device only"):
        ResidualConvBlock(32)(torch.zeros(1, 32, 2, 2))
    with pytest.raises(UcHipError, match="HIP device only"):
        MLPFeature(16, patch_size=2, output_dim=1)(PredictionHeadInput(last_feature=torch.zeros(1, 16, 2, 2)))


def test_workspace_sizes_grow_with_the_map():
    _, lib = _lib_or_build()
    f = [lib.uc_group_norm_nhwc_ws_bytes(2, s, s, 64, 2) for s in (1, 16, 17, 37, 296)]
    b = [lib.uc_group_norm_nhwc_bwd_ws_bytes(2, s, s, 64, 2) for s in (1, 16, 17, 37, 296)]
    assert all(v > 0 for v in f + b) and f == sorted(f) and b == sorted(b) and f[-1] > f[0] and b[-1] > b[0]
    assert lib.uc_group_norm_nhwc_ws_bytes(2, 4, 4, 60, 4) == 0 and lib.uc_group_norm_nhwc_bwd_ws_bytes(2, 4, 4, 64, 3) == 0


@pytest.mark.parametrize("kw,needle", [
    (dict(C=64, G=3), "C (64) is not a multiple of G (3)"),
    (dict(C=48, G=4), "channels per group (12) must be a multiple of 8"),
    (dict(dtype=3), "unsupported dtype 3"),
    (dict(x=None), "null pointer"),
    (dict(y=None), "null pointer"),
    (dict(gamma=None), "null pointer"),
    (dict(mean=None), "null pointer"),
    (dict(ws=None), "null pointer"),
    (dict(B=0), "bad shape"),
    (dict(x=P + 8), "16-byte aligned"),
    (dict(eps=0.0), "eps must be positive"),
    (dict(C=4096, G=1), "exceeds 2048"),
])
def test_group_norm_arguments_are_checked_before_any_launch(kw, needle):
    _, lib = _lib_or_build()
    a = dict(x=P, y=P, gamma=P, beta=P, mean=P, rstd=P, ws=P, dtype=1, B=2, H=5, W=7, C=64, G=2, eps=1e-5)
    a.update(kw)
    status = lib.uc_group_norm_nhwc(a["x"], a["y"], a["gamma"], a["beta"], a["mean"], a["rstd"], a["ws"], a["dtype"], a["B"], a["H"], a["W"],
                                    a["C"], a["G"], a["eps"], 1, None)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith("uc_group_norm_nhwc:") and needle in msg, msg


@pytest.mark.parametrize("kw,needle", [
    (dict(C=64, G=3), "C (64) is not a multiple of G (3)"),
    (dict(C=48, G=4), "channels per group (12) must be a multiple of 8"),
    (dict(dtype=-1), "unsupported dtype -1"),
    (dict(dy=None), "null pointer"),
    (dict(dx=None), "null pointer"),
    (dict(dgamma=None), "null pointer"),
    (dict(gate=P + 2), "16-byte aligned"),
])
def test_group_norm_bwd_arguments_are_checked_before_any_launch(kw, needle):
    _, lib = _lib_or_build()
    a = dict(dy=P, x=P, gate=None, mean=P, rstd=P, gamma=P, dx=P, dgamma=P, dbeta=P, ws=P, dtype=1, B=2, H=5, W=7, C=64, G=2)
    a.update(kw)
    status = lib.uc_group_norm_nhwc_bwd(a["dy"], a["x"], a["gate"], a["mean"], a["rstd"], a["gamma"], a["dx"], a["dgamma"], a["dbeta"], a["ws"],
                                        a["dtype"], a["B"], a["H"], a["W"], a["C"], a["G"], None)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith("uc_group_norm_nhwc_bwd:") and needle in msg, msg


@pytest.mark.parametrize("fn", ["uc_replicate_pad_nhwc", "uc_replicate_pad_nhwc_bwd", "uc_crop_embed_nhwc"])
@pytest.mark.parametrize("kw,needle", [
    (dict(a=None), "null pointer"), (dict(b=None), "null pointer"), (dict(dtype=7), "unsupported dtype 7"), (dict(C=12), "C must be a multiple of 8"),
    (dict(H=0), "bad shape"), (dict(a=P + 4), "16-byte aligned"),
])
def test_pad_and_crop_arguments_are_checked_before_any_launch(fn, kw, needle):
    _, lib = _lib_or_build()
    a = dict(a=P, b=P, dtype=0, B=1, H=3, W=5, C=8)
    a.update(kw)
    status = getattr(lib, fn)(a["a"], a["b"], a["dtype"], a["B"], a["H"], a["W"], a["C"], None)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith(fn + ":") and needle in msg, msg


@pytest.mark.parametrize("fn", ["uc_resize_bilinear_nhwc", "uc_resize_bilinear_nhwc_bwd"])
@pytest.mark.parametrize("kw,needle", [
    (dict(a=None), "null pointer"), (dict(dtype=5), "unsupported dtype 5"), (dict(C=4), "C must be a multiple of 8"), (dict(Ho=0), "bad output size"),
])
def test_resize_arguments_are_checked_before_any_launch(fn, kw, needle):
    _, lib = _lib_or_build()
    a = dict(a=P, b=P, dtype=1, B=1, Hi=3, Wi=5, C=8, Ho=6, Wo=9)
    a.update(kw)
    status = getattr(lib, fn)(a["a"], a["b"], a["dtype"], a["B"], a["Hi"], a["Wi"], a["C"], a["Ho"], a["Wo"], 0, None)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith(fn + ":") and needle in msg, msg


@pytest.mark.parametrize("kw,needle", [
    (dict(src=None), "null pointer"), (dict(dst=None), "null pointer"), (dict(dtype=3), "unsupported dtype 3"), (dict(dtype=-2), "unsupported dtype -2"),
    (dict(C=12), "C must be a multiple of 8"), (dict(C=0), "bad shape"), (dict(B=0), "bad shape"), (dict(H=0), "bad shape"), (dict(W=-1), "bad shape"),
    (dict(src=P + 4), "16-byte aligned"), (dict(dst=P + 8), "16-byte aligned"), (dict(res=P + 8), "residual must be 16-byte aligned"),
    (dict(res=P + 2, relu=1), "residual must be 16-byte aligned"),
])
def test_crop_add_arguments_are_checked_before_any_launch(kw, needle):
    _, lib = _lib_or_build()
    a = dict(src=P, res=None, dst=P, dtype=1, B=1, H=3, W=5, C=8, relu=0)
    a.update(kw)
    status = lib.uc_crop_add_nhwc(a["src"], a["res"], a["dst"], a["dtype"], a["B"], a["H"], a["W"], a["C"], a["relu"], None)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith("uc_crop_add_nhwc:") and needle in msg, msg


def test_pretrained_checkpoint_path_loads(tmp_path, capsys):
    for name in ("moge_ln_p16", "mlpfeature_small"):
        kind, kw, _, _ = CASES[name]
        src = _cls(kind)(**kw)
        fill(src)
        path = str(tmp_path / f"{kind}.pth")
        torch.save({"model": src.state_dict()}, path)
        got = _cls(kind)(pretrained_checkpoint_path=path, **kw)
        assert "<All keys matched successfully>" in capsys.readouterr().out
        for (k, u), (_, v) in zip(src.state_dict().items(), got.state_dict().items()):
            assert torch.equal(u, v), k
