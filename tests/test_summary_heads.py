"""CPU: the summary heads (PoseHead, GlobalHead, MLPHead, ResConvBlock) and the token pooling behind them are declared, bound,
exported and checked before any launch; the modules carry the reference's state_dict keys, shapes and constructor signatures
(tests/golden/summary_heads.npz, written by tests/golden/make_golden_summary_heads.py from the real reference classes)."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from tests.golden.summary_heads_cases import CASES, MODULE_OF, fill, keys_of, signature
from tests.helpers import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("uc_token_pool", "uc_token_pool_bwd", "uc_token_pool_ws_bytes")
P = 4096      # a pointer that is never dereferenced: every call that receives it here is rejected before any launch


def _lib_or_build():
    from uniception_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib, _lib.load()


def _gold():
    return np.load(os.path.join(GOLDEN_DIR, "summary_heads.npz"))


def _cls(kind):
    return getattr(importlib.import_module(f"uniception_amd.models.prediction_heads.{MODULE_OF[kind]}"), kind)


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uc_hip.h")).read(), flags=re.S)
    _lib, lib = _lib_or_build()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/uc_hip.h"
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.uc_abi_version() >= 18
    from uniception_amd import autograd, ops
    assert callable(ops.token_pool) and callable(ops.token_pool_bwd)
    assert callable(autograd.token_pool) and callable(autograd.head_linear)


def test_workspace_size_is_positive_and_monotone_in_T():
    _, lib = _lib_or_build()
    sizes = [lib.uc_token_pool_ws_bytes(2, T, 1024) for T in (1, 63, 64, 65, 196, 1024, 4133, 100000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.uc_token_pool_ws_bytes(3, 4133, 64) >= 3 * 65 * 64 * 4      # one fp32 partial per (sample, 64-row chunk, column)


@pytest.mark.parametrize("kw,needle", [
    (dict(x=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(ws=None), "null pointer"),
    (dict(dtype=3), "unsupported dtype 3"),
    (dict(B=0), "bad shape"),
    (dict(T=0), "bad shape"),
    (dict(C=-8), "bad shape"),
    (dict(ld=56), "ld (56) < C (64)"),
    (dict(x=P + 8), "16-byte aligned"),
    (dict(dtype=1, ld=68), "ld a multiple of 8"),
    (dict(dtype=0, ld=66), "ld a multiple of 4"),
    (dict(out=P + 2), "4-byte aligned"),
    (dict(B=65536), "grid limit"),
    (dict(T=65535 * 64 + 1), "grid limit"),
])
def test_token_pool_arguments_are_checked_before_any_launch(kw, needle):
    _, lib = _lib_or_build()
    a = dict(x=P, dtype=1, ld=64, out=P, ws=P, B=2, T=100, C=64)
    a.update(kw)
    status = lib.uc_token_pool(a["x"], a["dtype"], a["ld"], a["out"], a["ws"], a["B"], a["T"], a["C"], None)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith("uc_token_pool:") and needle in msg, msg


@pytest.mark.parametrize("kw,needle", [
    (dict(g=None), "null pointer"),
    (dict(out=None), "null pointer"),
    (dict(dtype=-1), "unsupported dtype -1"),
    (dict(B=0), "bad shape"),
    (dict(T=-1), "bad shape"),
    (dict(C=0), "bad shape"),
    (dict(ld_out=63), "ld_out (63) < C (64)"),
    (dict(gate=P, ld_gate=32), "ld_gate (32) < C (64)"),
    (dict(out=P + 4), "16-byte aligned"),
    (dict(ld_out=68), "ld_out a multiple of 8"),
    (dict(g=P + 1), "4-byte aligned"),
    (dict(gate=P + 2, ld_gate=64), "gate must be 16-byte aligned"),
    (dict(gate=P, ld_gate=68), "ld_gate a multiple of 8"),
    (dict(B=1 << 20, T=1 << 20), "grid limit"),
])
def test_token_pool_bwd_arguments_are_checked_before_any_launch(kw, needle):
    _, lib = _lib_or_build()
    a = dict(g=P, gate=None, ld_gate=0, out=P, ld_out=64, dtype=1, B=2, T=100, C=64)
    a.update(kw)
    status = lib.uc_token_pool_bwd(a["g"], a["gate"], a["ld_gate"], a["out"], a["ld_out"], a["dtype"], a["B"], a["T"], a["C"], None)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith("uc_token_pool_bwd:") and needle in msg, msg


def test_classes_import_from_the_reference_module_paths():
    from uniception_amd.models import prediction_heads as PH
    from uniception_amd.models.prediction_heads.global_head import GlobalHead
    from uniception_amd.models.prediction_heads.mlp_head import MLPHead
    from uniception_amd.models.prediction_heads.pose_head import PoseHead, ResConvBlock
    assert (PH.PoseHead, PH.ResConvBlock, PH.GlobalHead, PH.MLPHead) == (PoseHead, ResConvBlock, GlobalHead, MLPHead)
    assert PH.PredictionHeadTokenInput is not None and PH.SummaryTaskOutput is not None


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    kind, kw, _ = CASES[name]
    assert keys_of(_cls(kind)(**kw)).split("\n") == str(_gold()[f"{name}/keys"]).split("\n")


@pytest.mark.parametrize("name", list(CASES))
def test_constructor_signature_equals_the_reference(name):
    kind = CASES[name][0]
    assert signature(_cls(kind)).split("\n") == str(_gold()[f"{name}/signature"]).split("\n")


@pytest.mark.parametrize("name", list(CASES))
def test_load_state_dict_strict_round_trips(name):
    kind, kw, _ = CASES[name]
    a, b = _cls(kind)(**kw), _cls(kind)(**kw)
    fill(a)
    res = b.load_state_dict(a.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, u), (_, v) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(u, v), k


def test_attributes_and_input_assertions_follow_the_reference():
    from uniception_amd.models.prediction_heads import (GlobalHead, MLPHead, PoseHead, PredictionHeadInput, PredictionHeadTokenInput,
                                                        ResConvBlock)
    p = PoseHead(patch_size=4, input_feature_dim=16)
    assert (p.patch_size, p.input_feature_dim, p.num_resconv_block, p.rot_representation_dim, p.output_dim) == (4, 16, 2, 4, 64)
    assert p.pretrained_checkpoint_path is None and isinstance(p.res_conv[0], ResConvBlock) and isinstance(p.res_conv[0].head_skip, torch.nn.Identity)
    g = GlobalHead(patch_size=2, input_feature_dim=8, num_resconv_block=1)
    assert (g.output_representation_dim, g.output_dim, len(g.res_conv), g.fc_output.out_features) == (1, 16, 1, 1)
    m = MLPHead(input_feature_dim=8, output_dim=2)
    assert (m.input_feature_dim, m.num_mlp_layers, m.hidden_dim, len(m.mlp), m.output_proj.out_features) == (8, 2, 196, 2, 2)
    assert isinstance(ResConvBlock(8, 16).head_skip, torch.nn.Conv2d)
    with pytest.raises(AssertionError, match="does not match expected dimension 16"):
        p(PredictionHeadInput(last_feature=torch.zeros(1, 8, 2, 2)))
    with pytest.raises(AssertionError, match="does not match expected dimension 8"):
        g(PredictionHeadInput(last_feature=torch.zeros(1, 4, 2, 2)))
    with pytest.raises(AssertionError, match="must have 3 dimensions"):
        m(PredictionHeadTokenInput(last_feature=torch.zeros(1, 8)))
    with pytest.raises(AssertionError, match="does not match expected dimension 8"):
        m(PredictionHeadTokenInput(last_feature=torch.zeros(1, 4, 3)))


def test_pretrained_checkpoint_path_loads(tmp_path, capsys):
    from uniception_amd.models.prediction_heads import GlobalHead, MLPHead, PoseHead
    for cls, kw in ((PoseHead, dict(patch_size=2, input_feature_dim=8)), (GlobalHead, dict(patch_size=2, input_feature_dim=8)),
                    (MLPHead, dict(input_feature_dim=8, output_dim=2, hidden_dim=12))):
        src = cls(**kw)
        fill(src)
        path = str(tmp_path / f"{cls.__name__}.pth")
        torch.save({"model": src.state_dict()}, path)
        got = cls(pretrained_checkpoint_path=path, **kw)
        assert "<All keys matched successfully>" in capsys.readouterr().out
        for (k, u), (_, v) in zip(src.state_dict().items(), got.state_dict().items()):
            assert torch.equal(u, v), k


def test_heads_have_no_cpu_fallback():
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.prediction_heads import PoseHead, PredictionHeadInput
    with pytest.raises(UcHipError, match="HIP device only"):
        PoseHead(patch_size=2, input_feature_dim=8)(PredictionHeadInput(last_feature=torch.zeros(1, 8, 2, 2)))
