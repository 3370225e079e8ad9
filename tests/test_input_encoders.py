"""CPU: the non-image input encoders (PatchEmbedder, DenseRepresentationEncoder, GlobalRepresentationEncoder) and the streaming
kernels behind them (uc_unshuffle_rows, uc_unshuffle_rows_bwd, uc_act, uc_ln_pe_ln, uc_ln_param_grads) are declared, bound, exported and checked before any
launch; the modules carry the reference's state_dict keys, shapes and constructor signatures (tests/golden/input_encoders.npz, written
by tests/golden/make_golden_input_encoders.py from the real reference classes)."""
import importlib
import os
import re
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.golden.input_encoders_cases import CASES, MODULE_OF, fill, keys_of, kwargs, signature
from tests.helpers import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("uc_unshuffle_rows", "uc_unshuffle_rows_bwd", "uc_act", "uc_ln_pe_ln", "uc_ln_param_grads")
FACTORY = {"DenseRepresentationEncoder": "dense_rep_encoder", "PatchEmbedder": "patch_embedder", "GlobalRepresentationEncoder": "global_rep_encoder"}
P = 4096      # a pointer that is never dereferenced: every call that receives it here is rejected before any launch


def _lib_or_build():
    from uniception_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib, _lib.load()


def _gold():
    return np.load(os.path.join(GOLDEN_DIR, "input_encoders.npz"))


def _cls(kind):
    return getattr(importlib.import_module(f"uniception_amd.models.encoders.{MODULE_OF[kind]}"), kind)


def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uc_hip.h")).read(), flags=re.S)
    _lib, lib = _lib_or_build()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/uc_hip.h"
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.uc_abi_version() >= 20 and _lib.ABI_VERSION >= 20
    from uniception_amd import autograd, ops
    assert "uc_ln_param_grads_ws_bytes" in _lib.SIGNATURES and lib.uc_ln_param_grads_ws_bytes(130, 64) == 4 * (2 * 130 + 2 * 64 * 3)
    for fn in ("unshuffle_rows", "unshuffle_rows_bwd", "act", "ln_pe_ln", "ln_param_grads"):
        assert callable(getattr(ops, fn))
    for fn in ("unshuffle_rows", "act", "ln_pe_ln", "conv3x3_padded"):
        assert callable(getattr(autograd, fn))


def test_classes_factory_entries_and_normalization():
    from uniception_amd.models import encoders as E
    from uniception_amd.models.encoders.dense_rep_encoder import DenseRepresentationEncoder, ResidualBlock
    from uniception_amd.models.encoders.global_rep_encoder import GlobalRepresentationEncoder
    from uniception_amd.models.encoders.patch_embedder import PatchEmbedder
    assert (E.DenseRepresentationEncoder, E.ResidualBlock, E.GlobalRepresentationEncoder, E.PatchEmbedder) == \
        (DenseRepresentationEncoder, ResidualBlock, GlobalRepresentationEncoder, PatchEmbedder)
    want = {"dense_rep_encoder": (DenseRepresentationEncoder, ["Dense-Representation-Encoder"]),
            "global_rep_encoder": (GlobalRepresentationEncoder, ["Global-Representation-Encoder"]),
            "patch_embedder": (PatchEmbedder, ["Patch-Embedder"])}
    for key, (cls, models) in want.items():
        cfg = E.ENCODER_CONFIGS[key]
        assert cfg["class"] is cls and cfg["supported_models"] == models and "intermediate_feature_returner_class" not in cfg
        assert key in E.get_available_encoders()
        with pytest.raises(KeyError):                       # the reference's behaviour for an encoder without a feature returner
            E.feature_returner_encoder_factory(key, name="x")
    norm = E.IMAGE_NORMALIZATION_DICT["patch_embedder"]
    assert torch.equal(norm.mean, torch.tensor([0.485, 0.456, 0.406])) and torch.equal(norm.std, torch.tensor([0.229, 0.224, 0.225]))


@pytest.mark.parametrize("name", list(CASES))
def test_encoder_factory_builds_each_case_with_the_reference_keys_and_shapes(name):
    from uniception_amd.models.encoders import encoder_factory
    kind = CASES[name][0]
    model = encoder_factory(FACTORY[kind], **kwargs(name))
    assert type(model) is _cls(kind)
    assert keys_of(model).split("\n") == str(_gold()[f"{name}/keys"]).split("\n")


@pytest.mark.parametrize("kind", sorted(set(k for k, _ in CASES.values())))
def test_constructor_signature_equals_the_reference(kind):
    name = next(n for n, (k, _) in CASES.items() if k == kind)
    assert signature(_cls(kind)).split("\n") == str(_gold()[f"{name}/signature"]).split("\n")


@pytest.mark.parametrize("name", ["dense_small", "dense_native_p14"])
def test_sinusoid_table_equals_the_reference_bit_for_bit(name):
    model = _cls("DenseRepresentationEncoder")(**kwargs(name))
    assert torch.equal(model.pos_embed, torch.from_numpy(_gold()[f"{name}/pos_embed_init"]))
    assert "pos_embed" in dict(model.named_buffers()) and "pos_embed" not in dict(model.named_parameters())


def test_position_table_is_a_parameter_of_the_patch_embedder_and_absent_without_pe():
    pe = _cls("PatchEmbedder")(**kwargs("patch_small"))
    assert isinstance(pe.pos_embed, nn.Parameter) and tuple(pe.pos_embed.shape) == (1, 25, 64)
    assert isinstance(pe.norm, nn.Identity) and isinstance(pe.post_pe_norm, nn.LayerNorm) and pe.post_pe_norm.eps == 1e-6
    plain = _cls("DenseRepresentationEncoder")(**kwargs("dense_plain"))
    assert "pos_embed" not in plain.state_dict() and not hasattr(plain, "post_pe_norm") and isinstance(plain.norm_layer, nn.Identity)
    g = _cls("GlobalRepresentationEncoder")(**kwargs("global_default"))
    assert [tuple(l.weight.shape) for l in g.linears()] == [(128, 3), (256, 128), (512, 256), (1024, 512)]
    assert list(g.state_dict())[0] == "encoder.0.0.0.0.weight"


@pytest.mark.parametrize("name", list(CASES))
def test_load_state_dict_strict_round_trips(name):
    kind = CASES[name][0]
    a, b = _cls(kind)(**kwargs(name)), _cls(kind)(**kwargs(name))
    fill(a)
    res = b.load_state_dict(a.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, u), (_, v) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(u, v), k


def test_pretrained_checkpoint_path_loads(tmp_path, capsys):
    for name in ("dense_small", "patch_small", "global_small"):
        kind = CASES[name][0]
        src = _cls(kind)(**kwargs(name))
        fill(src)
        path = str(tmp_path / f"{kind}.pth")
        torch.save({"model": src.state_dict()}, path)
        got = _cls(kind)(pretrained_checkpoint_path=path, **kwargs(name))
        assert "<All keys matched successfully>" in capsys.readouterr().out
        for (k, u), (_, v) in zip(src.state_dict().items(), got.state_dict().items()):
            assert torch.equal(u, v), k


def test_resized_position_table_follows_the_reference_formula():
    "scale-factor form, size form, antialias on and off, and the native-grid shortcut, against F.interpolate called as the reference calls it"
    import torch.nn.functional as F
    from uniception_amd.models.encoders.patch_embedder import resize_pos_table
    table = torch.randn(1, 25, 8, generator=torch.Generator().manual_seed(1))
    grid = table.reshape(1, 5, 5, 8).permute(0, 3, 1, 2)
    for antialias in (False, True):
        got = resize_pos_table(table, 21, 12, 28, 4, 0.1, antialias)
        want = F.interpolate(grid, mode="bicubic", antialias=antialias, scale_factor=(3.1 / 5, 7.1 / 5)).permute(0, 2, 3, 1).reshape(1, 21, 8)
        assert torch.equal(got, want)
        got = resize_pos_table(table, 21, 12, 28, 4, 0.0, antialias)
        want = F.interpolate(grid, mode="bicubic", antialias=antialias, size=(3, 7)).permute(0, 2, 3, 1).reshape(1, 21, 8)
        assert torch.equal(got, want)
    assert resize_pos_table(table, 25, 20, 20, 4, 0.1, False) is table              # the native grid returns the raw table
    with pytest.raises(AssertionError):
        resize_pos_table(torch.zeros(1, 24, 8), 21, 12, 28, 4, 0.1, False)           # N == M * M
    t = table.clone().requires_grad_(True)
    resize_pos_table(t, 21, 12, 28, 4, 0.1, False).sum().backward()                  # differentiable
    assert t.grad is not None and float(t.grad.abs().sum()) > 0


def test_unsupported_layers_are_refused_at_construction():
    from uniception_amd._lib import UcHipError
    D, Pt, G = _cls("DenseRepresentationEncoder"), _cls("PatchEmbedder"), _cls("GlobalRepresentationEncoder")
    from uniception_amd.models.encoders.dense_rep_encoder import ResidualBlock
    with pytest.raises(UcHipError, match="act_layer=SiLU"):
        D(name="d", act_layer=nn.SiLU, intermediate_dims=[8, 8], enc_embed_dim=8)
    with pytest.raises(UcHipError, match="act_layer=SiLU"):
        D(name="d", act_layer=nn.SiLU, intermediate_dims=[8], enc_embed_dim=8)          # no residual block: refused all the same
    with pytest.raises(UcHipError, match="act_layer=GELU"):
        G(name="g", act_layer=partial(nn.GELU, approximate="tanh"))
    with pytest.raises(UcHipError, match="act_layer=Tanh"):
        ResidualBlock(8, 8, act_layer=nn.Tanh)
    with pytest.raises(UcHipError, match="norm_layer=BatchNorm1d"):
        D(name="d", norm_layer=nn.BatchNorm1d, intermediate_dims=[8], enc_embed_dim=8)
    with pytest.raises(UcHipError, match="post_pe_norm_layer=GroupNorm"):
        Pt(name="p", post_pe_norm_layer=partial(nn.GroupNorm, 1), enc_embed_dim=8, input_size=8, patch_size=4)
    with pytest.raises(UcHipError, match="norm_layer=LayerNorm"):
        G(name="g", norm_layer=partial(nn.LayerNorm, elementwise_affine=False))
    assert isinstance(G(name="g", act_layer=nn.ReLU, norm_layer=None).norm_layer, nn.Identity)


def test_encoders_have_no_cpu_fallback_and_keep_the_reference_input_checks():
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.encoders import EncoderGlobalRepInput, ViTEncoderInput, ViTEncoderNonImageInput
    d = _cls("DenseRepresentationEncoder")(**kwargs("dense_small"))
    p = _cls("PatchEmbedder")(**kwargs("patch_small"))
    g = _cls("GlobalRepresentationEncoder")(**kwargs("global_small"))
    with pytest.raises(UcHipError, match="HIP device only"):
        d(ViTEncoderNonImageInput(data=torch.zeros(1, 2, 8, 8)))
    with pytest.raises(UcHipError, match="HIP device only"):
        p(ViTEncoderInput(data_norm_type="patch_embedder", image=torch.zeros(1, 3, 8, 8)))
    with pytest.raises(UcHipError, match="HIP device only"):
        g(EncoderGlobalRepInput(data=torch.zeros(2, 9)))
    with pytest.raises(AssertionError, match="does not match the encoder's normalization type"):
        p(ViTEncoderInput(data_norm_type="dinov2", image=torch.zeros(1, 3, 8, 8)))
    with pytest.raises(AssertionError, match="divisible by patch size"):
        d(ViTEncoderNonImageInput(data=torch.zeros(1, 2, 8, 9)))
    with pytest.raises(AssertionError, match="Input channels must be 2"):
        d(ViTEncoderNonImageInput(data=torch.zeros(1, 3, 8, 8)))
    with pytest.raises(AssertionError, match="must have 9 channels"):
        g(EncoderGlobalRepInput(data=torch.zeros(2, 3)))
    with pytest.raises(ValueError, match="Unsupported input type"):
        p(EncoderGlobalRepInput(data=torch.zeros(2, 3)))


def test_gradient_checkpointing_wraps_the_residual_blocks_only():
    m = _cls("DenseRepresentationEncoder")(gradient_checkpointing=True, **kwargs("dense_small"))
    assert [type(b).__name__ for b in m.encoder] == ["CheckpointedResidualBlock", "CheckpointedResidualBlock", "Conv2d"]
    assert keys_of(m) == keys_of(_cls("DenseRepresentationEncoder")(**kwargs("dense_small")))


def test_new_entry_points_reject_other_dtype_codes_before_any_launch():
    """The form of test_abi.test_single_dtype_entry_points_reject_other_dtype_codes_before_any_launch: every dtype argument of the new
    entry points takes UC_F32 / UC_BF16 only; any other code is answered with '<fn>: unsupported dtype <d> (...)' before anything is
    launched.  Decided entirely on the host, so it is skipped where a GPU is visible (a dispatch that wrongly accepted a code would
    launch on these pointers)."""
    if torch.cuda.is_available():
        pytest.skip("GPU present: a wrongly accepted code would launch on invalid pointers")
    _lib, lib = _lib_or_build()
    D = "DTYPE"
    table = [
        ("uc_unshuffle_rows", (P, D, P, 0, 2, 3, 5, 7, 2, 16, None)),
        ("uc_unshuffle_rows", (P, 1, P, D, 2, 3, 5, 7, 2, 16, None)),
        ("uc_unshuffle_rows_bwd", (P, D, P, 2, 3, 5, 7, 2, 16, None)),
        ("uc_act", (P, P, D, _lib.UC_ACT_GELU_ERF, 480, None)),
        ("uc_ln_pe_ln", (P, D, P, P, 1e-6, P, P, P, 1e-6, P, 0, P, 2, 21, 64, None)),
        ("uc_ln_pe_ln", (P, 1, P, P, 1e-6, P, P, P, 1e-6, P, D, None, 2, 21, 64, None)),
        ("uc_ln_param_grads", (P, D, P, 0, P, P, P, 42, 64, 1e-6, None)),
        ("uc_ln_param_grads", (P, 0, P, D, P, P, P, 42, 64, 1e-6, None)),
    ]
    assert {name for name, _ in table} == set(NEW)
    for name, args in table:
        assert len(args) == len(_lib.SIGNATURES[name]) and args.count(D) == 1, name
        for code in (2, 3, -1):
            status = getattr(lib, name)(*[code if a is D else a for a in args])
            msg = lib.uc_last_error().decode()
            assert status != 0 and msg.startswith(name + ":") and f"unsupported dtype {code} " in msg, (name, code, status, msg)


@pytest.mark.parametrize("fn,args,needle", [
    ("uc_unshuffle_rows", (None, 0, P, 0, 2, 3, 5, 7, 2, 16, None), "null pointer"),
    ("uc_unshuffle_rows", (P, 0, P, 0, 2, 3, 5, 7, 2, 11, None), "ld=11 is smaller than C P P = 12"),
    ("uc_unshuffle_rows", (P, 0, P, 0, 0, 3, 5, 7, 2, 16, None), "bad shape"),
    ("uc_unshuffle_rows_bwd", (P, 0, None, 2, 3, 5, 7, 2, 16, None), "null pointer"),
    ("uc_unshuffle_rows_bwd", (P, 0, P, 2, 3, 5, 7, 0, 16, None), "bad shape"),
    ("uc_act", (P, None, 0, 1, 8, None), "bad argument"),
    ("uc_act", (P, P, 0, 0, 8, None), "bad act 0"),
    ("uc_act", (P, P, 1, 3, 8, None), "bad act 3"),
    ("uc_ln_pe_ln", (None, 0, P, P, 1e-6, P, P, P, 1e-6, P, 0, None, 2, 21, 64, None), "null pointer"),
    ("uc_ln_pe_ln", (P, 0, None, None, 0.0, None, None, None, 0.0, P, 0, None, 2, 21, 64, None), "nothing to do"),
    ("uc_ln_pe_ln", (P, 0, P, None, 1e-6, None, None, None, 0.0, P, 0, None, 2, 21, 64, None), "gamma and beta together"),
    ("uc_ln_pe_ln", (P, 0, P, P, 0.0, None, None, None, 0.0, P, 0, None, 2, 21, 64, None), "eps must be positive"),
    ("uc_ln_pe_ln", (P, 0, None, None, 0.0, P, P, P, -1.0, P, 0, None, 2, 21, 64, None), "eps must be positive"),
    ("uc_ln_pe_ln", (P, 0, P, P, 1e-6, None, None, None, 0.0, P, 0, None, 0, 21, 64, None), "bad shape"),
    ("uc_ln_pe_ln", (P, 0, P, P, 1e-6, None, None, None, 0.0, P, 0, None, 2, 21, 0, None), "bad shape"),
    ("uc_ln_param_grads", (P, 0, P, 0, P, P, None, 42, 64, 1e-6, None), "null pointer"),
    ("uc_ln_param_grads", (P, 0, P, 0, P, P, P, 0, 64, 1e-6, None), "bad shape"),
    ("uc_ln_param_grads", (P, 0, P, 0, P, P, P, 42, 64, 0.0, None), "eps must be positive"),
    ("uc_ln_param_grads", (P, 0, P, 0, P, P, P + 4, 42, 64, 1e-6, None), "8-byte aligned"),
])
def test_arguments_are_checked_before_any_launch(fn, args, needle):
    _, lib = _lib_or_build()
    status = getattr(lib, fn)(*args)
    msg = lib.uc_last_error().decode()
    assert status != 0 and msg.startswith(fn + ":") and needle in msg, msg
