"""CPU: the Perception Encoder mirror (models/libs/perception_encoder/vision_encoder, encoders/perception_encoder.py) carries the
reference's module paths, factory entries, config table, state_dict keys / shapes / order and constructor signatures
(tests/golden/perception_encoder_<case>.npz and pe_configs.json, written by tests/golden/make_golden_perception_encoder.py from the real
reference classes), its refusals, its two block-count quirks, and the channel permutation that lets the RoPE kernels of this package
serve the reference's interleaved RoPE layout.

Permutation tolerance: q and k gathered with the mirror's permutation and rotated by the oracle's CroCo RoPE-2D (base 10000, the
positions the mirror builds) against the reference's own Rope2D output (fixture rope/) gathered alike, and the scores q k^T against the
unpermuted reference scores: 1e-5 absolute.  The two differ by the fp32 rounding of the angle table the reference keeps (measured
1e-6 on these randn inputs at head_dim 64); the bound is ten times that — a wrong frequency, axis or offset moves values by order 1."""
import importlib
import json
import os
from dataclasses import asdict

import numpy as np
import pytest
import torch

from tests.golden.input_encoders_cases import keys_of, signature
from tests.golden.perception_encoder_cases import CASES, CONFIG_NAME, CONFIGS, ROPE_GRID, fill, kwargs, rope_inputs
from tests.helpers import GOLDEN_DIR

P = 4096      # a pointer that is never dereferenced: every call that receives it here is rejected before any launch


def _gold(name):
    return np.load(os.path.join(GOLDEN_DIR, f"perception_encoder_{name}.npz"))


def _pe():
    return importlib.import_module("uniception_amd.models.libs.perception_encoder.vision_encoder.pe")


def _config():
    return importlib.import_module("uniception_amd.models.libs.perception_encoder.vision_encoder.config")


def _build(name, monkeypatch, **extra):
    "the wrapper of case `name` around its tiny tower, put into the config table under the published name it stands in for"
    from uniception_amd.models import encoders as E
    kind, cfg, key = CASES[name][:3]
    monkeypatch.setitem(_config().PE_VISION_CONFIG, CONFIG_NAME[key], _config().PEConfig(**CONFIGS[cfg]))
    return getattr(E, kind)(**kwargs(name), **extra)


def test_classes_are_importable_at_the_reference_module_paths():
    from uniception_amd.models import encoders as E
    from uniception_amd.models.encoders.perception_encoder import PerceptionEncoder, PerceptionEncoderIntermediateFeatureReturner
    from uniception_amd.models.libs.perception_encoder.vision_encoder import config, pe
    from uniception_amd.models.utils.intermediate_feature_return import IntermediateFeatureReturner
    assert E.PerceptionEncoder is PerceptionEncoder and E.PerceptionEncoderIntermediateFeatureReturner is PerceptionEncoderIntermediateFeatureReturner
    assert issubclass(PerceptionEncoderIntermediateFeatureReturner, (PerceptionEncoder, IntermediateFeatureReturner))
    for attr in ("VisionTransformer", "Transformer", "ResidualAttentionBlock", "SelfAttention", "AttentionPooling", "LayerScale"):
        assert hasattr(pe, attr)
    assert hasattr(config, "PEConfig") and hasattr(config, "PE_VISION_CONFIG") and not hasattr(config, "fetch_pe_checkpoint")


def test_factory_entry_supported_models_and_normalization():
    from uniception_amd.models import encoders as E
    cfg = E.ENCODER_CONFIGS["perception_encoder"]
    assert cfg["class"] is E.PerceptionEncoder and cfg["intermediate_feature_returner_class"] is E.PerceptionEncoderIntermediateFeatureReturner
    assert cfg["supported_models"] == ["Perception Encoder Core", "Preception Encoder Spatial"]          # (the reference's spelling)
    assert "perception_encoder" in E.get_available_encoders()
    norm = E.IMAGE_NORMALIZATION_DICT["perception_encoder"]
    assert torch.equal(norm.mean, torch.tensor([0.5, 0.5, 0.5])) and torch.equal(norm.std, torch.tensor([0.5, 0.5, 0.5]))


def test_config_table_and_wrapper_map_equal_the_reference():
    from uniception_amd.models.encoders.perception_encoder import MODEL_CKPT_DICT
    want = json.load(open(os.path.join(GOLDEN_DIR, "pe_configs.json")))
    got = json.loads(json.dumps({k: asdict(v) for k, v in _config().PE_VISION_CONFIG.items()}))       # (tuples -> lists, as in the file)
    assert got == want["configs"]
    assert {f"{a}/{b}": c for (a, b), c in MODEL_CKPT_DICT.items()} == want["wrapper"]
    assert signature(_config().PEConfig) == "\n".join(
        f"{k}" if k in ("patch_size", "width", "layers", "heads", "mlp_ratio", "output_dim") else f"{k}={v!r}"
        for k, v in [("patch_size", 0), ("width", 0), ("layers", 0), ("heads", 0), ("mlp_ratio", 0), ("output_dim", 0), ("ls_init_value", None),
                     ("drop_path", 0.0), ("image_size", (224,)), ("use_abs_posemb", True), ("use_cls_token", False), ("use_rope2d", True),
                     ("pool_type", "attn"), ("attn_pooler_heads", 8), ("use_ln_pre", True), ("use_ln_post", True)])


@pytest.mark.parametrize("name", list(CASES))
def test_keys_shapes_order_and_signature_equal_the_reference(name, monkeypatch):
    from uniception_amd.models import encoders as E
    G = _gold(name)
    model = _build(name, monkeypatch)
    assert keys_of(model).split("\n") == str(G[f"{name}/keys"]).split("\n")
    assert signature(getattr(E, CASES[name][0])).split("\n") == str(G[f"{name}/signature"]).split("\n")
    assert "rope" not in "".join(model.state_dict()) and not any("rope" in n for n, _ in model.named_modules())
    # load_state_dict of the reference's keys, unused pooling parameters included
    other = _build(name, monkeypatch)
    fill(model)
    res = other.load_state_dict(model.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_vision_transformer_constructor_signature_equals_the_reference():
    "restated from the reference's pe.py:304-325 (it is not a fixture: the defaults hold nn classes)"
    import inspect
    p = inspect.signature(_pe().VisionTransformer.__init__).parameters
    assert list(p)[1:] == ["patch_size", "width", "layers", "heads", "mlp_ratio", "act_layer", "norm_layer", "use_ln_pre", "use_ln_post", "ls_init_value",
                           "drop_path", "image_size", "use_abs_posemb", "use_rope2d", "use_cls_token", "output_dim", "attn_pooler_heads", "pool_type"]
    assert (p["image_size"].default, p["output_dim"].default, p["attn_pooler_heads"].default, p["pool_type"].default) == (448, 1280, 8, "attn")
    assert p["use_cls_token"].default is False and p["use_rope2d"].default is True and p["norm_layer"].default.keywords == {"eps": 1e-5}


def test_unsupported_combinations_raise_what_the_issue_of_each_is():
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.encoders import PerceptionEncoder
    for ctype in ("core", "lang", "spatial"):
        with pytest.raises(UcHipError, match="head_dim 96") as e:
            PerceptionEncoder(name="x", size="giant", checkpoint_type=ctype)
        assert "head_dim-64 attention kernels" in str(e.value)
    with pytest.raises(RuntimeError, match="PE-Lang-B16-224 not found in configs."):
        PerceptionEncoder(name="x", size="base", checkpoint_type="lang")
    with pytest.raises(ValueError, match="Unsupported combination of checkpoint_type 'spatial' and size 'large'"):
        PerceptionEncoder(name="x", size="large", checkpoint_type="spatial")
    with pytest.raises(UcHipError, match="drop_path"):
        _pe().VisionTransformer(**dict(CONFIGS["lang_ls"], drop_path=0.1))
    with pytest.raises(UcHipError, match="checkpoint_path"):
        _pe().VisionTransformer.from_config("PE-Core-B16-224", pretrained=True)
    tower = _pe().VisionTransformer(**CONFIGS["core_cls"])
    with pytest.raises(UcHipError, match="pooled CLIP embedding"):
        tower(torch.zeros(1, 3, 56, 56))


def test_truncate_and_integer_n_keep_the_reference_arithmetic(monkeypatch):
    tower = _pe().VisionTransformer(**CONFIGS["core_cls"])
    tower.truncate(1)                                  # ((3 + 1) % 3) + 1
    assert len(tower.transformer.resblocks) == tower.layers == tower.transformer.layers == 2
    tower = _pe().VisionTransformer(**CONFIGS["core_cls"])
    tower.truncate(-1)                                 # ((3 - 1) % 3) + 1: nothing goes
    assert len(tower.transformer.resblocks) == 3
    assert len(_build("ret_trunc", monkeypatch).model.transformer.resblocks) == 2
    # which blocks a call taps: an integer n is the SINGLE layer len - n
    seen = []
    monkeypatch.setattr(_pe().VisionTransformer, "_blocks", lambda self, x, taps: seen.append(list(taps)) or ([torch.zeros(2, 4)] * len(taps), 1, 2))
    monkeypatch.setattr(_pe().VisionTransformer, "_finish", lambda self, o, B, T, norm, strip: o)
    tower = _pe().VisionTransformer(**CONFIGS["core_cls"])
    assert len(tower.get_intermediate_layers(None, n=1)) == 1 and len(tower.get_intermediate_layers(None, n=3)) == 1
    assert len(tower.get_intermediate_layers(None, n=[0, 2])) == 2 and len(tower.get_intermediate_layers(None, n=range(3))) == 3
    tower.forward_features(None)
    tower.forward_features(None, layer_idx=1)
    assert seen == [[2], [0], [0, 2], [0, 1, 2], [2], [1]]


def test_gradient_checkpointing_wraps_every_block_and_keeps_the_keys(monkeypatch):
    m = _build("core_cls", monkeypatch, gradient_checkpointing=True)
    assert [type(b).__name__ for b in m.model.transformer.resblocks] == ["CheckpointedResidualAttentionBlock"] * 3
    assert keys_of(m) == keys_of(_build("core_cls", monkeypatch))
    m.model.set_grad_checkpointing(False)
    assert [type(b).__name__ for b in m.model.transformer.resblocks] == ["ResidualAttentionBlock"] * 3


def test_permutation_is_a_bijection_per_head_and_leaves_v_alone():
    pe = _pe()
    perm = pe.head_channel_permutation(64)
    assert sorted(perm.tolist()) == list(range(64))
    # the issue's table: y half n = r 16 + i -> 32 + 2 i + r, x half n = 32 + r 16 + i -> 2 i + r
    for r in (0, 1):
        for i in range(16):
            assert perm[r * 16 + i] == 32 + 2 * i + r and perm[32 + r * 16 + i] == 2 * i + r
    W, H = 128, 2
    rows = pe.rope_row_permutation(W, H)
    assert sorted(rows.tolist()) == list(range(3 * W)) and torch.equal(rows[2 * W:], torch.arange(2 * W, 3 * W))
    for blk in range(2):                       # q, k: every head's rows stay inside the head
        for h in range(H):
            seg = rows[blk * W + h * 64: blk * W + (h + 1) * 64]
            assert torch.equal(seg, blk * W + h * 64 + perm)
    attn = pe.SelfAttention(W, H, rope=object())
    attn.init_tensors()
    proj = attn.in_proj(False)
    assert torch.equal(proj.weight, attn.in_proj_weight.detach()[rows]) and torch.equal(proj.bias, attn.in_proj_bias.detach()[rows])
    assert list(attn.state_dict()) == ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
    assert attn.in_proj(False) is proj                             # cached per version of the parameters ...
    with torch.no_grad():
        attn.in_proj_bias.add_(1.0)
    assert torch.equal(attn.in_proj(False).bias, attn.in_proj_bias.detach()[rows])          # ... and rebuilt after an update
    train = attn.in_proj(True)                                     # training: a differentiable gather, gradients in the stored order
    (train.weight * torch.arange(3 * W, dtype=torch.float32)[:, None]).sum().backward()
    want = torch.empty(3 * W)
    want[rows] = torch.arange(3 * W, dtype=torch.float32)
    assert torch.equal(attn.in_proj_weight.grad, want[:, None].expand(3 * W, W))
    plain = pe.SelfAttention(W, H, rope=None)
    assert plain.in_proj(True).weight is plain.in_proj_weight


@pytest.mark.parametrize("tag,with_cls", [("cls", True), ("nocls", False)])
def test_permuted_croco_rope_equals_the_reference_rope(tag, with_cls):
    from oracle import dust3r_oracle as O
    G = _gold("rope")
    tower = _pe().VisionTransformer(**dict(CONFIGS["lang_ls"], use_cls_token=with_cls))
    assert tower.rope.base == 10000.0 and tower.rope.F0 == 1.0
    pos = tower.rope_positions(1, *ROPE_GRID, torch.device("cpu"))
    n = ROPE_GRID[0] * ROPE_GRID[1] + int(with_cls)
    assert pos.dtype == torch.int64 and tuple(pos.shape) == (1, n, 2) and tower.rope_positions(1, *ROPE_GRID, torch.device("cpu")) is pos
    if with_cls:
        assert pos[0, 0].tolist() == [0, 0] and pos[0, 1].tolist() == [1, 1] and pos[0, -1].tolist() == [ROPE_GRID[0], ROPE_GRID[1]]
    else:
        assert pos[0, 0].tolist() == [0, 0] and pos[0, -1].tolist() == [ROPE_GRID[0] - 1, ROPE_GRID[1] - 1]
    perm = _pe().head_channel_permutation(64)
    q, k = rope_inputs(with_cls)
    ref_q, ref_k = torch.from_numpy(G[f"rope/{tag}/q"]), torch.from_numpy(G[f"rope/{tag}/k"])
    got_q = O.rope2d(q[..., perm], pos, base=10000.0, F0=1.0)
    got_k = O.rope2d(k[..., perm], pos, base=10000.0, F0=1.0)
    eq, ek = float((got_q - ref_q[..., perm]).abs().max()), float((got_k - ref_k[..., perm]).abs().max())
    es = float((got_q @ got_k.transpose(-1, -2) - ref_q @ ref_k.transpose(-1, -2)).abs().max())
    print(f"rope {tag}: rotated q {eq:.3e}, k {ek:.3e}, scores {es:.3e} (bound 1e-5)")
    assert eq <= 1e-5 and ek <= 1e-5 and es <= 1e-5
    # the check can fail: CroCo's own base, or the positions without the class-token offset, are far outside the bound
    assert float((O.rope2d(q[..., perm], pos, base=100.0) - ref_q[..., perm]).abs().max()) > 1e-2
    assert float((O.rope2d(q[..., perm], pos.flip(-1), base=10000.0) - ref_q[..., perm]).abs().max()) > 1e-2


@pytest.mark.parametrize("form", ["bare", "state_dict", "weights", "module", "clip"])
def test_converter_round_trip(form, tmp_path, monkeypatch, capsys):
    from uniception_amd.tools import convert_checkpoint as cc
    model = _build("core_cls", monkeypatch)
    fill(model)
    tower = {k: v.clone() for k, v in model.model.state_dict().items()}
    ckpt = {"bare": tower, "state_dict": {"state_dict": tower}, "weights": {"weights": tower},
            "module": {"state_dict": {"module." + k: v for k, v in tower.items()}},
            "clip": {"state_dict": {**{"module.visual." + k: v for k, v in tower.items()}, "module.logit_scale": torch.ones(()),
                                    "module.token_embedding.weight": torch.zeros(4, 4)}}}[form]
    src, out = str(tmp_path / "pe.pt"), str(tmp_path / "out.pth")
    torch.save(ckpt, src)
    cc.main([src, out, "--mode", "perception_encoder", "--pe-config", CONFIG_NAME[CASES["core_cls"][2]]])
    converted = torch.load(out, weights_only=False)
    assert list(converted) == ["model"] and list(converted["model"]) == list(model.state_dict())
    loaded = _build("core_cls", monkeypatch, pretrained_checkpoint_path=out)
    assert "<All keys matched successfully>" in capsys.readouterr().out
    for (k, u), (_, v) in zip(model.state_dict().items(), loaded.state_dict().items()):
        assert torch.equal(u, v), k
    if form == "bare":
        # the tower's own load_ckpt takes the original forms too
        t2 = _pe().VisionTransformer.from_config(CONFIG_NAME[CASES["core_cls"][2]], pretrained=True, checkpoint_path=src)
        assert all(torch.equal(u, v) for u, v in zip(t2.state_dict().values(), tower.values()))
        missing = {k: v for k, v in tower.items() if k != "ln_pre.bias"}
        with pytest.raises(KeyError, match="missing key ln_pre.bias"):
            cc.perception_encoder_to_uniception(missing, CONFIG_NAME[CASES["core_cls"][2]])
        with pytest.raises(KeyError, match="unexpected key text_projection"):
            cc.perception_encoder_to_uniception({**tower, "text_projection": torch.zeros(2)}, CONFIG_NAME[CASES["core_cls"][2]])
        with pytest.raises(ValueError, match="positional_embedding has shape"):
            cc.perception_encoder_to_uniception({**tower, "positional_embedding": torch.zeros(5, 128)}, CONFIG_NAME[CASES["core_cls"][2]])


def test_cpu_tensors_are_refused_and_the_input_checks_are_the_reference_ones(monkeypatch):
    from uniception_amd._lib import UcHipError
    from uniception_amd.models.encoders import ViTEncoderInput
    for name in ("core_cls", "ret_norm"):
        m = _build(name, monkeypatch)
        with pytest.raises(UcHipError, match="HIP device only"):
            m(ViTEncoderInput(data_norm_type="perception_encoder", image=torch.zeros(1, 3, 56, 56)))
        with pytest.raises(AssertionError, match="does not match the encoder's normalization type"):
            m(ViTEncoderInput(data_norm_type="dinov2", image=torch.zeros(1, 3, 56, 56)))
        with pytest.raises(AssertionError, match="divisible by patch size"):
            m(ViTEncoderInput(data_norm_type="perception_encoder", image=torch.zeros(1, 3, 56, 57)))
        with pytest.raises(AssertionError, match="must have 3 channels"):
            m(ViTEncoderInput(data_norm_type="perception_encoder", image=torch.zeros(1, 2, 56, 56)))


def _lib_or_build():
    from uniception_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib, _lib.load()


def test_stem_symbols_are_declared_bound_and_exported():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "uc_hip.h")).read(), flags=re.S)
    _lib, lib = _lib_or_build()
    for name in ("uc_vit_stem", "uc_vit_stem_bwd", "uc_vit_stem_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/uc_hip.h"
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.uc_abi_version() >= 21 and _lib.ABI_VERSION >= 21
    # B = 9 -> 2 slabs of 8 images, T = 17 -> 3 groups of 8 tokens: 2 * 17 * C for dpos, 2 * 3 * 2 * C for dgamma / dbeta
    assert lib.uc_vit_stem_ws_bytes(9, 17, 128) == 4 * (2 * 17 * 128 + 2 * 3 * 2 * 128)
    from uniception_amd import autograd, ops
    assert callable(ops.vit_stem) and callable(ops.vit_stem_bwd) and callable(autograd.vit_stem)


@pytest.mark.parametrize("fn,args,needle", [
    ("uc_vit_stem", (P, 0, P, P, P, P, 1e-5, None, 0, None, 2, 15, 128, None), "null pointer"),
    ("uc_vit_stem", (P, 0, P, P, P, P, 1e-5, P, 0, None, 2, 15, 12, None), "C=12 must be a multiple of 8"),
    ("uc_vit_stem", (P, 0, P, P, P, P, 1e-5, P, 0, None, 2, 15, 4096, None), "at most 2048"),
    ("uc_vit_stem", (P, 0, P, P, P, P, 1e-5, P, 0, None, 0, 15, 128, None), "bad shape"),
    ("uc_vit_stem", (P, 0, P, P, P, None, 1e-5, P, 0, None, 2, 15, 128, None), "gamma and beta together"),
    ("uc_vit_stem", (P, 0, P, P, P, P, 0.0, P, 0, None, 2, 15, 128, None), "eps must be positive"),
    ("uc_vit_stem", (P, 0, P, P, None, None, 0.0, P, 0, P, 2, 15, 128, None), "stats without a LayerNorm"),
    ("uc_vit_stem", (P, 0, P + 4, P, P, P, 1e-5, P, 0, None, 2, 15, 128, None), "16-byte aligned"),
    ("uc_vit_stem", (P, 3, P, P, P, P, 1e-5, P, 0, None, 2, 15, 128, None), "unsupported dtype 3"),
    ("uc_vit_stem_bwd", (P, 0, P, 0, P, P, P, P, P, P, P, P, P, None, 2, 15, 128, None), "null pointer"),
    ("uc_vit_stem_bwd", (P, 0, P, 0, P, P, P, P, P, P, P, P, P, P, 2, 15, 12, None), "C=12 must be a multiple of 8"),
    ("uc_vit_stem_bwd", (P, 0, P, 0, P, P, P, None, P, P, P, P, P, P, 2, 15, 128, None), "needs the forward's stats"),
    ("uc_vit_stem_bwd", (P, 0, P, 0, P, P, None, None, P, P, P, P, None, P, 2, 15, 128, None), "dgamma / dbeta without a LayerNorm"),
    ("uc_vit_stem_bwd", (P, 0, P, 0, None, P, P, P, P, P, P, P, P, P, 2, 15, 128, None), "dcls without a class token"),
    ("uc_vit_stem_bwd", (P, 0, P, 0, P, None, P, P, P, P, P, P, P, P, 2, 15, 128, None), "dpos without a position table"),
    ("uc_vit_stem_bwd", (P, 0, P, 2, P, P, P, P, P, P, P, P, P, P, 2, 15, 128, None), "unsupported dtype 2"),
])
def test_stem_arguments_are_checked_before_any_launch(fn, args, needle):
    _lib, lib = _lib_or_build()
    assert len(args) == len(_lib.SIGNATURES[fn])
    status = getattr(lib, fn)(*args)
    msg = lib.uc_last_error().decode()
    assert status == -1 and msg.startswith(fn + ":") and needle in msg, msg
