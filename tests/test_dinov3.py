"""CPU: the host side of the DINOv3 ViT encoder — the axial RoPE tables against transformers' DINOv3ViTRopePositionEmbedding bit for
bit, the kernel's indexing (a torch model of uc_rope_axial) against transformers' apply_rotary_pos_emb, the train-mode coordinate
augmentation, the parameter container per size, the refusal of the size without a kernel, the checkpoint converter, the registry, and
engine.attention_route answering today's argument tuples exactly as it did before this encoder existed."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests.dinov3_formulas import rope_axial_model
from tests.golden.dinov3_cases import DINOV3_HF_CASES, HEADS, HIDDEN, dinov3_hf_config_kwargs, dinov3_hf_state_dict, dinov3_size
from tests.helpers import GOLDEN_DIR

GRIDS = ((2, 3), (3, 2), (14, 14))


def _reference_cos_sin(h, w):
    "(cos, sin) [h*w, 64] of transformers' module when it imports, else its stored values (tests/golden/dinov3_hf.npz)"
    try:
        from transformers import DINOv3ViTConfig
        from transformers.models.dinov3_vit.modeling_dinov3_vit import DINOv3ViTRopePositionEmbedding
    except ImportError:
        gold = np.load(os.path.join(GOLDEN_DIR, "dinov3_hf.npz"))
        return torch.from_numpy(gold[f"rope/{h}x{w}/cos"]), torch.from_numpy(gold[f"rope/{h}x{w}/sin"])
    rope = DINOv3ViTRopePositionEmbedding(DINOv3ViTConfig(**dinov3_hf_config_kwargs(DINOV3_HF_CASES["mlp_32x48"]))).eval()
    return rope(torch.zeros(1, 3, h * 16, w * 16))


@pytest.mark.parametrize("h,w", GRIDS)
def test_tables_equal_the_reference_cos_sin_bit_for_bit(h, w):
    from uniception_amd.models.libs.dinov3.rope import RoPEAxial
    cos, sin = _reference_cos_sin(h, w)
    ty, tx = RoPEAxial(64).tables(h, w, "cpu")
    assert ty.shape == (h, 16, 2) and tx.shape == (w, 16, 2) and ty.dtype == tx.dtype == torch.float32
    p = torch.arange(h * w)
    # the reference's [y | x | y | x] rows, rebuilt from the two tables: every one of the h*w*64 entries, no tolerance
    for k, ref in ((0, cos), (1, sin)):
        ours = torch.cat([ty[p // w, :, k], tx[p % w, :, k]], dim=-1).tile(2)
        assert torch.equal(ours, ref), (h, w, "cos" if k == 0 else "sin")
    # cached in eval: the same objects on the second call
    r = RoPEAxial(64)
    assert r.tables(h, w, "cpu")[0] is r.tables(h, w, "cpu", training=False)[0]


def test_stored_reference_tables_are_the_ones_transformers_gives_today():
    pytest.importorskip("transformers")
    gold = np.load(os.path.join(GOLDEN_DIR, "dinov3_hf.npz"))
    for h, w in GRIDS:
        cos, sin = _reference_cos_sin(h, w)
        assert np.array_equal(gold[f"rope/{h}x{w}/cos"], cos.numpy()) and np.array_equal(gold[f"rope/{h}x{w}/sin"], sin.numpy())


@pytest.mark.parametrize("h,w", GRIDS[:2])
@pytest.mark.parametrize("prefix", [5, 0])
def test_kernel_indexing_model_equals_apply_rotary_pos_emb(h, w, prefix):
    from uniception_amd.models.libs.dinov3.rope import RoPEAxial
    try:
        from transformers.models.dinov3_vit.modeling_dinov3_vit import apply_rotary_pos_emb
    except ImportError:          # transformers' function restated (modeling_dinov3_vit.py:203-268): patches * cos + rotate_half(patches) * sin
        def apply_rotary_pos_emb(q, k, cos, sin):
            def rot(t):
                n = t.shape[-2] - sin.shape[-2]
                pre, pat = t[..., :n, :], t[..., n:, :]
                half = torch.cat((-pat[..., pat.shape[-1] // 2:], pat[..., :pat.shape[-1] // 2]), dim=-1)
                return torch.cat((pre, pat * cos + half * sin), dim=-2)
            return rot(q), rot(k)
    g = torch.Generator().manual_seed(7 + h)
    B, H, D, N = 2, 3, 64, prefix + h * w
    q, k = torch.randn(B, N, H, D, generator=g, dtype=torch.float64), torch.randn(B, N, H, D, generator=g, dtype=torch.float64)
    cos, sin = _reference_cos_sin(h, w)
    qr, kr = apply_rotary_pos_emb(q.transpose(1, 2), k.transpose(1, 2), cos.double(), sin.double())
    ty, tx = RoPEAxial(D).tables(h, w, "cpu")
    for t, ref in ((q, qr), (k, kr)):
        ours = rope_axial_model(t, ty, tx, prefix, h, w)
        assert torch.equal(ours[:, :prefix], t[:, :prefix])                          # the prefix tokens: untouched
        assert torch.allclose(ours, ref.transpose(1, 2), rtol=0, atol=1e-15)         # (fp64 on fp32 tables: u c - v s vs u c + (-v) s)
        back = rope_axial_model(ours, ty, tx, prefix, h, w, inverse=True)
        assert torch.allclose(back, t, rtol=0, atol=1e-6)                            # (cos^2 + sin^2 of fp32 entries is 1 to 1e-7)


def test_augmented_coordinates_are_affine_maps_within_the_reference_ranges():
    from uniception_amd.models.libs.dinov3.rope import RoPEAxial
    h, w = 5, 7
    cy, cx = RoPEAxial.centres(h, "cpu"), RoPEAxial.centres(w, "cpu")
    assert torch.equal(cy, 2.0 * (torch.arange(0.5, h) / h) - 1.0) and float(cy[0]) == pytest.approx(-0.8) and float(cx[-1]) == pytest.approx(6 / 7)

    def affine(c2, c):          # c2 = a * c + b, solved from the end points, checked on every point
        a = float((c2[-1] - c2[0]) / (c[-1] - c[0]))
        b = float(c2[0] - a * c[0])
        assert torch.allclose(c2, a * c + b, rtol=0, atol=1e-6)
        return a, b

    torch.manual_seed(1)
    seen = []
    for _ in range(50):
        r = RoPEAxial(64, shift=0.3, jitter=1.5, rescale=2.0)
        y2, x2 = r.augmented(cy, cx)
        (ay, by), (ax, bx) = affine(y2, cy), affine(x2, cx)
        for a, b in ((ay, by), (ax, bx)):           # c' = (c + s) j m: a = j m in [1/3, 3], b / a = s in [-0.3, 0.3]
            assert 1 / (1.5 * 2.0) - 1e-6 <= a <= 1.5 * 2.0 + 1e-6 and abs(b / a) <= 0.3 + 1e-6
        seen.append((ay, ax, by / ay, bx / ax))
    assert len({round(s[0], 6) for s in seen}) > 40 and any(abs(s[0] - s[1]) > 1e-3 for s in seen) and any(abs(s[2] - s[3]) > 1e-3 for s in seen)
    for _ in range(10):                              # rescale alone: ONE factor for both axes, no offset
        y2, x2 = RoPEAxial(64, rescale=2.0).augmented(cy, cx)
        (ay, by), (ax, bx) = affine(y2, cy), affine(x2, cx)
        assert 0.5 - 1e-6 <= ay <= 2.0 + 1e-6 and ay == pytest.approx(ax, abs=1e-6) and abs(by) < 1e-6 and abs(bx) < 1e-6
    # the tables of a training call are the tables of the augmented coordinates; eval and unaugmented training calls are the plain ones
    r = RoPEAxial(64, rescale=2.0)
    torch.manual_seed(5)
    ty, tx = r.tables(h, w, "cpu", training=True)
    torch.manual_seed(5)
    y2, x2 = r.augmented(cy, cx)
    assert torch.equal(ty, r._table(y2)) and torch.equal(tx, r._table(x2)) and not torch.equal(ty, r.tables(h, w, "cpu")[0])
    plain = RoPEAxial(64)
    assert plain.tables(h, w, "cpu", training=True)[0] is plain.tables(h, w, "cpu")[0]


SIZES = {"small": (384, 12, 6, None), "small+": (384, 12, 6, 1536), "base": (768, 12, 12, None), "large": (1024, 24, 16, None),
         "huge+": (1280, 32, 20, 5120)}       # embed dim, depth, heads, SwiGLU hidden (None: the GELU MLP of 4 x dim)


@pytest.mark.parametrize("size", list(SIZES))
def test_constructor_attributes_state_dict_keys_and_shapes(size):
    from uniception_amd.models.encoders import DINOv3Encoder
    D, depth, heads, swiglu = SIZES[size]
    with torch.device("meta"):
        enc = DINOv3Encoder(name="d3", dinov3_repo_dir="/nowhere", size=size)
    assert (enc.name, enc.data_norm_type, enc.patch_size, enc.version, enc.enc_embed_dim, enc.gradient_checkpointing) == \
        ("d3", "dinov3", 16, size, D, False)
    sd = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    want = {"model.cls_token": (1, 1, D), "model.storage_tokens": (1, 4, D), "model.mask_token": (1, D),
            "model.patch_embed.proj.weight": (D, 3, 16, 16), "model.patch_embed.proj.bias": (D,), "model.rope_embed.periods": (16,),
            "model.norm.weight": (D,), "model.norm.bias": (D,)}
    for i in range(depth):
        b = f"model.blocks.{i}."
        want.update({b + "norm1.weight": (D,), b + "norm1.bias": (D,), b + "attn.qkv.weight": (3 * D, D), b + "attn.qkv.bias": (3 * D,),
                     b + "attn.qkv.bias_mask": (3 * D,), b + "attn.proj.weight": (D, D), b + "attn.proj.bias": (D,), b + "ls1.gamma": (D,),
                     b + "norm2.weight": (D,), b + "norm2.bias": (D,), b + "ls2.gamma": (D,)})
        if swiglu:
            want.update({b + "mlp.w1.weight": (swiglu, D), b + "mlp.w1.bias": (swiglu,), b + "mlp.w2.weight": (swiglu, D),
                         b + "mlp.w2.bias": (swiglu,), b + "mlp.w3.weight": (D, swiglu), b + "mlp.w3.bias": (D,)})
        else:
            want.update({b + "mlp.fc1.weight": (4 * D, D), b + "mlp.fc1.bias": (4 * D,), b + "mlp.fc2.weight": (D, 4 * D), b + "mlp.fc2.bias": (D,)})
    assert sd == want
    blk = enc.model.blocks[0]
    assert blk.attn.num_heads == heads and D // heads == 64 and blk.norm1.eps == blk.norm2.eps == enc.model.norm.eps == 1e-5
    assert not any("rope" in k and "periods" not in k for k in sd)                   # the rope object: outside the state_dict
    assert enc.model.rope.base == 100.0 and enc.model.rope.rescale == 2.0 and enc.model.rope.shift is None and enc.model.rope.jitter is None


def test_bias_mask_periods_and_the_constructor_signature():
    from uniception_amd.models.encoders import DINOv3Encoder, DINOv3IntermediateFeatureReturner
    enc = DINOv3Encoder(name="d3", size=dinov3_size(DINOV3_HF_CASES["gated_32x48"]), keep_first_n_layers=1)
    assert len(enc.model.blocks) == 1
    m = enc.model.blocks[0].attn.qkv.bias_mask
    assert torch.equal(m, torch.cat([torch.ones(HIDDEN), torch.zeros(HIDDEN), torch.ones(HIDDEN)]))
    assert torch.allclose(enc.model.rope_embed.periods, 1 / enc.model.rope.inv_freq, rtol=1e-6)
    # the reference's parameters, in its order, in front of this project's own
    ref = ["self", "name", "dinov3_repo_dir", "data_norm_type", "patch_size", "size", "weights", "pretrained_checkpoint_path",
           "gradient_checkpointing", "keep_first_n_layers", "disable_torch_compile_for_pe"]
    assert list(inspect.signature(DINOv3Encoder.__init__).parameters)[:len(ref)] == ref
    assert list(inspect.signature(DINOv3IntermediateFeatureReturner.__init__).parameters)[:len(ref) + 2] == ref + ["indices", "norm_intermediate"]
    ret = DINOv3IntermediateFeatureReturner(name="d3", dinov3_repo_dir=None, size=dinov3_size(DINOV3_HF_CASES["mlp_32x48"]), indices=[0, 1],
                                            norm_intermediate=False, gradient_checkpointing=True)
    assert ret.indices == [0, 1] and ret.norm_intermediate is False and type(ret.model.blocks[0]).__name__ == "Checkpointed_Block"


def test_the_size_without_a_kernel_is_refused_by_name():
    from uniception_amd.engine import UcHipError
    from uniception_amd.models.encoders import DINOv3Encoder
    with pytest.raises(UcHipError, match="head_dim 128"):
        DINOv3Encoder(name="d3", size="7b")
    with pytest.raises(UcHipError, match="unknown DINOv3 size"):
        DINOv3Encoder(name="d3", size="giant")
    with pytest.raises(UcHipError, match="head_dim 32"):
        DINOv3Encoder(name="d3", size=dict(embed_dim=128, depth=1, num_heads=4))


@pytest.mark.parametrize("name", ["mlp_32x48", "gated_48x32"])
def test_converter_round_trip_on_the_tiny_configuration(name, tmp_path):
    from uniception_amd.models.encoders import DINOv3Encoder
    from uniception_amd.tools import convert_checkpoint as cc
    c = DINOV3_HF_CASES[name]
    hf = dinov3_hf_state_dict(c)
    src, out = tmp_path / "hf.pth", tmp_path / "uc.pth"
    torch.save(hf, src)
    cc.main([str(src), str(out), "--mode", "dinov3", "--num-heads", str(HEADS)])
    enc = DINOv3Encoder(name="d3", dinov3_repo_dir=None, size=dinov3_size(c), pretrained_checkpoint_path=str(out))      # strict load
    sd = enc.state_dict()
    assert set(torch.load(out)["model"]) == set(sd)
    D = HIDDEN
    for i in range(2):
        b, h = f"model.blocks.{i}.", f"model.layer.{i}."
        qw, kw, vw = sd[b + "attn.qkv.weight"].split(D, 0)
        qb, kb, vb = sd[b + "attn.qkv.bias"].split(D, 0)
        assert torch.equal(qw, hf[h + "attention.q_proj.weight"]) and torch.equal(kw, hf[h + "attention.k_proj.weight"])
        assert torch.equal(vw, hf[h + "attention.v_proj.weight"]) and torch.equal(qb, hf[h + "attention.q_proj.bias"])
        assert torch.equal(vb, hf[h + "attention.v_proj.bias"]) and not kb.any()
        assert torch.equal(sd[b + "attn.qkv.bias_mask"].split(D, 0)[1], torch.zeros(D)) and sd[b + "attn.qkv.bias_mask"].sum() == 2 * D
        assert torch.equal(sd[b + "ls1.gamma"], hf[h + "layer_scale1.lambda1"]) and torch.equal(sd[b + "ls2.gamma"], hf[h + "layer_scale2.lambda1"])
        assert torch.equal(sd[b + "attn.proj.weight"], hf[h + "attention.o_proj.weight"])
        if c["gated"]:
            for ours, theirs in (("w1", "gate_proj"), ("w2", "up_proj"), ("w3", "down_proj")):
                assert torch.equal(sd[b + f"mlp.{ours}.weight"], hf[h + f"mlp.{theirs}.weight"]) and torch.equal(sd[b + f"mlp.{ours}.bias"], hf[h + f"mlp.{theirs}.bias"])
        else:
            for ours, theirs in (("fc1", "up_proj"), ("fc2", "down_proj")):
                assert torch.equal(sd[b + f"mlp.{ours}.weight"], hf[h + f"mlp.{theirs}.weight"])
    assert torch.equal(sd["model.storage_tokens"], hf["embeddings.register_tokens"]) and torch.equal(sd["model.cls_token"], hf["embeddings.cls_token"])
    assert torch.equal(sd["model.patch_embed.proj.weight"], hf["embeddings.patch_embeddings.weight"]) and sd["model.mask_token"].shape == (1, D)
    assert torch.equal(sd["model.rope_embed.periods"], enc.model.rope_embed.periods)
    with pytest.raises(KeyError, match="unexpected key embeddings.position_embeddings"):
        cc.dinov3_hf_to_uniception(dict(hf, **{"embeddings.position_embeddings": torch.zeros(1)}))


def test_registry_factories_and_normalisation():
    from uniception_amd.models import encoders as E
    cfg = E.ENCODER_CONFIGS["dinov3"]
    assert cfg["class"] is E.DINOv3Encoder and cfg["intermediate_feature_returner_class"] is E.DINOv3IntermediateFeatureReturner
    assert "dinov3" in E.get_available_encoders() and cfg["supported_models"] == ["DINOv3-ViT"]
    norm = E.IMAGE_NORMALIZATION_DICT["dinov3"]
    assert torch.allclose(norm.mean, torch.tensor([0.485, 0.456, 0.406])) and torch.allclose(norm.std, torch.tensor([0.229, 0.224, 0.225]))
    size = dinov3_size(DINOV3_HF_CASES["mlp_32x48"])
    enc = E.encoder_factory("dinov3", name="f", dinov3_repo_dir="ignored", size=size)
    assert isinstance(enc, E.DINOv3Encoder) and enc.enc_embed_dim == HIDDEN
    ret = E.feature_returner_encoder_factory("dinov3", name="f", dinov3_repo_dir="ignored", size=size, indices=2)
    assert isinstance(ret, E.DINOv3IntermediateFeatureReturner) and ret.indices == 2 and ret.norm_intermediate is True


def test_the_bound_rope_is_the_second_native_kind_and_nothing_else():
    from uniception_amd import engine
    from uniception_amd.models.libs.croco.pos_embed import RoPE2D
    from uniception_amd.models.libs.dinov3.rope import RoPEAxial
    bound = RoPEAxial(64).bind(5, 2, 3, "cpu")
    assert engine.is_axial_rope(bound) and not engine.is_native_rope(bound) and engine._rope_epilogue(bound, None, 128) is None
    assert not engine.is_axial_rope(None) and not engine.is_axial_rope(RoPE2D(freq=100.0)) and not engine.is_axial_rope(lambda t, p: t)
    assert (bound.prefix, bound.grid_h, bound.grid_w) == (5, 2, 3) and bound.table_y.shape == (2, 16, 2) and bound.table_x.shape == (3, 16, 2)
    with pytest.raises(engine.UcHipError, match="not a positional-encoding callable"):
        bound(torch.zeros(1), None)
    with pytest.raises(engine.UcHipError, match="self-attention only"), torch.no_grad():
        engine.cross_attention(torch.zeros(6, 128), torch.zeros(6, 128), 1, 6, 6, None, None, None, None, 2, bound, None, None, 0.125, None, torch.float32)


# engine.attention_route(dtype, head_dim, native_rope, qk_norm, separate_v, n_keys, has_rope) [under attention_precision("fp8")] -> route,
# as the commit before this encoder answered ("raises": UcHipError) — recorded from a checkout of that commit, not from this code
ROUTES_BEFORE = """
bfloat16 64 1 0 0 1024 0 0 vt_epilogue|bfloat16 64 1 0 0 1024 0 1 fp8|bfloat16 64 1 0 0 1024 1 0 vt_epilogue|bfloat16 64 1 0 0 1024 1 1 fp8
bfloat16 64 1 0 0 1370 0 0 vt_pack|bfloat16 64 1 0 0 1370 0 1 fp8|bfloat16 64 1 0 0 1370 1 0 vt_pack|bfloat16 64 1 0 0 1370 1 1 fp8
bfloat16 64 1 0 0 35 0 0 vt_pack|bfloat16 64 1 0 0 35 0 1 fp8|bfloat16 64 1 0 0 35 1 0 vt_pack|bfloat16 64 1 0 0 35 1 1 fp8
bfloat16 64 1 0 1 1024 0 0 unfused|bfloat16 64 1 0 1 1024 0 1 unfused|bfloat16 64 1 0 1 1024 1 0 unfused|bfloat16 64 1 0 1 1024 1 1 unfused
bfloat16 64 1 1 0 1024 0 0 unfused|bfloat16 64 1 1 0 1024 0 1 unfused|bfloat16 64 1 1 0 1024 1 0 unfused|bfloat16 64 1 1 0 1024 1 1 unfused
bfloat16 64 1 1 0 1370 0 0 unfused|bfloat16 64 1 1 0 1370 1 1 unfused|bfloat16 64 1 1 0 35 0 0 unfused|bfloat16 64 1 1 0 35 1 1 unfused
bfloat16 64 0 0 0 1024 0 0 unfused|bfloat16 64 0 0 0 1024 0 1 unfused|bfloat16 64 0 0 0 1024 1 0 unfused|bfloat16 64 0 0 0 1024 1 1 unfused
bfloat16 64 0 0 0 1370 0 0 unfused|bfloat16 64 0 0 0 1370 1 1 unfused|bfloat16 64 0 0 0 35 0 0 unfused|bfloat16 64 0 0 0 35 1 1 unfused
bfloat16 64 0 0 1 1024 0 0 unfused|bfloat16 64 0 0 1 1024 1 1 unfused|bfloat16 64 0 1 0 1024 0 0 unfused|bfloat16 64 0 1 0 1024 1 1 unfused
bfloat16 64 0 1 0 1370 1 0 unfused|bfloat16 64 0 1 0 35 0 1 unfused
bfloat16 80 1 0 0 1370 0 0 wide|bfloat16 80 1 0 0 1370 1 0 raises|bfloat16 80 1 1 0 1370 0 0 raises|bfloat16 80 1 1 0 1370 1 0 raises
bfloat16 80 0 0 0 1370 0 0 raises|bfloat16 80 0 0 0 1370 1 0 raises|bfloat16 80 0 1 0 1370 0 0 raises|bfloat16 80 0 1 0 1370 1 0 raises
bfloat16 128 1 0 0 1370 0 0 raises|bfloat16 128 1 0 0 1370 1 0 raises|bfloat16 128 1 1 0 1370 0 0 raises|bfloat16 128 0 0 0 1370 1 0 raises
float32 64 1 0 0 1024 0 0 unfused|float32 64 1 0 0 1024 1 0 unfused|float32 64 1 1 0 1024 0 0 unfused|float32 64 1 1 0 1024 1 0 unfused
float32 64 0 0 0 1024 0 0 unfused|float32 64 0 0 0 1024 1 0 unfused|float32 64 0 1 0 1024 0 0 unfused|float32 64 0 1 0 1024 1 0 unfused
float32 32 1 0 0 1024 0 0 unfused|float32 32 1 0 0 1024 1 0 unfused|float32 32 1 1 0 1024 1 0 unfused|float32 32 0 0 0 1024 1 0 unfused
float16 64 1 0 0 35 0 0 unfused|float16 64 1 0 0 35 1 0 unfused|float16 64 0 0 0 35 0 0 unfused|float16 64 0 0 0 35 1 0 unfused
"""


def test_attention_route_answers_todays_argument_tuples_as_before():
    from uniception_amd import engine
    rows = [r.split() for line in ROUTES_BEFORE.strip().splitlines() for r in line.split("|")]
    assert len(rows) == 66
    for dt, hd, native, qkn, sep, nk, has_rope, fp8, want in rows:
        args = (getattr(torch, dt), int(hd), native == "1", qkn == "1", sep == "1", int(nk))
        try:
            with torch.no_grad():
                if fp8 == "1":
                    with engine.attention_precision("fp8"):
                        got = engine.attention_route(*args, has_rope=has_rope == "1")
                else:
                    got = engine.attention_route(*args, has_rope=has_rope == "1")
        except engine.UcHipError:
            got = "raises"
        assert got == want, (dt, hd, native, qkn, sep, nk, has_rope, fp8, got, want)
