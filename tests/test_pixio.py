"""CPU: the PixioEncoder mirror against the fixtures of the real reference class (tests/golden/pixio_<case>.npz) — state_dict keys, shapes and
order in both key layouts, the constructor's signature, the factories, the registry and normalisation entries, the refusal to download —
and the routing of its head dims: engine.attention_route gives "wide" for bf16 at head_dim 80 / 96, raises for qk_norm and RoPE there,
and keeps the old messages for head dims without a kernel."""
import os

import numpy as np
import pytest
import torch

from tests.golden.input_encoders_cases import keys_of, signature
from tests.golden.pixio_cases import CASES, fill, kwargs, plain_key
from tests.helpers import GOLDEN_DIR


def gold(name):
    return np.load(os.path.join(GOLDEN_DIR, f"pixio_{name}.npz"))


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_keys_shapes_and_order_match_the_reference(name):
    from uniception_amd.models.encoders import PixioEncoder
    model = PixioEncoder(**kwargs(name))
    assert keys_of(model) == str(gold(name)[f"{name}/keys"])
    inner = [k for k in model.state_dict() if ".inner." in k]
    assert bool(inner) == CASES[name][3]      # blocks.N.inner.* exactly under gradient checkpointing


def test_both_key_layouts_hold_the_same_weights_under_the_cases_filler():
    from uniception_amd.models.encoders import PixioEncoder
    a, b = PixioEncoder(**kwargs("h80")), PixioEncoder(**kwargs("h80_nockpt"))
    fill(a, "h80")
    fill(b, "h80_nockpt")
    sb = b.state_dict()
    assert all(torch.equal(v, sb[plain_key(k)]) for k, v in a.state_dict().items())


def test_constructor_signature_is_the_reference_plus_the_checkpoint_path():
    from uniception_amd.models.encoders import PixioEncoder
    ref = str(gold("h80")["h80/signature"]).split("\n")
    ours = signature(PixioEncoder).split("\n")
    extra = "pretrained_checkpoint_path=None"
    assert extra in ours and ours.index(extra) == ours.index("gradient_checkpointing=True") + 1
    ours.remove(extra)
    assert ours == ref


@pytest.mark.parametrize("factory,width,depth,heads", [("pixio_vitb16", 768, 12, 12), ("pixio_vitl16", 1024, 24, 16), ("pixio_vith16", 1280, 32, 16),
                                                       ("pixio_vit1b16", 1536, 48, 24), ("pixio_vit5b16", 3072, 48, 32)])
def test_factories_build_the_published_sizes(factory, width, depth, heads):
    from uniception_amd.models.encoders import pixio
    with torch.device("meta"):
        m = getattr(pixio, factory)()
    assert m.enc_embed_dim == width and len(m.blocks) == depth and m.blocks[0].inner.attn.num_heads == heads
    assert m.n_cls_tokens == 8 and m.patch_size == 16 and tuple(m.pos_embed.shape) == (1, 8 + 256, width)
    assert m.blocks[0].inner.mlp.fc1.out_features == 4 * width and m.norm.eps == 1e-6


def test_registry_normalisation_and_the_refusal_to_download():
    from uniception_amd.engine import UcHipError
    from uniception_amd.models.encoders import ENCODER_CONFIGS, PixioEncoder, encoder_factory
    from uniception_amd.models.encoders.image_normalizations import IMAGE_NORMALIZATION_DICT
    assert ENCODER_CONFIGS["pixio"]["class"] is PixioEncoder and ENCODER_CONFIGS["pixio"]["supported_models"] == ["Pixio-Encoder"]
    assert "intermediate_feature_returner_class" not in ENCODER_CONFIGS["pixio"]
    n = IMAGE_NORMALIZATION_DICT["pixio"]
    assert torch.equal(n.mean, torch.tensor([0.485, 0.456, 0.406])) and torch.equal(n.std, torch.tensor([0.229, 0.224, 0.225]))
    m = encoder_factory("pixio", **kwargs("h64"))
    assert m.hf_model_name == "facebook/pixio-vith16"
    with pytest.raises(UcHipError, match="pretrained_checkpoint_path"):
        m.get_pth_file("facebook/pixio-vith16")


def test_the_position_table_is_returned_as_stored_only_at_the_square_native_grid():
    from uniception_amd.models.encoders import PixioEncoder
    m = PixioEncoder(**kwargs("h80"))
    fill(m, "h80")
    assert m._interpolate_pos_emb(torch.zeros(1, 3, 64, 64)) is m.pos_embed
    pe = m._interpolate_pos_emb(torch.zeros(1, 3, 48, 80))
    assert tuple(pe.shape) == (1, 8 + 15, 160) and torch.equal(pe[:, :8], m.pos_embed[:, :8])
    grid = m.pos_embed[:, 8:].reshape(1, 4, 4, -1).permute(0, 3, 1, 2)
    want = torch.nn.functional.interpolate(grid, size=(3, 5), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).reshape(1, 15, -1)
    assert torch.equal(pe[:, 8:], want)


def test_attention_route_at_the_wide_head_dims():
    from uniception_amd import engine
    from uniception_amd.engine import UcHipError
    bf = torch.bfloat16
    for hd in (80, 96):
        assert engine.attention_route(bf, hd, True, False, False, 264) == "wide"
        assert engine.attention_route(bf, hd, True, False, True, 263) == "wide"
        with engine.attention_precision("fp8"):
            assert engine.attention_route(bf, hd, True, False, False, 264) == "wide"
        assert engine.attention_route(torch.float32, hd, True, False, False, 264) == "unfused"
        with pytest.raises(UcHipError, match=f"qk_norm.*head_dim {hd}"):
            engine.attention_route(bf, hd, True, True, False, 264)
        with pytest.raises(UcHipError, match=f"RoPE.*head_dim {hd}"):
            engine.attention_route(bf, hd, True, False, False, 264, has_rope=True)
        with pytest.raises(UcHipError, match=f"RoPE.*head_dim {hd}"):
            engine.attention_route(bf, hd, False, False, False, 264)
    assert engine.attention_route(bf, 64, True, False, False, 264) == "vt_epilogue"
    with pytest.raises(UcHipError, match=r"bf16 attention needs head_dim 64 \(got 32\)"):
        engine.attention_route(bf, 32, True, False, False, 264)
    with pytest.raises(UcHipError, match="bf16 attention needs head_dim 64"):
        engine.attention_route(bf, 128, True, False, False, 264)
