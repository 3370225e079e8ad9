"""CPU: the oracle restatement against the committed golden vectors (generated from the real reference by
tests/golden/make_golden.py).  Weights come from the name-keyed filler applied to the state_dict of the
uniception_amd modules, so this also proves their state_dict keys/shapes equal the reference's — any missing
or renamed parameter would change the weights and break parity."""
import os

import pytest
import torch

from oracle import dust3r_oracle as O
from tests.golden.cases import CASES
from tests.helpers import build_case_model, case_images, compare_to_golden, load_golden


@pytest.mark.parametrize("name", list(CASES.keys()))
def test_oracle_matches_reference_golden(name):
    torch.set_num_threads(max(1, torch.get_num_threads()))
    model, c = build_case_model(name)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    img1, img2 = case_images(c)
    collect = {}
    with torch.no_grad():
        o1, o2 = O.dust3r_forward(sd, img1, img2, head=c["head"], enc_depth=c["enc_depth"], enc_heads=c["enc_heads"],
                                  dec_depth=c["dec_depth"], dec_heads=c["dec_heads"], patch_size=c["patch"],
                                  indices=tuple(c["indices"]), collect=collect)
    tensors = dict(collect)
    tensors.update(pts3d_1=o1["pts3d"], conf_1=o1["conf"], pts3d_2=o2["pts3d_in_other_view"], conf_2=o2["conf"])
    worst = compare_to_golden(load_golden(name), tensors, c, tol=2e-5)
    print(f"{name}: worst {worst}")


def test_filler_is_name_keyed_and_deterministic():
    a = O.filler_tensor("encoder.enc_blocks.0.attn.qkv.weight", (6, 4))
    b = O.filler_tensor("encoder.enc_blocks.0.attn.qkv.weight", (6, 4))
    c = O.filler_tensor("encoder.enc_blocks.1.attn.qkv.weight", (6, 4))
    assert torch.equal(a, b) and not torch.equal(a, c)
    n = O.filler_tensor("encoder.enc_norm.weight", (1000,))
    assert abs(float(n.mean()) - 1.0) < 0.02  # LayerNorm gains are centred on 1


def test_rope_roundtrip_and_quarters():
    """fwd then inverse rotation is the identity; position 0 leaves tokens unchanged (curope2d.py:24-28)."""
    g = torch.Generator().manual_seed(0)
    t = torch.randn(2, 3, 6, 64, generator=g)
    pos = O.grid_positions(2, 2, 3)
    r = O.rope2d(t, pos, 100.0, 1.0)
    back = O.rope2d(r, pos, 100.0, -1.0)
    assert (back - t).abs().max() < 1e-5
    assert torch.equal(r[:, :, 0], t[:, :, 0])  # token (0,0)
    # the x-half is untouched for tokens in column 0, the y-half for tokens in row 0
    assert torch.equal(r[:, :, 3, 32:], t[:, :, 3, 32:]) and torch.equal(r[:, :, 1, :32], t[:, :, 1, :32])


@pytest.mark.parametrize("name", ["small_noreg", "small_reg", "base_reg", "large_full", "small_reg_224", "base_reg_448x336", "small_reg_700x560",
                                  "giant_reg_224", "giant_noreg"])      # giant_*: ViT-g/14's SwiGLU FFN
def test_oracle_dinov2_matches_huggingface_transformers(name):
    """The oracle's restatement of the DINOv2 ViT (cls token, registers inserted after the position embedding, LayerScale, erf-GELU,
    final LayerNorm) against an independent implementation of the same published network: transformers' Dinov2Model /
    Dinov2WithRegistersModel (tests/golden/make_golden_dinov2_hf.py).  The hub code the reference loads is not available here."""
    import os

    import numpy as np

    from tests.golden.cases import sample_indices
    from tests.golden.dinov2_cases import DINOV2_HF_CASES, SIZES, dinov2_hub_state_dict, dinov2_image
    from tests.helpers import GOLDEN_DIR, rel_l2
    gold = np.load(os.path.join(GOLDEN_DIR, "dinov2_hf.npz"))
    c = DINOV2_HF_CASES[name]
    with torch.no_grad():
        feats, regs = O.dinov2_encoder(dinov2_image(c), dinov2_hub_state_dict(c), "model.", num_heads=SIZES[c["size"]][1],
                                       num_registers=4 if c["regs"] else 0)
    assert tuple(feats.shape) == tuple(gold[f"{name}/features__shape"])
    idx = sample_indices(feats.numel())
    e_f = rel_l2(feats.flatten()[idx], gold[f"{name}/features__samples"])
    e_n = abs(float(feats.double().norm()) - float(gold[f"{name}/features__norm"])) / float(gold[f"{name}/features__norm"])
    e_r = rel_l2(regs, gold[f"{name}/registers"])
    print(f"\n[oracle vs transformers {gold['transformers_version']}] {name}: features {e_f:.2e} (norm {e_n:.1e}), cls/registers {e_r:.2e}")
    assert e_f < 2e-5 and e_n < 2e-5 and e_r < 2e-5


def test_oracle_attention_options_match_reference_golden():
    """qk_norm=True and value tokens that are not the key tokens (utils/transformer_blocks.py:196-197, 229, 341-348): the oracle's
    self_attention / cross_attention against outputs of the reference's Attention / CrossAttention (tests/golden/attn_opts.npz,
    make_golden_attn_opts.py)."""
    import numpy as np
    from tests.golden.attn_opts_cases import CASES as ACASES, make_inputs
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "attn_opts.npz"))
    for name, c in ACASES.items():
        sd = {"l." + k[len(name) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "/sd/")}
        ins = make_inputs(c)
        if c["kind"] == "self":
            out = O.self_attention(ins["x"], ins["xpos"] if c["rope"] else None, sd, "l", c["heads"], 100.0)
        else:
            out = O.cross_attention(ins["q"], ins["k"], ins["qpos"] if c["rope"] else None, ins["kpos"] if c["rope"] else None, sd, "l",
                                    c["heads"], 100.0, value=ins["v"] if c["sep_v"] else None)
        ref = torch.from_numpy(z[name + "/out"])
        err = float((out - ref).norm() / ref.norm())
        assert err < 2e-5, (name, err)


def test_oracle_q_scalings_match_reference_golden():
    """`use_scalable_softmax` / `use_entropy_scaling` (utils/transformer_blocks.py:231-241, 360-370) and `latent_attn_dim` (:178-199): the
    oracle's q_scaling / self_attention against outputs of the reference's Attention / CrossAttention with those options
    (tests/golden/attn_scale_opts.npz, make_golden_attn_scale.py)."""
    import numpy as np
    from tests.golden.attn_opts_cases import SCALE_CASES, make_inputs
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "attn_scale_opts.npz"))
    for name, c in SCALE_CASES.items():
        sd = {"l." + k[len(name) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "/sd/")}
        ins = make_inputs(c)
        qs = O.q_scaling(c["gh"] * c["gw"], c["scalable"], c["entropy"])
        if c["kind"] == "self":
            out = O.self_attention(ins["x"], ins["xpos"] if c["rope"] else None, sd, "l", c["heads"], 100.0, q_scale=qs)
        else:
            out = O.cross_attention(ins["q"], ins["k"], ins["qpos"] if c["rope"] else None, ins["kpos"] if c["rope"] else None, sd, "l",
                                    c["heads"], 100.0, q_scale=qs)
        ref = torch.from_numpy(z[name + "/out"])
        err = float((out - ref).norm() / ref.norm())
        assert err < 2e-5, (name, err)


def test_oracle_rope_matches_the_references_own_compiled_cpu_loop():
    """oracle/_ref/curope_ref.so = the reference's curope.cpp compiled from where it lies (oracle/build_ref.py): its `rope_2d` on CPU
    tensors runs `rope_2d_cpu` (curope.cpp:11-46), the loop the CUDA kernel mirrors.  The oracle's rope2d — and through it every
    golden fixture that involves RoPE — against it: forward and the inverse rotation (fwd = -1), 32- and 64-wide heads.  Its outputs
    are stored in tests/golden/curope_ref.npz (make_golden_curope.py); where the shared object is built, it is run live as well."""
    from oracle import build_ref
    from tests.golden import curope_cases
    build_ref.build(verbose=False)
    ref = build_ref.load()
    for key, t, pos, stored in curope_cases.load("oracle"):
        for fwd in (1.0, -1.0):
            want = stored[fwd]
            if ref is not None:
                live = t.clone()
                ref.rope_2d(live, pos, 100.0, fwd)                 # in place, [B, N, H, D]
                assert float((live - want).abs().max()) < 1e-6, (key, fwd)
            got = O.rope2d(t.transpose(1, 2), pos, 100.0, fwd).transpose(1, 2)
            assert float((got - want).abs().max()) < 2e-5, (key, fwd)
    back = O.rope2d(want.transpose(1, 2), pos, 100.0, 1.0).transpose(1, 2)   # the inverse of the inverse
    if ref is not None:
        back_ref = want.clone()
        ref.rope_2d(back_ref, pos, 100.0, 1.0)
        assert float((back_ref - t).abs().max()) < 2e-5
    assert float((back - t).abs().max()) < 2e-5


def test_fullsize_oracle_fixture_equals_the_reference_at_1024():
    """tests/golden/fullsize.npz (oracle outputs of config 5 at 1024 x 1024 on every 16th pixel) against fullsize_ref.npz — the REAL
    reference's factory model run at that size by make_golden_fullsize_ref.py: data replay, < 2e-5 (observed 6.5e-7)."""
    import numpy as np
    d = os.path.join(os.path.dirname(__file__), "golden")
    a, b = np.load(os.path.join(d, "fullsize.npz")), np.load(os.path.join(d, "fullsize_ref.npz"))
    for k in ("pts3d_1", "conf_1", "pts3d_2", "conf_2"):
        o, r = torch.from_numpy(a["c5_" + k]), torch.from_numpy(b["c5ref_" + k])
        assert o.shape == r.shape and float((o - r).norm() / r.norm()) < 2e-5, k


def test_factory_fixture_intermediates_were_confirmed_by_the_reference():
    """tests/golden/factory_intermediates_ref.json (make_golden_factory_intermediates.py): the intermediates stored in the two factory
    fixtures — encoder features, decoder finals / takes, DPT feature maps, decoded channels — against forward hooks on the REAL
    reference's own sub-modules: every entry below 2e-5 (observed <= 8.6e-7), every stored intermediate covered."""
    import json
    import numpy as np
    d = os.path.join(os.path.dirname(__file__), "golden")
    rep = json.load(open(os.path.join(d, "factory_intermediates_ref.json")))["cases"]
    assert set(rep) == {"vitl_linear_224", "vitl_dpt_512"}
    for name, entries in rep.items():
        z = np.load(os.path.join(d, name + ".npz"))
        stored = {k.rsplit("__", 1)[0] for k in z.files if k.endswith("__samples")} - {"pts3d_1", "conf_1", "pts3d_2", "conf_2"}
        assert stored == set(entries), (name, stored ^ set(entries))
        for k, e in entries.items():
            assert e["samples_rel_l2"] < 2e-5 and e["norm_rel_diff"] < 2e-5, (name, k, e)
