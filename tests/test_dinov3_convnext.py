"""CPU: the host side of the DINOv3 ConvNeXt encoder — the registry, the parameter container per size, the checkpoint converter, the
fp64 formula models of the depthwise 7x7 kernel, its weight gradient and the 2x2 gather against torch.nn.functional.conv2d and its
autograd, planted defects the per-element bound must catch, the launch plan of csrc/dwconv_plan.h walked by a C++ driver, and the
provenance of the golden files."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.dinov3_convnext_formulas import (DEFECTS, WITNESS_SHAPES, dwconv7x7_model, dwconv7x7_wgrad_model, forward_bound, patch2_gather_bwd_model,
                                            patch2_gather_model, patch2_weight)
from tests.golden.dinov3_convnext_cases import (DEPTHS, DINOV3_CONVNEXT_CASES, DINOV3_CONVNEXT_GRAD_CASES, HIDDEN_SIZES, convnext_hf_config_kwargs,
                                                convnext_hf_shapes, convnext_hf_state_dict, convnext_size)
from tests.helpers import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"tiny": ((96, 192, 384, 768), (3, 3, 9, 3), 768), "small": ((96, 192, 384, 768), (3, 3, 27, 3), 768),
         "base": ((128, 256, 512, 1024), (3, 3, 27, 3), 1024), "large": ((192, 384, 768, 1536), (3, 3, 27, 3), 1536)}
# the large size's stage maps for a 512 x 512 image
LARGE_512 = [(2, 128, 128, 192), (2, 64, 64, 384), (2, 32, 32, 768), (2, 16, 16, 1536)]


def test_registry_serves_the_two_classes():
    from uniception_amd.models.encoders import (ENCODER_CONFIGS, DINOv3ConvNextEncoder, DINOv3ConvNextIntermediateFeatureReturner, encoder_factory,
                                                feature_returner_encoder_factory)
    cfg = ENCODER_CONFIGS["dinov3_convnext"]
    assert cfg == {"class": DINOv3ConvNextEncoder, "intermediate_feature_returner_class": DINOv3ConvNextIntermediateFeatureReturner,
                   "supported_models": ["DINOv3-ConvNext"]}
    enc = encoder_factory("dinov3_convnext", name="cn", dinov3_repo_dir=None, size=convnext_size())
    assert type(enc) is DINOv3ConvNextEncoder
    ret = feature_returner_encoder_factory("dinov3_convnext", name="cn", dinov3_repo_dir=None, size=convnext_size(), indices=[0, 2],
                                           norm_intermediate=False)
    assert type(ret) is DINOv3ConvNextIntermediateFeatureReturner and ret.indices == [0, 2] and ret.norm_intermediate is False


def expected_state_dict_shapes(widths, depths):
    want = {"model.downsample_layers.0.0.weight": (widths[0], 3, 4, 4), "model.downsample_layers.0.0.bias": (widths[0],),
            "model.downsample_layers.0.1.weight": (widths[0],), "model.downsample_layers.0.1.bias": (widths[0],),
            "model.norm.weight": (widths[3],), "model.norm.bias": (widths[3],)}
    for i in range(4):
        if i > 0:
            want.update({f"model.downsample_layers.{i}.0.weight": (widths[i - 1],), f"model.downsample_layers.{i}.0.bias": (widths[i - 1],),
                         f"model.downsample_layers.{i}.1.weight": (widths[i], widths[i - 1], 2, 2), f"model.downsample_layers.{i}.1.bias": (widths[i],)})
        C = widths[i]
        for j in range(depths[i]):
            p = f"model.stages.{i}.{j}."
            want.update({p + "dwconv.weight": (C, 1, 7, 7), p + "dwconv.bias": (C,), p + "norm.weight": (C,), p + "norm.bias": (C,),
                         p + "pwconv1.weight": (4 * C, C), p + "pwconv1.bias": (4 * C,), p + "pwconv2.weight": (C, 4 * C), p + "pwconv2.bias": (C,),
                         p + "gamma": (C,)})
    return want


@pytest.mark.parametrize("size", list(SIZES))
def test_constructor_attributes_and_state_dict_of_every_named_size(size):
    from uniception_amd.models.encoders import DINOv3ConvNextEncoder
    widths, depths, embed = SIZES[size]
    with torch.device("meta"):          # (no storage: the large size costs nothing)
        enc = DINOv3ConvNextEncoder(name="cn", dinov3_repo_dir="/nowhere", size=size, weights=None)
    assert enc.patch_size == 16 and enc.final_layer_patch_size == 32 and enc.enc_embed_dim == embed and enc.version == size
    assert enc.data_norm_type == "dinov3" and enc.model.patch_size == 16
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert got == expected_state_dict_shapes(widths, depths)
    layer = enc.model.stages[0][0]
    assert layer.norm.eps == 1e-6 and enc.model.norm.eps == 1e-6 and isinstance(layer.act, torch.nn.GELU) and layer.act.approximate == "none"
    assert DINOv3ConvNextEncoder(name="cn", size=convnext_size(), patch_size=32).patch_size == 32


def test_unknown_or_unserved_sizes_are_refused():
    from uniception_amd.models.encoders import DINOv3ConvNextEncoder
    from uniception_amd._lib import UcHipError
    with pytest.raises(UcHipError, match="unknown DINOv3 ConvNeXt size"):
        DINOv3ConvNextEncoder(name="cn", size="huge")
    with pytest.raises(UcHipError, match="multiples of 8"):
        DINOv3ConvNextEncoder(name="cn", size=dict(hidden_sizes=[20, 40, 80, 160], depths=[1, 1, 1, 1]))


def test_converter_round_trip_consumes_every_transformers_key(tmp_path):
    from uniception_amd.models.encoders import DINOv3ConvNextEncoder
    from uniception_amd.tools import convert_checkpoint as cc
    sd = convnext_hf_state_dict()
    src, dst = tmp_path / "hf.pth", tmp_path / "uc.pth"
    torch.save(sd, src)
    cc.main([str(src), str(dst), "--mode", "dinov3_convnext"])
    conv = torch.load(dst, weights_only=False)["model"]
    assert len(conv) == len(sd)                                   # every transformers key consumed, one to one
    enc = DINOv3ConvNextEncoder(name="cn", size=convnext_size(), pretrained_checkpoint_path=str(dst))
    assert set(conv) == set(enc.state_dict())                     # ... and none left over on either side
    for k, v in enc.state_dict().items():
        assert torch.equal(v, conv[k]), k
    assert torch.equal(conv["model.stages.2.1.dwconv.weight"], sd["model.stages.2.layers.1.depthwise_conv.weight"])
    assert torch.equal(conv["model.downsample_layers.3.1.weight"], sd["model.stages.3.downsample_layers.1.weight"])
    assert torch.equal(conv["model.norm.bias"], sd["layer_norm.bias"]) and torch.equal(conv["model.stages.0.0.gamma"], sd["model.stages.0.layers.0.gamma"])
    assert float((conv["model.stages.0.0.gamma"] - 1).abs().min()) > 1e-3          # drawn away from 1
    with pytest.raises(KeyError, match="unexpected key model.stages.0.layers.0.grn.weight"):
        cc.dinov3_convnext_hf_to_uniception({**sd, "model.stages.0.layers.0.grn.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="missing key layer_norm.weight"):
        cc.dinov3_convnext_hf_to_uniception({k: v for k, v in sd.items() if not k.startswith("layer_norm")})


def witness(shape, seed=0):
    "(x NHWC, w [C,1,7,7], b [C], dy NHWC) in fp64"
    B, H, W, C = shape
    g = torch.Generator().manual_seed(1000 * seed + B * 131 + H * 17 + W * 5 + C)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return r(B, H, W, C), r(C, 1, 7, 7), r(C), r(B, H, W, C)


def taps(w):
    return w.reshape(w.shape[0], 49).t().contiguous()


def close(a, b, what):
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
    assert err <= 1e-12, (what, err)


@pytest.mark.parametrize("shape", WITNESS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_formula_model_equals_torch_conv2d_and_its_autograd(shape):
    x, w, b, dy = witness(shape)
    xc, wc, bc = x.permute(0, 3, 1, 2).clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    ref = F.conv2d(xc, wc, bc, padding=3, groups=shape[3])
    ref.backward(dy.permute(0, 3, 1, 2))
    y, mag = dwconv7x7_model(x, taps(w), b)
    close(y, ref.detach().permute(0, 2, 3, 1), "forward")
    assert bool((mag >= y.abs() - 1e-12 * mag).all())                                  # the magnitude bounds the value
    close(dwconv7x7_model(x, taps(w), None)[0], (ref.detach() - b[None, :, None, None]).permute(0, 2, 3, 1), "no bias")
    dx, _ = dwconv7x7_model(dy, taps(w), None, flip=True)                              # the flip form IS the data gradient
    close(dx, xc.grad.permute(0, 2, 3, 1), "dx")
    dw, db, mw, mb = dwconv7x7_wgrad_model(x, dy)
    close(dw.t().reshape(-1, 1, 7, 7), wc.grad, "dw")
    close(db, bc.grad, "db")
    assert bool((mw >= dw.abs() - 1e-12 * mw).all()) and bool((mb >= db.abs() - 1e-12 * mb).all())


@pytest.mark.parametrize("shape", [(2, 4, 6, 8), (1, 3, 5, 16), (2, 5, 4, 8), (1, 1, 2, 8), (1, 2, 1, 8)], ids=lambda s: "x".join(map(str, s)))
def test_gather_model_equals_conv2d_k2_s2_odd_maps_included(shape):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    w, b = torch.randn(24, C, 2, 2, generator=g, dtype=torch.float64), torch.randn(24, generator=g, dtype=torch.float64)
    xc = x.permute(0, 3, 1, 2).clone().requires_grad_()
    if H < 2 or W < 2:                  # Conv2d refuses a map smaller than its kernel; the gather hands out no rows
        assert patch2_gather_model(x).shape == (0, 4 * C)
        assert not patch2_gather_bwd_model(torch.zeros(0, 4 * C, dtype=torch.float64), B, H, W).any()
        return
    ref = F.conv2d(xc, w, b, stride=2)
    rows = patch2_gather_model(x)
    assert rows.shape == (B * (H // 2) * (W // 2), 4 * C)
    got = (rows @ patch2_weight(w).t() + b).reshape(B, H // 2, W // 2, 24)
    close(got, ref.detach().permute(0, 2, 3, 1), "conv k2 s2")
    dy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(dy)
    drows = dy.permute(0, 2, 3, 1).reshape(-1, 24) @ patch2_weight(w)
    dx = patch2_gather_bwd_model(drows, B, H, W)
    close(dx, xc.grad.permute(0, 2, 3, 1), "dx")
    assert not dx[:, 2 * (H // 2):].any() and not dx[:, :, 2 * (W // 2):].any()      # the unread odd row / column: zero gradient
    assert torch.equal(patch2_gather_model(dx), drows)                                # a permutation: the adjoint inverts it on its range


# which witness shape can show which planted defect (the others compute the same function there):
#   the one-pixel map reads only the centre tap (3, 3), which a transposition and a row-only flip leave in place (24 = 48 - 24)
CATCHES = {
    "tap_order_transposed": [s for s in WITNESS_SHAPES if s != (1, 1, 1, 8)],
    "padding_2": list(WITNESS_SHAPES),
    "bias_dropped": list(WITNESS_SHAPES),
    "flip_rows_only": [s for s in WITNESS_SHAPES if s != (1, 1, 1, 8)],
    "right_halo_not_zeroed": list(WITNESS_SHAPES),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_exceed_the_per_element_bound(defect):
    assert set(CATCHES) == set(DEFECTS)
    flip = defect == "flip_rows_only"
    for shape in WITNESS_SHAPES:
        x, w, b, _ = witness(shape, seed=3)
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            xs = x.to(dtype).double()                                     # what a kernel of that storage type reads
            ref, mag = dwconv7x7_model(xs, taps(w).float().double(), b.float().double(), flip=flip)
            bad, _ = dwconv7x7_model(xs, taps(w).float().double(), b.float().double(), flip=flip, defect=defect)
            worst = float(((bad - ref).abs() / forward_bound(ref, mag, dtype)).max())
            if shape in CATCHES[defect]:
                assert worst > 1.0, (defect, shape, dtype, worst)
            else:
                assert torch.equal(bad, ref), (defect, shape)             # this shape cannot show it: the same function


def build_driver(tmpdir):
    "Compile tests/dwconv_plan_driver.cpp with the system C++ compiler into tmpdir; returns run(launches) -> output lines."
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/dwconv_plan_driver.cpp"
    exe = os.path.join(str(tmpdir), "dwconv_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "uniception_amd", "csrc"),
                           os.path.join(ROOT, "tests", "dwconv_plan_driver.cpp"), "-o", exe])

    def run(launches):
        text = "".join(" ".join(f"{k}={v}" for k, v in l.items()) + "\n" for l in launches)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(launches)
        return out
    return run


FWD_FIELDS = ("tile_h tile_w c8 pix_stride chunks tiles_y tiles_x items threads lds_in_bytes lds_w_bytes lds_bytes grid cover_min cover_max "
              "lds_ok").split()
WGRAD_FIELDS = ("tile_h tile_w c8 pix_stride chunks tiles_y tiles_x row_groups threads lds_x_bytes lds_dy_bytes lds_red_bytes lds_bytes units "
                "partials merge_depth ws_bytes cover_min cover_max lds_ok ws_ok").split()
LDS_BUDGET = 65536


def test_plan_covers_every_output_once_within_its_lds_budget_and_workspace(tmp_path):
    run = build_driver(tmp_path)
    shapes = WITNESS_SHAPES + LARGE_512 + [(1, 1, 2, 256), (1, 3, 5, 192)]           # (+ the golden cases' smallest maps)
    launches = [dict(op=op, dtype=dt, B=B, H=H, W=W, C=C) for (B, H, W, C) in shapes for dt in (0, 1, 2) for op in ("fwd", "wgrad")]
    seen_threads = set()
    for l, line in zip(launches, run(launches)):
        tok = line.split()
        assert tok[0] == l["op"]
        p = dict(zip(FWD_FIELDS if l["op"] == "fwd" else WGRAD_FIELDS, map(int, tok[1:])))
        assert len(tok) - 1 == len(p)
        B, H, W, C, vb = l["B"], l["H"], l["W"], l["C"], 32 if l["dtype"] == 0 else 16
        assert p["cover_min"] == 1 and p["cover_max"] == 1, (l, p)                       # every output exactly once
        assert p["lds_ok"] == 1 and p["lds_bytes"] <= LDS_BUDGET, (l, p)
        assert 1 <= p["tile_h"] <= min(H, 16) and p["tile_w"] % 4 == 0 and p["tile_w"] <= 16 and p["pix_stride"] == p["c8"] | 1
        assert p["tiles_y"] == -(-H // p["tile_h"]) and p["tiles_x"] == -(-W // p["tile_w"]) and p["chunks"] == -(-(C // 8) // p["c8"])
        assert p["threads"] % 64 == 0 and p["threads"] <= 256
        if l["op"] == "fwd":
            assert p["grid"] == B * p["chunks"] * p["tiles_y"] * p["tiles_x"] and p["items"] == p["c8"] * p["tile_h"] * p["tile_w"] // 4 <= p["threads"]
            assert p["lds_in_bytes"] == (p["tile_h"] + 6) * (p["tile_w"] + 6) * p["pix_stride"] * vb and p["lds_w_bytes"] == 49 * p["c8"] * 32
            seen_threads.add(p["threads"])
        else:
            assert p["ws_ok"] == 1 and p["units"] == B * p["tiles_y"] * p["tiles_x"] and 1 <= p["partials"] <= p["units"]
            assert p["ws_bytes"] == p["partials"] * 50 * C * 4 and p["merge_depth"] == p["row_groups"] - 1 + p["partials"] - 1
            assert 7 * p["c8"] * p["row_groups"] <= p["threads"]
    assert {64, 192, 256} <= seen_threads
    # the workspace the entry point reports is the plan's, whatever the dtype (one query serves all three)
    from uniception_amd import _lib
    lib = _lib.load()
    for l, line in zip(launches, run(launches)):
        if l["op"] == "wgrad":
            ws = int(line.split()[1 + WGRAD_FIELDS.index("ws_bytes")])
            assert lib.uc_dwconv7x7_nhwc_wgrad_ws_bytes(l["B"], l["H"], l["W"], l["C"]) == ws, l
    assert lib.uc_dwconv7x7_nhwc_wgrad_ws_bytes(1, 4, 4, 12) == 0                        # (a shape the entry point refuses)


def test_bad_arguments_are_refused_on_the_host():
    """uc_dwconv7x7_nhwc and its companions validate before they launch: decided entirely on the host, so skipped where a GPU is visible
    (a wrongly accepted call would launch on these pointers; tests/test_dinov3_convnext_gpu.py repeats it on real buffers)."""
    from uniception_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present: a wrongly accepted call would launch on invalid pointers")
    lib = _lib.load()
    P = 4096
    calls = {
        "uc_dwconv7x7_nhwc": [((P, P, P, 2 * P, 1, 1, 4, 4, 12, 0, None), "multiple of 8"), ((P + 4, P, P, 2 * P, 1, 1, 4, 4, 16, 0, None), "16-byte aligned"),
                              ((P, P, P, P, 1, 1, 4, 4, 16, 0, None), "y == x"), ((P, P, P, 2 * P, 3, 1, 4, 4, 16, 0, None), "unsupported dtype 3 "),
                              ((P, None, P, 2 * P, 1, 1, 4, 4, 16, 0, None), "null pointer")],
        "uc_dwconv7x7_nhwc_wgrad": [((P, P, P, P, P, 1, 1, 4, 4, 12, None), "multiple of 8"), ((P, P + 8, P, P, P, 1, 1, 4, 4, 16, None), "16-byte aligned"),
                                    ((P, P, P, P, None, 1, 1, 4, 4, 16, None), "null pointer"), ((P, P, P, P, P, -1, 1, 4, 4, 16, None), "unsupported dtype -1 ")],
        "uc_patch2_gather_nhwc": [((P, P, 1, 1, 4, 4, 12, None), "multiple of 8"), ((P, P + 2, 1, 1, 4, 4, 16, None), "16-byte aligned"),
                                  ((P, P, 7, 1, 4, 4, 16, None), "unsupported dtype 7 ")],
        "uc_patch2_gather_nhwc_bwd": [((P, P, 1, 1, 4, 4, 12, None), "multiple of 8"), ((P + 2, P, 1, 1, 4, 4, 16, None), "16-byte aligned"),
                                      ((P, P, 7, 1, 4, 4, 16, None), "unsupported dtype 7 ")],
    }
    for name, rows in calls.items():
        for args, text in rows:
            assert len(args) == len(_lib.SIGNATURES[name])
            status = getattr(lib, name)(*args)
            msg = lib.uc_last_error().decode()
            assert status == -1 and msg.startswith(name + ":") and text in msg, (name, args, status, msg)
    empty = {"uc_dwconv7x7_nhwc": (P, P, P, 2 * P, 1, 0, 4, 4, 16, 0, None), "uc_dwconv7x7_nhwc_wgrad": (P, P, P, P, P, 1, 0, 4, 4, 16, None),
             "uc_patch2_gather_nhwc": (P, P, 1, 0, 4, 4, 16, None), "uc_patch2_gather_nhwc_bwd": (P, P, 1, 0, 4, 4, 16, None)}
    for name, args in empty.items():                    # B == 0: UC_OK, nothing launched
        assert getattr(lib, name)(*args) == 0, (name, lib.uc_last_error())


def test_golden_files_are_what_the_generator_writes_today():
    transformers = pytest.importorskip("transformers")
    pytest.importorskip("transformers.models.dinov3_convnext")
    from tests.golden import make_golden_dinov3_convnext_hf as gen
    gold = np.load(os.path.join(GOLDEN_DIR, "dinov3_convnext_hf.npz"))
    stage0 = np.load(os.path.join(GOLDEN_DIR, "dinov3_convnext_hf_stage0.npz"))
    assert str(gold["transformers_version"]) == transformers.__version__
    assert sorted(list(gold.files) + list(stage0.files)) == gen.golden_keys()
    assert sorted(stage0.files) == sorted(f"{n}/stage0_raw" for n in DINOV3_CONVNEXT_CASES)
    # the configuration the generator builds has exactly the keys and shapes the cases file states
    from transformers.models.dinov3_convnext import DINOv3ConvNextConfig, DINOv3ConvNextModel
    with torch.device("meta"):
        model = DINOv3ConvNextModel(DINOv3ConvNextConfig(**convnext_hf_config_kwargs()))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == convnext_hf_shapes()
    for name, c in DINOV3_CONVNEXT_CASES.items():
        H, W = c["hw"]
        assert gold[f"{name}/features"].shape == (c["B"], HIDDEN_SIZES[3], H // 32, W // 32) == gold[f"{name}/stage3_norm"].shape
        assert np.array_equal(gold[f"{name}/features"], gold[f"{name}/stage3_norm"])
        for i in range(4):
            m = stage0[f"{name}/stage0_raw"] if i == 0 else gold[f"{name}/stage{i}_raw"]
            assert m.shape == (c["B"], HIDDEN_SIZES[i], H // (4 << i), W // (4 << i))
    n_params = len(convnext_hf_shapes())
    assert n_params == 6 + 4 * 3 + 9 * sum(DEPTHS)
    for name in DINOV3_CONVNEXT_GRAD_CASES:
        assert sum(1 for f in gold.files if f.startswith(f"{name}/grad/") and f.endswith("__samples")) == n_params
