"""DINOv3 ConvNeXt on the HIP kernels.  Kernels (csrc/dwconv.hip): uc_dwconv7x7_nhwc, uc_dwconv7x7_nhwc_wgrad, uc_patch2_gather_nhwc and
its adjoint, every element against the fp64 models of tests/dinov3_convnext_formulas.py, which read the same stored inputs — nothing is
sampled.  The bounds are derived there, not measured: forward gamma_50 (|b| + sum |w x|) plus half an ulp of the storage format taken
at |reference| + the arithmetic bound; weight gradient gamma_n sum |dy x| with n = B H W + the merge depth of the launch plan.
Model: the encoder and the intermediate-feature returner against goldens of an INDEPENDENT implementation of the published network
(transformers' DINOv3ConvNextModel: tests/golden/dinov3_convnext_hf.npz, make_golden_dinov3_convnext_hf.py) — outputs in fp32 and bf16
mode and parameter gradients against transformers' autograd, under the tolerances of the DINOv3 ViT tests.  The golden weights are
loaded through uniception_amd.tools.convert_checkpoint (--mode dinov3_convnext).  PARITY UNPINNED against the hub code."""
import os

import numpy as np
import pytest
import torch

from tests.dinov3_convnext_formulas import (WITNESS_SHAPES, dwconv7x7_model, dwconv7x7_wgrad_model, forward_bound, gamma, patch2_gather_bwd_model,
                                            patch2_gather_model)
from tests.golden.cases import sample_indices
from tests.golden.dinov3_convnext_cases import (DINOV3_CONVNEXT_CASES, DINOV3_CONVNEXT_GRAD_CASES, HIDDEN_SIZES, convnext_grad_weights,
                                                convnext_hf_state_dict, convnext_image, convnext_size)
from tests.helpers import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GUARD = 64          # guard elements in front of and behind y (a multiple of 8: y stays 16-byte aligned)
IDS = lambda s: "x".join(map(str, s))


def operands(shape, dtype, gpu, seed=0):
    "(x, dy in `dtype`; w49 fp32 [49, C]; bias fp32 [C]) on the GPU"
    B, H, W, C = shape
    g = torch.Generator().manual_seed(7000 + 100 * seed + B * 131 + H * 17 + W * 5 + C)
    x, dy = torch.randn(B, H, W, C, generator=g).to(dtype).to(gpu), torch.randn(B, H, W, C, generator=g).to(dtype).to(gpu)
    w = torch.randn(C, 1, 7, 7, generator=g)
    return x, dy, w.reshape(C, 49).t().contiguous().to(gpu), torch.randn(C, generator=g).to(gpu)


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("flip", [0, 1], ids=["fwd", "flip"])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", WITNESS_SHAPES, ids=IDS)
def test_dwconv7x7_per_element_against_fp64_and_writes_nothing_outside_y(gpu, shape, dt, flip, bias):
    from uniception_amd import _lib, ops
    dtype = DTYPES[dt]
    B, H, W, C = shape
    x, _, w49, b = operands(shape, dtype, gpu)
    n = x.numel()
    buf = torch.full((GUARD + n + GUARD,), 77.0, dtype=dtype, device=gpu)
    y = buf[GUARD:GUARD + n].view(B, H, W, C)
    assert y.data_ptr() % 16 == 0
    _lib.check(_lib.load().uc_dwconv7x7_nhwc(x.data_ptr(), w49.data_ptr(), b.data_ptr() if bias else None, y.data_ptr(), ops._dt(dtype),
                                             B, H, W, C, flip, stream()), "uc_dwconv7x7_nhwc")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 77.0).all()) and bool((buf[GUARD + n:] == 77.0).all()), "wrote outside y"
    ref, mag = dwconv7x7_model(x.double(), w49.double(), b.double() if bias else None, flip=bool(flip))
    bound = forward_bound(ref, mag, dtype)
    err = (y.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"\n[uc_dwconv7x7_nhwc {shape} {dt} flip={flip} bias={bias}] max error / bound {worst:.3f}, max abs error {float(err.max()):.3e}")
    assert bool((err <= bound).all()), worst
    assert torch.equal(ops.dwconv7x7_nhwc(x, w49, b if bias else None, flip=bool(flip)), y)          # the wrapper: the same launch, the same bits


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", WITNESS_SHAPES, ids=IDS)
def test_dwconv7x7_wgrad_per_element_against_fp64_and_is_reproducible(gpu, shape, dt):
    from uniception_amd import _lib, ops
    dtype = DTYPES[dt]
    B, H, W, C = shape
    x, dy, _, _ = operands(shape, dtype, gpu, seed=1)
    dw, db = ops.dwconv7x7_nhwc_wgrad(x, dy)
    dw2, db2 = ops.dwconv7x7_nhwc_wgrad(x, dy)
    torch.cuda.synchronize()
    assert dw.shape == (49, C) and db.shape == (C,) and dw.dtype == db.dtype == torch.float32
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two runs differ"
    # merge depth of the launch plan (csrc/dwconv_plan.h): the row groups of a workgroup, then the partials of the workspace
    partials = _lib.load().uc_dwconv7x7_nhwc_wgrad_ws_bytes(B, H, W, C) // (50 * C * 4)
    assert partials >= 1
    n = B * H * W + (min(H, 8) - 1) + (partials - 1)
    rw, rb, mw, mb = dwconv7x7_wgrad_model(x.double(), dy.double())
    ew, eb = (dw.double() - rw).abs(), (db.double() - rb).abs()
    worst = max(float((ew / (gamma(n) * mw).clamp_min(1e-300)).max()), float((eb / (gamma(n) * mb).clamp_min(1e-300)).max()))
    print(f"\n[uc_dwconv7x7_nhwc_wgrad {shape} {dt}] n = {n}, max error / bound {worst:.3f}")
    assert bool((ew <= gamma(n) * mw).all()) and bool((eb <= gamma(n) * mb).all()), worst
    assert ops.dwconv7x7_nhwc_wgrad(x, dy, bias=False)[1] is None


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", [(2, 4, 6, 8), (1, 3, 5, 16), (2, 5, 4, 24), (1, 1, 2, 8), (2, 33, 18, 40)], ids=IDS)
def test_patch2_gather_and_its_adjoint_are_exact_permutations(gpu, shape, dt):
    from uniception_amd import ops
    B, H, W, C = shape
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randn(B, H, W, C, generator=g).to(DTYPES[dt]).to(gpu)
    rows = ops.patch2_gather_nhwc(x)
    assert torch.equal(rows, patch2_gather_model(x))
    d = torch.randn(rows.shape, generator=g).to(DTYPES[dt]).to(gpu)
    dx = ops.patch2_gather_nhwc_bwd(d, B, H, W)
    torch.cuda.synchronize()
    assert torch.equal(dx, patch2_gather_bwd_model(d, B, H, W))
    assert not dx[:, 2 * (H // 2):].any() and not dx[:, :, 2 * (W // 2):].any()          # the unread odd row / column: zero gradient


def test_empty_problems_launch_nothing(gpu):
    from uniception_amd import ops
    e = torch.empty(0, 5, 9, 24, device=gpu)
    w = torch.zeros(49, 24, device=gpu)
    assert ops.dwconv7x7_nhwc(e, w, None).shape == e.shape and ops.patch2_gather_nhwc(e).shape == (0, 96)
    assert ops.patch2_gather_nhwc_bwd(torch.empty(0, 96, device=gpu), 0, 5, 9).shape == e.shape
    torch.cuda.synchronize()


def test_bad_arguments_are_refused_before_any_launch(gpu):
    from uniception_amd import _lib, ops
    lib = _lib.load()
    x, dy, w49, b = operands((2, 5, 9, 24), torch.float32, gpu)
    y = torch.full_like(x, 77.0)
    dw, db, ws = torch.full((49, 24), 77.0, device=gpu), torch.full((24,), 77.0, device=gpu), torch.full((50 * 24 * 4,), 77.0, device=gpu)
    F32 = _lib.UC_F32

    def fwd(x_=x.data_ptr(), w_=w49.data_ptr(), y_=y.data_ptr(), dtype=F32, C=24):
        return lib.uc_dwconv7x7_nhwc(x_, w_, b.data_ptr(), y_, dtype, 2, 5, 9, C, 0, stream())

    def wgrad(x_=x.data_ptr(), ws_=ws.data_ptr(), dtype=F32, C=24):
        return lib.uc_dwconv7x7_nhwc_wgrad(x_, dy.data_ptr(), dw.data_ptr(), db.data_ptr(), ws_, dtype, 2, 5, 9, C, stream())

    def gather(fn, a=x.data_ptr(), dtype=F32, C=24):
        return getattr(lib, fn)(a, y.data_ptr(), dtype, 2, 5, 9, C, stream())

    cases = [("uc_dwconv7x7_nhwc", lambda: fwd(C=12), "multiple of 8"), ("uc_dwconv7x7_nhwc", lambda: fwd(x_=x.data_ptr() + 4), "16-byte aligned"),
             ("uc_dwconv7x7_nhwc", lambda: fwd(y_=x.data_ptr()), "y == x"), ("uc_dwconv7x7_nhwc", lambda: fwd(dtype=3), "unsupported dtype 3 "),
             ("uc_dwconv7x7_nhwc", lambda: fwd(w_=w49.data_ptr() + 8), "16-byte aligned"),
             ("uc_dwconv7x7_nhwc_wgrad", lambda: wgrad(C=20), "multiple of 8"), ("uc_dwconv7x7_nhwc_wgrad", lambda: wgrad(x_=x.data_ptr() + 4), "16-byte aligned"),
             ("uc_dwconv7x7_nhwc_wgrad", lambda: wgrad(dtype=-1), "unsupported dtype -1 "), ("uc_dwconv7x7_nhwc_wgrad", lambda: wgrad(ws_=None), "null pointer"),
             ("uc_patch2_gather_nhwc", lambda: gather("uc_patch2_gather_nhwc", C=12), "multiple of 8"),
             ("uc_patch2_gather_nhwc", lambda: gather("uc_patch2_gather_nhwc", a=x.data_ptr() + 4), "16-byte aligned"),
             ("uc_patch2_gather_nhwc", lambda: gather("uc_patch2_gather_nhwc", dtype=5), "unsupported dtype 5 "),
             ("uc_patch2_gather_nhwc_bwd", lambda: gather("uc_patch2_gather_nhwc_bwd", C=12), "multiple of 8"),
             ("uc_patch2_gather_nhwc_bwd", lambda: gather("uc_patch2_gather_nhwc_bwd", a=x.data_ptr() + 4), "16-byte aligned"),
             ("uc_patch2_gather_nhwc_bwd", lambda: gather("uc_patch2_gather_nhwc_bwd", dtype=5), "unsupported dtype 5 ")]
    for name, call, text in cases:
        assert call() == -1, (name, text)
        msg = lib.uc_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, (name, text, msg)
    # a too-small workspace: the C entry point is not told its size, the wrapper is — refused there, by the function's name
    need = lib.uc_dwconv7x7_nhwc_wgrad_ws_bytes(2, 5, 9, 24)
    assert need > 0 and need % 16 == 0
    with pytest.raises(ops.UcHipError, match=rf"uc_dwconv7x7_nhwc_wgrad: the workspace holds {need - 4} bytes .* needs {need} bytes"):
        ops.dwconv7x7_nhwc_wgrad(x, dy, ws=torch.full((need // 4 - 1,), 77.0, device=gpu))
    with pytest.raises(ops.UcHipError, match="uc_dwconv7x7_nhwc failed"):
        ops.dwconv7x7_nhwc(x[..., :12].contiguous(), w49[:, :12].contiguous(), None)
    torch.cuda.synchronize()
    for t in (y, dw, db, ws):
        assert bool((t == 77.0).all())                 # nothing ran
    assert fwd() == 0 and wgrad(ws_=torch.empty(need // 4, device=gpu).data_ptr()) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# the encoder against transformers' DINOv3ConvNextModel
# ---------------------------------------------------------------------------------------------------------------------------------
# Tolerances: the project's own, from the DINOv3 ViT tests (tests/test_dinov3_gpu.py): fp32 1e-3, bf16 3e-2 rel-L2 on outputs; gradients
# fp32 rel-L2 < 1e-3 per parameter on samples and norm and the loss within 1e-4, bf16 cosine over all sampled gradients > 0.999.
MODES = [("fp32", 1e-3), ("bf16", 3e-2)]


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN_DIR, "dinov3_convnext_hf.npz")))
    g.update(np.load(os.path.join(GOLDEN_DIR, "dinov3_convnext_hf_stage0.npz")))
    return g


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    "the {'model': ...} file the converter writes from the transformers-named golden weights (one set of weights for every case)"
    from uniception_amd.tools import convert_checkpoint as cc
    d = tmp_path_factory.mktemp("dinov3_convnext")
    src, dst = d / "hf.pth", d / "uc.pth"
    torch.save(convnext_hf_state_dict(), src)
    cc.main([str(src), str(dst), "--mode", "dinov3_convnext"])
    return str(dst)


def build(checkpoint, returner=False, **kw):
    from uniception_amd.models.encoders import encoder_factory, feature_returner_encoder_factory
    make = feature_returner_encoder_factory if returner else encoder_factory
    return make("dinov3_convnext", name="cn", dinov3_repo_dir=None, size=convnext_size(), pretrained_checkpoint_path=checkpoint, **kw)


def run(enc, name, gpu):
    from uniception_amd.models.encoders.base import ViTEncoderInput
    return enc(ViTEncoderInput(image=convnext_image(DINOV3_CONVNEXT_CASES[name]).to(gpu), data_norm_type="dinov3"))


@pytest.mark.parametrize("name", list(DINOV3_CONVNEXT_CASES))
@pytest.mark.parametrize("mode,tol", MODES)
def test_encoder_matches_huggingface_transformers_golden(gpu, gold, checkpoint, name, mode, tol):
    from uniception_amd import engine
    enc = build(checkpoint).eval().to(gpu)
    with torch.no_grad(), engine.precision(mode):
        out = run(enc, name, gpu)
    want = gold[f"{name}/features"]
    assert tuple(out.features.shape) == want.shape and out.features.dtype == torch.float32 and out.features.is_contiguous()
    e = rel_l2(out.features.cpu(), want)
    print(f"\n[dinov3_convnext {mode} vs transformers {gold['transformers_version']}] {name}: features {e:.2e}")
    assert e < tol


@pytest.mark.parametrize("name", ["96x64", "48x80"])
@pytest.mark.parametrize("mode,tol", MODES)
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("indices", [1, 4, [0, 2], None], ids=["last1", "last4", "list02", "all"])
def test_returner_matches_huggingface_transformers_golden(gpu, gold, checkpoint, name, mode, tol, indices, norm):
    from uniception_amd import engine
    enc = build(checkpoint, returner=True, indices=indices, norm_intermediate=norm).eval().to(gpu)
    with torch.no_grad(), engine.precision(mode):
        outs = run(enc, name, gpu)
    stages = [3] if indices == 1 else [0, 2] if indices == [0, 2] else [0, 1, 2, 3]
    assert len(outs) == len(stages)
    H, W = DINOV3_CONVNEXT_CASES[name]["hw"]
    for o, i in zip(outs, stages):
        want = gold[f"{name}/stage3_norm"] if (norm and i == 3) else gold[f"{name}/stage{i}_raw"]      # the final norm has stage 3's width only
        assert tuple(o.features.shape) == want.shape == (DINOV3_CONVNEXT_CASES[name]["B"], HIDDEN_SIZES[i], H // (4 << i), W // (4 << i))
        assert o.features.dtype == torch.float32
        e = rel_l2(o.features.cpu(), want)
        assert e < tol, (i, e)
    if norm and 3 in stages:       # stage 3 through the final norm is the encoder's own output
        own = build(checkpoint).eval().to(gpu)
        with torch.no_grad(), engine.precision(mode):
            assert torch.equal(outs[-1].features, run(own, name, gpu).features)
        assert rel_l2(outs[-1].features.cpu(), gold[f"{name}/features"]) < tol


@pytest.mark.parametrize("name", DINOV3_CONVNEXT_GRAD_CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gradients_match_huggingface_transformers_autograd(gpu, gold, checkpoint, name, mode):
    """Gradients of <features, Wf> with respect to every parameter (stem, depthwise and pointwise convolutions, LayerScale gammas, every
    LayerNorm, the stage downsamples — through the floor of the stride-2 gather on 48x80's odd maps —, the final norm) against
    transformers' autograd on the same weights."""
    from uniception_amd import engine
    enc = build(checkpoint).train().to(gpu)
    with engine.precision(mode):
        out = run(enc, name, gpu)
        loss = (out.features * convnext_grad_weights(name, out.features.shape).to(gpu)).sum()
    loss.backward()
    torch.cuda.synchronize()
    want_loss = float(gold[f"{name}/loss"])
    if mode == "fp32":
        assert abs(float(loss.detach()) - want_loss) <= 1e-4 * max(1.0, abs(want_loss)), (float(loss.detach()), want_loss)
    got_all, ref_all, worst, n = [], [], ("", 0.0), 0
    for k, p in enc.named_parameters():
        key = f"{name}/grad/{k}__samples"
        assert key in gold, k
        assert p.grad is not None, k                                              # every parameter has a gradient
        idx = torch.from_numpy(sample_indices(p.numel(), 512)).to(gpu)
        got = p.grad.flatten()[idx].double().cpu()
        ref = torch.from_numpy(gold[key]).double()
        want_n, got_n = float(gold[f"{name}/grad/{k}__norm"]), float(p.grad.double().norm())
        e = max(rel_l2(got, ref), abs(got_n - want_n) / max(want_n, 1e-30))
        if e > worst[1]:
            worst = (k, e)
        got_all.append(got)
        ref_all.append(ref)
        n += 1
    got_all, ref_all = torch.cat(got_all), torch.cat(ref_all)
    cos = float(torch.dot(got_all, ref_all) / (got_all.norm() * ref_all.norm()))
    print(f"\n[dinov3_convnext {mode} grads vs transformers autograd] {name}: {n} parameters, worst {worst[0]} {worst[1]:.2e}, cosine {cos:.6f}")
    assert n == sum(1 for f in gold if f.startswith(f"{name}/grad/") and f.endswith("__samples"))      # the parameter count equals the golden's
    if mode == "fp32":
        assert worst[1] < 1e-3, worst
    else:
        assert cos > 0.999, cos


def test_the_input_image_receives_a_gradient(gpu, checkpoint):
    from uniception_amd import engine
    from uniception_amd.models.encoders.base import ViTEncoderInput
    enc = build(checkpoint).train().to(gpu)
    for p in enc.parameters():
        p.requires_grad_(False)
    img = convnext_image(DINOV3_CONVNEXT_CASES["48x80"]).to(gpu).requires_grad_()
    with engine.precision("fp32"):
        enc(ViTEncoderInput(image=img, data_norm_type="dinov3")).features.square().sum().backward()
    torch.cuda.synchronize()
    assert img.grad is not None and img.grad.shape == img.shape and torch.isfinite(img.grad).all() and bool(img.grad.any())


def test_named_size_tiny_runs_at_64x96(gpu):
    "the published widths 96, 192, 384, 768 and depths 3, 3, 9, 3 (random initialisation): shapes of the features and of the four stage maps"
    from uniception_amd import engine
    from uniception_amd.models.encoders import feature_returner_encoder_factory
    from uniception_amd.models.encoders.base import ViTEncoderInput
    torch.manual_seed(0)
    enc = feature_returner_encoder_factory("dinov3_convnext", name="cn_t", dinov3_repo_dir=None, size="tiny", indices=None).eval().to(gpu)
    img = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).to(gpu)
    with torch.no_grad(), engine.precision("bf16"):
        outs = enc(ViTEncoderInput(image=img, data_norm_type="dinov3"))
    assert [tuple(o.features.shape) for o in outs] == [(2, 96, 16, 24), (2, 192, 8, 12), (2, 384, 4, 6), (2, 768, 2, 3)]
    assert all(torch.isfinite(o.features).all() and o.features.dtype == torch.float32 for o in outs)
