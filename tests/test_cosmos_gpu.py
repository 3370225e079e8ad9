"""GPU: the Cosmos tokenizer kernels against the float64 formulas of tests/cosmos_formulas.py, the wide single-head attention against
float64, and CosmosEncoder / CosmosSingleChannel / CosmosFeature against the float64 run of the REAL reference (tests/golden/cosmos.npz),
outputs and every gradient, in train mode.

Tolerances (the rules of test_moge_heads_gpu.py).
  fp32 kernels: rel-L2 <= 1e-5 against float64; 1e-6 for the Haar transform, the nearest upsample and the inner-product identity
    <A x, y> = <x, A^T y> of every adjoint pair; the gathers are exact.
  bf16 / fp16 kernels: <= 2 x the error of the same formula evaluated by PyTorch in that dtype on the CPU from the same rounded inputs.
  GroupNorm inputs are 0.5 + N(0, 1); x = 100 + N(0, 1) in fp32 must give rstd within 1e-4 of float64.
  modules, fp32: outputs within max(2e-6, 8 e32), gradients within 1e-3; bf16: every quantity within 2 x e16 (e32 / e16: the reference's
    own fp32 / bfloat16-on-CPU error against float64, from the fixture).  Parameter-gradient errors are normalised as
    cosmos_cases.grad_errors does, in the fixture and here."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import cosmos_formulas as cf
from tests.golden.cases import sample_indices
from tests.golden.cosmos_cases import CASES, MODULE_OF, NSAMP, cotangent, fill, grad_errors, input_of, run
from tests.helpers import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu

LOW = [torch.bfloat16, torch.float16]
DTYPES = [torch.float32] + LOW
_GOLD = []


def gold():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(GOLDEN_DIR, "cosmos.npz")))
    return _GOLD[0]


def _rand(shape, seed, dtype=torch.float32, mean=0.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) + mean).to(dtype)


def _check(what, got, ref, bounds):
    "every got[k] within bounds[k] of ref[k] (rel-L2), all figures printed before the assertion"
    bad = []
    for k in got:
        err = rel_l2(got[k].detach().cpu().double(), ref[k].double())
        print(f"{what} {k}: rel-L2 {err:.3e} (bound {bounds[k]:.3e})")
        if not err <= bounds[k]:
            bad.append((k, err, bounds[k]))
    assert not bad, bad


def _dot_identity(what, ax, y, x, aty):
    "<A x, y> = <x, A^T y> to 1e-6 of |A x| |y|"
    ax, y, x, aty = (t.detach().cpu().double() for t in (ax, y, x, aty))
    err = abs(float((ax * y).sum()) - float((x * aty).sum())) / float(ax.norm() * y.norm())
    print(f"{what}: <A x, y> - <x, A^T y> = {err:.3e} (bound 1e-6)")
    assert err <= 1e-6


# ---- Haar patcher ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,H,W", [(1, 3, 4, 4), (2, 3, 8, 12), (1, 3, 36, 20)])
def test_haar_patch_and_unpatch_against_fp64(gpu, B, C, H, W, dtype):
    from uniception_amd import ops
    img = _rand((B, C, H, W), 1 + H)
    want = cf.haar_patch(img.double()).permute(0, 2, 3, 1)
    got = ops.haar_patch(img.to(gpu), dtype, 64)
    assert got.shape == (B, H // 4, W // 4, 64) and got.dtype == dtype
    assert float(got[..., 16 * C:].abs().max()) == 0.0                      # the K padding is written, as zeros
    tight = ops.haar_patch(img.to(gpu), dtype)
    assert tight.shape[-1] == 16 * C and torch.equal(tight, got[..., :16 * C])
    bound = 1e-6 if dtype == torch.float32 else 2.0 * rel_l2(cf.haar_patch(img.to(dtype)).permute(0, 2, 3, 1).double(), want)
    rows = _rand((B, H // 4, W // 4, 64), 2 + H, dtype)
    want_u = cf.haar_unpatch(rows[..., :16 * C].double().permute(0, 3, 1, 2))
    got_u = ops.haar_unpatch(rows.to(gpu), C)
    assert got_u.shape == (B, C, H, W) and got_u.dtype == torch.float32
    bound_u = 1e-6 if dtype == torch.float32 else 2.0 * rel_l2(cf.haar_unpatch(rows[..., :16 * C].permute(0, 3, 1, 2)).double(), want_u)
    _check(f"haar {dtype} {(B, C, H, W)}", dict(patch=got[..., :16 * C], unpatch=got_u), dict(patch=want, unpatch=want_u),
           dict(patch=bound, unpatch=bound_u))
    if dtype == torch.float32:
        assert rel_l2(ops.haar_unpatch(got, C).cpu(), img) <= 1e-6          # the inverse round-trips
        y = _rand((B, H // 4, W // 4, 16 * C), 3 + H)
        _dot_identity("haar patch", tight, y, img, ops.haar_unpatch(y.to(gpu), C, 1.0 / 16.0))
        g = _rand((B, C, H, W), 4 + H)
        _dot_identity("haar unpatch", ops.haar_unpatch(y.to(gpu), C), g, y, ops.haar_patch(g.to(gpu), dtype, None, 16.0))


# ---- GroupNorm + SiLU ------------------------------------------------------------------------------------------------------------
# (1, 23, 29, 256, 32): 667 pixels cross the 64-pixel chunk of C = 256; (2, 4, 5, 128, 32): groups of four channels (Normalize(128))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C,G", [(2, 4, 5, 256, 32), (1, 2, 3, 512, 32), (1, 23, 29, 256, 32), (2, 4, 5, 128, 32), (1, 9, 7, 128, 32)])
def test_group_norm_silu_forward_and_backward_against_fp64(gpu, B, H, W, C, G, dtype):
    from uniception_amd import ops
    eps = 1e-6
    x = _rand((B, H, W, C), 10 + H + C, dtype, 0.5)
    dy = _rand((B, H, W, C), 20 + H + C, dtype, 0.25)
    gamma = 1.0 + 0.1 * _rand((C,), 30 + C)
    beta = 0.1 * _rand((C,), 40 + C)
    y64, mean64, rstd64 = cf.group_norm_silu(x.double(), gamma.double(), beta.double(), G, eps)
    dx64, dg64, db64 = cf.group_norm_silu_bwd(dy.double(), x.double(), gamma.double(), beta.double(), G, eps)
    xd, dyd, gd, bd = x.to(gpu), dy.to(gpu), gamma.to(gpu), beta.to(gpu)
    y, mean, rstd = ops.group_norm_silu_nhwc(xd, gd, bd, G, eps)
    dx, dg, db = ops.group_norm_silu_nhwc_bwd(dyd, xd, mean, rstd, gd, bd)
    y2, mean2, rstd2 = ops.group_norm_silu_nhwc(xd, gd, bd, G, eps)
    dx2, dg2, db2 = ops.group_norm_silu_nhwc_bwd(dyd, xd, mean2, rstd2, gd, bd)
    torch.cuda.synchronize()
    assert y.dtype == dtype and dx.dtype == dtype and dg.dtype == db.dtype == mean.dtype == rstd.dtype == torch.float32
    for a, b in ((y, y2), (mean, mean2), (rstd, rstd2), (dx, dx2), (dg, dg2), (db, db2)):
        assert torch.equal(a, b)                    # fixed-order reductions: two calls give the same bits
    got = dict(y=y, dx=dx, dgamma=dg, dbeta=db, mean=mean, rstd=rstd)
    ref = dict(y=y64, dx=dx64, dgamma=dg64, dbeta=db64, mean=mean64, rstd=rstd64)
    bounds = dict.fromkeys(got, 1e-5)
    if dtype != torch.float32:
        # the twin: statistics and x^ in `dtype`, gamma / beta in fp32 as the kernel reads them, maps rounded to `dtype` as it writes them
        y_t = cf.group_norm_silu(x, gamma, beta, G, eps)[0].to(dtype)
        dx_t, dg_t, db_t = cf.group_norm_silu_bwd(dy, x, gamma, beta, G, eps)
        for k, t in zip(("y", "dx", "dgamma", "dbeta"), (y_t, dx_t.to(dtype), dg_t, db_t)):
            bounds[k] = 2.0 * rel_l2(t.double(), ref[k])
    _check(f"group_norm_silu {dtype} {(B, H, W, C, G)}", got, ref, bounds)


def test_group_norm_silu_statistics_do_not_cancel_at_an_offset(gpu):
    from uniception_amd import ops
    for B, H, W, C, G in ((2, 23, 29, 256, 32), (2, 23, 29, 128, 32)):
        x = 100.0 + _rand((B, H, W, C), 5 + C)
        xg = x.double().view(B, H * W, G, C // G)
        rstd64 = 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + 1e-6)
        _, mean, rstd = ops.group_norm_silu_nhwc(x.to(gpu), torch.ones(C, device=gpu), torch.zeros(C, device=gpu), G, 1e-6)
        worst = float(((rstd.cpu().double() - rstd64).abs() / rstd64).max())
        print(f"C {C}: rstd at offset 100: worst relative error {worst:.3e} (bound 1e-4)")
        assert worst <= 1e-4
        assert float(((mean.cpu().double() - xg.mean(dim=(1, 3))).abs() / 100.0).max()) <= 1e-6


def test_plain_group_norm_still_refuses_groups_of_four(gpu):
    from uniception_amd import ops
    from uniception_amd._lib import UcHipError
    with pytest.raises(UcHipError, match="channels per group .4. must be a multiple of 8"):
        ops.group_norm_nhwc(torch.zeros(1, 2, 2, 128, device=gpu), torch.ones(128, device=gpu), torch.zeros(128, device=gpu), 32, 1e-6)


# ---- Downsample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 8), (2, 4, 6, 64), (1, 10, 6, 128)])
def test_down2_gather_is_exact_and_its_adjoint_is_the_adjoint(gpu, B, H, W, C, dtype):
    from uniception_amd import ops
    x = _rand((B, H, W, C), 50 + H + C, dtype)
    rows = ops.down2_gather(x.to(gpu))
    assert rows.shape == (B * (H // 2) * (W // 2), 9 * C) and torch.equal(rows.cpu(), cf.down2_rows(x))
    r6 = rows.cpu().view(B, H // 2, W // 2, 3, 3, C)
    # by hand: the third tap row of the last output row and the third tap column of the last output column are the zero pad, and the
    # tap before them is the map's last row / column — not the next row's first pixel
    assert float(r6[:, -1, :, 2].abs().max()) == 0.0 and float(r6[:, :, -1, :, 2].abs().max()) == 0.0
    assert torch.equal(r6[:, -1, :, 1, 0], x[:, H - 1, 0::2]) and torch.equal(r6[:, :, -1, 0, 1], x[:, 0::2, W - 1])
    d = _rand(tuple(rows.shape), 51 + H + C, dtype)
    got = ops.down2_gather_bwd(d.to(gpu), B, H, W)
    assert torch.equal(got, ops.down2_gather_bwd(d.to(gpu), B, H, W))
    want = cf.down2_rows_adjoint(d.double(), B, H, W)
    bound = 1e-5 if dtype == torch.float32 else 2.0 * rel_l2(cf.down2_rows_adjoint(d, B, H, W).double(), want)
    _check(f"down2 adjoint {dtype} {(B, H, W, C)}", dict(dx=got), dict(dx=want), dict(dx=bound))
    if dtype == torch.float32:
        _dot_identity("down2 gather", rows, d, x, got)


def test_down2_gather_refuses_an_odd_map(gpu):
    from uniception_amd import ops
    from uniception_amd._lib import UcHipError
    with pytest.raises(UcHipError, match="odd map"):
        ops.down2_gather(torch.zeros(1, 3, 4, 8, device=gpu))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_downsample_and_upsample_modules_against_fp64(gpu, mode):
    from uniception_amd import engine
    from uniception_amd.models.libs.cosmos_tokenizer.modules.layers2d import Downsample, Upsample
    B, H, W, C = 2, 4, 6, 64
    dtype = torch.float32 if mode == "fp32" else torch.bfloat16
    for cls in (Downsample, Upsample):
        torch.manual_seed(3)
        m = cls(C)
        x = _rand((B, H, W, C), 60, dtype)
        w0, b0 = m.conv.weight.detach().clone(), m.conv.bias.detach().clone()
        wq = w0.to(dtype)              # the kernel multiplies the weights rounded to the operand dtype

        def cpu(dt):
            xc = x.to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            w, b = (wq if dt == torch.float64 else w0).to(dt).requires_grad_(True), b0.to(dt).requires_grad_(True)
            if cls is Downsample:
                y = F.conv2d(F.pad(xc, (0, 1, 0, 1)), w, b, stride=2)
            else:
                y = F.conv2d(xc.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), w, b, padding=1)
            dy = _rand(tuple(y.permute(0, 2, 3, 1).shape), 61, dtype)
            y.backward(dy.to(dt).permute(0, 3, 1, 2))
            return dict(y=y.detach().permute(0, 2, 3, 1).double(), dx=xc.grad.permute(0, 2, 3, 1).double(), dW=w.grad.double(), db=b.grad.double()), dy
        ref, dy = cpu(torch.float64)
        m = m.to(gpu)
        xd = x.to(gpu).requires_grad_(True)
        with engine.precision(mode):
            y = m.forward_nhwc(xd)
            y.backward(dy.to(gpu))
        torch.cuda.synchronize()
        got = dict(y=y, dx=xd.grad, dW=m.conv.weight.grad, db=m.conv.bias.grad)
        bounds = dict.fromkeys(got, 1e-5)
        if mode == "bf16":
            twin, _ = cpu(torch.bfloat16)
            bounds = {k: 2.0 * rel_l2(twin[k], ref[k]) for k in got}
        _check(f"{cls.__name__} {mode}", got, ref, bounds)


# ---- nearest upsample --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (2, 3, 5, 64)])
def test_upsample2_is_exact_and_its_adjoint_is_the_adjoint(gpu, B, H, W, C, dtype):
    from uniception_amd import ops
    x = _rand((B, H, W, C), 70 + H + C, dtype)
    y = ops.upsample2_nhwc(x.to(gpu))
    assert y.shape == (B, 2 * H, 2 * W, C) and torch.equal(y.cpu(), cf.upsample2(x))
    g = _rand((B, 2 * H, 2 * W, C), 71 + H + C, dtype)
    got = ops.upsample2_nhwc_bwd(g.to(gpu))
    want = cf.upsample2_adjoint(g.double())
    bound = 1e-6 if dtype == torch.float32 else 2.0 * rel_l2(cf.upsample2_adjoint(g).double(), want)
    _check(f"upsample2 adjoint {dtype} {(B, H, W, C)}", dict(dx=got), dict(dx=want), dict(dx=bound))
    if dtype == torch.float32:
        _dot_identity("upsample2", y, g, x, got)


# ---- row softmax -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,N", [(3, 1), (5, 12), (20, 20), (7, 1000), (2, 2050), (2, 4200)])
def test_softmax_rows_forward_and_backward_against_fp64(gpu, rows, N, dtype, padded):
    """padded: S and dP are the first N columns of buffers with a leading dimension of a multiple of 64 and P / dS are written with their
    zero padding (the 16-byte path); else everything is contiguous [rows, N] (the scalar path unless N % 8 == 0).  4200 columns: longer
    than the 4096 a workgroup keeps in registers."""
    from uniception_amd import ops
    scale = 512 ** -0.5
    s = 8.0 * _rand((rows, N), 80 + N)
    dp = _rand((rows, N), 81 + N)
    Np = (N + 63) // 64 * 64
    if padded:
        sbuf = torch.full((rows, Np), float("nan"), device=gpu)
        sbuf[:, :N] = s.to(gpu)
        p = ops.softmax_rows(sbuf[:, :N], scale, dtype, out=torch.full((rows, Np), 7.0, dtype=dtype, device=gpu))
        gbuf = torch.full((rows, Np), float("nan"), device=gpu)
        gbuf[:, :N] = dp.to(gpu)
        ds = ops.softmax_rows_bwd(p, gbuf[:, :N], N, scale)
        assert p.shape == ds.shape == (rows, Np)
        if Np > N:
            assert float(p[:, N:].float().abs().max()) == 0.0 and float(ds[:, N:].float().abs().max()) == 0.0
    else:
        p = ops.softmax_rows(s.to(gpu), scale, dtype)
        ds = ops.softmax_rows_bwd(p, dp.to(gpu), N, scale)
    torch.cuda.synchronize()
    p, ds = p[:, :N].cpu(), ds[:, :N].cpu()
    assert p.dtype == dtype and ds.dtype == dtype and bool(torch.isfinite(p.float()).all())
    p64 = cf.softmax_rows(s.double(), scale)
    ds64 = cf.softmax_rows_bwd(p.double(), dp.double(), scale)               # from the same (rounded) P the kernel read
    bounds = dict(P=1e-5, dS=1e-5)
    if dtype == torch.float32:
        worst = float((p.double().sum(1) - 1).abs().max())
        print(f"softmax {rows}x{N}: worst |row sum - 1| = {worst:.3e} (bound 1e-6)")
        assert worst <= 1e-6
    else:
        bounds = dict(P=2.0 * rel_l2(cf.softmax_rows(s.to(dtype), scale).double(), p64),
                      dS=2.0 * rel_l2(cf.softmax_rows_bwd(p, dp, scale).to(dtype).double(), ds64))      # (dP in fp32, as the kernel reads it)
    if N == 1:
        assert torch.equal(p.float(), torch.ones(rows, 1)) and float(ds.float().abs().max()) == 0.0       # (dS = 0: no relative error)
        return
    _check(f"softmax {dtype} {rows}x{N} padded={padded}", dict(P=p, dS=ds), dict(P=p64, dS=ds64), bounds)


# ---- wide single-head attention ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("N,panel", [(12, 4096), (20, 4096), (130, 4096), (20, 8), (130, 64)])
def test_wide_attention_against_fp64(gpu, N, panel, mode):
    """C = 512, one head over N pixels; panel < N: several score panels per sample, the seam between them is exercised.  fp16: the dtype
    the head's maps have in inference under the default head policy (the products follow the operands' dtype)."""
    from uniception_amd import autograd, engine
    B, C = 2, 512
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    scale = C ** -0.5
    qkv = (2.0 * _rand((B * N, 3 * C), 90 + N)).to(dtype)
    do = _rand((B * N, C), 91 + N, dtype)

    def cpu(dt):
        t = qkv.to(dt).requires_grad_(True)
        o = cf.wide_attention(t, B, N, scale)
        o.backward(do.to(dt))
        return dict(o=o.detach().double(), dqkv=t.grad.double())
    ref = cpu(torch.float64)
    t = qkv.to(gpu).requires_grad_(True)
    with engine.precision("fp32" if mode == "fp32" else "bf16"):
        o = autograd.wide_attention(t, B, N, scale, panel)
        o.backward(do.to(gpu))
    torch.cuda.synchronize()
    assert o.dtype == dtype and o.shape == (B * N, C) and t.grad.shape == qkv.shape
    bounds = dict(o=1e-5, dqkv=1e-5)
    if mode != "fp32":
        twin = cpu(dtype)
        bounds = {k: 2.0 * rel_l2(twin[k], ref[k]) for k in ref}
    _check(f"wide_attention {mode} N {N} panel {panel}", dict(o=o, dqkv=t.grad), ref, bounds)


# ---- modules -----------------------------------------------------------------------------------------------------------------------
def _model(name, gpu):
    kind, kw, _ = CASES[name]
    cls = getattr(importlib.import_module(f"uniception_amd.models.{MODULE_OF[kind]}"), kind)
    model = cls(**kw)
    fill(model)                                # the reference's state_dict, rebuilt from the case's seeds (name-keyed filler)
    return model.to(gpu)


def _run(name, model, x):
    from uniception_amd.models.encoders.base import ViTEncoderInput
    from uniception_amd.models.prediction_heads.base import PredictionHeadInput
    return run(name, model, x, ViTEncoderInput, PredictionHeadInput)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_module_forward_and_backward_against_the_reference_in_fp64(gpu, name, mode, capsys):
    from uniception_amd import engine
    G = gold()
    with capsys.disabled():
        model = _model(name, gpu).train()
    x = input_of(name).to(gpu).requires_grad_(True)
    with engine.precision(mode):
        outs = _run(name, model, x)
        (outs[0].float() * cotangent(name, tuple(outs[0].shape)).to(gpu)).sum().backward()
    torch.cuda.synchronize()
    fp32 = mode == "fp32"
    tag = "e32" if fp32 else "e16"
    errs = {}
    for i, o in enumerate(outs):
        assert tuple(o.shape) == G[f"{name}/out{i}"].shape
        errs[f"out{i}"] = rel_l2(o.detach().float().cpu(), torch.from_numpy(G[f"{name}/out{i}"]))
    assert outs[0].dtype == torch.float32 and f"{name}/out{len(outs)}" not in G.files
    assert x.grad is not None
    errs["din"] = rel_l2(x.grad.cpu(), torch.from_numpy(G[f"{name}/din"]))
    names = str(G[f"{name}/p_names"]).split("\n")
    params = dict(model.named_parameters())
    assert list(params) == names
    got, want = {}, {}
    for j, k in enumerate(names):
        assert params[k].grad is not None, f"{k} received no gradient"
        idx = torch.from_numpy(sample_indices(params[k].numel(), NSAMP))
        got[k], want[k] = params[k].grad.flatten().cpu()[idx], torch.from_numpy(G[f"{name}/p_samples"][j][:len(idx)])
    perr = grad_errors(got, want)
    bad = []
    for q, err in errs.items():
        ref_err = float(G[f"{name}/{tag}/{q}"])
        bound = (max(2e-6, 8.0 * ref_err) if q.startswith("out") else 1e-3) if fp32 else 2.0 * ref_err
        print(f"{name} {mode} {q}: {err:.3e} (bound {bound:.3e})")
        if not err < bound:
            bad.append((q, err, bound))
    ratios = []
    for j, k in enumerate(names):
        bound = 1e-3 if fp32 else 2.0 * float(G[f"{name}/{tag}/p"][j])
        ratios.append((perr[k] / bound, k))
        if not perr[k] < bound:
            bad.append((f"p/{k}", perr[k], bound))
    worst = max(ratios)
    print(f"{name} {mode} parameter gradients: worst error / bound = {worst[0]:.3f} ({worst[1]}), {len(names)} parameters")
    assert not bad, bad


@pytest.mark.parametrize("name", ["single_p8", "feature_p16"])
def test_head_inference_under_the_default_head_policy_stays_within_the_bf16_bound(gpu, name, capsys):
    "no_grad next to a bf16 transformer: the default head policy gives the head fp16 maps; every output within 2 x e16"
    from uniception_amd import engine
    with capsys.disabled():
        model = _model(name, gpu).eval()
    with torch.no_grad(), engine.precision("bf16"):
        policy, dt = engine.head_dtype_name(), engine.head_dtype()
        outs = _run(name, model, input_of(name).to(gpu))
    torch.cuda.synchronize()
    assert (policy, dt) == ("fp16", torch.float16), (policy, dt)          # the path this test is about
    assert outs[0].grad_fn is None and outs[0].dtype == torch.float32
    bad = []
    for i, o in enumerate(outs):
        err, bound = rel_l2(o.float().cpu(), torch.from_numpy(gold()[f"{name}/out{i}"])), 2.0 * float(gold()[f"{name}/e16/out{i}"])
        print(f"{name} inference, head policy {policy}, out{i}: rel-L2 {err:.3e} (bound {bound:.3e})")
        if not err < bound:
            bad.append((i, err, bound))
    assert not bad, bad


def test_encoder_forward_is_captured_into_a_hip_graph(gpu, capsys):
    "one capture-and-replay of enc_p8's forward: the replay gives the eager output bit for bit"
    from uniception_amd import engine, ops
    name = "enc_p8"
    with capsys.disabled():
        model = _model(name, gpu).eval()
    static = input_of(name).to(gpu)

    def forward():
        with torch.no_grad(), engine.precision("bf16"):
            return _run(name, model, static)[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = forward().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    err, bound = rel_l2(eager.cpu(), torch.from_numpy(gold()[f"{name}/out0"])), 2.0 * float(gold()[f"{name}/e16/out0"])
    print(f"{name} inference: rel-L2 {err:.3e} (bound {bound:.3e})")
    assert err < bound
    token = 0x436F736D
    ops.fuse_ws_reserve(4)
    graph = torch.cuda.CUDAGraph()
    try:
        with ops.capture_scope(token), torch.cuda.graph(graph):
            out = forward()
        keep = static.clone()
        static.add_(1.0)
        graph.replay()                      # another input: the graph really recomputes
        torch.cuda.synchronize()
        assert not torch.equal(out, eager)
        static.copy_(keep)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    finally:
        torch.cuda.synchronize()
        del graph
