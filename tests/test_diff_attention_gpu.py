"""GPU: the fused differential-attention kernels against an fp64 CPU statement of the layer (kernel level), and the new modules
against golden vectors of the REAL reference (tests/golden/diff_attention.npz), outputs and every gradient.

Tolerances.
  fp32, module level: the gates the sibling tests apply to the plain transformers (tests/test_multiview_transformers_gpu.py: rel-L2
    < 1e-3 on outputs, input gradients, sampled parameter gradients and their norms).
  fp32, kernel level: rel-L2 < 1e-5 — fp32 has unit roundoff 6e-8, every output is a sum of at most 200 terms of one sign pattern
    (softmax weights), so 1e-5 leaves two orders of magnitude for the summation order and expf; LSE to 2e-5 absolute (|LSE| < 10).
  bf16, module level: 2 x the error of the reference's OWN arithmetic run in bfloat16 on the CPU against its fp32 result, stored in
    the fixture per quantity (the factor 2 allows for a different summation order).
  bf16, kernel level: the same rule with the yardstick computed here — the layer's formula evaluated by PyTorch in bfloat16 on the
    CPU from the same bf16 inputs, against fp64.  The combine-backward writes dA in bf16: one rounding (2^-9 relative per element)
    on top of fp32 arithmetic, bound 2^-8; its fp32 reductions d lambda and d w: 1e-5 like fp32."""
import os

import numpy as np
import pytest
import torch

from tests.golden.cases import sample_indices
from tests.golden.diff_cases import CASES, cotangents, fill, inputs, resolve, run
from tests.helpers import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu

B, H = 2, 3
EPS, LAM, OUT_SCALE = 1e-5, 0.37, 0.64


def layer_statement(q, k, v, w, scale, dtype):
    """The layer as the reference writes it (utils/transformer_blocks.py:908-940) on q [B,Nq,2H,hd], k [B,Nk,2H,hd], v [B,Nk,H,2hd] in
    `dtype` (float64: the truth; bfloat16: the yardstick).  Returns y [B,Nq,H,2hd], lse1, lse2 [B,H,Nq]."""
    q, k, v = (t.to(dtype).permute(0, 2, 1, 3) for t in (q, k, v))
    outs, lses = [], []
    for qi, ki in zip(q.chunk(2, dim=1), k.chunk(2, dim=1)):
        s = (qi * scale) @ ki.transpose(-2, -1)
        lses.append(torch.logsumexp(s.double(), dim=-1))
        outs.append(s.softmax(dim=-1) @ v)
    a = (outs[0] - LAM * outs[1]).transpose(1, 2)
    n = (a.float() if dtype != torch.float64 else a)
    n = (n * torch.rsqrt(n.pow(2).mean(-1, keepdim=True) + EPS)).to(dtype) * w.to(dtype)
    return n * OUT_SCALE, lses[0], lses[1]


def make_qkv(Nq, Nk, hd, dtype, strided, seed):
    g = torch.Generator().manual_seed(seed)
    C = 2 * H * hd
    if strided:      # q | k | v views of one fused [B, N, 3C] buffer (the DiffAttention layout); Nq == Nk
        t = torch.randn(B, Nq, 3 * C, generator=g).to(dtype)
        return t, lambda t: (t[:, :, :C].view(B, Nq, 2 * H, hd), t[:, :, C:2 * C].view(B, Nk, 2 * H, hd), t[:, :, 2 * C:].view(B, Nk, H, 2 * hd))
    t = (torch.randn(B, Nq, 2 * H, hd, generator=g).to(dtype), torch.randn(B, Nk, 2 * H, hd, generator=g).to(dtype),
         torch.randn(B, Nk, H, 2 * hd, generator=g).to(dtype))
    return t, lambda t: t


SHAPES = [(64, 64, 32, False), (77, 77, 32, False), (200, 136, 32, False), (77, 77, 32, True)]


@pytest.mark.parametrize("dtype,Nq,Nk,hd,strided",
                         [(dt, *s) for dt in (torch.float32, torch.bfloat16) for s in SHAPES] + [(torch.float32, 77, 52, 16, False)])
def test_fused_forward_and_lse_against_fp64(gpu, dtype, Nq, Nk, hd, strided):
    from uniception_amd import ops
    host, views = make_qkv(Nq, Nk, hd, dtype, strided, 1000 + Nq + hd)
    q, k, v = views(host)
    w = 1.0 + 0.3 * torch.randn(2 * hd, generator=torch.Generator().manual_seed(5))
    scale = hd ** -0.5
    want, l1, l2 = layer_statement(q, k, v, w, scale, torch.float64)
    dev = host.to(gpu) if strided else tuple(t.to(gpu) for t in host)
    qd, kd, vd = views(dev)
    bf = dtype == torch.bfloat16
    out, (lse1, lse2, a1, a2) = ops.diff_attention(qd, kd, ops.vt_pack(vd) if bf else vd, scale, LAM, w.to(gpu), EPS, OUT_SCALE,
                                                   v_packed=bf, save=True)
    plain = ops.diff_attention(qd, kd, ops.vt_pack(vd) if bf else vd, scale, LAM, w.to(gpu), EPS, OUT_SCALE, v_packed=bf)
    torch.cuda.synchronize()
    assert torch.equal(out, plain)          # the saves do not change the result
    if bf:
        yard = rel_l2(layer_statement(q, k, v, w, scale, torch.bfloat16)[0].double(), want)
        tol = 2.0 * yard
    else:
        tol = 1e-5
    err = rel_l2(out.float().cpu(), want)
    print(f"forward {dtype} Nq {Nq} Nk {Nk} hd {hd} strided {strided}: rel-L2 {err:.3e} (bound {tol:.3e})")
    assert err < tol
    for got, ref in ((lse1, l1), (lse2, l2)):
        assert float((got.cpu().double() - ref).abs().max()) < 2e-5
    # the saved attention outputs are those of the two softmaxes (bf16: P and the stored value are each rounded once, 2^-9 relative per
    # element, and the fp32 sums sit between them: bound 2^-7)
    qh, kh, vh = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    for a, i in ((a1, 0), (a2, 1)):
        ref = ((qh[:, i * H:(i + 1) * H] * scale) @ kh[:, i * H:(i + 1) * H].transpose(-2, -1)).softmax(-1) @ vh
        assert rel_l2(a.float().cpu().permute(0, 2, 1, 3), ref) < (2.0 ** -7 if bf else 1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,D,head_major", [(77, 64, False), (200, 64, True), (52, 32, False)])
def test_combine_backward_against_fp64_and_bitwise_reproducible(gpu, dtype, N, D, head_major):
    from uniception_amd import ops
    g = torch.Generator().manual_seed(N + D)
    a1, a2 = (torch.randn(B, N, H, D, generator=g).to(dtype) for _ in range(2))
    dy = torch.randn((B, H, N, D) if head_major else (B, N, H, D), generator=g).to(dtype)
    w = 1.0 + 0.3 * torch.randn(D, generator=g)
    dy4 = dy.permute(0, 2, 1, 3) if head_major else dy
    A1, A2, W = (t.double().requires_grad_(True) for t in (a1, a2, w))
    lam = torch.tensor(LAM, dtype=torch.float64, requires_grad=True)
    a = A1 - lam * A2
    y = a * torch.rsqrt(a.pow(2).mean(-1, keepdim=True) + EPS) * W * OUT_SCALE
    (y * dy4.double()).sum().backward()
    dyd = dy.to(gpu)
    args = (dyd.permute(0, 2, 1, 3) if head_major else dyd, a1.to(gpu), a2.to(gpu), LAM, w.to(gpu), EPS, OUT_SCALE)
    first = ops.diff_attention_combine_bwd(*args)
    second = ops.diff_attention_combine_bwd(*args)
    torch.cuda.synchronize()
    for x, y2 in zip(first, second):
        assert torch.equal(x, y2)           # fixed-order reductions: the same bits
    da1, da2, dw, dl = (t.float().cpu() for t in first)
    tol = 2.0 ** -8 if dtype == torch.bfloat16 else 1e-5
    errs = dict(dA1=rel_l2(da1, A1.grad), dA2=rel_l2(da2, A2.grad), dw=rel_l2(dw, W.grad), dlambda=rel_l2(dl, lam.grad))
    print(dtype, N, D, errs)
    assert errs["dA1"] < tol and errs["dA2"] < tol and errs["dw"] < 1e-5 and errs["dlambda"] < 1e-5


# ---- module level, against the reference's golden vectors --------------------------------------------------------------------------
def _build(kind, kw):
    from uniception_amd.models import info_sharing
    from uniception_amd.models.libs.croco.pos_embed import RoPE2D
    from uniception_amd.models.utils import transformer_blocks as TB
    cls = getattr(TB, kind, None) or getattr(info_sharing, kind)
    return cls(**resolve(kw, RoPE2D))


_gold = {}


def gold():
    if not _gold:
        _gold["z"] = np.load(os.path.join(GOLDEN_DIR, "diff_attention.npz"))
    return _gold["z"]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_module_outputs_and_gradients_against_the_reference(gpu, name, mode):
    from uniception_amd import engine
    from uniception_amd.models.info_sharing import MultiViewTransformerInput
    z = gold()
    kind, kw = CASES[name]
    model = _build(kind, kw).train()
    fill(model, name)
    for k, p in model.named_parameters():            # the perturbed parameters are what the fixture was made with
        if f"{name}/diffp/{k}" in z.files:
            torch.testing.assert_close(p.detach(), torch.from_numpy(z[f"{name}/diffp/{k}"]))
    model = model.to(gpu)
    ins, pos = inputs(name)
    ins = [t.to(gpu).requires_grad_(True) for t in ins]
    pos = [p.to(gpu) for p in pos]
    with engine.precision(mode):
        outs = run(name, model, ins, pos, MultiViewTransformerInput)
        ws = cotangents(name, [tuple(o.shape) for o in outs])
        loss = sum((o.float() * w.to(gpu)).sum() for o, w in zip(outs, ws))
    loss.backward()
    torch.cuda.synchronize()

    def bound(key):
        return 1e-3 if mode == "fp32" else 2.0 * float(z[f"{name}/bf16/{key}"])

    report, bad = [], []

    def check(what, key, got, want):
        e, b = rel_l2(got, want), bound(key)
        report.append(f"{what}: rel-L2 {e:.3e} (bound {b:.3e})")
        if not e < b:
            bad.append(report[-1])

    for j, o in enumerate(outs):
        check(f"out{j}", f"out{j}", o.detach().float().cpu(), z[f"{name}/out{j}"])
    for i, t in enumerate(ins):
        check(f"din{i}", f"din{i}", t.grad.float().cpu(), z[f"{name}/din{i}"])
    params = dict(model.named_parameters())
    want_keys = sorted(k[len(name) + 3:-len("__samples")] for k in z.files if k.startswith(f"{name}/p/") and k.endswith("__samples"))
    assert want_keys == sorted(params)
    for k in want_keys:
        want, want_n = z[f"{name}/p/{k}__samples"], float(z[f"{name}/p/{k}__norm"])
        g = params[k].grad
        assert g is not None, f"{k}: no gradient"
        if want_n < 1e-12:
            assert float(g.double().norm()) < 1e-6, k
            continue
        check(f"d {k}", f"p/{k}", g.flatten()[torch.from_numpy(sample_indices(g.numel(), want.size)).to(gpu)].float().cpu(), want)
        if mode == "fp32":
            got_n = float(g.double().norm())
            assert abs(got_n - want_n) < 1e-3 * want_n, f"{k}: norm {got_n} vs {want_n}"
    print("\n".join(report))
    assert not bad, bad


def test_state_dict_round_trip_and_inference_forward(gpu):
    "load_state_dict(strict=True) between two instances; the inference forward (eval, no autograd graph) meets the fp32 gate of the fixture"
    from uniception_amd import engine
    from uniception_amd.models.info_sharing import MultiViewTransformerInput
    kind, kw = CASES["transformer"]
    model = _build(kind, kw).eval()
    fill(model, "transformer")
    other = _build(kind, kw)
    other.load_state_dict(model.state_dict(), strict=True)
    model = model.to(gpu)
    ins, _ = inputs("transformer")
    ins = [t.to(gpu) for t in ins]
    with engine.precision("fp32"), torch.no_grad():
        a = model(MultiViewTransformerInput(features=ins)).features
    z = gold()
    for j, o in enumerate(a):
        assert rel_l2(o.float().cpu(), z[f"transformer/out{j}"]) < 1e-3
