"""GPU: uc_vit_stem and uc_vit_stem_bwd (csrc/vit_stem.hip) against the formula
    z[b, t] = (t < ncls ? cls : tok[b, t - ncls]) + pos[t],   y = LN(z) gamma + beta
evaluated by PyTorch in float64 on the CPU, and its float64 autograd for the five gradients (dtok, dcls, dpos, dgamma, dbeta).

Shapes: (B 2, hw 15, class token, C 128): an odd token count, one image slab, two token groups of the backward; (B 3, hw 72, no class
token, C 192): no offset between token and row, nine token groups, a row that does not fill the 64 lanes x 8 channels of a chunk; the
first shape again without the LayerNorm.  With B <= 8 the backward has one image slab; (B 9, hw 15) adds the second one.
Tolerance, rel-L2 per output and gradient: fp32 -> fp32: max(2e-6, 8 e), bf16 -> bf16: 2 e, where e is the error against float64 of
PyTorch's own evaluation of the same formula on the CPU in the storage dtype (float32, bfloat16), measured here on the same inputs.
The backward's five results are the same bits on every call (fixed-order sums, no atomics)."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu

EPS = 1e-5
SHAPES = [(2, 15, True, 128, True), (3, 72, False, 192, True), (2, 15, True, 128, False), (9, 15, True, 128, True)]      # B, hw, cls, C, LN
NAMES = ("y", "dtok", "dcls", "dpos", "dgamma", "dbeta")


def _rand(shape, seed, mean=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) + mean


def _case(B, hw, with_cls, C, with_ln, dtype):
    T = hw + int(with_cls)
    s = 1000 * B + 10 * hw + C
    return dict(tok=_rand((B, hw, C), s, 0.5).to(dtype), cls=_rand((C,), s + 1) if with_cls else None, pos=_rand((T, C), s + 2),
                gamma=1.0 + 0.5 * _rand((C,), s + 3) if with_ln else None, beta=0.5 * _rand((C,), s + 4) if with_ln else None,
                dy=_rand((B, T, C), s + 5).to(dtype))


def _formula(c, dtype):
    "(y, dtok, dcls, dpos, dgamma, dbeta) by PyTorch on the CPU in `dtype`, on the stored (already rounded) tok and dy"
    leaf = lambda t: None if t is None else t.detach().to(dtype, copy=True).requires_grad_(True)      # noqa: E731
    tok, cls, pos, gamma, beta = (leaf(c[k]) for k in ("tok", "cls", "pos", "gamma", "beta"))
    z = tok if cls is None else torch.cat([cls.view(1, 1, -1).expand(tok.shape[0], -1, -1), tok], 1)
    z = z + pos
    y = z if gamma is None else F.layer_norm(z, (z.shape[-1],), gamma, beta, EPS)
    y.backward(c["dy"].to(dtype))
    return (y.detach(),) + tuple(None if t is None else t.grad for t in (tok, cls, pos, gamma, beta))


def _run(c, gpu):
    from uniception_amd import ops
    d = {k: None if v is None else v.to(gpu) for k, v in c.items()}
    ln = None if d["gamma"] is None else (d["gamma"], d["beta"], EPS)
    y, stats = ops.vit_stem(d["tok"], d["cls"], d["pos"], ln, d["tok"].dtype, want_stats=True)
    grads = ops.vit_stem_bwd(d["dy"], d["tok"], d["cls"], d["pos"], d["gamma"], stats)
    again = ops.vit_stem_bwd(d["dy"], d["tok"], d["cls"], d["pos"], d["gamma"], stats)
    torch.cuda.synchronize()
    return y, stats, grads, again


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,hw,with_cls,C,with_ln", SHAPES)
def test_vit_stem_forward_and_backward_against_fp64(gpu, B, hw, with_cls, C, with_ln, dtype):
    from uniception_amd import ops
    c = _case(B, hw, with_cls, C, with_ln, dtype)
    want = _formula(c, torch.float64)
    own = _formula(c, dtype)
    y, stats, grads, again = _run(c, gpu)
    T = hw + int(with_cls)
    assert y.dtype == dtype and tuple(y.shape) == (B, T, C) and grads[0].dtype == dtype and tuple(grads[0].shape) == (B, hw, C)
    assert (stats is None) == (not with_ln)
    if with_ln:       # the statistics the backward reads are those of z
        z = _formula(dict(c, gamma=None, beta=None), torch.float64)[0]
        assert rel_l2(stats.view(B, T, 2)[..., 0].cpu(), z.mean(-1)) <= 1e-5
        assert rel_l2(stats.view(B, T, 2)[..., 1].cpu(), (z.var(-1, unbiased=False) + EPS).rsqrt()) <= 1e-5
    for a, b in zip(grads, again):                       # fixed-order sums: two calls, the same bits
        assert (a is None and b is None) or torch.equal(a, b)
    # the inference form (no statistics kept) is the same kernel: the same bits
    d = {k: None if v is None else v.to(gpu) for k, v in c.items()}
    assert torch.equal(ops.vit_stem(d["tok"], d["cls"], d["pos"], None if not with_ln else (d["gamma"], d["beta"], EPS), dtype), y)
    bad = []
    for name, got, w, o in zip(NAMES, (y,) + grads, want, own):
        assert (got is None) == (w is None), name
        if w is None:
            continue
        assert got.dtype == (dtype if name in ("y", "dtok") else torch.float32)
        e = rel_l2(o, w)
        bound = max(2e-6, 8.0 * e) if dtype == torch.float32 else 2.0 * e
        err = rel_l2(got.cpu(), w)
        print(f"vit_stem {dtype} (B {B}, hw {hw}, cls {with_cls}, C {C}, LN {with_ln}) {name}: rel-L2 {err:.3e} (torch's own {e:.3e}, bound {bound:.3e})")
        if not err <= bound:
            bad.append((name, err, bound))
    assert not bad, bad


def test_vit_stem_mixed_dtypes_and_the_function(gpu):
    "fp32 tokens into a bf16 stream (what the encoder does in bf16 mode), through autograd.vit_stem with module parameters"
    from uniception_amd import autograd
    B, hw, C = 2, 15, 128
    c = _case(B, hw, True, C, True, torch.float32)
    want = _formula(c, torch.float64)
    ln = torch.nn.LayerNorm(C, eps=EPS).to(gpu)
    with torch.no_grad():
        ln.weight.copy_(c["gamma"])
        ln.bias.copy_(c["beta"])
    tok = c["tok"].to(gpu).requires_grad_(True)
    cls, pos = c["cls"].to(gpu).requires_grad_(True), c["pos"].to(gpu).requires_grad_(True)
    y = autograd.vit_stem(tok, cls, pos, ln, torch.bfloat16)
    assert y.dtype == torch.bfloat16
    y.backward(c["dy"].to(gpu).bfloat16())
    torch.cuda.synchronize()
    assert rel_l2(y.detach().float().cpu(), want[0]) <= 2.0 * rel_l2(want[0].bfloat16(), want[0])           # one rounding of the output
    w64 = _formula(dict(c, dy=c["dy"].bfloat16().float()), torch.float64)
    for name, got, w in zip(NAMES[1:], (tok.grad, cls.grad, pos.grad, ln.weight.grad, ln.bias.grad), w64[1:]):
        assert got is not None and got.dtype == torch.float32 and rel_l2(got.cpu(), w) <= 1e-5, name
    with torch.no_grad():          # no graph: the plain kernel call, the same bits
        assert torch.equal(autograd.vit_stem(tok.detach(), cls.detach(), pos.detach(), ln, torch.bfloat16), y.detach())


def test_bad_arguments_are_refused_without_a_launch(gpu):
    from uniception_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    tok, y = torch.zeros(2, 15, 128, device=gpu), torch.full((2, 16, 128), 7.0, device=gpu)
    v = torch.zeros(16, 128, device=gpu)
    p = lambda t: t.data_ptr()      # noqa: E731
    assert lib.uc_vit_stem(p(tok), 0, p(v), p(v), p(v), p(v), EPS, p(y), 0, None, 2, 15, 12, st) == -1
    assert "C=12 must be a multiple of 8" in lib.uc_last_error().decode()
    assert lib.uc_vit_stem(p(tok), 0, p(v), p(v), p(v), p(v), EPS, None, 0, None, 2, 15, 128, st) == -1
    assert "null pointer" in lib.uc_last_error().decode()
    assert lib.uc_vit_stem_bwd(p(y), 0, p(tok), 0, p(v), p(v), p(v), p(v), p(tok), p(v), p(v), p(v), p(v), p(y), 2, 15, 12, st) == -1
    assert lib.uc_vit_stem_bwd(p(y), 0, p(tok), 0, p(v), p(v), p(v), p(v), p(tok), p(v), p(v), p(v), p(v), None, 2, 15, 128, st) == -1
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(tok.abs().max()) == 0.0 and float(v.abs().max()) == 0.0      # nothing was written
