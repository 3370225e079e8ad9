"""DINOv3 ViT encoder on the HIP kernels: uc_rope_axial per element against an fp64 evaluation that reads the same fp32 tables, and the
encoder / intermediate-feature returner against goldens of an INDEPENDENT implementation of the published network (transformers'
DINOv3ViTModel: tests/golden/dinov3_hf.npz, make_golden_dinov3_hf.py) — outputs in fp32 and bf16 mode, parameter gradients against
transformers' autograd, the gradient-checkpointed backward, the train-mode coordinate augmentation.  The golden weights are loaded
through uniception_amd.tools.convert_checkpoint (--mode dinov3).  PARITY UNPINNED against the hub code, which is not available.

Per-element bound of the kernel test.  The kernel reads u, v exactly, takes (c, s) exactly from the table and evaluates u c - v s
(or v c + u s) in fp32: at most three roundings (two products, one sum; fewer where the compiler contracts to an fma), each relative
2^-24 of a quantity bounded by |u c| + |v s| — so |fp32 result - exact| <= 3 * 2^-24 * (|u c| + |v s|).  Storing rounds to nearest in
the output format: another half ulp AT the stored value, ulp = 2^(floor(log2 |x|) - 7) for bf16 and 2^(floor(log2 |x|) - 10) for f16
(nothing for f32).  Relative to |x| that half ulp lies between 2^-9 and 2^-8 for bf16 (2^-12 and 2^-11 for f16): the flat "2^-9 |x|"
is the best case, which a correctly rounded store of e.g. 1.004 (half ulp 2^-8) exceeds, so the test uses the half ulp itself, taken at
|reference| + the arithmetic bound (the stored value may sit one binade above the reference).  No element is skipped or sampled.
Inverse after forward: the error of the first pass is carried through the second rotation, |c| E(u') + |s| E(v'), and the second
pass adds its own bound on what it reads — the sum of the two passes' bounds ("twice"), against the fp64 evaluation of both passes
(which carries c^2 + s^2 != 1 of the fp32 table entries exactly)."""
import os

import numpy as np
import pytest
import torch

from tests.dinov3_formulas import rope_axial_model
from tests.golden.cases import sample_indices
from tests.golden.dinov3_cases import (DINOV3_HF_CASES, DINOV3_HF_GRAD_CASES, HEADS, HIDDEN, dinov3_grad_weights, dinov3_hf_state_dict,
                                       dinov3_image, dinov3_size)
from tests.helpers import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu

# (B, prefix, grid_h, grid_w, H, D): 33 tokens — not a multiple of the workgroup's 8 — with a prefix; no prefix, D = 32; one patch token
KERNEL_SHAPES = [(3, 5, 2, 3, 2, 64), (2, 0, 3, 2, 3, 32), (1, 1, 1, 1, 1, 64)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
EPS32 = 2.0 ** -24


def half_ulp(x, dtype):
    "half a unit in the last place of `dtype` at magnitude x (fp64 tensor); 0 for fp32 — the fp32 roundings are the arithmetic bound"
    if dtype == torch.float32:
        return torch.zeros_like(x)
    bits, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(x.abs().clamp_min(2.0 ** emin).cpu())[1].double() - 1     # floor(log2 x) exactly, clamped to the smallest normal
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - bits - 1).to(x.device)


def element_bound(ref, mag, dtype):
    arith = 3 * EPS32 * mag
    return arith + half_ulp(ref.abs() + arith, dtype)


def tables(gh, gw, D, gpu, seed):
    "fp32 (cos, sin) tables of arbitrary angles (the kernel does not care where they come from), unit length to fp32 rounding"
    g = torch.Generator().manual_seed(seed)
    ay, ax = torch.rand(gh, D // 4, generator=g) * 6.28, torch.rand(gw, D // 4, generator=g) * 6.28
    return (torch.stack([ay.cos(), ay.sin()], -1).contiguous().to(gpu), torch.stack([ax.cos(), ax.sin()], -1).contiguous().to(gpu))


def check_pass(got, x64, ty, tx, prefix, gh, gw, dtype, what):
    "one forward pass of the kernel, every element, against fp64; returns (fp64 reference, per-element bound)"
    ref, mag = rope_axial_model(x64, ty, tx, prefix, gh, gw, with_bound=True)
    bound = element_bound(ref, mag, dtype)
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300))[:, prefix:].max()) if got[:, prefix:].numel() else 0.0
    print(f"\n[uc_rope_axial {what}] max error / bound {worst:.3f}, max abs error {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (what, worst)
    return ref, bound


@pytest.mark.parametrize("layout", ["contiguous", "packed_qkv", "offset_scalar"])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rope_axial_kernel_per_element_against_fp64(gpu, shape, dt, layout):
    from uniception_amd import ops
    B, prefix, gh, gw, H, D = shape
    dtype, N = DTYPES[dt], prefix + gh * gw
    ty, tx = tables(gh, gw, D, gpu, 11 + D)
    g = torch.Generator().manual_seed(B * 100 + N)
    if layout == "packed_qkv":                 # q | k rotated in ONE launch on the views of a packed projection; V must not change
        buf = torch.randn(B, N, 3, H, D, generator=g).to(dtype).to(gpu)
        before = buf.clone()
        q, k = buf[:, :, 0], buf[:, :, 1]
        ops.rope_axial_(q, k, ty, tx, prefix, gh, gw)
        torch.cuda.synchronize()
        assert torch.equal(buf[:, :, 2], before[:, :, 2]), "the V slice changed"
        views, inputs = (q, k), (before[:, :, 0], before[:, :, 1])
    else:
        flat = torch.randn(B * N * H * D + 2, generator=g).to(dtype).to(gpu)
        off = 2 if layout == "offset_scalar" else 0          # 2 elements off a 16-byte boundary: the element-access kernel
        before = flat.clone()
        t = flat[off:off + B * N * H * D].view(B, N, H, D)
        assert (t.data_ptr() % 16 != 0) == (layout == "offset_scalar")
        ops.rope_axial_(t, None, ty, tx, prefix, gh, gw)
        torch.cuda.synchronize()
        assert torch.equal(flat[:off], before[:off]) and torch.equal(flat[off + t.numel():], before[off + t.numel():]), "wrote outside the view"
        views, inputs = (t,), (before[off:off + t.numel()].view(B, N, H, D),)
    fwd = []
    for i, (v, x) in enumerate(zip(views, inputs)):
        assert torch.equal(v[:, :prefix], x[:, :prefix]), "a prefix row changed"                     # bit-identical
        fwd.append(check_pass(v, x.double(), ty, tx, prefix, gh, gw, dtype, f"{shape} {dt} {layout} operand {i}"))
    # inverse after forward
    stored = [v.clone() for v in views]
    ops.rope_axial_(views[0], views[1] if len(views) == 2 else None, ty, tx, prefix, gh, gw, inverse=True)
    torch.cuda.synchronize()
    Q = D // 4
    for v, x, s, (ref1, b1) in zip(views, inputs, stored, fwd):
        assert torch.equal(v[:, :prefix], x[:, :prefix])
        # fp64 of both passes, and the first pass's bound carried through the second rotation
        ref2, mag2 = rope_axial_model(ref1, ty, tx, prefix, gh, gw, inverse=True, with_bound=True)
        p = torch.arange(N - prefix, device=gpu)
        c = torch.cat([ty[p // gw, :, 0], tx[p % gw, :, 0]], -1).double().abs()[None, :, None, :]
        sn = torch.cat([ty[p // gw, :, 1], tx[p % gw, :, 1]], -1).double().abs()[None, :, None, :]
        carried = torch.zeros_like(b1)
        bu, bv = b1[:, prefix:, :, :2 * Q], b1[:, prefix:, :, 2 * Q:]
        carried[:, prefix:, :, :2 * Q] = c * bu + sn * bv
        carried[:, prefix:, :, 2 * Q:] = c * bv + sn * bu
        # the second pass's own bound, on what it actually read (the stored first-pass values)
        _, mag_read = rope_axial_model(s.double(), ty, tx, prefix, gh, gw, inverse=True, with_bound=True)
        bound = carried + element_bound(ref2.abs() + carried, mag_read, dtype)
        err = (v.double() - ref2).abs()
        assert bool((err <= bound).all()), (shape, dt, layout, float((err / bound.clamp_min(1e-300)).max()))
        # ... and that is the input again, to the unit-length error of the fp32 table entries
        assert float((ref2 - x.double()).abs().max()) <= 8 * EPS32 * float(x.double().abs().max()) + 1e-30


def test_rope_axial_separate_operands_and_empty_problems(gpu):
    from uniception_amd import ops
    ty, tx = tables(2, 3, 64, gpu, 3)
    g = torch.Generator().manual_seed(9)
    q, k = torch.randn(2, 11, 2, 64, generator=g).to(gpu), torch.randn(2, 11, 2, 64, generator=g).to(gpu)      # two allocations: two launches
    q0, k0 = q.clone(), k.clone()
    ops.rope_axial_(q, k, ty, tx, 5, 2, 3)
    for t, x in ((q, q0), (k, k0)):
        check_pass(t, x.double(), ty, tx, 5, 2, 3, torch.float32, "separate operands")
    e = torch.empty(0, 11, 2, 64, device=gpu)
    ops.rope_axial_(e, None, ty, tx, 5, 2, 3)                                      # B = 0: UC_OK, nothing launched
    torch.cuda.synchronize()


def test_rope_axial_refuses_bad_arguments_before_any_launch(gpu):
    from uniception_amd import _lib, ops
    lib = _lib.load()
    ty, tx = tables(2, 3, 64, gpu, 3)
    t = torch.randn(2, 11, 2, 64).to(gpu)
    keep = t.clone()

    def call(D=64, N=11, parts=1, prefix=5, gh=2, gw=3, y=ty.data_ptr(), x=tx.data_ptr(), dtype=_lib.UC_F32, H=2):
        return lib.uc_rope_axial(t.data_ptr(), 2, N, H, D, N * H * D, H * D, D, parts, 0, prefix, gh, gw, y, x, 0, dtype,
                                 torch.cuda.current_stream().cuda_stream)

    for kw, text in ((dict(D=60), b"multiple of 8"), (dict(D=2048), b"too large"), (dict(N=12), b"prefix + grid_h * grid_w"),
                     (dict(prefix=4), b"prefix + grid_h * grid_w"), (dict(y=None), b"null table"), (dict(x=None), b"null table"),
                     (dict(parts=3), b"parts must be 1 or 2"), (dict(dtype=7), b"unsupported dtype"), (dict(H=-1), b"negative dimension")):
        assert call(**kw) != 0, kw
        assert text in lib.uc_last_error(), (kw, lib.uc_last_error())
    torch.cuda.synchronize()
    assert torch.equal(t, keep)                       # nothing ran
    with pytest.raises(ops.UcHipError, match=r"fp32 \[2, 16, 2\]"):
        ops.rope_axial_(t, None, ty.half(), tx, 5, 2, 3)
    with pytest.raises(ops.UcHipError, match="uc_rope_axial failed"):
        ops.rope_axial_(t, None, ty, tx, 4, 2, 3)
    assert call() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the encoder against transformers' DINOv3ViTModel
# ---------------------------------------------------------------------------------------------------------------------------------
# Tolerances: the ones DINOV2_HF_CASES uses for the same modes in tests/test_dinov2_gpu.py (test_matches_huggingface_transformers_golden:
# fp32 1e-3, bf16 3e-2 rel-L2; test_gradients_match_huggingface_transformers_autograd: fp32 rel-L2 < 1e-3 per parameter on samples and
# norm and the loss within 1e-4, bf16 cosine over all sampled gradients > 0.999) — the same kind of network pinned to the same package.
MODES = [("fp32", 1e-3), ("bf16", 3e-2)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "dinov3_hf.npz"))


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    "case name -> the {'model': ...} file the converter writes from the transformers-named golden weights"
    from uniception_amd.tools import convert_checkpoint as cc
    d = tmp_path_factory.mktemp("dinov3")
    out = {}
    for name, c in DINOV3_HF_CASES.items():
        src, dst = d / f"{name}_hf.pth", d / f"{name}.pth"
        torch.save(dinov3_hf_state_dict(c), src)
        cc.main([str(src), str(dst), "--mode", "dinov3", "--num-heads", str(HEADS)])
        out[name] = str(dst)
    return out


def build(name, checkpoints, returner=False, **kw):
    from uniception_amd.models.encoders import encoder_factory, feature_returner_encoder_factory
    make = feature_returner_encoder_factory if returner else encoder_factory
    return make("dinov3", name="d3", dinov3_repo_dir=None, size=dinov3_size(DINOV3_HF_CASES[name]),
                pretrained_checkpoint_path=checkpoints[name], **kw)


def run(enc, name, gpu):
    from uniception_amd.models.encoders.base import ViTEncoderInput
    return enc(ViTEncoderInput(image=dinov3_image(DINOV3_HF_CASES[name]).to(gpu), data_norm_type="dinov3"))


@pytest.mark.parametrize("name", list(DINOV3_HF_CASES))
@pytest.mark.parametrize("mode,tol", MODES)
def test_encoder_matches_huggingface_transformers_golden(gpu, gold, checkpoints, name, mode, tol):
    from uniception_amd import engine
    enc = build(name, checkpoints).eval().to(gpu)
    with torch.no_grad(), engine.precision(mode):
        out = run(enc, name, gpu)
    want = gold[f"{name}/features"]
    assert out.registers is None and tuple(out.features.shape) == want.shape and out.features.dtype == torch.float32
    e = rel_l2(out.features.cpu(), want)
    print(f"\n[dinov3 {mode} vs transformers {gold['transformers_version']}] {name}: features {e:.2e}")
    assert e < tol


@pytest.mark.parametrize("name", ["mlp_48x32", "gated_32x48"])
@pytest.mark.parametrize("mode,tol", MODES)
@pytest.mark.parametrize("indices,norm", [(2, True), (2, False), ([0, 1], True), ([0, 1], False), (1, True)])
def test_returner_matches_huggingface_transformers_golden(gpu, gold, checkpoints, name, mode, tol, indices, norm):
    from uniception_amd import engine
    enc = build(name, checkpoints, returner=True, indices=indices, norm_intermediate=norm).eval().to(gpu)
    with torch.no_grad(), engine.precision(mode):
        outs = run(enc, name, gpu)
    layers = [0, 1] if indices != 1 else [1]
    assert len(outs) == len(layers)
    for o, i in zip(outs, layers):
        want = gold[f"{name}/take{i}_{'norm' if norm else 'raw'}"]
        assert tuple(o.features.shape) == want.shape and o.registers is None
        e = rel_l2(o.features.float().cpu(), want)
        assert e < tol, (i, e)
    if norm and 1 in layers:       # the last block through the final norm is the encoder's own output
        assert rel_l2(outs[-1].features.float().cpu(), gold[f"{name}/features"]) < tol


def grads_of(enc, name, gpu, mode):
    from uniception_amd import engine
    enc.zero_grad(set_to_none=True)
    with engine.precision(mode):
        out = run(enc, name, gpu)
        loss = (out.features * dinov3_grad_weights(name, out.features.shape).to(gpu)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return out.features.detach(), loss.detach(), {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name", DINOV3_HF_GRAD_CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gradients_match_huggingface_transformers_autograd(gpu, gold, checkpoints, name, mode):
    """Gradients of <patch map, Wf> with respect to every parameter (patch embedding, cls / storage tokens, LayerScale gammas, all
    block weights — the q | v bias through the K mask —, final norm) against transformers' autograd on the same weights, with the
    position augmentation off (pos_embed_rescale=None), under the DINOv2 gradient test's criteria."""
    enc = build(name, checkpoints, pos_embed_rescale=None).train().to(gpu)
    _, loss, grads = grads_of(enc, name, gpu, mode)
    want_loss = float(gold[f"{name}/loss"])
    if mode == "fp32":
        assert abs(float(loss) - want_loss) <= 1e-4 * max(1.0, abs(want_loss)), (float(loss), want_loss)
    got_all, ref_all, worst, n = [], [], ("", 0.0), 0
    for k, p in enc.named_parameters():
        if k == "model.mask_token":              # kept so checkpoints load; no forward reads it
            assert p.grad is None
            continue
        key = f"{name}/grad/{k}__samples"
        assert key in gold.files, k
        assert k in grads, k
        idx = torch.from_numpy(sample_indices(p.numel(), 512)).to(gpu)
        got = grads[k].flatten()[idx].double().cpu()
        ref = torch.from_numpy(gold[key]).double()
        want_n, got_n = float(gold[f"{name}/grad/{k}__norm"]), float(grads[k].double().norm())
        e = max(rel_l2(got, ref), abs(got_n - want_n) / max(want_n, 1e-30))
        if e > worst[1]:
            worst = (k, e)
        got_all.append(got)
        ref_all.append(ref)
        n += 1
    got_all, ref_all = torch.cat(got_all), torch.cat(ref_all)
    cos = float(torch.dot(got_all, ref_all) / (got_all.norm() * ref_all.norm()))
    print(f"\n[dinov3 {mode} grads vs transformers autograd] {name}: {n} parameters, worst {worst[0]} {worst[1]:.2e}, cosine {cos:.6f}")
    assert n == sum(1 for f in gold.files if f.startswith(f"{name}/grad/") and f.endswith("__samples"))
    D = HIDDEN
    assert not grads["model.blocks.0.attn.qkv.bias"][D:2 * D].any()          # the masked K bias receives exactly nothing
    if mode == "fp32":
        assert worst[1] < 1e-3, worst
    else:
        assert cos > 0.999, cos


@pytest.mark.parametrize("name", DINOV3_HF_GRAD_CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_checkpointed_backward_equals_plain(gpu, checkpoints, name, mode):
    "the existing wrapper re-computes a block with the SAME bound RoPE tables — under augmentation too (one draw per forward, outside the blocks)"
    for kw, seed in ((dict(pos_embed_rescale=None), None), (dict(pos_embed_rescale=2.0, pos_embed_shift=0.2), 21)):
        res = []
        for ckpt in (False, True):
            enc = build(name, checkpoints, gradient_checkpointing=ckpt, **kw).train().to(gpu)
            assert (type(enc.model.blocks[0]).__name__ == "Checkpointed_Block") == ckpt
            if seed is not None:
                torch.manual_seed(seed)
            res.append(grads_of(enc, name, gpu, mode))
        (f0, l0, g0), (f1, l1, g1) = res
        assert torch.equal(f0, f1) and set(g0) == set(g1)
        for k in g0:      # (the criterion of tests/test_checkpointing_gpu.py)
            assert rel_l2(g1[k].double().cpu(), g0[k].double().cpu()) < 1e-5, (k, kw)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_train_mode_augmentation_changes_the_output(gpu, checkpoints, mode):
    from uniception_amd import engine
    name = "mlp_32x48"
    enc = build(name, checkpoints, pos_embed_rescale=2.0).to(gpu)
    with torch.no_grad(), engine.precision(mode):
        ev = run(enc.eval(), name, gpu).features.clone()
        torch.manual_seed(4)
        tr = run(enc.train(), name, gpu).features.clone()          # train mode without gradients: the inference kernels, augmented tables
        ev2 = run(enc.eval(), name, gpu).features
    assert torch.isfinite(tr).all() and torch.equal(ev, ev2)
    assert rel_l2(tr.cpu(), ev.cpu()) > 1e-3
    torch.manual_seed(4)
    _, _, g = grads_of(enc.train(), name, gpu, mode)               # ... and with gradients: the training Functions
    assert all(torch.isfinite(v).all() for v in g.values()) and len(g) > 30


def test_large_at_224_returns_a_14x14_map(gpu):
    from uniception_amd import engine
    from uniception_amd.models.encoders import encoder_factory
    from uniception_amd.models.encoders.base import ViTEncoderInput
    torch.manual_seed(0)
    enc = encoder_factory("dinov3", name="d3l", dinov3_repo_dir=None, size="large", keep_first_n_layers=2).eval().to(gpu)
    img = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(gpu)
    with torch.no_grad(), engine.precision("bf16"):
        out = enc(ViTEncoderInput(image=img, data_norm_type="dinov3"))
    assert tuple(out.features.shape) == (2, 1024, 14, 14) and torch.isfinite(out.features).all()
