"""Training path of the DUSt3R hot path: ``torch.autograd.Function``s whose forward AND backward are the HIP kernels.

The reference trains through PyTorch autograd over its modules (it ships no hand-written backward); here autograd only
wires the graph (residual stream, the Jacobi update between the two views, the view ops at the BCHW boundary) while every
sub-layer's backward is one Function calling uc_hip entry points:

    pre-LN sub-layer  x_out = x + f(LN(x)):   backward gets d(x_out) and returns
        dx = LN_bwd(x, gamma, df/dh) + d(x_out)              (residual add fused into uc_layernorm_bwd)
    linear y = h W^T + b:
        dW = dy^T h   -> uc_gemm_tn (both operands row-major, transposing LDS reads, as many split-K slabs as the library
                         recommends for the shape, + uc_splitk_reduce —
                         straight into the flat gradient buffer under the Trainer); fp32 mode: uc_transpose2d + fp32 uc_gemm
        db = column sums of dy formed inside uc_gemm_tn; dh = uc_gemm(dy, W^T)   (W^T prepared once per weight version)
    attention: uc_attention_fwd saves LSE; uc_attention_bwd recomputes P tile by tile (dQ kernel + dK/dV kernel)
    RoPE: gradients of the rotated q/k are rotated back in place with the inverse angle (curope2d.py:24-28)

Precision follows the forward: bf16 operands with fp32 accumulation, fp32 residual stream, fp32 weight gradients; in
fp32 verification mode every kernel is the exact-fp32 variant.
"""
import weakref
from typing import Optional

import torch
import torch.nn as nn
from torch.autograd import Function

from . import engine, ops
from ._lib import UcHipError

KPAD = 64  # the weight-gradient GEMMs reduce over tokens: pad that axis to the direct-to-LDS kernel's K granule


def grad_needed(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _c(g: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if g is None else (g if g.is_contiguous() else g.contiguous())


def _tp(x2d: torch.Tensor, dt: torch.dtype, with_copy: bool = False):
    return ops.transpose2d(x2d, dt, pad_to=KPAD, with_copy=with_copy)


def _split_k_x3(I: int, J: int, T: int, dt) -> int:
    """split_k of an fp32 weight-gradient GEMM on the split-operand (bf16x3) route: its output is a few 128 x 128 tiles and its
    reduction runs over every token / pixel (x3) — unsplit, the fp32-class heads' 3x3 weight gradients ran on 9 CUs for 44 ms.
    1 on the exact-fp32 route (the verification kernel has no split form)."""
    if dt != torch.float32 or ops.fp32_matmul_hook() != "bf16x3":
        return 1
    tiles = ((I + 127) // 128) * ((J + 127) // 128)
    return max(1, min(T // 1024, 256 // max(tiles, 1), 64))


def _tn_ok(*ts) -> bool:
    return all(t.dtype == torch.bfloat16 and t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and t.shape[-1] % 8 == 0
               and (t.dim() != 2 or t.stride(0) % 8 == 0) for t in ts)


def _reduce_slabs(ws: torch.Tensor) -> torch.Tensor:
    return ws[0] if ws.shape[0] == 1 else ops.splitk_reduce(ws)


# Gradient sink (switched on by training.Trainer): weight gradients that come out of the TN kernel as split-K slabs are
# reduced STRAIGHT INTO the parameter's existing .grad (a view of the flat gradient buffer) — the reduction kernel does
# autograd's accumulation and the Function returns None for that input.  The parameter's AccumulateGrad node still runs
# once all of its contributions are in (with an undefined gradient) and fires its post-accumulate hooks, so the bucket
# bookkeeping of the trainer needs no extra signal; should a PyTorch build skip the hook for undefined gradients, the
# trainer's finish() reduces the buckets that never completed.
_grad_sink = False
# Two-stream training with SHARED parameters (the encoder's two views on two streams, engine.run_branches(shared_params=True)): the
# sink's reduction is a plain read-modify-write of the parameter's gradient slice, and two streams doing that concurrently would race.
# Functions whose forward ran inside the forked (second) branch therefore return their weight gradients as tensors — autograd's
# AccumulateGrad adds them on the stream the parameter was first used on, behind the first branch's sink writes.  `_sink_fwd_ok` is what
# a Function records at forward time (ctx._uc_sink_ok, see _sink_aware); `_grad_sink_gate` is that record during its backward.
_sink_fwd_ok = [True]
_grad_sink_gate = True


def set_grad_sink(enabled) -> None:
    global _grad_sink
    _grad_sink = bool(enabled)


def _sink_aware(cls):
    "Class decorator of the autograd Functions below: remember at forward time whether this node may sink, apply it in backward."
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *args, **kw):
        ctx._uc_sink_ok = _sink_fwd_ok[0]
        # how fp32-operand GEMMs ran in this forward (exact VALU kernel / split-operand bf16x3 MFMA: engine._fp32_matmul).  The backward
        # is called by the autograd engine OUTSIDE the caller's engine.precision(...) scope, where the policy would read "exact": the
        # fp32-class heads' training step ran 86 % of its time in gemm_f32_kernel (round 6, 14x the bf16-head step) — the backward now
        # runs its fp32 GEMMs the way the forward did
        ctx._uc_mm = ops.fp32_matmul_hook()
        return fwd(ctx, *args, **kw)

    def backward(ctx, *grads):
        global _grad_sink_gate
        prev = _grad_sink_gate
        _grad_sink_gate = getattr(ctx, "_uc_sink_ok", True)
        prev_mm, engine._mm_override = engine._mm_override, getattr(ctx, "_uc_mm", None)
        try:
            return bwd(ctx, *grads)
        finally:
            _grad_sink_gate = prev
            engine._mm_override = prev_mm
    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return cls


def _sinkable(param, rows: int, cols: int) -> bool:
    g = param.grad if param.is_leaf else None      # (rows gathered from a parameter — the Perception Encoder's in_proj — own no buffer)
    return (_grad_sink and _grad_sink_gate and g is not None and g.dtype == torch.float32 and g.is_contiguous()
            and g.numel() == rows * cols and param.requires_grad)


def _ln_grad_targets(ln, g):
    """(dgamma buffer, dbeta buffer, sunk): with the gradient sink on, uc_layernorm_bwd adds (atomically, per block) STRAIGHT INTO the
    LayerNorm parameters' own gradient buffers — views of the trainer's flat buffer — and the Function returns None for them: no zero
    fill, no autograd add kernel per LayerNorm (240 of each per training step of the ViT-L model); otherwise fresh zeroed buffers."""
    w, b = getattr(ln, "weight", None), getattr(ln, "bias", None)
    if w is not None and b is not None and _sinkable(w, w.numel(), 1) and _sinkable(b, b.numel(), 1):
        return w.grad.view(-1), b.grad.view(-1), True
    return torch.zeros_like(g), torch.zeros_like(g), False


def _bias_target(bias_sink, N: int):
    """One contiguous fp32 [N] view covering the gradient buffers of the bias parameter(s) of a linear (two adjacent ones
    for the fused K|V projection), or None when they cannot take direct accumulation."""
    if not _grad_sink or not _grad_sink_gate or not bias_sink or any(p is None or not _sinkable(p, p.numel(), 1) for p in bias_sink):
        return None
    g0 = bias_sink[0].grad
    total, ptr = 0, g0.data_ptr()
    for p in bias_sink:
        if p.grad.data_ptr() != ptr + 4 * total:
            return None          # not adjacent in the flat gradient buffer
        total += p.numel()
    if total != N:
        return None
    return g0.reshape(-1) if len(bias_sink) == 1 else torch.as_strided(g0, (N,), (1,))


def _wgrad(dy2d: torch.Tensor, x2d: torch.Tensor, dt: torch.dtype, bias: bool = False, sink=None, bias_sink=None):
    """(dW [N,K] fp32, db [N] fp32 | None) = (dy^T x, column sums of dy) for row-major dy [M,N], x [M,K].
    sink: optional list of (parameter, row0, row1) covering the rows of dW; when every target has a gradient buffer the
    slabs are reduced into those buffers and dW is returned as None (see _grad_sink).
    bf16: the TN kernel contracts over the slow axis directly (uc_gemm_tn: split-K slabs + uc_splitk_reduce) and forms the
    bias gradient from the dy fragments it already holds; fp32 verification mode: explicit transposes + the exact fp32
    GEMM + uc_colsum."""
    if dt == torch.bfloat16:
        a = dy2d if dy2d.dtype == dt else ops.convert(_c(dy2d), dt)
        b = x2d if x2d.dtype == dt else ops.convert(_c(x2d), dt)
        if _tn_ok(a, b):
            K = b.shape[1]
            bt = _bias_target(bias_sink, a.shape[1]) if bias else None
            if bt is not None:      # bias gradient added atomically into the bias's own gradient buffer: db is returned None
                ws, db = ops.gemm_tn(a, b, colsum_into=bt), None
            elif bias:
                ws, cs = ops.gemm_tn(a, b, colsum=True)
                db = _reduce_slabs(cs.unsqueeze(1)).reshape(-1)
            else:
                ws, db = ops.gemm_tn(a, b), None
            if sink is not None and all(_sinkable(p, r1 - r0, K) for p, r0, r1 in sink):
                for p, r0, r1 in sink:
                    ops.splitk_reduce(ws[:, r0:r1], out=p.grad.view(r1 - r0, K), accumulate=True)
                return None, db
            return _reduce_slabs(ws), db
    aT, bT = _tp(_c(dy2d), dt), _tp(_c(x2d), dt)
    sk = _split_k_x3(aT.shape[0], bT.shape[0], aT.shape[1], dt)
    dW = ops.gemm(aT, bT, out_dtype=torch.float32, split_k=sk)
    return (dW if sk <= 1 else _reduce_slabs(dW)), (_colsum(_c(dy2d)) if bias else None)


def _wgrad_conv(dz: torch.Tensor, x: torch.Tensor, stride: int, relu_in: bool, bias: bool = False):
    """(dW_gemm [Cout, 9*Cin] with K ordered (ky,kx,c), db | None) of a 3x3/pad-1 conv: dz NHWC [B,Ho,Wo,Cout], x NHWC."""
    Cout = dz.shape[-1]
    dz2 = dz.view(-1, Cout)
    if x.dtype == torch.bfloat16 and _tn_ok(dz2, x):
        if bias:
            ws, cs = ops.gemm_tn(dz2, x, conv=(stride, relu_in), colsum=True)
            return _reduce_slabs(ws), _reduce_slabs(cs.unsqueeze(1)).reshape(-1)
        return _reduce_slabs(ops.gemm_tn(dz2, x, conv=(stride, relu_in))), None
    aT, bT = _tp(dz2, x.dtype), ops.im2col_t(x, stride, relu_in, KPAD)
    sk = _split_k_x3(aT.shape[0], bT.shape[0], aT.shape[1], x.dtype)
    dW = ops.gemm(aT, bT, out_dtype=torch.float32, split_k=sk)
    return (dW if sk <= 1 else _reduce_slabs(dW)), (_colsum(dz2) if bias else None)


# bf16 twins of residual-stream gradients: uc_layernorm_bwd writes a bf16 copy of the dx it produces; the sub-layer that
# receives exactly that tensor as its d(x_out) (autograd hands it over untouched when x_out had a single consumer) takes
# the twin instead of running a conversion pass.  Keyed by storage address, validated by OBJECT IDENTITY through a weak
# reference (a recycled address can never alias a stale entry), a handful of entries at most.
_twins = {}


def _ln_bwd_residual(x2d, g, dh, eps, dg, db, dres, dt):
    if dres is not None and dres.dtype != x2d.dtype:
        dres = ops.convert(dres, x2d.dtype)
    if dt != torch.bfloat16 or x2d.dtype == torch.bfloat16:      # (a bf16 stream's dx IS the bf16 operand of the next backward GEMMs)
        return ops.layernorm_bwd(x2d, g, dh, eps, dg, db, dres=dres)
    dx, twin = ops.layernorm_bwd(x2d, g, dh, eps, dg, db, dres=dres, bf16_twin=True)
    if len(_twins) > 8:
        _twins.clear()
    _twins[dx.data_ptr()] = (weakref.ref(dx), dx._version, twin)
    return dx


def _as_dt(g: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    if g.dtype == dt:
        return g
    hit = _twins.pop(g.data_ptr(), None)
    if hit is not None and dt == torch.bfloat16 and hit[0]() is g and hit[1] == g._version:
        return hit[2]
    return ops.convert(g, dt)


def _colsum(src2d: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(src2d.shape[1], dtype=torch.float32, device=src2d.device)
    ops.colsum_(src2d, out)
    return out


def _w_t(owner, tag, weight2d_sources, build_2d, dt):
    """W^T [K,N] in dt of a [N,K] fp32 weight, cached per weight version."""
    return engine.prepared(owner, (tag, "T", dt), weight2d_sources, lambda: ops.transpose2d(build_2d(), dt))


def lin_weight_t(lin, dt):
    return _w_t(lin, "lin", (lin.weight,), lambda: lin.weight.detach().float().reshape(lin.weight.shape[0], -1).contiguous(), dt)


def kv_weight_t(projk, projv, dt):
    return _w_t(projk, "kv", (projk.weight, projv.weight),
                lambda: torch.cat([projk.weight.detach(), projv.weight.detach()], 0).float().contiguous(), dt)


def _check_rope(rope):
    if rope is not None and not engine.is_native_rope(rope) and not engine.is_axial_rope(rope):
        raise UcHipError("training through a foreign positional-encoding callable is not supported; use RoPE2D / cuRoPE2D")


def _rope_inverse_(t4, pos, rope):
    if rope is not None:
        ops.rope_2d_(t4, pos.contiguous(), rope.base, -rope.F0)


def _rope_forward_(q4, k4, qpos, kpos, rope):
    "the positional encoding of q / k as a pass of its own, in place: the axial RoPE's one launch over q | k, or two uc_rope2d passes"
    if engine.is_axial_rope(rope):
        rope.rotate_(q4, k4)
    else:
        ops.rope_2d_(q4, qpos.contiguous(), rope.base, rope.F0)
        ops.rope_2d_(k4, kpos.contiguous(), rope.base, rope.F0)


def _bwd_rope(rope, qpos, kpos, dt):
    "rope argument of ops.attention_bwd when the inverse rotation can ride in the bf16 backward kernels, else None."
    if rope is None or engine.is_axial_rope(rope) or dt != torch.bfloat16 or qpos is None or kpos is None or qpos.numel() == 0:
        return None
    return (engine._pos2d(qpos), engine._pos2d(kpos), rope.base, rope.F0)


class Drops:
    """The dropout masks of ONE sub-layer call in training (uint8, 1 = keep; made by make_drops from PyTorch's generator, which owns the
    RNG state): `out` = nn.Dropout on the sub-layer's output (proj_drop / the Mlp's drop2), `path` = DropPath on the sub-layer's branch
    (one byte per sample), `mid` = the Mlp's drop1 on the hidden activation.  attn_drop (dropout of the attention probabilities inside
    the flash kernels) is not supported."""
    __slots__ = ("out", "out_scale", "path", "path_rows", "path_scale", "mid", "mid_scale")

    def __init__(self):
        self.out = self.path = self.mid = None
        self.out_scale = self.path_scale = self.mid_scale = 1.0
        self.path_rows = 0

    @property
    def has_out(self):
        return self.out is not None or self.path is not None


def make_drops(training: bool, device, B: int, N: int, C: int, p_out: float = 0.0, p_path: float = 0.0, hidden: int = 0,
               p_mid: float = 0.0, scale_by_keep: bool = True):
    """Drops for one sub-layer over [B * N, C] tokens, or None (eval mode / every rate 0).  Semantics: nn.Dropout (keep with
    probability 1 - p, scale 1 / (1 - p)); timm's DropPath (per sample, scale 1 / keep when scale_by_keep)."""
    if not training or (p_out <= 0.0 and p_path <= 0.0 and p_mid <= 0.0):
        return None
    d = Drops()
    if p_out > 0.0:
        d.out = torch.empty((B * N, C), dtype=torch.uint8, device=device).bernoulli_(1.0 - p_out)
        d.out_scale = 1.0 / (1.0 - p_out) if p_out < 1.0 else 0.0
    if p_path > 0.0:
        keep = 1.0 - p_path
        d.path = torch.empty((B,), dtype=torch.uint8, device=device).bernoulli_(keep)
        d.path_rows = N
        d.path_scale = 1.0 / keep if (scale_by_keep and keep > 0.0) else 1.0
    if p_mid > 0.0:
        d.mid = torch.empty((B * N, hidden), dtype=torch.uint8, device=device).bernoulli_(1.0 - p_mid)
        d.mid_scale = 1.0 / (1.0 - p_mid) if p_mid < 1.0 else 0.0
    return d


def _drops_saved(drops):
    """(mask tensors, spec) of a call's Drops: the masks go through ctx.save_for_backward — visible to checkpoint's saved-tensor hooks
    (dropped with the other activations of a checkpointed block and re-drawn from the restored generator state) and covered by
    autograd's version check; ctx.meta keeps only the scales."""
    if drops is None:
        return (), None
    masks = tuple(m for m in (drops.out, drops.path, drops.mid) if m is not None)
    return masks, (drops.out is not None, drops.out_scale, drops.path is not None, drops.path_rows, drops.path_scale,
                   drops.mid is not None, drops.mid_scale)


def _drops_restore(spec, saved):
    "(Drops or None, the saved tensors without the trailing masks): inverse of _drops_saved in a backward."
    if spec is None:
        return None, tuple(saved)
    n = int(spec[0]) + int(spec[2]) + int(spec[5])
    masks, saved = list(saved[len(saved) - n:]), tuple(saved[:len(saved) - n])
    d = Drops()
    if spec[0]:
        d.out, d.out_scale = masks.pop(0), spec[1]
    if spec[2]:
        d.path, d.path_rows, d.path_scale = masks.pop(0), spec[3], spec[4]
    if spec[5]:
        d.mid, d.mid_scale = masks.pop(0), spec[6]
    return d, saved


def _drop_out(f2d, drops, residual=None, out_dtype=None):
    "residual + dropout(f) (+ DropPath): the output masks of `drops`, the residual add riding in the last pass."
    steps = [(m, r, sc) for m, r, sc in ((drops.out, 0, drops.out_scale), (drops.path, drops.path_rows, drops.path_scale)) if m is not None]
    for i, (m, r, sc) in enumerate(steps):
        last = i == len(steps) - 1
        f2d = ops.mask_scale(f2d, m, r, sc, residual if last else None, out_dtype if last else None)
    return f2d


def _norm_or_none(norm):
    return None if norm is None or isinstance(norm, nn.Identity) else norm


def _qknorm_bwd(view4, norm, dn):
    "(d view4 [contiguous], dgamma, dbeta) of engine.qk_layernorm: uc_layernorm_bwd over B N H rows of head_dim (its 64-wide kernel)."
    pre = view4.contiguous()
    Dh = pre.shape[-1]
    g = norm.weight.detach().float()
    dg, db = torch.zeros_like(g), torch.zeros_like(g)
    dpre = ops.layernorm_bwd(pre.view(-1, Dh), g, dn.contiguous().view(-1, Dh), norm.eps, dg, db)
    return dpre.view(pre.shape), dg, db


def _attention_fwd(q, k, v, scale, lse, dropout=None):
    ops.attention_served(q.dtype, q.shape[-1], dropout=dropout is not None)
    if q.dtype == torch.bfloat16:
        return ops.attention(q, k, ops.vt_pack(v), scale, v_packed=True, lse=lse, dropout=dropout)
    return ops.attention(q, k, v, scale, lse=lse, dropout=dropout)


def attn_dropout(training: bool, p: float):
    """(p, seed) for a sub-layer's attention dropout, or None (eval mode / rate 0).  The seed comes from PyTorch's CPU generator —
    torch.manual_seed reproduces it, and a checkpointed block's re-computation draws the same one (preserve_rng_state) — and keys the
    counter-based mask the forward and backward kernels evaluate (uc_attention_fwd's drop_p / seed)."""
    if not training or p <= 0.0:
        return None
    if p >= 1.0:
        raise UcHipError("attn_drop must be below 1")
    return (float(p), int(torch.randint(0, 2 ** 62, (1,)).item()))


# =================================================================================================================
# LayerNorm alone (encoder / decoder final norms, intermediate norms)
# =================================================================================================================
@_sink_aware
class LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x2d, weight, bias, eps, out_dtype):
        x2d = _c(x2d)
        if x2d.dtype not in (torch.float32, torch.bfloat16):
            raise UcHipError("the training residual stream is fp32 or bf16")
        g, b = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        ctx.save_for_backward(x2d, g)
        ctx.eps = eps
        return ops.layernorm(x2d, g, b, eps, out_dtype)

    @staticmethod
    def backward(ctx, dy):
        x2d, g = ctx.saved_tensors
        dy = _c(dy)
        dg, db = torch.zeros_like(g), torch.zeros_like(g)
        dx = ops.layernorm_bwd(x2d, g, dy, ctx.eps, dg, db)
        return dx, dg, db, None, None


def layer_norm(x2d, ln, out_dtype):
    return LayerNormFn.apply(x2d, ln.weight, ln.bias, ln.eps, out_dtype)


# =================================================================================================================
# Linear (proj_embed, the linear head's 1x1 conv, patch embedding GEMM)
# =================================================================================================================
@_sink_aware
class LinearFn(Function):
    @staticmethod
    def forward(ctx, x2d, weight, bias, owner, dt, out_dtype):
        x2d = _c(x2d)
        xb = x2d if x2d.dtype == dt else ops.convert(x2d, dt)
        w, b = engine.prepared(owner, ("lin2d", dt), (weight, bias),
                               lambda: (weight.detach().reshape(weight.shape[0], -1).to(dt).contiguous(),
                                        None if bias is None else bias.detach().float().contiguous()))
        ctx.save_for_backward(xb)
        ctx.owner, ctx.dt, ctx.x_dtype, ctx.wshape, ctx.has_bias = owner, dt, x2d.dtype, weight.shape, bias is not None
        ctx.weight = weight
        return ops.gemm(xb, w, b, out_dtype=out_dtype)

    @staticmethod
    def backward(ctx, dy):
        (xb,) = ctx.saved_tensors
        dt = ctx.dt
        dy = _c(dy)
        need_dx = ctx.needs_input_grad[0]
        dyb = _as_dt(dy, dt)
        dW, db = _wgrad(dyb, xb, dt, ctx.has_bias, sink=[(ctx.weight, 0, ctx.wshape[0])])
        dW = None if dW is None else dW.view(ctx.wshape)
        dx = None
        if need_dx:
            wT = _w_t(ctx.owner, "lin2d", (ctx.weight,),
                      lambda: ctx.weight.detach().float().reshape(ctx.wshape[0], -1).contiguous(), dt)
            dx = ops.gemm(dyb, wT, out_dtype=ctx.x_dtype)
        return dx, dW, db, None, None, None


def linear(x2d, weight, bias, owner, dt, out_dtype):
    return LinearFn.apply(x2d, weight, bias, owner, dt, out_dtype)


@_sink_aware
class PatchEmbedFn(Function):
    """tokens = gather(img) . W^T + b (libs/croco/patch_embed.py:47,69-82).  The image's gradient (round 6; free under the reference's
    autograd) is d cols = d tok . W — one more GEMM — scattered back: patches do not overlap (stride = patch size), so the adjoint of the
    gather is a permutation of [B, gh, gw, c, u, v] into [B, c, gh u, gw v]."""

    @staticmethod
    def forward(ctx, img, weight, bias, owner, P, dt, out_dtype=torch.float32):
        cols = ops.patch_gather(img, P, dt)
        w, b = engine.patch_weights(owner, dt)
        ctx.save_for_backward(cols)
        ctx.dt, ctx.wshape, ctx.has_bias, ctx.weight, ctx.owner, ctx.P, ctx.ishape = dt, weight.shape, bias is not None, weight, owner, P, img.shape
        return ops.gemm(cols, w, b, out_dtype=out_dtype)

    @staticmethod
    def backward(ctx, dtok):
        (cols,) = ctx.saved_tensors
        dtok = _as_dt(_c(dtok), ctx.dt)
        dimg = None
        if ctx.needs_input_grad[0]:
            owner, P, (B, Cn, H, W) = ctx.owner, ctx.P, ctx.ishape
            wt = _w_t(owner, "pe", (owner.weight,), lambda: owner.weight.detach().float().reshape(owner.weight.shape[0], -1).contiguous(), ctx.dt)
            dcols = ops.gemm(dtok, wt, out_dtype=torch.float32)                       # [B gh gw, (c, u, v)]
            dimg = dcols.view(B, H // P, W // P, Cn, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, Cn, H, W)
        dW, db = (None, None)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dW, db = _wgrad(dtok, cols, ctx.dt, ctx.has_bias, sink=[(ctx.weight, 0, ctx.wshape[0])])
            dW = None if dW is None else dW.view(ctx.wshape)
        return dimg, dW, db, None, None, None, None


def patch_embed(img, conv, P, dt, out_dtype=torch.float32):
    return PatchEmbedFn.apply(img, conv.weight, conv.bias, conv, P, dt, out_dtype)


# =================================================================================================================
# Attention alone, and the UNFUSED sub-layers built from it: training through a FOREIGN positional-encoding callable (round 6; free
# under the reference's autograd: custom_positional_encoding is any callable of (tokens [B, H, N, Dh], positions),
# utils/transformer_blocks.py:226-229, 352-356).  The callable runs as ordinary PyTorch code between HIP Functions — LayerNorm, the
# QKV / q / kv linears, attention forward + backward, the output projection — and PyTorch's autograd differentiates it.
# =================================================================================================================
class AttentionFn(Function):
    "o = softmax(scale q k^T) v for [B, N, H, Dh] views; backward = uc_attention_bwd from the saved log-sum-exp."

    @staticmethod
    def forward(ctx, q, k, v, scale, adrop=None):
        q, k, v = (t if t.stride(3) == 1 else t.contiguous() for t in (q, k, v))
        B, Nq, H, _ = q.shape
        lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        o = _attention_fwd(q, k, v, scale, lse, adrop)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale, ctx.adrop = scale, adrop
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = ops.attention_bwd(q, k, v, o, _c(do).to(q.dtype), lse, ctx.scale, dropout=ctx.adrop)
        return dq, dk, dv, None, None


def attention(q, k, v, scale, attn_drop=None):
    return AttentionFn.apply(q, k, v, scale, attn_drop)


def _foreign_rope(rope, t4, pos):
    "the reference's call: rope(tokens [B, H, N, Dh], positions) (utils/transformer_blocks.py:228-229) on a [B, N, H, Dh] view"
    return rope(t4.transpose(1, 2), pos).transpose(1, 2)


def self_attn_sublayer_unfused(x2d, ln, qkv, proj, B, N, H, rope, pos, scale, dt, drops=None, attn_drop=None):
    """x + proj(SDPA(rope(q), rope(k), v)) with a foreign `rope` callable: HIP Functions around PyTorch-differentiated rope calls."""
    M, C = x2d.shape
    Ca = qkv.out_features // 3
    h = layer_norm(x2d, ln, dt)
    t5 = linear(h, qkv.weight, qkv.bias, qkv, dt, dt).view(B, N, 3, H, Ca // H)
    q, k = _foreign_rope(rope, t5[:, :, 0], pos), _foreign_rope(rope, t5[:, :, 1], pos)
    o = attention(q.to(dt), k.to(dt), t5[:, :, 2], scale, attn_drop)
    f = linear(o.reshape(M, Ca), proj.weight, proj.bias, proj, dt, x2d.dtype)
    if drops is not None and drops.has_out:
        raise UcHipError("dropout of the sub-layer output next to a foreign positional-encoding callable has no HIP path")
    return x2d + f


def cross_attn_sublayer_unfused(x2d, y2d, ln, lny, ca, B, Nq, Nk, H, rope, qpos, kpos, scale, dt, drops=None, attn_drop=None):
    "the cross-attention sub-layer of CrossAttentionBlock with a foreign `rope` callable (see self_attn_sublayer_unfused)"
    Mq, C = x2d.shape
    Dh = C // H
    hq = layer_norm(x2d, ln, dt)
    hy = layer_norm(y2d, lny, dt) if lny is not None else convert(y2d, dt)
    q = linear(hq, ca.projq.weight, ca.projq.bias, ca.projq, dt, dt).view(B, Nq, H, Dh)
    k = linear(hy, ca.projk.weight, ca.projk.bias, ca.projk, dt, dt).view(B, Nk, H, Dh)
    v = linear(hy, ca.projv.weight, ca.projv.bias, ca.projv, dt, dt).view(B, Nk, H, Dh)
    q, k = _foreign_rope(rope, q, qpos), _foreign_rope(rope, k, kpos)
    o = attention(q.to(dt), k.to(dt), v, scale, attn_drop)
    f = linear(o.reshape(Mq, C), ca.proj.weight, ca.proj.bias, ca.proj, dt, x2d.dtype)
    if drops is not None and drops.has_out:
        raise UcHipError("dropout of the sub-layer output next to a foreign positional-encoding callable has no HIP path")
    return x2d + f


# LayerScale behind a sub-layer's output linear (DINOv2 blocks, SelfAttentionBlock(init_values=...)): the forward runs the linear with
# the folded weights W_f = gamma[:,None] W, b_f = gamma b (engine.layerscale_lin_weights — zero kernel work); the backward takes the
# gradients of the FOLDED parameters from the usual weight-gradient GEMM and unfolds them:
#   dW = gamma[:,None] dW_f,  db = gamma db_f,  dgamma = rowsum(dW_f * W) + db_f * b.
def _folded_weight_t(lin, gamma, dt):
    return _w_t(lin, "ls", (lin.weight, gamma),
                lambda: (lin.weight.detach().float() * gamma.detach().float()[:, None]).contiguous(), dt)


def _unfold_layerscale(lin, gamma, dWf, dbf):
    W = lin.weight.detach().float()
    g = gamma.detach().float()
    dgamma = (dWf * W).sum(1)
    db = None
    if dbf is not None:
        dgamma = dgamma + dbf * lin.bias.detach().float()
        db = dbf * g
    return dWf * g[:, None], db, dgamma.to(gamma.dtype)


# =================================================================================================================
# pre-LN sub-layers of the transformer blocks: the steps the four Functions share, then the Functions
# =================================================================================================================
def _rope_in_gemm(rope, qn, kn, dt, Dh) -> bool:
    "Does the q / k GEMM's epilogue rotate its output (bf16 with a rope and no qk_norm)?  Else _prep_qk rotates behind the GEMM."
    if qn is not None or kn is not None or dt != torch.bfloat16 or rope is None or engine.is_axial_rope(rope):
        return False
    ops.attention_served(dt, Dh, rope=True)
    return True


def _prep_qk(q4, k4, qn, kn, rope, qpos, kpos, in_gemm: bool):
    """What lies between the q / k GEMM(s) and the attention forward, on the [B, N, H, Dh] views of the GEMM output.  qk_norm: q / k are
    normalised over head_dim BEFORE the positional encoding — the unfused route: the GEMM output keeps the RAW q | k, and the
    normalised, rotated copies the attention sees are returned (to be saved next to it).  Otherwise the views are rotated in place,
    unless the GEMM's epilogue did (`in_gemm`, see _rope_in_gemm), and None is returned."""
    if qn is None and kn is None:
        if rope is not None and not in_gemm:
            _rope_forward_(q4, k4, qpos, kpos, rope)
        return None
    qx = engine.qk_layernorm(q4, qn) if qn is not None else q4.contiguous()
    kx = engine.qk_layernorm(k4, kn) if kn is not None else k4.contiguous()
    if rope is not None:
        _rope_forward_(qx, kx, qpos, kpos, rope)
    return qx, kx


def _attention_bwd_block(q4, k4, v4, qkn, o, do4, lse, scale, dq4, dk4, dv4, rope, qpos, kpos, dt, qn, kn, adrop):
    """Backward of _prep_qk + attention: fills the views dq4 / dk4 / dv4 of the gradient of the q / k / v GEMM output (q4, k4, v4: views of
    that output; qkn: _prep_qk's copies or None) and returns (dq_norm.weight, dq_norm.bias, dk_norm.weight, dk_norm.bias)."""
    fused_rope = _bwd_rope(rope, qpos, kpos, dt)      # (bf16: the inverse rotation of dq / dk rides in the backward kernels)
    qa, ka = qkn if qkn else (q4, k4)
    dqa, dka = (torch.empty_like(qa), torch.empty_like(ka)) if qkn else (dq4, dk4)
    ops.attention_bwd(qa, ka, v4, o, do4, lse, scale, out=(dqa, dka, dv4), rope=fused_rope, dropout=adrop)
    if engine.is_axial_rope(rope):        # (gradients of the rotated q | k -> one inverse pass over dq | dk)
        rope.rotate_(dqa, dka, inverse=True)
    elif fused_rope is None:
        _rope_inverse_(dqa, qpos, rope)
        _rope_inverse_(dka, kpos, rope)
    dqn_w = dqn_b = dkn_w = dkn_b = None
    if qkn:
        if qn is not None:
            dqa, dqn_w, dqn_b = _qknorm_bwd(q4, qn, dqa)
        if kn is not None:
            dka, dkn_w, dkn_b = _qknorm_bwd(k4, kn, dka)
        dq4.copy_(dqa)
        dk4.copy_(dka)
    return dqn_w, dqn_b, dkn_w, dkn_b


def _out_linear_bwd(dyb, a2d, lin, gamma, has_bias, dt):
    """(dW, db, dgamma, W^T for the data gradient) of a sub-layer's output linear (proj, fc2, w3) on the operand a2d.  gamma: the
    LayerScale folded into it (see above) — gradient of the folded weight, unfolded into d W, d b, d gamma — or None."""
    if gamma is None:
        dW, db = _wgrad(dyb, a2d, dt, has_bias, sink=[(lin.weight, 0, lin.weight.shape[0])], bias_sink=[lin.bias])
        return dW, db, None, lin_weight_t(lin, dt)
    dW, db = _wgrad(dyb, a2d, dt, has_bias)
    return _unfold_layerscale(lin, gamma, dW, db) + (_folded_weight_t(lin, gamma, dt),)


def _ln_bwd_tail(x2d, ln, g, dh, dres=None, dt=None, residual: bool = True):
    """(dx, dgamma, dbeta) of the sub-layer's LayerNorm, dgamma / dbeta None where the kernel added them into the parameters' own
    gradient buffers (_ln_grad_targets).  residual: the residual-stream form (_ln_bwd_residual: d(x_out) = dres added in the same pass,
    a bf16 twin of dx where the next backward wants one); False: the LayerNorm of tokens that are not this sub-layer's stream (the
    other view's, in cross-attention) — the plain kernel call."""
    dg, db, sunk = _ln_grad_targets(ln, g)
    if residual:
        dx = _ln_bwd_residual(x2d, g, dh, ln.eps, dg, db, dres, dt)
    else:
        dx = ops.layernorm_bwd(x2d, g, dh, ln.eps, dg, db)
    return (dx, None, None) if sunk else (dx, dg, db)


@_sink_aware
class SelfAttnSubLayerFn(Function):
    """x + proj(SDPA(rope(q), rope(k), v)),  q,k,v = qkv(LN(x))   (blocks.py:105-125,154-158; transformer_blocks.py:214-260)."""

    @staticmethod
    def forward(ctx, x2d, ln_w, ln_b, w_qkv, b_qkv, w_proj, b_proj, ln, qkv, proj, B, N, H, rope, pos, scale, dt, gamma=None,
                qn_w=None, qn_b=None, kn_w=None, kn_b=None, qn=None, kn=None, drops=None, adrop=None):
        x2d = _c(x2d)
        M, C = x2d.shape
        Ca = qkv.out_features // 3          # width of q / k / v: C, or the layer's latent_attn_dim (utils/transformer_blocks.py:178-199)
        Dh = Ca // H
        _check_rope(rope)
        ops.attention_served(dt, Dh, dropout=adrop is not None, rope=rope is not None, qk_norm=qn is not None or kn is not None)
        g, bta = engine.ln_params(ln)
        h = ops.layernorm(x2d, g, bta, ln.eps, dt)
        wq, bq = engine.lin_weights(qkv, dt)
        wp, bp = engine.lin_weights(proj, dt) if gamma is None else engine.layerscale_lin_weights(proj, gamma, dt)
        in_gemm = _rope_in_gemm(rope, qn, kn, dt, Dh)
        t = ops.gemm(h, wq, bq, rope=engine._rope_epilogue(rope if in_gemm else None, pos, 2 * Ca))
        t5 = t.view(B, N, 3, H, Dh)
        qkn = _prep_qk(t5[:, :, 0], t5[:, :, 1], qn, kn, rope, pos, pos, in_gemm)
        lse = torch.empty((B, H, N), dtype=torch.float32, device=x2d.device)
        o = _attention_fwd(*(qkn if qkn is not None else (t5[:, :, 0], t5[:, :, 1])), t5[:, :, 2], scale, lse, adrop)
        if drops is not None and drops.has_out:
            out = _drop_out(ops.gemm(o.view(M, Ca), wp, bp), drops, x2d, x2d.dtype)
        else:
            out = ops.gemm(o.view(M, Ca), wp, bp, residual=x2d, out_dtype=x2d.dtype)
        # (gamma goes through save_for_backward: autograd's version check then catches an in-place edit between forward and backward)
        masks, dspec = _drops_saved(drops)
        ctx.save_for_backward(x2d, g, h, t, o, lse, pos if pos is not None else torch.empty(0), *(() if qkn is None else qkn),
                              *(() if gamma is None else (gamma,)), *masks)
        ctx.meta = (ln, qkv, proj, B, N, H, rope, scale, dt, b_qkv is not None, b_proj is not None, qn, kn, qkn is not None, dspec)
        ctx.adrop = adrop
        return out

    @staticmethod
    def backward(ctx, dxo):
        ln, qkv, proj, B, N, H, rope, scale, dt, has_bq, has_bp, qn, kn, has_qkn, dspec = ctx.meta
        drops, saved = _drops_restore(dspec, ctx.saved_tensors)
        x2d, g, h, t, o, lse, pos, *rest = saved
        qkn = rest[:2] if has_qkn else []
        rest = rest[2:] if has_qkn else rest
        gamma = rest[0] if rest else None
        M, C = x2d.shape
        Ca = qkv.out_features // 3          # width of q / k / v: C, or the layer's latent_attn_dim (utils/transformer_blocks.py:178-199)
        Dh = Ca // H
        dxo = _c(dxo)
        dyb = _as_dt(dxo, dt)
        if drops is not None and drops.has_out:
            dyb = _drop_out(dyb, drops)
        dWp, dbp, dgamma, wpt = _out_linear_bwd(dyb, o.view(M, Ca), proj, gamma, has_bp, dt)
        do = ops.gemm(dyb, wpt)
        dt3 = torch.empty_like(t)
        d5, t5 = dt3.view(B, N, 3, H, Dh), t.view(B, N, 3, H, Dh)
        dqn_w, dqn_b, dkn_w, dkn_b = _attention_bwd_block(t5[:, :, 0], t5[:, :, 1], t5[:, :, 2], qkn, o, do.view(B, N, H, Dh), lse, scale,
                                                          d5[:, :, 0], d5[:, :, 1], d5[:, :, 2], rope, pos, pos, dt, qn, kn, ctx.adrop)
        dWq, dbq = _wgrad(dt3, h, dt, has_bq, sink=[(qkv.weight, 0, 3 * Ca)], bias_sink=[qkv.bias])
        dh = ops.gemm(dt3, lin_weight_t(qkv, dt))
        dx, dg, db = _ln_bwd_tail(x2d, ln, g, dh, dxo, dt)
        return (dx, dg, db, dWq, dbq, dWp, dbp) + (None,) * 10 + (dgamma, dqn_w, dqn_b, dkn_w, dkn_b, None, None, None, None)


def self_attn_sublayer(x2d, ln, qkv, proj, B, N, H, rope, pos, scale, dt, gamma=None, q_norm=None, k_norm=None, drops=None, attn_drop=None):
    """gamma: LayerScale on the sub-layer's output (x + gamma * proj(...)), or None.  q_norm / k_norm: the layer's qk_norm modules
    (LayerNorm over head_dim before the positional encoding; nn.Identity / None: off).  attn_drop: (p, seed) from attn_dropout, or None."""
    qn, kn = _norm_or_none(q_norm), _norm_or_none(k_norm)
    if rope is not None and not engine.is_native_rope(rope) and not engine.is_axial_rope(rope):      # a foreign positional-encoding callable: the unfused route
        if gamma is not None or qn is not None or kn is not None:
            raise UcHipError("LayerScale / qk_norm next to a foreign positional-encoding callable have no HIP training path")
        return self_attn_sublayer_unfused(x2d, ln, qkv, proj, B, N, H, rope, pos, scale, dt, drops, attn_drop)
    return SelfAttnSubLayerFn.apply(x2d, ln.weight, ln.bias, qkv.weight, qkv.bias, proj.weight, proj.bias, ln, qkv, proj,
                                    B, N, H, rope, pos, scale, dt, gamma, getattr(qn, "weight", None), getattr(qn, "bias", None),
                                    getattr(kn, "weight", None), getattr(kn, "bias", None), qn, kn, drops, attn_drop)


@_sink_aware
class CrossAttnSubLayerFn(Function):
    """x + proj(SDPA(rope(projq(LN2(x)), xpos), rope(projk(LNy(y)), ypos), projv(LNy(y))))  (transformer_blocks.py:329-412,604-647)."""

    @staticmethod
    def forward(ctx, x2d, y2d, ln_w, ln_b, lny_w, lny_b, wq_, bq_, wk_, bk_, wv_, bv_, wp_, bp_, ln, lny, projq, projk, projv, proj,
                B, Nq, Nk, H, rope, qpos, kpos, scale, dt, qn_w=None, qn_b=None, kn_w=None, kn_b=None, qn=None, kn=None, drops=None,
                gamma=None, adrop=None):
        x2d, y2d = _c(x2d), _c(y2d)
        Mq, C = x2d.shape
        Dh = C // H
        _check_rope(rope)
        ops.attention_served(dt, Dh, dropout=adrop is not None, rope=rope is not None, qk_norm=qn is not None or kn is not None)
        g, bta = engine.ln_params(ln)
        hq = ops.layernorm(x2d, g, bta, ln.eps, dt)
        if lny is not None:
            gy, by = engine.ln_params(lny)
            hy = ops.layernorm(y2d, gy, by, lny.eps, dt)
        else:
            gy = torch.empty(0, device=x2d.device)
            hy = y2d if y2d.dtype == dt else ops.convert(y2d, dt)
        wq, bq = engine.lin_weights(projq, dt)
        wkv, bkv = engine.kv_weights(projk, projv, dt)
        wp, bp = engine.lin_weights(proj, dt) if gamma is None else engine.layerscale_lin_weights(proj, gamma, dt)
        in_gemm = _rope_in_gemm(rope, qn, kn, dt, Dh)
        q = ops.gemm(hq, wq, bq, rope=engine._rope_epilogue(rope if in_gemm else None, qpos, C))
        kv = ops.gemm(hy, wkv, bkv, rope=engine._rope_epilogue(rope if in_gemm else None, kpos, C))
        kv5 = kv.view(B, Nk, 2, H, Dh)
        qkn = _prep_qk(q.view(B, Nq, H, Dh), kv5[:, :, 0], qn, kn, rope, qpos, kpos, in_gemm)
        lse = torch.empty((B, H, Nq), dtype=torch.float32, device=x2d.device)
        o = _attention_fwd(*(qkn if qkn is not None else (q.view(B, Nq, H, Dh), kv5[:, :, 0])), kv5[:, :, 1], scale, lse, adrop)
        ctx.adrop = adrop
        if drops is not None and drops.has_out:
            out = _drop_out(ops.gemm(o.view(Mq, C), wp, bp), drops, x2d, x2d.dtype)
        else:
            out = ops.gemm(o.view(Mq, C), wp, bp, residual=x2d, out_dtype=x2d.dtype)
        e = torch.empty(0)
        masks, dspec = _drops_saved(drops)
        ctx.save_for_backward(x2d, y2d, g, gy, hq, hy, q, kv, o, lse, qpos if qpos is not None else e, kpos if kpos is not None else e,
                              *(() if qkn is None else qkn), *(() if gamma is None else (gamma,)), *masks)
        ctx.meta = (ln, lny, projq, projk, projv, proj, B, Nq, Nk, H, rope, scale, dt,
                    bq_ is not None, bk_ is not None, bv_ is not None, bp_ is not None, qn, kn, dspec, qkn is not None)
        return out

    @staticmethod
    def backward(ctx, dxo):
        ln, lny, projq, projk, projv, proj, B, Nq, Nk, H, rope, scale, dt, has_bq, has_bk, has_bv, has_bp, qn, kn, dspec, has_qkn = ctx.meta
        drops, saved = _drops_restore(dspec, ctx.saved_tensors)
        x2d, y2d, g, gy, hq, hy, q, kv, o, lse, qpos, kpos, *rest = saved
        qkn = rest[:2] if has_qkn else []
        rest = rest[2:] if has_qkn else rest
        gamma = rest[0] if rest else None
        Mq, C = x2d.shape
        Dh = C // H
        dxo = _c(dxo)
        dyb = _as_dt(dxo, dt)
        if drops is not None and drops.has_out:
            dyb = _drop_out(dyb, drops)
        dWp, dbp, dgamma, wpt = _out_linear_bwd(dyb, o.view(Mq, C), proj, gamma, has_bp, dt)
        do = ops.gemm(dyb, wpt)
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        kv5, dkv5 = kv.view(B, Nk, 2, H, Dh), dkv.view(B, Nk, 2, H, Dh)
        dqn_w, dqn_b, dkn_w, dkn_b = _attention_bwd_block(q.view(B, Nq, H, Dh), kv5[:, :, 0], kv5[:, :, 1], qkn, o, do.view(B, Nq, H, Dh), lse,
                                                          scale, dq.view(B, Nq, H, Dh), dkv5[:, :, 0], dkv5[:, :, 1], rope, qpos, kpos, dt,
                                                          qn, kn, ctx.adrop)
        # query side
        dWq, dbq = _wgrad(dq, hq, dt, has_bq, sink=[(projq.weight, 0, C)], bias_sink=[projq.bias])
        dhq = ops.gemm(dq, lin_weight_t(projq, dt))
        dx, dg, db = _ln_bwd_tail(x2d, ln, g, dhq, dxo, dt)
        # key/value side (the other view's tokens)
        dWkv, dbkv = _wgrad(dkv, hy, dt, has_bk or has_bv, sink=[(projk.weight, 0, C), (projv.weight, C, 2 * C)],
                            bias_sink=[projk.bias, projv.bias] if (has_bk and has_bv) else None)
        dhy = ops.gemm(dkv, kv_weight_t(projk, projv, dt), out_dtype=dt if lny is not None else y2d.dtype)
        # (the other view's tokens are not this sub-layer's residual stream: no d(x_out) to add, no bf16 twin of dy)
        dy, dgy, dby = _ln_bwd_tail(y2d, lny, gy, dhy, residual=False) if lny is not None else (dhy, None, None)
        dWk, dWv = (None, None) if dWkv is None else (dWkv[:C], dWkv[C:])
        dbk = dbkv[:C] if (has_bk and dbkv is not None) else None
        dbv = dbkv[C:] if (has_bv and dbkv is not None) else None
        return (dx, dy, dg, db, dgy, dby, dWq, dbq, dWk, dbk, dWv, dbv, dWp, dbp) + (None,) * 15 + (dqn_w, dqn_b, dkn_w, dkn_b, None, None, None,
                                                                                                      dgamma, None)


def cross_attn_sublayer(x2d, y2d, ln, lny, ca, B, Nq, Nk, H, rope, qpos, kpos, scale, dt, drops=None, gamma=None, attn_drop=None):
    lw, lb = (lny.weight, lny.bias) if lny is not None else (None, None)
    qn, kn = _norm_or_none(getattr(ca, "q_norm", None)), _norm_or_none(getattr(ca, "k_norm", None))
    if rope is not None and not engine.is_native_rope(rope):      # a foreign positional-encoding callable: the unfused route
        if gamma is not None or qn is not None or kn is not None:
            raise UcHipError("LayerScale / qk_norm next to a foreign positional-encoding callable have no HIP training path")
        return cross_attn_sublayer_unfused(x2d, y2d, ln, lny, ca, B, Nq, Nk, H, rope, qpos, kpos, scale, dt, drops, attn_drop)
    return CrossAttnSubLayerFn.apply(x2d, y2d, ln.weight, ln.bias, lw, lb, ca.projq.weight, ca.projq.bias, ca.projk.weight,
                                     ca.projk.bias, ca.projv.weight, ca.projv.bias, ca.proj.weight, ca.proj.bias, ln, lny,
                                     ca.projq, ca.projk, ca.projv, ca.proj, B, Nq, Nk, H, rope, qpos, kpos, scale, dt,
                                     getattr(qn, "weight", None), getattr(qn, "bias", None), getattr(kn, "weight", None),
                                     getattr(kn, "bias", None), qn, kn, drops, gamma, attn_drop)


def _mlp_bwd(dyb, h, u, a, fc1, fc2, gamma, act, dt, has_b1, has_b2, drops):
    """(dW2, db2, dgamma, du, dW1, db1) of fc2(act(fc1(h))) for the already-dropped cotangent dyb (u: the pre-activation, a: fc2's
    operand): what the backwards of MlpSubLayerFn and MlpFn share."""
    dW2, db2, dgamma, w2t = _out_linear_bwd(dyb, a, fc2, gamma, has_b2, dt)
    if act != "none" and dt == torch.bfloat16 and w2t.shape[1] % 64 == 0:
        du = ops.gemm(dyb, w2t, dact=(u, act))          # act'(u) applied in the data-gradient GEMM's epilogue
    else:
        da = ops.gemm(dyb, w2t)
        du = ops.act_bwd(da, u, act) if act != "none" else da
    if drops is not None and drops.mid is not None:      # (elementwise factors commute: mask * act'(u) * da)
        du = ops.mask_scale(du, drops.mid, 0, drops.mid_scale)
    dW1, db1 = _wgrad(du, h, dt, has_b1, sink=[(fc1.weight, 0, fc1.weight.shape[0])], bias_sink=[fc1.bias])
    return dW2, db2, dgamma, du, dW1, db1


@_sink_aware
class MlpSubLayerFn(Function):
    """x + fc2(act(fc1(LN(x))))   (blocks.py:64-86,159; transformer_blocks.py:517-560)."""

    @staticmethod
    def forward(ctx, x2d, ln_w, ln_b, w1_, b1_, w2_, b2_, ln, fc1, fc2, act, dt, gamma=None, drops=None):
        x2d = _c(x2d)
        g, bta = engine.ln_params(ln)
        h = ops.layernorm(x2d, g, bta, ln.eps, dt)
        w1, b1 = engine.lin_weights(fc1, dt)
        w2, b2 = engine.lin_weights(fc2, dt) if gamma is None else engine.layerscale_lin_weights(fc2, gamma, dt)
        u = torch.empty((x2d.shape[0], w1.shape[0]), dtype=dt, device=x2d.device)
        if dt == torch.bfloat16 and h.shape[1] % 64 != 0:
            # a width the direct-to-LDS GEMM does not take (K % 64 != 0: its preact_out epilogue is not there): the pre-activation
            # leaves the plain GEMM and uc_act applies the activation in a pass of its own
            ops.gemm(h, w1, b1, out=u)
            a = ops.act(u, act) if act != "none" else u
        else:
            a = ops.gemm(h, w1, b1, act=act, preact_out=u)
        if drops is not None and drops.mid is not None:      # drop1: the hidden activation fc2 (and its weight gradient) sees
            a = ops.mask_scale(a, drops.mid, 0, drops.mid_scale)
        if drops is not None and drops.has_out:
            out = _drop_out(ops.gemm(a, w2, b2), drops, x2d, x2d.dtype)
        else:
            out = ops.gemm(a, w2, b2, residual=x2d, out_dtype=x2d.dtype)
        masks, dspec = _drops_saved(drops)
        ctx.save_for_backward(x2d, g, h, u, a, *(() if gamma is None else (gamma,)), *masks)
        ctx.meta = (ln, fc1, fc2, act, dt, b1_ is not None, b2_ is not None, dspec)
        return out

    @staticmethod
    def backward(ctx, dxo):
        ln, fc1, fc2, act, dt, has_b1, has_b2, dspec = ctx.meta
        drops, saved = _drops_restore(dspec, ctx.saved_tensors)
        x2d, g, h, u, a, *rest = saved
        gamma = rest[0] if rest else None
        dxo = _c(dxo)
        dyb = _as_dt(dxo, dt)
        if drops is not None and drops.has_out:
            dyb = _drop_out(dyb, drops)
        dW2, db2, dgamma, du, dW1, db1 = _mlp_bwd(dyb, h, u, a, fc1, fc2, gamma, act, dt, has_b1, has_b2, drops)
        dh = ops.gemm(du, lin_weight_t(fc1, dt))
        dx, dg, db = _ln_bwd_tail(x2d, ln, g, dh, dxo, dt)
        return (dx, dg, db, dW1, db1, dW2, db2) + (None,) * 5 + (dgamma, None)


def mlp_sublayer(x2d, ln, fc1, fc2, act, dt, gamma=None, drops=None):
    "gamma: LayerScale on the sub-layer's output (x + gamma * fc2(...)), or None.  drops: the call's dropout masks (make_drops) or None."
    return MlpSubLayerFn.apply(x2d, ln.weight, ln.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, ln, fc1, fc2, act, dt, gamma, drops)


@_sink_aware
class SwiGLUSubLayerFn(Function):
    """x + w3(silu(x1) * x2),  x1, x2 = w12(LN(x)).chunk(2)   (DINOv2 giant: the hub's SwiGLUFFNFused behind encoders/dinov2.py:68-84)."""

    @staticmethod
    def forward(ctx, x2d, ln_w, ln_b, w12_, b12_, w3_, b3_, ln, w12, w3, dt, gamma=None):
        x2d = _c(x2d)
        g, bta = engine.ln_params(ln)
        h = ops.layernorm(x2d, g, bta, ln.eps, dt)
        w1, b1 = engine.lin_weights(w12, dt)
        w2, b2 = engine.lin_weights(w3, dt) if gamma is None else engine.layerscale_lin_weights(w3, gamma, dt)
        t = ops.gemm(h, w1, b1)
        a = ops.swiglu(t)
        out = ops.gemm(a, w2, b2, residual=x2d, out_dtype=x2d.dtype)
        ctx.save_for_backward(x2d, g, h, t, a, *(() if gamma is None else (gamma,)))
        ctx.meta = (ln, w12, w3, dt, b12_ is not None, b3_ is not None)
        return out

    @staticmethod
    def backward(ctx, dxo):
        x2d, g, h, t, a, *rest = ctx.saved_tensors
        gamma = rest[0] if rest else None
        ln, w12, w3, dt, has_b1, has_b2 = ctx.meta
        dxo = _c(dxo)
        dyb = _as_dt(dxo, dt)
        dW2, db2, dgamma, w2t = _out_linear_bwd(dyb, a, w3, gamma, has_b2, dt)
        dtt = ops.swiglu_bwd(ops.gemm(dyb, w2t), t)
        dW1, db1 = _wgrad(dtt, h, dt, has_b1, sink=[(w12.weight, 0, w12.weight.shape[0])], bias_sink=[w12.bias])
        dh = ops.gemm(dtt, lin_weight_t(w12, dt))
        dx, dg, db = _ln_bwd_tail(x2d, ln, g, dh, dxo, dt)
        return (dx, dg, db, dW1, db1, dW2, db2) + (None,) * 4 + (dgamma,)


def swiglu_sublayer(x2d, ln, w12, w3, dt, gamma=None):
    "gamma: LayerScale on the sub-layer's output (x + gamma * w3(...)), or None."
    return SwiGLUSubLayerFn.apply(x2d, ln.weight, ln.bias, w12.weight, w12.bias, w3.weight, w3.bias, ln, w12, w3, dt, gamma)


# =================================================================================================================
# heads: pixel shuffle, adaptor, loss
# =================================================================================================================
@_sink_aware
class PixelShuffleFn(Function):
    @staticmethod
    def forward(ctx, rows, B, h, w, P, Cout):
        ctx.P = P
        return ops.pixel_shuffle(_c(rows), B, h, w, P, Cout)

    @staticmethod
    def backward(ctx, dimg):
        return ops.pixel_unshuffle(_c(dimg), ctx.P, torch.float32), None, None, None, None, None


def pixel_shuffle(rows, B, h, w, P, Cout):
    return PixelShuffleFn.apply(rows, B, h, w, P, Cout)


@_sink_aware
class PointmapAdaptorFn(Function):
    @staticmethod
    def forward(ctx, x, vmin, vmax):
        ctx.save_for_backward(x)
        ctx.v = (vmin, vmax)
        pts, conf = ops.pointmap_adaptor(x, vmin, vmax)
        return pts, conf

    @staticmethod
    def backward(ctx, dpts, dconf):
        (x,) = ctx.saved_tensors
        return ops.pointmap_adaptor_bwd(x, _c(dpts), _c(dconf), *ctx.v), None, None


def pointmap_adaptor(x, vmin, vmax):
    return PointmapAdaptorFn.apply(x, vmin, vmax)


@_sink_aware
class AdaptorProgramFn(Function):
    """A channel program of the generic adaptor pass (ops.adaptor_program) and its gradient with respect to the decoded channels
    (what torch autograd computes through the reference's adaptor compositions, prediction_heads/adaptors.py:25-2300)."""

    @staticmethod
    def forward(ctx, x, segs, cout):
        ctx.save_for_backward(x)
        ctx.segs = segs
        return ops.adaptor_program(x, segs, cout)

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        return ops.adaptor_program_bwd(x, _c(dout), ctx.segs), None, None


def adaptor_program(x, segs, cout):
    return AdaptorProgramFn.apply(x, segs, cout)


@_sink_aware
class ConfLossFn(Function):
    """mean_pix(conf * |pts - gt|) - alpha * mean_pix(log conf): the DUSt3R confidence-weighted regression objective
    (the reference ships no loss; SURVEY §8d names this one).  One kernel computes the loss and both gradients."""

    @staticmethod
    def forward(ctx, pts, conf, gt, alpha):
        pts, conf, gt = _c(pts), _c(conf), _c(gt)
        npix = conf.numel()
        acc = torch.zeros(1, dtype=torch.float32, device=pts.device)
        dpts, dconf = ops.conf_loss(pts, conf, gt, alpha, 1.0 / npix, acc)
        ctx.save_for_backward(dpts, dconf)
        return acc[0] / npix

    @staticmethod
    def backward(ctx, g):
        dpts, dconf = ctx.saved_tensors
        return dpts * g, dconf * g, None, None


def conf_loss(pts, conf, gt, alpha: float = 0.2):
    return ConfLossFn.apply(pts, conf, gt.float(), alpha)


# =================================================================================================================
# DPT head (NHWC maps in the head dtype): 3x3 implicit-GEMM convs, 1x1 convs (LinearFn on the pixel matrix),
# ConvTranspose2d(k=s), bilinear resize, the 4-channel regressor tail, and the dtype hop at the head's entry
# =================================================================================================================
@_sink_aware
class ConvertFn(Function):
    @staticmethod
    def forward(ctx, x, dt):
        ctx.src = x.dtype
        x = _c(x)
        return x if x.dtype == dt else ops.convert(x, dt)

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        return (dy if dy.dtype == ctx.src else ops.convert(dy, ctx.src)), None


def convert(x, dt):
    return ConvertFn.apply(x, dt)


def _conv3x3_rot_weight(conv, dt, cin_pad: int, cout_pad: int):
    """GEMM weight of the data gradient: [cin_pad, 9*cout_pad] with K ordered (ky', kx', o) = W[o, c, 2-ky', 2-kx']: the forward layout of
    the flipped, transposed weight."""
    return engine.prepared(conv, ("c3rot", dt, cin_pad, cout_pad), (conv.weight,),
                           lambda: engine.conv3x3_weight2d(conv.weight.flip(2, 3).transpose(0, 1), cout_pad, cin_pad).to(dt).contiguous())


@_sink_aware
class Conv3x3Fn(Function):
    """y = [residual +] act(conv3x3(relu?(x)) + b) on NHWC maps (dpt_block.py:17-289, dpt.py:116-178,271-277).  x may carry zero
    channels beyond conv.in_channels and y zero channels up to `cout_pad` (zero weight columns / rows: the MoGe output block's
    Conv2d(64 + 2 -> 32), the dense encoder's ResidualBlock); stride 1 without `relu_in` only.  out_dtype: of y, default x's."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, residual2, conv, relu_in, act, grad_mask_cell=None, cout_pad=None, out_dtype=None):
        ctx.grad_mask_cell = grad_mask_cell
        x = _c(x)
        B, H, W, cin_pad = x.shape
        s = conv.stride[0]
        if (cin_pad != conv.in_channels or (cout_pad or conv.out_channels) != conv.out_channels) and (s != 1 or relu_in):
            raise UcHipError("conv3x3: zero-padded channel counts are for stride 1 without a fused input ReLU")
        w, b = engine.conv3x3_weights(conv, x.dtype, cin_pad, cout_pad)
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        r1 = None if residual is None else _c(residual).reshape(-1, residual.shape[-1])
        r2 = None if residual2 is None else _c(residual2).reshape(-1, residual2.shape[-1])
        y = ops.gemm(x, w, b, act=act, residual=r1, residual2=r2, relu_a=relu_in, conv=(B, H, W, cin_pad, s), out_dtype=out_dtype)
        y = y.view(B, Ho, Wo, -1)
        if act not in (None, "none", "relu"):
            raise UcHipError(f"conv3x3 backward: unsupported fused activation {act}")
        if act == "relu" and residual is not None:
            raise UcHipError("conv3x3 backward: fused ReLU together with a residual is not used by the DPT head")
        ctx.save_for_backward(x, y if act == "relu" else torch.empty(0))
        ctx.meta = (conv, relu_in, act, bias is not None, s, [None if r is None else r.dtype for r in (residual, residual2)])
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        conv, relu_in, act, has_b, s, res_dtypes = ctx.meta
        B, H, W, cin_pad = x.shape
        dt = x.dtype
        dy = _c(dy)
        cout_pad = dy.shape[-1]
        cell = ctx.grad_mask_cell
        already_masked = cell is not None and cell[0]          # the only consumer's backward applied this ReLU's mask (Conv1x1To4Fn)
        if cell is not None:
            cell[0] = False
        dz = _as_dt(dy, dt)
        if act == "relu" and not already_masked:
            dz = ops.act_bwd(dz, y, "relu")
        if has_b and dy.dtype != dt:       # an fp32 cotangent (the head's last layer): the bias gradient sums it unrounded
            dWg, db = _wgrad_conv(dz, x, s, relu_in)[0], _colsum(dy.view(-1, cout_pad))
        else:
            dWg, db = _wgrad_conv(dz, x, s, relu_in, has_b)                      # [cout_pad, 9*cin_pad], K ordered (ky,kx,c)
        dW = dWg.view(cout_pad, 3, 3, cin_pad)[:conv.out_channels, :, :, :conv.in_channels].permute(0, 3, 1, 2)
        dx = None
        if ctx.needs_input_grad[0]:
            g = dz if s == 1 else ops.dilate_nhwc(dz, H, W, s)
            wr = _conv3x3_rot_weight(conv, dt, cin_pad, cout_pad)
            if relu_in and dt == torch.bfloat16 and cout_pad % 64 == 0:
                dx = ops.gemm(g, wr, conv=(B, H, W, cout_pad, 1), dact=(x.view(-1, cin_pad), "relu")).view(B, H, W, cin_pad)
            else:
                dx = ops.gemm(g, wr, conv=(B, H, W, cout_pad, 1)).view(B, H, W, cin_pad)
                if relu_in:
                    dx = ops.act_bwd(dx, x, "relu")
        dr1, dr2 = (None if rdt is None or not ctx.needs_input_grad[i] else _as_dt(dy, rdt) for i, rdt in zip((3, 4), res_dtypes))
        return dx, dW, (db[:conv.out_channels] if has_b else None), dr1, dr2, None, None, None, None, None, None


def conv3x3(x, conv, relu_in=False, act=None, residual=None, residual2=None, grad_mask_cell=None):
    """grad_mask_cell: a one-element list shared with the SOLE consumer of a fused-ReLU output (conv1x1_to4(relu_cell=...)); when that
    consumer's backward has applied the ReLU mask it sets cell[0] and this backward skips its own mask pass."""
    return Conv3x3Fn.apply(x, conv.weight, conv.bias, residual, residual2, conv, relu_in, act, grad_mask_cell)


def conv1x1(x, conv):
    B, H, W, Cin = x.shape
    y = LinearFn.apply(x.reshape(-1, Cin), conv.weight, conv.bias, conv, x.dtype, x.dtype)
    return y.view(B, H, W, -1)


def _padded_conv1x1_weight2d(conv, cpad):
    "fp32 [cpad, Cin] of a Conv2d(k=1) weight: zero rows beyond conv.out_channels"
    w = torch.zeros(cpad, conv.in_channels, device=conv.weight.device)
    w[:conv.out_channels] = conv.weight.detach().reshape(conv.out_channels, -1).float()
    return w


def padded_conv1x1_weights(conv, dt, cpad):
    "Conv2d(k=1) weights with the output channels padded by zero rows to `cpad` (the 8-channel granule of the NHWC kernels)."
    def build():
        b = torch.zeros(cpad, device=conv.weight.device)
        if conv.bias is not None:
            b[:conv.out_channels] = conv.bias.detach().float()
        return _padded_conv1x1_weight2d(conv, cpad).to(dt).contiguous(), b
    return engine.prepared(conv, ("c1pad", dt), (conv.weight, conv.bias), build)


@_sink_aware
class PaddedConv1x1Fn(Function):
    """A 1x1 convolution to a channel count that is not a multiple of 8 (DPTSegmentationProcessor's class logits, dpt.py:314-381; the
    MoGe head's last conv): computed on `cpad` output columns (zero weight rows), fp32 output [M, cpad]; gradients of the real rows only.
    fp32_bias: the bias gradient is the column sum of the fp32 cotangent itself, not of its copy rounded to the operand dtype (a sum
    over every pixel of the image in which the rounding errors of the summands do not average out against a cancelling total)."""

    @staticmethod
    def forward(ctx, x2d, weight, bias, conv, dt, cpad, fp32_bias):
        x2d = _c(x2d)
        xb = x2d if x2d.dtype == dt else ops.convert(x2d, dt)
        w, b = padded_conv1x1_weights(conv, dt, cpad)
        ctx.save_for_backward(xb)
        ctx.meta = (conv, dt, x2d.dtype, weight.shape, bias is not None, cpad, fp32_bias)
        return ops.gemm(xb, w, b, out_dtype=torch.float32)

    @staticmethod
    def backward(ctx, dy):
        (xb,) = ctx.saved_tensors
        conv, dt, x_dtype, wshape, has_b, cpad, fp32_bias = ctx.meta
        n = wshape[0]
        dy = _c(dy)
        dyb = _as_dt(dy, dt)
        dW, db = _wgrad(dyb, xb, dt, has_b and not fp32_bias)
        if has_b and fp32_bias:
            db = _colsum(dy)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(dyb, _w_t(conv, "c1pad", (conv.weight,), lambda: _padded_conv1x1_weight2d(conv, cpad), dt), out_dtype=x_dtype)
        return dx, dW[:n].reshape(wshape), (db[:n] if has_b else None), None, None, None, None


def padded_conv1x1(x, conv, dt, cpad, fp32_bias: bool = False):
    B, H, W, Cin = x.shape
    return PaddedConv1x1Fn.apply(x.reshape(-1, Cin), conv.weight, conv.bias, conv, dt, cpad, fp32_bias).view(B, H, W, cpad)


def out_conv1x1(x, conv, dt, cpad):
    "the head's last 1x1 convolution: padded_conv1x1 with the bias gradient summed from the fp32 cotangent"
    return padded_conv1x1(x, conv, dt, cpad, fp32_bias=True)


@_sink_aware
class ConvTransposeFn(Function):
    """ConvTranspose2d(kernel = stride, no padding) = GEMM to (u,v,o) columns + pixel scatter (dpt.py:116-140).  x may carry zero
    channels beyond ct.in_channels (the K granule of the dense GEMM: 514 -> 576, ...), matched by zero weight columns."""

    @staticmethod
    def forward(ctx, x, weight, bias, ct):
        x = _c(x)
        B, H, W, kpad = x.shape
        k = ct.kernel_size[0]
        w, b = engine.convt_weights(ct, x.dtype, kpad)
        x2 = x.view(-1, kpad)
        y = ops.gemm(x2, w, b)
        ctx.save_for_backward(x2)
        ctx.meta = (ct, k, (B, H, W, kpad), bias is not None)
        return ops.convt_scatter(y, B, H, W, k, ct.out_channels)

    @staticmethod
    def backward(ctx, dy):
        (x2,) = ctx.saved_tensors
        ct, k, (B, H, W, kpad), has_b = ctx.meta
        dt = x2.dtype
        Cout = ct.out_channels
        dyg = ops.convt_gather(_as_dt(_c(dy), dt), k)                            # [B*H*W, k*k*Cout]
        dWg, dbg = _wgrad(dyg, x2, dt, has_b)                                    # [k*k*Cout, kpad], [k*k*Cout]
        dW = dWg.view(k, k, Cout, kpad)[..., :ct.in_channels].permute(3, 2, 0, 1)
        db = dbg.view(k * k, Cout).sum(0) if has_b else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(dyg, _w_t(ct, ("ct", kpad), (ct.weight,), lambda: engine.convt_weight2d(ct, kpad), dt)).view(B, H, W, kpad)
        return dx, dW, db, None


def conv_transpose_ks(x, ct):
    return ConvTransposeFn.apply(x, ct.weight, ct.bias, ct)


def conv_transpose_padded(x, ct):
    if ct.kernel_size != ct.stride or ct.kernel_size[0] != ct.kernel_size[1] or ct.padding != (0, 0) or ct.output_padding != (0, 0):
        raise UcHipError("conv_transpose_padded: only ConvTranspose2d(kernel = stride, no padding) has a HIP path")
    return ConvTransposeFn.apply(x, ct.weight, ct.bias, ct)


@_sink_aware
class BilinearFn(Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo, crop):
        x = _c(x)
        ctx.geom = (x.shape[1], x.shape[2], Ho, Wo)
        return ops.bilinear_nhwc(x, Ho, Wo, crop)

    @staticmethod
    def backward(ctx, dy):
        Hi, Wi, Ho, Wo = ctx.geom
        return ops.bilinear_nhwc_bwd(_c(dy), Hi, Wi, Ho, Wo), None, None, None


def bilinear(x, Ho, Wo, crop=None):
    return BilinearFn.apply(x, Ho, Wo, crop)


@_sink_aware
class Conv1x1To4Fn(Function):
    """Regressor tail: features -> 4 decoded channels, fp32 output (dpt.py:271-277 conv2[2])."""

    @staticmethod
    def forward(ctx, x, weight, bias, w4, b4, relu_cell=None):
        x = _c(x)
        ctx.save_for_backward(x, w4)
        ctx.wshape, ctx.has_b, ctx.relu_cell = weight.shape, bias is not None, relu_cell
        return ops.conv1x1_to4(x, w4, b4)

    @staticmethod
    def backward(ctx, dout):
        x, w4 = ctx.saved_tensors
        dw = torch.zeros_like(w4)
        db = torch.zeros(4, dtype=torch.float32, device=x.device)
        # x straight out of a fused-ReLU conv3x3 (relu_cell from conv3x3(..., grad_mask_cell=...)): that ReLU's backward rides in this
        # kernel, and the cell tells the conv's backward not to mask again
        masked = ctx.relu_cell is not None
        dfeat = ops.conv1x1_to4_bwd(x, w4, _c(dout), dw, db, relu_mask=masked)
        if masked:
            ctx.relu_cell[0] = True
        return dfeat, dw.view(ctx.wshape), (db if ctx.has_b else None), None, None, None


def conv1x1_to4(x, conv, w4, b4, relu_cell=None):
    return Conv1x1To4Fn.apply(x, conv.weight, conv.bias, w4, b4, relu_cell)


# =================================================================================================================
# Differential attention (reference: utils/transformer_blocks.py:686-945).  Forward: ONE fused kernel (uc_diff_attention_fwd: both
# softmaxes over one staged V, combine, RMSNorm).  Backward: uc_diff_attention_combine_bwd (dA1, dA2, dlambda, d subln.weight; fixed-order
# reductions), then uc_attention_bwd once per softmax on Q / K zero-padded to V's head_dim — padding leaves the scores unchanged and the
# padded gradient columns are exactly zero — with the saved LSEs; dV is the sum of the two calls.
# =================================================================================================================
class Rope2dFn(Function):
    "native RoPE-2D of a [B, N, H, D] view as a pass of its own (uc_rope2d, any D % 4 == 0); backward = the inverse rotation"

    @staticmethod
    def forward(ctx, t4, pos, base, F0):
        out = t4.clone() if t4.is_contiguous() else t4.contiguous()
        pos = pos.contiguous()
        ops.rope_2d_(out, pos, base, F0)
        ctx.pos, ctx.base, ctx.F0 = pos, base, F0
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().clone()
        ops.rope_2d_(g, ctx.pos, ctx.base, -ctx.F0)
        return g, None, None, None


def rope2d(t4, pos, rope):
    if rope is None:
        return t4
    _check_rope(rope)
    return Rope2dFn.apply(t4, pos if pos.dtype == torch.int64 else pos.long(), rope.base, rope.F0)


class DiffAttentionFunction(Function):
    """y [B * Nq, H * 2hd] = RMSNorm(softmax(scale q1 k1^T) v - lam softmax(scale q2 k2^T) v; w, eps) * out_scale for
    q [B, Nq, 2H, hd], k [B, Nk, 2H, hd] (heads [0, H) feed softmax 1, [H, 2H) softmax 2), v [B, Nk, H, 2hd]; lam: 0-d fp32 tensor.
    head_major: the result's memory order is [B, H, Nq, 2hd] (what DiffAttention.forward reshapes WITHOUT a transpose), else
    [B, Nq, H, 2hd]."""

    @staticmethod
    def forward(ctx, q, k, v, lam, w, scale, eps, out_scale, head_major):
        q, k, v = (t if t.stride(3) == 1 else t.contiguous() for t in (q, k, v))
        B, Nq, H2, hd = q.shape
        H, D = H2 // 2, 2 * hd
        lam_f = float(lam)
        wf = w.detach().float().contiguous()
        out = torch.empty((B, H, Nq, D) if head_major else (B, Nq, H, D), dtype=q.dtype, device=q.device)
        out4 = out.permute(0, 2, 1, 3) if head_major else out
        vk = ops.vt_pack(v) if q.dtype == torch.bfloat16 else v
        save = any(ctx.needs_input_grad[:5])      # (autograd is off inside forward: the inputs' requires_grad is what counts)
        res = ops.diff_attention(q, k, vk, scale, lam_f, wf, eps, out_scale, out=out4, v_packed=q.dtype == torch.bfloat16, save=save)
        if save:
            lse1, lse2, a1, a2 = res[1]
            ctx.save_for_backward(q, k, v, wf, lse1, lse2, a1, a2)
        ctx.meta = (lam_f, scale, eps, out_scale, head_major)
        return out.view(B * Nq, H * D)

    @staticmethod
    def backward(ctx, dy):
        q, k, v, wf, lse1, lse2, a1, a2 = ctx.saved_tensors
        lam_f, scale, eps, out_scale, head_major = ctx.meta
        B, Nq, H2, hd = q.shape
        Nk, H, D = k.shape[1], H2 // 2, 2 * hd
        dy = _c(dy)
        if dy.dtype != q.dtype:
            dy = ops.convert(dy, q.dtype)
        dy4 = dy.view(B, H, Nq, D).permute(0, 2, 1, 3) if head_major else dy.view(B, Nq, H, D)
        da1, da2, dw, dl = ops.diff_attention_combine_bwd(dy4, a1, a2, lam_f, wf, eps, out_scale)
        dq = torch.empty_like(q, memory_format=torch.contiguous_format)
        dk = torch.empty_like(k, memory_format=torch.contiguous_format)
        dv = None
        for i, (a, da, lse) in enumerate(((a1, da1, lse1), (a2, da2, lse2))):
            qp = q.new_zeros((B, Nq, H, D))
            kp = k.new_zeros((B, Nk, H, D))
            qp[..., :hd].copy_(q[:, :, i * H:(i + 1) * H])
            kp[..., :hd].copy_(k[:, :, i * H:(i + 1) * H])
            dqp, dkp, dvi = ops.attention_bwd(qp, kp, v, a, da, lse, scale)
            dq[:, :, i * H:(i + 1) * H].copy_(dqp[..., :hd])
            dk[:, :, i * H:(i + 1) * H].copy_(dkp[..., :hd])
            dv = dvi if dv is None else dv.add_(dvi)
        return dq, dk, dv, dl.view(()), dw, None, None, None, None


def diff_attention(q, k, v, lam, w, scale, eps, out_scale, head_major=False):
    return DiffAttentionFunction.apply(q, k, v, lam, w, scale, eps, out_scale, head_major)


class MaskScaleFn(Function):
    "x * (mask ? scale : 0): nn.Dropout (one mask byte per element) or DropPath (one per `rows_per_mask` rows); its own backward"

    @staticmethod
    def forward(ctx, x2d, mask, rows_per_mask, scale):
        ctx.save_for_backward(mask)
        ctx.meta = (rows_per_mask, scale)
        return ops.mask_scale(_c(x2d), mask, rows_per_mask, scale)

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return ops.mask_scale(_c(dy), mask, ctx.meta[0], ctx.meta[1]), None, None, None


def _diff_out(x2d, f, gamma, drops):
    "x + drop_path(ls(proj_drop(f))): LayerScale and the sub-layer's drops behind a differential attention's output projection"
    if drops is not None and drops.out is not None:
        f = MaskScaleFn.apply(f, drops.out, 0, drops.out_scale)
    if gamma is not None:
        f = f * gamma.to(f.dtype)
    if drops is not None and drops.path is not None:
        f = MaskScaleFn.apply(f, drops.path, drops.path_rows, drops.path_scale)
    return x2d + f


def diff_lambda(m):
    "lambda_full of a differential attention layer (utils/transformer_blocks.py:793-795), a 0-d fp32 tensor autograd differentiates"
    l1 = torch.exp(torch.sum(m.lambda_q1 * m.lambda_k1, dim=-1).float())
    l2 = torch.exp(torch.sum(m.lambda_q2 * m.lambda_k2, dim=-1).float())
    return l1 - l2 + m.lambda_init


def diff_cross_attn_core(da, hq, hk, hv, B, Nq, Nk, rope, qpos, kpos, dt):
    "DiffCrossAttention on already normalised operands hq [B * Nq, C], hk / hv [B * Nk, C] (dt): projections, RoPE, fused kernel, proj"
    H, hd = da.num_heads, da.head_dim
    q = linear(hq, da.projq.weight, da.projq.bias, da.projq, dt, dt).view(B, Nq, 2 * H, hd)
    k = linear(hk, da.projk.weight, da.projk.bias, da.projk, dt, dt).view(B, Nk, 2 * H, hd)
    v = linear(hv, da.projv.weight, da.projv.bias, da.projv, dt, dt).view(B, Nk, H, 2 * hd)
    q, k = rope2d(q, qpos, rope), rope2d(k, kpos, rope)
    return diff_attention(q, k, v, diff_lambda(da), da.subln.weight, da.scale, da.subln.eps, 1.0 - da.lambda_init)


def diff_self_attn_core(sa, h, B, N, rope, pos, dt):
    "DiffAttention on the normalised operand h [B * N, C] (dt)"
    H, hd = sa.num_heads, sa.head_dim
    C = 2 * H * hd
    t = linear(h, sa.qkv.weight, sa.qkv.bias, sa.qkv, dt, dt).view(B, N, 3 * C)
    q, k = t[:, :, :C].view(B, N, 2 * H, hd), t[:, :, C:2 * C].view(B, N, 2 * H, hd)
    v = t[:, :, 2 * C:].view(B, N, H, 2 * hd)
    q, k = rope2d(q, pos, rope), rope2d(k, pos, rope)
    # head_major: the reference reshapes its [B, H, N, 2hd] result to [B, N, C] without transposing heads and tokens back
    # (utils/transformer_blocks.py:796-800); the kernel writes that memory order directly
    return diff_attention(q, k, v, diff_lambda(sa), sa.subln.weight, sa.scale, sa.subln.eps, 1.0 - sa.lambda_init, head_major=True)


def diff_cross_attn_sublayer(x2d, y2d, ln, lny, da, B, Nq, Nk, rope, qpos, kpos, dt, gamma=None, drops=None):
    "x + ls(proj(DiffCrossAttention core)) with the block's LayerNorms; every step a HIP Function, forward and backward"
    hq = layer_norm(x2d, ln, dt)
    hy = layer_norm(y2d, lny, dt) if lny is not None else convert(y2d, dt)
    o = diff_cross_attn_core(da, hq, hy, hy, B, Nq, Nk, rope, qpos, kpos, dt)
    f = linear(o, da.proj.weight, da.proj.bias, da.proj, dt, x2d.dtype)
    return _diff_out(x2d, f, gamma, drops)


def diff_self_attn_sublayer(x2d, ln, sa, B, N, rope, pos, dt, gamma=None, drops=None):
    h = layer_norm(x2d, ln, dt)
    o = diff_self_attn_core(sa, h, B, N, rope, pos, dt)
    f = linear(o, sa.proj.weight, sa.proj.bias, sa.proj, dt, x2d.dtype)
    return _diff_out(x2d, f, gamma, drops)


# =================================================================================================================
# Summary heads (PoseHead / GlobalHead / MLPHead, prediction_heads/pose_head.py, global_head.py, mlp_head.py): chains of
# 1x1 convolutions / Linear layers with a ReLU and, in the ResConvBlocks, a residual, around one mean over the tokens.
# Every layer is ONE uc_gemm (bias + ReLU + residual in its epilogue).  The layers work on PADDED widths: a hidden width is
# rounded up to HEAD_PAD columns (MLPHead's default 196 -> 256, a patch-14 head's 784 -> 832) by zero rows / columns in the
# prepared weights and zero bias entries, so that the padded activations are exact zeros and every launch meets the K % 64
# of the direct-to-LDS kernels (preact_out, the split weight-gradient kernel); the modules slice the last layer's output.
# =================================================================================================================
HEAD_PAD = 64


def head_pad(n: int, granule: int = HEAD_PAD) -> int:
    return (n + granule - 1) // granule * granule


def _head_w2d(layers):
    return torch.cat([l.weight.detach().reshape(l.weight.shape[0], -1) for l in layers], 0).float()


def head_weights(layers, dt, kp: int, npad: int):
    """(W [npad, kp] in dt, bias fp32 [npad]) of the row-concatenated `layers` (nn.Linear / 1x1 nn.Conv2d; fc_t | fc_rot come out of
    one GEMM), zero-padded, prepared once per weight version; owned by the first layer."""
    def build():
        w = _head_w2d(layers)
        wp = torch.zeros((npad, kp), dtype=dt, device=w.device)
        wp[:w.shape[0], :w.shape[1]].copy_(w)
        bp = torch.zeros(npad, dtype=torch.float32, device=w.device)
        r = 0
        for l in layers:
            if l.bias is not None:
                bp[r:r + l.bias.numel()].copy_(l.bias.detach())
            r += l.weight.shape[0]
        return wp, bp
    srcs = tuple(t for l in layers for t in (l.weight, l.bias))
    return engine.prepared(layers[0], ("head", dt, kp, npad, len(layers)), srcs, build)


def _head_weight_t(layers, dt, kp: int, npad: int):
    def build_2d():
        w = _head_w2d(layers)
        wp = torch.zeros((npad, kp), dtype=torch.float32, device=w.device)
        wp[:w.shape[0], :w.shape[1]].copy_(w)
        return wp
    return _w_t(layers[0], ("head", kp, npad, len(layers)), tuple(l.weight for l in layers), build_2d, dt)


def _head_linear_fwd(x2d, residual, layers, dt, out_dtype, act: Optional[str], npad: int, want_gate: bool):
    """(y [M, npad], gate | None, the operand rows in dt).  gate is what the activation's backward reads: for a ReLU the output itself,
    or — under a residual, where the output no longer tells, and for a GELU always — the pre-activation the same launch stores
    (uc_gemm preact_out)."""
    x2d = _c(x2d)
    xb = x2d if x2d.dtype == dt else ops.convert(x2d, dt)
    w, b = head_weights(layers, dt, xb.shape[1], npad)
    if act is not None and want_gate and (residual is not None or act != "relu"):
        gate = torch.empty((xb.shape[0], npad), dtype=out_dtype, device=xb.device)
        return ops.gemm(xb, w, b, act=act, residual=residual, out_dtype=out_dtype, preact_out=gate), gate, xb
    y = ops.gemm(xb, w, b, act=act, residual=residual, out_dtype=out_dtype)
    return y, (y if act is not None and want_gate else None), xb


@_sink_aware
class HeadLinearFn(Function):
    """y = [act](x W^T + b) [+ residual] (act: "relu" | "gelu" | None) over padded widths, optionally followed by the mean over each sample's T rows
    (pool = (B, T): the ResConvBlock's last convolution and the AdaptiveAvgPool2d(1) after it as one node, whose backward
    writes the ReLU-gated broadcast with uc_token_pool_bwd instead of storing the broadcast map first)."""

    @staticmethod
    def forward(ctx, x2d, residual, layers, dt, out_dtype, act, npad, pool, *params):
        y, gate, xb = _head_linear_fwd(x2d, residual, layers, dt, dt if pool else out_dtype, act, npad, True)
        ctx.save_for_backward(xb, gate)
        ctx.layers, ctx.dt, ctx.act, ctx.npad, ctx.pool, ctx.x_dtype = layers, dt, act, npad, pool, x2d.dtype
        ctx.res_dtype = None if residual is None else residual.dtype
        return ops.token_pool(y, *pool) if pool else y

    @staticmethod
    def backward(ctx, dy):
        xb, gate = ctx.saved_tensors
        layers, dt, npad = ctx.layers, ctx.dt, ctx.npad
        dy = _c(dy)
        dres = None
        if ctx.pool:
            T = ctx.pool[1]
            g = dy if dy.dtype == torch.float32 else ops.convert(dy, torch.float32)
            du = ops.token_pool_bwd(g, T, dt, gate if ctx.act else None)
            if ctx.res_dtype is not None and ctx.needs_input_grad[1]:
                dres = ops.token_pool_bwd(g, T, ctx.res_dtype)
        else:
            if ctx.res_dtype is not None and ctx.needs_input_grad[1]:
                dres = dy if dy.dtype == ctx.res_dtype else ops.convert(dy, ctx.res_dtype)
            du = dy
            if ctx.act:
                du = ops.act_bwd(dy if dy.dtype == gate.dtype else ops.convert(dy, gate.dtype), gate, ctx.act)
        du = _as_dt(_c(du), dt)
        kp = xb.shape[1]
        rows = [l.weight.shape[0] for l in layers]
        K = layers[0].weight[0].numel()
        sink = None
        if sum(rows) == npad and K == kp:
            sink, r = [], 0
            for l, n in zip(layers, rows):
                sink.append((l.weight, r, r + n))
                r += n
        dW, db = _wgrad(du, xb, dt, True, sink=sink)
        grads, r = [], 0
        for l, n in zip(layers, rows):
            grads.append(None if dW is None else dW[r:r + n, :K].reshape(l.weight.shape))
            grads.append(None if l.bias is None else db[r:r + n])
            r += n
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(du, _head_weight_t(layers, dt, kp, npad), out_dtype=ctx.x_dtype)
        return (dx, dres, None, None, None, None, None, None) + tuple(grads)


def head_linear(x2d, layers, dt, out_dtype=None, relu: bool = False, residual=None, npad: Optional[int] = None, pool=None, act: Optional[str] = None):
    """One layer of a summary head on padded widths (see above): x2d [M, Kp] -> [M, npad] in out_dtype (default dt), or the
    fp32 [B, npad] mean over each sample's T rows with pool = (B, T).  `layers`: one nn.Linear / 1x1 nn.Conv2d, or several
    sharing the input (their outputs side by side).  relu / act="relu" | "gelu": the activation in the GEMM's epilogue (the GELU's
    backward reads the pre-activation stored by the same launch, which needs Kp % 64 == 0; no pooled form).  Records a HeadLinearFn
    when a gradient is needed, else only launches."""
    layers = tuple(layers)
    act = act or ("relu" if relu else None)
    N, K = sum(l.weight.shape[0] for l in layers), layers[0].weight[0].numel()
    npad = head_pad(N) if npad is None else npad
    if x2d.shape[1] < K or npad < N or (residual is not None and residual.shape[1] != npad):
        raise UcHipError(f"head_linear: operand width {x2d.shape[1]} / padded output width {npad} do not fit a [{N}, {K}] layer")
    if act not in (None, "relu", "gelu") or (pool and act == "gelu"):
        raise UcHipError(f"head_linear: act={act!r}{' with a pooled output' if pool else ''} has no HIP path")
    params = tuple(t for l in layers for t in (l.weight, l.bias))
    if grad_needed(x2d, residual, *params):
        return HeadLinearFn.apply(x2d, residual, layers, dt, out_dtype or dt, act, npad, pool, *params)
    y, _, _ = _head_linear_fwd(x2d, residual, layers, dt, dt if pool else (out_dtype or dt), act, npad, False)
    return ops.token_pool(y, *pool) if pool else y


@_sink_aware
class TokenPoolFn(Function):
    "mean over each sample's T rows (nn.AdaptiveAvgPool2d(1) on the token matrix); backward: the broadcast of uc_token_pool_bwd."

    @staticmethod
    def forward(ctx, x2d, B, T):
        ctx.T, ctx.x_dtype = T, x2d.dtype
        return ops.token_pool(x2d, B, T)

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        return ops.token_pool_bwd(dy if dy.dtype == torch.float32 else ops.convert(dy, torch.float32), ctx.T, ctx.x_dtype), None, None


def token_pool(x2d, B: int, T: int):
    return TokenPoolFn.apply(x2d, B, T) if grad_needed(x2d) else ops.token_pool(x2d, B, T)


# =================================================================================================================
# MoGe convolutional head (prediction_heads/moge_conv.py) and MLPFeature (prediction_heads/mlp_feature.py).
# GroupNorm (+ ReLU), the replicate-padded 3x3 convolution as pad -> zero-padded conv on the (H + 2) x (W + 2) map -> crop
# (+ residual, + ReLU), the half-pixel resize, the channel-padded forms of the transposed and the 3x3 convolution (the two UV
# channels make the channel counts 514 / 258 / 130 / 66: zero-padded to the GEMM's granule, the zero columns built into the
# prepared weights), the sum of the 1x1 projections as one GEMM over K-concatenated operands, and the Mlp of MLPFeature.
# =================================================================================================================
def check_group_size(C: int, G: int, what: str = "group_norm", group4: bool = False) -> None:
    "what uc_group_norm_nhwc (group4: uc_group_norm_silu_nhwc, which also takes 4 channels per group) would reject, said before any tensor is touched"
    if G <= 0 or C % G != 0 or ((C // G) % 8 != 0 and not (group4 and C // G == 4)):
        raise UcHipError(f"{what}: {C} channels in {G} groups: channels per group ({C / max(G, 1):g}) must be a multiple of 8 "
                         + ("or 4 (uc_group_norm_silu_nhwc)" if group4 else "(uc_group_norm_nhwc)"))


@_sink_aware
class GroupNormFn(Function):
    """y = act(GroupNorm(x)) on an NHWC map, act in ("none", "relu", "silu") (uc_group_norm_nhwc / uc_group_norm_silu_nhwc and their
    _bwd).  The ReLU's backward gates on the saved output; the SiLU's recomputes the pre-activation from x and beta."""

    @staticmethod
    def forward(ctx, x, weight, bias, gn, act):
        x = _c(x)
        g, b = engine.ln_params(gn)
        if act == "silu":
            y, mean, rstd = ops.group_norm_silu_nhwc(x, g, b, gn.num_groups, gn.eps)
        else:
            y, mean, rstd = ops.group_norm_nhwc(x, g, b, gn.num_groups, gn.eps, act == "relu")
        ctx.save_for_backward(x, g, mean, rstd, {"none": torch.empty(0), "relu": y, "silu": b}[act])
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, mean, rstd, aux = ctx.saved_tensors
        dy = _as_dt(_c(dy), x.dtype)
        if ctx.act == "silu":
            dx, dg, db = ops.group_norm_silu_nhwc_bwd(dy, x, mean, rstd, g, aux)
        else:
            dx, dg, db = ops.group_norm_nhwc_bwd(dy, x, mean, rstd, g, gate=aux if ctx.act == "relu" else None)
        return dx, dg, db, None, None


def _group_norm(x, gn, act: str, what: str):
    check_group_size(x.shape[-1], gn.num_groups, what, group4=act == "silu")
    if gn.weight is None:
        raise UcHipError(f"{what}: GroupNorm(affine=False) has no HIP path")
    return GroupNormFn.apply(x, gn.weight, gn.bias, gn, act)


def group_norm(x, gn, relu: bool):
    return _group_norm(x, gn, "relu" if relu else "none", "group_norm")


def group_norm_silu(x, gn):
    return _group_norm(x, gn, "silu", "group_norm_silu")


@_sink_aware
class ReplicatePadFn(Function):
    @staticmethod
    def forward(ctx, x):
        return ops.replicate_pad_nhwc(_c(x))

    @staticmethod
    def backward(ctx, dy):
        return ops.replicate_pad_nhwc_bwd(_c(dy))


@_sink_aware
class CropAddFn(Function):
    "act(padded[:, 1:-1, 1:-1] (+ residual)); the ReLU's backward gates on the output."

    @staticmethod
    def forward(ctx, xp, residual, relu):
        y = ops.crop_add_nhwc(_c(xp), None if residual is None else _c(residual), relu)
        ctx.save_for_backward(y if relu else torch.empty(0))
        ctx.meta = (relu, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        relu, has_res = ctx.meta
        dy = _c(dy)
        g = ops.act_bwd(dy, y, "relu") if relu else dy
        return ops.crop_embed_nhwc(g), (g if has_res else None), None


@_sink_aware
class ResizeBilinearFn(Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo, align_corners):
        x = _c(x)
        ctx.geom = (x.shape[1], x.shape[2], align_corners)
        return ops.resize_bilinear_nhwc(x, Ho, Wo, align_corners)

    @staticmethod
    def backward(ctx, dy):
        Hi, Wi, ac = ctx.geom
        return ops.resize_bilinear_nhwc_bwd(_c(dy), Hi, Wi, ac), None, None, None


def resize_bilinear(x, Ho: int, Wo: int, align_corners: bool):
    return ResizeBilinearFn.apply(x, Ho, Wo, align_corners)


def check_conv3x3_replicate(conv) -> None:
    if conv.padding_mode != "replicate":
        raise UcHipError(f"conv3x3_replicate: padding_mode={conv.padding_mode!r} has no HIP path (supported: 'replicate')")
    if conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1:
        raise UcHipError("conv3x3_replicate: only a dense 3x3 convolution of stride 1 has a HIP path")


def replicate_pad(x):
    "[B, H, W, C] -> [B, H + 2, W + 2, C], border pixels repeated; differentiable"
    return ReplicatePadFn.apply(x)


def conv3x3_replicate(x, conv, residual=None, relu_out: bool = False, out_dtype=None, padded: bool = False):
    """Conv2d(k=3, padding=1, padding_mode="replicate") on an NHWC map: pad -> zero-padded convolution on the (H + 2) x (W + 2) map ->
    crop (+ residual, + ReLU).  x may carry zero channels beyond conv.in_channels; the result has head_pad(conv.out_channels, 8)
    channels (zero beyond the real ones).  padded: x is already the replicate-padded map (several convolutions of one map share
    one pad pass and one adjoint)."""
    check_conv3x3_replicate(conv)
    xp = x if padded else ReplicatePadFn.apply(x)
    yp = Conv3x3Fn.apply(xp, conv.weight, conv.bias, None, None, conv, False, None, None, head_pad(conv.out_channels, 8), out_dtype)
    return CropAddFn.apply(yp, residual, relu_out)


def _cat_k_weights(layers, dt):
    "(W [N, sum K_i] in dt, sum of the biases fp32) of 1x1 convolutions whose outputs are added: one GEMM over K-concatenated operands"
    def build():
        w = torch.cat([l.weight.detach().reshape(l.weight.shape[0], -1).float() for l in layers], 1).to(dt).contiguous()
        bs = [l.bias.detach().float() for l in layers if l.bias is not None]
        return w, (torch.stack(bs, 0).sum(0).contiguous() if bs else None)
    return engine.prepared(layers[0], ("catk", dt, len(layers)), tuple(t for l in layers for t in (l.weight, l.bias)), build)


@_sink_aware
class SumLinearFn(Function):
    "sum_i (x_i W_i^T + b_i) as one GEMM: x2d = [x_0 | x_1 | ...] (K-concatenated rows), params = weights then biases."

    @staticmethod
    def forward(ctx, x2d, layers, dt, *params):
        x2d = _c(x2d)
        xb = x2d if x2d.dtype == dt else ops.convert(x2d, dt)
        w, b = _cat_k_weights(layers, dt)
        ctx.save_for_backward(xb)
        ctx.meta = (layers, dt, x2d.dtype)
        return ops.gemm(xb, w, b)

    @staticmethod
    def backward(ctx, dy):
        (xb,) = ctx.saved_tensors
        layers, dt, x_dtype = ctx.meta
        dyb = _as_dt(_c(dy), dt)
        has_b = any(l.bias is not None for l in layers)
        dW, db = _wgrad(dyb, xb, dt, has_b)
        dws, k0 = [], 0
        for l in layers:
            k1 = k0 + l.weight[0].numel()
            dws.append(dW[:, k0:k1].reshape(l.weight.shape))
            k0 = k1
        dx = None
        if ctx.needs_input_grad[0]:
            wT = _w_t(layers[0], ("catk", len(layers)), tuple(l.weight for l in layers),
                      lambda: torch.cat([l.weight.detach().reshape(l.weight.shape[0], -1).float() for l in layers], 1).contiguous(), dt)
            dx = ops.gemm(dyb, wT, out_dtype=x_dtype)
        return (dx, None, None, *dws, *[(db if l.bias is not None else None) for l in layers])


def sum_linear(x2d, layers, dt):
    layers = tuple(layers)
    return SumLinearFn.apply(x2d, layers, dt, *[l.weight for l in layers], *[l.bias for l in layers])


@_sink_aware
class MlpFn(Function):
    "fc2(act(fc1(x))) on token rows: MlpSubLayerFn without the LayerNorm and the residual (MLPFeature's Mlp, mlp_feature.py:57-63)."

    @staticmethod
    def forward(ctx, x2d, w1_, b1_, w2_, b2_, fc1, fc2, act, dt, drops=None):
        x2d = _c(x2d)
        h = x2d if x2d.dtype == dt else ops.convert(x2d, dt)
        w1, b1 = engine.lin_weights(fc1, dt)
        w2, b2 = engine.lin_weights(fc2, dt)
        if act != "none" and (dt == torch.float32 or (dt == torch.bfloat16 and h.shape[1] % 64 == 0)):
            u = torch.empty((h.shape[0], w1.shape[0]), dtype=dt, device=h.device)
            a = ops.gemm(h, w1, b1, act=act, preact_out=u)
        elif act != "none" and any(ctx.needs_input_grad):      # K off the direct-to-LDS granule: the pre-activation from its own launch
            u = ops.gemm(h, w1, b1)
            a = ops.gemm(h, w1, b1, act=act)
        else:
            u = a = ops.gemm(h, w1, b1, act=act)
        if drops is not None and drops.mid is not None:
            a = ops.mask_scale(a, drops.mid, 0, drops.mid_scale)
        out = ops.gemm(a, w2, b2)
        if drops is not None and drops.has_out:
            out = _drop_out(out, drops)
        masks, dspec = _drops_saved(drops)
        ctx.save_for_backward(h, u, a, *masks)
        ctx.meta = (fc1, fc2, act, dt, x2d.dtype, b1_ is not None, b2_ is not None, dspec)
        return out

    @staticmethod
    def backward(ctx, dy):
        fc1, fc2, act, dt, x_dtype, has_b1, has_b2, dspec = ctx.meta
        drops, (h, u, a) = _drops_restore(dspec, ctx.saved_tensors)
        dyb = _as_dt(_c(dy), dt)
        if drops is not None and drops.has_out:
            dyb = _drop_out(dyb, drops)
        dW2, db2, _, du, dW1, db1 = _mlp_bwd(dyb, h, u, a, fc1, fc2, None, act, dt, has_b1, has_b2, drops)
        dx = ops.gemm(du, lin_weight_t(fc1, dt), out_dtype=x_dtype) if ctx.needs_input_grad[0] else None
        return (dx, dW1, db1, dW2, db2) + (None,) * 5


def mlp(x2d, fc1, fc2, act, dt, drops=None):
    return MlpFn.apply(x2d, fc1.weight, fc1.bias, fc2.weight, fc2.bias, fc1, fc2, act, dt, drops)


# =================================================================================================================
# Non-image input encoders (encoders/patch_embedder.py, dense_rep_encoder.py, global_rep_encoder.py): PixelUnshuffle as operand rows,
# the activation around the residual sum, and LN2(LN1(x) + pe) in one pass.  Channel counts are zero-padded to ENC_PAD (the Cin % 64 /
# K % 64 granule of the direct-to-LDS routes) in the prepared weights and in the activations; zero weight rows and zero bias entries
# keep the padded channels exactly zero through bias, GELU(0) = ReLU(0) = 0 and the residual sum.
# =================================================================================================================
ENC_PAD = 64


@_sink_aware
class UnshuffleRowsFn(Function):
    "rows [B h w, ld] in dt = PixelUnshuffle(P)(img [B, C, h P, w P]), columns beyond C P P zero; the backward is the inverse permutation"

    @staticmethod
    def forward(ctx, img, P, ld, dt):
        ctx.geom = (tuple(img.shape), P, img.dtype)
        img = _c(img if img.dtype in (torch.float32, torch.bfloat16) else img.float())
        return ops.unshuffle_rows(img, P, ld, dt)

    @staticmethod
    def backward(ctx, dy):
        (B, Cn, H, W), P, idt = ctx.geom
        dimg = ops.unshuffle_rows_bwd(_c(dy), B, Cn, H // P, W // P, P)
        return (dimg if idt == torch.float32 else dimg.to(idt)), None, None, None


def unshuffle_rows(img, P: int, ld: int, dt):
    if grad_needed(img):
        return UnshuffleRowsFn.apply(img, P, ld, dt)
    return ops.unshuffle_rows(_c(img if img.dtype in (torch.float32, torch.bfloat16) else img.float()), P, ld, dt)


@_sink_aware
class ActFn(Function):
    "y = act(u) as a pass of its own (the activation AFTER a residual sum; uc_gemm's epilogues apply theirs before it); saves u"

    @staticmethod
    def forward(ctx, u, name):
        u = _c(u)
        ctx.save_for_backward(u)
        ctx.name = name
        return ops.act(u, name)

    @staticmethod
    def backward(ctx, dy):
        (u,) = ctx.saved_tensors
        return ops.act_bwd(_as_dt(_c(dy), u.dtype), u, ctx.name), None


def act(u, name: str):
    "act(u), name in ('gelu', 'relu'); without a graph the pass runs in place on u (which must be the caller's own temporary)"
    if grad_needed(u):
        return ActFn.apply(u, name)
    u = _c(u)
    return ops.act(u, name, out=u)


def conv3x3_padded(x, conv, cout_pad: int, out_dtype=None, residual=None):
    "Conv2d(k=3, padding=1) on an NHWC map with zero-padded channel counts (Conv3x3Fn), residual added in the epilogue"
    if conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.padding != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1 \
            or conv.padding_mode != "zeros":
        raise UcHipError("conv3x3_padded: only a dense zero-padded 3x3 convolution of stride 1 has a HIP path")
    return Conv3x3Fn.apply(x, conv.weight, conv.bias, residual, None, conv, False, None, None, cout_pad, out_dtype or x.dtype)


def _ln_args(ln):
    "(gamma, beta, eps) fp32 of an nn.LayerNorm, None for Identity / None"
    if ln is None or isinstance(ln, nn.Identity):
        return None
    g, b = engine.ln_params(ln)
    return g, b, ln.eps


@_sink_aware
class LnPeLnFn(Function):
    """y = LN2(LN1(x) + pe) over rows [B N, C] in one kernel (uc_ln_pe_ln), each step optional.  The backward is composed:
    uc_layernorm_bwd on the saved LN2 input, uc_colsum over the batch ([B, N C]) for pe, uc_layernorm_bwd on x.  The one case the
    existing kernels cannot express is a REPRODUCIBLE dgamma / dbeta (uc_layernorm_bwd adds them with fp32 atomics): those come from
    uc_ln_param_grads, in a fixed order, and uc_layernorm_bwd's own are discarded."""

    @staticmethod
    def forward(ctx, x2d, pe, g1, b1, g2, b2, B, N, eps1, eps2, out_dtype):
        x2d = _c(x2d)
        if x2d.dtype not in (torch.float32, torch.bfloat16):
            raise UcHipError("ln_pe_ln: the token rows are fp32 or bf16")
        f = lambda t: None if t is None else t.detach().float().contiguous()      # noqa: E731
        pe_, g1_, b1_, g2_, b2_ = f(pe), f(g1), f(b1), f(g2), f(b2)
        ln1 = None if g1 is None else (g1_, b1_, eps1)
        ln2 = None if g2 is None else (g2_, b2_, eps2)
        if ln2 is not None:
            y, mid = ops.ln_pe_ln(x2d, B, N, ln1, pe_, ln2, out_dtype, want_mid=True)
        else:
            y, mid = ops.ln_pe_ln(x2d, B, N, ln1, pe_, None, out_dtype), None
        ctx.save_for_backward(x2d if ln1 is not None else None, mid, g1_, g2_)
        ctx.meta = (B, N, eps1, eps2, x2d.dtype, pe is not None and tuple(pe.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        x2d, mid, g1, g2 = ctx.saved_tensors
        B, N, eps1, eps2, x_dtype, pe_shape = ctx.meta
        d = _c(dy)
        dg1 = db1 = dg2 = db2 = dpe = None
        if g2 is not None:
            dg2, db2 = ops.ln_param_grads(mid, d, eps2)
            d = ops.layernorm_bwd(mid, g2, d, eps2, torch.zeros_like(g2), torch.zeros_like(g2))       # fp32 (mid's dtype)
        if pe_shape and ctx.needs_input_grad[1]:
            d32 = d if d.dtype == torch.float32 else ops.convert(d, torch.float32)
            dpe = _colsum(d32.view(B, -1)).view(pe_shape)
        if g1 is not None:
            dg1, db1 = ops.ln_param_grads(x2d, d, eps1)
            dx = ops.layernorm_bwd(x2d, g1, d, eps1, torch.zeros_like(g1), torch.zeros_like(g1))
        else:
            dx = d if d.dtype == x_dtype else ops.convert(d, x_dtype)
        return dx, dpe, dg1, db1, dg2, db2, None, None, None, None, None


def ln_pe_ln(x2d, B: int, N: int, ln1, pe, ln2, out_dtype=torch.float32):
    """LN2(LN1(x2d) + pe): ln1 / ln2 an nn.LayerNorm, nn.Identity or None; pe [N, C] (any float dtype; may require grad) or None.
    With nothing to apply the rows are returned as they are (converted to out_dtype)."""
    a1, a2 = _ln_args(ln1), _ln_args(ln2)
    if a1 is None and a2 is None and pe is None:
        return x2d if x2d.dtype == out_dtype else convert(x2d, out_dtype)
    p1 = (ln1.weight, ln1.bias) if a1 is not None else (None, None)
    p2 = (ln2.weight, ln2.bias) if a2 is not None else (None, None)
    if grad_needed(x2d, pe, *p1, *p2):
        return LnPeLnFn.apply(x2d, pe, p1[0], p1[1], p2[0], p2[1], B, N, a1[2] if a1 else 0.0, a2[2] if a2 else 0.0, out_dtype)
    pe_ = None if pe is None else (pe if pe.dtype == torch.float32 and pe.is_contiguous() else pe.float().contiguous())
    return ops.ln_pe_ln(_c(x2d), B, N, a1, pe_, a2, out_dtype)


@_sink_aware
class VitStemFn(Function):
    """y = LN(cat(cls, tok) + pos) in one kernel (uc_vit_stem) and its adjoint in one (uc_vit_stem_bwd): the token gradient, and the
    gradients of the class embedding, the position table and the norm's parameters from fixed-order sums."""

    @staticmethod
    def forward(ctx, tok, cls, pos, gamma, beta, eps, out_dtype):
        tok = _c(tok)
        if tok.dtype not in (torch.float32, torch.bfloat16):
            raise UcHipError("vit_stem: the patch tokens are fp32 or bf16")
        f = lambda t: None if t is None else t.detach().float().contiguous()      # noqa: E731
        cls_, pos_, g_, b_ = f(cls), f(pos), f(gamma), f(beta)
        y, stats = ops.vit_stem(tok, cls_, pos_, None if g_ is None else (g_, b_, eps), out_dtype, want_stats=True)
        ctx.save_for_backward(tok, cls_, pos_, g_, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        tok, cls_, pos_, g_, stats = ctx.saved_tensors
        dtok, dcls, dpos, dg, db = ops.vit_stem_bwd(_c(dy), tok, cls_, pos_, g_, stats, need_dtok=ctx.needs_input_grad[0])
        return dtok, dcls, dpos, dg, db, None, None


def vit_stem(tok, cls, pos, ln, out_dtype=torch.float32):
    """LN(cat(cls, tok) + pos): tok [B, hw, C]; cls [C] or None; pos [hw + (cls is not None), C] or None; ln an nn.LayerNorm,
    nn.Identity or None.  Returns [B, T, C] in out_dtype."""
    a = _ln_args(ln)
    p = (ln.weight, ln.bias) if a is not None else (None, None)
    if grad_needed(tok, cls, pos, *p):
        return VitStemFn.apply(tok, cls, pos, p[0], p[1], a[2] if a else 0.0, out_dtype)
    f = lambda t: None if t is None else (t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous())      # noqa: E731
    return ops.vit_stem(_c(tok), f(cls), f(pos), a, out_dtype)


# =================================================================================================================
# Cosmos continuous image tokenizer (libs/cosmos_tokenizer, encoders/cosmos.py, prediction_heads/cosmos.py): the Haar patcher and its
# inverse, GroupNorm + SiLU, the stride-2 Downsample convolution as operand gather + dense GEMM, the nearest x2 upsample, and the
# single-head attention over all pixels (head_dim 512) assembled from uc_gemm, the row softmax and uc_gemm_tn.
# =================================================================================================================
@_sink_aware
class HaarPatchFn(Function):
    "fp32 NCHW image -> NHWC two-level Haar coefficients (16 C channels, zero-padded to ld); the adjoint is the inverse / 16"

    @staticmethod
    def forward(ctx, img, dt, ld):
        img = _c(img)
        ctx.Cn = img.shape[1]
        return ops.haar_patch(img if img.dtype == torch.float32 else img.float(), dt, ld)

    @staticmethod
    def backward(ctx, dy):
        return ops.haar_unpatch(_c(dy), ctx.Cn, 1.0 / 16.0), None, None


def haar_patch(img, dt, ld=None):
    return HaarPatchFn.apply(img, dt, ld)


@_sink_aware
class HaarUnpatchFn(Function):
    "NHWC coefficients [B, h, w, ld >= 16 Cn] -> fp32 NCHW image [B, Cn, 4h, 4w]; the adjoint is 16 x the patcher"

    @staticmethod
    def forward(ctx, rows, Cn):
        rows = _c(rows)
        ctx.meta = (rows.dtype, rows.shape[-1])
        return ops.haar_unpatch(rows, Cn)

    @staticmethod
    def backward(ctx, dy):
        dt, ld = ctx.meta
        return ops.haar_patch(_c(dy), dt, ld, 16.0), None


def haar_unpatch(rows, Cn: int):
    return HaarUnpatchFn.apply(rows, Cn)


@_sink_aware
class Down2ConvFn(Function):
    """The tokenizer's Downsample: F.pad(x, (0, 1, 0, 1)) + Conv2d(k = 3, stride = 2, padding = 0) on an NHWC map, as operand rows
    (uc_down2_gather) times the [Cout, 9 Cin] weight.  The backward regathers the rows for the weight gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, conv):
        x = _c(x)
        B, H, W, Cin = x.shape
        w, b = engine.conv3x3_weights(conv, x.dtype)
        ctx.save_for_backward(x)
        ctx.meta = (conv, bias is not None)
        return ops.gemm(ops.down2_gather(x), w, b).view(B, H // 2, W // 2, -1)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        conv, has_b = ctx.meta
        B, H, W, Cin = x.shape
        dt = x.dtype
        dy2 = _as_dt(_c(dy), dt).view(-1, conv.out_channels)
        dWg, db = _wgrad(dy2, ops.down2_gather(x), dt, has_b)
        dW = dWg.view(conv.out_channels, 3, 3, Cin).permute(0, 3, 1, 2)
        dx = None
        if ctx.needs_input_grad[0]:
            drows = ops.gemm(dy2, _w_t(conv, "down2", (conv.weight,), lambda: engine.conv3x3_weight2d(conv.weight), dt))
            dx = ops.down2_gather_bwd(drows, B, H, W)
        return dx, dW, db, None


def down2_conv(x, conv):
    if conv.kernel_size != (3, 3) or conv.stride != (2, 2) or conv.padding != (0, 0) or conv.dilation != (1, 1) or conv.groups != 1:
        raise UcHipError("down2_conv: only the 3x3 / stride-2 / unpadded convolution of the tokenizer's Downsample has a HIP path")
    if x.shape[1] % 2 or x.shape[2] % 2:
        raise UcHipError(f"down2_conv: the Downsample of an odd map ({x.shape[1]} x {x.shape[2]}) has no HIP path")
    return Down2ConvFn.apply(x, conv.weight, conv.bias, conv)


@_sink_aware
class Upsample2Fn(Function):
    "nearest-neighbour x2 on an NHWC map; the adjoint sums every 2x2 block in a fixed order"

    @staticmethod
    def forward(ctx, x):
        return ops.upsample2_nhwc(_c(x))

    @staticmethod
    def backward(ctx, dy):
        return ops.upsample2_nhwc_bwd(_c(dy))


def upsample2(x):
    return Upsample2Fn.apply(x)


WIDE_ATTN_PANEL = 4096      # query rows per score panel: the fp32 score buffer holds at most PANEL x N_pad values


def _wide_attn_operands(rows, N: int, C: int):
    "(k, v zero-padded to a multiple of 64 rows, contiguous) of one sample's qkv rows [N, 3C]"
    Np = head_pad(N)
    kp = rows.new_zeros((Np, C))
    vp = rows.new_zeros((Np, C))
    kp[:N].copy_(rows[:, C:2 * C])
    vp[:N].copy_(rows[:, 2 * C:])
    return kp, vp, Np


def _wide_attn_probs(q, kp, N: int, Np: int, scale: float):
    "P [n, Np] (zeros beyond N) of one panel of query rows q [n, C]: S = q k^T (uc_gemm) -> row softmax"
    s = ops.gemm(q, kp, out_dtype=torch.float32)
    return ops.softmax_rows(s[:, :N], scale, q.dtype, out=torch.empty((q.shape[0], Np), dtype=q.dtype, device=q.device))


@_sink_aware
class WideAttentionFn(Function):
    """softmax(q k^T scale) v with ONE head over all N pixels of a sample (head_dim = C = 512: beyond the fused kernels), assembled from
    uc_gemm, uc_softmax_rows, uc_transpose2d and uc_gemm_tn per sample and per panel of at most `panel` query rows.  qkv: [B N, 3C]
    rows (q | k | v).  P is NOT saved: the backward recomputes each panel's scores and probabilities (two launches) instead of keeping
    B N^2 values alive."""

    @staticmethod
    def forward(ctx, qkv, B, N, scale, panel):
        qkv = _c(qkv)
        C = qkv.shape[1] // 3
        o = torch.empty((B * N, C), dtype=qkv.dtype, device=qkv.device)
        for b in range(B):
            rows = qkv[b * N:(b + 1) * N]
            kp, vp, Np = _wide_attn_operands(rows, N, C)
            vt = ops.transpose2d(vp)                                   # [C, Np]
            for r0 in range(0, N, panel):
                r1 = min(N, r0 + panel)
                p = _wide_attn_probs(rows[r0:r1, :C], kp, N, Np, scale)
                ops.gemm(p, vt, out=o[b * N + r0:b * N + r1])
        ctx.save_for_backward(qkv)
        ctx.meta = (B, N, scale, panel)
        return o

    @staticmethod
    def backward(ctx, do):
        (qkv,) = ctx.saved_tensors
        B, N, scale, panel = ctx.meta
        C = qkv.shape[1] // 3
        dt = qkv.dtype
        do = _as_dt(_c(do), dt)
        dqkv = torch.empty_like(qkv)
        for b in range(B):
            rows, drows = qkv[b * N:(b + 1) * N], dqkv[b * N:(b + 1) * N]
            kp, vp, Np = _wide_attn_operands(rows, N, C)
            kt = ops.transpose2d(kp)                                   # [C, Np]
            dk = dv = None
            for r0 in range(0, N, panel):
                r1 = min(N, r0 + panel)
                q, g = rows[r0:r1, :C], do[b * N + r0:b * N + r1]
                p = _wide_attn_probs(q, kp, N, Np, scale)
                dp = ops.gemm(g, vp, out_dtype=torch.float32)          # dP = dO v^T  [n, Np]
                ds = ops.softmax_rows_bwd(p, dp[:, :N], N, scale)      # [n, Np], zeros beyond N
                ops.gemm(ds, kt, out=drows[r0:r1, :C])                 # dQ = dS k
                dvp, dkp = _wgrad(p, g, dt)[0], _wgrad(ds, q, dt)[0]   # dV = P^T dO, dK = dS^T q  [Np, C] fp32
                dv, dk = (dvp, dkp) if dv is None else (dv + dvp, dk + dkp)      # (panels in ascending order)
            drows[:, C:2 * C].copy_(dk[:N])
            drows[:, 2 * C:].copy_(dv[:N])
        return dqkv, None, None, None, None


def wide_attention(qkv, B: int, N: int, scale: float, panel: int = WIDE_ATTN_PANEL):
    "single-head attention over all pixels: qkv [B N, 3C] -> [B N, C] (WideAttentionFn); panel: query rows per score panel"
    if qkv.dim() != 2 or qkv.shape[0] != B * N or qkv.shape[1] % 3 != 0 or (qkv.shape[1] // 3) % 64 != 0:
        raise UcHipError(f"wide_attention: qkv {tuple(qkv.shape)} is not [B N, 3C] with C a multiple of 64 (B={B}, N={N})")
    if panel < 1:
        raise UcHipError(f"wide_attention: panel={panel}")
    return WideAttentionFn.apply(qkv, B, N, float(scale), int(panel))


# =================================================================================================================
# DINOv3 ConvNeXt (encoders/dinov3.py): the depthwise 7x7 convolution and the operand rows of the stage downsample
# =================================================================================================================
def dwconv7x7_weights(conv):
    "(fp32 [49, C] tap-major, fp32 bias [C] | None) of nn.Conv2d(C, C, 7, padding=3, groups=C), prepared once per weight version"
    return engine.prepared(conv, "dw49", (conv.weight, conv.bias),
                           lambda: (conv.weight.detach().float().reshape(conv.out_channels, 49).t().contiguous(),
                                    None if conv.bias is None else conv.bias.detach().float().contiguous()))


def check_dwconv7x7(conv) -> None:
    if (conv.kernel_size != (7, 7) or conv.stride != (1, 1) or conv.padding != (3, 3) or conv.dilation != (1, 1)
            or conv.groups != conv.in_channels or conv.out_channels != conv.in_channels or conv.padding_mode != "zeros"):
        raise UcHipError("dwconv7x7: only the zero-padded depthwise 7x7 convolution of stride 1 has a HIP path (uc_dwconv7x7_nhwc)")
    if conv.in_channels % 8:
        raise UcHipError(f"dwconv7x7: {conv.in_channels} channels: uc_dwconv7x7_nhwc takes multiples of 8")


@_sink_aware
class DwConv7x7(Function):
    """Depthwise 7x7 / padding 3 convolution on an NHWC map (uc_dwconv7x7_nhwc).  Backward: the data gradient is the same kernel on dy
    with the taps read in reverse (flip: no flipped copy of weights that change every step), the weight and bias gradients are
    uc_dwconv7x7_nhwc_wgrad (two fixed-order stages)."""

    @staticmethod
    def forward(ctx, x, weight, bias, conv):
        x = _c(x)
        w, b = dwconv7x7_weights(conv)
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return ops.dwconv7x7_nhwc(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _as_dt(_c(dy), x.dtype)
        dx = ops.dwconv7x7_nhwc(dy, w, None, flip=True) if ctx.needs_input_grad[0] else None
        dw, db = ops.dwconv7x7_nhwc_wgrad(x, dy, bias=ctx.has_bias)
        return dx, dw.t().reshape(-1, 1, 7, 7), db, None


def dwconv7x7(x, conv):
    "x NHWC [B, H, W, C] -> conv(x), same shape and dtype"
    check_dwconv7x7(conv)
    return DwConv7x7.apply(x, conv.weight, conv.bias, conv)


@_sink_aware
class Patch2Gather(Function):
    "operand rows [B (H//2) (W//2), 4 C] of Conv2d(k = 2, stride = 2) on an NHWC map, K ordered (ky, kx, c); the adjoint is a permutation"

    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        ctx.geom = tuple(x.shape[:3])
        return ops.patch2_gather_nhwc(x)

    @staticmethod
    def backward(ctx, drows):
        return ops.patch2_gather_nhwc_bwd(_c(drows), *ctx.geom)


def patch2_gather(x):
    return Patch2Gather.apply(x)
