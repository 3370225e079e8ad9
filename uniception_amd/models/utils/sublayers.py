"""The pre-LN residual sub-layers every block is a list of: x + drop_path(ls(drop(f(LN(x))))).

A block passes modules and numbers; the runner decides.  With `train` (the block's one autograd.grad_needed) a sub-layer is its
autograd.*_sublayer Function (HIP forward + HIP backward, LayerScale as `gamma`, the masks as `drops`).  Without it: engine.ln_operand
hands the LayerNorm over (stand-alone kernel, or the producer's bf16 twin + row statistics folded into the first GEMM), the engine.*
pipeline adds the residual in its last GEMM's epilogue and emits the next LayerNorm's twin / statistics, and a LayerScale is folded
into that GEMM's weights (no kernel work).  The helpers build what a block hands in: gamma_of, drops_for / attn_drop_for (which draw from
PyTorch's generator, so a block calls them in its own fixed order) and the one refusal of masks without gradients.
"""
import torch.nn as nn

from ... import autograd, engine


def gamma_of(ls):
    "The parameter of a LayerScale container, or None (nn.Identity: the block was built without init_values)."
    return getattr(ls, "gamma", None)


def as_dt(x2d, dt):
    return x2d if x2d.dtype == dt else engine.ops.convert(x2d, dt)


def refuse_drops(training: bool, train: bool, *rates) -> None:
    "Train mode without gradients: the inference pipelines apply no masks, so any rate > 0 has no HIP form."
    if training and not train and any(p > 0.0 for p in rates):
        raise engine.UcHipError("dropout / attn_drop / DropPath > 0 in train mode without gradients has no HIP form "
                                "(the inference kernels apply no masks)")


def drops_for(training: bool, train: bool, x2d, B: int, N: int, p_out: float, path, p_mid: float = 0.0, hidden: int = 0):
    """One sub-layer's autograd.Drops, or None (eval mode, no gradients, every rate 0).  p_out: the rate of the nn.Dropout on the
    sub-layer's output; path: the block's DropPath or nn.Identity; p_mid / hidden: an Mlp's drop1 rate and hidden width."""
    if not training:       # (the inference hot path: nothing to draw, nothing to refuse)
        return None
    p_path, scale_by_keep = getattr(path, "drop_prob", 0.0), getattr(path, "scale_by_keep", True)
    refuse_drops(training, train, p_out, p_path, p_mid)
    return autograd.make_drops(train, x2d.device, B, N, x2d.shape[1], p_out=p_out, p_path=p_path, hidden=hidden,
                               p_mid=p_mid, scale_by_keep=scale_by_keep)


def attn_drop_for(training: bool, train: bool, p: float):
    "(p, seed) of one attention sub-layer's dropout inside the attention kernels, or None."
    if not training:
        return None
    refuse_drops(training, train, p)
    return autograd.attn_dropout(train, p)


def _ls_wb(lin, g, dt):
    return None if g is None else engine.layerscale_lin_weights(lin, g, dt)


def self_attn(x2d, norm, qkv, proj, B, N, heads, rope, pos, scale, dt, *, train, gamma=None, q_norm=None, k_norm=None, drops=None,
              attn_drop=None):
    "x + ls(proj(SDPA(rope(q), rope(k), v))), q | k | v = qkv(norm(x)) over the N tokens of each of the B sequences"
    if train:
        return autograd.self_attn_sublayer(x2d, norm, qkv, proj, B, N, heads, rope, pos, scale, dt, gamma=gamma, q_norm=q_norm,
                                           k_norm=k_norm, drops=drops, attn_drop=attn_drop)
    h, fold = engine.ln_operand(x2d, norm, dt)
    return engine.self_attention(h, B, N, qkv, proj, heads, rope, pos, scale, x2d, x2d.dtype, proj_wb=_ls_wb(proj, gamma, dt), fold=fold,
                                 emit_ln=True, q_norm=q_norm, k_norm=k_norm)


def cross_attn(x2d, y2d, norm, norm_y, ca, B, Nq, Nk, rope, qpos, kpos, scale, dt, *, train, gamma=None, drops=None, attn_drop=None):
    "x + ls(proj(SDPA(rope(projq(norm(x))), rope(projk(norm_y(y))), projv(norm_y(y))))); norm_y may be nn.Identity (y only converted)"
    lny = None if isinstance(norm_y, nn.Identity) else norm_y
    if train:
        return autograd.cross_attn_sublayer(x2d, y2d, norm, lny, ca, B, Nq, Nk, ca.num_heads, rope, qpos, kpos, scale, dt, gamma=gamma,
                                            drops=drops, attn_drop=attn_drop)
    yn, fold_y = (as_dt(y2d, dt), None) if lny is None else engine.ln_operand(y2d, lny, dt)
    h, fold = engine.ln_operand(x2d, norm, dt)
    return engine.cross_attention(h, yn, B, Nq, Nk, ca.projq, ca.projk, ca.projv, ca.proj, ca.num_heads, rope, qpos, kpos, scale, x2d,
                                  x2d.dtype, fold_q=fold, fold_kv=fold_y, emit_ln=True, q_norm=ca.q_norm, k_norm=ca.k_norm,
                                  proj_wb=_ls_wb(ca.proj, gamma, dt))


def mlp(x2d, norm, fc1, fc2, act, dt, *, train, gamma=None, drops=None):
    "x + ls(fc2(act(fc1(norm(x))))); act: the activation module (GELU(erf) / ReLU / Identity)"
    act = engine.act_name(act)
    if train:
        return autograd.mlp_sublayer(x2d, norm, fc1, fc2, act, dt, gamma=gamma, drops=drops)
    h, fold = engine.ln_operand(x2d, norm, dt)
    return engine.mlp(h, fc1, fc2, act, x2d, x2d.dtype, fc2_wb=_ls_wb(fc2, gamma, dt), fold=fold, emit_ln=True)


def swiglu(x2d, norm, w12, w3, dt, *, train, gamma=None):
    "x + ls(w3(silu(x1) * x2)), x1 | x2 = w12(norm(x))"
    if train:
        return autograd.swiglu_sublayer(x2d, norm, w12, w3, dt, gamma=gamma)
    h, fold = engine.ln_operand(x2d, norm, dt)
    return engine.mlp_swiglu(h, w12, w3, x2d, x2d.dtype, w3_wb=_ls_wb(w3, gamma, dt), fold=fold, emit_ln=True)
