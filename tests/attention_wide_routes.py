"""Route audit of uc_attention_fwd / uc_attention_bwd at head_dim > 64 (uniception_amd/csrc/attention_wide.hip and the fp32 verification
kernels at DMAX 96), by the method of tests/attention_routes.py and with its plan driver and kernel names: one witness per kernel the plan
(uniception_amd/csrc/attention_plan.h) can choose at head_dim > 64, the fp64 reference of every output and the per-element bound.
tests/test_attention_wide_plan.py pins the plans and runs the bound's self-check on the CPU; tests/test_attention_wide_gpu.py launches
every witness, proves the kernel it took and compares every element.

Operands and layouts are those of tests/attention_routes.py (`make_operands`, `place`: q and k are slots of fused [B, N, 2 or 3, H, D]
buffers whose other slots are NaN, gradients go into fused NaN buffers with a slot nobody writes, NaN guard rows behind O and LSE, one
spiked key in the last key tile).  `reference` is restated here because that file's has c(64) written in: every D-long chain uses c(D).

BOUND, per element; u = 2^-24, c(n) = 8 sqrt(n) u, u_out = 2^-8 (bf16) / 2^-24 (fp32), r = 2^-8 where the kernel rounds an MFMA operand to
bf16 (bf16) and 0 for fp32.  The terms are those of tests/attention_routes.py with these differences, which follow the kernels:
 * NO 2^-9 term anywhere.  The wide forward keeps Q as stored and applies scale log2(e) to the fp32 score (attention_wide.hip,
   aw_softmax_step); the wide backward kernels do the same (exp2(fma(s, c, -lse2))): neither re-rounds scale log2(e) Q or K to bf16.
 * score error  e_s = c(D) scale max_k sum_d |q_d| |k_d| + 2^-22 (1 + |lse|)   for the forward and the backward alike.
 * delta and dP are D-long chains: c(D) where tests/attention_routes.py has c(64).
 O:   u_out |o| + r A + E / (1 - E) sum_k p_k |v_kd - o_d| + c(Nk) (A + |o|),   E = expm1(e_s), A = sum_k p_k |v_kd|
 LSE: e_s + c(Nk) + 2^-22 (1 + |lse| + max_k |s_k|)
 backward (on the forward's stored o and lse): E_b = expm1(e_s + bound(LSE)),
    e_delta = sum_d |dO_d| bound(O)_d + c(D) sum_d |dO_d o_d|
    e_dS = (E_b + r) |dS| + (1 + E_b) P (c(D) (sum_d |dO_d v_d| + |delta|) + e_delta)
    dV:  u_out |dV| + sum_q (E_b + r + c(Nq)) p_q |dO_qd|
    dQ:  u_out |dQ| + scale sum_k (e_dS + c(Nk) |dS|) |k_kd|
    dK:  u_out |dK| + scale sum_q (e_dS + c(Nq) |dS|) |q_qd|
Nothing is fitted to results: `emulate_fwd` / `emulate_bwd` perform exactly these roundings in fp32 torch and stay inside the bound on
every bf16 witness, and each seeded fault (FAULTS) leaves it (tests/test_attention_wide_plan.py).

MEASURED on an MI355X (pytest -m gpu -s tests/test_attention_wide_gpu.py prints one line per witness: worst err / bound per output):
see DESIGN.md section 14.
"""
import torch

from tests.attention_routes import (BF16, F32, FWD_FIELDS, BWD_FIELDS, LOG2E, ROOT, U_OUT, CHUNK_ELEMS, _bh, _un_bh, _rb, _w, c_sum,   # noqa: F401
                                    build_driver, check, driver_row, make_operands, place, ratio, route_of, shape_for, spike_position, spy)
from tests.attention_routes import WIDE_FWD_KERNELS as FWD_KERNELS, WIDE_DQ_KERNELS as DQ_KERNELS, WIDE_DKV_KERNELS as DKV_KERNELS   # noqa: F401

WITNESSES = {}
for _D in (80, 96):
    WITNESSES[f"fwd{_D}_ragged"] = _w("fwd", f"bf16_{_D}", (2, 3, 130, 70), D=_D)
    WITNESSES[f"fwd{_D}_whole_tile"] = _w("fwd", f"bf16_{_D}", (2, 3, 130, 64), D=_D)
    WITNESSES[f"fwd{_D}_tiny"] = _w("fwd", f"bf16_{_D}", (1, 1, 5, 3), D=_D)
    WITNESSES[f"bwd{_D}_ragged"] = _w("bwd", f"dq{_D} dkv{_D}", (2, 3, 130, 70), D=_D)
    WITNESSES[f"bwd{_D}_two_tiles"] = _w("bwd", f"dq{_D} dkv{_D}", (2, 2, 200, 200), D=_D)
    WITNESSES[f"f32_fwd_{_D}"] = _w("fwd", "f32_96", (2, 2, 130, 70), dtype=F32, D=_D)
    WITNESSES[f"f32_bwd_{_D}"] = _w("bwd", "f32_dq96 f32_dkv96", (2, 2, 130, 70), dtype=F32, D=_D)
WITNESSES["f32_fwd_72"] = _w("fwd", "f32_96", (2, 2, 130, 70), dtype=F32, D=72)      # not a multiple of 16
SEEDS = {n: i for i, n in enumerate(sorted(WITNESSES))}

# the model shapes whose plans tests/test_attention_wide_plan.py pins next to the witnesses': (B, H, N, D), self-attention, fused qkv
MODEL_SHAPES = {"pixio_h16_256": (32, 16, 264, 80), "pixio_h16_512": (32, 16, 1032, 80),
                "pixio_5b16_256": (32, 32, 264, 96), "pixio_5b16_512": (32, 32, 1032, 96)}


def model_rows(name):
    "(forward row, backward row) of a MODEL_SHAPES entry as ops.attention / ops.attention_bwd fill the descriptors from a fused qkv buffer"
    B, H, N, D = MODEL_SHAPES[name]
    s = dict(dtype=BF16, B=B, H=H, Nq=N, Nk=N, D=D, q_sb=N * 3 * H * D, q_sn=3 * H * D, q_sh=D, k_sb=N * 3 * H * D, k_sn=3 * H * D, k_sh=D,
             o_sb=N * H * D, o_sn=H * D, o_sh=D)
    return dict(fn="fwd", v_layout=1, O=4096, **s), dict(fn="bwd", v_sb=N * 3 * H * D, v_sn=3 * H * D, v_sh=D, **s)


# ------------------------------------------------------------------------------------------ reference and bound
def reference(w, t, scale, dev=None):
    "fp64 reference and bound of every output of the witness: {name: (ref, bound)} for O, LSE and, for a backward witness, dQ, dK, dV"
    dev = dev or t["q"].device
    B, Nq, H, D = t["q"].shape
    Nk = t["k"].shape[1]
    bf = w["dtype"] == BF16
    r = 2.0 ** -8 if bf else 0.0
    u_out = U_OUT[w["dtype"]]
    bwd = w["fn"] == "bwd"
    Q, K, V, dO = (_bh(t[n].to(dev)) for n in ("q", "k", "v", "do"))
    n_bh = max(1, CHUNK_ELEMS // (Nq * Nk * D))
    names = ["O", "LSE"] + (["dQ", "dK", "dV"] if bwd else [])
    parts = {n: [] for n in names}
    for i0 in range(0, B * H, n_bh):
        q, k, v = Q[i0:i0 + n_bh], K[i0:i0 + n_bh], V[i0:i0 + n_bh]
        S = scale * (q @ k.transpose(1, 2))
        s_abs = scale * (q.abs() @ k.abs().transpose(1, 2)).max(-1).values
        s_max = S.abs().max(-1).values
        lse = torch.logsumexp(S, -1)
        P = torch.exp(S - lse[..., None])
        e_s = c_sum(D) * s_abs + 2.0 ** -22 * (1 + lse.abs())
        o = P @ v
        A = P @ v.abs()
        dev_sum = (P[..., None] * (v[:, None] - o[:, :, None]).abs()).sum(2)
        E = torch.expm1(e_s)[..., None]
        b_o = u_out * o.abs() + r * A + E / (1 - E) * dev_sum + c_sum(Nk) * (A + o.abs())
        b_lse = e_s + c_sum(Nk) + 2.0 ** -22 * (1 + lse.abs() + s_max)
        parts["O"].append((o, b_o))
        parts["LSE"].append((lse, b_lse))
        if not bwd:
            continue
        do = dO[i0:i0 + n_bh]
        Eb = torch.expm1(e_s + b_lse)[..., None]
        delta = (do * o).sum(-1, keepdim=True)
        e_delta = (do.abs() * b_o).sum(-1, keepdim=True) + c_sum(D) * (do.abs() * o.abs()).sum(-1, keepdim=True)
        dP = do @ v.transpose(1, 2)
        dPabs = do.abs() @ v.abs().transpose(1, 2)
        dS = P * (dP - delta)
        e_dS = (Eb + r) * dS.abs() + (1 + Eb) * P * (c_sum(D) * (dPabs + delta.abs()) + e_delta)
        dv = P.transpose(1, 2) @ do
        b_dv = ((Eb + r + c_sum(Nq)) * P).transpose(1, 2) @ do.abs()
        dq = scale * (dS @ k)
        b_dq = scale * ((e_dS + c_sum(Nk) * dS.abs()) @ k.abs())
        dk = scale * (dS.transpose(1, 2) @ q)
        b_dk = scale * ((e_dS + c_sum(Nq) * dS.abs()).transpose(1, 2) @ q.abs())
        parts["dQ"].append((dq, b_dq + u_out * dq.abs()))
        parts["dK"].append((dk, b_dk + u_out * dk.abs()))
        parts["dV"].append((dv, b_dv + u_out * dv.abs()))
    out = {}
    for n in names:
        if n == "LSE":
            out[n] = tuple(torch.cat([p[j] for p in parts[n]]).view(B, H, Nq) for j in (0, 1))
        else:
            out[n] = tuple(_un_bh(torch.cat([p[j] for p in parts[n]]), B) for j in (0, 1))
    return out


# ------------------------------------------------------------------------------------------ emulation of the stated roundings (CPU)
# the seeded faults: the channel ones are what a 64-wide habit produces
FAULTS = ("one_key_left_out_of_one_row", "channel_D_minus_1_of_v_zeroed", "channels_64_up_of_k_zeroed", "last_query_row_against_Nk_minus_1_keys")


def emulate_fwd(w, t, scale, fault=None):
    """The wide forward's arithmetic as the bound models it, in fp32 torch: 64-key tiles, the online softmax with the deferred rescale, the
    score scaled in fp32, P rounded to bf16 ahead of P V, the row sum of the unrounded P, one rounding of O.  Returns (O, LSE)."""
    bf = w["dtype"] == BF16
    B, Nq, H, D = t["q"].shape
    Nk = t["k"].shape[1]
    q, k, v = (t[n].float().permute(0, 2, 1, 3).clone() for n in ("q", "k", "v"))
    if fault == "channel_D_minus_1_of_v_zeroed":
        v[..., D - 1] = 0
    if fault == "channels_64_up_of_k_zeroed":
        k[..., 64:] = 0
    s2 = (q @ k.transpose(2, 3)) * (scale * LOG2E)
    if fault == "one_key_left_out_of_one_row":
        s2[0, 0, min(7, Nq - 1), min(37, Nk - 1)] = -1e30
    if fault == "last_query_row_against_Nk_minus_1_keys":
        s2[:, :, Nq - 1, Nk - 1] = -1e30
    m_run = torch.full((B, H, Nq), -1e30)
    l_run = torch.zeros(B, H, Nq)
    o = torch.zeros(B, H, Nq, D)
    for k0 in range(0, Nk, 64):
        st = s2[..., k0:min(k0 + 64, Nk)]
        mt = st.max(-1).values
        m_new = torch.where((mt - m_run) > 8.0, torch.maximum(m_run, mt), m_run)
        alpha = torch.exp2(m_run - m_new)
        m_run, l_run, o = m_new, l_run * alpha, o * alpha[..., None]
        e = torch.exp2(st - m_run[..., None])
        l_run = l_run + e.sum(-1)
        o = o + _rb(e, bf) @ v[:, :, k0:k0 + 64]
    return (o / l_run[..., None]).permute(0, 2, 1, 3).to(t["q"].dtype), m_run / LOG2E + torch.log(l_run)


def emulate_bwd(w, t, o, lse, scale):
    "The wide backward's arithmetic as the bound models it, from the forward's stored o and its lse: P and dS to bf16, one rounding per output"
    bf = w["dtype"] == BF16
    dt = t["q"].dtype
    q, k, v, do, of = (x.float().permute(0, 2, 1, 3) for x in (t["q"], t["k"], t["v"], t["do"], o))
    delta = (do * of).sum(-1, keepdim=True)
    P = torch.exp2((q @ k.transpose(2, 3)) * (scale * LOG2E) - (lse * LOG2E)[..., None])
    dS = _rb(P * (do @ v.transpose(2, 3) - delta), bf)
    dq = (dS @ k).permute(0, 2, 1, 3) * scale
    dk = (dS.transpose(2, 3) @ q).permute(0, 2, 1, 3) * scale
    dv = (_rb(P, bf).transpose(2, 3) @ do).permute(0, 2, 1, 3)
    return dq.to(dt), dk.to(dt), dv.to(dt)
