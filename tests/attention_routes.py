"""Route audit of uc_attention_fwd / uc_attention_bwd: one witness per kernel the plan (uniception_amd/csrc/attention_plan.h) can choose, the
fp64 reference of every output, and the per-element bound.  tests/test_attention_routes.py checks the witnesses against the plan driver
(tests/attention_plan_driver.cpp) and the bound against a CPU emulation of the kernels' roundings with seeded faults;
tests/test_attention_routes_gpu.py launches every witness, proves the kernel it took and compares every element.

WITNESSES.  `WITNESSES[name]` = route (the driver's kernel name, or "dq dkv"), knobs, shape (B, H, Nq, Nk) for 256 CUs (`shape_for`
recomputes the ones whose rule reads the CU count), dtype / D, layout and extras.  Operands (`make_operands`, `place`): q and k are slots
of fused [B, N, 2 or 3, H, D] buffers whose other slots are NaN, the gradients slots of fused NaN buffers with one slot nobody writes, O
and LSE have GUARD NaN rows behind them, and one query row carries a spiked key (2 x the query: 16 nats at |q|^2 = 64, enough for the
rescale branch without making that key hold OTHER rows of its head at a stale maximum; 16 x for the fix-up witness) in the last key tile.  `UNWITNESSED` names what has no witness and why.

REFERENCE (`reference`).  fp64 on the operands as rounded to their type: S = scale Q K^T, LSE, P = exp(S - LSE), P' = P o mask / (1 - p)
under dropout (the materialised mask), O = P' V, delta = rowsum(dO o O), dP = (dO V^T) o mask / (1 - p), dS = P o (dP - delta),
dV = P'^T dO, dQ = scale dS K, dK = scale dS^T Q, then the inverse RoPE-2D of dQ / dK where the witness carries positions.  The backward
runs on the GPU forward's o and lse and is compared with the fp64 gradients of the fp64 o and lse.

BOUND, per element; u = 2^-24, c(n) = 8 sqrt(n) u (the fp32 summation term of tests/gemm_routes.py), u_out = 2^-8 (bf16) / 2^-24 (fp32),
r = 2^-8 where the kernel rounds an MFMA operand to bf16 (bf16 routes) and 0 for the fp32 kernels.

 score error (absolute, in nats), per query row, at its maximum over the keys:
    e_s = c(64) scale max_k sum_d |q_d k_d|                      the fp32 MFMA chain of a score
        + 2^-9 scale max_k sum_d |q_d| |k_d|                     p64, p64_tail and every bf16 backward kernel: scale log2(e) Q (dK / dV
                                                                 kernel: K) re-rounded to bf16 (attention_p64.h:448, attention_bwd.hip:181,
                                                                 :329, attention_bwd64.h:240, :700)
        + 2^-22 (1 + |lse|)                                      terms the starting model lacks: v_exp_f32 / expf are good to ~1 ulp (a
                                                                 relative 2^-23 of p is an absolute 2^-23 of the score), the fma
                                                                 s c - m c (attention.hip:199) and the backward's score chain, which
                                                                 starts at -lse log2(e) (attention_bwd.hip:241, :383), round at the
                                                                 magnitude of the maximum / of lse
 E = expm1(e_s): the relative error of a probability.  A normalised probability p_k (1 + eps_k) / sum_j p_j (1 + eps_j) moves O by
 sum_k p_k eps_k (v_k - o) / (1 + sum_j p_j eps_j): the factor 1 / (1 - E) below is that denominator (1 + O(e_s) in the starting model).

 O:   u_out |o| + r A + E / (1 - E) sum_k p_k |m_k v_kd - o_d| + c(Nk) (A + |o|),   A = sum_k p'_k |v_kd|, m_k = mask_k / (1 - p)
      (r A: P rounded to bf16 ahead of the second MFMA; c(Nk) |o|: the row sum l, attention.hip:213, a second fp32 chain of Nk terms)
 LSE: e_s + c(Nk) + 2^-22 (1 + |lse| + max_k |s_k|)             (m scale + logf(l): the product, logf and the sum round at those magnitudes;
                                                                 p64 keeps l against the first 32 keys' maximum: log l <= |lse| + max |s|)
 backward: the kernels rebuild P~ = exp2(s~ - lse~ log2(e)) and do not renormalise: |P~ - P| <= E_b P with
    E_b = expm1(e_s(backward kernel) + bound(LSE of the forward that ran)).
    delta~ = rowsum(dO o o~) of the STORED forward output:  e_delta = sum_d |dO_d| bound(O)_d + c(64) sum_d |dO_d o_d|
    dS~ = bf16(P~ (dP~ - delta~)):  e_dS = (E_b + r) |dS| + (1 + E_b) P (m (c(64) (sum_d |dO_d v_d| + |delta|)) + e_delta)
                                          [+ 2^-22 P m (|dP'| + 2 |delta|) under dropout: the fma form of attention_bwd.hip:255, :398]
    dV:  u_out |dV| + sum_q (E_b + r + c(Nq)) p'_q |dO_qd|
    dQ:  u_out |dQ| + scale sum_k (e_dS + c(Nk) |dS|) |k_kd|
    dK:  u_out |dK| + scale sum_q (e_dS + c(Nq) |dS|) |q_qd|
    inverse RoPE of a pair (u, v) = (channel c, c + 16) of a 32-channel half, ahead of the store: the pair's bounds turn with |cos|, |sin|,
    plus 2e-5 (|u| + |v|) for the hardware sine / cosine (the term of tests/gemm_routes.py; positions in [0, 32)).
 Nothing here is fitted to results: the CPU emulation of exactly these roundings stays inside the bound on every small bf16 witness and
 at or under half of it on the smallest forward and backward ones (tests/test_attention_routes.py; O sits at 0.4 - 0.6 everywhere: where
 one key holds a row, A = |o| and the store rounding alone is half the bound, and under dropout the kept probability 1 / (1 - p) of a
 row that one key holds is itself rounded: up to 0.75), and every seeded fault there leaves it.

Reference budget: a witness's fp64 work runs in chunks of (batch, head) pairs of at most CHUNK_ELEMS elements ([pairs, Nq, Nk, D] for
the forward's |m v - o| sum), so the largest witness needs about 0.4 GB at a time.

MEASURED on an MI355X (pytest -m gpu -s prints one line per witness: the forward kernel that ran and the worst err / bound of O, LSE, dQ,
dK, dV).  All 29 witnesses pass; the slowest (dma4) takes 1.2 s, every other one under 0.8 s.
  witness                  forward      O     LSE    dQ    dK    dV   | witness                  forward      O     LSE    dQ    dK    dV
  dma4_whole_tile          dma4         0.480 0.021                   | dq32_dkv32               dma4         0.458 0.026 0.106 0.075 0.165
  dma4_tiny                dma4         0.491 0.008                   | dq64_dkv64               dma4         0.406 0.022 0.085 0.091 0.143
  reg128                   reg128       0.450 0.020                   | dq64_dkv32               dma4         0.491 0.021 0.137 0.063 0.110
  dma8                     dma8         0.572 0.033                   | dq64_dkv32_rows_follow   dma4         0.391 0.024 0.097 0.077 0.185
  rs8                      rs8          0.650 0.030                   | dq64_dkv64_foreign_rows  dma4         0.475 0.021 0.085 0.073 0.139
  p64                      p64          0.313 0.189                   | bwd64_seams              dma4         0.507 0.028 0.123 0.120 0.221
  p64_tail                 p64_tail     0.533 0.129                   | dq32_dkv32_rope          dma4         0.478 0.022 0.109 0.098 0.146
  p64_seams                p64          0.278 0.220                   | dq64_dkv64_rope          dma4         0.883 0.022 0.120 0.061 0.139
  p64_fixup                p64_tail     0.752 0.366                   | dq32_dkv32_drop          reg128_drop  0.639 0.024 0.162 0.103 0.186
  reg128_drop              reg128_drop  0.669 0.025                   | f32_bwd_32               f32_32       0.014 0.030 0.004 0.002 0.006
  f32_32                   f32_32       0.019 0.030                   | f32_bwd_64               f32_64       0.020 0.028 0.003 0.002 0.006
  f32_64                   f32_64       0.017 0.023                   | f32_bwd_32_drop          f32_32_drop  0.026 0.031 0.004 0.003 0.010
  f32_32_drop              f32_32_drop  0.025 0.050                   | f32_bwd_64_drop          f32_64_drop  0.020 0.027 0.007 0.002 0.007
  f32_64_drop              f32_64_drop  0.040 0.031                   |
Above 0.5: only O of bf16 forwards (0.51 - 0.88), the band the CPU emulation already shows: u_out |o| + r A dominates where one key holds
a row (A = |o|: the store rounding alone is half the bound, the bf16 rounding of P the rest; the run did not record the worst element's
terms, so 0.883 of dq64_dkv64_rope is placed there by that argument, not by a breakdown).  Below 0.01: the gradients of the fp32
kernels — with r = 0 and u_out = 2^-24 their bound is the c(n) summation terms, worst cases over sums of magnitudes that random-sign
fp32 rounding stays two orders under.
"""
import contextlib
import math
import os
import shutil
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}
U = 2.0 ** -24
U_OUT = {F32: 2.0 ** -24, BF16: 2.0 ** -8}
GUARD = 8                 # NaN rows behind O (rows of H x D) and NaN floats behind LSE
GAP = 64                  # foreign NaN rows behind / between the batches of q, o and do in the rows_follow witnesses
ROPE_BASE, ROPE_F0 = 100.0, 1.0
CHUNK_ELEMS = 1 << 24
LOG2E = 1.4426950408889634
DROP_P, DROP_SEED = 0.25, 0x1234_5678_9ABC_DEF1
FWD_KERNELS = ("reg128", "dma4", "dma8", "rs8", "p64", "p64_tail", "reg128_drop", "f32_32", "f32_64", "f32_32_drop", "f32_64_drop", "dma4_dbg")
DQ_KERNELS = ("dq32", "dq64", "dq32_drop", "f32_dq32", "f32_dq64")
DKV_KERNELS = ("dkv32", "dkv64", "dkv32_drop", "f32_dkv32", "f32_dkv64")
# the head_dim > 64 kernels the same plan and driver name (they follow the ones above in the enums of attention_plan.h): witnessed in
# tests/attention_wide_routes.py, whose bound differs from this file's
WIDE_FWD_KERNELS = ("bf16_80", "bf16_96", "f32_96")
WIDE_DQ_KERNELS = ("dq80", "dq96", "f32_dq96")
WIDE_DKV_KERNELS = ("dkv80", "dkv96", "f32_dkv96")
REFUSALS = ("dtype", "bf16_head_dim", "f32_head_dim", "dropout", "rope_f32", "rope_head_dim", "bwd_grid")      # `refused <reason>`
REQUANT_FWD = ("p64", "p64_tail")      # forward kernels that re-round scale log2(e) Q to bf16
KNOBS = {"p64": "attn_p64", "bwd64": "attn_bwd64", "role_split": "attn_role_split"}      # driver name -> tuning knob


def _w(fn, route, shape, knobs=None, dtype=BF16, D=64, layout="fused", drop=0.0, rope=False, spike=2.0, cu_rule=None, seam=False, fixup=False):
    return dict(fn=fn, route=route, shape=shape, knobs=knobs or {}, dtype=dtype, D=D, layout=layout, drop=drop, rope=rope, spike=spike,
                cu_rule=cu_rule, seam=seam, fixup=fixup)


# layout: "fused" (q | k slots of fused buffers, contiguous O), "o68" (O = the 64-channel slice of a [B, Nq, H, 68] NaN buffer),
# "gap" (q, o, do = buf[:, :Nq] of [B, Nq + GAP, H, D] NaN buffers: foreign rows between the batches / behind the only one)
WITNESSES = {
    # ---- forward
    "dma4": _w("fwd", "dma4", (2, 3, 130, 70)),
    "dma4_whole_tile": _w("fwd", "dma4", (2, 3, 130, 64)),
    "dma4_tiny": _w("fwd", "dma4", (1, 1, 5, 3)),
    "reg128": _w("fwd", "reg128", (2, 3, 130, 70), layout="o68"),
    "dma8": _w("fwd", "dma8", (16, 16, 400, 70), cu_rule="dma8"),
    "rs8": _w("fwd", "rs8", (16, 16, 400, 70), {"role_split": 1}, cu_rule="dma8"),
    "p64": _w("fwd", "p64", (2, 2, 130, 128), {"p64": 2}),
    "p64_tail": _w("fwd", "p64_tail", (2, 2, 130, 130), {"p64": 2}),
    "p64_seams": _w("fwd", "p64", (65, 8, 256, 128), cu_rule="p64_seams", seam=True),
    "p64_fixup": _w("fwd", "p64_tail", (2, 2, 300, 200), {"p64": 2}, spike=16.0, fixup=True),
    "reg128_drop": _w("fwd", "reg128_drop", (2, 3, 130, 70), drop=DROP_P),
    "f32_32": _w("fwd", "f32_32", (2, 2, 130, 70), dtype=F32, D=32),
    "f32_64": _w("fwd", "f32_64", (2, 2, 130, 70), dtype=F32, D=64),
    "f32_32_drop": _w("fwd", "f32_32_drop", (2, 2, 130, 70), dtype=F32, D=32, drop=DROP_P),
    "f32_64_drop": _w("fwd", "f32_64_drop", (2, 2, 130, 70), dtype=F32, D=64, drop=DROP_P),
    # ---- backward
    "dq32_dkv32": _w("bwd", "dq32 dkv32", (2, 3, 130, 70)),
    "dq64_dkv64": _w("bwd", "dq64 dkv64", (2, 3, 200, 200)),
    "dq64_dkv32": _w("bwd", "dq64 dkv32", (2, 3, 200, 70)),
    "dq64_dkv32_rows_follow": _w("bwd", "dq64 dkv32", (2, 3, 200, 200), layout="gap"),
    "dq64_dkv64_foreign_rows": _w("bwd", "dq64 dkv64", (1, 3, 200, 200), layout="gap"),
    "bwd64_seams": _w("bwd", "dq64 dkv64", (33, 8, 256, 256), cu_rule="bwd64_seams", seam=True),
    "dq32_dkv32_rope": _w("bwd", "dq32 dkv32", (2, 3, 130, 70), rope=True),
    "dq64_dkv64_rope": _w("bwd", "dq64 dkv64", (2, 3, 200, 200), rope=True),
    "dq32_dkv32_drop": _w("bwd", "dq32_drop dkv32_drop", (2, 3, 130, 70), drop=DROP_P),
    "f32_bwd_32": _w("bwd", "f32_dq32 f32_dkv32", (2, 2, 130, 70), dtype=F32, D=32),
    "f32_bwd_64": _w("bwd", "f32_dq64 f32_dkv64", (2, 2, 130, 70), dtype=F32, D=64),
    "f32_bwd_32_drop": _w("bwd", "f32_dq32 f32_dkv32", (2, 2, 130, 70), dtype=F32, D=32, drop=DROP_P),
    "f32_bwd_64_drop": _w("bwd", "f32_dq64 f32_dkv64", (2, 2, 130, 70), dtype=F32, D=64, drop=DROP_P),
}
# operand seeds.  The three witnesses the CPU file holds to err / bound <= 0.5 have theirs chosen so that the clean emulation gets there:
# where one key holds a row (A = |o|) the output's store rounding alone reaches half the bound, so that bar sits at the model's limit
SEEDS = {n: i for i, n in enumerate(sorted(WITNESSES))}
SEEDS.update({"dma4": 1, "dma4_tiny": 4, "dq32_dkv32": 3})
UNWITNESSED = {
    "dma4_dbg": "diag build only (UC_ATTN_DBG): the release library never chooses it, and its results are wrong by design",
    "dq32 dkv64": "needs v_ext >= 4 GB (the 32-bit descriptor rule of the dQ kernel alone): more than 4 GB of V",
}


def shape_for(w, cus=256):
    "The witness's (B, H, Nq, Nk) on a device of `cus` compute units (the stored shape is the one for 256)."
    B, H, Nq, Nk = w["shape"]
    if w["cu_rule"] == "dma8":             # nw == 8 needs ceil(Nq / 256) H B >= 2 CUs: two query tiles, 16 heads
        B = (cus + H - 1) // H
    elif w["cu_rule"] == "p64_seams":      # more items than the 2 CUs workgroups, not a multiple of the 8 XCDs; the policy wants >= 512
        B = max(2 * cus // 8 + 1, 65)
    elif w["cu_rule"] == "bwd64_seams":    # more items than the CUs workgroups of the persistent backward kernels
        B = cus // 8 + 1
    return B, H, Nq, Nk


# ------------------------------------------------------------------------------------------ plan driver, spy
def build_driver(tmpdir):
    "Compile tests/attention_plan_driver.cpp with the system C++ compiler into tmpdir; returns run(rows) -> plan lines."
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/attention_plan_driver.cpp"
    exe = os.path.join(str(tmpdir), "attention_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "uniception_amd", "csrc"), os.path.join(ROOT, "tests", "attention_plan_driver.cpp"), "-o", exe])

    def run(rows):
        if not rows:
            return []
        lines = [" ".join(f"{k}={v}" for k, v in row.items()) for row in rows]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return run


def route_of(fn, plan_line):
    "The route a plan line stands for: the forward kernel, or `dq dkv`."
    t = plan_line.split()
    return t[0] if fn == "fwd" else f"{t[0]} {t[2]}"


_STRIDES = "q_sb q_sn q_sh k_sb k_sn k_sh v_sb v_sn v_sh o_sb o_sn o_sh".split()


def driver_row(w, cus=256):
    "The descriptor row of a witness in its layout, as the wrappers in ops.py fill it in (no launch: strides from the layout's shapes)."
    B, H, Nq, Nk = shape_for(w, cus)
    D = w["D"]
    q_sn = 2 * H * D if w["layout"] != "gap" else H * D
    q_rows = Nq if w["layout"] != "gap" else Nq + GAP
    row = dict(fn=w["fn"], dtype=w["dtype"], B=B, H=H, Nq=Nq, Nk=Nk, D=D, q_sb=q_rows * q_sn, q_sn=q_sn, q_sh=D,
               k_sb=Nk * 3 * H * D, k_sn=3 * H * D, k_sh=D)
    if w["fn"] == "bwd" or w["dtype"] == F32:
        row.update(v_sb=Nk * 3 * H * D, v_sn=3 * H * D, v_sh=D)
    if w["layout"] == "o68":
        row.update(o_sb=Nq * H * 68, o_sn=H * 68, o_sh=68)
    else:
        row.update(o_sb=q_rows * H * D if w["layout"] == "gap" else Nq * H * D, o_sn=H * D, o_sh=D)
    if w["fn"] == "fwd":
        row.update(v_layout=1 if w["dtype"] == BF16 else 0, O=4096)
    if w["drop"]:
        row["drop"] = 1
    if w["rope"] and w["fn"] == "bwd":
        row["rope"] = 1
    row.update(w["knobs"])
    row["cus"] = cus
    return row


@contextlib.contextmanager
def spy(fn_name, ctypes_fields):
    """Wrap libuc_hip's `fn_name` (uc_attention_fwd / uc_attention_bwd) so that every call's descriptor is recorded as a driver row
    (the fields the plan reads) before it goes on to the library.  Yields the list of rows."""
    from uniception_amd import _lib
    lib = _lib.load()
    real = getattr(lib, fn_name)
    captured = []

    def wrapper(desc_ref, stream):
        d = desc_ref._obj
        rec = {"fn": "fwd" if fn_name == "uc_attention_fwd" else "bwd"}
        for name in ctypes_fields:
            if hasattr(d, name):
                rec[name] = int(getattr(d, name) or 0)
        if float(d.drop_p) != 0.0:
            rec["drop"] = 1
        if getattr(d, "rope_qpos", None) or getattr(d, "rope_kpos", None):      # (the backward descriptor only)
            rec["rope"] = 1
        captured.append(rec)
        return real(desc_ref, stream)

    setattr(lib, fn_name, wrapper)
    try:
        yield captured
    finally:
        setattr(lib, fn_name, real)


FWD_FIELDS = ["dtype", "v_layout", "B", "H", "Nq", "Nk", "D", "O"] + _STRIDES
BWD_FIELDS = ["dtype", "B", "H", "Nq", "Nk", "D"] + _STRIDES


def live_knobs(ops):
    "The knob snapshot of the next launch on this device, in the driver's names."
    knobs = {"cus": torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count}
    for k, name in KNOBS.items():
        knobs[k] = ops.tuning_get(name)
    return knobs


@contextlib.contextmanager
def knobs_set(ops, knobs):
    "The witness's knobs through ops.tuning (restored on the way out)."
    with contextlib.ExitStack() as st:
        for k, v in knobs.items():
            st.enter_context(ops.tuning(KNOBS[k], v))
        yield


# ------------------------------------------------------------------------------------------ operands
def spike_position(w, shape):
    "(batch, query row, head, key) of the spiked key: the last key tile (the ragged one where there is one), a query of the last block."
    B, H, Nq, Nk = shape
    return 0, (Nq - 20 if Nq > 20 else Nq - 1), 0, (Nk - 5 if Nk > 5 else Nk - 1)


def make_operands(w, shape, seed=0):
    "Seeded operands of a witness on the CPU, as rounded to the witness's type: q, k, v, do [B, N, H, D] and the RoPE positions."
    B, H, Nq, Nk = shape
    D, dt = w["D"], TORCH_DT[w["dtype"]]
    g = torch.Generator().manual_seed(4000 + seed)
    t = {"q": torch.randn(B, Nq, H, D, generator=g).to(dt), "k": torch.randn(B, Nk, H, D, generator=g).to(dt),
         "v": torch.randn(B, Nk, H, D, generator=g).to(dt), "do": torch.randn(B, Nq, H, D, generator=g).to(dt)}
    b, qr, h, kk = spike_position(w, shape)
    t["k"][b, kk, h] = (t["q"][b, qr, h].float() * w["spike"]).to(dt)
    if w["rope"]:
        t["qpos"] = torch.randint(0, 32, (B * Nq, 2), generator=g, dtype=torch.int64)
        t["kpos"] = torch.randint(0, 32, (B * Nk, 2), generator=g, dtype=torch.int64)
    return t


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def place(w, t, dev):
    """The operands on `dev` in the witness's layout.  Returns views (q, k, v, do, out, lse, dq, dk, dv) and `nan_zones`: {name: tensor}
    of every guard band and unused slot, all of which must still be NaN after the launches."""
    B, Nq, H, D = t["q"].shape
    Nk = t["k"].shape[1]
    dt = t["q"].dtype
    p, zones = {}, {}
    kbuf = _nan((B, Nk, 3, H, D), dt, dev)
    kbuf[:, :, 1] = t["k"].to(dev)
    kbuf[:, :, 2] = t["v"].to(dev)
    p["k"], p["v"] = kbuf[:, :, 1], kbuf[:, :, 2]
    if w["layout"] == "gap":
        qbuf, obuf, dobuf = (_nan((B, Nq + GAP, H, D), dt, dev) for _ in range(3))
        qbuf[:, :Nq] = t["q"].to(dev)
        dobuf[:, :Nq] = t["do"].to(dev)
        p["q"], p["out"], p["do"] = qbuf[:, :Nq], obuf[:, :Nq], dobuf[:, :Nq]
        zones["rows behind O"] = obuf[:, Nq:]
    else:
        qbuf = _nan((B, Nq, 2, H, D), dt, dev)
        qbuf[:, :, 0] = t["q"].to(dev)
        p["q"], p["do"] = qbuf[:, :, 0], t["do"].to(dev)
        if w["layout"] == "o68":
            obuf = _nan((B, Nq, H, 68), dt, dev)
            p["out"] = obuf[..., :D]
            zones["channels 64..67 of O's buffer"] = obuf[..., D:]
        else:
            obuf = _nan((B * Nq + GUARD, H, D), dt, dev)
            p["out"] = obuf[:B * Nq].view(B, Nq, H, D)
            zones["guard behind O"] = obuf[B * Nq:]
    lbuf = _nan((B * H * Nq + GUARD,), torch.float32, dev)
    p["lse"] = lbuf[:B * H * Nq].view(B, H, Nq)
    zones["guard behind LSE"] = lbuf[B * H * Nq:]
    if w["fn"] == "bwd":
        gq, gkv = _nan((B, Nq, 2, H, D), dt, dev), _nan((B, Nk, 3, H, D), dt, dev)
        p["dq"], p["dk"], p["dv"] = gq[:, :, 0], gkv[:, :, 0], gkv[:, :, 1]
        zones["unused slot of dQ's fused buffer"] = gq[:, :, 1]
        zones["unused slot of dK | dV's fused buffer"] = gkv[:, :, 2]
    if w["rope"]:
        p["rope"] = (t["qpos"].to(dev), t["kpos"].to(dev), ROPE_BASE, ROPE_F0)
    return p, zones


# ------------------------------------------------------------------------------------------ reference and bound
def c_sum(n):
    return 8.0 * math.sqrt(n) * U


def _bh(x):
    "[B, N, H, D] -> [B H, N, D] fp64"
    B, N, H, D = x.shape
    return x.double().permute(0, 2, 1, 3).reshape(B * H, N, D)


def _un_bh(x, B):
    "[B H, N, D] -> [B, N, H, D]"
    BH, N, D = x.shape
    return x.view(B, BH // B, N, D).permute(0, 2, 1, 3).contiguous()


def rope_inverse(x, e, pos):
    """The inverse RoPE-2D of a gradient x [B, N, H, 64] (fp64) with its error bound e: halves (y, x) of 32 channels, pairs (c, c + 16),
    channel c of a half turned BACK by pos F0 base^(-c/16).  Returns (rotated x, rotated bound + the hardware sine's term)."""
    B, N, H, D = x.shape
    inv = ROPE_F0 / ROPE_BASE ** (torch.arange(16, device=x.device, dtype=x.dtype) / 16)
    ang = pos.to(x.dtype).view(B, N, 1, 2, 1) * inv                    # [B, N, 1, axis, 16]
    cs, sn = torch.cos(ang), torch.sin(ang)
    xx, ee = x.view(B, N, H, 2, 2, 16), e.view(B, N, H, 2, 2, 16)      # [.., axis, (u, v), 16]
    u, v, eu, ev = xx[..., 0, :], xx[..., 1, :], ee[..., 0, :], ee[..., 1, :]
    pair = 2e-5 * (u.abs() + v.abs())
    rot = torch.stack([u * cs + v * sn, v * cs - u * sn], 4).reshape(B, N, H, D)
    err = torch.stack([eu * cs.abs() + ev * sn.abs() + pair, ev * cs.abs() + eu * sn.abs() + pair], 4).reshape(B, N, H, D)
    return rot, err


def p64_flagged_rows(S):
    """Query rows whose 64-query block attn_bf16_p64_kernel flags for attn_bf16_fixup_kernel: the row sum of exp2 against the maximum of
    the item's FIRST 32 keys leaves [2^-100, 2^100] (attention_p64.h).  S: scaled scores [.., Nq, Nk] (fp64, nats)."""
    m = S[..., :32].max(-1, keepdim=True).values
    l2 = torch.logsumexp(S - m, -1) * LOG2E
    return (l2 > 100.0) | (l2 < -100.0)


def reference(w, t, scale, mask=None, fwd_requant=False, dev=None):
    """fp64 reference and bound of every output of the witness: {name: (ref, bound)} for O [B, Nq, H, D] and LSE [B, H, Nq], and for a
    backward witness dQ, dK, dV.  t: operands as from make_operands (any device); mask: the materialised keep mask [B, H, Nq, Nk] under
    dropout; fwd_requant: the forward that produced the backward's o / lse was p64 / p64_tail.  Also returns `flagged` [B, H, Nq]."""
    dev = dev or t["q"].device
    B, Nq, H, D = t["q"].shape
    Nk = t["k"].shape[1]
    bf = w["dtype"] == BF16
    r = 2.0 ** -8 if bf else 0.0
    u_out = U_OUT[w["dtype"]]
    bwd = w["fn"] == "bwd"
    requant_f = fwd_requant if bwd else w["route"] in REQUANT_FWD
    keep_scale = 1.0 / (1.0 - w["drop"]) if w["drop"] else 1.0
    Q, K, V, dO = (_bh(t[n].to(dev)) for n in ("q", "k", "v", "do"))
    M = None if mask is None else mask.to(dev).view(B * H, Nq, Nk)
    n_bh = max(1, CHUNK_ELEMS // (Nq * Nk * D))
    names = ["O", "LSE", "flag"] + (["dQ", "dK", "dV"] if bwd else [])
    parts = {n: [] for n in names}
    for i0 in range(0, B * H, n_bh):
        q, k, v = Q[i0:i0 + n_bh], K[i0:i0 + n_bh], V[i0:i0 + n_bh]
        S = scale * (q @ k.transpose(1, 2))
        s_abs = scale * (q.abs() @ k.abs().transpose(1, 2)).max(-1).values                # [n, Nq]: max_k sum_d |q_d| |k_d| scale
        s_max = S.abs().max(-1).values
        lse = torch.logsumexp(S, -1)
        P = torch.exp(S - lse[..., None])
        misc = 2.0 ** -22 * (1 + lse.abs())
        es_f = (c_sum(64) + (2.0 ** -9 if requant_f else 0.0)) * s_abs + misc
        m = keep_scale * M[i0:i0 + n_bh].double() if M is not None else None
        Pm = P * m if m is not None else P
        o = Pm @ v
        A = Pm @ v.abs()
        mv = v[:, None] if m is None else m[..., None] * v[:, None]                       # [n, Nq | 1, Nk, D]
        dev_sum = (P[..., None] * (mv - o[:, :, None]).abs()).sum(2)
        E = torch.expm1(es_f)[..., None]
        b_o = u_out * o.abs() + r * A + E / (1 - E) * dev_sum + c_sum(Nk) * (A + o.abs())
        b_lse = es_f + c_sum(Nk) + 2.0 ** -22 * (1 + lse.abs() + s_max)
        parts["O"].append((o, b_o))
        parts["LSE"].append((lse, b_lse))
        parts["flag"].append(p64_flagged_rows(S))
        if not bwd:
            continue
        do = dO[i0:i0 + n_bh]
        es_b = (c_sum(64) + (2.0 ** -9 if bf else 0.0)) * s_abs + misc
        Eb = torch.expm1(es_b + b_lse)[..., None]                                         # [n, Nq, 1]
        delta = (do * o).sum(-1, keepdim=True)
        e_delta = (do.abs() * b_o).sum(-1, keepdim=True) + c_sum(64) * (do.abs() * o.abs()).sum(-1, keepdim=True)
        dPp = do @ v.transpose(1, 2)
        dPabs = do.abs() @ v.abs().transpose(1, 2)
        mm = m if m is not None else 1.0
        dS = P * (dPp * mm - delta)
        e_dS = (Eb + r) * dS.abs() + (1 + Eb) * P * (mm * c_sum(64) * (dPabs + delta.abs()) + e_delta)
        if m is not None:
            e_dS = e_dS + 2.0 ** -22 * P * mm * (dPp.abs() + 2 * delta.abs())
        dv = Pm.transpose(1, 2) @ do
        b_dv = ((Eb + r + c_sum(Nq)) * Pm).transpose(1, 2) @ do.abs()
        dq = scale * (dS @ k)
        b_dq = scale * ((e_dS + c_sum(Nk) * dS.abs()) @ k.abs())
        dk = scale * (dS.transpose(1, 2) @ q)
        b_dk = scale * ((e_dS + c_sum(Nq) * dS.abs()).transpose(1, 2) @ q.abs())
        parts["dQ"].append((dq, b_dq))
        parts["dK"].append((dk, b_dk))
        parts["dV"].append((dv, b_dv))
    out = {}
    for n in ("O", "dQ", "dK", "dV"):
        if n in parts:
            out[n] = tuple(_un_bh(torch.cat([p[j] for p in parts[n]]), B) for j in (0, 1))
    out["LSE"] = tuple(torch.cat([p[j] for p in parts["LSE"]]).view(B, H, Nq) for j in (0, 1))
    flagged = torch.cat(parts["flag"]).view(B, H, Nq)
    if bwd:
        if w["rope"]:
            out["dQ"] = rope_inverse(*out["dQ"], t["qpos"].to(dev))
            out["dK"] = rope_inverse(*out["dK"], t["kpos"].to(dev))
        for n in ("dQ", "dK", "dV"):
            out[n] = (out[n][0], out[n][1] + u_out * out[n][0].abs())
    return out, flagged


# ------------------------------------------------------------------------------------------ emulation of the stated roundings (CPU)
def _rb(x, bf):
    "One rounding to bf16 where the kernel has one, as fp32."
    return x.bfloat16().float() if bf else x


def emulate_fwd(w, t, scale, mask=None, fault=None):
    """The forward kernels' arithmetic as the bound models it, in fp32 torch: 64-key tiles, the online softmax with the deferred rescale
    (attention.hip:178), P rounded to bf16 ahead of P V, the row sum of the unrounded P, one rounding of O; p64 / p64_tail: scale log2(e) Q
    re-rounded to bf16.  Returns (O [B, Nq, H, D] in the witness's type, LSE fp32 [B, H, Nq]).  fault: one of the seeded faults of
    tests/test_attention_routes.py."""
    bf = w["dtype"] == BF16
    B, Nq, H, D = t["q"].shape
    Nk = t["k"].shape[1]
    q, k, v = (t[n].float().permute(0, 2, 1, 3) for n in ("q", "k", "v"))                  # [B, H, N, D]
    c = scale * LOG2E
    b_s, q_s, h_s, k_s = spike_position(w, (B, H, Nq, Nk))
    if fault == "query_row_from_neighbouring_head":
        q = q.clone()
        q[0, 0, 40] = q[0, 1, 40]
    if fault == "v_rows_swapped_in_a_16_key_block":
        v = v.clone()
        v[:, :, [17, 21]] = v[:, :, [21, 17]]
    nk_eff = Nk - 1 if fault == "last_key_dropped" else Nk
    if w["route"] in REQUANT_FWD:
        s2 = _rb(q * c, True) @ k.transpose(2, 3)                                          # already in the exp2 domain
    else:
        s2 = (q @ k.transpose(2, 3)) * c
    keep = None if mask is None else mask.float() / (1.0 - w["drop"])
    m_run = torch.full((B, H, Nq), -1e30)
    l_run = torch.zeros(B, H, Nq)
    o = torch.zeros(B, H, Nq, D)
    for k0 in range(0, Nk, 64):
        k1 = min(k0 + 64, nk_eff)
        if k1 <= k0:
            break
        st = s2[..., k0:k1]
        mt = st.max(-1).values
        grow = (mt - m_run) > 8.0
        m_new = torch.where(grow, torch.maximum(m_run, mt), m_run)
        alpha = torch.exp2(m_run - m_new)
        if fault == "rescale_skipped_for_the_spiked_row" and k0 > 0:
            alpha[b_s, h_s, q_s] = 1.0
        m_run, l_run, o = m_new, l_run * alpha, o * alpha[..., None]
        e = torch.exp2(st - m_run[..., None])
        l_run = l_run + e.sum(-1)
        if fault == "pad_key_admitted_with_score_0" and k1 == nk_eff and Nk % 64:
            l_run = l_run + torch.exp2(0.0 - m_run)                                        # (its V row is the pad's zeros)
        if keep is not None:
            e = e * keep[..., k0:k1]
        o = o + _rb(e, bf) @ v[:, :, k0:k1]
    out = (o / l_run[..., None]).permute(0, 2, 1, 3).to(t["q"].dtype)
    lse = m_run / LOG2E + torch.log(l_run)
    return out, lse


def emulate_bwd(w, t, o, lse, scale, mask=None, fault=None):
    """The backward kernels' arithmetic as the bound models it (fp32 torch), from the forward's STORED o and its lse: the dQ kernel
    re-rounds scale log2(e) Q, the dK / dV kernel re-rounds scale log2(e) K, P and dS go to bf16 ahead of their MFMAs, one rounding per
    output, the inverse RoPE ahead of the store.  Returns dq, dk, dv [B, N, H, D] in the witness's type."""
    bf = w["dtype"] == BF16
    dt = t["q"].dtype
    q, k, v, do, of = (x.float().permute(0, 2, 1, 3) for x in (t["q"], t["k"], t["v"], t["do"], o))
    c = scale * LOG2E
    lse2 = (lse * LOG2E)[..., None]
    delta = (do * of).sum(-1, keepdim=True)
    if fault == "delta_omitted_from_dS":
        delta = torch.zeros_like(delta)
    mm = 1.0 if mask is None else mask.float() / (1.0 - w["drop"])
    dPm = (do @ v.transpose(2, 3)) * mm - delta
    if bf:
        P_q = torch.exp2(_rb(q * c, True) @ k.transpose(2, 3) - lse2)
        P_k = torch.exp2(q @ _rb(k * c, True).transpose(2, 3) - lse2)
    else:
        P_q = P_k = torch.exp(scale * (q @ k.transpose(2, 3)) - lse[..., None])
    dq = (_rb(P_q * dPm, bf) @ k).permute(0, 2, 1, 3)
    dk = (_rb(P_k * dPm, bf).transpose(2, 3) @ q).permute(0, 2, 1, 3)
    dv = (_rb(P_k * mm, bf).transpose(2, 3) @ do).permute(0, 2, 1, 3)
    if w["rope"]:
        z = torch.zeros_like(dq, dtype=torch.float64)
        dq = rope_inverse(dq.double().contiguous(), z, t["qpos"])[0].float()
        dk = rope_inverse(dk.double().contiguous(), torch.zeros_like(dk, dtype=torch.float64), t["kpos"])[0].float()
    dk = dk * scale
    if fault == "scale_applied_twice_to_dK":
        dk = dk * scale
    return (dq * scale).to(dt), dk.to(dt), dv.to(dt)


def host_drop_mask(shape, p, seed=0):
    "A stand-in keep mask for the CPU emulation (the GPU tests take the kernels' own from ops.attention_drop_mask)."
    B, H, Nq, Nk = shape
    g = torch.Generator().manual_seed(77 + seed)
    return (torch.rand(B, H, Nq, Nk, generator=g) >= p).to(torch.uint8)


# ------------------------------------------------------------------------------------------ checker
def ratio(got, ref, bnd):
    "err / bound per element (NaN — an element never written — is infinite)."
    x = (got.to(ref.dtype) - ref).abs() / bnd
    return torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x)


def check(route, name, got, ref, bnd):
    """Zero elements over the bound, or an AssertionError naming the route, the count and the worst element: its (b, h, row, d) and the
    64-row and 128-row tile it lies in.  Returns the worst err / bound.  got / ref: [B, N, H, D], or [B, H, N] for LSE."""
    x = ratio(got, ref, bnd)
    worst = float(x.max())
    if worst <= 1.0:
        return worst
    n = int((x > 1.0).sum())
    ix = [int(i) for i in (x == x.max()).nonzero()[0]]
    if len(ix) == 4:
        b, row, h, d = ix
    else:
        (b, h, row), d = ix, 0
    e = tuple(ix)
    raise AssertionError(f"route [{route}] output {name}: {n} of {x.numel()} elements over the bound; worst (b {b}, h {h}, row {row}, d {d}) "
                         f"got {float(got[e]):.9g} ref {float(ref[e]):.9g} bound {float(bnd[e]):.3g} err/bound {worst:.3g} "
                         f"64-row tile {row // 64}, 128-row tile {row // 128}")


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
