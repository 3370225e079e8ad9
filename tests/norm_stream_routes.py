"""Route audit of GroupNorm (uniception_amd/csrc/groupnorm.hip, geometry in csrc/groupnorm_plan.h) and of the Cosmos tokenizer's streaming
kernels (csrc/cosmos.hip): routes, witness shapes, operands inside guard bands, the fp64 reference, the per-element bound and a CPU model of
each kernel's index arithmetic that can be given the defects these kernels can have.  No GPU code is imported;
`python -m tests.norm_stream_routes` prints the witness table.  The machinery (`_banded`, `bands_untouched`, `check`, `ratio`, GUARD,
SENTINEL, U_OUT, ACC, U24) is that of tests/head_stream_routes.py and tests/layernorm_routes.py.

ROUTES.  `route(w)` is a witness's route as text, `required_routes()` the list every pull request has to keep witnessed.
  gn    uc_group_norm_nhwc          act {none, relu} x {f, b, h}, kernel `stats` (cg % 8 == 0)
        uc_group_norm_silu_nhwc     {f, b, h} x kernel {`stats`, `stats4` (cg == 4: a channel vector spans two groups)}
  gnb   uc_group_norm_nhwc_bwd      act {none, relu (gate operand)} x {f, b, h}
        uc_group_norm_silu_nhwc_bwd {f, b, h} x {cg8, half}
  hp / hu                           uc_haar_patch / uc_haar_unpatch x {f, b, h} x {ld == 16 C, ld > 16 C}
  d2 / d2b / up / upb               uc_down2_gather, its adjoint, uc_upsample2_nhwc, its adjoint x {f, b, h}
  sm / smb                          uc_softmax_rows / _bwd x {f, b, h} x {vec, scalar} x {regs (N <= 4096), tail1 (one lap of the tail
                                    loop, N <= 6144), tail2}

WITNESSES, each the smallest shape at which its kernel can still go wrong; B = 2 unless said; the geometry in brackets is asserted against
tests/groupnorm_plan_driver.cpp (tests/test_norm_stream_routes.py), not trusted.  H x W is a real factorisation with an odd W where HW allows.
  plain GroupNorm (C, G, HW), forward and backward, act none and relu, the dtypes rotating over the shapes:
    (8, 1, 1), (8, 1, 7) [C8 = 1, rows = 256]; (48, 2, 43), (48, 2, 336), (48, 2, 337) [cg8 = 3, rows = 42, 4 dead threads, chunk = 336:
    the second register slot with one pixel, exactly one chunk, a second chunk of one pixel]; (24, 3, 5) [rows = 85, 1 dead thread], also
    with B = 3 (the sample sum of dgamma / dbeta); (24, 1, 5); (64, 2, 37 * 37) [6 chunks: 5 full + 89 pixels; the backward's four chains get
    2, 2, 1, 1]; (256, 32, 23 * 29) [11 chunks]; (1600, 2, 9) [rows = 1, 56 dead threads, chunks of 8 + 1 pixels, cg8 = 100];
    the large one (2048, 8, 523) [rows = 1, 66 chunks: lanes 0 and 1 of the finalize take a second chunk, the last chunk has 3 pixels, the
    backward chains get 17, 17, 16, 16, gs[2][GN_MAX_C] is full].
  SiLU entry: (128, 32, 20), (128, 32, 129) [half, rows = 16, chunk = 128]; (8, 2, 3) [half, C8 = 1]; (40, 10, 52) [half, rows = 51, one dead
    thread, the second slot with one pixel]; (2048, 512, 11) [half, G > 256: both `+= 256` laps; 2 chunks]; (2048, 512, 523) in bf16 (large);
    (256, 32, 33), (512, 32, 33) [cg8 = 1 and 2 under SiLU].
  Haar (B, C, H, W, ld): (2, 3, 4, 4, 48); (2, 3, 8, 12, 64) (two zero vectors per pixel), in every dtype; (1, 1, 4, 8, 16); (2, 5, 12, 20, 80);
    (2, 3, 36, 20, 48) (270 items: a ragged second workgroup); scale in {1, 16, 1 / 16} rotating.
  gathers and upsample (B, H, W, C): (1, 2, 2, 8), (2, 4, 6, 24), (2, 10, 6, 64); upsample also (1, 1, 1, 8), (2, 3, 5, 16); every dtype.
  softmax: rows = 3; N in {1, 7, 8, 12, 2048, 2049, 4096, 4097, 4104, 6152} contiguous (ld = N) and padded (lds = ldp = N rounded up to 64);
    N = 6153 contiguous (the scalar route with two tail laps: none of the listed N reaches it); N = 4090 with lds = ldp = 4160 (the tail stores
    whole zero vectors); N = 16 with the P pointer 4 bytes off 16-byte alignment (scalar route); scale in {512^-0.5, 1} rotating; every dtype.

INPUTS (`make_case`).  Operands are rounded to their storage dtype first; every buffer is a slice between NaN bands (inputs, their padding
columns NaN too) or starts as NaN between SENTINEL bands (outputs); the forward / backward workspace, mean and rstd are banded too and sized
by the `uc_*_ws_bytes` formula (gn_fwd_ws_bytes / gn_bwd_ws_bytes, checked against the driver and on the device against the entry points).
  GroupNorm families: `steps` (per (sample, group) mean 3 (g % 5) - 2 b and sd 0.5 + (g % 3): a wrong group or sample index moves every element
  by far more than the bound), `wide` N(0.5, 3^2), `offset` 100 + N(0, 1), `tiny` sd = sqrt(eps), `const` (`wide` with one (sample, group) set to
  one bf16-representable value, so fp32 sums of it are exact: y = act(beta), rstd = eps^-1/2).  All five on every small witness, the first
  two on the large ones.  gamma ~ 1 + 0.2 N, beta ~ 0.1 N, dy ~ N(0.25, 1).  The backward takes mean and rstd as operands: the fp64 values
  rounded to fp32.  The ReLU gate is an operand: the fp64 pre-activation rounded to the dtype, with exact +0 and -0 planted, both signs.
  Softmax families: `wide` 8 N(0, 1), `peak` (one logit 1e4 above the rest), `flat` (P = 1 / N), `neg` (all near -1e4).
  The Haar and gather kernels reuse `wide`, `ramp` and `spike` of tests/head_stream_routes.py.

REFERENCE: the expressions of include/uc_hip.h in float64 on the rounded operands.
BOUND per element, the constants of tests/gemm_routes.py (u_out = U_OUT of the store, an fp16 store term never below 2^-25; M = HW cg;
c = (|x| + |mean|) rstd; S = the expression on absolute values; E_EXP = 2 ulp for the device expf: ASSUMED, no HIP / OCML accuracy table was
found under the installed ROCm tree; it is not fitted to any device result):
    mean     U24 |ref| + ACC sqrt(M) mean_g |x|
    rstd     3 U24 |ref| + ACC sqrt(M) rstd^3 mean_g(|x - mean| (|x| + |mean|))        (half of d(var), d(d^2) = 2 |d| d|d|)
             RE-DERIVED from U24 |ref|: 1 / sqrtf(fl(var + eps)) rounds three times after the accumulation: the addition (U24 on var + eps,
             half of it on rstd), the square root (U24) and the division (U24), 2.5 U24 together; a constant group (accumulation term 0)
             shows it on the float32 CPU model at 1.05 U24
    t        e_t = ACC sqrt(M) (|gamma| c + |beta|)                                     (the pre-activation)
    y        u_out |ref| + L e_t;  L = 1 for none / relu;  L = 1.1 for SiLU, plus (2 E_EXP + 2) U24 |ref|
    dx       u_out |ref| + ACC sqrt(M) rstd (|a| + mean_g |a| + c mean_g(|a| c)),  a = g gamma, g = dy | dy gated | dy silu'(t)
             SiLU: g itself carries dg = |dy| (0.5 e_t + (2 E_EXP + 4) U24) (|silu''| <= 0.5; the evaluation of silu'); dg is an error of g, not
             of the accumulation, so it enters dx through the same expression WITHOUT the factor ACC sqrt(M):
             + rstd (D + mean_g D + c mean_g(D c)), D = |gamma| dg; likewise + sum dg c in dgamma and + sum dg in dbeta.
             Exactly 0 wherever the whole group's g is 0.
    dgamma   U24 |ref| + ACC sqrt(B HW) sum |g| c;   dbeta  U24 |ref| + ACC sqrt(B HW) sum |g|    (plain stores, no prefill)
    Haar patch    u_out |ref| + ACC sqrt(16) S;   Haar unpatch   U24 |ref| + ACC sqrt(16) S;   zero columns [16 C, ld) exactly 0
    down2 gather, upsample2   bound 0, also compared as integer views; the zero taps exactly 0
    down2 adjoint, upsample2 adjoint   u_out |ref| + n U24 S, n = the summed terms; n = 1: exact
    softmax P     ref (u_out + U24 (8 sqrt(N) + 2 E_EXP + d + sum_j P_j d_j)),  d = |z| + |z - m|, z = s scale (the error of m cancels between
                  numerator and denominator); columns [N, ldp) exactly 0; a reference below 2^-126 gets the absolute floor 2^-126
    softmax dS    u_out |ref| + ACC sqrt(N) |scale| P (|dP| + sum |dP| P),  P the operand as stored

MODEL (`model`): float32 torch on the CPU that follows each kernel's index arithmetic on the flat banded buffers: for GroupNorm the thread
(row, c8) layout with its dead threads, the per-chunk two-pass, Chan's merge in lane order and then in the butterfly's order, the four
backward chains, gn_group; it writes through the kernel's destination index, so a defect (`DEFECTS`) reads and writes what the device would.
REFERENCE BUDGET: no witness needs more than REF_BUDGET_ELEMS fp64 multiply-adds for reference and bound together.
"""
import math
import os
import re
import shutil
import subprocess

import torch

from tests.gemm_routes import BF16, F16, F32, ROOT, U_OUT      # noqa: F401
from tests.head_stream_routes import (ACC, BYTES, CODE, DT, GUARD, INTV, SENTINEL, U24, _banded, _draw, _emit, _fetch, _store_term,      # noqa: F401
                                      bands_untouched, check, ratio)

E_EXP = 2.0      # ulp of the device expf: assumed (see the docstring)
EPS = 1e-6
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))
GN_FAMILIES = ("steps", "wide", "offset", "tiny", "const")
SM_FAMILIES = ("wide", "peak", "flat", "neg")
HS_FAMILIES = ("wide", "ramp", "spike")
REF_BUDGET_ELEMS = 2.0e8
GN_OPS, HAAR_OPS, MOVE_OPS, SM_OPS = ("gn", "gnb"), ("hp", "hu"), ("d2", "d2b", "up", "upb"), ("sm", "smb")
OPS = GN_OPS + HAAR_OPS + MOVE_OPS + SM_OPS
BITS = ("d2", "up")      # pure moves: integer views are compared


def _plan_constants():
    "GN_THREADS, GN_VECS, GN_MAX_C of groupnorm_plan.h and SM_THREADS, SM_SLOTS of cosmos.hip: read, not retyped."
    csrc = os.path.join(ROOT, "uniception_amd", "csrc")
    out = {k: int(v) for k, v in re.findall(r"static constexpr int (GN_\w+) = (\d+);", open(os.path.join(csrc, "groupnorm_plan.h")).read())}
    out.update({k: int(v) for k, v in re.findall(r"#define (SM_\w+) (\d+)\b", open(os.path.join(csrc, "cosmos.hip")).read())})
    return out


PLAN = _plan_constants()
GN_THREADS, GN_VECS, GN_MAX_C = PLAN["GN_THREADS"], PLAN["GN_VECS"], PLAN["GN_MAX_C"]
SM_REGS = PLAN["SM_THREADS"] * PLAN["SM_SLOTS"] * 8      # columns a workgroup keeps in registers
SM_LAP = PLAN["SM_THREADS"] * 8                          # columns of one lap of the tail loop


def geom(C, G, HW):
    "gn_geom of groupnorm_plan.h, worked here."
    C8, cg = C // 8, C // G
    rows = GN_THREADS // C8
    return dict(C=C, G=G, HW=HW, C8=C8, cg=cg, cg8=cg // 8, half=int(cg == 4), rows=rows, chunk=rows * GN_VECS, nchunk=-(-HW // (rows * GN_VECS)),
                dead=GN_THREADS - rows * C8)


def ws_elems(w):
    "fp32 elements of the witness's workspace: gn_fwd_ws_bytes / gn_bwd_ws_bytes of groupnorm_plan.h over 4, worked here."
    gm, B = geom(w["C"], w["G"], w["H"] * w["W"]), w["B"]
    return B * gm["nchunk"] * w["G"] * 2 if w["op"] == "gn" else B * gm["nchunk"] * 2 * w["C"] + B * 2 * w["C"] + B * w["G"] * 2


def gn_shape_ok(B, H, W, C, G, group4):
    "The one shape rule of groupnorm_plan.h (without the grid limits), worked here."
    return min(B, H, W, C, G) > 0 and C % G == 0 and ((C // G) % 8 == 0 or (group4 and C // G == 4)) and C % 8 == 0 and C <= GN_MAX_C


# ------------------------------------------------------------------------------------------ witnesses
PLAIN = [(8, 1, 1, 1, 2), (8, 1, 1, 7, 2), (48, 2, 1, 43, 2), (48, 2, 16, 21, 2), (48, 2, 1, 337, 2), (24, 3, 1, 5, 2), (24, 1, 1, 5, 2), (64, 2, 37, 37, 2),
         (256, 32, 23, 29, 2), (1600, 2, 3, 3, 2), (24, 3, 1, 5, 3)]      # (C, G, H, W, B)
PLAIN_BIG = (2048, 8, 1, 523, 2)
SILU4 = [(128, 32, 4, 5), (128, 32, 3, 43), (8, 2, 1, 3), (40, 10, 4, 13), (2048, 512, 1, 11)]
SILU8 = [((256, 32, 3, 11), "fh"), ((512, 32, 3, 11), "b")]
SILU_BIG = (2048, 512, 1, 523)
HAAR = [(2, 3, 4, 4, 48), (1, 1, 4, 8, 16), (2, 5, 12, 20, 80), (2, 3, 36, 20, 48)]      # (B, C, H, W, ld), ld == 16 C
HAAR_PAD = (2, 3, 8, 12, 64)
HAAR_SCALES = (1.0, 16.0, 1.0 / 16.0)
MOVES = [(1, 2, 2, 8), (2, 4, 6, 24), (2, 10, 6, 64)]      # (B, H, W, C)
UP_EXTRA = [(1, 1, 1, 8), (2, 3, 5, 16)]
SM_ROWS = 3
SM_N = (1, 7, 8, 12, 2048, 2049, 4096, 4097, 4104, 6152)
SM_SCALES = (float(torch.tensor(512.0 ** -0.5, dtype=torch.float32)), 1.0)


def _w(op, dt, tag, big=False, **kw):
    return dict(name=f"{op}_{dt}_{tag}", op=op, dt=dt, big=big, **kw)


def _gn(op, dt, act, shape, B=2, big=False):
    C, G, H, W = shape
    return _w(op, dt, f"{act}_c{C}g{G}_{H}x{W}" + (f"_b{B}" if B != 2 else ""), big=big, act=act, C=C, G=G, H=H, W=W, B=B)


def _sm_shape(i, N, ld, mis=0):
    return dict(rows=SM_ROWS, N=N, lds=ld, ldp=ld, mis=mis, scale=SM_SCALES[i % 2])


def _witnesses():
    out = []
    for i, (C, G, H, W, B) in enumerate(PLAIN):
        for op in GN_OPS:
            out += [_gn(op, "fbh"[i % 3], "none", (C, G, H, W), B), _gn(op, "fbh"[(i + 1) % 3], "relu", (C, G, H, W), B)]
    out += [_gn("gn", "b", "none", PLAIN_BIG[:4], big=True), _gn("gn", "f", "relu", PLAIN_BIG[:4], big=True),
            _gn("gnb", "f", "none", PLAIN_BIG[:4], big=True), _gn("gnb", "b", "relu", PLAIN_BIG[:4], big=True)]
    for i, shape in enumerate(SILU4):
        out += [_gn(op, "fbh"[i % 3], "silu", shape) for op in GN_OPS]
    for shape, dts in SILU8:
        out += [_gn(op, dt, "silu", shape) for dt in dts for op in GN_OPS]
    out += [_gn(op, "b", "silu", SILU_BIG, big=True) for op in GN_OPS]
    for op in HAAR_OPS:
        for i, (B, C, H, W, ld) in enumerate(HAAR):
            out.append(_w(op, "fbh"[i % 3], f"b{B}c{C}_{H}x{W}_ld{ld}", B=B, C=C, H=H, W=W, ld=ld, scale=HAAR_SCALES[i % 3]))
        B, C, H, W, ld = HAAR_PAD
        out += [_w(op, dt, f"b{B}c{C}_{H}x{W}_ld{ld}", B=B, C=C, H=H, W=W, ld=ld, scale=HAAR_SCALES[(j + 1) % 3]) for j, dt in enumerate("fbh")]
    for dt in "fbh":
        for op in MOVE_OPS:
            out += [_w(op, dt, f"b{B}_{H}x{W}_c{C}", B=B, H=H, W=W, C=C) for B, H, W, C in MOVES + (UP_EXTRA if op in ("up", "upb") else [])]
        for op in SM_OPS:
            shapes = [("n%d" % N, _sm_shape(i, N, N)) for i, N in enumerate(SM_N + (6153,))]
            shapes += [("n%d_pad" % N, _sm_shape(i + 1, N, -(-N // 64) * 64)) for i, N in enumerate(SM_N)]
            shapes += [("n4090_ld4160", _sm_shape(0, 4090, 4160)), ("n16_mis", _sm_shape(0, 16, 16, mis=4 // BYTES[dt]))]
            out += [_w(op, dt, tag, **kw) for tag, kw in shapes]
    names = [w["name"] for w in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return {w["name"]: w for w in out}


WITNESSES = _witnesses()
NAMES = list(WITNESSES)
SMALL = [n for n in NAMES if not WITNESSES[n]["big"]]
BIG = [n for n in NAMES if WITNESSES[n]["big"]]


def seed_of(w):
    return NAMES.index(w["name"])


def families(w):
    "The input families a witness runs on: all of its operation's on a small witness, the first two on a large one."
    f = GN_FAMILIES if w["op"] in GN_OPS else SM_FAMILIES if w["op"] in SM_OPS else HS_FAMILIES
    return f[:2] if w["big"] else f


def gn_geom_of(w):
    return geom(w["C"], w["G"], w["H"] * w["W"])


def gn_kernel(w):
    return "stats4" if w["C"] // w["G"] == 4 else "stats"


def sm_vec(w):
    "SM_VEC of cosmos.hip: both leading dimensions multiples of 8 and every pointer 16-byte aligned."
    return w["lds"] % 8 == 0 and w["ldp"] % 8 == 0 and not w["mis"]


def sm_tail(w):
    return "regs" if w["N"] <= SM_REGS else "tail1" if w["N"] <= SM_REGS + SM_LAP else "tail2"


def route(w):
    op, dt = w["op"], w["dt"]
    if op == "gn":
        return f"uc_group_norm_silu_nhwc {gn_kernel(w)} {dt}" if w["act"] == "silu" else f"uc_group_norm_nhwc {w['act']} stats {dt}"
    if op == "gnb":
        return f"uc_group_norm_silu_nhwc_bwd {'half' if gn_kernel(w) == 'stats4' else 'cg8'} {dt}" if w["act"] == "silu" else f"uc_group_norm_nhwc_bwd {w['act']} {dt}"
    if op in HAAR_OPS:
        return f"uc_haar_{'patch' if op == 'hp' else 'unpatch'} {dt} ld{'=' if w['ld'] == 16 * w['C'] else '>'}16C"
    if op in MOVE_OPS:
        return {"d2": "uc_down2_gather", "d2b": "uc_down2_gather_bwd", "up": "uc_upsample2_nhwc", "upb": "uc_upsample2_nhwc_bwd"}[op] + f" {dt}"
    return f"uc_softmax_rows{'_bwd' if op == 'smb' else ''} {dt} {'vec' if sm_vec(w) else 'scalar'} {sm_tail(w)}"


def required_routes():
    "The routes of the issue's table, generated from the table and not from the witnesses."
    r = []
    for dt in "fbh":
        r += [f"uc_group_norm_nhwc {act} stats {dt}" for act in ("none", "relu")] + [f"uc_group_norm_silu_nhwc {k} {dt}" for k in ("stats", "stats4")]
        r += [f"uc_group_norm_nhwc_bwd {act} {dt}" for act in ("none", "relu")] + [f"uc_group_norm_silu_nhwc_bwd {k} {dt}" for k in ("cg8", "half")]
        r += [f"uc_haar_{p} {dt} ld{c}16C" for p in ("patch", "unpatch") for c in "=>"]
        r += [f"{e} {dt}" for e in ("uc_down2_gather", "uc_down2_gather_bwd", "uc_upsample2_nhwc", "uc_upsample2_nhwc_bwd")]
        r += [f"uc_softmax_rows{b} {dt} {v} {t}" for b in ("", "_bwd") for v in ("vec", "scalar") for t in ("regs", "tail1", "tail2")]
    return r


# ------------------------------------------------------------------------------------------ plan driver
def build_driver(tmpdir):
    "Compile tests/groupnorm_plan_driver.cpp with the system C++ compiler into tmpdir; returns run(rows of (C, G, H, W, group4[, B])) -> lines."
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/groupnorm_plan_driver.cpp"
    exe = os.path.join(str(tmpdir), "groupnorm_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "uniception_amd", "csrc"),
                           os.path.join(ROOT, "tests", "groupnorm_plan_driver.cpp"), "-o", exe])

    def run(rows):
        if not rows:
            return []
        text = "".join(" ".join(str(int(v)) for v in row) + "\n" for row in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return run


def driver_row(w):
    return (w["C"], w["G"], w["H"], w["W"], int(w["act"] == "silu"), w["B"])


def expected_plan(w):
    "The driver's line of a GroupNorm witness, worked here."
    gm = gn_geom_of(w)
    fwd, bwd = (ws_elems(dict(w, op=o)) * 4 for o in GN_OPS)
    return f"ok {gm['C8']} {gm['cg8']} {gm['half']} {gm['rows']} {gm['chunk']} {gm['nchunk']} {gm['dead']} {fwd} {bwd}"


# ------------------------------------------------------------------------------------------ operands
def buffers(w):
    "(inputs, outputs): lists of (name, shape, dtype char).  `ws` is an output that is banded and never compared."
    op, dt = w["op"], w["dt"]
    g = w.get
    if op in GN_OPS:
        m, v, s = (g("B"), g("H") * g("W"), g("C")), (g("C"),), (g("B") * g("G"),)
        if op == "gn":
            return [("x", m, dt), ("gamma", v, "f"), ("beta", v, "f")], [("y", m, dt), ("mean", s, "f"), ("rstd", s, "f"), ("ws", (ws_elems(w),), "f")]
        ins = [("dy", m, dt), ("x", m, dt)] + ([("gate", m, dt)] if g("act") == "relu" else []) + [("mean", s, "f"), ("rstd", s, "f"), ("gamma", v, "f")]
        return ins + ([("beta", v, "f")] if g("act") == "silu" else []), [("dx", m, dt), ("dgamma", v, "f"), ("dbeta", v, "f"), ("ws", (ws_elems(w),), "f")]
    if op in HAAR_OPS:
        img, rows = ("img", (g("B"), g("C"), g("H"), g("W")), "f"), ("rows", (g("B") * (g("H") // 4) * (g("W") // 4), g("ld")), dt)
        return ([img], [rows]) if op == "hp" else ([rows], [img])
    if op in MOVE_OPS:
        B, H, W, C = g("B"), g("H"), g("W"), g("C")
        a = (B, H, W, C)
        if op in ("d2", "d2b"):
            b = (B * (H // 2) * (W // 2), 9 * C)
            return ([("x", a, dt)], [("rows", b, dt)]) if op == "d2" else ([("drows", b, dt)], [("dx", a, dt)])
        b = (B, 2 * H, 2 * W, C)
        return ([("x", a, dt)], [("y", b, dt)]) if op == "up" else ([("dy", b, dt)], [("dx", a, dt)])
    s, p = (g("rows"), g("lds")), (g("rows"), g("ldp"))
    return ([("S", s, "f")], [("P", p, dt)]) if op == "sm" else ([("P", p, dt), ("dP", s, "f")], [("dS", p, dt)])


def outputs(w):
    "The outputs that are compared with the reference."
    return tuple(n for n, _, _ in buffers(w)[1] if n != "ws")


def banded_outputs(w):
    return tuple(n for n, _, _ in buffers(w)[1])


def _gn_x(w, family, g, device):
    B, HW, C, G = w["B"], w["H"] * w["W"], w["C"], w["G"]
    cg = C // G
    r = torch.randn(B, HW, G, cg, generator=g, device=device)
    if family == "steps":
        gi, bi = torch.arange(G, device=device).view(1, 1, G, 1), torch.arange(B, device=device).view(B, 1, 1, 1)
        x = (3.0 * (gi % 5) - 2.0 * bi).float() + (0.5 + (gi % 3).float()) * r
    elif family == "offset":
        x = 100.0 + r
    elif family == "tiny":
        x = math.sqrt(EPS) * r
    else:
        x = 0.5 + 3.0 * r
        if family == "const":      # one bf16 value: the fp32 sums of up to 2^16 copies of it are exact
            x[B - 1, :, G // 2, :] = x[B - 1, 0, G // 2, 0].bfloat16().float()
    return x.view(B, HW, C)


def _gn_stats64(w, x):
    "(mean, rstd) [B, 1, G, 1] of x [B, HW, C] in float64."
    x = x.double().view(w["B"], -1, w["G"], w["C"] // w["G"])
    mean = x.mean(dim=(1, 3), keepdim=True)
    return mean, (((x - mean) ** 2).mean(dim=(1, 3), keepdim=True) + EPS32) ** -0.5


def _sm_logits(w, family, g, device):
    rows, N = w["rows"], w["N"]
    r = torch.randn(rows, N, generator=g, device=device)
    if family == "wide":
        return 8.0 * r
    if family == "peak":
        r[torch.arange(rows), (torch.arange(rows) * 5 + N - 1) % N] += 1e4      # row 0: the last column
        return r
    if family == "flat":
        return torch.full((rows, N), 0.75, device=device)
    return -1e4 + r


def make_case(w, family, device, seed=0):
    """Seeded operands and output buffers of a witness on `device`: t[name] is the shaped view, t[name + "_buf"] the flat banded buffer and
    t[name + "_at"] the view's first element in it."""
    assert family in families(dict(w, big=False)), (family, w["name"])
    g = torch.Generator(device=device).manual_seed(11000 + seed)
    nan = float("nan")
    op, dt = w["op"], w["dt"]
    ins, outs = buffers(w)
    val = {}
    if op in GN_OPS:
        x = _gn_x(w, family, g, device).to(DT[dt])
        val["x"] = x
        val["gamma"] = 1.0 + 0.2 * torch.randn(w["C"], generator=g, device=device)
        val["beta"] = 0.1 * torch.randn(w["C"], generator=g, device=device)
        if op == "gnb":
            val["dy"] = (0.25 + torch.randn(x.shape, generator=g, device=device)).to(DT[dt])
            mean, rstd = _gn_stats64(w, x)
            val["mean"], val["rstd"] = mean.float().flatten(), rstd.float().flatten()
            if w["act"] == "relu":
                cg = w["C"] // w["G"]
                t64 = (x.double().view(w["B"], -1, w["G"], cg) - mean) * rstd * val["gamma"].double().view(1, 1, w["G"], cg) + val["beta"].double().view(1, 1, w["G"], cg)
                gate = t64.to(DT[dt]).flatten()
                gate[0::7] = 0.0
                gate[3::7] = -0.0
                val["gate"] = gate
    elif op in HAAR_OPS:
        name, shape, _ = ins[0]
        v = _draw(shape, family, g, device, adjoint=False).to(DT[dt] if op == "hu" else torch.float32)
        if op == "hu":
            v[:, 16 * w["C"]:] = nan
        val[name] = v
    elif op in MOVE_OPS:
        name, shape, _ = ins[0]
        val[name] = _draw(shape, family, g, device, adjoint=False).to(DT[dt])
    else:
        s = _sm_logits(w, family, g, device)
        S = torch.full((w["rows"], w["lds"]), nan, device=device)
        S[:, :w["N"]] = s
        if op == "sm":
            val["S"] = S
        else:
            P = torch.full((w["rows"], w["ldp"]), nan, device=device, dtype=DT[dt])
            P[:, :w["N"]] = torch.softmax(s.double() * w["scale"], 1).to(DT[dt])
            S[:, :w["N"]] = torch.randn(w["rows"], w["N"], generator=g, device=device)
            val["P"], val["dP"] = P, S
    t = {}
    for name, shape, d in ins:
        off = w.get("mis", 0) if name == "P" else 0
        buf, at, view = _banded(math.prod(shape), DT[d], device, nan, val[name].to(DT[d]).flatten(), off=off)
        t[name + "_buf"], t[name + "_at"], t[name] = buf, at, view.view(shape)
    for name, shape, d in outs:
        off = w.get("mis", 0) if name == "P" else 0
        buf, at, view = _banded(math.prod(shape), DT[d], device, SENTINEL, nan, off=off)
        t[name + "_buf"], t[name + "_at"], t[name] = buf, at, view.view(shape)
    return t


def results(w, t, bufs=None):
    "{output: tensor} of what a launch (or `model`: bufs) left."
    out = {}
    for name in outputs(w):
        out[name] = t[name] if bufs is None else bufs[name][t[name + "_at"]:t[name + "_at"] + t[name].numel()].view(t[name].shape)
    return out


def bands_ok(w, t, bufs=None):
    "Whether the sentinel bands around every output, the workspace included, are untouched."
    return all(bands_untouched(t[n + "_buf"] if bufs is None or n not in bufs else bufs[n], t[n + "_at"], t[n].numel()) for n in banded_outputs(w))


# ------------------------------------------------------------------------------------------ reference and bound
def _st(front, ref, code):
    "The store's term of a bound; `front`: of the value in front of the store (fp32's rounding)."
    return U24 * ref.abs() if front else _store_term(ref, code)


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _ref_gn(w, t, front=False):
    op, code = w["op"], CODE[w["dt"]]
    B, HW, C, G = w["B"], w["H"] * w["W"], w["C"], w["G"]
    cg = C // G
    M = HW * cg
    v4 = lambda a: a.double().view(B, HW, G, cg)      # noqa: E731
    p4 = lambda a: a.double().view(1, 1, G, cg)      # noqa: E731
    red = lambda a: a.mean(dim=(1, 3), keepdim=True)      # noqa: E731
    x, gamma = v4(t["x"]), p4(t["gamma"])
    beta = p4(t["beta"]) if "beta" in t else torch.zeros_like(gamma)
    if op == "gn":
        mean, rstd = _gn_stats64(w, t["x"])
    else:
        mean, rstd = t["mean"].double().view(B, 1, G, 1), t["rstd"].double().view(B, 1, G, 1)
    ax = x.abs()
    c = (ax + mean.abs()) * rstd
    xh = (x - mean) * rstd
    tt = xh * gamma + beta
    e_t = ACC * math.sqrt(M) * (gamma.abs() * c + beta.abs())
    if op == "gn":
        y = {"none": tt, "relu": tt.clamp(min=0) + 0.0, "silu": tt * torch.sigmoid(tt)}[w["act"]]
        by = _st(front, y, code) + (1.1 * e_t + (2 * E_EXP + 2) * U24 * y.abs() if w["act"] == "silu" else e_t)
        bm = U24 * mean.abs() + ACC * math.sqrt(M) * red(ax)
        br = 3 * U24 * rstd.abs() + ACC * math.sqrt(M) * rstd ** 3 * red((x - mean).abs() * (ax + mean.abs()))
        return {"y": (y.view(B, HW, C), by.view(B, HW, C)), "mean": (mean.flatten(), bm.flatten()), "rstd": (rstd.flatten(), br.flatten())}
    dy = v4(t["dy"])
    dg = torch.zeros_like(dy)
    if w["act"] == "relu":
        g = dy * (v4(t["gate"]) > 0)
    elif w["act"] == "silu":
        g = dy * _silu_grad(tt)
        dg = dy.abs() * (0.5 * e_t + (2 * E_EXP + 4) * U24)
    else:
        g = dy
    a, A, D = g * gamma, (g * gamma).abs(), gamma.abs() * dg
    dx = rstd * (a - red(a) - xh * red(a * xh))
    S = rstd * (A + red(A) + c * red(A * c))
    bdx = (_st(front, dx, code) + ACC * math.sqrt(M) * S + rstd * (D + red(D) + c * red(D * c))) * (red(g.abs()) > 0)
    dgam, dbet = (g * xh).sum(dim=(0, 1)).flatten(), g.sum(dim=(0, 1)).flatten()
    n = math.sqrt(B * HW)
    bg = U24 * dgam.abs() + ACC * n * (g.abs() * c).sum(dim=(0, 1)).flatten() + (dg * c).sum(dim=(0, 1)).flatten()
    bb = U24 * dbet.abs() + ACC * n * g.abs().sum(dim=(0, 1)).flatten() + dg.sum(dim=(0, 1)).flatten()
    return {"dx": (dx.view(B, HW, C), bdx.view(B, HW, C)), "dgamma": (dgam, bg), "dbeta": (dbet, bb)}


def haar4(a, b, c, d, swapped=False):
    "haar4 of cosmos.hip: (ll, lh, hl, hh) of a 2x2 block (a b / c d); `swapped`: the defect that exchanges lh and hl."
    s0, s1, d0, d1 = a + b, c + d, a - b, c - d
    return (s0 + s1, d0 + d1, s0 - s1, d0 - d1) if swapped else (s0 + s1, s0 - s1, d0 + d1, d0 - d1)


def haar_patch(x, swapped=False):
    "Both levels on x [B, C, H, W] in x's precision, unscaled: coef[s2][s1] as [B, C, H / 4, W / 4]."
    B, C, H, W = x.shape
    v = x.reshape(B, C, H // 4, 2, 2, W // 4, 2, 2)      # [.., i, u, row in the 2x2 block, j, v, column in the 2x2 block]
    l1 = haar4(v[:, :, :, :, 0, :, :, 0], v[:, :, :, :, 0, :, :, 1], v[:, :, :, :, 1, :, :, 0], v[:, :, :, :, 1, :, :, 1], swapped)      # each [B, C, i, u, j, v]
    per_s1 = [haar4(s[:, :, :, 0, :, 0], s[:, :, :, 0, :, 1], s[:, :, :, 1, :, 0], s[:, :, :, 1, :, 1], swapped) for s in l1]
    return [[per_s1[s1][s2] for s1 in range(4)] for s2 in range(4)]


def haar_unpatch(p, swapped=False):
    "The inverse on p[s2][s1], each [B, C, h4, w4] (already scaled): x [B, C, H, W]."
    B, C, h4, w4 = p[0][0].shape
    l1 = [haar4(p[0][s1], p[1][s1], p[2][s1], p[3][s1], swapped) for s1 in range(4)]      # l1[s1][2 u + v]
    x = torch.zeros(B, C, h4, 2, 2, w4, 2, 2, dtype=p[0][0].dtype, device=p[0][0].device)
    for u in range(2):
        for v in range(2):
            o = haar4(*(l1[s1][2 * u + v] for s1 in range(4)), swapped)
            for k in range(4):
                x[:, :, :, u, k // 2, :, v, k % 2] = o[k]
    return x.view(B, C, 4 * h4, 4 * w4)


def _rows_to_coef(rows, w, order=lambda s2, s1: s2 * 4 + s1):
    "rows [B h4 w4, ld] -> p[s2][s1] [B, C, h4, w4]."
    B, C, h4, w4 = w["B"], w["C"], w["H"] // 4, w["W"] // 4
    r = rows.view(B, h4, w4, -1)
    return [[r[..., order(s2, s1) * C:order(s2, s1) * C + C].permute(0, 3, 1, 2) for s1 in range(4)] for s2 in range(4)]


def _ref_haar(w, t, front=False):
    B, C, H, W, ld, scale = (w[k] for k in ("B", "C", "H", "W", "ld", "scale"))
    code = CODE[w["dt"]]
    if w["op"] == "hp":
        x = t["img"].double()
        coef = haar_patch(x)
        S = x.abs().view(B, C, H // 4, 4, W // 4, 4).sum(dim=(3, 5)) * abs(scale) / 16      # the same for all 16 coefficients
        ref = torch.zeros(B, H // 4, W // 4, ld, dtype=torch.float64, device=x.device)
        bnd = torch.zeros_like(ref)
        for s2 in range(4):
            for s1 in range(4):
                k = (s2 * 4 + s1) * C
                ref[..., k:k + C] = (coef[s2][s1] * (scale / 16)).permute(0, 2, 3, 1)
                bnd[..., k:k + C] = _st(front, ref[..., k:k + C], code) + ACC * 4.0 * S.permute(0, 2, 3, 1)
        return {"rows": (ref.view(-1, ld), bnd.view(-1, ld))}
    rows = t["rows"].double() * scale
    ref = haar_unpatch(_rows_to_coef(rows, w))
    S = sum(sum(p.abs() for p in ps) for ps in _rows_to_coef(rows, w))      # [B, C, h4, w4]
    S = S.view(B, C, H // 4, 1, W // 4, 1).expand(B, C, H // 4, 4, W // 4, 4).reshape(B, C, H, W)
    return {"img": (ref, U24 * ref.abs() + ACC * 4.0 * S)}


def _d2_taps(w, dev):
    "(y, x, valid) [Ho, Wo, 9] of the Downsample's taps: the map padded by one row below and one column to the right."
    H, W = w["H"], w["W"]
    i, j, tap = torch.arange(H // 2, device=dev).view(-1, 1, 1), torch.arange(W // 2, device=dev).view(1, -1, 1), torch.arange(9, device=dev).view(1, 1, 9)
    y, x = 2 * i + tap // 3 + 0 * j, 2 * j + tap % 3 + 0 * i
    return y, x, (y < H) & (x < W)


def _ref_moves(w, t, front=False):
    op, code = w["op"], CODE[w["dt"]]
    B, H, W, C = w["B"], w["H"], w["W"], w["C"]
    z = lambda r: (r, torch.zeros_like(r))      # noqa: E731
    if op == "up":
        return {"y": z(t["x"].double().repeat_interleave(2, 1).repeat_interleave(2, 2))}
    if op == "upb":
        g = t["dy"].double().view(B, H, 2, W, 2, C)
        ref, S = g.sum(dim=(2, 4)), g.abs().sum(dim=(2, 4))
        return {"dx": (ref, _st(front, ref, code) * (S > 0) + 4 * U24 * S)}
    dev = t["x" if op == "d2" else "drows"].device
    y, x, ok = _d2_taps(w, dev)
    if op == "d2":
        src = t["x"].double()
        r = src[:, y.clamp(max=H - 1), x.clamp(max=W - 1)] * ok[None, ..., None]      # [B, Ho, Wo, 9, C]
        return {"rows": z(r.reshape(-1, 9 * C) + 0.0)}
    g = t["drows"].double().view(B, H // 2, W // 2, 9, C)
    ref, S, n = (torch.zeros(B, H * W, C, dtype=torch.float64, device=dev) for _ in range(3))
    flat = (y * W + x)[ok]
    ref.index_add_(1, flat, g[:, ok])
    S.index_add_(1, flat, g[:, ok].abs())
    n.index_add_(1, flat, torch.ones_like(g[:, ok]))
    ref, S, n = (v.view(B, H, W, C) for v in (ref, S, n))
    return {"dx": (ref, torch.where(n > 1, _st(front, ref, code) * (S > 0) + n * U24 * S, torch.zeros_like(ref)))}


def _ref_sm(w, t, front=False):
    op, code, N, scale = w["op"], CODE[w["dt"]], w["N"], w["scale"]
    if op == "sm":
        z = t["S"][:, :N].double() * scale
        m = z.max(1, keepdim=True).values
        P = torch.softmax(z, 1)
        d = z.abs() + (z - m).abs()
        acc = P * U24 * (8 * math.sqrt(N) + 2 * E_EXP + d + (P * d).sum(1, keepdim=True))
        bnd = _st(front, P, code) + torch.where(P < 2.0 ** -126, acc.clamp(min=2.0 ** -126), acc)
        ref, b = torch.zeros(t["P"].shape, dtype=torch.float64, device=z.device), torch.zeros(t["P"].shape, dtype=torch.float64, device=z.device)
        ref[:, :N], b[:, :N] = P, bnd
        return {"P": (ref, b)}
    P, g = t["P"][:, :N].double(), t["dP"][:, :N].double()
    dS = scale * P * (g - (g * P).sum(1, keepdim=True))
    bnd = _st(front, dS, code) * (P > 0) + ACC * math.sqrt(N) * abs(scale) * P * (g.abs() + (g.abs() * P).sum(1, keepdim=True))
    ref, b = torch.zeros(t["dS"].shape, dtype=torch.float64, device=P.device), torch.zeros(t["dS"].shape, dtype=torch.float64, device=P.device)
    ref[:, :N], b[:, :N] = dS, bnd
    return {"dS": (ref, b)}


def reference(w, t, front=False):
    """{output: (ref, bound)} in float64 on the device of the case; bound 0: exact.  `front`: the bound of the value in front of the store
    (the store's own rounding replaced by fp32's; worked term by term, since subtracting an fp16 store term of 2^-25 from the bound of a tiny
    softmax value cancels in float64)."""
    op = w["op"]
    return (_ref_gn if op in GN_OPS else _ref_haar if op in HAAR_OPS else _ref_moves if op in MOVE_OPS else _ref_sm)(w, t, front)


def store_code(w, o):
    return CODE[w["dt"]] if o in ("y", "dx", "rows", "P", "dS") else F32


def reference_elems(w):
    "fp64 multiply-adds of reference and bound together, to an order of magnitude: what REF_BUDGET_ELEMS limits."
    ins, outs = buffers(w)
    return 20 * sum(math.prod(s) for n, s, _ in ins + outs if n != "ws")


# ------------------------------------------------------------------------------------------ model
# defect -> the operations it belongs to.  What each one is, in the kernels' terms:
#   last_chunk_count_full          gn_stats_partial*: `cnt` from chunk_pix instead of the chunk's own pixel count
#   dead_thread_counted            the workgroup reductions walk ceil(256 / C8) rows and the `active` mask is gone: the dead threads' values
#                                  (pixels rows, 2 rows, .. of the chunk, read once more) are added
#   half_groups_swapped            gn_group under `half`: 2 c8 + 1 - hi
#   group_from_c8_mod              gn_group: c8 % cg8 for c8 / cg8
#   finalize_second_lap_dropped    gn_stats_finalize: `if` for the `k += 64` loop
#   chan_counts_equal              gn_stats_finalize: every chunk merged with the count of a full chunk
#   group_loop_stops_at_256        gn_stats_partial4 / gn_bwd_finalize: `if (tid < G)` for the `g += 256` loop: groups >= 256 stay unwritten
#   bwd_chain_tail_dropped         gn_bwd_finalize: the chains stop at the last whole lap of four chunks
#   sample_sum_skips_last          gn_bwd_params: `b < B - 1`
#   inv_m_from_C                   inv_m = 1 / (HW C)
#   relu_gate_ge_zero              `yv >= 0`
#   silu_grad_without_z_term       silu'(z) = sigmoid(z)
#   eps_outside_sqrt               rstd = 1 / (sqrt(var) + eps)
#   stats_of_previous_sample       the apply kernels index mean / rstd / S with sample b - 1 (sample 0: the last one)
#   haar_levels_transposed         column (s1 * 4 + s2) C;  haar_lh_hl_swapped: haar4 returns hl for lh;  haar_pad_unwritten: no zero columns;
#   haar_scale_without_sixteenth   f = scale
#   down2_bottom_pad_reads_next_row / down2_right_pad_reads_next_pixel   the `y < H` / `xx < W` guard gone
#   down2_bwd_third_tap_dropped    `ky < 2`, `kx < 2`;  down2_bwd_negative_index_unguarded: without `p.y < ky` / `p.x < kx`
#   up_bwd_row_stride_W            the second row at base + W C
#   sm_tail_left_out_of_max / _of_sum   the tail loop missing in that pass;  sm_pad_columns_unwritten: stores stop at N
#   sm_fill_zero_in_max            the columns behind N of the last vector enter the maximum as 0 * scale
#   sm_scale_after_max             the maximum of the unscaled logits
#   smb_dot_without_tail           the tail loop missing in the dot product
DEFECTS = {"last_chunk_count_full": ("gn",), "dead_thread_counted": ("gn", "gnb"), "half_groups_swapped": ("gn", "gnb"), "group_from_c8_mod": ("gn", "gnb"),
           "finalize_second_lap_dropped": ("gn",), "chan_counts_equal": ("gn",), "group_loop_stops_at_256": ("gn", "gnb"),
           "bwd_chain_tail_dropped": ("gnb",), "sample_sum_skips_last": ("gnb",), "inv_m_from_C": ("gnb",), "relu_gate_ge_zero": ("gnb",),
           "silu_grad_without_z_term": ("gnb",), "eps_outside_sqrt": ("gn",), "stats_of_previous_sample": ("gn", "gnb"),
           "haar_levels_transposed": ("hp", "hu"), "haar_lh_hl_swapped": ("hp", "hu"), "haar_pad_unwritten": ("hp",), "haar_scale_without_sixteenth": ("hp",),
           "down2_bottom_pad_reads_next_row": ("d2",), "down2_right_pad_reads_next_pixel": ("d2",), "down2_bwd_third_tap_dropped": ("d2b",),
           "down2_bwd_negative_index_unguarded": ("d2b",), "up_bwd_row_stride_W": ("upb",),
           "sm_tail_left_out_of_max": ("sm",), "sm_tail_left_out_of_sum": ("sm",), "sm_pad_columns_unwritten": ("sm", "smb"), "sm_fill_zero_in_max": ("sm",),
           "sm_scale_after_max": ("sm",), "smb_dot_without_tail": ("smb",)}
NAN = float("nan")


def _own(bufs, t, name, idx):
    "What loads at element offsets idx of one of the launch's OWN outputs (mean, rstd written by an earlier kernel) return."
    flat = bufs[name].float()
    at = t[name + "_at"] + idx
    ok = (at >= 0) & (at < flat.numel())
    return torch.where(ok, flat[at.clamp(0, flat.numel() - 1)], torch.full((), NAN))


def _chunked(T, gm):
    "[B, HW, C] -> [B, nchunk, chunk_pix, C], zeros behind the map."
    out = torch.zeros(T.shape[0], gm["nchunk"] * gm["chunk"], gm["C"])
    out[:, :gm["HW"]] = T
    return out.view(T.shape[0], gm["nchunk"], gm["chunk"], gm["C"])


def _chunk_channel_sum(Tc, gm, defect):
    "The workgroup's sum per channel: a thread (row r, vector c8) over its GN_VECS pixels j * rows + r, then the rows."
    B, rows, dead = Tc.shape[0], gm["rows"], gm["dead"]
    col = Tc.view(B, gm["nchunk"], GN_VECS, rows, gm["C"]).sum(2).sum(2)
    if defect == "dead_thread_counted" and dead:
        col = col.clone()
        col[..., :dead * 8] += Tc[:, :, rows::rows, :dead * 8].sum(2)
    return col


def _channel_group(gm, defect):
    "gn_group per channel [C]."
    c = torch.arange(gm["C"])
    c8, hi = c // 8, (c % 8) // 4
    if gm["half"]:
        return 2 * c8 + (1 - hi if defect == "half_groups_swapped" else hi)
    return c8 % gm["cg8"] if defect == "group_from_c8_mod" else c8 // gm["cg8"]


def _sample(B, defect):
    b = torch.arange(B)
    return (b + B - 1) % B if defect == "stats_of_previous_sample" else b


def _gn_merge(na, ma, Ma, nb, mb, Mb):
    "gn_merge of groupnorm.hip: counts in double, the rest in float."
    n = na + nb
    f = torch.where(n > 0, nb / n.clamp(min=1), torch.zeros_like(n)).float()
    d = mb - ma
    return n, ma + d * f, (Ma + Mb) + (d * d) * (na.float() * f)


def _model_gn(w, t, bufs, defect):
    gm = gn_geom_of(w)
    B, HW, C, G, cg, nchunk, chunk = w["B"], gm["HW"], w["C"], w["G"], gm["cg"], gm["nchunk"], gm["chunk"]
    X = _fetch(t, "x", torch.arange(B * HW * C)).view(B, HW, C)
    gamma, beta = _fetch(t, "gamma", torch.arange(C)), _fetch(t, "beta", torch.arange(C))
    valid = (torch.arange(nchunk * chunk) < HW).view(1, nchunk, chunk, 1)
    npix = valid.sum(2).float().view(1, nchunk, 1)
    cnt = (torch.full_like(npix, chunk) if defect == "last_chunk_count_full" else npix) * float(cg)
    Xc = _chunked(X, gm)
    grp = lambda col: col.view(B, nchunk, G, cg).sum(3)      # noqa: E731  (cg8 vectors of a group, or one half of a vector)
    mean_c = grp(_chunk_channel_sum(Xc, gm, defect)) / cnt
    D = torch.where(valid, Xc - mean_c.repeat_interleave(cg, 2).view(B, nchunk, 1, C), torch.zeros(()))
    m2_c = grp(_chunk_channel_sum(D * D, gm, defect))
    if defect == "group_loop_stops_at_256" and gm["half"]:
        mean_c[..., GN_THREADS:], m2_c[..., GN_THREADS:] = NAN, NAN      # the workspace's prefill
    # finalize: lane l merges chunks l, l + 64, ..; then the butterfly, the lower lane's triple on the left
    n_k = (torch.full_like(npix, chunk) if defect == "chan_counts_equal" else npix).double().view(1, nchunk, 1) * cg
    laps = 1 if defect == "finalize_second_lap_dropped" else -(-nchunk // 64)
    pad = lambda v, fill: torch.cat([v.expand(B, nchunk, G), torch.full((B, max(laps * 64 - nchunk, 0), G), fill, dtype=v.dtype)], 1)[:, :laps * 64]      # noqa: E731
    nk, mk, Mk = (pad(v, 0.0).view(B, laps, 64, G) for v in (n_k, mean_c, m2_c))
    n, mu, m2 = torch.zeros(B, 64, G, dtype=torch.float64), torch.zeros(B, 64, G), torch.zeros(B, 64, G)
    live = (torch.arange(laps * 64) < nchunk).view(1, laps, 64, 1)
    for lap in range(laps):
        n2, mu2, m22 = _gn_merge(n, mu, m2, nk[:, lap], mk[:, lap], Mk[:, lap])
        n, mu, m2 = (torch.where(live[:, lap], a, b) for a, b in ((n2, n), (mu2, mu), (m22, m2)))
    lane = torch.arange(64)
    o = 1
    while o < 64:
        lo, hi = lane & ~o, lane | o
        n, mu, m2 = _gn_merge(n[:, lo], mu[:, lo], m2[:, lo], n[:, hi], mu[:, hi], m2[:, hi])
        o *= 2
    var = (m2[:, 0].double() / n[:, 0]).float()
    rstd = 1.0 / (var.sqrt() + EPS32) if defect == "eps_outside_sqrt" else 1.0 / (var + EPS32).sqrt()
    _emit(bufs, t, "mean", torch.arange(B * G).view(B, G), mu[:, 0])
    _emit(bufs, t, "rstd", torch.arange(B * G).view(B, G), rstd)
    sg = _sample(B, defect).view(B, 1) * G + _channel_group(gm, defect).view(1, C)
    mu_c, rs_c = _own(bufs, t, "mean", sg).view(B, 1, C), _own(bufs, t, "rstd", sg).view(B, 1, C)
    tt = (X - mu_c) * rs_c * gamma + beta
    y = {"none": tt, "relu": torch.where(tt > 0, tt, torch.zeros(())), "silu": tt / (1.0 + torch.exp(-tt))}[w["act"]]      # fmaxf(NaN, 0) = 0
    _emit(bufs, t, "y", torch.arange(B * HW * C).view(B, HW, C), y)


def _model_gnb(w, t, bufs, defect):
    gm = gn_geom_of(w)
    B, HW, C, G, cg, nchunk = w["B"], gm["HW"], w["C"], w["G"], gm["cg"], gm["nchunk"]
    it = torch.arange(B * HW * C)
    X, g = _fetch(t, "x", it).view(B, HW, C), _fetch(t, "dy", it).view(B, HW, C)
    gamma = _fetch(t, "gamma", torch.arange(C))
    sg = _sample(B, defect).view(B, 1) * G + _channel_group(gm, defect).view(1, C)
    mu, rs = _fetch(t, "mean", sg).view(B, 1, C), _fetch(t, "rstd", sg).view(B, 1, C)
    xh = (X - mu) * rs
    if w["act"] == "relu":
        gate = _fetch(t, "gate", it).view(B, HW, C)
        g = torch.where((gate >= 0) if defect == "relu_gate_ge_zero" else (gate > 0), g, torch.zeros(()))
    elif w["act"] == "silu":
        z = xh * gamma + _fetch(t, "beta", torch.arange(C))
        s = 1.0 / (1.0 + torch.exp(-z))
        g = g * (s if defect == "silu_grad_without_z_term" else s * (z * (1.0 - s) + 1.0))
    part_a, part_b = _chunk_channel_sum(_chunked(g * xh, gm), gm, defect), _chunk_channel_sum(_chunked(g, gm), gm, defect)      # [B, nchunk, C]
    laps = nchunk // 4 if defect == "bwd_chain_tail_dropped" else -(-nchunk // 4)

    def chains(p):
        p = torch.cat([p, torch.zeros(B, 4 * (nchunk // 4 + 1) - nchunk, C)], 1).view(B, -1, 4, C)
        acc = torch.zeros(B, 4, C)
        for lap in range(laps):
            acc = acc + p[:, lap]
        return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    t0, t1 = chains(part_a), chains(part_b)      # pc [B][2][C]
    S1, S2 = (gamma * t1).view(B, G, cg).sum(2), (gamma * t0).view(B, G, cg).sum(2)
    if defect == "group_loop_stops_at_256":
        S1[:, 256:], S2[:, 256:] = NAN, NAN      # the workspace's prefill
    nb = B - 1 if defect == "sample_sum_skips_last" else B
    _emit(bufs, t, "dgamma", torch.arange(C), t0[:nb].sum(0))
    _emit(bufs, t, "dbeta", torch.arange(C), t1[:nb].sum(0))
    inv_m = float(torch.tensor(1.0 / (HW * (C if defect == "inv_m_from_C" else cg)), dtype=torch.float32))
    flat = lambda S: torch.cat([S.flatten(), torch.full((G,), NAN)])[sg.clamp(max=B * G)].view(B, 1, C) * inv_m      # noqa: E731  (behind S: the band)
    dx = rs * ((g * gamma - flat(S1)) - xh * flat(S2))
    _emit(bufs, t, "dx", it.view(B, HW, C), dx)


def _model_haar(w, t, bufs, defect):
    B, C, H, W, ld, scale = (w[k] for k in ("B", "C", "H", "W", "ld", "scale"))
    h4, w4 = H // 4, W // 4
    swapped = defect == "haar_lh_hl_swapped"
    order = (lambda s2, s1: s1 * 4 + s2) if defect == "haar_levels_transposed" else (lambda s2, s1: s2 * 4 + s1)
    row = ((torch.arange(B).view(B, 1, 1, 1) * h4 + torch.arange(h4).view(1, 1, h4, 1)) * w4 + torch.arange(w4).view(1, 1, 1, w4)) * ld + torch.arange(C).view(1, C, 1, 1)
    if w["op"] == "hp":
        coef = haar_patch(_fetch(t, "img", torch.arange(B * C * H * W)).view(B, C, H, W), swapped)
        f = float(torch.tensor(scale, dtype=torch.float32) * (1.0 if defect == "haar_scale_without_sixteenth" else torch.tensor(1.0 / 16.0)))
        for s2 in range(4):
            for s1 in range(4):
                _emit(bufs, t, "rows", row + order(s2, s1) * C, coef[s2][s1] * f)
        if defect != "haar_pad_unwritten" and ld > 16 * C:
            k = torch.arange(16 * C, ld).view(1, 1, 1, -1)
            _emit(bufs, t, "rows", row[:, :1].permute(0, 2, 3, 1) + k, torch.zeros(()))
        return
    p = [[_fetch(t, "rows", row + order(s2, s1) * C) * torch.tensor(scale, dtype=torch.float32) for s1 in range(4)] for s2 in range(4)]
    _emit(bufs, t, "img", torch.arange(B * C * H * W).view(B, C, H, W), haar_unpatch(p, swapped))


def _model_moves(w, t, bufs, defect):
    op = w["op"]
    B, H, W, C = w["B"], w["H"], w["W"], w["C"]
    if op == "d2":
        Ho, Wo = H // 2, W // 2
        it = torch.arange(B * Ho * Wo * 9 * C)
        c, r = it % C, it // C
        tap, r = r % 9, r // 9
        j, r = r % Wo, r // Wo
        i, b = r % Ho, r // Ho
        y, x = 2 * i + tap // 3, 2 * j + tap % 3
        ok = ((y < H) | (defect == "down2_bottom_pad_reads_next_row")) & ((x < W) | (defect == "down2_right_pad_reads_next_pixel"))
        v = _fetch(t, "x", (((b * H + y) * W + x) * C + c) * ok)
        _emit(bufs, t, "rows", it, torch.where(ok, v, torch.zeros(())))
        return
    Hd, Wd = (2 * H, 2 * W) if op == "up" else (H, W)
    it = torch.arange(B * Hd * Wd * C)
    c, r = it % C, it // C
    X, r = r % Wd, r // Wd
    Y, b = r % Hd, r // Hd
    if op == "up":
        _emit(bufs, t, "y", it, _fetch(t, "x", ((b * H + Y // 2) * W + X // 2) * C + c))
    elif op == "upb":
        base = ((b * 2 * H + 2 * Y) * (2 * W) + 2 * X) * C + c
        down = (W if defect == "up_bwd_row_stride_W" else 2 * W) * C
        f = lambda k: _fetch(t, "dy", base + k)      # noqa: E731
        _emit(bufs, t, "dx", it, ((f(0) + f(C)) + f(down)) + f(down + C))
    else:      # d2b: ky ascending, then kx ascending
        Ho, Wo = H // 2, W // 2
        last = 2 if defect == "down2_bwd_third_tap_dropped" else 3
        acc = torch.zeros(it.shape)
        for ky in range(last):
            for kx in range(last):
                ok = (ky % 2 == Y % 2) & (kx % 2 == X % 2)
                if defect != "down2_bwd_negative_index_unguarded":
                    ok &= (Y >= ky) & (X >= kx)
                i, j = torch.div(Y - ky, 2, rounding_mode="trunc"), torch.div(X - kx, 2, rounding_mode="trunc")
                v = _fetch(t, "drows", ((((b * Ho + i) * Wo + j) * 9 + ky * 3 + kx) * C + c) * ok)
                acc = acc + torch.where(ok, v, torch.zeros(()))
        _emit(bufs, t, "dx", it, acc)


def _model_sm(w, t, bufs, defect):
    rows, N, lds, ldp = w["rows"], w["N"], w["lds"], w["ldp"]
    scale = torch.tensor(w["scale"], dtype=torch.float32)
    r, col = torch.arange(rows).view(rows, 1), torch.arange(N).view(1, N)
    regs = (col < SM_REGS).expand(rows, N)
    out = "P" if w["op"] == "sm" else "dS"
    if w["op"] == "sm":
        s = _fetch(t, "S", r * lds + col)
        z = s * scale
        NEG = torch.tensor(-3.0e38)
        zm = s if defect == "sm_scale_after_max" else z
        if defect == "sm_tail_left_out_of_max":
            zm = torch.where(regs, zm, NEG)
        m = zm.max(1, keepdim=True).values
        if defect == "sm_fill_zero_in_max" and N % 8:
            m = m.clamp(min=0.0)
        e = torch.exp(z - m)
        inv = 1.0 / torch.where(regs | (defect != "sm_tail_left_out_of_sum"), e, torch.zeros(())).sum(1, keepdim=True)
        val = e * inv
    else:
        p, g = _fetch(t, "P", r * ldp + col), _fetch(t, "dP", r * lds + col)
        dot = torch.where(regs | (defect != "smb_dot_without_tail"), p * g, torch.zeros(())).sum(1, keepdim=True)
        val = scale * p * (g - dot)
    _emit(bufs, t, out, r * ldp + col, val)
    if defect != "sm_pad_columns_unwritten" and ldp > N:
        _emit(bufs, t, out, r * ldp + torch.arange(N, ldp).view(1, -1), torch.zeros(()))


def model(w, t, defect=None, store=True):
    """The kernels' arithmetic in float32 torch on CPU tensors, every operand fetched from and every result stored into the flat banded
    buffers by the kernels' index arithmetic; stores rounded to the output dtype (`store=False`: kept in float32).  `defect`: one of
    DEFECTS.  Returns {output: the flat buffer after the launch} for `results` / `bands_ok` (the workspace is not modelled)."""
    assert defect is None or w["op"] in DEFECTS[defect], (defect, w["name"])
    bufs = {n: t[n + "_buf"].clone() if store else t[n + "_buf"].to(torch.float32, copy=True) for n in outputs(w)}
    op = w["op"]
    (_model_gn if op == "gn" else _model_gnb if op == "gnb" else _model_haar if op in HAAR_OPS else _model_moves if op in MOVE_OPS else _model_sm)(w, t, bufs, defect)
    return bufs


# ------------------------------------------------------------------------------------------ launching (the GPU test file)
def launch(lib, w, t, stream, **over):
    "One call of the witness's entry point on the case's buffers; the status.  `over` replaces arguments by name."
    p = lambda n: over.get(n, t[n].data_ptr() if n in t else None)      # noqa: E731
    g = lambda k: over.get(k, w.get(k))      # noqa: E731
    code, op = over.get("dtype", CODE[w["dt"]]), w["op"]
    if op == "gn":
        a = (p("x"), p("y"), p("gamma"), p("beta"), p("mean"), p("rstd"), p("ws"), code, g("B"), g("H"), g("W"), g("C"), g("G"), EPS32)
        return lib.uc_group_norm_silu_nhwc(*a, stream) if g("act") == "silu" else lib.uc_group_norm_nhwc(*a, int(g("act") == "relu"), stream)
    if op == "gnb":
        shape = (code, g("B"), g("H"), g("W"), g("C"), g("G"), stream)
        if g("act") == "silu":
            return lib.uc_group_norm_silu_nhwc_bwd(p("dy"), p("x"), p("mean"), p("rstd"), p("gamma"), p("beta"), p("dx"), p("dgamma"), p("dbeta"), p("ws"), *shape)
        return lib.uc_group_norm_nhwc_bwd(p("dy"), p("x"), p("gate"), p("mean"), p("rstd"), p("gamma"), p("dx"), p("dgamma"), p("dbeta"), p("ws"), *shape)
    if op == "hp":
        return lib.uc_haar_patch(p("img"), p("rows"), code, g("B"), g("C"), g("H"), g("W"), g("ld"), g("scale"), stream)
    if op == "hu":
        return lib.uc_haar_unpatch(p("rows"), code, p("img"), g("B"), g("C"), g("H"), g("W"), g("ld"), g("scale"), stream)
    if op in MOVE_OPS:
        fn, a, b = {"d2": ("uc_down2_gather", "x", "rows"), "d2b": ("uc_down2_gather_bwd", "drows", "dx"), "up": ("uc_upsample2_nhwc", "x", "y"),
                    "upb": ("uc_upsample2_nhwc_bwd", "dy", "dx")}[op]
        return getattr(lib, fn)(p(a), p(b), code, g("B"), g("H"), g("W"), g("C"), stream)
    if op == "sm":
        return lib.uc_softmax_rows(p("S"), g("lds"), p("P"), code, g("ldp"), g("rows"), g("N"), g("scale"), stream)
    return lib.uc_softmax_rows_bwd(p("P"), p("dP"), g("lds"), p("dS"), code, g("ldp"), g("rows"), g("N"), g("scale"), stream)


def _bits(x):
    return x.contiguous().view(INTV["f" if x.dtype == torch.float32 else "b"])


def run_on_device(lib, w, family, device):
    """Launch the witness on one input family, twice, and measure everything: {status, bands, same: the two launches agree bit for bit,
    worst: {output: err / bound}, over: elements over the bound or NaN, first: the text of the first failure, case, got, ref}."""
    t = make_case(w, family, device, seed=seed_of(w))
    stream = torch.cuda.current_stream().cuda_stream
    status = launch(lib, w, t, stream)
    torch.cuda.synchronize()
    first = {o: t[o].clone() for o in outputs(w)}
    status2 = launch(lib, w, t, stream)
    torch.cuda.synchronize()
    got = results(w, t)
    rec = dict(name=w["name"], family=family, status=status or status2, bands=bands_ok(w, t), worst={}, over=0, first=None, case=t, got=got,
               same=all(torch.equal(_bits(first[o]), _bits(got[o])) for o in outputs(w)))
    ref = reference(w, t)
    rec["ref"] = ref
    label = f"{w['name']} ({family}): {route(w)}"
    for o in outputs(w):
        worst, bad, _ = ratio(got[o], *ref[o])
        rec["worst"][o] = worst
        rec["over"] += bad
        if w["op"] in BITS and not torch.equal(_bits(got[o]), _bits(ref[o][0].to(got[o].dtype))):
            rec["over"] += 1
            rec["first"] = rec["first"] or f"route [{label}] output {o}: a pure move does not return the input's bits"
        if bad and rec["first"] is None:
            try:
                check(label, o, *(v.reshape(-1, v.shape[-1]) for v in (got[o],) + tuple(ref[o])))
            except AssertionError as e:
                rec["first"] = str(e)
    return rec


if __name__ == "__main__":
    print(f"{len(WITNESSES)} witnesses ({len(SMALL)} small, {len(BIG)} large), {len({route(w) for w in WITNESSES.values()})} routes")
    for n, w in WITNESSES.items():
        print(f"  {n:40s} [{route(w)}]" + (f"  plan [{expected_plan(w)}]" if w["op"] in GN_OPS else "") + f"  families {', '.join(families(w))}")
