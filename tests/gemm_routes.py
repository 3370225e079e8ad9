"""Route audit of uc_gemm: signature of a launch, witness shapes, fp64 reference and the per-element bound.

A ROUTE is everything the device code can see that selects code, and no sizes (`signature`).  Every route found in
tests/golden/gemm_plan_bench.json gets a WITNESS: the smallest recorded row of that route, shrunk greedily while the plan driver
(tests/gemm_plan_driver.cpp over uniception_amd/csrc/gemm_plan.h) still returns the same signature, then given a ragged edge where the
route survives one.  The witnesses are stored in tests/golden/gemm_route_witnesses.json (descriptor rows only; regenerate with
`python -m tests.gemm_routes`); tests/test_gemm_routes.py re-derives them and checks each against the driver, and
tests/test_gemm_routes_gpu.py launches each on the device and compares every output element with `reference` under `bound`.

Reference: fp64 on the same rounded operands, the expression include/uc_hip.h states for the descriptor.  Bound per element:

    |got - ref| <= u_out * |ref| + 8 * sqrt(K_eff + n_epi) * 2^-24 * S + extra

u_out = 2^-8 / 2^-11 / 2^-24 (half an ulp of a bf16 / fp16 / fp32 store, relative; fp16 below 2^-14 is subnormal with spacing 2^-24,
so its store term is never below 2^-25); S = the same expression on absolute values; K_eff = reduction length (+ 128 for the fused
tail); n_epi = fp32 epilogue operations.  `extra` covers what is not an fp32 addition: 2e-5 * (|u| + |v|) for a RoPE pair (u, v) (the
bar of test_rope2d_against_the_references_compiled_cpu_loop) and 3e-6 * S for GELU and its derivative (the bar of test_gemm_f32 with
GELU).  The error of the kernels' erf approximation is ABSOLUTE (1.5e-7 on erf), so it scales with what erf multiplies: the GELU term
takes S of the pre-activation, the derivative's term S of the value the derivative multiplies (not of the product, which vanishes
where GELU' does).  RoPE positions of the witnesses lie in [0, 32), the bench's (512 / 16 patches per side): the hardware sine takes
its argument in turns after v_fract, whose absolute error grows with the number of turns.

Reference budget: no witness may need more than REF_BUDGET_FLOP of fp64 work (reference + S: 4 * M * N * K).  The GPU file computes
references with torch's fp64 matmul on the device in row chunks; all witnesses together are about 2.6 TFLOP
(measured on an MI355X: the 89 tests of the GPU file take 4 s; the CPU file takes 10 s).

Launch options that need size: nt_out != 0 needs an output above 128 MiB, so it is not part of the signature; its launches are
witnessed apart (the "nt" part of the fixture), one per (epi, out_dtype, compute_dtype, RoPE, tail) with the smallest K the route allows.  stagger > 0 does not occur
in the recorded rows (the bf16 stream keeps it off, and no fp32-family launch is long enough): left out.

Witnesses kept unragged, because no ragged variant keeps their route (the segmented eight-wave row kernel needs whole 512-pixel
tiles of row segments of one image, M % 512 == 0): every `conv_rows8 ...` signature (the flat form, `conv_rows8_flat`, is ragged);
and `t256x256 all side0 fuse0 vec1 relu_a0 slices0 cd1 od1 am1 stride1` (65 images of 16 x 16: one image per 256-row tile; every
smaller map or odd side moves the launch to another tile).
Outputs ops.gemm allocates itself (tail_out, stats_out) cannot carry a guard band; C, preact_out and vt_out do.

Tile order: a witness is shrunk to the fewest row tiles its route allows (MIN_ROWS: two to four), and nothing makes the shrinker keep a
full tile group next to a ragged last one (tiles_m % group_m != 0, group_m = 4) with more than one column tile — the `last` / dGmLast
branch of the workgroup -> tile map that each of the five direct-to-LDS kernels carries.  The hand-written "tile_order" part of the
fixture has one row per kernel with six row tiles and two or more column tiles (`load_tile_order`), checked like the others.
"""
import json
import math
import os
import shutil
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_JSON = os.path.join(ROOT, "tests", "golden", "gemm_plan_bench.json")
WITNESS_JSON = os.path.join(ROOT, "tests", "golden", "gemm_route_witnesses.json")
F32, BF16, F16 = 0, 1, 2
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
U_OUT = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}
REF_BUDGET_FLOP = 4.0e11
ROPE_BASE = 100.0
LN_EPS = 1e-6
PLAN_FIELDS = "kernel epi tiles_m tiles_n slices stagger nt_out side_lds fuse_split2 vec_ok relu_a".split()
PRESENCE = "bias residual residual2 rope_cols preact_out twin_out stats_out ln_stats tail_out tail_b sat_flag".split()
TILE = {"reg": (128, 128), "f32": (64, 64), "t128x128_s2": (128, 128), "t128x128_s3": (128, 128), "t256x128_s2": (256, 128),
        "t256x128_s3": (256, 128), "t256x256": (256, 256), "t256x128_bk32": (256, 128), "t128x64": (128, 64), "eight_wave": (256, 256),
        "four_wave": (256, 256), "conv_rows": (256, 128), "conv_rows8": (512, 128), "conv_rows8_flat": (512, 128)}


# ------------------------------------------------------------------------------------------ plan driver
def build_driver(tmpdir):
    "Compile tests/gemm_plan_driver.cpp with the system C++ compiler into tmpdir; returns run(rows) -> plan lines."
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/gemm_plan_driver.cpp"
    exe = os.path.join(str(tmpdir), "gemm_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "uniception_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_plan_driver.cpp"), "-o", exe])

    def run(rows):
        if not rows:
            return []
        lines = [" ".join(f"{k}={v}" for k, v in row.items()) for row in rows]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return run


def load_bench():
    with open(BENCH_JSON) as f:
        return json.load(f)


DERIVED_PARTS = ("routes", "nt")


def load_witnesses():
    "The derived parts of the fixture (what `derive_witnesses` returns)."
    with open(WITNESS_JSON) as f:
        w = json.load(f)
    return {part: w[part] for part in DERIVED_PARTS}


def load_tile_order():
    """The hand-written part of the fixture: {kernel: row}, one row per direct-to-LDS kernel with SIX row tiles — with the default
    group_m = 4 one full tile group and a ragged one of two, which the shrinker does not aim for — and two or more column tiles.  A row may carry the knobs that force its kernel (gemm_variant, conv_rows); the plan driver reads them."""
    with open(WITNESS_JSON) as f:
        return json.load(f)["tile_order"]


# ------------------------------------------------------------------------------------------ signature
def signature(row, plan_line):
    "Everything of a launch that selects device code, no sizes (and not nt_out / stagger: see the module docstring)."
    p = dict(zip(PLAN_FIELDS, plan_line.split()))
    s = [p["kernel"], p["epi"], "side" + p["side_lds"], "fuse" + p["fuse_split2"], "vec" + p["vec_ok"], "relu_a" + p["relu_a"],
         "slices" + str(int(int(p["slices"]) > 1)), "cd%d" % row["compute_dtype"], "od%d" % row.get("out_dtype", 0),
         "am%d" % row.get("a_mode", 0), "stride%d" % row.get("conv_stride", 0)]
    if row.get("residual"):
        s.append("res%d" % row.get("res_dtype", 0))
    if row.get("split_k", 0) > 1:
        s.append("split_k")
    if row.get("ln_nblk", 0) > 0:
        s.append("ln_nblk")
    if row.get("act", 0):
        s.append("act%d" % row["act"])
    if row.get("vt_col0", -1) >= 0:
        s.append("vt")
    if row.get("dact_u"):
        s.append("dact%d" % row.get("dact_act", 0))
    s += [f for f in PRESENCE if row.get(f)]
    return " ".join(s)


def nt_combo(row, plan_line):
    "(epi, out_dtype, compute_dtype, RoPE, tail) of a launch whose plan has nt_out != 0, else None."
    p = dict(zip(PLAN_FIELDS, plan_line.split()))
    if p["nt_out"] == "0":
        return None
    return "nt %s od%d cd%d rope%d tail%d" % (p["epi"], row.get("out_dtype", 0), row["compute_dtype"], int(row.get("rope_cols", 0) > 0),
                                              int(bool(row.get("tail_out"))))


def normalize(row):
    "Derived fields as the callers fill them in (conv geometry -> M, K; packed leading dimensions; ln_nblk, vt_npad)."
    r = dict(row)
    if r.get("a_mode", 0) == 1:
        s = r.get("conv_stride", 1) or 1
        r["M"] = r["conv_B"] * ((r["conv_H"] - 1) // s + 1) * ((r["conv_W"] - 1) // s + 1)
        r["K"] = 9 * r["conv_Cin"]
    else:
        r["lda"] = r["K"]
    n_out = r["vt_col0"] if r.get("vt_col0", -1) >= 0 else r["N"]
    r["ldc"] = n_out
    if r.get("residual"):
        r["ldr"] = r["N"]
    if r.get("ln_nblk", 0) > 0:
        r["ln_nblk"] = r["K"] // 64
    if r.get("vt_col0", -1) >= 0:
        r["vt_npad"] = (r["vt_ntok"] + 63) // 64 * 64
    return r


def ref_flop(row):
    return 4.0 * row["M"] * row["N"] * row["K"]


# ------------------------------------------------------------------------------------------ witnesses
def _shrink_steps(r):
    "Candidate smaller rows of r, most ambitious first."
    out = []
    conv = r.get("a_mode", 0) == 1
    vt = r.get("vt_col0", -1) >= 0
    for num, den in ((1, 2), (3, 4), (7, 8)):
        if conv:
            for f in ("conv_B", "conv_H"):
                if (r[f] * num) % den == 0 and r[f] * num // den >= 1:
                    out.append({f: r[f] * num // den})
        elif vt:
            b = r["M"] // r["vt_ntok"]
            if (b * num) % den == 0 and b * num // den >= 1:
                out.append({"M": r["vt_ntok"] * b * num // den})
        elif (r["M"] * num) % (den * 8) == 0:
            out.append({"M": r["M"] * num // den})
    if conv and r["conv_H"] == r["conv_W"] and r["conv_H"] % 2 == 0:
        out.append({"conv_H": r["conv_H"] // 2, "conv_W": r["conv_W"] // 2})
    if vt and r["vt_ntok"] % 128 == 0:
        out.append({"vt_ntok": r["vt_ntok"] // 2, "M": r["M"] // 2})
    if conv:
        if r["conv_Cin"] % 64 == 0:
            out.append({"conv_Cin": r["conv_Cin"] // 2})
    elif r["K"] % 64 == 0:
        out.append({"K": r["K"] // 2})
    if not vt and not r.get("rope_cols") and not r.get("tail_out") and r["N"] % 128 == 0 and r["N"] // 2 >= 256:
        out.append({"N": r["N"] // 2})
    return out


MIN_ROWS = 512      # no witness is shrunk below two to four row tiles: every wave position of a tile and a tile boundary stay covered


def _valid(r, min_rows=MIN_ROWS, min_side=8):
    if r.get("a_mode", 0) == 1 and (r["conv_H"] < min_side or r["conv_W"] < min_side or r["conv_B"] < 1):
        return False
    return r["M"] >= min_rows and r["K"] >= 64


def _key(row, plan_line, with_nt):
    return (signature(row, plan_line), nt_combo(row, plan_line) if with_nt else None)


def shrink(row, run, with_nt=False):
    "Greedy: apply the first step that keeps the signature (and, with_nt, nt_out) until none does."
    cur = normalize(row)
    want = _key(cur, run([cur])[0], with_nt)
    while True:
        cands = [c for c in (normalize({**cur, **step}) for step in _shrink_steps(cur)) if _valid(c)]
        lines = run(cands)
        nxt = next((c for c, l in zip(cands, lines) if _key(c, l, with_nt) == want), None)
        if nxt is None:
            return cur
        cur = nxt


def _ragged_steps(r, tile_m):
    conv = r.get("a_mode", 0) == 1
    if conv:     # an image border inside a tile / more than one image per tile, and a pixel count that is no multiple of the tile
        H, W, B = r["conv_H"], r["conv_W"], r["conv_B"]
        return [{"conv_H": H - 1, "conv_W": W - 3, "conv_B": B + 1}, {"conv_H": H - 1, "conv_W": W - 3, "conv_B": B + B // 4 + 1},
                {"conv_H": H - 1, "conv_W": W - 1}, {"conv_H": H - 1, "conv_B": B + 1},
                {"conv_H": H - 1}, {"conv_B": B + 1}]
    if r.get("vt_col0", -1) >= 0:
        n, b = r["vt_ntok"], r["M"] // r["vt_ntok"]
        return [{"vt_ntok": n - d, "M": b * (n - d)} for d in (63, 60, 56, 40, 8, 4, 1) if n - d > 0 and (b * (n - d)) % tile_m != 0]
    M = r["M"]      # (one more row tile, cut back: the ragged witness is never smaller than the shrunk one)
    return [{"M": M + tile_m - d} for d in (tile_m - 1, tile_m - 3, tile_m - 8, tile_m // 2 + 8, 72, 8, 1)]


def ragged(row, run):
    "The first ragged variant of a witness that keeps its signature, or the witness itself."
    line = run([row])[0]
    want = signature(row, line)
    tile_m = TILE[line.split()[0]][0]
    cands = [c for c in (normalize({**row, **step}) for step in _ragged_steps(row, tile_m)) if _valid(c, 256, 4)]
    for c, l in zip(cands, run(cands)):
        if signature(c, l) == want and ref_flop(c) <= max(ref_flop(row) * 1.6, 1e9):
            return c
    return row


def derive_witnesses(run):
    "{signature: witness row} over every recorded row, plus {nt combo: witness row} (section 4)."
    bench = load_bench()
    smallest, smallest_nt = {}, {}
    for cfg in sorted(bench):
        for row, _ in bench[cfg]:
            row = {k: v for k, v in row.items()}
            line = run([row])[0]
            sig, nt = signature(row, line), nt_combo(row, line)
            size = (row["M"] * row["N"] * row["K"], json.dumps(row, sort_keys=True))
            if sig not in smallest or size < smallest[sig][0]:
                smallest[sig] = (size, row)
            if nt and (nt not in smallest_nt or size < smallest_nt[nt][0]):
                smallest_nt[nt] = (size, row)
    routes = {sig: ragged(shrink(row, run), run) for sig, (_, row) in sorted(smallest.items())}
    nts = {nt: shrink(row, run, with_nt=True) for nt, (_, row) in sorted(smallest_nt.items())}
    return {"routes": routes, "nt": nts}


# ------------------------------------------------------------------------------------------ operands
def vt_perm(w):
    "uc_vt_perm of include/uc_hip.h, literally."
    return ((w >> 2) & 1) * 8 + (w & 3) + 4 * (w >> 3)


def vt_positions(ntok):
    n = torch.arange(ntok)
    return 16 * (n // 16) + vt_perm(n % 16)


def make_operands(row, device, seed=0, saturate=False):
    """Seeded operands of a witness, on `device`: A, W and whatever the descriptor carries.  Outputs are O(1); inputs hold negative
    values and exact zeros (ReLU, ReLU-on-load).  saturate: a few output elements are driven past the fp16 range."""
    g = torch.Generator(device=device).manual_seed(1000 + seed)
    cd = TORCH_DT[row["compute_dtype"]]
    M, N, K = row["M"], row["N"], row["K"]
    conv = row.get("a_mode", 0) == 1

    def randn(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=g, device=device) * scale + shift

    t = {}
    ln = bool(row.get("ln_stats"))
    if conv:
        a = randn(row["conv_B"], row["conv_H"], row["conv_W"], row["conv_Cin"])
    else:
        a = randn(M, K, shift=0.4 if ln else 0.0)
    a = a * (torch.rand(a.shape, generator=g, device=device) > 0.1)          # exact zeros
    t["A"] = a.to(cd)
    t["W"] = randn(N, K, scale=1.0 / math.sqrt(K)).to(cd)
    if row.get("bias"):
        t["bias"] = randn(N)
    for f in ("residual", "residual2"):
        if row.get(f):
            t[f] = randn(M, N).to(TORCH_DT[row["res_dtype"]])
    if row.get("dact_u"):
        t["dact_u"] = randn(M, N).bfloat16()
    if row.get("rope_cols"):
        t["rope_pos"] = torch.randint(0, 32, (M, 2), generator=g, device=device, dtype=torch.int64)
    if row.get("tail_out"):
        t["tail_w"] = randn(4, N, scale=1.0 / math.sqrt(N))
        if row.get("tail_b"):
            t["tail_b"] = randn(4)
    if ln:
        x = t["A"].double().view(M, K // 64, 64)
        if row.get("ln_nblk", 0) > 0:      # the producer's block partials [K/64][M] (sum, squared deviations from the block mean)
            s = x.sum(2)
            q = ((x - s[:, :, None] / 64) ** 2).sum(2)
            t["ln_stats"] = torch.stack([s.t(), q.t()], 2).float().contiguous()
        else:
            xf = x.view(M, K)
            t["ln_stats"] = torch.stack([xf.mean(1), 1 / torch.sqrt(xf.var(1, unbiased=False) + LN_EPS)], 1).float().contiguous()
        t["ln_colsum"] = t["W"].double().sum(1).float()
    if saturate:
        assert row["compute_dtype"] == F16
        if "bias" in t:
            t["bias"][3] = 1.0e6
        else:      # no bias on this route: one pixel / row of A lined up with one weight row, large enough for 30000 * sum |w| > 65504
            wrow = t["W"][5].double()
            if conv:
                cin = row["conv_Cin"]
                t["A"][0, 1, 1, :] = (30000.0 * torch.sign(wrow[4 * cin:5 * cin])).to(cd)      # centre tap
            else:
                t["A"][1, :] = (30000.0 * torch.sign(wrow)).to(cd)
    return t


# ------------------------------------------------------------------------------------------ reference / emulation
def a_rows(row, t, dt, b0=None, b1=None):
    "A_op as a [rows, K] matrix in dtype dt: dense rows b0:b1, or the literal im2col (ky, kx, c) of images b0:b1 (3x3, pad 1)."
    if row.get("a_mode", 0) == 0:
        a = t["A"][b0:b1].to(dt)
    else:
        x = t["A"][b0:b1].to(dt)
        s, H, W = row.get("conv_stride", 1) or 1, row["conv_H"], row["conv_W"]
        xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
        a = torch.cat([xp[:, ky:ky + H:s, kx:kx + W:s, :] for ky in range(3) for kx in range(3)], dim=3).reshape(-1, 9 * row["conv_Cin"])
    return torch.relu(a) if row.get("relu_a") else a


def ln_mean_rstd(row, t, dt):
    "(mean, rstd) per row from the statistics as given (finalized rows, or the block partials merged as uc_ln_stats_finalize does)."
    st = t["ln_stats"].to(dt)
    if row.get("ln_nblk", 0) <= 0:
        return st[:, 0], st[:, 1]
    s, q = st[:, :, 0], st[:, :, 1]      # [nblk][M]
    nblk = s.shape[0]
    mean = s.sum(0) / (64 * nblk)
    m2 = q.sum(0) + (64 * (s / 64 - mean[None]) ** 2).sum(0)
    return mean, 1 / torch.sqrt(m2 / (64 * nblk) + LN_EPS)


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))


def _dgelu(x):
    return 0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def evaluate(row, t, dt, r0, r1, want_s=True):
    """The descriptor's expression for output rows r0:r1 (conv: r0, r1 on image boundaries) in dtype dt, before the store.
    Returns {name: (value, S, extra)} for name in C / vt / preact / tail, and n_epi."""
    conv = row.get("a_mode", 0) == 1
    M, N = row["M"], row["N"]
    if conv:
        per = M // row["conv_B"]
        assert r0 % per == 0 and (r1 % per == 0 or r1 == M)
        A = a_rows(row, t, dt, r0 // per, (r1 + per - 1) // per)
    else:
        A = a_rows(row, t, dt, r0, r1)
    W = t["W"].to(dt)
    acc = A @ W.t()
    S = (A.abs() @ W.abs().t()) if want_s else torch.zeros_like(acc)
    del A
    n_epi = 0
    bias = t["bias"].to(dt) if "bias" in t else None
    if "ln_stats" in t:
        mean, rstd = ln_mean_rstd(row, t, dt)
        mean, rstd, cs = mean[r0:r1, None], rstd[r0:r1, None], t["ln_colsum"].to(dt)[None]
        pre = rstd * (acc - mean * cs) + bias
        S = rstd * (S + mean.abs() * cs.abs()) + bias.abs()
        n_epi += 3
    elif bias is not None:
        pre, S, n_epi = acc + bias, S + bias.abs(), n_epi + 1
    else:
        pre = acc
    out = {}
    extra = torch.zeros_like(S)
    if row.get("preact_out"):
        out["preact"] = (pre, S, extra)
    act = row.get("act", 0)
    if act == 1:
        v, extra, n_epi = _gelu(pre), extra + 3e-6 * S, n_epi + 1
    elif act == 2:
        v, n_epi = torch.relu(pre), n_epi + 1
    else:
        v = pre
    for f in ("residual", "residual2"):
        if f in t:
            r = t[f][r0:r1].to(dt)
            v, S, n_epi = v + r, S + r.abs(), n_epi + 1
    if "dact_u" in t:
        u = t["dact_u"][r0:r1].to(dt)
        if row["dact_act"] == 2:
            d = (u > 0).to(dt)
            extra = extra * d
        else:
            d = _dgelu(u)
            extra = extra * d.abs() + 3e-6 * S
        v, S, n_epi = v * d, S * d.abs(), n_epi + 1
    if row.get("tail_out"):
        tw = t["tail_w"].to(dt)
        tv, ts, te = v @ tw.t(), S @ tw.abs().t(), extra @ tw.abs().t()
        if "tail_b" in t:
            tv, ts, n_epi = tv + t["tail_b"].to(dt), ts + t["tail_b"].to(dt).abs(), n_epi + 1
        out["tail"] = (tv, ts, te)
        return out, n_epi
    rc = row.get("rope_cols", 0)
    if rc:
        # columns are (head, d), head_dim 64: quarters (u_y, v_y, u_x, v_x) of 16 channels, channel i of a quarter turns by
        # pos * base^(-i/16) (F0 = 1)
        rows = v.shape[0]
        inv = (1.0 / ROPE_BASE ** (torch.arange(16, device=v.device, dtype=dt) / 16))
        pos = t["rope_pos"][r0:r1].to(dt)
        ang = pos[:, None, :, None] * inv[None, None, None, :]               # [rows, 1, axis, 16]
        c, s = torch.cos(ang), torch.sin(ang)
        x = v[:, :rc].reshape(rows, rc // 64, 2, 2, 16)                      # [rows, head, axis, (u, v), 16]
        xs = S[:, :rc].reshape(rows, rc // 64, 2, 2, 16)
        xe = extra[:, :rc].reshape(rows, rc // 64, 2, 2, 16)
        u_, w_ = x[:, :, :, 0], x[:, :, :, 1]
        su, sw = xs[:, :, :, 0], xs[:, :, :, 1]
        eu, ew = xe[:, :, :, 0], xe[:, :, :, 1]
        pair = 2e-5 * (u_.abs() + w_.abs())
        rot = torch.stack([u_ * c - w_ * s, w_ * c + u_ * s], 3).reshape(rows, rc)
        rs = torch.stack([su * c.abs() + sw * s.abs(), sw * c.abs() + su * s.abs()], 3).reshape(rows, rc)
        re = torch.stack([eu * c.abs() + ew * s.abs() + pair, ew * c.abs() + eu * s.abs() + pair], 3).reshape(rows, rc)
        v, S, extra = torch.cat([rot, v[:, rc:]], 1), torch.cat([rs, S[:, rc:]], 1), torch.cat([re, extra[:, rc:]], 1)
        n_epi += 2
    v0 = row.get("vt_col0", -1)
    if v0 >= 0:
        out["vt"] = (v[:, v0:], S[:, v0:], extra[:, v0:])
        v, S, extra = v[:, :v0], S[:, :v0], extra[:, :v0]
    out["C"] = (v, S, extra)
    return out, n_epi


def out_code(row, name):
    return F32 if name == "tail" else (BF16 if name == "vt" else row.get("out_dtype", 0))


def saturate_f16(x):
    return x.clamp(-65504.0, 65504.0)


def bound(ref, S, extra, code, k_eff, n_epi):
    store = U_OUT[code] * ref.abs()
    if code == F16:
        store = store.clamp_min(2.0 ** -25)
    return store + 8.0 * math.sqrt(k_eff + n_epi) * 2.0 ** -24 * S + extra


def k_eff(row):
    return row["K"] + (128 if row.get("tail_out") else 0)


def reference(row, t, chunk_rows=32768):
    "fp64 reference of every output of the descriptor: {name: (ref, bound)} as fp64 tensors on the operands' device."
    M = row["M"]
    step = M
    if M > chunk_rows:
        per = M // row["conv_B"] if row.get("a_mode", 0) == 1 else 1
        step = max(per, chunk_rows // per * per)
    parts = {}
    for r0 in range(0, M, step):
        outs, n_epi = evaluate(row, t, torch.float64, r0, min(M, r0 + step))
        for name, (v, S, extra) in outs.items():
            code = out_code(row, name)
            if code == F16:
                v = saturate_f16(v)
            parts.setdefault(name, []).append((v, bound(v, S, extra, code, k_eff(row), n_epi)))
    return {name: (torch.cat([p[0] for p in ps]), torch.cat([p[1] for p in ps])) for name, ps in parts.items()}


def emulate(row, t):
    """The kernels' arithmetic as the bound models it: fp32 matmul of the rounded operands, fp32 epilogue, ONE rounding to the
    output type (fp16 saturating).  {name: stored tensor}."""
    outs, _ = evaluate(row, t, torch.float32, 0, row["M"], want_s=False)
    got = {}
    for name, (v, _, _) in outs.items():
        code = out_code(row, name)
        got[name] = (saturate_f16(v) if code == F16 else v).to(TORCH_DT[code])
    return got


def stats_reference(stored, dt=torch.float64):
    """stats_out of the STORED rows [M, N]: per 64-column block (sum, squared deviations from the block mean), block-major [N/64][M][2],
    with its bound: the same form, S built from the stored rows (64 additions; the deviations carry the error of the mean)."""
    M, N = stored.shape
    x = stored.to(dt).view(M, N // 64, 64)
    s = x.sum(2)
    mu = s / 64
    q = ((x - mu[:, :, None]) ** 2).sum(2)
    ref = torch.stack([s.t(), q.t()], 2)
    S = torch.stack([x.abs().sum(2).t(), ((x.abs() + mu.abs()[:, :, None]) ** 2).sum(2).t()], 2)
    return ref, bound(ref, S, torch.zeros_like(S), F32, 64, 3)


def emulate_stats(stored):
    return stats_reference(stored, torch.float32)[0]


def unpack_vt(vt_out, row):
    "vt_out [B, H, 64, npad] -> the V columns [M, N - vt_col0] it holds, by the literal index formula of include/uc_hip.h."
    ntok, heads = row["vt_ntok"], (row["N"] - row["vt_col0"]) // 64
    B = row["M"] // ntok
    pos = vt_positions(ntok).to(vt_out.device)
    return vt_out.view(B, heads, 64, row["vt_npad"])[:, :, :, pos].permute(0, 3, 1, 2).reshape(row["M"], heads * 64)


def pack_vt(v, row, fill=float("nan")):
    "The inverse, for the emulation: V columns [M, heads * 64] -> [B, H, 64, npad] with `fill` where no key lives."
    ntok, heads = row["vt_ntok"], (row["N"] - row["vt_col0"]) // 64
    B = row["M"] // ntok
    out = torch.full((B, heads, 64, row["vt_npad"]), fill, dtype=v.dtype, device=v.device)
    out[:, :, :, vt_positions(ntok).to(v.device)] = v.view(B, ntok, heads, 64).permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------ checker
def violations(got, ref, bnd):
    "Boolean mask of the elements over the bound (NaN — an element never written — counts)."
    return ~((got.to(ref.dtype) - ref).abs() <= bnd)


def check(route, name, got, ref, bnd, tile=(128, 128)):
    "Zero elements over the bound, or an AssertionError naming the route, the count and the first few elements with their tiles."
    bad = violations(got, ref, bnd)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero()[:6].tolist()
    lines = []
    for ix in idx:
        r, c = ix[0], ix[1] if len(ix) > 1 else 0
        e = tuple(ix)
        lines.append(f"  (row {r}, col {c}{'' if len(ix) < 3 else ', ' + str(ix[2])}) got {float(got[e]):.9g} ref {float(ref[e]):.9g} "
                     f"bound {float(bnd[e]):.3g} tile ({r // tile[0]}, {c // tile[1]})")
    raise AssertionError(f"route [{route}] output {name}: {n} of {bad.numel()} elements over the bound\n" + "\n".join(lines))


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        w = derive_witnesses(build_driver(tmp))
    w["tile_order"] = load_tile_order()      # hand-written: kept as it is
    with open(WITNESS_JSON, "w") as f:
        json.dump(w, f, indent=0, sort_keys=True)
        f.write("\n")
    tot = sum(ref_flop(r) for part in w.values() for r in part.values())
    print(f"{len(w['routes'])} routes, {len(w['nt'])} nt witnesses, {tot / 1e12:.2f} TFLOP of fp64 reference work")
    for part in ("routes", "nt"):
        for sig, r in w[part].items():
            print(f"{ref_flop(r) / 1e9:9.1f} GFLOP  M {r['M']:8d} N {r['N']:5d} K {r['K']:5d}  {sig}")
