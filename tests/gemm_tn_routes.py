"""Route audit of uc_gemm_tn (dW = dY^T X, uniception_amd/csrc/gemm_tn.hip): routes, witness shapes, operands inside NaN, the fp64
reference, the per-element bound and a CPU emulation that can be given the faults these kernels can have.

ROUTES.  The launches recorded in tests/golden/gemm_tn_plan_bench.json come from a kernel trace and carry neither the colsum form nor
leading dimensions, so the routes are NOT derived from them (as tests/gemm_routes.py does for uc_gemm) but enumerated by hand from
what the device code can see that selects code:
  kernel   256_dense | 128_dense | 256_conv | 128_conv | conv_rows   the template instance uc_gemm_tn's switch launches from
           uc_gemm_tn_plan (gemm_tn_kernel<BM_, CONV>: the `if constexpr (!CONV)` source address and the tap / pixel decode in
           issue_stage, NI_A / PER / RA; conv_dw_rows_kernel is code of its own)
  relu_b   0 | 1, conv kernels only (tn_check_shape rejects it on dense): `CONV && p.relu_b != 0` in the B-fragment TN_FRAG of
           gemm_tn_kernel, `if (relu)` on the fragments of conv_dw_rows_kernel
  colsum   none | slabs | atomic: `do_colsum = p.colsum != nullptr && tj == 0 && wc == 0` (rows: `ky == 1 && tc == 0 && wc == 0`) guards
           the v_dot2 chain and the fold, `if (p.colsum_atomic) unsafeAtomicAdd(...) else p.colsum[ksplit * I + ii] = v` picks the store
6 dense + 12 im2col + 6 row-kernel routes = 24 (`ROUTES`); every one has a witness, nothing is left unwitnessed.

FEATURES are no code selectors, but where the kernels go wrong; they are spread over the witnesses so that every kernel that can carry
one sees it at least once (`FEATURES` names the kernels, `features(w)` derives them from the witness, tests/test_gemm_tn_routes.py
checks the table below against both):
  sk=1       split_k == 1                                    short      split_k > 1, the last non-empty slice shorter than the others
  empty      a K-slice without any 64-row block / segment    ring       >= 3 blocks in a slice (two-stage ring reused); rows: >= 4 segments
  s1 / s2    conv stride 1 / 2 (im2col kernels)              lda / ldb  leading dimension above I / J (ldb: dense only)
  off        operand starts inside a wider buffer            tiles_j    colsum asked for with several column tiles (tj / tc ownership)

  witness           T    I     J  sk  B  H   W Cin stride   lda a_off  ldb b_off  features
  d256_none        197  392   264   1                      408    8   264   0  sk=1 ring lda off
  d256_slabs       301  264   520   2                      264    0   528   8  short ring ldb off tiles_j
  d256_atomic      333  264   264   4                      272    0   264   0  empty lda tiles_j
  d128_none        197    8     8   1                       24    8    16   8  sk=1 ring lda ldb off
  d128_slabs       301   72   264   2                       72    0   264   0  short ring tiles_j
  d128_atomic      197  128   520   5                      384  128   520   0  empty lda off tiles_j
  c256_r0_none      70  136    72   1   2  5   7   8 1     136    0            sk=1 s1
  c256_r0_slabs    286  136   360   2   2 13  11  40 1     144    8            short ring s1 lda off tiles_j
  c256_r0_atomic    60  136   216   2   2  9  11  24 2     136    0            empty s2
  c256_r1_none      22  136   216   1   2  1  11  24 1     152    0            sk=1 s1 lda
  c256_r1_slabs    144  136   360   2   2 18  16  40 2     136    0            short s2 tiles_j
  c256_r1_atomic    14  136    72   3   2  7   1   8 1     136    0            empty s1
  c128_r0_none      24   24   216   1   2  5   7  24 2      24    0            sk=1 s2
  c128_r0_slabs    198   24   360   3   2  9  11  40 1      24    0            empty s1 tiles_j
  c128_r0_atomic   162   24    72   2   2  9   9   8 1      40    8            short s1 lda off
  c128_r1_none      22   24    72   1   2  1  11   8 1      24    0            sk=1 s1
  c128_r1_slabs    288   24   216   2   2 16  36  24 2      32    0            short ring s2 lda
  c128_r1_atomic    14   24   360   3   2  7   1  40 1      24    0            empty s1 tiles_j
  rows_r0_none     768  128  1152   1   2  3 128 128 1     128    0            sk=1 ring
  rows_r0_slabs    640  256  2304   3   2  5  64 256 1     256    0            short ring tiles_j
  rows_r0_atomic   128  256  1152   3   2  1  64 128 1     384  128            empty lda off
  rows_r1_none     256  128  2304   1   2  1 128 256 1     136    0            sk=1 ring lda
  rows_r1_slabs    384  256  1152   4   2  3  64 128 1     256    0            empty
  rows_r1_atomic   768  128  2304   5   2  3 128 256 1     128    0            empty tiles_j
The im2col witnesses have two images (a wrong border test can reach the other one), odd 5 x 7, 9 x 11, 13 x 11 and 9 x 9 maps, a one-row
(1 x 11) and a one-column (7 x 1) image, stride 2 on odd (5 x 7, 9 x 11) and even (18 x 16, 16 x 36) sizes, Cin 8 / 24 (a 256-column tile
spans several taps) and 40 (J = 360: a second column tile, whose border falls inside a tap).  Dense: I = 264 leaves 8 valid columns in the
last row tile, J = 264 / 520 a ragged second / third column tile, J = 8 clamps every B chunk, T = 197 / 301 / 333 is no multiple of 64 nor 8;
"short" needs a block count no slice count divides evenly, hence T = 301 (5 blocks: 3 + 2) next to 197 (4) and 333 (6).
conv_rows can NOT be ragged: W % 64 == 0, Cin % 128 == 0 and Cout % 128 == 0 are its routing conditions (uc_tn_conv_rows_ok).  Its
witnesses have W = 128 (an interior segment border: pixel ox0 - 1 is a real pixel of the neighbouring segment) and 64, H 1 and 3, two
images, Cin / Cout 128 and 256 (tiles_c = 2: only tc == 0 owns the colsum), 12 and 4 segments in one slice (the three-stage ring wraps),
split_k 5 on 12 and 4 on 6 segments (does not divide: an empty slice), 3 on 2 (above the count); the segment counts of H in {1, 3}
(2, 4, 6, 12) leave no slice count with a short last slice, so rows_r0_slabs has H = 5: 10 segments in slices of 4 + 4 + 2.
Every witness is checked against tests/gemm_tn_plan_driver.cpp (kernel, tiles, block, lds_bytes, grid) on the CPU, and the descriptor
the wrapper really passed goes to the same driver on the GPU, so a change of routing breaks a witness instead of testing another kernel.
No witness needs more than REF_BUDGET_FLOP of fp64 work (4 * T * I * J: reference and S).

OPERANDS (`make_operands`): seeded bf16, O(1), normal numbers only (magnitudes >= 2^-6).  Under relu_b the image holds negative values,
exact +0.0 and exact -0.0 (relu_bf16x4 is an int16 max: -0.0 = 0x8000 must come out as zero).  Every operand lives inside NaN: A is a view
[:T, a_off : a_off + I] of a NaN-filled [T + 8, lda] buffer, dense B likewise, the conv image is images 1 .. B of a NaN-filled
[B + 2, H, W, Cin] buffer.  A kernel that multiplies anything it should have replaced by zero, and stores it, produces a NaN.

REFERENCE: fp64 on the same bf16 operands, the expression include/uc_hip.h states for uc_gemm_tn_desc (literal im2col through a zero-padded
copy): every slab by itself (slice s covers the 64-row blocks [s * nk_per, (s + 1) * nk_per), nk_per = ceil(ceil(T / 64) / split_k); for
the row kernel the segments [s * per, (s + 1) * per), which is the same thing because T = 64 * segments), their sum dW, and the colsum.
BOUND: bf16 products are exact in fp32, so the only roundings are the fp32 accumulation and the slab sum; tests/gemm_routes.py's model,
no new constant:
    |got - ref| <= 2^-24 * |ref| + 8 * sqrt(K_eff + n_epi) * 2^-24 * S
K_eff = the slice's rows for a slab, T for the sum; n_epi = 0 for a slab, split_k for the sum; S = the same expression on absolute
values (colsum: S = sum_t |A[t,i]|).  An empty slice has K_eff = 0, S = 0: its slab and colsum must be exactly zero.  The atomic colsum
is compared as target - prefill with n_epi = split_k and 2^-24 * |prefill| added.

EMULATION (`emulate`): plain fp32 — 32-row steps in t order, slabs added in slice order — that fetches every operand element from
the flat NaN-filled buffer by the kernels' own address arithmetic, so a fault of the addressing (`FAULTS`) reads what the device would read.

Measured on an MI355X: the 31 tests of tests/test_gemm_tn_routes_gpu.py take 3.2 s (the slowest, the first to touch the device, 0.8 s; every other under
0.15 s); the 80 tests of the CPU file take 5 s.  Largest err / bound per witness (the colsum's partial sums of bf16 values are exact in
fp32 at these sizes, so its slabs show 0; the atomic form rounds against the prefilled value):
  witness             dW  slabs  colsum
  d256_none       0.0143 0.0143  -
  d256_slabs      0.0072 0.0159  0.0000
  d256_atomic     0.0050 0.0237  0.0012
  d128_none       0.0036 0.0036  -
  d128_slabs      0.0057 0.0150  0.0000
  d128_atomic     0.0069 0.0538  0.0015
  c256_r0_none    0.0198 0.0200  -
  c256_r0_slabs   0.0073 0.0163  0.0000
  c256_r0_atomic  0.0215 0.0219  0.0029
  c256_r1_none    0.0247 0.0252  -
  c256_r1_slabs   0.0212 0.0326  0.0000
  c256_r1_atomic  0.0245 0.0269  0.0220
  c128_r0_none    0.0225 0.0230  -
  c128_r0_slabs   0.0069 0.0255  0.0000
  c128_r0_atomic  0.0069 0.0166  0.0009
  c128_r1_none    0.0202 0.0207  -
  c128_r1_slabs   0.0060 0.0152  0.0000
  c128_r1_atomic  0.0218 0.0239  0.0117
  rows_r0_none    0.0068 0.0068  -
  rows_r0_slabs   0.0045 0.0205  0.0000
  rows_r0_atomic  0.0097 0.0209  0.0042
  rows_r1_none    0.0119 0.0119  -
  rows_r1_slabs   0.0065 0.0193  0.0000
  rows_r1_atomic  0.0041 0.0180  0.0003
"""
import os
import shutil
import subprocess

import torch

from tests.gemm_routes import F32, ROOT, bound, check, violations  # noqa: F401  (check / violations: re-exported for the test files)

KERNELS = ("256_dense", "128_dense", "256_conv", "128_conv", "conv_rows")
IM2COL = ("256_conv", "128_conv")
COLSUMS = ("none", "slabs", "atomic")
ROUTES = [f"{k} {c}" for k in KERNELS[:2] for c in COLSUMS] + [f"{k} relu{r} {c}" for k in KERNELS[2:] for r in (0, 1) for c in COLSUMS]
GUARD_ROWS = 8
REF_BUDGET_FLOP = 4.0e9
TILE = {"256_dense": (256, 256), "256_conv": (256, 256), "128_dense": (128, 256), "128_conv": (128, 256), "conv_rows": (128, 128)}
# feature -> the kernels that can carry it
FEATURES = {"sk=1": KERNELS, "short": KERNELS, "empty": KERNELS, "ring": KERNELS, "s1": IM2COL, "s2": IM2COL,
            "lda": KERNELS, "ldb": KERNELS[:2], "off": KERNELS, "tiles_j": KERNELS}


def _dense(kernel, colsum, T, I, J, sk, lda=0, a_off=0, ldb=0, b_off=0):
    return dict(kernel=kernel, relu_b=0, colsum=colsum, T=T, I=I, J=J, split_k=sk, lda=lda or I, a_off=a_off, ldb=ldb or J, b_off=b_off, conv=None)


def _conv(kernel, relu, colsum, B, H, W, Cin, Cout, stride, sk, lda=0, a_off=0):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return dict(kernel=kernel, relu_b=relu, colsum=colsum, T=B * Ho * Wo, I=Cout, J=9 * Cin, split_k=sk, lda=lda or Cout, a_off=a_off, ldb=0, b_off=0,
                conv=(B, H, W, Cin, stride))


WITNESSES = {
    "d256_none": _dense("256_dense", "none", 197, 392, 264, 1, lda=408, a_off=8),
    "d256_slabs": _dense("256_dense", "slabs", 301, 264, 520, 2, ldb=528, b_off=8),
    "d256_atomic": _dense("256_dense", "atomic", 333, 264, 264, 4, lda=272),
    "d128_none": _dense("128_dense", "none", 197, 8, 8, 1, lda=24, a_off=8, ldb=16, b_off=8),
    "d128_slabs": _dense("128_dense", "slabs", 301, 72, 264, 2),
    "d128_atomic": _dense("128_dense", "atomic", 197, 128, 520, 5, lda=384, a_off=128),
    "c256_r0_none": _conv("256_conv", 0, "none", 2, 5, 7, 8, 136, 1, 1),
    "c256_r0_slabs": _conv("256_conv", 0, "slabs", 2, 13, 11, 40, 136, 1, 2, lda=144, a_off=8),
    "c256_r0_atomic": _conv("256_conv", 0, "atomic", 2, 9, 11, 24, 136, 2, 2),
    "c256_r1_none": _conv("256_conv", 1, "none", 2, 1, 11, 24, 136, 1, 1, lda=152),
    "c256_r1_slabs": _conv("256_conv", 1, "slabs", 2, 18, 16, 40, 136, 2, 2),
    "c256_r1_atomic": _conv("256_conv", 1, "atomic", 2, 7, 1, 8, 136, 1, 3),
    "c128_r0_none": _conv("128_conv", 0, "none", 2, 5, 7, 24, 24, 2, 1),
    "c128_r0_slabs": _conv("128_conv", 0, "slabs", 2, 9, 11, 40, 24, 1, 3),
    "c128_r0_atomic": _conv("128_conv", 0, "atomic", 2, 9, 9, 8, 24, 1, 2, lda=40, a_off=8),
    "c128_r1_none": _conv("128_conv", 1, "none", 2, 1, 11, 8, 24, 1, 1),
    "c128_r1_slabs": _conv("128_conv", 1, "slabs", 2, 16, 36, 24, 24, 2, 2, lda=32),
    "c128_r1_atomic": _conv("128_conv", 1, "atomic", 2, 7, 1, 40, 24, 1, 3),
    "rows_r0_none": _conv("conv_rows", 0, "none", 2, 3, 128, 128, 128, 1, 1),
    "rows_r0_slabs": _conv("conv_rows", 0, "slabs", 2, 5, 64, 256, 256, 1, 3),
    "rows_r0_atomic": _conv("conv_rows", 0, "atomic", 2, 1, 64, 128, 256, 1, 3, lda=384, a_off=128),
    "rows_r1_none": _conv("conv_rows", 1, "none", 2, 1, 128, 256, 128, 1, 1, lda=136),
    "rows_r1_slabs": _conv("conv_rows", 1, "slabs", 2, 3, 64, 128, 256, 1, 4),
    "rows_r1_atomic": _conv("conv_rows", 1, "atomic", 2, 3, 128, 256, 128, 1, 5),
}
NAMES = list(WITNESSES)


def route(w):
    return f"{w['kernel']} {w['colsum']}" if w["conv"] is None else f"{w['kernel']} relu{w['relu_b']} {w['colsum']}"


def slices(w):
    "[(t0, t1)] rows of every K-slice: 64-row blocks [s * nk_per, (s + 1) * nk_per) of ceil(T / 64), cut at T."
    nblk = (w["T"] + 63) // 64
    per = (nblk + w["split_k"] - 1) // w["split_k"]
    return [(min(s * per * 64, w["T"]), min((s + 1) * per * 64, w["T"])) for s in range(w["split_k"])]


def tiles_ij(w):
    if w["kernel"] == "conv_rows":
        return w["I"] // 128, w["conv"][3] // 128
    bm = TILE[w["kernel"]][0]
    return (w["I"] + bm - 1) // bm, (w["J"] + 255) // 256


def features(w):
    f = set()
    blocks = [(t1 - t0 + 63) // 64 for t0, t1 in slices(w)]
    live = [b for b in blocks if b]
    if w["split_k"] == 1:
        f.add("sk=1")
    elif live[-1] < live[0]:
        f.add("short")
    if 0 in blocks:
        f.add("empty")
    if max(blocks) >= (4 if w["kernel"] == "conv_rows" else 3):
        f.add("ring")
    if w["kernel"] in IM2COL:
        f.add("s%d" % w["conv"][4])
    if w["lda"] > w["I"]:
        f.add("lda")
    if w["conv"] is None and w["ldb"] > w["J"]:
        f.add("ldb")
    if w["a_off"] or w["b_off"]:
        f.add("off")
    if w["colsum"] != "none" and tiles_ij(w)[1] > 1:
        f.add("tiles_j")
    return f


def ref_flop(w):
    return 4.0 * w["T"] * w["I"] * w["J"]


# ------------------------------------------------------------------------------------------ plan driver
def build_driver(tmpdir):
    "Compile tests/gemm_tn_plan_driver.cpp with the system C++ compiler into tmpdir; returns run(rows) -> plan lines."
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/gemm_tn_plan_driver.cpp"
    exe = os.path.join(str(tmpdir), "gemm_tn_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "uniception_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_tn_plan_driver.cpp"), "-o", exe])

    def run(rows):
        lines = [" ".join(f"{k}={v}" for k, v in row.items()) for row in rows]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return run


def driver_row(w):
    "The uc_gemm_tn_desc ops.gemm_tn builds for the witness (pointers as placeholders)."
    row = dict(A=4096, B=4096, C=4096, T=w["T"], I=w["I"], J=w["J"], lda=w["lda"], ldb=w["ldb"], relu_b=w["relu_b"], split_k=w["split_k"],
               colsum_a=0 if w["colsum"] == "none" else 4096, colsum_atomic=int(w["colsum"] == "atomic"))
    if w["conv"]:
        row.update(zip(("conv_B", "conv_H", "conv_W", "conv_Cin", "conv_stride"), w["conv"]))
    return row


def expected_plan(w):
    "`kernel tiles_i tiles_j tiles block lds_bytes grid` by the rules tests/test_gemm_tn_plan.py states, worked here without the header."
    ti, tj = tiles_ij(w)
    if w["kernel"] == "conv_rows":
        tiles, block, lds = 3 * ti * tj, 512, 3 * (64 * 256 + 68 * 256)
    else:
        bm = TILE[w["kernel"]][0]
        tiles, block, lds = ti * tj, 4 * bm, 2 * (64 * bm * 2 + 64 * 256 * 2)
    return f"{w['kernel']} {ti} {tj} {tiles} {block} {lds} {tiles * w['split_k']}"


# ------------------------------------------------------------------------------------------ operands
def make_operands(w, device, seed=0):
    "Seeded operands of a witness on `device`: views A, B (dense [T, J] / image [B, H, W, Cin]) of the NaN-filled A_buf, B_buf."
    g = torch.Generator(device=device).manual_seed(2000 + seed)

    def vals(*shape):
        x = torch.randn(*shape, generator=g, device=device)
        return (x + torch.copysign(torch.full_like(x, 2.0 ** -6), x)).bfloat16()      # normal numbers only, no exact zeros

    def nan(*shape):
        return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=device)

    T, I, J = w["T"], w["I"], w["J"]
    assert w["a_off"] % 8 == 0 and w["a_off"] + I <= w["lda"]
    t = {"A_buf": nan(T + GUARD_ROWS, w["lda"])}
    t["A"] = t["A_buf"][:T, w["a_off"]:w["a_off"] + I]
    t["A"].copy_(vals(T, I))
    if w["conv"] is None:
        assert w["b_off"] % 8 == 0 and w["b_off"] + J <= w["ldb"]
        t["B_buf"] = nan(T + GUARD_ROWS, w["ldb"])
        t["B"] = t["B_buf"][:T, w["b_off"]:w["b_off"] + J]
        t["B"].copy_(vals(T, J))
    else:
        B, H, W, Cin, _ = w["conv"]
        x = vals(B, H, W, Cin)
        if w["relu_b"]:
            u = torch.rand(x.shape, generator=g, device=device)
            x[u < 0.06] = 0.0
            x[(u >= 0.06) & (u < 0.12)] = -0.0
        t["B_buf"] = nan(B + 2, H, W, Cin)
        t["B"] = t["B_buf"][1:B + 1]
        t["B"].copy_(x)
    return t


def prefill(w, device, seed=0):
    "The non-zero values the atomic colsum's target holds before the launch."
    g = torch.Generator(device=device).manual_seed(3000 + seed)
    return 1.0 + torch.rand(w["I"], generator=g, device=device)


# ------------------------------------------------------------------------------------------ reference
def b_matrix(w, t, dt):
    "B_op [T, J] in dtype dt: dense B, or the literal im2col (ky, kx, c) of the 3x3 / pad 1 conv through a zero-padded copy; ReLU on load."
    if w["conv"] is None:
        return t["B"].to(dt)
    B, H, W, Cin, s = w["conv"]
    x = t["B"].to(dt)
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    b = torch.cat([xp[:, ky:ky + H:s, kx:kx + W:s, :] for ky in range(3) for kx in range(3)], dim=3).reshape(-1, 9 * Cin)
    return torch.relu(b) if w["relu_b"] else b


def reference(w, t, pre=None):
    """fp64 reference of every output, {name: (ref, bound)}: "slabs" [split_k, I, J], "dW" [I, J], "colsum_slabs" [split_k, I], "colsum" [I]
    (the sum of the slabs, or with `pre` what the atomic form adds to a target holding `pre`)."""
    a, b = t["A"].double(), b_matrix(w, t, torch.float64)
    aa, ba = a.abs(), b.abs()
    sl = slices(w)
    slab = [a[t0:t1].t() @ b[t0:t1] for t0, t1 in sl]
    slab_s = [aa[t0:t1].t() @ ba[t0:t1] for t0, t1 in sl]
    cs = [a[t0:t1].sum(0) for t0, t1 in sl]
    cs_s = [aa[t0:t1].sum(0) for t0, t1 in sl]
    T, sk = w["T"], w["split_k"]
    out = {"slabs": (torch.stack(slab), torch.stack([bound(r, s, 0.0, F32, t1 - t0, 0) for r, s, (t0, t1) in zip(slab, slab_s, sl)])),
           "colsum_slabs": (torch.stack(cs), torch.stack([bound(r, s, 0.0, F32, t1 - t0, 0) for r, s, (t0, t1) in zip(cs, cs_s, sl)]))}
    dw, cst = sum(slab), sum(cs)
    out["dW"] = (dw, bound(dw, sum(slab_s), 0.0, F32, T, sk))
    extra = 0.0 if pre is None else 2.0 ** -24 * pre.double().abs()
    out["colsum"] = (cst, bound(cst, sum(cs_s), extra, F32, T, sk))
    return out


def ratio(got, ref, bnd):
    "(largest err / bound, NaN count); an element with bound 0 must be exact."
    err = (got.double() - ref).abs()
    nan = torch.isnan(err)
    r = torch.where((err == 0) | nan, torch.zeros_like(err), err / bnd)
    return float(r.max()) if r.numel() else 0.0, int(nan.sum())


# ------------------------------------------------------------------------------------------ emulation
FAULTS = ("last_row_dropped", "block_counted_twice", "empty_slab_unwritten", "ix_m1_reads_row_above", "iy_H_reads_next_image", "stride2_as_1",
          "kx_shift_off_by_one", "interior_left_pixel_zeroed", "relu_ignored", "relu_on_dense", "colsum_twice", "dup_chunk_stored",
          "lda_as_I", "ldb_as_J")


def _fetch(buf, addr, valid=None):
    flat = buf.flatten().float()
    v = flat[addr.clamp(0, flat.numel() - 1)]
    return v if valid is None else torch.where(valid, v, torch.zeros_like(v))


def _gather_a(w, t, fault):
    lda = w["I"] if fault == "lda_as_I" else w["lda"]
    return _fetch(t["A_buf"], w["a_off"] + torch.arange(w["T"])[:, None] * lda + torch.arange(w["I"])[None])


def _gather_b(w, t, fault):
    "B_op [T, J] fp32 by the kernels' address arithmetic on the flat buffer (issue_stage of gemm_tn_kernel / conv_dw_rows_kernel)."
    T, J = w["T"], w["J"]
    tt = torch.arange(T)
    if w["conv"] is None:
        ldb = J if fault == "ldb_as_J" else w["ldb"]
        b = _fetch(t["B_buf"], w["b_off"] + tt[:, None] * ldb + torch.arange(J)[None])
        return torch.relu(b) if fault == "relu_on_dense" else b
    B, H, W, Cin, s = w["conv"]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    if fault == "stride2_as_1":
        s = 1
    row = tt // Wo
    ox, bimg, oy = tt - row * Wo, row // Ho, row % Ho
    k3 = torch.arange(3)
    iy = (oy * s - 1)[:, None, None] + k3[None, :, None]                 # [T, ky, 1]
    ix = (ox * s - 1)[:, None, None] + k3[None, None, :]                 # [T, 1, kx]
    iy_ok, ix_ok = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
    valid = iy_ok & ix_ok
    if w["kernel"] == "conv_rows":      # the staged pixels ox0 - 1 .. ox0 + 64 are LDS rows 0 .. 65 (66, 67: zero); tap kx reads row ox - ox0 + kx
        ox0 = (ox // 64 * 64)[:, None, None]
        r = ox[:, None, None] - ox0 + k3[None, None, :] + (1 if fault == "kx_shift_off_by_one" else 0)
        ix = ox0 - 1 + r
        valid = iy_ok & (r < 66) & (ix >= 0) & (ix < W)
        if fault == "interior_left_pixel_zeroed":
            valid = valid & ~((r == 0) & (ox0 > 0))
    if fault == "ix_m1_reads_row_above":
        valid = valid | (iy_ok & (ix == -1))
    if fault == "iy_H_reads_next_image":
        valid = valid | ((iy == H) & ix_ok)
    pix = (bimg[:, None, None] * H + iy) * W + ix                        # [T, ky, kx], relative to the first image
    addr = (H * W + pix)[..., None] * Cin + torch.arange(Cin)            # one NaN image lies in front
    b = _fetch(t["B_buf"], addr, valid[..., None].expand(addr.shape)).reshape(T, J)
    return torch.relu(b) if w["relu_b"] and fault != "relu_ignored" else b


def emulate(w, t, fault=None, pre=None):
    """The kernels' arithmetic as the bound models it, on CPU tensors: fp32, 32-row steps in t order, slabs added in slice order; the atomic
    colsum adds the slices to `pre` in slice order.  `fault`: one of FAULTS.  {name: tensor} as `reference`."""
    assert fault is None or fault in FAULTS
    a, b = _gather_a(w, t, fault), _gather_b(w, t, fault)
    T, I, J = w["T"], w["I"], w["J"]
    if fault == "last_row_dropped":
        a[T - 1], b[T - 1] = 0.0, 0.0
    sl = slices(w)
    if fault == "block_counted_twice" and len(sl) > 1:
        sl[0] = (sl[0][0], min(T, sl[0][1] + 64))
    owners = 2 if fault == "colsum_twice" and (tiles_ij(w)[1] > 1 or w["kernel"] == "conv_rows") else 1
    slabs, css = [], []
    for t0, t1 in sl:
        acc, cs = torch.zeros(I, J), torch.zeros(I)
        for u in range(t0, t1, 32):
            acc = acc + a[u:min(u + 32, t1)].t() @ b[u:min(u + 32, t1)]
            cs = cs + a[u:min(u + 32, t1)].sum(0)
        if fault == "empty_slab_unwritten" and t0 == t1:
            acc, cs = acc + float("nan"), cs + float("nan")
        if fault == "dup_chunk_stored":      # the columns past J of row i (products with the duplicated chunk J - 8 .. J - 1) land in row i + 1
            acc[1:, J - 8:] = a[t0:t1, :-1].t() @ b[t0:t1, J - 8:]
        slabs.append(acc)
        css.append(cs * owners)
    dw, cst = torch.zeros(I, J), (torch.zeros(I) if pre is None else pre.clone().float())
    for s_, c_ in zip(slabs, css):
        dw, cst = dw + s_, cst + c_
    if pre is not None:
        cst = (cst.double() - pre.double())
    return {"slabs": torch.stack(slabs), "dW": dw, "colsum_slabs": torch.stack(css), "colsum": cst}


if __name__ == "__main__":
    print(f"{len(ROUTES)} routes, {len(WITNESSES)} witnesses, {sum(ref_flop(w) for w in WITNESSES.values()) / 1e9:.1f} GFLOP of fp64 reference work")
    for n, w in WITNESSES.items():
        geo = " ".join(map(str, w["conv"])) if w["conv"] else ""
        print(f"  {n:15s} {w['T']:4d} {w['I']:4d} {w['J']:5d} {w['split_k']:2d}  {geo:16s} {w['lda']:4d} {w['a_off']:3d} {w['ldb']:4d} {w['b_off']:2d}  "
              f"{' '.join(sorted(features(w)))}   [{route(w)}]  {ref_flop(w) / 1e9:.2f} GFLOP")
