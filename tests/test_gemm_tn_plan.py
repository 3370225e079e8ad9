"""CPU: uc_gemm_tn's routing (uniception_amd/csrc/gemm_tn_plan.h) — which kernel, tiles, workgroup size, dynamic LDS and grid a
weight-gradient launch gets, and the split_k the library recommends for its shape.

tests/gemm_tn_plan_driver.cpp is compiled with the system C++ compiler against the host-only header and fed one descriptor per line.
Expected plans: `kernel tiles_i tiles_j tiles block lds_bytes grid auto_split_k`, worked by hand from the launcher and the two Python
split rules as they were before the plan header existed (uc_gemm_tn chose the kernel, autograd._split_k / _wgrad_conv the slice
count): tiles = ceil(I / (I <= 128 ? 128 : 256)) * ceil(J / 256), or 3 * (Cout / 128) * (Cin / 128) for the row kernel;
auto_split_k = max(1, min(T // 512, 256 // tiles)).  The bench rows are what the training legs launched, from their kernel trace."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every distinct uc_gemm_tn launch of the bench's training legs, recorded before the plan header existed:
# {leg: [[descriptor row incl. the split_k the caller passed, {kernel, block, lds_bytes, grid} of the kernel trace, launches per step], ...]}
with open(os.path.join(ROOT, "tests", "golden", "gemm_tn_plan_bench.json")) as _f:
    BENCH = json.load(_f)
KERNELS = {"256_dense", "256_conv", "128_dense", "128_conv", "conv_rows"}


def dense(T, I, J, **kw):
    row = dict(T=T, I=I, J=J, lda=I, ldb=J, A=4096, B=4096, C=4096)
    row.update(kw)
    return row


def conv(B, H, W, Cin, Cout, stride=1, **kw):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    row = dict(T=B * Ho * Wo, I=Cout, J=9 * Cin, lda=Cout, conv_B=B, conv_H=H, conv_W=W, conv_Cin=Cin, conv_stride=stride, A=4096, B=4096, C=4096)
    row.update(kw)
    return row


# one row on each side of every rule
RULES = {
 # dense tiles and the split rule
 "dense_1024x1024": (dense(131072, 1024, 1024, split_k=16),          # 4 x 4 tiles; min(256, 256 // 16)
     "256_dense 4 4 16 1024 131072 256 16"),
 "dense_explicit_split_k": (dense(131072, 1024, 1024, split_k=3),    # an explicit split_k multiplies the grid, the recommendation stays
     "256_dense 4 4 16 1024 131072 48 16"),
 "dense_split_by_cus": (dense(131072, 3072, 1024, split_k=5),        # 12 x 4 tiles; min(256, 256 // 48 = 5)
     "256_dense 12 4 48 1024 131072 240 5"),
 "dense_split_by_rows": (dense(4096, 128, 1152, split_k=8),          # half-height tile, 1 x 5; min(4096 // 512 = 8, 51)
     "128_dense 1 5 5 512 98304 40 8"),
 "dense_more_tiles_than_cus": (dense(131072, 4096, 4352),            # 16 x 17 = 272 tiles: 256 // 272 = 0 -> 1
     "256_dense 16 17 272 1024 131072 272 1"),
 "dense_short_reduction": (dense(256, 256, 256),                     # 256 // 512 = 0 -> 1
     "256_dense 1 1 1 1024 131072 1 1"),
 "dense_i_128": (dense(4096, 128, 256),
     "128_dense 1 1 1 512 98304 1 8"),
 "dense_i_136": (dense(4096, 136, 256),
     "256_dense 1 1 1 1024 131072 1 8"),
 "dense_j_512": (dense(131072, 256, 512),                            # min(256, 256 // 2)
     "256_dense 1 2 2 1024 131072 2 128"),
 "dense_j_520": (dense(131072, 256, 520),                            # one step past: a third column tile; min(256, 256 // 3)
     "256_dense 1 3 3 1024 131072 3 85"),
 # convolutions: the row kernel and each of its conditions failing alone
 "conv_rows": (conv(2, 64, 64, 256, 256, split_k=16),                # 3 ky x 2 x 2; T = 8192: min(16, 256 // 12 = 21)
     "conv_rows 2 2 12 512 101376 192 16"),
 "conv_rows_cout_128": (conv(2, 64, 64, 128, 128),                   # the row kernel comes before the half-height tile
     "conv_rows 1 1 3 512 101376 3 16"),
 "conv_stride_2": (conv(2, 64, 64, 256, 256, stride=2, split_k=4),   # T = 2048, J = 2304: 1 x 9; min(4, 28)
     "256_conv 1 9 9 1024 131072 36 4"),
 "conv_w_96": (conv(2, 64, 96, 256, 256),                            # T = 12288: min(24, 28)
     "256_conv 1 9 9 1024 131072 9 24"),
 "conv_cin_64": (conv(2, 64, 64, 64, 256),                           # J = 576: 3 column tiles; min(16, 85)
     "256_conv 1 3 3 1024 131072 3 16"),
 "conv_cout_192": (conv(2, 64, 64, 256, 192),
     "256_conv 1 9 9 1024 131072 9 16"),
 "conv_cout_128_im2col": (conv(2, 64, 96, 64, 128),                  # not a row-kernel shape (W, Cin) and I <= 128: half-height conv tile
     "128_conv 1 3 3 512 98304 3 24"),
}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/gemm_tn_plan_driver.cpp"
    exe = str(tmp_path_factory.mktemp("gemm_tn_plan") / "gemm_tn_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "uniception_amd", "csrc"), os.path.join(ROOT, "tests", "gemm_tn_plan_driver.cpp"), "-o", exe])

    def run(rows):
        lines = [" ".join(f"{k}={v}" for k, v in row.items()) for row in rows]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return run


def test_every_rule_on_both_sides(plan):
    got = plan([row for row, _ in RULES.values()])
    wrong = {name: (want, g) for (name, (_, want)), g in zip(RULES.items(), got) if g != want}
    assert not wrong, "\n".join(f"{n}: want {w!r}, got {g!r}" for n, (w, g) in wrong.items())


@pytest.mark.parametrize("leg", sorted(BENCH))
def test_bench_launches(plan, leg):
    """Every distinct uc_gemm_tn launch of the training legs of the bench (ViT-L/16 + 12-block decoder at 512^2: DPT heads at 64 pairs,
    the reference-policy leg's 16 pairs with bf16 and with fp32-class heads, the linear head at 64 pairs): the plan names the kernel,
    workgroup size, dynamic LDS and grid the kernel trace shows, and the recommended split_k is the one the caller had computed."""
    cases = BENCH[leg]
    got = [g.split() for g in plan([row for row, _, _ in cases])]
    wrong = []
    for i, ((row, ran, _), g) in enumerate(zip(cases, got)):
        kernel, tiles, block, lds, grid, auto = g[0], int(g[3]), int(g[4]), int(g[5]), int(g[6]), int(g[7])
        if (kernel, block, lds, grid, auto) != (ran["kernel"], ran["block"], ran["lds_bytes"], ran["grid"], row["split_k"]) or tiles * auto != grid:
            wrong.append(f"{leg}[{i}] {row}: ran {ran}, plan {' '.join(g)}")
    assert not wrong, "\n".join(wrong)


def test_every_kernel_is_covered(plan):
    seen = {want.split()[0] for _, want in RULES.values()} | {ran["kernel"] for cases in BENCH.values() for _, ran, _ in cases}
    assert seen == KERNELS


def test_descriptors_are_checked_before_any_launch():
    """uc_gemm_tn_query / uc_gemm_tn reject a bad descriptor with uc_gemm_tn's message before they touch the device (the pointers below
    are never dereferenced); the query checks the shape and nothing else."""
    from uniception_amd import _lib

    lib = _lib.load()

    def desc(**kw):
        d = _lib.GemmTnDesc(A=4096, B=4096, C=4096, T=4096, I=256, J=512, lda=256, ldb=512, split_k=1)
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def launch(**kw):
        return lib.uc_gemm_tn(C.byref(desc(**kw)), None), lib.uc_last_error().decode()

    def query(**kw):
        tiles, sk = C.c_int(-1), C.c_int(-1)
        return lib.uc_gemm_tn_query(C.byref(desc(**kw)), C.byref(tiles), C.byref(sk)), lib.uc_last_error().decode(), tiles.value, sk.value

    conv_geom = dict(T=2 * 64 * 64, conv_B=2, conv_H=64, conv_W=64, conv_Cin=256, conv_stride=1, ldb=0)
    for bad, text in ((dict(I=252), "multiples of 8"), (dict(J=9 * 128, **conv_geom), "conv shape mismatch"), (dict(relu_b=1), "ldb must be")):
        for status, msg in (launch(**bad), query(**bad)[:2]):
            assert status != 0 and msg.startswith("uc_gemm_tn:") and text in msg, (bad, status, msg)
    # launch only: split_k and the operands' alignment are not the shape's business
    for bad, text in ((dict(split_k=0), "bad split_k"), (dict(split_k=1025), "bad split_k"), (dict(A=4104), "16-byte aligned"), (dict(C=0), "null pointer")):
        status, msg = launch(**bad)
        assert status != 0 and msg.startswith("uc_gemm_tn:") and text in msg, (bad, status, msg)
        assert query(**bad)[0] == 0, bad
    assert lib.uc_gemm_tn(None, None) != 0 and lib.uc_last_error().decode() == "uc_gemm_tn: null descriptor"
    assert lib.uc_gemm_tn_query(None, None, None) != 0 and lib.uc_last_error().decode() == "uc_gemm_tn: null descriptor"
    # the query answers with NULL operands, ignores split_k, and either out-pointer may be NULL
    assert query(A=0, B=0, C=0, split_k=0)[2:] == (2, 8)                       # 1 x 2 tiles; min(4096 // 512, 256 // 2)
    assert query(A=0, B=0, C=0, J=9 * 256, I=256, lda=256, **conv_geom)[2:] == (12, 16)     # the row kernel: 3 x 2 x 2; min(16, 21)
    sk = C.c_int(-1)
    assert lib.uc_gemm_tn_query(C.byref(desc()), None, C.byref(sk)) == 0 and sk.value == 8
    assert lib.uc_gemm_tn_query(C.byref(desc()), None, None) == 0
