"""CPU: the uc_gemm_tn route audit's own machinery (tests/gemm_tn_routes.py) — every witness takes the kernel its route names on the plan
driver, every route and every feature is witnessed, the per-element bound passes an fp32 emulation of exactly the roundings it models at or
under half, without a NaN, and seeded faults of the kinds these kernels can have leave the bound or produce a NaN."""
import re

import pytest
import torch

from tests import gemm_tn_routes as R

CPU = torch.device("cpu")
OUTPUTS = ("slabs", "dW", "colsum_slabs", "colsum")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("gemm_tn_routes"))


def test_every_witness_takes_its_kernel_on_the_plan_driver(plan):
    lines = plan([R.driver_row(R.WITNESSES[n]) for n in R.NAMES])
    for n, line in zip(R.NAMES, lines):
        w = R.WITNESSES[n]
        assert line.split()[0] == w["kernel"], f"{n}: the plan gives [{line}], the witness stands for [{R.route(w)}]"
        assert " ".join(line.split()[:7]) == R.expected_plan(w), (n, line)


def test_every_route_and_every_feature_is_witnessed():
    assert len(R.ROUTES) == 24 and len(set(R.ROUTES)) == 24
    assert sorted(R.route(w) for w in R.WITNESSES.values()) == sorted(R.ROUTES)      # one witness per route, none for anything else
    for feat, kernels in R.FEATURES.items():
        for k in kernels:
            assert any(w["kernel"] == k and feat in R.features(w) for w in R.WITNESSES.values()), f"no {k} witness carries [{feat}]"
    for n, w in R.WITNESSES.items():
        assert R.features(w) <= set(R.FEATURES), n
        assert R.ref_flop(w) <= R.REF_BUDGET_FLOP, n
    # the shapes the mechanisms need (tests/gemm_tn_routes.py says why)
    W = R.WITNESSES
    rows = [w for w in W.values() if w["kernel"] == "conv_rows"]
    assert {w["conv"][2] for w in rows} == {64, 128} and {w["conv"][1] for w in rows} >= {1, 3} and {w["conv"][3] for w in rows} == {128, 256}
    assert {w["I"] for w in rows} == {128, 256} and all(w["conv"][0] == 2 for w in W.values() if w["conv"])
    assert any(w["split_k"] > w["T"] // 64 for w in rows) and any((w["T"] // 64) % w["split_k"] for w in rows)
    im = [w for w in W.values() if w["kernel"] in R.IM2COL]
    assert {w["conv"][3] for w in im} == {8, 24, 40} and any(w["conv"][1] == 1 for w in im) and any(w["conv"][2] == 1 for w in im)
    assert {(w["conv"][1] % 2, w["conv"][2] % 2) for w in im if w["conv"][4] == 2} >= {(1, 1), (0, 0)}
    assert {w["I"] for w in W.values() if w["kernel"] == "128_dense"} == {8, 72, 128} and W["d128_none"]["J"] == 8
    assert all(w["T"] % 8 for w in W.values() if w["conv"] is None)


def test_the_docstring_table_is_the_witnesses():
    "The table of tests/gemm_tn_routes.py's docstring, row by row: sizes, geometry, leading dimensions and the features derived from them."
    doc = R.__doc__
    for n, w in R.WITNESSES.items():
        m = re.search(rf"^\s+{n}\s+(.*)$", doc, re.M)
        assert m, f"{n} is missing from the table"
        tok = m.group(1).split()
        nums = [int(x) for x in tok if re.fullmatch(r"\d+", x)]
        want = [w["T"], w["I"], w["J"], w["split_k"]] + (list(w["conv"]) if w["conv"] else []) + [w["lda"], w["a_off"]]
        want += [w["ldb"], w["b_off"]] if w["conv"] is None else []
        assert nums == want, (n, nums, want)
        assert {x for x in tok if not re.fullmatch(r"\d+", x)} == R.features(w), n


# ------------------------------------------------------------------------------------------ the bound, without a GPU
_CACHE = {}


def _witness(name):
    "Operands, prefill and reference of a witness, computed once and left unchanged."
    if name not in _CACHE:
        w = R.WITNESSES[name]
        t = R.make_operands(w, CPU, seed=R.NAMES.index(name))
        pre = R.prefill(w, CPU, seed=R.NAMES.index(name)) if w["colsum"] == "atomic" else None
        _CACHE[name] = (w, t, pre, R.reference(w, t, pre))
    return _CACHE[name]


def _worst(name, fault=None):
    "{output: (largest err / bound, NaN count)} of the emulation of the witness."
    w, t, pre, ref = _witness(name)
    got = R.emulate(w, t, fault, pre)
    return {o: R.ratio(got[o], *ref[o]) for o in OUTPUTS}


@pytest.mark.parametrize("name", R.NAMES)
def test_the_emulated_roundings_stay_at_or_under_half_the_bound(name):
    """fp32 accumulation in 32-row steps, slabs added in slice order — the arithmetic the bound models, with every operand element fetched
    from the NaN-filled buffers by the kernels' address arithmetic: the witnesses, the guard layout and the reference agree."""
    w, t, _, _ = _witness(name)
    assert bool(torch.isnan(t["A_buf"]).any()) and bool(torch.isnan(t["B_buf"]).any()) and not bool(torch.isnan(t["A"]).any() | torch.isnan(t["B"]).any())
    if w["relu_b"]:
        x = t["B"].float()
        z = x == 0
        assert bool((x < 0).any()) and bool((z & ~torch.signbit(x)).any()) and bool((z & torch.signbit(x)).any())
    worst = _worst(name)
    print(name, {o: round(r, 4) for o, (r, _) in worst.items()})
    assert all(n == 0 for _, n in worst.values()), worst
    assert max(r for r, _ in worst.values()) <= 0.5, worst


# fault -> the witnesses (one of every kernel the fault belongs to) on which it must leave the bound or produce a NaN.
# Lines: uniception_amd/csrc/gemm_tn.hip, gemm_tn_kernel (G) / conv_dw_rows_kernel (R).
FAULT_CASES = {
    # 1. G issue_stage `if (t < p.T)` off by one; R has no row test (whole segments): the last segment's last A / pixel row lost
    "last_row_dropped": ["d256_none", "d128_none", "c256_r0_none", "c128_r0_none", "rows_r0_none"],
    # 2. G `nk = max(0, min(nk_per, nk_total - kt0))` / R `nk = max(0, min(per, nseg - s0))` one too many for slice 0
    "block_counted_twice": ["d256_slabs", "d128_slabs", "c256_r0_slabs", "c128_r0_slabs", "rows_r0_slabs"],
    # 3. nk == 0: the epilogue and the colsum store skipped (an early return on an empty slice) -> torch.empty memory
    "empty_slab_unwritten": ["d256_atomic", "d128_atomic", "c256_r0_atomic", "c128_r0_slabs", "rows_r1_slabs"],
    # 4. G `ix >= 0` missing in `if (iy >= 0 && iy < p.cH && ix >= 0 && ix < p.cW)`; 8b. R `ix >= 0` missing in
    #    `if (row_ok && r < 66 && ix >= 0 && ix < p.W)`: pixel W - 1 of the row above (the NaN image in front for row 0 of image 0)
    "ix_m1_reads_row_above": ["c256_r0_none", "c128_r0_slabs", "rows_r0_none", "rows_r1_slabs"],
    # 5. G `iy < p.cH` missing: row 0 of the next image (the NaN image behind the last one)
    "iy_H_reads_next_image": ["c256_r0_none", "c128_r0_atomic"],
    # 6. G `iy = oy * p.cStride - 1 + ky, ix = ox * p.cStride - 1 + kx` without the stride
    "stride2_as_1": ["c256_r0_atomic", "c256_r1_slabs", "c128_r0_none", "c128_r1_slabs"],
    # 7. R b_off: `row = f_row + 4 * h + kx` one row further along
    "kx_shift_off_by_one": ["rows_r0_none", "rows_r1_none"],
    # 8a. R the left pixel of an interior segment (ox0 > 0, LDS row 0) zeroed as if ox0 - 1 were outside the image
    "interior_left_pixel_zeroed": ["rows_r0_none", "rows_r1_atomic"],
    # 9. G `CONV && p.relu_b != 0` / R `if (relu)` dropped; G the `CONV &&` dropped with relu_b left over from a conv descriptor
    "relu_ignored": ["c256_r1_none", "c128_r1_none", "rows_r1_none"],
    "relu_on_dense": ["d256_none", "d128_none"],
    # 10. G `tj == 0` missing in do_colsum (two column tiles); R `tc == 0` (rows_r1_atomic: tiles_c = 2) or `ky == 1` missing
    "colsum_twice": ["d256_slabs", "d128_atomic", "c256_r0_slabs", "c128_r1_atomic", "rows_r1_atomic", "rows_r1_slabs"],
    # 11. G epilogue `jj + 3 < p.J` missing: the products with the clamped chunk (`col = lim - 8`) stored past J, i.e. into the next row
    "dup_chunk_stored": ["d256_slabs", "d128_none", "c256_r0_none", "c128_r0_none"],
    # 12. `p.A + t * p.lda` / `p.B + t * p.ldb` with I / J for the leading dimension
    "lda_as_I": ["d256_none", "d128_atomic", "c256_r1_none", "c128_r1_slabs", "rows_r0_atomic"],
    "ldb_as_J": ["d256_slabs", "d128_none"],
}


def test_every_fault_is_seeded_on_every_kernel_it_belongs_to():
    assert set(FAULT_CASES) == set(R.FAULTS)
    kernels = {f: {R.WITNESSES[n]["kernel"] for n in names} for f, names in FAULT_CASES.items()}
    for f in ("last_row_dropped", "block_counted_twice", "empty_slab_unwritten", "colsum_twice", "lda_as_I"):
        assert kernels[f] == set(R.KERNELS), f
    for f in ("iy_H_reads_next_image", "stride2_as_1"):
        assert kernels[f] == set(R.IM2COL), f
    assert kernels["ix_m1_reads_row_above"] == set(R.IM2COL) | {"conv_rows"}
    assert kernels["kx_shift_off_by_one"] == kernels["interior_left_pixel_zeroed"] == {"conv_rows"}
    assert kernels["relu_ignored"] == set(R.KERNELS[2:]) and kernels["relu_on_dense"] == kernels["ldb_as_J"] == set(R.KERNELS[:2])
    assert kernels["dup_chunk_stored"] == set(R.KERNELS[:4])


@pytest.mark.parametrize("fault,name", [(f, n) for f, names in FAULT_CASES.items() for n in names])
def test_a_seeded_fault_leaves_the_bound_or_produces_a_nan(fault, name):
    worst = _worst(name, fault)
    hit = {o: v for o, v in worst.items() if v[0] > 1.0 or v[1] > 0}
    print(f"fault [{fault}] on [{name}]: (err / bound, NaN) {worst}")
    assert hit, f"fault [{fault}] on [{name}] stays inside the bound of every output"
    w, t, pre, ref = _witness(name)
    o = sorted(hit)[0]
    got = R.emulate(w, t, fault, pre)[o]
    with pytest.raises(AssertionError, match="over the bound"):
        R.check(R.route(w), o, got.reshape(-1, got.shape[-1]), ref[o][0].reshape(-1, got.shape[-1]), ref[o][1].reshape(-1, got.shape[-1]),
                R.TILE[w["kernel"]])


def test_one_wrong_element_is_named():
    "What a whole-tensor rel-L2 of 2e-5 lets through: one element of a slab off by 1e-4 of its size."
    w, t, pre, ref = _witness("d256_slabs")
    got = R.emulate(w, t)["dW"].clone()
    got[200, 300] *= 1.0 + 1e-4
    assert float((got.double() - ref["dW"][0]).norm() / ref["dW"][0].norm()) < 2e-5
    with pytest.raises(AssertionError, match=r"1 of .*\n.*\(row 200, col 300\)"):
        R.check(R.route(w), "dW", got, *ref["dW"], R.TILE[w["kernel"]])
