"""CPU: the uc_gemm route audit's own machinery (tests/gemm_routes.py) — every route the bench launches has a driver-verified
witness, and the per-element checker passes correct fp32 arithmetic and catches seeded faults the global rel-L2 bar lets through."""
import time

import pytest
import torch

from tests import gemm_routes as R


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("gemm_routes"))


@pytest.fixture(scope="module")
def stored():
    return R.load_witnesses()


def test_every_recorded_signature_has_a_driver_verified_witness(plan, stored):
    bench = R.load_bench()
    rows = [row for cfg in sorted(bench) for row, _ in bench[cfg]]
    lines = plan(rows)
    sigs = {R.signature(r, l) for r, l in zip(rows, lines)}
    nts = {R.nt_combo(r, l) for r, l in zip(rows, lines)} - {None}
    print(f"{len(rows)} recorded rows, {len(sigs)} route signatures, {len(nts)} nt_out combinations")
    assert all("stagger" not in r for r in rows) and all(int(l.split()[5]) <= 0 for l in lines), "stagger > 0 occurs: witness it"
    assert sigs == set(stored["routes"]) and nts == set(stored["nt"])
    # default knobs, cus = 256 (the recorded rows carry no knob of their own)
    for sig, row in stored["routes"].items():
        assert R.signature(row, plan([row])[0]) == sig, sig
        assert row == R.normalize(row), sig
    for nt, row in stored["nt"].items():
        line = plan([row])[0]
        assert R.nt_combo(row, line) == nt, nt
        out_bytes = row["M"] * row["N"] * (4 if row.get("out_dtype", 0) == R.F32 else 2)
        assert (128 << 20) < out_bytes <= (160 << 20), (nt, out_bytes)


def test_stored_witnesses_are_what_the_shrinker_derives(plan, stored):
    "No hand-picked shapes: the fixture is the greedy shrinker's output on this tree's plan (regenerate: python -m tests.gemm_routes)."
    assert R.derive_witnesses(plan) == stored


def test_witnesses_stay_within_the_reference_budget(stored):
    flops = {sig: R.ref_flop(r) for part in stored.values() for sig, r in part.items()}
    print(f"fp64 reference work of all witnesses: {sum(flops.values()) / 1e12:.2f} TFLOP, largest {max(flops.values()) / 1e9:.0f} GFLOP")
    over = {s: f for s, f in flops.items() if f > R.REF_BUDGET_FLOP}
    assert not over, over


def test_ragged_edges(plan, stored):
    "Every witness has a ragged last row tile except the ones the module docstring names."
    unragged = []
    for sig, row in stored["routes"].items():
        kernel = plan([row])[0].split()[0]
        if row["M"] % R.TILE[kernel][0] == 0:
            unragged.append(sig)
    assert all(s.startswith("conv_rows8 ") or s == "t256x256 all side0 fuse0 vec1 relu_a0 slices0 cd1 od1 am1 stride1" for s in unragged), unragged


def test_tile_order_rows_have_a_full_and_a_ragged_tile_group_on_every_kernel(plan):
    """The hand-written part of the fixture: one row per direct-to-LDS kernel, planned onto that kernel with six row tiles (group_m = 4:
    one full tile group and a ragged one of two) and at least two column tiles, within the reference budget."""
    rows = R.load_tile_order()
    assert set(rows) == {"t128x128_s3", "t256x256", "eight_wave", "four_wave", "conv_rows", "conv_rows8", "conv_rows8_flat"}
    for kernel, row in rows.items():
        assert row == R.normalize(row), kernel
        p = dict(zip(R.PLAN_FIELDS, plan([row])[0].split()))
        assert p["kernel"] == kernel, (kernel, p)
        assert int(p["tiles_m"]) == 6 and int(p["tiles_n"]) >= 2 and int(p["slices"]) == 1, (kernel, p)
        assert "gemm_group_m" not in row      # the default: 4 row panels per group, 6 % 4 != 0
        assert 2 <= row["K"] // 64 <= 9, kernel
        assert R.ref_flop(row) <= R.REF_BUDGET_FLOP, kernel


def test_vt_positions_are_the_literal_formula():
    for ntok in (35, 64, 449):
        want = [16 * (n // 16) + (((n % 16) >> 2) & 1) * 8 + ((n % 16) & 3) + 4 * ((n % 16) >> 3) for n in range(ntok)]
        assert R.vt_positions(ntok).tolist() == want
    row = {"M": 70, "N": 192, "vt_col0": 64, "vt_ntok": 35, "vt_npad": 64}
    v = torch.arange(70 * 128, dtype=torch.float32).view(70, 128)
    packed = R.pack_vt(v, row)
    for (b, n, h, d) in [(0, 0, 0, 0), (1, 34, 1, 63), (0, 7, 1, 5), (1, 20, 0, 33)]:
        w = n % 16
        assert packed[b, h, d, 16 * (n // 16) + ((w >> 2) & 1) * 8 + (w & 3) + 4 * (w >> 3)] == v[b * 35 + n, h * 64 + d]
    assert torch.equal(R.unpack_vt(packed, row), v)


# ------------------------------------------------------------------------------------------ the checker, without a GPU
EMU_FLOP = 8.0e9      # witnesses emulated on the CPU: the smallest of each epilogue kind, none above this


def _kind(sig):
    "Epilogue kind of a signature: the family and every epilogue feature, without kernel / tile / operand-path words."
    w = sig.split()
    drop = ("side", "fuse", "vec", "slices", "am", "stride")
    return " ".join(x for x in w[1:] if not x.startswith(drop))


def _emu_witnesses(stored):
    """The smallest witness of every epilogue kind.  A kind whose every witness is above EMU_FLOP (the row kernels need 256 tiles) is
    emulated on fewer images / rows of its witness: the emulation's arithmetic does not know the route, only the expression."""
    best = {}
    for sig, row in stored["routes"].items():
        k = _kind(sig)
        if k not in best or R.ref_flop(row) < R.ref_flop(best[k][1]):
            best[k] = (sig, row)
    for k, (sig, row) in best.items():
        while R.ref_flop(row) > EMU_FLOP:
            f = ("conv_B" if row["conv_B"] > 1 else "conv_H") if row.get("a_mode", 0) == 1 else "M"
            assert not row.get("vt_col0", -1) >= 0 and row[f] > 1
            row = R.normalize({**row, f: row[f] // 2})
        best[k] = (sig, row)
    return best


def _check_all(sig, row, t, got, tile=(128, 128)):
    ref = R.reference(row, t)
    for name, (r, b) in ref.items():
        R.check(sig, name, got[name], r, b, tile)
    if row.get("stats_out"):
        r, b = R.stats_reference(got["C"])
        R.check(sig, "stats", got["stats"], r, b, tile)
    return ref


def _emulate(row, t):
    got = R.emulate(row, t)
    if row.get("stats_out"):
        got["stats"] = R.emulate_stats(got["C"])
    return got


def test_fp32_emulation_passes_the_bound_for_every_epilogue_kind(stored):
    """The bound is not tighter than correct arithmetic: fp32 matmul of the rounded operands, fp32 epilogue (torch's fp32 erf, sin,
    cos), one rounding — zero violations for a witness of each epilogue kind, in range and (fp16 outputs) with saturated elements."""
    torch.manual_seed(0)
    kinds = _emu_witnesses(stored)
    assert set(kinds) == {_kind(s) for s in stored["routes"]}
    t0 = time.time()
    for i, (k, (sig, row)) in enumerate(sorted(kinds.items())):
        t = R.make_operands(row, torch.device("cpu"), seed=i)
        _check_all(sig, row, t, _emulate(row, t))
        if row.get("out_dtype", 0) == R.F16 and not row.get("tail_out"):
            t = R.make_operands(row, torch.device("cpu"), seed=i, saturate=True)
            got = _emulate(row, t)
            assert int((got["C"].float().abs() == 65504).sum()) > 0, sig
            _check_all(sig, row, t, got)
    print(f"{len(kinds)} epilogue kinds emulated in {time.time() - t0:.1f} s")


def _witness(stored, sig):
    return stored["routes"][sig]


BS = "t128x128_s3 bs side0 fuse0 vec1 relu_a0 slices0 cd1 od1 am0 stride0 res1 bias residual stats_out"
RES2 = "t128x128_s3 all side0 fuse0 vec1 relu_a0 slices0 cd2 od2 am1 stride1 res2 bias residual residual2 sat_flag"
VT = "t128x128_s3 bf16 side0 fuse0 vec1 relu_a0 slices0 cd1 od1 am0 stride0 ln_nblk vt bias rope_cols ln_stats"


def _caught(sig, row, t, got):
    with pytest.raises(AssertionError, match="over the bound") as e:
        _check_all(sig, row, t, got)
    return str(e.value)


def test_seeded_faults_are_caught_and_the_global_metric_misses_the_local_ones(stored):
    row = _witness(stored, BS)
    t = R.make_operands(row, torch.device("cpu"), seed=3)
    good = _emulate(row, t)
    ref = _check_all(BS, row, t, good)
    c_ref, c_bnd = ref["C"]
    assert R.rel_l2(good["C"], c_ref) < 6e-3

    # one element with |value| >= 0.25 moved by 3 ulp of the output type
    got = {k: v.clone() for k, v in good.items()}
    r, c = (good["C"].float().abs() >= 0.25).nonzero()[17].tolist()
    bits = got["C"].view(torch.int16)
    bits[r, c] += 3
    got["stats"] = R.emulate_stats(got["C"])
    msg = _caught(BS, row, t, got)
    assert f"(row {r}, col {c})" in msg and f"tile ({r // 128}, {c // 128})" in msg and "1 of" in msg
    assert R.rel_l2(got["C"], c_ref) < 6e-3, "the old global bar does not see it"

    # one element replaced by the element one row below (the two differ by more than the bound)
    got = {k: v.clone() for k, v in good.items()}
    far = ((c_ref[1:] - c_ref[:-1]).abs() > 2 * c_bnd[:-1]).nonzero()[5].tolist()
    got["C"][far[0], far[1]] = good["C"][far[0] + 1, far[1]]
    got["stats"] = R.emulate_stats(got["C"])
    _caught(BS, row, t, got)
    assert R.rel_l2(got["C"], c_ref) < 6e-3, "the old global bar does not see it"

    # bias shifted by one column in one 64-column block
    t2 = dict(t)
    t2["bias"] = t["bias"].clone()
    t2["bias"][64:128] = t["bias"][63:127]
    shifted = _emulate(row, t2)
    got = {k: v.clone() for k, v in good.items()}
    got["C"][:, 64:128] = shifted["C"][:, 64:128]
    got["stats"] = R.emulate_stats(got["C"])
    _caught(BS, row, t, got)

    # the last row of a ragged M left at its initial fill
    assert row["M"] % 128 != 0
    got = {k: v.clone() for k, v in good.items()}
    got["C"][-1, :] = float("nan")
    got["stats"] = R.emulate_stats(torch.nan_to_num(got["C"]))
    assert f"row {row['M'] - 1}" in _caught(BS, row, t, got)

    # statistics of another row
    got = {k: v.clone() for k, v in good.items()}
    got["stats"][1, 5] = good["stats"][1, 6]
    assert "output stats" in _caught(BS, row, t, got)


def test_a_dropped_second_residual_on_one_row_is_caught(stored):
    row = _witness(stored, RES2)
    t = R.make_operands(row, torch.device("cpu"), seed=4)
    good = _emulate(row, t)
    _check_all(RES2, row, t, good)
    t2 = {k: v for k, v in t.items() if k != "residual2"}
    dropped = R.emulate({k: v for k, v in row.items() if k != "residual2"}, t2)
    got = {k: v.clone() for k, v in good.items()}
    r = row["M"] - 3      # a row of the last tile
    got["C"][r] = dropped["C"][r]
    assert f"(row {r}," in _caught(RES2, row, t, got)


def test_an_unpermuted_vt_position_is_caught(stored):
    row = _witness(stored, VT)
    t = R.make_operands(row, torch.device("cpu"), seed=5)
    good = _emulate(row, t)
    _check_all(VT, row, t, good)
    packed = R.pack_vt(good["vt"], row)
    assert torch.equal(R.unpack_vt(packed, row), good["vt"])
    n = 20      # token 20 of image 0 belongs at position 16 + perm(4) = 24; written at 20, where token 24's value belongs
    assert int(R.vt_positions(row["vt_ntok"])[n]) == 24
    packed[0, :, :, 20] = good["vt"].view(-1, row["vt_ntok"], packed.shape[1], 64)[0, n]
    got = dict(good)
    got["vt"] = R.unpack_vt(packed, row)
    assert "output vt" in _caught(VT, row, t, got)
