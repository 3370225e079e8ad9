"""CPU: the attention route audit's own machinery (tests/attention_routes.py) — every kernel name the plan driver can print has a
driver-verified witness or a stated excuse, the per-element bound passes an emulation of exactly the roundings it models with room to
spare, and seeded faults of the kinds these kernels can have leave the bound (most of them under the old whole-tensor rel-L2 bars)."""
import pytest
import torch

from tests import attention_routes as R

FWD_BAR, BWD_BAR = 8e-3, 1.5e-2      # the whole-tensor rel-L2 bars of tests/test_ops_gpu.py and tests/test_train_ops_gpu.py


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("attention_routes"))


def test_every_witness_takes_its_route_and_every_printable_route_is_witnessed_or_excused(plan):
    names = sorted(R.WITNESSES)
    lines = plan([R.driver_row(R.WITNESSES[n], cus=256) for n in names])
    for n, line in zip(names, lines):
        w = R.WITNESSES[n]
        assert R.route_of(w["fn"], line) == w["route"], f"{n}: the plan gives [{line}], the witness stands for [{w['route']}]"
        assert R.shape_for(w, 256) == w["shape"], n
    routes = {w["route"] for w in R.WITNESSES.values()}
    fwd = set(R.FWD_KERNELS)
    # the backward pairs the plan can print: bf16 without dropout any (dq32 | dq64) x (dkv32 | dkv64), dropout and fp32 in matched pairs
    bwd = {f"{a} {b}" for a in ("dq32", "dq64") for b in ("dkv32", "dkv64")} | {"dq32_drop dkv32_drop", "f32_dq32 f32_dkv32", "f32_dq64 f32_dkv64"}
    assert {k for pair in bwd for k in pair.split()} == set(R.DQ_KERNELS) | set(R.DKV_KERNELS)
    missing = (fwd | bwd) - routes
    assert missing == set(R.UNWITNESSED), f"neither witnessed nor excused: {missing - set(R.UNWITNESSED)}; excused but witnessed: {set(R.UNWITNESSED) - missing}"
    assert routes <= fwd | bwd
    # the excuses hold: the diag kernel needs dbg != 0, dq32 dkv64 the 4 GB rule
    assert plan([{**R.driver_row(R.WITNESSES["dma4"]), "dbg": 1}])[0].split()[0] == "dma4_dbg"
    row = R.driver_row(R.WITNESSES["dq64_dkv64"])
    big = {**row, "v_sn": 8388608, "v_sb": row["Nk"] * 8388608}
    ext = ((row["B"] - 1) * big["v_sb"] + (row["H"] - 1) * row["v_sh"] + (row["Nk"] - 1) * big["v_sn"] + 64) * 2
    assert ext > (4 << 30) - 1 and R.route_of("bwd", plan([big])[0]) == "dq32 dkv64"
    small = {**row, "v_sn": 4194304, "v_sb": row["Nk"] * 4194304}
    assert R.route_of("bwd", plan([small])[0]) == "dq64 dkv64"


@pytest.mark.parametrize("cus", [304, 128, 80])
def test_cu_dependent_witnesses_keep_their_route_on_other_devices(plan, cus):
    names = [n for n in sorted(R.WITNESSES) if R.WITNESSES[n]["cu_rule"]]
    assert names
    for n, line in zip(names, plan([R.driver_row(R.WITNESSES[n], cus=cus) for n in names])):
        w = R.WITNESSES[n]
        assert R.route_of(w["fn"], line) == w["route"], (n, cus, line)
        if w["seam"]:      # more items than workgroups
            B, H, Nq, Nk = R.shape_for(w, cus)
            grid = int(line.split()[1])
            assert B * H * ((Nq + 255) // 256) > grid and (B * H) % grid != 0, (n, cus, line)


def test_witnesses_stay_small():
    for n, w in R.WITNESSES.items():
        B, H, Nq, Nk = w["shape"]
        assert B * max(Nq, Nk) * H * w["D"] * (2 if w["dtype"] == R.BF16 else 4) <= 21e6, n          # the largest operand
        n_bh = max(1, R.CHUNK_ELEMS // (Nq * Nk * w["D"]))
        assert min(n_bh, B * H) * Nq * Nk * w["D"] * 8 * 3 <= 0.5e9, n                                 # a chunk and its two temporaries


# ------------------------------------------------------------------------------------------ the bound, without a GPU
EMU = [n for n, w in R.WITNESSES.items() if w["dtype"] == R.BF16 and not w["cu_rule"]]      # every small bf16 witness
SEEDS = R.SEEDS
HALF = ("dma4_tiny", "dma4", "dq32_dkv32")      # the smallest bf16 forward and backward witnesses: err / bound <= 0.5


def _run(name, fault=None):
    "Emulate the witness (forward, then the backward on the emulated o and lse) and return {output: (got, ref, bound)}, flagged rows."
    w = R.WITNESSES[name]
    shape = R.shape_for(w)
    t = R.make_operands(w, shape, seed=SEEDS[name])
    scale = w["D"] ** -0.5
    mask = R.host_drop_mask(shape, w["drop"], SEEDS[name]) if w["drop"] else None
    bwd = w["fn"] == "bwd"
    fwd_w = dict(w, route="dma4") if bwd else w
    o, lse = R.emulate_fwd(fwd_w, t, scale, mask, None if bwd else fault)
    got = {"O": o, "LSE": lse}
    if bwd:
        got["dQ"], got["dK"], got["dV"] = R.emulate_bwd(w, t, o, lse, scale, mask, fault)
    ref, flagged = R.reference(w, t, scale, mask)
    return {n: (got[n], *ref[n]) for n in ref}, flagged


@pytest.mark.parametrize("name", EMU)
def test_the_emulated_roundings_stay_at_or_under_half_the_bound(name):
    """bf16 P, the re-rounded Q / K, bf16 dS, one bf16 store, fp32 sums: the arithmetic the bound models, on every small bf16 witness (the
    CU-sized ones differ from them in size only).  Every output inside the bound; worst err / bound <= 0.5 on the smallest forward and
    backward witnesses (their seeds are chosen for it: tests/attention_routes.py SEEDS says why O sits at that bar)."""
    res, flagged = _run(name)
    worst = {n: R.check(name, n, *res[n]) for n in res}
    print(name, {n: round(v, 3) for n, v in worst.items()})
    assert max(worst.values()) <= (0.5 if name in HALF else 1.0), worst
    assert bool(flagged.any()) == R.WITNESSES[name]["fixup"], "only the fix-up witness leaves the persistent kernel's score range"


def test_the_fixup_witness_spikes_a_block_of_the_ragged_last_key_tile():
    w = R.WITNESSES["p64_fixup"]
    shape = R.shape_for(w)
    _, flagged = _run("p64_fixup")
    b, q, h, k = R.spike_position(w, shape)
    assert bool(flagged[b, h, q]) and k // 64 == (shape[3] - 1) // 64 and shape[3] % 64 and q // 64 == (shape[2] - 1) // 64
    assert int(flagged.sum()) == 1


def _caught(name, fault, outputs):
    res, _ = _run(name, fault)
    clean, _ = _run(name)
    over, global_sees = {}, {}
    for n in outputs:
        got, ref, bnd = res[n]
        over[n] = int((R.ratio(got, ref, bnd) > 1.0).sum())
        bar = FWD_BAR if R.WITNESSES[name]["fn"] == "fwd" else BWD_BAR
        global_sees[n] = R.rel_l2(got, ref) >= bar
        assert R.rel_l2(clean[n][0], ref) < bar
    hit = [n for n in outputs if over[n]]
    print(f"fault [{fault}] on [{name}]: elements over the bound {over}; caught by the whole-tensor rel-L2 bar: {global_sees}")
    assert hit, f"fault [{fault}] on [{name}] stays inside the bound of every output"
    with pytest.raises(AssertionError, match="over the bound"):
        R.check(name, hit[0], *res[hit[0]])
    return global_sees


FWD_FAULTS = ["last_key_dropped", "pad_key_admitted_with_score_0", "v_rows_swapped_in_a_16_key_block", "rescale_skipped_for_the_spiked_row",
              "query_row_from_neighbouring_head"]
BWD_FAULTS = ["delta_omitted_from_dS", "scale_applied_twice_to_dK"]


@pytest.mark.parametrize("fault", FWD_FAULTS)
def test_a_seeded_forward_fault_leaves_the_bound(fault):
    _caught("dma4", fault, ["O", "LSE"])


@pytest.mark.parametrize("fault", BWD_FAULTS)
def test_a_seeded_backward_fault_leaves_the_bound(fault):
    _caught("dq32_dkv32", fault, ["dQ", "dK", "dV"])


def test_the_failure_names_the_element_and_its_tiles():
    res, _ = _run("dma4")
    got, ref, bnd = res["O"]
    got = got.clone()
    got[1, 70, 2, 33] += 0.5
    with pytest.raises(AssertionError) as e:
        R.check("dma4", "O", got, ref, bnd)
    assert "(b 1, h 2, row 70, d 33)" in str(e.value) and "64-row tile 1, 128-row tile 0" in str(e.value) and "1 of" in str(e.value)
    lse = res["LSE"][0].clone()
    lse[0, 1, 129] = float("nan")
    with pytest.raises(AssertionError, match=r"\(b 0, h 1, row 129, d 0\)"):
        R.check("dma4", "LSE", lse, *res["LSE"][1:])
