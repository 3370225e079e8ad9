"""CPU: the head streaming kernels' route audit's own machinery (tests/head_stream_routes.py) — every witness takes the kernel its route
names on the plan driver (tests/stream_plan_driver.cpp over uniception_amd/csrc/stream_plan.h), no route of the table goes unwitnessed and
every witness group the module names is there, the per-element bound passes a float32 model of each kernel's index arithmetic at or under
half (in front of the store; behind a 16-bit store it is held to the bound itself), every planted defect leaves the bound, leaves a NaN,
writes a guard band or breaks an exact relation on a witness of its own operation in every dtype, and the fp64 reference stays in budget."""
import pytest
import torch

from tests import head_stream_routes as R

CPU = torch.device("cpu")
W = R.WITNESSES


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("head_stream_routes"))


# ------------------------------------------------------------------------------------------ the plans and the table
def test_every_witness_takes_its_kernel_on_the_plan_driver(plan):
    names = [n for n in R.NAMES if R.planned(W[n])]
    for n, line in zip(names, plan([R.driver_row(W[n]) for n in names])):
        assert line == R.expected_plan(W[n]), f"{n}: the plan gives [{line}], the witness stands for [{R.route(W[n])}]: [{R.expected_plan(W[n])}]"


def test_no_route_of_the_table_goes_unwitnessed():
    have = {R.route(w) for w in W.values()}
    missing = [r for r in R.required_routes() if r not in have]
    assert not missing, f"routes without a witness: {missing}"
    assert have == set(R.required_routes()), f"witnessed routes the table does not know: {have - set(R.required_routes())}"


def test_the_grid_caps_of_the_witnesses_are_the_plans(plan):
    "npix = cap * per + k means a second iteration only if `cap` is where the plan stops growing the grid."
    rows = [dict(op="conv1x1", Cin=128, bias=R.BASE, npix=n) for n in (R.COOP_CAP * 16 - 1, R.COOP_CAP * 16, R.COOP_CAP * 16 + 1, 1 << 40)]
    rows += [dict(op="conv1x1_bwd", Cin=256, npix=n) for n in (R.BWD_CAP * 8 - 1, R.BWD_CAP * 8, R.BWD_CAP * 8 + 1, 1 << 40)]
    rows += [dict(op="conv1x1", Cin=24, bias=R.BASE, npix=n) for n in (R.EW_CAP * R.WG, R.EW_CAP * R.WG + 1)]
    out = [line.split() for line in plan(rows)]
    assert [line[-1] for line in out[:4]] == [str(R.COOP_CAP)] * 4 and {line[1] for line in out[:4]} == {"coop"}
    assert [line[-1] for line in out[4:8]] == [str(R.BWD_CAP)] * 4
    assert [line[-1] for line in out[8:]] == [str(R.EW_CAP)] * 2 and out[8][1] == "pixel"
    big = {W[n]["op"]: W[n] for n in R.BIG}
    assert big["c1"]["npix"] == R.COOP_CAP * R.WG // 16 + 3 and big["c1"]["Cin"] == 128 and big["c1"]["dt"] == "b"
    assert big["c1b"]["npix"] == R.BWD_CAP * R.lanes_of(256) + 5 and big["c1b"]["Cin"] == 256


def test_the_plan_is_the_rule_of_the_entry_points(plan):
    "rows kernel: rows2 != 0, sy <= 0.5f, a 16-bit dtype; fp16 always R = 4; bf16 R = 4 when rows2 == 4, else 2.  Cooperative: aligned bias, Cin = 8 * 2^k."
    rows, want = [], []
    for dt in "fbh":
        for Hi, Ho in ((3, 5), (19, 38), (37, 65), (5, 5), (5, 1), (1, 4), (4, 6), (4, 7)):
            for rows2 in (0, 1, 2, 3, 4, 8):
                rows.append(dict(op="bilinear", dtype=R.CODE[dt], Hi=Hi, Ho=Ho, crop_h=Ho, crop_w=3, C=8, B=2, rows2=rows2))
                up = R.scale32(Hi, Ho) <= 0.5 and rows2 != 0 and dt != "f"
                want.append(("rows", 4 if dt == "h" or rows2 == 4 else 2) if up else ("one_row", 1))
    for row, (k, r), line in zip(rows, want, plan(rows)):
        assert line.split()[1:3] == [k, str(r)] and int(line.split()[4]) == -(-row["crop_h"] // r), (row, line)
    rows = [dict(op="conv1x1", Cin=c, bias=R.BASE + a, npix=1000) for c in range(8, 257, 8) for a in (0, 4, 8, 12, 16)]
    for row, line in zip(rows, plan(rows)):
        coop = row["Cin"] in R.COOP_CIN and row["bias"] % 16 == 0
        assert line.split()[1:3] == (["coop", str(row["Cin"] // 8)] if coop else ["pixel", "0"]), (row, line)


def _group(op, **fields):
    return [w for w in W.values() if w["op"] == op and all(w.get(k) == v for k, v in fields.items())]


def _shape(w):
    return (w["Hi"], w["Wi"], w["Ho"], w["Wo"]), w["C"], ((w["ch"], w["cw"]) if R._cropped(w) else None)


def test_the_witness_table_is_what_the_module_says():
    for dt in "fbh":      # bilinear forward: every shape under every knob value that changes the dtype's kernel
        for rows2 in R.KNOBS[dt]:
            g = _group("bl", dt=dt, rule="ac", entry="bilinear", rows2=rows2)
            assert sorted(map(str, map(_shape, g))) == sorted(map(str, R.BL_SHAPES)), (dt, rows2)
    shapes = {s for s, _, _ in R.BL_SHAPES}
    assert {(19, 19, 38, 38), (3, 3, 5, 5), (5, 7, 10, 14), (37, 3, 65, 5), (37, 9, 19, 5), (1, 1, 4, 5), (5, 7, 1, 1), (6, 5, 6, 5)} <= shapes
    assert {c[0] for s, _, c in R.BL_SHAPES if s == (5, 5, 10, 10)} == set(range(1, 8))
    assert (R.DPT[2][1] * R.DPT[1] // 8, R.DPT[1]) == (296, 64) and {C for _, C, _ in R.BL_SHAPES} == {8, 64}
    assert R.scale32(3, 5) == 0.5 and R.scale32(37, 65) == 0.5625 and R.scale32(19, 38) < 0.5
    for dt in "bh":      # what the knob selects
        assert {R.bl_kernel(w) for w in _group("bl", dt=dt, rule="ac", entry="bilinear", rows2=0)} == {("one_row", 1)}
        assert ("rows", 4) in {R.bl_kernel(w) for w in _group("bl", dt=dt, rule="ac", entry="bilinear", rows2=4)}
    assert {R.bl_kernel(w) for w in _group("bl", dt="b", rule="ac", entry="bilinear", rows2=2)} == {("rows", 2), ("one_row", 1)}
    for dt in "fb":
        g = _group("blb", dt=dt, rule="ac", entry="bilinear")
        assert sorted(map(str, map(_shape, g))) == sorted(map(str, R.BL_SHAPES + R.BLB_EXTRA)), dt
    assert {s for s, _, _ in R.BLB_EXTRA} == {(37, 5, 10, 3), (19, 19, 38, 38), (5, 7, 1, 6)}
    for op, dts in (("bl", "fbh"), ("blb", "fbh")):
        for dt in dts:
            assert sorted(str((_shape(w)[0], w["C"])) for w in _group(op, dt=dt, rule="hp")) == sorted(map(str, R.HP_SHAPES)), (op, dt)
    assert {s for s, _ in R.HP_SHAPES} == {(5, 7, 12, 9), (7, 7, 3, 3), (7, 5, 2, 2), (4, 4, 8, 8), (5, 6, 5, 6), (1, 1, 3, 4), (5, 7, 1, 1)}
    for dt in "fbh":
        assert len(_group("bl", dt=dt, rule="ac", entry="resize")) == len(R.AC_RESIZE)
    for Cin in R.COOP_CIN:
        ppb = R.WG // (Cin // 8)
        assert {w["npix"] for w in _group("c1", Cin=Cin, mis=0, big=False)} == {1, ppb, ppb + 1, 3 * ppb + 2}
        assert {w["dt"] for w in _group("c1", Cin=Cin, mis=0, big=False)} == set("fbh")
    for dt in "fbh":
        assert {w["Cin"] for w in _group("c1", dt=dt) if R.c1_kernel(w)[0] == "pixel" and not w["mis"]} == {24, 72, 200}
        assert [w["Cin"] for w in _group("c1", dt=dt, mis=1)] == [64]
    for dt in "fb":
        for relu in (0, 1):
            for Cin in (8, 24, 72, 128, 256):
                ln = R.lanes_of(Cin)
                assert {w["npix"] for w in _group("c1b", dt=dt, relu=relu, Cin=Cin, big=False)} == {1, ln + 1, 3 * ln + 2}
    assert R.WG - R.lanes_of(24) * 3 == 1 and R.WG - R.lanes_of(72) * 9 == 4      # the dead threads
    for dt in "fb":
        g = _group("im", dt=dt)
        assert {(w["Cin"], w["stride"], w["relu"], w["ld"] - w["npix"]) for w in g} == {(c, s, r, p) for c in (5, 16, 72) for s in (1, 2) for r in (0, 1) for p in (0, 37)}
        assert all(w["npix"] % 64 and w["H"] % 2 and w["W"] % 2 for w in g)
        assert {(w["H"] - 2 * w["h"], w["W"] - 2 * w["w"]) for w in _group("di", dt=dt)} == {(0, -1), (-1, 0)}
    for op in ("pad", "padb", "emb"):
        assert {(w["H"], w["W"]) for w in _group(op)} == {(3, 5), (1, 5), (5, 1), (1, 1)}
    assert {(w["res"], w["relu"], w["dt"]) for w in _group("cadd")} == {(a, b, d) for a in (0, 1) for b in (0, 1) for d in "fbh"}
    assert all(w.get("B", 2) == 2 for w in W.values())


def test_the_reference_stays_inside_its_budget():
    for n in R.SMALL:
        assert R.reference_elems(W[n]) <= R.REF_BUDGET_ELEMS, n


# ------------------------------------------------------------------------------------------ the bound, without a GPU
_CACHE = {}
BIG_WINDOW = {n: (R.COOP_CAP * 16 - 40, W[n]["npix"]) for n in R.BIG if W[n]["op"] == "c1"}      # the seam of the second iteration


def _case(name, family):
    "Operands and reference of a witness, computed once and left unchanged."
    if (name, family) not in _CACHE:
        t = R.make_case(W[name], family, CPU, seed=R.seed_of(W[name]), window=BIG_WINDOW.get(name))
        _CACHE[name, family] = (t, R.reference(W[name], t))
    return _CACHE[name, family]


def _exact_relations(w, t, got):
    "The relations a launch must meet exactly; the names of those it breaks."
    broken = []
    if w["op"] == "c1b" and w["relu"] and bool((got["dfeat"][t["feat"] <= 0] != 0).any()):
        broken.append("dfeat is not exactly 0 under the mask")
    if w["op"] in ("bl", "blb") and (w["Hi"], w["Wi"]) == (w["Ho"], w["Wo"]) == (w["ch"], w["cw"]):
        src = t["src" if w["op"] == "bl" else "dy"]
        if not torch.equal(got[R.outputs(w)[0]].view(R.INTV[w["dt"]]), src.view(R.INTV[w["dt"]])):
            broken.append("an identity resize does not return the input's bits")
    return broken


@pytest.mark.parametrize("op", R.OPS)
def test_the_model_stays_at_or_under_half_the_bound(op):
    """In front of an fp32-class store at or under half the bound; behind a 16-bit store (one correct rounding, whose worst case IS
    u_out |ref|) inside the bound; the bands untouched, no NaN left, the exact relations met."""
    for name in [n for n in R.NAMES if W[n]["op"] == op]:
        w = W[name]
        for family in (R.FAMILIES if not w["big"] else ("wide",)):
            t, ref = _case(name, family)
            raw_b, got_b = R.model(w, t, store=False), R.model(w, t)
            assert R.bands_ok(w, t, raw_b) and R.bands_ok(w, t, got_b), (name, family)
            raw, got = R.results(w, t, raw_b), R.results(w, t, got_b)
            assert not _exact_relations(w, t, got), (name, family, _exact_relations(w, t, got))
            for o in R.outputs(w):
                code = R.store_code(w, o)
                front = R.ratio(raw[o], ref[o][0], R.unstored(*ref[o], code))
                behind = R.ratio(got[o], *ref[o])
                assert front[1] == 0 and front[0] <= 0.5, (name, family, o, front)
                assert behind[1] == 0 and behind[0] <= (0.5 if code == R.F32 else 1.0), (name, family, o, behind)


def _caught(w, t, ref, defect):
    "Why the defect shows on this case: a text, or None."
    bufs = R.model(w, t, defect)
    if not R.bands_ok(w, t, bufs):
        return "a guard band was written"
    got = R.results(w, t, bufs)
    for o in R.outputs(w):
        worst, bad, at = R.ratio(got[o], *ref[o])
        if bad:
            with pytest.raises(AssertionError, match=r"over the bound, worst err / bound .* at \(row \d+, col \d+\)"):
                R.check(R.route(w), o, got[o].reshape(-1, got[o].shape[-1]), *(v.reshape(-1, v.shape[-1]) for v in ref[o]))
            return f"{o}: {bad} elements over the bound or NaN, worst err / bound {worst:.3g}"
    broken = _exact_relations(w, t, got)
    return broken[0] if broken else None


def _applies(defect, w):
    "The witnesses on which the defect changes what the kernel does at all."
    if defect in R.HALFPIX_ONLY:
        return w["rule"] == "hp"
    if w["op"] in ("bl", "blb") and w["rule"] == "hp":
        return defect in ("range_without_margin", "clamped_tap_dropped")
    if defect in ("ragged_row_group_unwritten", "row_group_picks_next_row"):
        return R.bl_kernel(w)[0] == "rows"
    if defect == "fold_stops_one_step_early":
        return R.c1_kernel(w)[1] >= 2
    if defect == "second_stride_iteration_dropped":      # only the witnesses above a grid cap have a second iteration
        return w["npix"] > R.grid_of(w) * (R.lanes_of(w["Cin"]) if w["op"] == "c1b" or R.c1_kernel(w)[0] == "coop" else R.WG)
    if defect == "dead_thread_counted":
        return R.WG % (w["Cin"] // 8) != 0
    if defect == "dst_batch_stride_from_Ho":
        return bool(R._cropped(w))
    return True


def _kernels(defect, op):
    "The (dtype, kernel) pairs of the operation on each of which the defect has to be caught."
    out = {}
    for n in R.NAMES:
        w = W[n]
        if w["op"] == op and _applies(defect, w):
            key = (w["dt"],) + (R.bl_kernel(w) if op == "bl" else (w["rule"],) if op == "blb" else R.c1_kernel(w)[:1] if op == "c1" else ())
            out.setdefault(key, []).append(n)
    return out


@pytest.mark.parametrize("defect,op", [(d, op) for d, ops in R.DEFECTS.items() for op in ops])
def test_a_planted_defect_is_caught_by_a_witness_of_its_operation(defect, op):
    "On every (dtype, kernel) of the operation the defect can sit in: over the bound, a NaN left, a band written or an exact relation broken."
    groups = _kernels(defect, op)
    assert groups, (defect, op)
    for key, names in groups.items():
        hit = None
        for name in names:
            for family in (R.FAMILIES if not W[name]["big"] else ("wide",)):
                t, ref = _case(name, family)
                why = _caught(W[name], t, ref, defect)
                if why:
                    hit = (name, family, why)
                    break
            if hit:
                break
        assert hit, f"defect [{defect}] stays unseen on every witness of {op} {key}: {names}"
        print(f"defect [{defect}] on {op} {key}: first caught by [{hit[0]}] ({hit[1]}): {hit[2]}")


def test_one_wrong_column_is_named():
    "What a whole-tensor rel-L2 of 4e-3 lets through: the last column of one output row of the DPT shape 3 % off."
    name = next(n for n in R.PARENT if W[n]["op"] == "bl" and W[n]["dt"] == "b" and _shape(W[n]) == R.DPT)
    w = W[name]
    t, ref = _case(name, "wide")
    got = R.results(w, t, R.model(w, t))["dst"].clone()
    got[1, 36, 36] = (got[1, 36, 36].float() * 1.03).bfloat16()
    r = ref["dst"][0]
    assert float((got.double() - r).norm() / r.norm()) < 4e-3
    with pytest.raises(AssertionError, match=r"elements over the bound, worst err / bound"):
        R.check(R.route(w), "dst", got.reshape(-1, 64), r.reshape(-1, 64), ref["dst"][1].reshape(-1, 64))
