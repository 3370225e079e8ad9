"""CPU: the LayerNorm route audit's own machinery (tests/layernorm_routes.py) — every witness takes the kernel its route names on the plan
driver, no (direction, kernel, nv, nt) the plans can return goes unwitnessed, the per-element bound passes a float32 model of the kernel
arithmetic at or under half (in front of the store; behind a bf16 store it is held to the bound itself, see the module), and every planted
defect of the kinds these kernels can have leaves the bound or produces a NaN on a witness of every kernel it belongs to."""
import os

import pytest
import torch

from tests import layernorm_routes as R

CPU = torch.device("cpu")
W = R.WITNESSES


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("layernorm_routes"))


# ------------------------------------------------------------------------------------------ the plans
def test_every_witness_takes_its_kernel_on_the_plan_driver(plan):
    lines = plan([R.driver_row(W[n]) for n in R.NAMES])
    for n, line in zip(R.NAMES, lines):
        assert line == R.expected_plan(W[n]), f"{n}: the plan gives [{line}], the witness stands for [{R.route(W[n])}]"


def test_the_witness_table_is_what_the_module_says():
    fwd = [w for w in W.values() if w["dir"] == "fwd"]
    bwd = [w for w in W.values() if w["dir"] == "bwd"]
    small = [w for w in fwd if not w["nt"]]
    assert {w["rows"] for w in small} == {1, 5, 9}
    for k in ("exact", "vec", "scalar"):
        assert {(w["x"], w["o"], w["twin"]) for w in small if w["kernel"] == k} == {(x, y, t) for x, y in R.PAIRS for t in (0, 1)}, k
        assert {w["rows"] for w in small if w["kernel"] == k} == {1, 5, 9}, k
    for nv in R.NVS:
        assert {(w["x"], w["o"], w["twin"]) for w in small if w["kernel"] == "exact" and w["nv"] == nv} == {(x, y, t) for x, y in R.PAIRS for t in (0, 1)}
        assert {w["rows"] for w in small if w["kernel"] == "exact" and w["nv"] == nv} == {1, 5, 9}
    assert {w["C"] for w in small if w["kernel"] == "vec"} == {4, 64, 80, 96, 100, 1280, 1792, 2044}
    assert {(w["C"], w["mis"]) for w in small if w["kernel"] == "scalar"} == {(1, None), (67, None), (2052, None), (768, "x"), (768, "twin"), (768, "y"),
                                                                              (768, "gamma"), (768, "beta")}
    nt = [w for w in fwd if w["nt"]]
    assert sorted((w["x"], w["o"], w["nv"]) for w in nt) == sorted([("f", y, nv) for nv in R.NVS for y in "fb"] + [("b", "b", 1), ("b", "f", 1)])
    for w in nt:       # the smallest rows above the policy's threshold with a ragged last workgroup
        b = R.BYTES[w["x"]]
        assert w["rows"] % 4 == 1 and w["rows"] * w["C"] * b > R.NT_BYTES and (w["rows"] - 4) * w["C"] * b <= R.NT_BYTES
    wide = [w for w in bwd if w["kernel"] == "wide"]
    combos = {(x, dy, d, t) for x, dy in R.PAIRS for d in (0, 1) for t in ((0, 1) if x == "f" else (0,))}
    for nv in R.NVS:
        for rows in (1, 13):
            assert {(w["x"], w["o"], w["dres"], w["twin"]) for w in wide if w["nv"] == nv and w["rows"] == rows} == combos
        assert sorted(w["rows"] for w in wide if w["nv"] == nv and w["big"]) == [R.WIDE_CAP + 3, 2 * R.WIDE_CAP + 5]
        assert all(w["dres"] for w in wide if w["nv"] == nv and w["big"])
    c64 = [w for w in bwd if w["kernel"] == "c64"]
    assert {(w["x"], w["o"], w["rows"]) for w in c64} == {(x, dy, r) for x, dy in R.PAIRS for r in (1, 3, 18, R.C64_CAP + 7)}
    gen = [w for w in bwd if w["kernel"] == "generic"]
    assert any(w["C"] == 64 and w["dres"] for w in gen) and any(w["C"] == 64 and w["twin"] for w in gen)
    assert {w["C"] for w in gen if not w["mis"]} == {1, 64, 67, 80, 96, 1280, 2052}
    assert {w["mis"] for w in gen if w["C"] == 768} == {"x", "dy", "dres", "dx", "twin", "gamma"}
    for C in (1, 67, 80, 96, 1280, 2052):
        assert {(w["x"], w["o"]) for w in gen if w["C"] == C} == set(R.PAIRS)
    assert {w["dres"] for w in gen} == {0, 1} and {w["twin"] for w in gen} == {0, 1}


def test_the_grid_caps_of_the_witnesses_are_the_plans(plan):
    "rows = cap + 3 / 2 cap + 5 / cap + 7 mean what the module says only if `cap` is where the plan stops growing the grid."
    rows = [dict(dir="bwd", rows=r, C=C, x=R.BASE, dy=R.BASE, dx=R.BASE, gamma=R.BASE) for C, cap in ((768, R.WIDE_CAP), (64, R.C64_CAP))
            for r in (cap - 1, cap, cap + 1, 1 << 40)]
    out = [line.split() for line in plan(rows)]
    for k, (kernel, cap) in enumerate((("wide", R.WIDE_CAP), ("c64", R.C64_CAP))):
        below, at, above, far = out[4 * k:4 * k + 4]
        assert {line[1] for line in (below, at, above, far)} == {kernel}
        per = int(at[3])
        assert int(at[4]) * per == cap and int(below[4]) == int(at[4]) == int(above[4]) == int(far[4]) and int(below[4]) * per - (cap - 1) < per


def test_no_route_the_plans_return_goes_unwitnessed(plan):
    """Every (direction, kernel, nv, nt) the plans give over C in [1, 4200] x all pointers at alignment 16, 8, 4 or 2 x x of 4 / 2 bytes x
    has_dres x has_twin x rows in {1, 2^20} (the larger is above the non-temporal threshold from C = 32), and with one pointer at a time
    misaligned at the witnesses' widths, has a witness.  A condition, not a quota."""
    have = {R.plan_key(w) for w in W.values()}
    rows = []
    for C in range(1, 4201):
        for a in (16, 8, 4, 2):
            p = R.BASE + a % 16
            for r in (1, 1 << 20):
                for xb in (4, 2):
                    if a < xb:
                        continue      # not element-aligned: outside the contract
                    for twin in (0, p):
                        rows.append(dict(dir="fwd", rows=r, C=C, x_bytes=xb, x=p, y=p, gamma=R.BASE + a % 16 if a >= 4 else R.BASE, beta=R.BASE, twin=twin))
                        for dres in (0, p):
                            rows.append(dict(dir="bwd", rows=r, C=C, x_bytes=xb, dy_bytes=xb, x=p, dy=p, dx=p, gamma=R.BASE, dres=dres, twin=twin))
    for C in sorted({w["C"] for w in W.values()}):
        for name in ("x", "y", "twin", "gamma", "beta", "dy", "dres", "dx"):
            for a in (8, 4, 2):
                base = dict(rows=9, C=C, x_bytes=2, dy_bytes=2, x=R.BASE, y=R.BASE, twin=R.BASE, gamma=R.BASE, beta=R.BASE, dy=R.BASE, dres=R.BASE, dx=R.BASE)
                base[name] = R.BASE + a
                rows.append(dict(dir="fwd", **{k: v for k, v in base.items() if k not in ("dy", "dres", "dx", "dy_bytes")}))
                rows.append(dict(dir="bwd", **{k: v for k, v in base.items() if k not in ("y", "beta")}))
    seen = {}
    for row, line in zip(rows, plan(rows)):
        tok = line.split()
        key = (tok[0], tok[1], int(tok[2]), int(tok[3]) if tok[0] == "fwd" else 0)
        seen.setdefault(key, row)
    missing = {k: v for k, v in seen.items() if k not in have}
    assert not missing, f"planned but unwitnessed: {missing}"
    assert set(seen) == have, f"witnessed but never planned: {have - set(seen)}"


def test_a_misaligned_backward_launch_plans_to_the_generic_kernel(plan):
    "The one behaviour change of the plan: the vector backward kernels are no longer handed pointers they would access misaligned."
    rows = []
    for C in (64, 768):
        for xb, db in ((4, 4), (2, 2), (4, 2), (2, 4)):
            for name, need in (("x", 4 * xb), ("dy", 4 * db), ("dres", 4 * xb), ("dx", 4 * xb), ("twin", 8), ("gamma", 16)):
                if name == "twin" and xb == 2:
                    continue
                elem = {"x": xb, "dy": db, "dres": xb, "dx": xb, "twin": 2, "gamma": 4}[name]
                for a in (0, elem, need // 2, need):
                    row = dict(dir="bwd", rows=9, C=C, x_bytes=xb, dy_bytes=db, x=R.BASE, dy=R.BASE, dx=R.BASE, gamma=R.BASE,
                               dres=R.BASE if name == "dres" or C == 768 else 0, twin=R.BASE if name == "twin" else 0)
                    row[name] = R.BASE + a
                    rows.append((row, a % need == 0))
    for (row, aligned), line in zip(rows, plan([r for r, _ in rows])):
        vector = "wide" if row["C"] == 768 else "c64" if not row["dres"] and not row["twin"] else "generic"
        assert line.split()[1] == (vector if aligned else "generic"), (row, line)


def test_the_header_states_the_alignment_contract():
    text = " ".join(open(os.path.join(R.ROOT, "include", "uc_hip.h")).read().replace(" * ", " ").split())
    assert text.count("any element-aligned pointer; 16-byte alignment takes the vector kernels") == 2


# ------------------------------------------------------------------------------------------ the bound, without a GPU
_CACHE = {}


def _case(name, family):
    "Operands and reference of a witness, computed once and left unchanged."
    if (name, family) not in _CACHE:
        t = R.make_case(W[name], family, CPU, seed=R.NAMES.index(name))
        _CACHE[name, family] = (t, R.reference(W[name], t))
    return _CACHE[name, family]


def _store_code(w, o):
    return R.BF16 if o == "twin" else R.CODE[w["o"] if w["dir"] == "fwd" else w["x"]] if o in ("y", "dx") else R.F32


@pytest.mark.parametrize("name", R.SMALL)
def test_the_model_stays_at_or_under_half_the_bound(name):
    """float32, two-pass statistics, the stated expressions: in front of the store at or under half the bound with fp32's u_out; behind a
    bf16 store (one correct rounding, whose worst case IS u_out |ref|) inside the bound.  The operands lie between NaN, the reference of
    a constant row is beta."""
    w = W[name]
    for family in R.FAMILIES:
        t, ref = _case(name, family)
        assert bool(torch.isnan(t["x_buf"][:R.GUARD]).all()) and not bool(torch.isnan(t["x"]).any())
        if family == "const" and w["dir"] == "fwd":
            r = t["const_row"]
            assert float((ref["y"][0][r] - t["beta"].double()).abs().max()) <= 1e-9
        raw, got = R.model(w, t, store=False), R.model(w, t)
        for o in R.outputs(w):
            code = _store_code(w, o)
            front = R.ratio(raw[o], ref[o][0], R.unstored(*ref[o], code))
            behind = R.ratio(got[o], *ref[o])
            assert front[1] == 0 and front[0] <= 0.5, (name, family, o, front)
            assert behind[1] == 0 and behind[0] <= (0.5 if code == R.F32 else 1.0), (name, family, o, behind)


def pick(direction, kernel, **fields):
    "The one witness of the table with these fields."
    hits = [n for n in R.SMALL if W[n]["dir"] == direction and W[n]["kernel"] == kernel and all(W[n][k] == v for k, v in fields.items())]
    assert len(hits) == 1, (direction, kernel, fields, hits)
    return hits[0]


F_EXACT = [pick("fwd", "exact", nv=3, x="f", o="f", twin=1), pick("fwd", "exact", nv=8, x="b", o="b", twin=1), pick("fwd", "exact", nv=1, x="f", o="b", twin=1)]
F_VEC = [pick("fwd", "vec", C=2044, x="f", o="f"), pick("fwd", "vec", C=96, x="b", o="b"), pick("fwd", "vec", C=100, x="f", o="b")]
F_SCALAR = [pick("fwd", "scalar", C=2052, x="b", o="f"), pick("fwd", "scalar", C=67, x="f", o="f"), pick("fwd", "scalar", C=768, mis="twin", x="f", o="b")]
B_WIDE = [pick("bwd", "wide", nv=3, x="f", o="f", dres=1, twin=1, rows=13), pick("bwd", "wide", nv=8, x="b", o="b", dres=1, rows=13),
          pick("bwd", "wide", nv=1, x="f", o="b", dres=1, twin=0, rows=13)]
B_C64 = [pick("bwd", "c64", x="f", o="f", rows=18), pick("bwd", "c64", x="b", o="b", rows=3)]
B_GENERIC = [pick("bwd", "generic", C=2052, x="f", o="f"), pick("bwd", "generic", C=64, x="b", o="b", dres=1), pick("bwd", "generic", C=768, mis="dres", x="f")]
KERNELS = {"fwd exact": F_EXACT, "fwd vec": F_VEC, "fwd scalar": F_SCALAR, "bwd wide": B_WIDE, "bwd c64": B_C64, "bwd generic": B_GENERIC}
ALL = tuple(KERNELS)
FWD, BWD = ALL[:3], ALL[3:]
# defect -> (the kernels it belongs to, the input family that must show it).  The kernels:
#   last_vec_unwritten / last_vec_from_next_row   the store / the loads of a row's last 4-column vector (`(i * 64 + lane) * 4`, `c < C`)
#   inv_c_minus_1                                 `1.0f / (float)C`, `/ (float)C`, `1.0f / 64.0f`
#   eps_dropped                                   `rsqrtf(... + eps)`: only where the variance does not drown eps (tiny), or is zero (const)
#   gamma_shift4 / beta_shift4                    `gamma + (i * 64 + lane) * 4`, `gamma[c]`: the last four come from the NaN band
#   mean_from_full_chunks                         the partial chunk left out of the first sum; whole-chunk widths (exact, wide) have none
#   dres_not_added                                `if (dres)`; c64 takes no dres
#   s2_without_gamma                              `s2 += d * v` in front of `d *= g`
#   dgamma_missing_last_row                       the wave's last row left out of dg
#   twin_from_x                                   the twin packed from v[i] instead of o
DEFECT_CASES = {
    "last_vec_unwritten": (ALL, "wide"), "last_vec_from_next_row": (ALL, "wide"), "inv_c_minus_1": (ALL, "offset"), "eps_dropped": (ALL, "tiny"),
    "gamma_shift4": (ALL, "wide"), "beta_shift4": (FWD, "wide"), "mean_from_full_chunks": (("fwd vec", "fwd scalar", "bwd c64", "bwd generic"), "wide"),
    "dres_not_added": (("bwd wide", "bwd generic"), "wide"), "s2_without_gamma": (BWD, "wide"), "dgamma_missing_last_row": (BWD, "wide"),
    "twin_from_x": (FWD, "wide"),
}


def test_every_defect_is_planted_on_every_kernel_it_belongs_to():
    assert set(DEFECT_CASES) == set(R.DEFECTS)
    for d, (kernels, family) in DEFECT_CASES.items():
        assert {k.split()[0] for k in kernels} == set(R.DEFECTS[d]) and family in R.FAMILIES, d
    for k, names in KERNELS.items():
        assert all(f"{W[n]['dir']} {W[n]['kernel']}" == k for n in names)
    assert all(W[n]["twin"] for n in F_EXACT + F_VEC + F_SCALAR) and all(W[n]["dres"] for n in B_WIDE + B_GENERIC)


def _hits(name, family, defect):
    w = W[name]
    t, ref = _case(name, family)
    got = R.model(w, t, defect)
    return got, ref, {o: R.ratio(got[o], *ref[o]) for o in R.outputs(w) if R.ratio(got[o], *ref[o])[1] > 0}


@pytest.mark.parametrize("defect,kernel", [(d, k) for d, (kernels, _) in DEFECT_CASES.items() for k in kernels])
def test_a_planted_defect_leaves_the_bound_or_produces_a_nan(defect, kernel):
    "On EVERY chosen witness of the kernel (fp32 and bf16 streams, the widest and a narrow shape), not on one of them."
    family = DEFECT_CASES[defect][1]
    for name in KERNELS[kernel]:
        if defect == "mean_from_full_chunks" and W[name]["C"] % 256 == 0:
            continue      # the misaligned 768-wide witnesses have whole chunks only
        got, ref, hit = _hits(name, family, defect)
        print(f"defect [{defect}] on [{name}] ({family}): (err / bound, over, at) {hit}")
        assert hit, f"defect [{defect}] on [{name}] ({family}) stays inside the bound of every output"
        o = sorted(hit)[0]
        with pytest.raises(AssertionError, match=r"over the bound, worst err / bound .* at \(row \d+, col \d+\)"):
            R.check(R.route(W[name]), o, got[o], *ref[o])


def test_one_wrong_vector_is_named():
    "What a whole-tensor rel-L2 of 5e-3 lets through: the last 4-column vector of one 768-wide row 2 % off."
    name = pick("fwd", "exact", nv=3, x="f", o="b", twin=1)
    w = W[name]
    t, ref = _case(name, "wide")
    got = R.model(w, t)["y"].clone()
    got[2, -4:] = (got[2, -4:].float() * 1.02).bfloat16()
    assert float((got.double() - ref["y"][0]).norm() / ref["y"][0].norm()) < 5e-3
    with pytest.raises(AssertionError, match=r"elements over the bound, worst err / bound .* at \(row 2, col 76[4-7]\)"):
        R.check(R.route(w), "y", got, *ref["y"])
