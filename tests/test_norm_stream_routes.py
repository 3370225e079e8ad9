"""CPU: the GroupNorm / Cosmos stream route audit's own machinery (tests/norm_stream_routes.py) — the geometry every GroupNorm witness
claims is what tests/groupnorm_plan_driver.cpp prints over uniception_amd/csrc/groupnorm_plan.h, the workspace sizes are the formula worked
in Python, the shapes the one rule refuses are refused (C % 8 != 0 under groups of 4 included), no route of the table goes unwitnessed and
every witness group the module names is there, the per-element bound passes a float32 model of each kernel's index arithmetic at or under
half (in front of the store; behind a 16-bit store it is held to the bound itself), every planted defect leaves the bound, leaves a NaN,
writes a guard band or breaks an exact relation on a witness of its own operation in every (dtype, kernel), and the fp64 reference stays
in budget."""
import pytest
import torch

from tests import norm_stream_routes as R

CPU = torch.device("cpu")
W = R.WITNESSES


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("norm_stream_routes"))


def _group(op, **fields):
    return [w for w in W.values() if w["op"] == op and all(w.get(k) == v for k, v in fields.items())]


def _gn_shape(w):
    return (w["C"], w["G"], w["H"] * w["W"])


# ------------------------------------------------------------------------------------------ the plan and the table
def test_every_groupnorm_witness_has_the_geometry_it_claims_on_the_plan_driver(plan):
    names = [n for n in R.NAMES if W[n]["op"] in R.GN_OPS]
    for n, line in zip(names, plan([R.driver_row(W[n]) for n in names])):
        assert line == R.expected_plan(W[n]), f"{n}: the driver gives [{line}], the module works out [{R.expected_plan(W[n])}]"
    # the geometry in the docstring's brackets: (C, G, HW) -> the fields named there
    claims = {(8, 1, 1): dict(C8=1, rows=256), (8, 1, 7): dict(C8=1, rows=256),
              (48, 2, 43): dict(cg8=3, rows=42, dead=4, chunk=336, nchunk=1), (48, 2, 336): dict(chunk=336, nchunk=1), (48, 2, 337): dict(chunk=336, nchunk=2),
              (24, 3, 5): dict(rows=85, dead=1), (64, 2, 37 * 37): dict(nchunk=6, chunk=256), (256, 32, 23 * 29): dict(nchunk=11),
              (1600, 2, 9): dict(rows=1, dead=56, chunk=8, nchunk=2, cg8=100), (2048, 8, 523): dict(rows=1, nchunk=66, chunk=8, dead=0, C8=256),
              (128, 32, 20): dict(half=1, rows=16, chunk=128, nchunk=1), (128, 32, 129): dict(half=1, rows=16, chunk=128, nchunk=2), (8, 2, 3): dict(half=1, C8=1),
              (40, 10, 52): dict(half=1, rows=51, dead=1), (2048, 512, 11): dict(half=1, nchunk=2, G=512), (2048, 512, 523): dict(half=1, nchunk=66),
              (256, 32, 33): dict(cg8=1, half=0), (512, 32, 33): dict(cg8=2, half=0)}
    fields = ("C8", "cg8", "half", "rows", "chunk", "nchunk", "dead")
    for (C, G, HW), want in claims.items():
        ws = [w for w in W.values() if w["op"] in R.GN_OPS and _gn_shape(w) == (C, G, HW)]
        assert ws, (C, G, HW)
        w = ws[0]
        got = dict(zip(fields, map(int, plan([R.driver_row(w)])[0].split()[1:8])), G=G)
        assert all(got[k] == v for k, v in want.items()), ((C, G, HW), got, want)
    assert 523 - 65 * 8 == 3 and 37 * 37 - 5 * 256 == 89 and 52 - 51 == 1 and 43 - 42 == 1      # the last chunks and the second slots
    assert [len(range(q, 66, 4)) for q in range(4)] == [17, 17, 16, 16] and [len(range(q, 6, 4)) for q in range(4)] == [2, 2, 1, 1]
    assert R.geom(2048, 8, 523)["C"] == R.GN_MAX_C and R.geom(2048, 8, 523)["nchunk"] > 64 and R.geom(2048, 512, 11)["G"] > R.GN_THREADS


def test_the_workspace_sizes_are_the_formula(plan):
    rows = [(C, G, H, Wd, g4, B) for C, G, H, Wd, g4 in ((64, 2, 5, 7, 0), (128, 32, 8, 8, 1), (2048, 8, 1, 523, 0), (2048, 512, 1, 11, 1), (8, 1, 1, 1, 0)) for B in (1, 2, 5)]
    for (C, G, H, Wd, g4, B), line in zip(rows, plan(rows)):
        gm = R.geom(C, G, H * Wd)
        fwd, bwd = B * gm["nchunk"] * G * 8, (B * gm["nchunk"] * 2 * C + B * 2 * C + B * G * 2) * 4
        assert line.split()[-2:] == [str(fwd), str(bwd)], (C, G, H, Wd, B, line)
    for n in R.NAMES:      # what make_case sizes the banded workspace by
        w = W[n]
        if w["op"] in R.GN_OPS:
            assert R.ws_elems(w) * 4 == int(R.expected_plan(w).split()[-2 if w["op"] == "gn" else -1])


def test_the_one_shape_rule_refuses_what_no_kernel_can_take(plan):
    refused = [(12, 3, 5, 7, 1), (12, 3, 5, 7, 0), (20, 5, 4, 4, 1), (48, 4, 5, 7, 1), (48, 4, 5, 7, 0), (128, 32, 8, 8, 0), (64, 3, 5, 7, 1), (2056, 257, 2, 2, 1),
               (4096, 8, 2, 2, 0), (64, 2, 0, 7, 0), (64, 0, 5, 7, 0), (0, 1, 5, 7, 1), (64, 2, 1 << 16, 1 << 16, 0), (4, 1, 3, 3, 1)]
    taken = [(8, 2, 5, 7, 1), (128, 32, 8, 8, 1), (24, 3, 5, 7, 0), (2048, 512, 3, 3, 1), (2048, 1, 3, 3, 0), (8, 1, 1, 1, 1)]
    for row, line in zip(refused + taken, plan(refused + taken)):
        assert (line == "refused") == (row in refused), (row, line)
        C, G, H, Wd, g4 = row
        if H * Wd < 1 << 31:
            assert bool(R.gn_shape_ok(2, H, Wd, C, G, g4)) == (row in taken), row


def test_no_route_of_the_table_goes_unwitnessed():
    have = {R.route(w) for w in W.values()}
    missing = [r for r in R.required_routes() if r not in have]
    assert not missing, f"routes without a witness: {missing}"
    assert have == set(R.required_routes()), f"witnessed routes the table does not know: {have - set(R.required_routes())}"


def test_the_witness_table_is_what_the_module_says():
    plain = {(8, 1, 1), (8, 1, 7), (48, 2, 43), (48, 2, 336), (48, 2, 337), (24, 3, 5), (24, 1, 5), (64, 2, 1369), (256, 32, 667), (1600, 2, 9), (2048, 8, 523)}
    silu = {(128, 32, 20), (128, 32, 129), (8, 2, 3), (40, 10, 52), (2048, 512, 11), (2048, 512, 523), (256, 32, 33), (512, 32, 33)}
    for op in R.GN_OPS:
        for act in ("none", "relu"):
            assert {_gn_shape(w) for w in _group(op, act=act)} == plain, (op, act)
            assert {w["dt"] for w in _group(op, act=act)} == set("fbh")
            assert [w["B"] for w in _group(op, act=act) if w["B"] != 2] == [3]
        assert {_gn_shape(w) for w in _group(op, act="silu")} == silu and {w["dt"] for w in _group(op, act="silu")} == set("fbh")
        assert {_gn_shape(w) for w in _group(op, big=True)} == {(2048, 8, 523), (2048, 512, 523)}
        assert [w["dt"] for w in _group(op, big=True, act="silu")] == ["b"]
    for w in W.values():
        if w["op"] in R.GN_OPS and w["H"] * w["W"] not in (1, 3, 5, 7, 11, 43, 337, 523):      # a real factorisation with an odd W where HW is no prime
            assert w["H"] > 1 and w["W"] > 1 and w["W"] % 2 == 1, w["name"]
    assert max(w["B"] * w["H"] * w["W"] * w["C"] for w in W.values() if w["op"] in R.GN_OPS) == 2 * 523 * 2048
    for op in R.HAAR_OPS:
        assert {(w["B"], w["C"], w["H"], w["W"], w["ld"]) for w in _group(op)} == {(2, 3, 4, 4, 48), (2, 3, 8, 12, 64), (1, 1, 4, 8, 16), (2, 5, 12, 20, 80), (2, 3, 36, 20, 48)}
        assert {w["dt"] for w in _group(op, ld=64)} == set("fbh") and {w["scale"] for w in _group(op)} == {1.0, 16.0, 1.0 / 16.0}
        assert 2 * 3 * 9 * 5 == 270 > 256
    for dt in "fbh":
        for op in R.MOVE_OPS:
            want = {(1, 2, 2, 8), (2, 4, 6, 24), (2, 10, 6, 64)} | ({(1, 1, 1, 8), (2, 3, 5, 16)} if op in ("up", "upb") else set())
            assert {(w["B"], w["H"], w["W"], w["C"]) for w in _group(op, dt=dt)} == want, (op, dt)
        for op in R.SM_OPS:
            g = _group(op, dt=dt)
            assert {w["rows"] for w in g} == {3} and {round(w["scale"], 6) for w in g} == {round(512.0 ** -0.5, 6), 1.0}
            assert {w["N"] for w in g if w["lds"] == w["N"] and not w["mis"]} == set(R.SM_N) | {6153}
            assert {(w["N"], w["ldp"]) for w in g if w["lds"] > w["N"]} == {(N, -(-N // 64) * 64) for N in R.SM_N if N % 64} | {(4090, 4160)}
            assert {w["N"] for w in g if w["lds"] == w["N"] and w["N"] % 64 == 0} >= {2048, 4096}
            assert [(w["N"], w["mis"] * R.BYTES[dt]) for w in g if w["mis"]] == [(16, 4)]
    assert (R.SM_REGS, R.SM_LAP) == (4096, 2048) and len({round(s, 6) for s in R.SM_SCALES}) == 2


def test_the_reference_stays_inside_its_budget():
    for n in R.NAMES:
        assert R.reference_elems(W[n]) <= R.REF_BUDGET_ELEMS, n


# ------------------------------------------------------------------------------------------ the bound, without a GPU
_CACHE = {}


def _case(name, family):
    "Operands and reference of a witness, computed once and left unchanged."
    if (name, family) not in _CACHE:
        t = R.make_case(W[name], family, CPU, seed=R.seed_of(W[name]))
        _CACHE[name, family] = (t, R.reference(W[name], t), R.reference(W[name], t, front=True))
    return _CACHE[name, family]


def _exact_relations(w, t, got):
    "The relations a launch must meet exactly; the names of those it breaks."
    broken = []
    if w["op"] in R.BITS:
        src = t["x"]
        want = (src.repeat_interleave(2, 1).repeat_interleave(2, 2) if w["op"] == "up" else R.reference(w, t)[R.outputs(w)[0]][0].to(src.dtype))
        if not torch.equal(got[R.outputs(w)[0]].view(R.INTV[w["dt"]]).flatten(), want.contiguous().view(R.INTV[w["dt"]]).flatten()):
            broken.append("a pure move does not return the input's bits")
    if w["op"] in R.SM_OPS + ("hp",):
        o = R.outputs(w)[0]
        first = w["N"] if w["op"] in R.SM_OPS else 16 * w["C"]
        pad = got[o][:, first:]
        if pad.numel() and not bool((pad == 0).all()):
            broken.append("the padding columns are not exactly 0")
    if w["op"] == "gnb" and w["act"] == "relu" and bool((t["gate"] <= 0).view(w["B"], -1, w["G"], w["C"] // w["G"]).all(3).all(1).any()):
        dead = (t["gate"] <= 0).view(w["B"], -1, w["G"], w["C"] // w["G"]).all(3, keepdim=True).all(1, keepdim=True).expand(w["B"], w["H"] * w["W"], w["G"], w["C"] // w["G"])
        if bool((got["dx"].view(dead.shape)[dead] != 0).any()):
            broken.append("dx is not exactly 0 in a group whose gate is closed")
    return broken


@pytest.mark.parametrize("op", R.OPS)
def test_the_model_stays_at_or_under_half_the_bound(op):
    """In front of an fp32-class store at or under half the bound; behind a 16-bit store (one correct rounding, whose worst case IS
    u_out |ref|) inside the bound; the bands untouched, no NaN left, the exact relations met."""
    for name in [n for n in R.NAMES if W[n]["op"] == op]:
        w = W[name]
        for family in R.families(w):
            t, ref, front_ref = _case(name, family)
            raw_b, got_b = R.model(w, t, store=False), R.model(w, t)
            assert R.bands_ok(w, t, raw_b) and R.bands_ok(w, t, got_b), (name, family)
            raw, got = R.results(w, t, raw_b), R.results(w, t, got_b)
            assert not _exact_relations(w, t, got), (name, family, _exact_relations(w, t, got))
            for o in R.outputs(w):
                code = R.store_code(w, o)
                front = R.ratio(raw[o], *front_ref[o])
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
                R.check(R.route(w), o, *(v.reshape(-1, v.shape[-1]) for v in (got[o],) + tuple(ref[o])))
            return f"{o}: {bad} elements over the bound or NaN, worst err / bound {worst:.3g}"
    broken = _exact_relations(w, t, got)
    return broken[0] if broken else None


def _applies(defect, w):
    "The witnesses on which the defect changes what the kernel does at all."
    op = w["op"]
    if op in R.GN_OPS:
        gm = R.gn_geom_of(w)
        ragged = gm["HW"] % gm["chunk"] != 0
        return {"last_chunk_count_full": ragged, "chan_counts_equal": ragged, "dead_thread_counted": gm["dead"] > 0 and gm["HW"] > gm["rows"],
                "half_groups_swapped": bool(gm["half"]), "group_from_c8_mod": not gm["half"] and w["G"] > 1,
                "finalize_second_lap_dropped": gm["nchunk"] > 64, "group_loop_stops_at_256": bool(gm["half"]) and w["G"] > 256,
                "bwd_chain_tail_dropped": gm["nchunk"] % 4 != 0, "sample_sum_skips_last": True, "inv_m_from_C": w["G"] > 1,
                "relu_gate_ge_zero": w["act"] == "relu", "silu_grad_without_z_term": w["act"] == "silu", "eps_outside_sqrt": True,
                "stats_of_previous_sample": True}[defect]
    if defect == "haar_pad_unwritten":
        return w["ld"] > 16 * w["C"]
    if op in R.SM_OPS:
        if defect in ("sm_tail_left_out_of_max", "sm_tail_left_out_of_sum", "smb_dot_without_tail"):
            return w["N"] > R.SM_REGS
        if defect == "sm_pad_columns_unwritten":
            return w["ldp"] > w["N"]
        if defect == "sm_fill_zero_in_max":
            return w["N"] % 8 != 0
        if defect == "sm_scale_after_max":
            return w["scale"] != 1.0
    return True


def _kernels(defect, op):
    "The (dtype, kernel) pairs of the operation on each of which the defect has to be caught."
    out = {}
    for n in R.NAMES:
        w = W[n]
        if w["op"] == op and _applies(defect, w):
            key = (w["dt"],) + ((R.gn_kernel(w), w["act"]) if op in R.GN_OPS else ("vec" if R.sm_vec(w) else "scalar",) if op in R.SM_OPS else ())
            out.setdefault(key, []).append(n)
    return out


@pytest.mark.parametrize("defect,op", [(d, op) for d, ops in R.DEFECTS.items() for op in ops])
def test_a_planted_defect_is_caught_by_a_witness_of_its_operation(defect, op):
    "On every (dtype, kernel) of the operation the defect can sit in: over the bound, a NaN left, a band written or an exact relation broken."
    groups = _kernels(defect, op)
    assert groups, (defect, op)
    for key, names in groups.items():
        hit = None
        for name in sorted(names, key=lambda n: W[n]["big"]):
            for family in R.families(W[name]):
                t, ref, _ = _case(name, family)
                why = _caught(W[name], t, ref, defect)
                if why:
                    hit = (name, family, why)
                    break
            if hit:
                break
        assert hit, f"defect [{defect}] stays unseen on every witness of {op} {key}: {names}"
        print(f"defect [{defect}] on {op} {key}: first caught by [{hit[0]}] ({hit[1]}): {hit[2]}")


def _rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def test_one_wrong_channel_vector_is_named():
    "What a whole-tensor rel-L2 of 8e-3 lets through: one channel vector of one pixel 3 % off in a bf16 GroupNorm output."
    name = "gn_b_none_c48g2_1x337"
    w = W[name]
    t, ref, _ = _case(name, "wide")
    got = R.results(w, t, R.model(w, t))["y"].clone()
    got[1, 200, 16:24] = (got[1, 200, 16:24].float() * 1.03).bfloat16()
    r, b = ref["y"]
    assert _rel_l2(got, r) < 8e-3
    with pytest.raises(AssertionError, match=r"elements over the bound, worst err / bound .* at \(row 537, col (1[6-9]|2[0-3])\)"):
        R.check(R.route(w), "y", got.reshape(-1, 48), r.reshape(-1, 48), b.reshape(-1, 48))


def test_swapped_halves_hide_from_rel_l2_on_iid_inputs_and_fail_on_steps():
    """The iid blind spot: with the two groups of a channel vector exchanged an N(0.5, 3^2) map moves by about sqrt(2 / M) in rel-L2
    (M = HW cg elements per group), `steps` by more than its own norm.  At the witness (128, 32, 129), M = 516, that is 8.3e-2 on `wide` (so
    NOT under the 8e-3 gate at this small shape: the gate goes blind from M of about 3e4 on) against 9.5 on `steps`;
    at M = 132096 (C = 8, G = 2, 256 x 129) the swapped map passes the gate at 5e-3.  The per-element bound names the defect on all three."""
    name = "gn_b_silu_c128g32_3x43"
    w = W[name]
    assert R.gn_geom_of(w)["half"] and (w["C"], w["G"], w["H"] * w["W"]) == (128, 32, 129)
    seen = {}
    for family in ("wide", "steps"):
        t, ref, _ = _case(name, family)
        got = R.results(w, t, R.model(w, t, "half_groups_swapped"))["y"]
        seen[family] = _rel_l2(got, ref["y"][0])
        assert _rel_l2(R.results(w, t, R.model(w, t))["y"], ref["y"][0]) < 8e-3      # the gate passes the correct kernel
        with pytest.raises(AssertionError, match="elements over the bound"):
            R.check(R.route(w), "y", got.reshape(-1, 128), *(v.reshape(-1, 128) for v in ref["y"]))
    print(f"swapped halves at (128, 32, 129): rel-L2 {seen['wide']:.3g} on wide, {seen['steps']:.3g} on steps")
    assert seen["wide"] < 4.0 * (2.0 / 516) ** 0.5 and seen["steps"] > 1.0 and seen["steps"] > 50 * seen["wide"]
    big = R._gn("gn", "b", "silu", (8, 2, 256, 129))      # the same route on a map large enough for the gate to go blind
    t = R.make_case(big, "wide", CPU, seed=1)
    ref = R.reference(big, t)["y"]
    got = R.results(big, t, R.model(big, t, "half_groups_swapped"))["y"]
    print(f"swapped halves at (8, 2, 256 x 129): rel-L2 {_rel_l2(got, ref[0]):.3g} on wide")
    assert _rel_l2(got, ref[0]) < 8e-3
    with pytest.raises(AssertionError, match="elements over the bound"):
        R.check(R.route(big), "y", got.reshape(-1, 8), *(v.reshape(-1, 8) for v in ref))
