"""GPU: every uc_gemm route the bench launches (tests/golden/gemm_route_witnesses.json, derived and checked on the CPU by
tests/test_gemm_routes.py) is launched at its witness shape through ops.gemm, proven to have taken that route — the uc_gemm_desc the
wrapper passed goes to the plan driver with the device's CU count and the live knobs — and compared element by element with the fp64
reference under the derived bound (tests/gemm_routes.py).  References run on the device in torch's fp64 matmul, in row chunks."""
import ctypes

import pytest
import torch

from tests import gemm_routes as R

pytestmark = pytest.mark.gpu

WITNESSES = R.load_witnesses()
CASES = [("routes", s) for s in WITNESSES["routes"]] + [("nt", s) for s in WITNESSES["nt"]]
GUARD = 8          # sentinel rows behind every output this file allocates
KNOBS = ("gemm_variant", "small_m_split", "gemm_stagger", "conv_rows", "conv_rows_flat", "gemm_group_m", "gemm_4wave")
DRIVER_FIELDS = set("""compute_dtype a_mode relu_a lda M N K conv_B conv_H conv_W conv_Cin conv_stride conv_Ho conv_Wo act res_dtype ldr
    rope_cols rope_npos vt_col0 vt_ntok vt_npad split_k dact_act out_dtype ldc ldt ln_nblk A W bias residual residual2 rope_pos rope_table
    vt_out preact_out dact_u C twin_out stats_out ln_stats ln_colsum tail_w tail_b tail_out fuse_ws sat_flag""".split())


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("gemm_routes_gpu"))


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _launch(ops, row, t, dev):
    "One ops.gemm call for the witness; returns {name: output}, the guard bands and the captured descriptor rows."
    from uniception_amd import _lib
    M, N = row["M"], row["N"]
    kw = {}
    if row.get("a_mode", 0) == 1:
        kw["conv"] = (row["conv_B"], row["conv_H"], row["conv_W"], row["conv_Cin"], row["conv_stride"])
    kw["bias"] = t.get("bias")
    kw["act"] = {0: None, 1: "gelu", 2: "relu"}[row.get("act", 0)]
    kw["residual"], kw["residual2"] = t.get("residual"), t.get("residual2")
    kw["relu_a"] = bool(row.get("relu_a"))
    guards = {}
    outs = {}
    out_dt = R.TORCH_DT[row.get("out_dtype", 0)]
    if row.get("tail_out"):
        kw["tail"] = (t["tail_w"], t.get("tail_b"))
    else:
        n_out = row["vt_col0"] if row.get("vt_col0", -1) >= 0 else N
        cbuf = _nan((M + GUARD, n_out), out_dt, dev)
        kw["out"] = cbuf[:M]
        guards["C"] = cbuf[M:]
        if row.get("preact_out"):
            pbuf = _nan((M + GUARD, n_out), out_dt, dev)
            kw["preact_out"] = pbuf[:M]
            guards["preact"], outs["preact"] = pbuf[M:], pbuf[:M]
    if row.get("rope_cols"):
        kw["rope"] = (t["rope_pos"], ops.rope_table(dev, 64, R.ROPE_BASE), row["rope_cols"])
    if row.get("vt_col0", -1) >= 0:
        heads, ntok, npad = (N - row["vt_col0"]) // 64, row["vt_ntok"], row["vt_npad"]
        n = (M // ntok) * heads * 64 * npad
        vbuf = _nan((n + 64 * GUARD,), torch.bfloat16, dev)
        outs["vt_raw"] = vbuf[:n].view(M // ntok, heads, 64, npad)
        guards["vt"] = vbuf[n:]
        kw["vt"] = (row["vt_col0"], outs["vt_raw"], ntok)
    if row.get("dact_u"):
        kw["dact"] = (t["dact_u"], {1: "gelu", 2: "relu"}[row["dact_act"]])
    if row.get("ln_stats"):
        st = ops.LnPartial(t["ln_stats"], R.LN_EPS) if row.get("ln_nblk", 0) > 0 else t["ln_stats"]
        kw["ln"] = (st, t["ln_colsum"])
    kw["emit_ln"] = bool(row.get("stats_out"))

    lib = _lib.load()
    real = lib.uc_gemm
    captured = []

    def spy(desc_ref, stream):
        d = desc_ref._obj
        rec = {}
        for name, _ in d._fields_:
            v = getattr(d, name)
            if name in DRIVER_FIELDS:
                rec[name] = int(v or 0)
        rec["ln_eps"] = float(d.ln_eps)
        captured.append(rec)
        return real(desc_ref, stream)

    flag = ops.f16_sat_flag()
    flag.zero_()
    lib.uc_gemm = spy
    try:
        res = ops.gemm(t["A"], t["W"], **kw)
    finally:
        lib.uc_gemm = real
    torch.cuda.synchronize()
    if row.get("tail_out"):
        outs["tail"] = res
    else:
        outs["C"] = res
        if row.get("stats_out"):
            outs["stats"] = res.uc_ln.partial
    if "vt_raw" in outs:
        outs["vt"] = R.unpack_vt(outs["vt_raw"], row)
    return outs, guards, captured, int(flag.item())


def _live_knobs(ops):
    from uniception_amd._lib import UcHipError
    knobs = {"cus": torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count}
    for k in KNOBS:
        try:
            knobs[k] = ops.tuning_get(k)
        except UcHipError:
            pass      # not switchable at run time: the driver's default is the library's
    return knobs


def _compare(label, row, t, outs, guards, tile):
    ref = R.reference(row, t)
    for name, (r, b) in ref.items():
        R.check(label, name, outs[name], r, b, tile)
    if row.get("stats_out"):
        r, b = R.stats_reference(outs["C"])
        R.check(label, "stats", outs["stats"], r, b, tile)
    for name, gd in guards.items():
        assert bool(torch.isnan(gd).all()), f"route [{label}]: the guard band behind {name} was written"


TILE_ORDER = R.load_tile_order()


@pytest.mark.parametrize("kernel", sorted(TILE_ORDER))
def test_tile_order_with_a_ragged_last_tile_group(gpu, plan, kernel):
    """Six row tiles with group_m = 4 — a full tile group and a ragged one of two — on every direct-to-LDS kernel, two or more column
    tiles: every output element against fp64.  C starts as NaN: a tile never written, or written from another tile's place, fails."""
    from uniception_amd import ops
    row = TILE_ORDER[kernel]
    for k in KNOBS:
        if k in row:
            ops.tuning_set(k, row[k])           # (reset after every test: conftest.py)
    t = R.make_operands(row, gpu, seed=200 + sorted(TILE_ORDER).index(kernel))
    outs, guards, captured, sat = _launch(ops, row, t, gpu)
    assert len(captured) == 1
    knobs = _live_knobs(ops)
    line = plan([{**captured[0], **knobs}])[0]
    p = dict(zip(R.PLAN_FIELDS, line.split()))
    assert p["kernel"] == kernel and int(p["tiles_m"]) == 6 and int(p["tiles_n"]) >= 2, line
    assert knobs.get("gemm_group_m", 4) == 4 and sat == 0
    _compare("tile order " + kernel, row, t, outs, guards, R.TILE[kernel])


@pytest.mark.parametrize("part,label", CASES, ids=[f"{p}-{i:02d}-{s.replace(' ', '_')}" for i, (p, s) in enumerate(CASES)])
def test_route_against_fp64(gpu, plan, part, label):
    from uniception_amd import ops
    row = WITNESSES[part][label]
    seed = CASES.index((part, label))
    t = R.make_operands(row, gpu, seed=seed)
    outs, guards, captured, sat = _launch(ops, row, t, gpu)
    # the launch took the route: the descriptor the wrapper passed, the device's CUs, the live knobs -> the plan driver
    assert len(captured) == 1
    line = plan([{**captured[0], **_live_knobs(ops)}])[0]
    got_sig = R.signature(captured[0], line)
    want_sig = label if part == "routes" else R.signature(row, plan([row])[0])
    assert got_sig == want_sig, f"the launch took [{got_sig}] ({line}), the witness stands for [{want_sig}]"
    if part == "nt":
        assert R.nt_combo(captured[0], line) == label, line
    tile = R.TILE[line.split()[0]]
    assert sat == 0, "sat_flag raised by a launch that stays in range"
    _compare(label, row, t, outs, guards, tile)
    if row["compute_dtype"] == R.F16 and row.get("out_dtype", 0) == R.F16 and not row.get("tail_out") and part == "routes":
        # a few elements driven past the fp16 range: stored saturated at +-65504, and reported
        del outs, guards
        t = R.make_operands(row, gpu, seed=seed, saturate=True)
        outs, guards, captured, sat = _launch(ops, row, t, gpu)
        assert R.signature(captured[0], plan([{**captured[0], **_live_knobs(ops)}])[0]) == want_sig
        assert int((outs["C"].float().abs() == 65504).sum()) > 0
        assert sat == 1, "values beyond the fp16 range were stored, sat_flag stayed 0"
        _compare(label + " (saturating)", row, t, outs, guards, tile)
