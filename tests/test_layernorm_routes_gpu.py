"""GPU: every LayerNorm route (tests/layernorm_routes.py, checked on the CPU by tests/test_layernorm_routes.py) is launched at its witness
shape through the C ABI (uc_layernorm_twin / uc_layernorm_bwd) on buffers that are slices of larger ones, proven to have taken its kernel —
the pointers the launch really got go to the plan driver — and every element of y, the twin, dx, dx_bf16, dgamma and dbeta is compared with
the fp64 reference under the derived bound.  Outputs start as NaN between bands of a sentinel that must be untouched afterwards, inputs lie
between bands of NaN, dgamma / dbeta start at a non-zero prefill (`+=`).  Exact relations: the twin is y.bfloat16() bit for bit (y itself
when y is bf16), dx_bf16 is dx.bfloat16().  dgamma / dbeta come from atomics: their bits are not asserted.  References run on the device
in torch's fp64, those of the non-temporal witnesses in row chunks.

Measured on an MI355X: the 346 tests of this file take 5.1 s together (309 small witnesses with four input families each, 14 non-temporal
launches, 16 other big witnesses, 7 argument tests); the first test to touch the device takes 0.9 s, every other test 0.01 s or less, each
non-temporal launch with its chunked fp64 reference included, so the non-temporal group stays whole.  The 365 tests of the CPU file take 11 s.
Largest err / bound over the witnesses and input families of each (direction, kernel, nv), by output and store dtype.  Behind a bf16 store
a correct result reaches 0.99 by the one rounding of the store alone (u_out = 2^-8 is exactly its worst case, tests/layernorm_routes.py);
the fp32 columns show the arithmetic.  No witness was over the bound, none needed a change of the kernels.
                          y/f32    y/bf16    dx/f32   dx/bf16 twin/bf16    dgamma     dbeta
  fwd exact nv1          0.0229    0.9845         -         -    0.9845         -         -
  fwd exact nv2          0.0196    0.9859         -         -    0.9833         -         -
  fwd exact nv3          0.0222    0.9917         -         -    0.9908         -         -
  fwd exact nv4          0.0137    0.9908         -         -    0.9922         -         -
  fwd exact nv6          0.0108    0.9880         -         -    0.9880         -         -
  fwd exact nv8          0.0099    0.9870         -         -    0.9871         -         -
  fwd vec                0.1241    0.9905         -         -    0.9912         -         -
  fwd scalar             0.0680    0.9874         -         -    0.9898         -         -
  fwd exact nv1 nt       0.1598    0.9942         -         -         -         -         -      (0.1598: bf16 x, C = 256, 262145 rows)
  fwd exact nv2 nt       0.0321    0.9934         -         -         -         -         -
  fwd exact nv3 nt       0.0213    0.9928         -         -         -         -         -
  fwd exact nv4 nt       0.0166    0.9922         -         -         -         -         -
  fwd exact nv6 nt       0.0148    0.9914         -         -         -         -         -
  fwd exact nv8 nt       0.0123    0.9906         -         -         -         -         -
  bwd wide nv1                -         -    0.0165    0.9874    0.9899    0.1131    0.1241
  bwd wide nv2                -         -    0.0140    0.9902    0.9916    0.1213    0.1214
  bwd wide nv3                -         -    0.0128    0.9854    0.9865    0.1099    0.1238
  bwd wide nv4                -         -    0.0112    0.9838    0.9886    0.1095    0.1240
  bwd wide nv6                -         -    0.0092    0.9886    0.9858    0.1134    0.1240
  bwd wide nv8                -         -    0.0081    0.9827    0.9888    0.1128    0.1224
  bwd c64                     -         -    0.0405    0.9865         -    0.0900    0.1370
  bwd generic                 -         -    0.0357    0.9879    0.9909    0.1226    0.1414
  bwd wide, cap rows          -         -    0.0169    0.9920    0.9929    0.0020    0.0022      (rows = 2051 and 4101, every nv)
  bwd c64, 16391 rows         -         -    0.0446    0.9943         -    0.0003    0.0005
"""
import pytest
import torch

from tests import layernorm_routes as R

pytestmark = pytest.mark.gpu

W = R.WITNESSES
CHUNK_ELEMS = 1 << 22      # fp64 reference of a big forward witness: this many elements at a time


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("layernorm_routes_gpu"))


def _ptr(t, name):
    return t[name].data_ptr() if name in t else None


def _launch(w, t, rows=None, x_code=None, o_code=None):
    "One call of the entry point on the case's buffers; the status."
    from uniception_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rows = w["rows"] if rows is None else rows
    xc = R.CODE[w["x"]] if x_code is None else x_code
    oc = R.CODE[w["o"]] if o_code is None else o_code
    if w["dir"] == "fwd":
        return lib.uc_layernorm_twin(_ptr(t, "x"), xc, _ptr(t, "gamma"), _ptr(t, "beta"), _ptr(t, "y"), oc, _ptr(t, "twin"), rows, w["C"], R.EPS, st)
    return lib.uc_layernorm_bwd(_ptr(t, "x"), xc, _ptr(t, "gamma"), _ptr(t, "dy"), oc, _ptr(t, "dres"), _ptr(t, "dx"), _ptr(t, "twin"),
                                _ptr(t, "dgamma"), _ptr(t, "dbeta"), rows, w["C"], R.EPS, st)


def _output_buffers(w):
    return ("y", "twin")[:1 + w["twin"]] if w["dir"] == "fwd" else ("dx",) + (("twin",) if w["twin"] else ()) + ("dgamma", "dbeta")


def _assert_nothing_written(w, t, label):
    for o in _output_buffers(w):
        assert R.bands_untouched(t[o + "_buf"], t[o + "_at"], t[o].numel()), f"[{label}]: the guard band around {o} was written"
    for o in _output_buffers(w):
        if o in ("dgamma", "dbeta"):
            assert torch.equal(t[o], t["pre_g" if o == "dgamma" else "pre_b"]), f"[{label}]: {o} was written"
        else:
            assert bool(torch.isnan(t[o]).all()), f"[{label}]: {o} was written"


def _bits(a):
    return a.view(torch.int16)


def _run(w, families, gpu, plan):
    "Launch the witness on every input family and check everything."
    cases = [R.make_case(w, f, gpu, seed=R.NAMES.index(w["name"])) for f in families]
    # the launches take the route: the pointers they get -> the plan driver
    lines = plan([R.driver_row(w, {n: t[n].data_ptr() for n in ("x", "y", "twin", "gamma", "beta", "dy", "dres", "dx") if n in t}) for t in cases])
    for family, t, line in zip(families, cases, lines):
        label = f"{w['name']} ({family}): {R.route(w)}"
        assert line == R.expected_plan(w), f"[{label}]: the launch takes [{line}], the witness stands for [{R.expected_plan(w)}]"
        rc = _launch(w, t)
        torch.cuda.synchronize()
        assert rc == 0, f"[{label}]: status {rc}"
        _check(w, family, t, label)


def _check(w, family, t, label):
    "Everything a finished launch left in the case's buffers; {output: largest err / bound}."
    for o in _output_buffers(w):
        assert R.bands_untouched(t[o + "_buf"], t[o + "_at"], t[o].numel()), f"[{label}]: the guard band around {o} was written"
    got = R.results(w, t)
    worst = {}
    rows, C = w["rows"], w["C"]
    if w["dir"] == "fwd":
        step = max(1, CHUNK_ELEMS // C)
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            ref = R.reference_fwd(w, t["x"][r0:r1], t["gamma"], t["beta"])
            for o in R.outputs(w):
                worst[o] = max(worst.get(o, 0.0), R.check(label + (f" rows {r0}.." if r0 else ""), o, got[o][r0:r1], *ref[o]))
            if t["const_row"] is not None and r0 <= t["const_row"] < r1:      # a constant row gives beta
                r = t["const_row"] - r0
                assert bool(((t["y"][t["const_row"]].double() - t["beta"].double()).abs() <= ref["y"][1][r] + 1e-9).all()), f"[{label}]: constant row"
    else:
        ref = R.reference_bwd(w, t)
        for o in R.outputs(w):
            worst[o] = R.check(label, o, got[o], *ref[o])
    if w["twin"]:      # the bf16 copy is the same value rounded once
        main = t["y"] if w["dir"] == "fwd" else t["dx"]
        same = torch.equal(_bits(t["twin"]), _bits(main.bfloat16()))
        assert same, f"[{label}]: {int((_bits(t['twin']) != _bits(main.bfloat16())).sum())} twin elements are not the bf16 rounding of their fp32 value"
    print(f"LNROUTE {w['name']} {family} [{R.route(w)}] " + " ".join(f"{o}={v:.4f}" for o, v in worst.items()))
    return worst


@pytest.mark.parametrize("name", R.SMALL)
def test_small_witness_against_fp64(gpu, plan, name):
    _run(W[name], R.FAMILIES, gpu, plan)


@pytest.mark.parametrize("name", R.BIG)
def test_big_witness_against_fp64(gpu, plan, name):
    """The non-temporal forward launches (above 128 MiB of x), the backward row counts at which the waves of the wide kernel take a second
    and a third software-pipelined row, and the second grid-stride iteration of the C = 64 kernel."""
    _run(W[name], ("wide",), gpu, plan)


@pytest.mark.parametrize("name", ["f_exact3_ff_t1_r9_c768", "f_vec_ff_t1_r5_c2044", "f_scalar_ff_t1_r5_c67", "b_wide3_ff_d1_t1_r13_c768", "b_c64_ff_d0_t0_r18_c64",
                                  "b_generic_ff_d1_t0_r9_c2052"])
def test_zero_rows_return_ok_and_write_nothing(gpu, name):
    w = W[name]
    t = R.make_case(w, "wide", gpu)
    assert _launch(w, t, rows=0) == 0
    torch.cuda.synchronize()
    _assert_nothing_written(w, t, name)


def test_unsupported_dtypes_are_refused_without_a_launch(gpu):
    from uniception_amd import _lib
    lib = _lib.load()
    F16 = 2
    w = W["f_exact3_ff_t1_r9_c768"]
    t = R.make_case(w, "wide", gpu)
    for xc, oc in ((F16, R.F32), (R.F32, F16), (F16, F16), (7, R.BF16)):
        assert _launch(w, t, x_code=xc, o_code=oc) == -1
        assert f"uc_layernorm: unsupported dtypes {xc} -> {oc}" in lib.uc_last_error().decode()
    torch.cuda.synchronize()
    _assert_nothing_written(w, t, w["name"])
    w = W["b_wide3_ff_d1_t1_r13_c768"]
    t = R.make_case(w, "wide", gpu)
    assert _launch(w, t, o_code=F16) == -1 and "uc_layernorm_bwd: bad dy dtype 2" in lib.uc_last_error().decode()
    assert _launch(w, t, x_code=F16) == -1 and "uc_layernorm_bwd: bad x dtype 2" in lib.uc_last_error().decode()
    assert _launch(w, t, x_code=R.BF16) == -1 and "dx_bf16 must be NULL" in lib.uc_last_error().decode()      # a bf16 stream has no twin
    torch.cuda.synchronize()
    _assert_nothing_written(w, t, w["name"])
