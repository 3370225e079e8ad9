"""GPU: every route of GroupNorm (csrc/groupnorm.hip) and of the Cosmos tokenizer's streaming kernels (csrc/cosmos.hip) — the table of
tests/norm_stream_routes.py, checked on the CPU by tests/test_norm_stream_routes.py — is launched at its witness shapes through the C ABI on
buffers that are slices of larger ones, and every output element is compared with the fp64 reference under the derived bound.  Outputs
start as NaN between bands of a sentinel that must be untouched afterwards (the forward and the backward workspace, mean and rstd
included; the workspaces are sized by the `uc_*_ws_bytes` entry points' own answer), inputs lie between bands of NaN, no NaN may be left.
Every launch runs twice and the two results agree bit for bit (fixed-order reductions, no atomics).  Exact relations:
d2b(d2(x)) = x times the number of taps that read the pixel, hu(hp(x)) = x within the two bounds, the upsample is a pure copy (integer
views), padding columns are exactly 0.  Refusals (C % 8 != 0 under groups of 4, unsupported dtypes) leave every output untouched.
The worst err / bound per operation and output is printed by every test (`pytest -s`).

Measured on an MI355X: the 277 tests of this file take 4.7 s together (260 small witnesses on all their input families and 6 large ones
on two, 1050 launch pairs; 3 + 7 relation tests, 1 refusal test); the first test to touch the device takes 1.1 s, every other 0.2 s or less.
No element was over its bound, no band was written, every repeat agreed bit for bit, no kernel needed a change.  Largest err / bound over
the witnesses and families of each entry point, by the store's dtype, and for the fp32 outputs.  Behind a 16-bit store a correct result
reaches 0.99 by the one rounding of the store alone; the f32 column shows the arithmetic.  0.0000: bound 0, bit for bit.
                                   f32    bf16     f16     mean    rstd  dgamma   dbeta
  uc_group_norm_nhwc            0.1337  0.9918  0.9794   0.0950  0.3484       -       -
  uc_group_norm_silu_nhwc       0.1161  0.9919  0.9718   0.0431  0.3484       -       -
  uc_group_norm_nhwc_bwd        0.0332  0.9822  0.9285        -       -  0.1355  0.0741
  uc_group_norm_silu_nhwc_bwd   0.0286  0.9925  0.9599        -       -  0.0360  0.0335
  uc_haar_patch                 0.0655  0.9775  0.9660        (uc_haar_unpatch, fp32 image: 0.0770)
  uc_down2_gather_bwd           0.4042  0.9961  0.9993        (uc_down2_gather: 0.0000)
  uc_upsample2_nhwc_bwd         0.4151  0.9960  0.9980        (uc_upsample2_nhwc: 0.0000)
  uc_softmax_rows               0.3217  0.9880  0.9996
  uc_softmax_rows_bwd           0.0848  0.9864  0.9997
"""
import pytest
import torch

from tests import norm_stream_routes as R

pytestmark = pytest.mark.gpu

W = R.WITNESSES


@pytest.fixture(scope="module")
def lib():
    from uniception_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws_bytes(lib, w):
    fn = "uc_group_norm" + ("_silu" if w["act"] == "silu" else "") + "_nhwc" + ("_bwd" if w["op"] == "gnb" else "") + "_ws_bytes"
    return getattr(lib, fn)(w["B"], w["H"], w["W"], w["C"], w["G"])


def _run(lib, name):
    "Every family of the witness: status, bands, bit-equal repeat, zero elements over the bound, no NaN, padding exactly 0."
    w = W[name]
    dev = torch.device("cuda")
    if w["op"] in R.GN_OPS:      # the banded workspace has exactly the size the entry point asks for
        assert _ws_bytes(lib, w) == R.ws_elems(w) * 4, (name, _ws_bytes(lib, w), R.ws_elems(w) * 4)
    for family in R.families(w):
        rec = R.run_on_device(lib, w, family, dev)
        assert rec["status"] == 0, (name, family, rec["status"])
        assert rec["bands"], f"{name} ({family}): a guard band of {R.banded_outputs(w)} was written"
        assert rec["over"] == 0, rec["first"]
        assert rec["same"], f"{name} ({family}): two launches differ in their bits"
        for o, v in rec["got"].items():
            assert not bool(torch.isnan(v).any()), (name, family, o)
        if w["op"] in R.SM_OPS + ("hp",):
            o = R.outputs(w)[0]
            pad = rec["got"][o][:, (w["N"] if w["op"] in R.SM_OPS else 16 * w["C"]):]
            assert bool((pad == 0).all()), (name, family, "padding columns")
        print(f"{R.route(w):48s} {name:36s} {family:7s} " + " ".join(f"{o} {v:.4f}" for o, v in rec["worst"].items()))
    return rec


@pytest.mark.parametrize("name", R.SMALL)
def test_small_witness_is_inside_the_bound_per_element(lib, name):
    _run(lib, name)


@pytest.mark.parametrize("name", R.BIG)
def test_large_witness_is_inside_the_bound_per_element(lib, name):
    _run(lib, name)


@pytest.mark.parametrize("dt", "fbh")
def test_down2_adjoint_of_the_gather_weights_every_pixel_by_its_taps(lib, dt):
    "d2b(d2(x)) = x * (1 + [y even, y >= 2]) * (1 + [x even, x >= 2]): the sums of 1, 2 or 4 equal terms are exact in every dtype."
    for name in [n for n in R.SMALL if W[n]["op"] == "d2" and W[n]["dt"] == dt]:
        w = W[name]
        wb = W[name.replace("d2_", "d2b_", 1)]
        t = R.make_case(w, "wide", torch.device("cuda"), seed=R.seed_of(w))
        tb = R.make_case(wb, "wide", torch.device("cuda"), seed=R.seed_of(wb))
        assert R.launch(lib, w, t, _stream()) == 0
        assert R.launch(lib, wb, tb, _stream(), drows=t["rows"].data_ptr()) == 0
        torch.cuda.synchronize()
        y, x = torch.arange(w["H"], device="cuda").view(1, -1, 1, 1), torch.arange(w["W"], device="cuda").view(1, 1, -1, 1)
        weight = (1 + ((y % 2 == 0) & (y >= 2)).int()) * (1 + ((x % 2 == 0) & (x >= 2)).int())
        assert torch.equal(tb["dx"].double(), t["x"].double() * weight), name
        assert R.bands_ok(w, t) and R.bands_ok(wb, tb)


@pytest.mark.parametrize("name", [n for n in R.SMALL if W[n]["op"] == "hp"])
def test_haar_unpatch_of_the_patch_returns_the_image(lib, name):
    "hu(hp(x), 1 / scale) = x within the patch's bound carried through the inverse (16 coefficients, |1 / scale| each) plus the inverse's own."
    w = W[name]
    wu = W[name.replace("hp_", "hu_", 1)]
    dev = torch.device("cuda")
    for family in R.HS_FAMILIES:
        t, tu = R.make_case(w, family, dev, seed=R.seed_of(w)), R.make_case(wu, family, dev, seed=R.seed_of(wu))
        assert R.launch(lib, w, t, _stream()) == 0
        assert R.launch(lib, wu, tu, _stream(), rows=t["rows"].data_ptr(), scale=1.0 / w["scale"]) == 0
        torch.cuda.synchronize()
        bp = R.reference(w, t)["rows"][1][:, :16 * w["C"]].view(w["B"], w["H"] // 4, w["W"] // 4, 16, w["C"]).sum(3).permute(0, 3, 1, 2) / w["scale"]
        bu = R.reference(dict(wu, scale=1.0 / w["scale"]), dict(tu, rows=t["rows"]))["img"][1]
        bnd = bu + bp.repeat_interleave(4, 2).repeat_interleave(4, 3)
        R.check(f"{name} ({family}): hu(hp(x))", "img", tu["img"].reshape(-1, w["W"]), t["img"].double().reshape(-1, w["W"]), bnd.reshape(-1, w["W"]))
        assert R.bands_ok(wu, tu)


def _untouched(w, t):
    return all(bool(torch.isnan(t[o]).all()) for o in R.banded_outputs(w)) and R.bands_ok(w, t)


def test_the_shape_rule_and_the_dtype_check_refuse_without_a_launch(lib):
    dev = torch.device("cuda")
    for op in R.GN_OPS:      # groups of 4 with an odd G: C = 12 is no multiple of 8
        w = R._gn(op, "b", "silu", (16, 4, 5, 7))
        t = R.make_case(w, "wide", dev)
        assert R.launch(lib, w, t, _stream(), C=12, G=3) != 0
        torch.cuda.synchronize()
        assert _untouched(w, t), op
    for fn in ("uc_group_norm_nhwc_ws_bytes", "uc_group_norm_silu_nhwc_ws_bytes", "uc_group_norm_nhwc_bwd_ws_bytes", "uc_group_norm_silu_nhwc_bwd_ws_bytes"):
        assert getattr(lib, fn)(2, 5, 7, 12, 3) == 0, fn
    seen = set()
    for name in R.SMALL:      # an unsupported dtype on the first witness of every operation
        w = W[name]
        if w["op"] in seen:
            continue
        seen.add(w["op"])
        t = R.make_case(w, R.families(w)[0], dev, seed=R.seed_of(w))
        for bad in (3, -1):
            assert R.launch(lib, w, t, _stream(), dtype=bad) != 0, (name, bad)
        torch.cuda.synchronize()
        assert _untouched(w, t), name
    assert seen == set(R.OPS)
