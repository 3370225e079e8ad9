"""GPU: every route of the DPT / MoGe heads' streaming kernels (tests/head_stream_routes.py, checked on the CPU by
tests/test_head_stream_routes.py) is launched at its witness shapes through the C ABI on buffers that are slices of larger ones, proven to
have taken its kernel — the pointers the launch really got go to the plan driver — and every output element is compared with the fp64
reference under the derived bound.  Outputs start as NaN between bands of a sentinel that must be untouched afterwards, inputs lie between
bands of NaN, dw / db start at a non-zero prefill (`+=`; their bits are not asserted: atomics).  Exact relations: a cropped bilinear launch
is the top-left window of the uncropped one, uc_resize_bilinear_nhwc(align_corners = 1) is uc_bilinear_nhwc (and the adjoints), an identity
resize returns the input's bits, gather(scatter(x)) = x, dfeat is exactly 0 under the mask, the pad adjoint of a crop-embed is the input;
the pure moves are compared as integer views.  The routes behind UC_BILINEAR_ROWS2 (R = 2; the one-row kernel on 16-bit upsampling) run
in one fresh child process per value, which prints one JSON line per witness; whether R = 2, R = 4 and the one-row kernel agree bit for bit
is printed, not asserted (the compiler's contraction may differ between kernels).

Measured on an MI355X: the 461 tests of this file take 11.3 s together (397 small witnesses with three input families each, 2 big ones, 58
relation tests, 2 child tests, 2 argument tests).  The slowest are the two child tests, 3.0 s (UC_BILINEAR_ROWS2 = 0, 32 witnesses) and 2.7 s
(= 2, 16 witnesses), both dominated by the start of the process, the load of the library and the compilation of the plan driver; the first
test to touch the device takes 0.9 s, every other test 0.11 s or less, the big witnesses (268 MB of features with the reference in row
chunks; 16389 pixels at Cin = 256) included.  The 46 tests of the CPU file take 9 s.
Largest err / bound over the witnesses and input families of each route, by the store's dtype (dst, dx, dfeat) and for the fp32 outputs
out, dw, db.  Behind a 16-bit store a correct result reaches 0.99 by the one rounding of the store alone (u_out is exactly its worst
case); the f32 column shows the arithmetic.  0.0000: bound 0, bit for bit.  No witness was over the bound, none needed a change of a kernel.
                                                   f32    bf16     f16     out      dw      db
  uc_bilinear_nhwc one_row crop1                0.1370  0.9957  0.9955       -       -       -      (16-bit upsampling: the child with the knob at 0)
  uc_bilinear_nhwc one_row crop0                0.1503  0.9959  0.9912       -       -       -
  uc_bilinear_nhwc rows4 crop1                       -  0.9957  0.9955       -       -       -
  uc_bilinear_nhwc rows4 crop0                       -  0.9958  0.9890       -       -       -
  uc_bilinear_nhwc rows2 crop1                       -  0.9957       -       -       -       -      (the child with the knob at 2)
  uc_bilinear_nhwc rows2 crop0                       -  0.9958       -       -       -       -
  uc_resize_bilinear_nhwc ac1 one_row crop0     0.1406  0.9959  0.9862       -       -       -
  uc_resize_bilinear_nhwc ac1 rows4 crop0            -  0.9702  0.9889       -       -       -
  uc_resize_bilinear_nhwc ac0 halfpix           0.1742  0.9958  0.9961       -       -       -
  uc_bilinear_nhwc_bwd crop1 s00                0.0956  0.9870       -       -       -       -
  uc_bilinear_nhwc_bwd crop0 s00                0.1089  0.9844       -       -       -       -
  uc_bilinear_nhwc_bwd crop0 s01                0.2673  0.7894       -       -       -       -
  uc_resize_bilinear_nhwc_bwd ac1 crop0 s00     0.0621  0.9835       -       -       -       -
  uc_resize_bilinear_nhwc_bwd ac0 halfpix       0.2111  0.9957  0.9828       -       -       -
  uc_conv1x1_to4 coop c8=1 2 4                       -       -       -  0.1040  (c8 = 1; 0.0593, 0.0376)
  uc_conv1x1_to4 coop c8=8 16 32                     -       -       -  0.0281  (c8 = 16; 0.0272, 0.0140)
  uc_conv1x1_to4 coop c8=16, 1048579 pixels          -       -       -  0.0168
  uc_conv1x1_to4 pixel cin24 72 200                  -       -       -  0.0951  (Cin = 24; 0.0494, 0.0320)
  uc_conv1x1_to4 pixel misbias                       -       -       -  0.0475
  uc_conv1x1_to4_bwd mask0 cin8                 0.1531  0.9921       -       -  0.1340  0.0696
  uc_conv1x1_to4_bwd mask0 cin24                0.1566  0.9946       -       -  0.1677  0.0848
  uc_conv1x1_to4_bwd mask0 cin72                0.1409  0.9937       -       -  0.1823  0.1066
  uc_conv1x1_to4_bwd mask0 cin128               0.1669  0.9918       -       -  0.1727  0.0701
  uc_conv1x1_to4_bwd mask0 cin256               0.1852  0.9942       -       -  0.1705  0.0683
  uc_conv1x1_to4_bwd mask1 cin8                 0.1402  0.9924       -       -  0.1093  0.1152
  uc_conv1x1_to4_bwd mask1 cin24                0.1361  0.9903       -       -  0.1840  0.0798
  uc_conv1x1_to4_bwd mask1 cin72                0.1541  0.9937       -       -  0.1782  0.0991
  uc_conv1x1_to4_bwd mask1 cin128               0.1834  0.9947       -       -  0.1935  0.0907
  uc_conv1x1_to4_bwd mask1 cin256               0.1377  0.9790       -       -  0.1909  0.0788
  uc_conv1x1_to4_bwd mask1 cin256, 16389 pixels      -  0.9956       -       -  0.0023  0.0021
  uc_replicate_pad_nhwc_bwd                     0.3565  0.9961  0.9788       -       -       -
  uc_crop_add_nhwc res1 relu0                   0.3318  0.9884  0.9954       -       -       -
  uc_crop_add_nhwc res1 relu1                   0.3247  0.9660  0.9659       -       -       -
  uc_convt_scatter k1 2 4, uc_convt_gather k2 4, uc_dilate_nhwc, uc_pixel_shuffle P2 14 16, uc_im2col_t (stride 1 2, relu 0 1),
  uc_replicate_pad_nhwc, uc_crop_embed_nhwc, uc_crop_add_nhwc res0: 0.0000 in every dtype
Printed, not asserted: of the (witness, family) launches whose kernel the knob changes, 29 of 39 (R = 2 against R = 4) and 47 of 78 (one-row
against R = 4) agree bit for bit.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import head_stream_routes as R

pytestmark = pytest.mark.gpu

W = R.WITNESSES
F16 = R.CODE["h"]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("head_stream_routes_gpu"))


@pytest.fixture(scope="module")
def lib():
    from uniception_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(w, x):
    return x.view(R.INTV[w["dt"]] if x.dtype != torch.float32 else torch.int32)


def _assert_record(w, rec):
    label = f"{w['name']} ({rec['family']}): {R.route(w)}"
    if R.planned(w):
        assert rec["route"] == R.expected_plan(w), f"[{label}]: the launch takes [{rec['route']}], the witness stands for [{R.expected_plan(w)}]"
    assert rec["status"] == 0, f"[{label}]: status {rec['status']}"
    assert rec["bands"], f"[{label}]: a guard band around an output was written"
    assert rec["over"] == 0, rec["first"]
    print(f"HSROUTE {w['name']} {rec['family']} [{R.route(w)}] " + " ".join(f"{o}={v:.4f}" for o, v in rec["worst"].items()))


def _run(lib, w, families, gpu, plan):
    for family in families:
        rec = R.run_on_device(lib, w, family, gpu, plan)
        _assert_record(w, rec)
        t, o = rec["case"], R.outputs(w)[0]
        label = f"{w['name']} ({family})"
        if w["op"] in R.BITS:      # pure moves: the bits
            assert torch.equal(_bits(w, t[o]), _bits(w, rec["ref"][o][0].to(t[o].dtype))), f"[{label}]: a pure move changed bits"
        if w["op"] == "c1b" and w["relu"]:
            assert not bool((t["dfeat"][t["feat"] <= 0] != 0).any()), f"[{label}]: dfeat is not exactly 0 under the mask"
        if w["op"] in ("bl", "blb") and (w["Hi"], w["Wi"]) == (w["Ho"], w["Wo"]) == (w["ch"], w["cw"]):
            src = t["src" if w["op"] == "bl" else "dy"]
            assert torch.equal(_bits(w, t[o]), _bits(w, src)), f"[{label}]: an identity resize does not return the input's bits"


@pytest.mark.parametrize("name", R.PARENT)
def test_small_witness_against_fp64(gpu, lib, plan, name):
    _run(lib, W[name], R.FAMILIES, gpu, plan)


@pytest.mark.parametrize("name", R.BIG)
def test_big_witness_against_fp64(gpu, lib, plan, name):
    """The grid-stride loops: uc_conv1x1_to4 at Cin = 128 with cap * 16 + 3 pixels (three workgroups take a second iteration; the reference in
    row chunks) and uc_conv1x1_to4_bwd at Cin = 256 with 2048 * 8 + 5 pixels (five do)."""
    _run(lib, W[name], ("wide",), gpu, plan)


# ------------------------------------------------------------------------------------------ exact relations between launches
def _fresh(w, family, gpu):
    return R.make_case(w, family, gpu, seed=R.seed_of(w))


def _go(lib, w, t, **over):
    rc = R.launch(lib, w, t, _stream(), **over)
    torch.cuda.synchronize()
    assert rc == 0, (w["name"], rc, lib.uc_last_error())
    assert R.bands_ok(w, t), w["name"]


@pytest.mark.parametrize("name", [n for n in R.PARENT if W[n]["op"] == "bl" and W[n]["rule"] == "ac" and R._cropped(W[n])])
def test_a_cropped_bilinear_launch_is_the_window_of_the_uncropped_one(gpu, lib, name):
    w = W[name]
    full = dict(w, ch=w["Ho"], cw=w["Wo"])
    for family in R.FAMILIES:
        a, b = _fresh(w, family, gpu), _fresh(full, family, gpu)
        assert torch.equal(_bits(w, a["src"]), _bits(w, b["src"]))
        _go(lib, w, a)
        _go(lib, full, b)
        assert torch.equal(_bits(w, a["dst"]), _bits(w, b["dst"][:, :w["ch"], :w["cw"]])), f"{name} ({family}): the crop is not the window, bit for bit"


@pytest.mark.parametrize("name", [n for n in R.PARENT if W[n]["op"] in ("bl", "blb") and W[n]["rule"] == "ac" and W[n]["entry"] == "resize"])
def test_resize_with_align_corners_is_the_dpt_kernel(gpu, lib, name):
    w = W[name]
    o = R.outputs(w)[0]
    for family in R.FAMILIES:
        a, b = _fresh(w, family, gpu), _fresh(w, family, gpu)
        _go(lib, w, a)
        _go(lib, dict(w, entry="bilinear"), b)
        assert torch.equal(_bits(w, a[o]), _bits(w, b[o])), f"{name} ({family}): uc_resize_bilinear_nhwc(align_corners = 1) is not uc_bilinear_nhwc, bit for bit"


@pytest.mark.parametrize("name", [n for n in R.PARENT if W[n]["op"] == "ga"])
def test_gather_of_scatter_is_the_input(gpu, lib, name):
    ga = W[name]
    sc = dict(ga, op="sc")
    for family in R.FAMILIES:
        t = _fresh(sc, family, gpu)
        _go(lib, sc, t)
        u = _fresh(ga, family, gpu)
        u["src"].copy_(t["dst"])
        _go(lib, ga, u)
        assert torch.equal(_bits(ga, u["dst"]), _bits(ga, t["src"])), f"{name} ({family})"


@pytest.mark.parametrize("name", [n for n in R.PARENT if W[n]["op"] == "emb"])
def test_the_pad_adjoint_of_a_crop_embed_is_the_input(gpu, lib, name):
    emb = W[name]
    padb = dict(emb, op="padb")
    for family in R.FAMILIES:
        t = _fresh(emb, family, gpu)
        _go(lib, emb, t)
        u = _fresh(padb, family, gpu)
        u["dy"].copy_(t["dst"])
        _go(lib, padb, u)
        assert bool((u["dx"] == t["dy"]).all()), f"{name} ({family})"      # sums of one value and zeros: the value (-0 + 0 = +0: values)


# ------------------------------------------------------------------------------------------ the routes behind UC_BILINEAR_ROWS2
CHILD_TIMEOUT = 240      # seconds: process start, the library, the driver's compilation and about a hundred tiny launches


@pytest.mark.parametrize("rows2", [2, 0])
def test_the_routes_behind_the_rows_knob_in_a_fresh_process(gpu, lib, plan, rows2):
    env = dict(os.environ, UC_BILINEAR_ROWS2=str(rows2))
    child = subprocess.run([sys.executable, "-m", "tests.head_stream_routes", "--bilinear-child"], cwd=R.ROOT, env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    assert child.returncode == 0, f"the child with UC_BILINEAR_ROWS2={rows2} ended with {child.returncode}:\n{child.stderr[-4000:]}"
    recs = [json.loads(line) for line in child.stdout.splitlines() if line.startswith("{")]
    names = R.knob_witnesses(rows2)
    assert [(r["name"], r["family"]) for r in recs] == [(n, f) for n in names for f in R.FAMILIES]
    kernels = set()
    for r in recs:
        w = W[r["name"]]
        label = f"{r['name']} ({r['family']}): {R.route(w)}"
        assert r["route"] == R.expected_plan(w), f"[{label}]: the launch takes [{r['route']}], the witness stands for [{R.expected_plan(w)}]"
        assert r["status"] == 0 and r["bands"], label
        assert r["over"] == 0, r["first"]
        kernels.add((w["dt"],) + R.bl_kernel(w))
        print(f"HSROUTE {r['name']} {r['family']} [{R.route(w)}] dst={r['worst']:.4f}")
    assert kernels == ({("b", "rows", 2), ("b", "one_row", 1)} if rows2 == 2 else {("b", "one_row", 1), ("h", "one_row", 1)})
    # printed, not asserted: whether this knob value's kernel and the default's (R = 4 where the rows route is taken) agree bit for bit
    same = total = 0
    for r in recs:
        w = W[r["name"]]
        twin = W[R.NAMES[R.seed_of(w)]]
        if R.bl_kernel(twin) == R.bl_kernel(w):
            continue
        t = _fresh(twin, r["family"], gpu)
        _go(lib, twin, t)
        total += 1
        same += R._bits_hex(t["dst"]) == r["bits"]
    print(f"HSBITS UC_BILINEAR_ROWS2={rows2}: {same} of {total} (witness, family) launches agree bit for bit with the default's kernel")


# ------------------------------------------------------------------------------------------ arguments
def _nothing_written(w, t):
    assert R.bands_ok(w, t), w["name"]
    for o in R.outputs(w):
        if o in ("dw", "db"):
            assert torch.equal(t[o], t["pre_" + o]), (w["name"], o)
        else:
            assert bool(torch.isnan(t[o]).all()), (w["name"], o)


def _refused(lib, gpu, name, message, **over):
    w = W[name]
    t = _fresh(w, "wide", gpu)
    rc = R.launch(lib, w, t, _stream(), **over)
    err = lib.uc_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and message in err, (name, over, rc, err)
    _nothing_written(w, t)


def test_bad_shapes_are_refused_without_a_launch(gpu, lib):
    bl, blb = "bl_f_ac_5x7-10x14_c8", "blb_f_ac_5x7-10x14_c8"
    for name, fn in ((bl, "uc_bilinear_nhwc"), (blb, "uc_bilinear_nhwc_bwd")):
        _refused(lib, gpu, name, f"{fn}: bad shape (C must be a multiple of 8)", C=12)
        _refused(lib, gpu, name, f"{fn}: bad shape", B=0)
        _refused(lib, gpu, name, f"{fn}: bad shape", Ho=0)
        _refused(lib, gpu, name, f"{fn}: bad crop", ch=11)
        _refused(lib, gpu, name, f"{fn}: bad crop", cw=15)
        _refused(lib, gpu, name, f"{fn}: bad crop", ch=0)
    _refused(lib, gpu, "bl_f_hpr_5x7-12x9_c8", "uc_resize_bilinear_nhwc: bad shape", C=12)
    _refused(lib, gpu, "blb_f_hpr_5x7-12x9_c8", "uc_resize_bilinear_nhwc_bwd: bad output size", Wo=0)
    _refused(lib, gpu, "c1_f_c64_n98", "uc_conv1x1_to4: Cin must be a multiple of 8 and <= 256 (got 264)", Cin=264)
    _refused(lib, gpu, "c1_f_c64_n98", "uc_conv1x1_to4: Cin must be a multiple of 8", Cin=12)
    _refused(lib, gpu, "c1_f_c64_n98", "uc_conv1x1_to4: bad argument", npix=0)
    _refused(lib, gpu, "c1b_f_c72_n86_m1", "uc_conv1x1_to4_bwd: Cin must be a multiple of 8 and <= 256", Cin=264)
    _refused(lib, gpu, "c1b_f_c72_n86_m1", "uc_conv1x1_to4_bwd: Cin must be a multiple of 8 and <= 256", npix=0)
    im = "im_f_c16_s1_r0_ld37"
    _refused(lib, gpu, im, "uc_im2col_t: ld must be in [npix, npix+64)", ld=W[im]["npix"] - 1)
    _refused(lib, gpu, im, "uc_im2col_t: ld must be in [npix, npix+64)", ld=W[im]["npix"] + 64)
    _refused(lib, gpu, im, "uc_im2col_t: bad argument", stride=0)
    _refused(lib, gpu, "sc_f_k2", "uc_convt_scatter: bad shape (Cout must be a multiple of 8)", C=4)
    _refused(lib, gpu, "ga_f_k2", "uc_convt_gather: bad argument (Cout must be a multiple of 8)", C=4)
    _refused(lib, gpu, "di_f_5x8", "uc_dilate_nhwc: source does not fit the dilated grid", H=4)
    _refused(lib, gpu, "ps_f_p2", "uc_pixel_shuffle: bad argument", P=0)
    for op, fn in (("pad", "uc_replicate_pad_nhwc"), ("padb", "uc_replicate_pad_nhwc_bwd"), ("emb", "uc_crop_embed_nhwc")):
        _refused(lib, gpu, f"{op}_f_3x5_c8", f"{fn}: bad shape", C=12)
        _refused(lib, gpu, f"{op}_f_3x5_c8", f"{fn}: bad shape", H=0)
    _refused(lib, gpu, "cadd_f_3x5_res1_relu1", "uc_crop_add_nhwc: bad shape", W=0)


def test_unsupported_dtypes_are_refused_without_a_launch(gpu, lib):
    two = "UC_F32 or UC_BF16"
    three = "UC_F32, UC_BF16 or UC_F16"
    for name, fn in (("blb_f_ac_5x7-10x14_c8", "uc_bilinear_nhwc_bwd"), ("c1b_f_c72_n86_m1", "uc_conv1x1_to4_bwd"), ("ga_f_k2", "uc_convt_gather"),
                     ("di_f_5x8", "uc_dilate_nhwc"), ("im_f_c16_s1_r0_ld37", "uc_im2col_t"), ("blb_f_acr_5x7-10x14_c8", "uc_bilinear_nhwc_bwd")):
        _refused(lib, gpu, name, f"{fn}: unsupported dtype {F16} ({two})", dtype=F16)
        _refused(lib, gpu, name, f"{fn}: unsupported dtype 7 ({two})", dtype=7)
    for name, fn in (("bl_f_ac_5x7-10x14_c8", "uc_bilinear_nhwc"), ("bl_f_hpr_5x7-12x9_c8", "uc_resize_bilinear_nhwc"),
                     ("blb_f_hpr_5x7-12x9_c8", "uc_resize_bilinear_nhwc_bwd"), ("c1_f_c64_n98", "uc_conv1x1_to4"), ("c1_f_c24_n257", "uc_conv1x1_to4"),
                     ("sc_f_k2", "uc_convt_scatter"), ("ps_f_p2", "uc_pixel_shuffle"), ("pad_f_3x5_c8", "uc_replicate_pad_nhwc"),
                     ("padb_f_3x5_c8", "uc_replicate_pad_nhwc_bwd"), ("emb_f_3x5_c8", "uc_crop_embed_nhwc"), ("cadd_f_3x5_res1_relu1", "uc_crop_add_nhwc")):
        _refused(lib, gpu, name, f"{fn}: unsupported dtype 7 ({three})", dtype=7)
        _refused(lib, gpu, name, f"{fn}: unsupported dtype -1 ({three})", dtype=-1)
