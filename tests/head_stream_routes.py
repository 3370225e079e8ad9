"""Route audit of the DPT / MoGe heads' streaming kernels (uniception_amd/csrc/elementwise.hip, csrc/dpt_bwd.hip, csrc/pad_resize.hip):
routes, witness shapes, operands inside guard bands, the fp64 reference, the per-element bound and a CPU model of each kernel's index
arithmetic that can be given the defects these kernels can have.  No GPU code is imported; `python -m tests.head_stream_routes` prints the
witness table, `--bilinear-child` is the child process of the two UC_BILINEAR_ROWS2 tests of tests/test_head_stream_routes_gpu.py.

ROUTES.  A route is (entry point, kernel, dtype, run-time branches); `route(w)` is its text, `required_routes()` the list every pull request
has to keep witnessed.  The two host-side choices (the kernel of a uc_bilinear_nhwc launch, the kernel of a uc_conv1x1_to4 launch) and
the grid caps come from uniception_amd/csrc/stream_plan.h, checked through tests/stream_plan_driver.cpp.
  bl    uc_bilinear_nhwc            one-row x {f32, bf16, f16} | rows R = 4 x {bf16, f16} | rows R = 2 x bf16; crop on / off
        uc_resize_bilinear_nhwc     align_corners = 1: the same kernels; align_corners = 0: the half-pixel kernel x {f32, bf16, f16}
  blb   uc_bilinear_nhwc_bwd        {f32, bf16}; crop on / off; the s <= 0 branch of tap_range
        uc_resize_bilinear_nhwc_bwd align_corners = 1: the same kernel; align_corners = 0: the half-pixel adjoint x {f32, bf16, f16}
  c1    uc_conv1x1_to4              cooperative C8 in {1, 2, 4, 8, 16, 32} | one thread per pixel by Cin (24, 72, 200) | by a bias 4 bytes off
                                    16-byte alignment; x {f32, bf16, f16}
  c1b   uc_conv1x1_to4_bwd          {f32, bf16} x relu_mask 0 / 1 x Cin in {8, 24, 72, 128, 256} (24: one dead thread, 72: four)
  sc / ga / di / ps / im            uc_convt_scatter, uc_convt_gather, uc_dilate_nhwc, uc_pixel_shuffle, uc_im2col_t
  pad / padb / emb / cadd           uc_replicate_pad_nhwc, its adjoint, uc_crop_embed_nhwc, uc_crop_add_nhwc (residual, relu)

WITNESSES (`WITNESSES`), each the smallest shape at which its kernel can still go wrong, B = 2 wherever a batch stride exists.
  bilinear forward, every route: 19 x 19 -> 38 x 38 cropped to 37 x 37 at C = 64 (the DPT shape, sy = 18 / 37; crop_w * C / 8 = 296: two
    x-blocks, the second ragged); 5 x 5 -> 10 x 10 with crop_h in 1 .. 7 (every remainder of a row group of 4 or 2, groups shorter than R);
    3 -> 5 (sy = 0.5 exactly, the boundary of the rows route); 5 x 7 -> 10 x 14 (C = 8 and 64); 37 -> 65 (sy = 0.5625: one-row); 37 -> 19;
    Hi = Wi = 1; Ho = Wo = 1 (scale 0); Hi = Ho, Wi = Wo.  The R = 2 route and the one-row route on 16-bit upsampling need
    UC_BILINEAR_ROWS2 = 2 / 0, which the library reads once: those witnesses (`rows2` 2 / 0) run in a child process.
  bilinear backward: the adjoint of each shape; 37 -> 10 (most inputs receive nothing and must be exactly 0); a 9 x 9 crop of the DPT shape
    (input rows without any tap); Ho = 1 (everything goes to input row 0, the other rows are written as zeros).
  half-pixel, both directions: 5 x 7 -> 12 x 9 (up and down; num <= 0 clamps at the start, i1 at the end), 7 -> 3, 7 -> 2, 4 -> 8, identity,
    in = 1, out = 1.
  conv1x1_to4: npix in {1, PPB, PPB + 1, 3 PPB + 2} per C8 (PPB = 256 / C8); one big witness Cin = 128, bf16, npix = cap * 16 + 3 (the first
    three workgroups take a second iteration; 268 MB of features, drawn on the device, the reference in row chunks; on the CPU only the
    rows around the seam are held).  The one-thread-per-pixel kernel's own cap needs more than 67 M pixels and is left out, as is the
    EW_GRID cap of the other grid-stride kernels.
  conv1x1_to4_bwd: npix in {1, lanes + 1, 3 lanes + 2} per Cin (lanes = 256 / (Cin / 8)); Cin = 256 at npix = 2048 * 8 + 5 (five workgroups
    take a second iteration); feat holds exact +0 and -0 and values of both signs.
  im2col_t: Cin in {5, 16, 72}, stride 1 / 2, H = 5, W = 7, ld = npix and npix + 37, npix (70 / 24) no multiple of 64.
  the rest: odd H and W; H = 1 or W = 1 for the pads (the adjoint then sums up to nine positions).

INPUTS (`make_case`): families `wide` N(0.5, 3^2); `ramp`, linear in (row, column) plus a per-channel offset (its interpolation is linear too:
a wrong scale or an off-by-one index shows at many elements); `spike`, N(0, 1) with one element of 1e4 in the last row and column — for an
adjoint dy is zero except two spikes, at the far corner and in the interior.  All three on every small witness, the first on the big ones.
Operands are rounded to their storage dtype first; every buffer is a slice of a larger one, inputs between bands of NaN, outputs NaN
between bands of SENTINEL; dw / db start at a non-zero prefill (`+=`).

REFERENCE: the expressions of include/uc_hip.h in float64; coordinates exact: the rational (in - 1) o / (out - 1) for the align-corners rule,
((2 d + 1) in - out) / (2 out) for the half-pixel rule.
BOUND per element, the form and constants of tests/gemm_routes.py (u_out = U_OUT of the store; S = the expression on absolute values):
    resize forward   u_out |ref| + 8 sqrt(4) 2^-24 S + dy Dy + dx Dx      d = the a-priori error of the fp32 coordinate (2^-23 c for the
                     align-corners rule: the scale and the product round once each; 2^-24 for the half-pixel rule: one division),
                     D = the largest |difference| of vertically / horizontally adjacent samples over the cell and its neighbour cells (the
                     interpolant is continuous, so a coordinate that lands in the next cell moves the value by at most d times a slope)
    resize adjoint   u_out |ref| + 8 sqrt(n_taps) 2^-24 S + sum_o (dy(o) + dx(o)) |dy_o| over the outputs within one input pixel (+ d);
                     an element with no such output has bound 0: exactly 0
    conv1x1_to4      2^-24 |ref| + 8 sqrt(Cin + 1) 2^-24 S
    dfeat            u_out |ref| + 8 sqrt(4) 2^-24 S; exactly 0 where relu_mask is set and feat <= 0
    dw, db           2^-24 |ref| + 8 sqrt(npix) 2^-24 S + 8 sqrt(n_add) 2^-24 |prefill|, compared as target - prefill, n_add = the grid
    pad adjoint, crop-add   u_out |ref| + n 2^-24 S, n = the summed terms; n = 1: exact
    everything else  bound 0 (`check` then compares values, so -0 = +0); pure moves (`BITS`) are also compared as integer views
An fp16 store below 2^-14 is subnormal with spacing 2^-24: its store term is never below 2^-25 (tests/gemm_routes.py).

MODEL (`model`): float32 torch on the CPU that follows each kernel's index arithmetic on the flat banded buffers — the fp32 coordinate and
its (int) truncation, the row-group selection of the rows kernel, tap_range / halfpix_range — and writes through the kernel's destination
index into a copy of the output buffer, so a defect (`DEFECTS`) reads and writes what the device would.
REFERENCE BUDGET: no small witness needs more than REF_BUDGET_ELEMS fp64 multiply-adds for reference and bound together.
"""
import json
import math
import os
import re
import shutil
import subprocess
import sys

import torch

from tests.gemm_routes import BF16, F16, F32, ROOT, U_OUT
from tests.layernorm_routes import GUARD, SENTINEL, _banded, bands_untouched, check, ratio      # noqa: F401  (re-exported to the test files)

FAMILIES = ("wide", "ramp", "spike")
DT = {"f": torch.float32, "b": torch.bfloat16, "h": torch.float16}
CODE = {"f": F32, "b": BF16, "h": F16}
BYTES = {"f": 4, "b": 2, "h": 2}
INTV = {"f": torch.int32, "b": torch.int16, "h": torch.int16}
ACC = 8.0 * 2.0 ** -24
U24 = 2.0 ** -24
REF_BUDGET_ELEMS = 2.0e8
BITS = ("sc", "ga", "di", "ps", "pad", "emb")      # pure moves: integer views are compared (im and cadd pass through fmaxf: values)


def _plan_constants():
    "The integer constants of stream_plan.h (grid caps, workgroup size): read, not retyped."
    text = open(os.path.join(ROOT, "uniception_amd", "csrc", "stream_plan.h")).read()
    return {k: math.prod(int(f) for f in v.split("*")) for k, v in re.findall(r"static constexpr int (UC_\w+) = ([\d *]+);", text)}


PLAN = _plan_constants()
WG = PLAN["UC_STREAM_WG"]
COOP_CAP, BWD_CAP, EW_CAP = PLAN["UC_CONV1X1_COOP_GRID_CAP"], PLAN["UC_CONV1X1_BWD_GRID_CAP"], PLAN["UC_EW_GRID_CAP"]
COOP_CIN = (8, 16, 32, 64, 128, 256)


# ------------------------------------------------------------------------------------------ witnesses
def _w(op, dt, tag, big=False, **kw):
    return dict(name=f"{op}_{dt}_{tag}", op=op, dt=dt, big=big, **kw)


def _bl(op, dt, shape, C, rule="ac", entry="bilinear", rows2=4, crop=None):
    Hi, Wi, Ho, Wo = shape
    ch, cw = crop or (Ho, Wo)
    tag = f"{rule}{'r' if entry == 'resize' else ''}_{Hi}x{Wi}-{Ho}x{Wo}_c{C}" + (f"_crop{ch}x{cw}" if crop else "") + (f"_k{rows2}" if rows2 != 4 else "")
    return _w(op, dt, tag, rule=rule, entry=entry, rows2=rows2, B=2, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, ch=ch, cw=cw, C=C)


DPT = ((19, 19, 38, 38), 64, (37, 37))
BL_SHAPES = ([DPT] + [((5, 5, 10, 10), 8, (ch, 7)) for ch in range(1, 8)] +
             [((3, 3, 5, 5), 8, None), ((5, 7, 10, 14), 8, None), ((5, 7, 10, 14), 64, None), ((37, 3, 65, 5), 8, None), ((37, 9, 19, 5), 8, None),
              ((1, 1, 4, 5), 8, None), ((5, 7, 1, 1), 8, None), ((6, 5, 6, 5), 8, None)])
BLB_EXTRA = [((37, 5, 10, 3), 8, None), ((19, 19, 38, 38), 8, (9, 9)), ((5, 7, 1, 6), 8, None)]
HP_SHAPES = [((5, 7, 12, 9), 8), ((5, 7, 12, 9), 16), ((7, 7, 3, 3), 8), ((7, 5, 2, 2), 8), ((4, 4, 8, 8), 8), ((5, 6, 5, 6), 8), ((1, 1, 3, 4), 8), ((5, 7, 1, 1), 8)]
AC_RESIZE = [((5, 7, 10, 14), 8), ((37, 3, 65, 5), 8), ((6, 5, 6, 5), 8)]
KNOBS = {"f": (4,), "b": (4, 2, 0), "h": (4, 0)}      # the UC_BILINEAR_ROWS2 values under which a dtype's witnesses run


def lanes_of(Cin):
    return WG // (Cin // 8)


def _witnesses():
    out = []
    for dt in "fbh":
        for rows2 in KNOBS[dt]:
            out += [_bl("bl", dt, s, C, rows2=rows2, crop=crop) for s, C, crop in BL_SHAPES]
        out += [_bl("bl", dt, s, C, entry="resize") for s, C in AC_RESIZE]
        out += [_bl("bl", dt, s, C, rule="hp", entry="resize") for s, C in HP_SHAPES]
        out += [_bl("blb", dt, s, C, rule="hp", entry="resize") for s, C in HP_SHAPES]
    for dt in "fb":
        out += [_bl("blb", dt, s, C, crop=crop) for s, C, crop in BL_SHAPES + BLB_EXTRA]
        out += [_bl("blb", dt, s, C, entry="resize") for s, C in AC_RESIZE]
    # ---- conv1x1_to4
    for i, Cin in enumerate(COOP_CIN):
        ppb = WG // (Cin // 8)
        for j, npix in enumerate((1, ppb, ppb + 1, 3 * ppb + 2)):
            for dt in ("fbh" if j == 3 else "fbh"[(i + j) % 3]):
                out.append(_w("c1", dt, f"c{Cin}_n{npix}", Cin=Cin, npix=npix, mis=0))
    for dt in "fbh":
        out += [_w("c1", dt, f"c{Cin}_n{npix}", Cin=Cin, npix=npix, mis=0) for Cin in (24, 72, 200) for npix in (1, WG + 1)]
        out.append(_w("c1", dt, f"c64_n{WG + 1}_misbias", Cin=64, npix=WG + 1, mis=1))
    out.append(_w("c1", "b", f"c128_n{COOP_CAP * 16 + 3}", big=True, Cin=128, npix=COOP_CAP * 16 + 3, mis=0))
    for dt in "fb":
        for relu in (0, 1):
            for Cin in (8, 24, 72, 128, 256):
                ln = lanes_of(Cin)
                out += [_w("c1b", dt, f"c{Cin}_n{n}_m{relu}", Cin=Cin, npix=n, relu=relu) for n in (1, ln + 1, 3 * ln + 2)]
    out.append(_w("c1b", "b", f"c256_n{BWD_CAP * 8 + 5}_m1", big=True, Cin=256, npix=BWD_CAP * 8 + 5, relu=1))
    # ---- the moves
    for dt in "fbh":
        out += [_w("sc", dt, f"k{k}", B=2, h=3, w=5, k=k, C=16 if k == 4 else 8) for k in (1, 2, 4)]
        out += [_w("ps", dt, f"p{P}", B=2, h=3, w=2, P=P, C=3) for P in (2, 14, 16)]
        for H, W, C in ((3, 5, 8), (3, 5, 16), (1, 5, 8), (5, 1, 8), (1, 1, 8)):
            out += [_w(op, dt, f"{H}x{W}_c{C}", B=2, H=H, W=W, C=C) for op in ("pad", "padb", "emb")]
        out += [_w("cadd", dt, f"3x5_res{res}_relu{relu}", B=2, H=3, W=5, C=8, res=res, relu=relu) for res in (0, 1) for relu in (0, 1)]
    for dt in "fb":
        out += [_w("ga", dt, f"k{k}", B=2, h=3, w=5, k=k, C=16 if k == 4 else 8) for k in (2, 4)]
        out += [_w("di", dt, f"{H}x{W}", B=2, h=3, w=4, H=H, W=W, C=8, s=2) for H, W in ((6, 7), (5, 8))]
        for stride in (1, 2):
            npix = 2 * ((5 - 1) // stride + 1) * ((7 - 1) // stride + 1)
            out += [_w("im", dt, f"c{Cin}_s{stride}_r{relu}_ld{pad}", B=2, H=5, W=7, Cin=Cin, stride=stride, relu=relu, npix=npix, ld=npix + pad)
                    for Cin in (5, 16, 72) for relu in (0, 1) for pad in (0, 37)]
    names = [w["name"] for w in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return {w["name"]: w for w in out}


WITNESSES = _witnesses()
NAMES = list(WITNESSES)
SMALL = [n for n in NAMES if not WITNESSES[n]["big"]]
BIG = [n for n in NAMES if WITNESSES[n]["big"]]
PARENT = [n for n in SMALL if WITNESSES[n].get("rows2", 4) == 4]      # what a process with the default knob can launch
OPS = ("bl", "blb", "c1", "c1b", "sc", "ga", "di", "ps", "im", "pad", "padb", "emb", "cadd")


def seed_of(w):
    "The seed of a witness's operands; the same under every knob value, so that the kernels a knob selects see the same maps."
    return NAMES.index(w["name"][:-3] if w.get("rows2", 4) != 4 else w["name"])      # without the knob's suffix `_k2` / `_k0`


def knob_witnesses(rows2):
    "The bilinear forward witnesses a process with UC_BILINEAR_ROWS2 = rows2 launches."
    return [n for n in SMALL if WITNESSES[n]["op"] == "bl" and WITNESSES[n]["entry"] == "bilinear" and WITNESSES[n]["rows2"] == rows2]


def scale32(n_in, n_out):
    return float(torch.tensor(float(n_in - 1)) / torch.tensor(float(n_out - 1))) if n_out > 1 else 0.0


def bl_kernel(w):
    "(kernel, R) of a bilinear forward witness by the rule of stream_plan.h, worked here."
    if w["rule"] == "hp":
        return "halfpix", 1
    rows = w["rows2"] != 0 and scale32(w["Hi"], w["Ho"]) <= 0.5 and w["dt"] in "bh"
    return ("rows", 4 if w["dt"] == "h" or w["rows2"] == 4 else 2) if rows else ("one_row", 1)


def c1_kernel(w):
    return ("coop", w["Cin"] // 8) if w["Cin"] in COOP_CIN and not w["mis"] else ("pixel", 0)


def _cropped(w):
    return int((w["ch"], w["cw"]) != (w["Ho"], w["Wo"]))


def route(w):
    op, dt = w["op"], w["dt"]
    if op == "bl":
        k, R = bl_kernel(w)
        if w["rule"] == "hp":
            return f"uc_resize_bilinear_nhwc ac0 halfpix {dt}"
        head = "uc_resize_bilinear_nhwc ac1" if w["entry"] == "resize" else "uc_bilinear_nhwc"
        return f"{head} {k}{R if k == 'rows' else ''} {dt} crop{_cropped(w)}"
    if op == "blb":
        if w["rule"] == "hp":
            return f"uc_resize_bilinear_nhwc_bwd ac0 halfpix {dt}"
        head = "uc_resize_bilinear_nhwc_bwd ac1" if w["entry"] == "resize" else "uc_bilinear_nhwc_bwd"
        return f"{head} {dt} crop{_cropped(w)} s0{int(w['Ho'] == 1 or w['Hi'] == 1)}"
    if op == "c1":
        k, c8 = c1_kernel(w)
        return f"uc_conv1x1_to4 {'coop c8=' + str(c8) if k == 'coop' else 'pixel ' + ('misbias' if w['mis'] else 'cin' + str(w['Cin']))} {dt}"
    if op == "c1b":
        return f"uc_conv1x1_to4_bwd {dt} mask{w['relu']} cin{w['Cin']}"
    tail = {"sc": lambda: f"uc_convt_scatter k{w['k']}", "ga": lambda: f"uc_convt_gather k{w['k']}",
            "di": lambda: f"uc_dilate_nhwc s2 {'even' if w['H'] == 2 * w['h'] else 'odd'}H", "ps": lambda: f"uc_pixel_shuffle P{w['P']}",
            "im": lambda: f"uc_im2col_t stride{w['stride']} relu{w['relu']}", "pad": lambda: "uc_replicate_pad_nhwc",
            "padb": lambda: "uc_replicate_pad_nhwc_bwd", "emb": lambda: "uc_crop_embed_nhwc",
            "cadd": lambda: f"uc_crop_add_nhwc res{w['res']} relu{w['relu']}"}[op]()
    return f"{tail} {dt}"


def required_routes():
    "The routes of the issue's table, generated from the table and not from the witnesses."
    r = []
    for crop in (0, 1):
        r += [f"uc_bilinear_nhwc one_row {dt} crop{crop}" for dt in "fbh"] + [f"uc_bilinear_nhwc rows4 {dt} crop{crop}" for dt in "bh"]
        r += [f"uc_bilinear_nhwc rows2 b crop{crop}"] + [f"uc_bilinear_nhwc_bwd {dt} crop{crop} s00" for dt in "fb"]
    r += [f"uc_bilinear_nhwc_bwd {dt} crop0 s01" for dt in "fb"]
    r += [f"uc_resize_bilinear_nhwc ac0 halfpix {dt}" for dt in "fbh"] + [f"uc_resize_bilinear_nhwc_bwd ac0 halfpix {dt}" for dt in "fbh"]
    r += [f"uc_resize_bilinear_nhwc ac1 one_row {dt} crop0" for dt in "fbh"] + [f"uc_resize_bilinear_nhwc ac1 rows4 {dt} crop0" for dt in "bh"]
    r += [f"uc_resize_bilinear_nhwc_bwd ac1 {dt} crop0 s00" for dt in "fb"]
    for dt in "fbh":
        r += [f"uc_conv1x1_to4 coop c8={c8} {dt}" for c8 in (1, 2, 4, 8, 16, 32)] + [f"uc_conv1x1_to4 pixel cin{c} {dt}" for c in (24, 72, 200)]
        r += [f"uc_conv1x1_to4 pixel misbias {dt}"] + [f"uc_convt_scatter k{k} {dt}" for k in (1, 2, 4)] + [f"uc_pixel_shuffle P{P} {dt}" for P in (2, 14, 16)]
        r += [f"{e} {dt}" for e in ("uc_replicate_pad_nhwc", "uc_replicate_pad_nhwc_bwd", "uc_crop_embed_nhwc")]
        r += [f"uc_crop_add_nhwc res{a} relu{b} {dt}" for a in (0, 1) for b in (0, 1)]
    for dt in "fb":
        r += [f"uc_conv1x1_to4_bwd {dt} mask{m} cin{c}" for m in (0, 1) for c in (8, 24, 72, 128, 256)]
        r += [f"uc_convt_gather k{k} {dt}" for k in (2, 4)] + [f"uc_dilate_nhwc s2 {p}H {dt}" for p in ("even", "odd")]
        r += [f"uc_im2col_t stride{s} relu{a} {dt}" for s in (1, 2) for a in (0, 1)]
    return r


# ------------------------------------------------------------------------------------------ plan driver
def build_driver(tmpdir):
    "Compile tests/stream_plan_driver.cpp with the system C++ compiler into tmpdir; returns run(rows) -> plan lines."
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/stream_plan_driver.cpp"
    exe = os.path.join(str(tmpdir), "stream_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "uniception_amd", "csrc"),
                           os.path.join(ROOT, "tests", "stream_plan_driver.cpp"), "-o", exe])

    def run(rows):
        if not rows:
            return []
        lines = [" ".join(f"{k}={v}" for k, v in row.items()) for row in rows]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return run


BASE = 1 << 20      # a placeholder address, aligned for everything


def planned(w):
    "Whether a host-side plan decides anything about the witness's launch."
    return (w["op"] == "bl" and w["rule"] == "ac") or w["op"] in ("c1", "c1b")


def driver_row(w, bias_ptr=None):
    "The launch of the witness as a driver row; `bias_ptr`: the real address, else a placeholder with the witness's misalignment."
    if w["op"] == "bl":
        return dict(op="bilinear", dtype=CODE[w["dt"]], Hi=w["Hi"], Ho=w["Ho"], crop_h=w["ch"], crop_w=w["cw"], C=w["C"], B=w["B"], rows2=w["rows2"])
    if w["op"] == "c1":
        return dict(op="conv1x1", Cin=w["Cin"], bias=BASE + 4 * w["mis"] if bias_ptr is None else bias_ptr, npix=w["npix"])
    return dict(op="conv1x1_bwd", Cin=w["Cin"], npix=w["npix"])


def grid_of(w):
    if w["op"] == "c1":
        k, c8 = c1_kernel(w)
        return min(COOP_CAP, -(-w["npix"] // (WG // c8))) if k == "coop" else min(EW_CAP, -(-w["npix"] // WG))
    return min(BWD_CAP, -(-w["npix"] // lanes_of(w["Cin"])))


def expected_plan(w):
    "The plan line of the witness, worked here from PLAN."
    if w["op"] == "bl":
        k, R = bl_kernel(w)
        return f"bilinear {k} {R} {-(-w['cw'] * (w['C'] // 8) // WG)} {-(-w['ch'] // R)} {w['B']}"
    if w["op"] == "c1":
        k, c8 = c1_kernel(w)
        return f"conv1x1 {k} {c8} {grid_of(w)}"
    return f"conv1x1_bwd {grid_of(w)}"


# ------------------------------------------------------------------------------------------ operands
def buffers(w):
    "(inputs, outputs): lists of (name, shape, dtype char)."
    op, dt = w["op"], w["dt"]
    g = w.get
    if op in ("bl", "blb"):
        a, b = ("src", (g("B"), g("Hi"), g("Wi"), g("C")), dt), ("dst", (g("B"), g("ch"), g("cw"), g("C")), dt)
        return ([a], [b]) if op == "bl" else ([("dy",) + b[1:]], [("dx",) + a[1:]])
    if op == "c1":
        return [("feat", (g("rows", g("npix")), g("Cin")), dt), ("w", (4, g("Cin")), "f"), ("bias", (4,), "f")], [("out", (g("rows", g("npix")), 4), "f")]
    if op == "c1b":
        return ([("feat", (g("npix"), g("Cin")), dt), ("w", (4, g("Cin")), "f"), ("dout", (g("npix"), 4), "f")],
                [("dfeat", (g("npix"), g("Cin")), dt), ("dw", (4, g("Cin")), "f"), ("db", (4,), "f")])
    if op in ("sc", "ga"):
        a, b = (g("B") * g("h") * g("w"), g("k") ** 2 * g("C")), (g("B"), g("k") * g("h"), g("k") * g("w"), g("C"))
        return ([("src", a, dt)], [("dst", b, dt)]) if op == "sc" else ([("src", b, dt)], [("dst", a, dt)])
    if op == "di":
        return [("src", (g("B"), g("h"), g("w"), g("C")), dt)], [("dst", (g("B"), g("H"), g("W"), g("C")), dt)]
    if op == "ps":
        return [("src", (g("B") * g("h") * g("w"), g("C") * g("P") ** 2), dt)], [("dst", (g("B"), g("C"), g("P") * g("h"), g("P") * g("w")), "f")]
    if op == "im":
        return [("src", (g("B"), g("H"), g("W"), g("Cin")), dt)], [("dst", (9 * g("Cin"), g("ld")), dt)]
    inner, outer = (g("B"), g("H"), g("W"), g("C")), (g("B"), g("H") + 2, g("W") + 2, g("C"))
    if op == "pad":
        return [("src", inner, dt)], [("dst", outer, dt)]
    if op == "padb":
        return [("dy", outer, dt)], [("dx", inner, dt)]
    if op == "emb":
        return [("dy", inner, dt)], [("dst", outer, dt)]
    return [("src", outer, dt)] + ([("res", inner, dt)] if g("res") else []), [("dst", inner, dt)]


def outputs(w):
    return tuple(n for n, _, _ in buffers(w)[1])


def _draw(shape, family, g, device, adjoint):
    "One operand of a family in float32: 4-D maps [B, H, W, C] or 2-D [rows, C]."
    shape4 = shape if len(shape) == 4 else (1, shape[0], 1, shape[1])
    B, H, W, C = shape4
    if family == "wide":
        x = 0.5 + 3.0 * torch.randn(shape4, generator=g, device=device)
    elif family == "ramp":
        ar = lambda n, k: torch.arange(n, device=device, dtype=torch.float32).view([n if i == k else 1 for i in range(4)])      # noqa: E731
        x = 2.0 * ar(B, 0) + 0.75 * ar(H, 1) - 0.5 * ar(W, 2) + 0.125 * ar(C, 3) + torch.zeros(shape4, device=device)
    elif adjoint:
        x = torch.zeros(shape4, device=device)
        x[-1, -1, -1, -1] = 1e4
        x[0, H // 2, W // 2, 0] = -3.0
    else:
        x = torch.randn(shape4, generator=g, device=device)
        x[-1, -1, -1, -1] = 1e4
    return x.view(shape)


def make_case(w, family, device, seed=0, window=None):
    """Seeded operands and output buffers of a witness on `device`: t[name] is the shaped view, t[name + "_buf"] the flat banded buffer and
    t[name + "_at"] the view's first element in it.  `window` = (r0, r1) (conv1x1_to4 only): the case holds pixels r0 .. r1 - 1 of the
    witness alone, t["row0"] = r0; the model and the reference index them as the launch would."""
    assert family in FAMILIES
    g = torch.Generator(device=device).manual_seed(9000 + seed)
    nan = float("nan")
    t = {"row0": 0}
    if window is not None:
        assert w["op"] == "c1"
        w = dict(w, rows=window[1] - window[0])
        t["row0"] = window[0]
    ins, outs = buffers(w)
    for name, shape, dt in ins:
        if name == "w":
            x = 0.2 * torch.randn(shape, generator=g, device=device)
        elif name == "bias":
            x = torch.randn(shape, generator=g, device=device)
        else:
            x = _draw(shape, family, g, device, adjoint=w["op"] in ("blb", "padb") and name == "dy")
            if w["op"] == "c1b" and name == "feat":      # exact zeros of both signs under the ReLU mask
                x.view(-1)[0::7] = 0.0
                x.view(-1)[3::7] = -0.0
        off = w.get("mis", 0) if name == "bias" else 0
        buf, at, view = _banded(math.prod(shape), DT[dt], device, nan, x.to(DT[dt]).flatten(), off=off)
        t[name + "_buf"], t[name + "_at"], t[name] = buf, at, view.view(shape)
    for name, shape, dt in outs:
        fill = nan
        if name in ("dw", "db"):
            fill = (0.5 + torch.rand(shape, generator=g, device=device)).flatten() * (1.0 if name == "dw" else -1.0)
            t["pre_" + name] = fill.view(shape).clone()
        buf, at, view = _banded(math.prod(shape), DT[dt], device, SENTINEL, fill)
        t[name + "_buf"], t[name + "_at"], t[name] = buf, at, view.view(shape)
    return t


def results(w, t, bufs=None):
    "{output: tensor} of what a launch (or `model`: bufs) left; dw / db as target - prefill in float64."
    out = {}
    for name in outputs(w):
        shape = tuple(t[name].shape)
        v = t[name] if bufs is None else bufs[name][t[name + "_at"]:t[name + "_at"] + t[name].numel()].view(shape)
        out[name] = v.double() - t["pre_" + name].double() if name in ("dw", "db") else v
    return out


def bands_ok(w, t, bufs=None):
    "Whether the sentinel bands around every output are untouched."
    return all(bands_untouched(t[n + "_buf"] if bufs is None else bufs[n], t[n + "_at"], t[n].numel()) for n in outputs(w))


# ------------------------------------------------------------------------------------------ reference and bound
def taps_exact(rule, n_in, n_out, n_used):
    "(i0, i1, lambda in float64, the a-priori error of the fp32 coordinate) of destination indices 0 .. n_used - 1, in integers."
    o = torch.arange(n_used, dtype=torch.int64)
    if rule == "ac":
        den = max(n_out - 1, 1)
        num = (n_in - 1) * o if n_out > 1 else 0 * o
        delta = 2.0 ** -23 * num.double() / den
    else:
        den = 2 * n_out
        num = ((2 * o + 1) * n_in - n_out).clamp(min=0)
        delta = torch.full((n_used,), U24, dtype=torch.float64)
    i0 = num // den
    return i0, (i0 + 1).clamp(max=n_in - 1), (num - i0 * den).double() / den, delta


def _weights64(rule, n_in, n_out, n_used):
    "[n_in, n_used] float64: the weight of input i in output o; the coordinate error of o where o lies within one input pixel of i, else 0."
    i0, i1, lam, delta = taps_exact(rule, n_in, n_out, n_used)
    i = torch.arange(n_in)[:, None]
    Wm = (i0[None] == i) * (1.0 - lam)[None] + (i1[None] == i) * lam[None]
    coord = i0.double() + lam
    reach = ((coord[None] - i).abs() < 1.0 + 1e-3) | (Wm != 0)
    return Wm, reach * delta[None], reach


def _store_term(ref, code):
    u = U_OUT[code] * ref.abs()
    return u.clamp(min=2.0 ** -25) if code == F16 else u


def _ref_bl(w, src):
    "Forward resize of src [B, Hi, Wi, C] in float64: (ref, bound)."
    x = src.double()
    dev = x.device
    Hi, Wi = w["Hi"], w["Wi"]
    y0, y1, ly, dy = (v.to(dev) for v in taps_exact(w["rule"], Hi, w["Ho"], w["ch"]))
    x0, x1, lx, dx = (v.to(dev) for v in taps_exact(w["rule"], Wi, w["Wo"], w["cw"]))
    ly, lx, dy, dx = ly[None, :, None, None], lx[None, None, :, None], dy[None, :, None, None], dx[None, None, :, None]

    def interp(p):
        g = lambda yy, xx: p[:, yy][:, :, xx]      # noqa: E731
        return (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))
    ref, S = interp(x), interp(x.abs())
    # the largest |difference| of adjacent samples over the cell and its neighbour cells
    dv = (x[:, 1:] - x[:, :-1]).abs() if Hi > 1 else torch.zeros_like(x[:, :1])
    dh = (x[:, :, 1:] - x[:, :, :-1]).abs() if Wi > 1 else torch.zeros_like(x[:, :, :1])
    Dy, Dx = torch.zeros_like(ref), torch.zeros_like(ref)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1, 2):
            Dy = torch.maximum(Dy, dv[:, (y0 + a).clamp(0, dv.shape[1] - 1)][:, :, (x0 + b).clamp(0, Wi - 1)])
            Dx = torch.maximum(Dx, dh[:, (y0 + b).clamp(0, Hi - 1)][:, :, (x0 + a).clamp(0, dh.shape[2] - 1)])
    return ref, _store_term(ref, CODE[w["dt"]]) + ACC * 2.0 * S + dy * Dy + dx * Dx


def _ref_blb(w, g):
    "Adjoint resize of dy [B, ch, cw, C] in float64: (ref, bound); bound 0 (exactly 0) where no output is in reach."
    g = g.double()
    dev = g.device
    Wy, Ey, Ry = (v.to(dev).double() for v in _weights64(w["rule"], w["Hi"], w["Ho"], w["ch"]))
    Wx, Ex, Rx = (v.to(dev).double() for v in _weights64(w["rule"], w["Wi"], w["Wo"], w["cw"]))
    e = lambda a, b, v: torch.einsum("yo,xp,bopc->byxc", a, b, v)      # noqa: E731
    ref, S = e(Wy, Wx, g), e(Wy, Wx, g.abs())
    n_taps = (Wy != 0).sum(1).double()[None, :, None, None] * (Wx != 0).sum(1).double()[None, None, :, None]
    coord = e(Ey, Rx, g.abs()) + e(Ry, Ex, g.abs())
    return ref, _store_term(ref, CODE[w["dt"]]) * (S > 0) + ACC * n_taps.sqrt() * S + coord


def _pad_index(w, dev):
    "Flat index into [H, W] of every position of the padded [H + 2, W + 2] map."
    H, W = w["H"], w["W"]
    yy = (torch.arange(H + 2, device=dev) - 1).clamp(0, H - 1)
    xx = (torch.arange(W + 2, device=dev) - 1).clamp(0, W - 1)
    return yy, xx


def reference(w, t):
    "{output: (ref, bound)} in float64 on the device of the case; bound 0: exact."
    op, code = w["op"], CODE[w["dt"]]
    z = lambda r: (r, torch.zeros_like(r))      # noqa: E731
    if op == "bl":
        return {"dst": _ref_bl(w, t["src"])}
    if op == "blb":
        return {"dx": _ref_blb(w, t["dy"])}
    if op == "c1":
        return {"out": reference_c1(w, t["feat"], t["w"], t["bias"])}
    if op == "c1b":
        f, wt, g = t["feat"].double(), t["w"].double(), t["dout"].double()
        d, Sd = g @ wt, g.abs() @ wt.abs()
        if w["relu"]:
            d, Sd = d * (f > 0), Sd * (f > 0)
        pre = ACC * math.sqrt(grid_of(w))
        dw, db = g.t() @ f, g.sum(0)
        n = math.sqrt(w["npix"])
        return {"dfeat": (d, _store_term(d, code) * (Sd > 0) + ACC * 2.0 * Sd),
                "dw": (dw, U24 * dw.abs() + ACC * n * (g.abs().t() @ f.abs()) + pre * t["pre_dw"].double().abs()),
                "db": (db, U24 * db.abs() + ACC * n * g.abs().sum(0) + pre * t["pre_db"].double().abs())}
    if op in ("sc", "ga"):
        B, h, ww, k, C = (w[x] for x in ("B", "h", "w", "k", "C"))
        x = t["src"].double()
        if op == "sc":
            return {"dst": z(x.view(B, h, ww, k, k, C).permute(0, 1, 3, 2, 4, 5).reshape(B, k * h, k * ww, C))}
        return {"dst": z(x.view(B, h, k, ww, k, C).permute(0, 1, 3, 2, 4, 5).reshape(B * h * ww, k * k * C))}
    if op == "di":
        r = torch.zeros(t["dst"].shape, dtype=torch.float64, device=t["src"].device)
        r[:, ::2, ::2] = t["src"].double()[:, :(w["H"] + 1) // 2, :(w["W"] + 1) // 2]
        return {"dst": z(r)}
    if op == "ps":
        B, h, ww, P, C = (w[x] for x in ("B", "h", "w", "P", "C"))
        return {"dst": z(t["src"].double().view(B, h, ww, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, C, P * h, P * ww))}
    if op == "im":
        x = t["src"].double()
        if w["relu"]:
            x = x.clamp(min=0) + 0.0
        B, H, W, Cin, s = (w[k] for k in ("B", "H", "W", "Cin", "stride"))
        xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float64, device=x.device)
        xp[:, 1:-1, 1:-1] = x
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        r = torch.zeros(9, Cin, w["ld"], dtype=torch.float64, device=x.device)
        for ky in range(3):
            for kx in range(3):
                r[ky * 3 + kx, :, :w["npix"]] = xp[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s].reshape(-1, Cin).t()
        return {"dst": z(r.view(9 * Cin, w["ld"]))}
    if op == "pad":
        yy, xx = _pad_index(w, t["src"].device)
        return {"dst": z(t["src"].double()[:, yy][:, :, xx])}
    if op == "emb":
        r = torch.zeros(t["dst"].shape, dtype=torch.float64, device=t["dy"].device)
        r[:, 1:-1, 1:-1] = t["dy"].double()
        return {"dst": z(r)}
    if op == "padb":
        g = t["dy"].double()
        yy, xx = _pad_index(w, g.device)
        My = (yy[None] == torch.arange(w["H"], device=g.device)[:, None]).double()
        Mx = (xx[None] == torch.arange(w["W"], device=g.device)[:, None]).double()
        e = lambda v: torch.einsum("yo,xp,bopc->byxc", My, Mx, v)      # noqa: E731
        ref, S = e(g), e(g.abs())
        n = (My.sum(1)[None, :, None, None] * Mx.sum(1)[None, None, :, None]).expand_as(ref)
        return {"dx": (ref, torch.where(n > 1, _store_term(ref, code) + n * U24 * S, torch.zeros_like(ref)))}
    x = t["src"].double()[:, 1:-1, 1:-1]      # cadd
    S = x.abs()
    if w["res"]:
        x, S = x + t["res"].double(), S + t["res"].double().abs()
    if w["relu"]:
        x = x.clamp(min=0) + 0.0
    return {"dst": (x, (_store_term(x, code) + 2 * U24 * S) if w["res"] else torch.zeros_like(x))}


def reference_c1(w, feat, wt, bias):
    "(ref, bound) of uc_conv1x1_to4 on the rows of feat given (the whole witness, or a chunk of its pixels)."
    f, wt, b = feat.double(), wt.double(), bias.double()
    ref, S = f @ wt.t() + b, f.abs() @ wt.abs().t() + b.abs()
    return ref, U24 * ref.abs() + ACC * math.sqrt(w["Cin"] + 1) * S


def unstored(ref, bnd, code):
    "The bound in front of a store of dtype `code`: the store's own rounding replaced by fp32's, where the bound is not 0."
    return torch.where(bnd > 0, bnd - _store_term(ref, code) + U24 * ref.abs(), bnd)


def store_code(w, o):
    return CODE[w["dt"]] if o in ("dst", "dx", "dfeat") and w["op"] != "ps" else F32


def reference_elems(w):
    "fp64 multiply-adds of reference and bound together, to an order of magnitude: what REF_BUDGET_ELEMS limits."
    ins, outs = buffers(w)
    n = sum(math.prod(s) for _, s, _ in ins + outs)
    if w["op"] == "blb":
        n += 4 * w["B"] * w["C"] * w["Hi"] * w["cw"] * (w["ch"] + w["Wi"])      # four separable contractions: rows, then columns
    if w["op"] == "bl":
        n += 40 * math.prod(outs[0][1])
    if w["op"] in ("c1", "c1b"):
        n += 16 * w["npix"] * w["Cin"]
    return n


# ------------------------------------------------------------------------------------------ model
# defect -> the operations it belongs to.  What each one is, in the kernels' terms:
#   second_x_block_unwritten      bilinear forward: work items t >= 256 of an output row return early
#   ragged_row_group_unwritten    rows kernel: the rows of a last group shorter than R are not stored (`if (oy + k >= ch) break` one group early)
#   row_group_picks_next_row      rows kernel: `rel == i ? h[i + 1]` for the top row (and h[i + 2] for the bottom one)
#   x1_unclamped                  `x1 = x0 + 1` without `min(.., Wi - 1)`: the last column reads the next row, or past the map
#   dst_batch_stride_from_Ho      the destination's image stride from Ho instead of crop_h
#   scale_in_over_out             `in / out` for `(in - 1) / (out - 1)`
#   ly_hy_swapped                 the vertical weights exchanged
#   range_without_margin          tap_range / halfpix_range from the input index itself: no +-1 input pixel, no +-1 / +-2 output
#   clamped_tap_dropped           an output whose second tap is clamped to the last row / column (i0 + 1 > in - 1) is skipped
#   crop_strides_from_Ho          the adjoint reads dy with the strides of the uncropped map
#   negative_coordinate_unclamped halfpix_tap without `num <= 0`: C's division truncates towards zero, lambda goes negative
#   i1_unclamped                  halfpix_tap without `min(i0 + 1, in - 1)`
#   bias_dropped / fold_stops_one_step_early (`off > 1`) / second_stride_iteration_dropped (`if` for `for`)
#   mask_ge_zero (`f >= 0`) / db_from_every_chunk (without `chunk == 0`) / dead_thread_counted (without `live`)
#   pad_columns_unwritten (`p < npix` at the store) / ky_kx_swapped / relu_skipped
#   odd_edge_row_dropped          dilate: `Y / s < H / s` for `Y / s < h`: the last source row / column of an odd map is lost
#   corner_counted_once           pad adjoint: a corner pixel leaves out the padded map's own corner position
DEFECTS = {"second_x_block_unwritten": ("bl",), "ragged_row_group_unwritten": ("bl",), "row_group_picks_next_row": ("bl",), "x1_unclamped": ("bl",),
           "dst_batch_stride_from_Ho": ("bl",), "scale_in_over_out": ("bl",), "ly_hy_swapped": ("bl",),
           "range_without_margin": ("blb",), "clamped_tap_dropped": ("blb",), "crop_strides_from_Ho": ("blb",),
           "negative_coordinate_unclamped": ("bl", "blb"), "i1_unclamped": ("bl", "blb"),
           "bias_dropped": ("c1",), "fold_stops_one_step_early": ("c1",), "second_stride_iteration_dropped": ("c1", "c1b"),
           "mask_ge_zero": ("c1b",), "db_from_every_chunk": ("c1b",), "dead_thread_counted": ("c1b",),
           "pad_columns_unwritten": ("im",), "ky_kx_swapped": ("im",), "relu_skipped": ("im",),
           "odd_edge_row_dropped": ("di",), "corner_counted_once": ("padb",)}
HALFPIX_ONLY = ("negative_coordinate_unclamped", "i1_unclamped")


def _fetch(t, name, idx):
    "What loads at element offsets idx from the operand's first element return: the flat banded buffer, NaN beyond it."
    flat = t[name + "_buf"].float()
    at = t[name + "_at"] + idx
    ok = (at >= 0) & (at < flat.numel())
    return torch.where(ok, flat[at.clamp(0, flat.numel() - 1)], torch.full((), float("nan")))


def _emit(bufs, t, name, idx, val, keep=None):
    "Stores of val at element offsets idx from the output's first element into the model's copy of the flat buffer."
    buf = bufs[name]
    at = (t[name + "_at"] + idx).flatten()
    ok = (at >= 0) & (at < buf.numel())
    if keep is not None:
        ok &= keep.expand(idx.shape).flatten()
    buf[at[ok]] = val.expand(idx.shape).flatten()[ok].to(buf.dtype)


def taps_model(w, axis, defect):
    "(i0, i1, lambda) of the kernels in float32 / int for destination indices 0 .. used - 1 of an axis (0: rows, 1: columns)."
    n_in, n_out, used = (w["Hi"], w["Ho"], w["ch"]) if axis == 0 else (w["Wi"], w["Wo"], w["cw"])
    o = torch.arange(used, dtype=torch.int64)
    if w["rule"] == "ac":
        s = torch.tensor(float(n_in)) / torch.tensor(float(n_out)) if defect == "scale_in_over_out" else torch.tensor(scale32(n_in, n_out))
        f = s * o.float()
        i0 = f.to(torch.int64)
        lam = f - i0.float()
        unclamped = defect == "x1_unclamped" and axis == 1
    else:
        num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
        if defect != "negative_coordinate_unclamped":
            num = num.clamp(min=0)
        i0 = torch.div(num, den, rounding_mode="trunc")
        lam = (num - i0 * den).float() / torch.tensor(float(den))
        unclamped = defect == "i1_unclamped"
    return i0, i0 + 1 if unclamped else (i0 + 1).clamp(max=n_in - 1), lam, s if w["rule"] == "ac" else None


def _model_bl(w, t, bufs, defect):
    B, Hi, Wi, C, ch, cw = (w[k] for k in ("B", "Hi", "Wi", "C", "ch", "cw"))
    y0, y1, ly, sy = taps_model(w, 0, defect)
    x0, x1, lx, _ = taps_model(w, 1, defect)
    kernel, R = bl_kernel(w)
    oy = torch.arange(ch)
    if kernel == "rows":      # the group's first row fixes ya; the rows come from h[rel], h[rel + 1], rows ya + i clamped to the last one
        rin = R // 2 + 2
        ya = (sy * ((oy // R) * R).float()).to(torch.int64)
        rel = y0 - ya
        sel = torch.where((rel >= 1) & (rel <= rin - 2), rel, torch.zeros_like(rel))
        if defect == "row_group_picks_next_row":
            sel = sel + 1
        y0, y1 = (ya + sel).clamp(max=Hi - 1), (ya + sel + 1).clamp(max=Hi - 1)
    if defect == "ly_hy_swapped":
        ly = 1.0 - ly
    b, c = torch.arange(B).view(B, 1, 1, 1), torch.arange(C).view(1, 1, 1, C)
    Y0, Y1, X0, X1 = y0.view(1, ch, 1, 1), y1.view(1, ch, 1, 1), x0.view(1, 1, cw, 1), x1.view(1, 1, cw, 1)
    ld = lambda yy, xx: _fetch(t, "src", ((b * Hi + yy) * Wi + xx) * C + c)      # noqa: E731
    ly, lx = ly.view(1, ch, 1, 1), lx.view(1, 1, cw, 1)
    hy, hx = 1.0 - ly, 1.0 - lx
    val = hy * (hx * ld(Y0, X0) + lx * ld(Y0, X1)) + ly * (hx * ld(Y1, X0) + lx * ld(Y1, X1))
    OY, OX = oy.view(1, ch, 1, 1), torch.arange(cw).view(1, 1, cw, 1)
    idx = ((b * (w["Ho"] if defect == "dst_batch_stride_from_Ho" else ch) + OY) * cw + OX) * C + c
    keep = None
    if defect == "second_x_block_unwritten":
        keep = (OX * (C // 8) + c // 8) < WG
    if defect == "ragged_row_group_unwritten" and kernel == "rows":
        keep = OY < (ch // R) * R
    _emit(bufs, t, "dst", idx + 0 * OX, val, None if keep is None else keep.expand(B, ch, cw, C))


def _range_model(w, axis, defect):
    "[n_in, used] bool: the destination indices the adjoint kernel visits for every source index."
    n_in, n_out, used = (w["Hi"], w["Ho"], w["ch"]) if axis == 0 else (w["Wi"], w["Wo"], w["cw"])
    i = torch.arange(n_in)
    m = 0 if defect == "range_without_margin" else 1
    if w["rule"] == "ac":
        s = torch.tensor(scale32(n_in, n_out))
        if float(s) <= 0:
            lo, hi = torch.zeros_like(i), torch.full_like(i, used - 1)
        else:
            lo = (torch.floor((i - m).float() / s).to(torch.int64) - m).clamp(min=0)
            hi = (torch.ceil((i + m).float() / s).to(torch.int64) + m).clamp(max=used - 1)
    else:
        lo = (torch.div((i - m) * n_out, n_in, rounding_mode="trunc") - 2 * m).clamp(min=0)
        hi = (torch.div((i + 1 + m) * n_out, n_in, rounding_mode="trunc") + 2 * m).clamp(max=used - 1)
    o = torch.arange(used)[None]
    return (o >= lo[:, None]) & (o <= hi[:, None])


def _model_blb(w, t, bufs, defect):
    B, Hi, Wi, C, ch, cw = (w[k] for k in ("B", "Hi", "Wi", "C", "ch", "cw"))

    def weights(axis):
        n_in = Hi if axis == 0 else Wi
        i0, i1, lam, _ = taps_model(w, axis, defect)
        i = torch.arange(n_in)[:, None]
        Wm = (i0[None] == i) * (1.0 - lam)[None] + (i1[None] == i) * lam[None]
        if defect == "clamped_tap_dropped":
            Wm = Wm * (i0 + 1 <= n_in - 1)[None]
        return (Wm * _range_model(w, axis, defect)).float()
    Wy, Wx = weights(0), weights(1)
    b, c = torch.arange(B).view(B, 1, 1, 1), torch.arange(C).view(1, 1, 1, C)
    sh, sw = (w["Ho"], w["Wo"]) if defect == "crop_strides_from_Ho" else (ch, cw)
    G = _fetch(t, "dy", ((b * sh + torch.arange(ch).view(1, ch, 1, 1)) * sw + torch.arange(cw).view(1, 1, cw, 1)) * C + c)
    e = lambda a, bb, v: torch.einsum("yo,xp,bopc->byxc", a, bb, v)      # noqa: E731
    val = e(Wy, Wx, torch.nan_to_num(G, nan=0.0))
    loaded_nan = e((Wy != 0).float(), (Wx != 0).float(), torch.isnan(G).float()) > 0      # a zero weight skips the load: no 0 * NaN
    val = torch.where(loaded_nan, torch.full((), float("nan")), val)
    _emit(bufs, t, "dx", torch.arange(B * Hi * Wi * C).view(B, Hi, Wi, C), val)


def _model_c1(w, t, bufs, defect):
    Cin, n = w["Cin"], t["feat"].shape[0]
    kernel, c8 = c1_kernel(w)
    pix = t["row0"] + torch.arange(n)
    f = _fetch(t, "feat", torch.arange(n * Cin).view(n, Cin))
    wt = _fetch(t, "w", torch.arange(4 * Cin).view(4, Cin))
    bias = torch.zeros(4) if defect == "bias_dropped" else _fetch(t, "bias", torch.arange(4))
    if kernel == "coop":
        part = (f.view(n, 1, c8, 8) * wt.view(1, 4, c8, 8)).sum(3)      # [n, 4, c8]: every lane's partial sum
        off = c8 // 2
        while off > (1 if defect == "fold_stops_one_step_early" else 0):
            part = part + part[:, :, torch.arange(c8) ^ off]
            off //= 2
        val = part[:, :, 0] + bias
        per = WG // c8
    else:
        val = bias + (f[:, None, :] * wt[None]).sum(2)
        per = WG
    keep = (pix < grid_of(w) * per).view(n, 1) if defect == "second_stride_iteration_dropped" else None
    _emit(bufs, t, "out", torch.arange(n * 4).view(n, 4), val, keep)


def _model_c1b(w, t, bufs, defect):
    Cin, n, C8 = w["Cin"], w["npix"], w["Cin"] // 8
    lanes, grid = lanes_of(Cin), grid_of(w)
    f = _fetch(t, "feat", torch.arange(n * Cin).view(n, Cin))
    wt = _fetch(t, "w", torch.arange(4 * Cin).view(4, Cin))
    g = _fetch(t, "dout", torch.arange(n * 4).view(n, 4))
    done = torch.arange(n) < grid * lanes if defect == "second_stride_iteration_dropped" else torch.ones(n, dtype=torch.bool)
    d = ((g[:, 0:1] * wt[0:1] + g[:, 1:2] * wt[1:2]) + g[:, 2:3] * wt[2:3]) + g[:, 3:4] * wt[3:4]
    if w["relu"]:
        d = torch.where((f >= 0) if defect == "mask_ge_zero" else (f > 0), d, torch.zeros(()))
    _emit(bufs, t, "dfeat", torch.arange(n * Cin).view(n, Cin), d, done.view(n, 1))
    gd, fd = g * done[:, None], f * done[:, None]
    dw, db = gd.t() @ fd, gd.sum(0) * (C8 if defect == "db_from_every_chunk" else 1)
    if defect == "dead_thread_counted":      # threads lanes * C8 .. 255: pixel lane `lanes` = the next workgroup's first pixel, once more
        for thread in range(lanes * C8, WG):
            chunk, pl = thread % C8, thread // C8
            p = (torch.arange(grid)[:, None] * lanes + pl + torch.arange(-(-n // (grid * lanes)))[None] * grid * lanes).flatten()
            p = p[p < n]
            dw[:, chunk * 8:chunk * 8 + 8] += g[p].t() @ f[p, chunk * 8:chunk * 8 + 8]
            if chunk == 0:
                db += g[p].sum(0)
    _emit(bufs, t, "dw", torch.arange(4 * Cin).view(4, Cin), t["pre_dw"] + dw)
    _emit(bufs, t, "db", torch.arange(4), t["pre_db"] + db)


def _model_moves(w, t, bufs, defect):
    op = w["op"]
    g = w.get
    if op in ("sc", "ga"):
        B, h, ww, k, C = g("B"), g("h"), g("w"), g("k"), g("C")
        it = torch.arange(B * k * h * k * ww * C)
        cc, r = it % C, it // C
        X, r = r % (k * ww), r // (k * ww)
        Y, b = r % (k * h), r // (k * h)
        row = ((b * h + Y // k) * ww + X // k) * (k * k * C) + ((Y % k) * k + X % k) * C + cc
        if op == "sc":
            _emit(bufs, t, "dst", it, _fetch(t, "src", row))
        else:
            _emit(bufs, t, "dst", row, _fetch(t, "src", it))
    elif op == "di":
        B, h, ww, H, W, C, s = g("B"), g("h"), g("w"), g("H"), g("W"), g("C"), g("s")
        it = torch.arange(B * H * W * C)
        cc, r = it % C, it // C
        X, r = r % W, r // W
        Y, b = r % H, r // H
        hh, wl = (H // s, W // s) if defect == "odd_edge_row_dropped" else (h, ww)
        ok = (Y % s == 0) & (X % s == 0) & (Y // s < hh) & (X // s < wl)
        v = _fetch(t, "src", (((b * h + Y // s) * ww + X // s) * C + cc) * ok)
        _emit(bufs, t, "dst", it, torch.where(ok, v, torch.zeros(())))
    elif op == "ps":
        B, h, ww, P, C = g("B"), g("h"), g("w"), g("P"), g("C")
        it = torch.arange(B * C * P * h * P * ww)
        X, r = it % (P * ww), it // (P * ww)
        Y, r = r % (P * h), r // (P * h)
        cc, b = r % C, r // C
        _emit(bufs, t, "dst", it, _fetch(t, "src", ((b * h + Y // P) * ww + X // P) * (C * P * P) + cc * P * P + (Y % P) * P + X % P))
    elif op == "im":
        B, H, W, Cin, s, ld, npix = g("B"), g("H"), g("W"), g("Cin"), g("stride"), g("ld"), g("npix")
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        tap, c, p = torch.arange(9).view(9, 1, 1), torch.arange(Cin).view(1, Cin, 1), torch.arange(ld).view(1, 1, ld)
        ky, kx = (tap % 3, tap // 3) if defect == "ky_kx_swapped" else (tap // 3, tap % 3)
        ox, oy, b = p % Wo, (p // Wo) % Ho, p // (Wo * Ho)
        iy, ix = oy * s - 1 + ky, ox * s - 1 + kx
        ok = (p < npix) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        v = _fetch(t, "src", ((((b * H + iy) * W + ix) * Cin + c) * ok).expand(9, Cin, ld))
        if w["relu"] and defect != "relu_skipped":
            v = v.clamp(min=0)
        keep = (p < npix).expand(9, Cin, ld) if defect == "pad_columns_unwritten" else None
        _emit(bufs, t, "dst", ((tap * Cin + c) * ld + p), torch.where(ok.expand(9, Cin, ld), v, torch.zeros(())), keep)
    else:
        B, H, W, C = g("B"), g("H"), g("W"), g("C")
        Hd, Wd = (H + 2, W + 2) if op in ("pad", "emb") else (H, W)
        it = torch.arange(B * Hd * Wd * C)
        cc, r = it % C, it // C
        X, r = r % Wd, r // Wd
        Y, b = r % Hd, r // Hd
        if op == "pad":
            v = _fetch(t, "src", ((b * H + (Y - 1).clamp(0, H - 1)) * W + (X - 1).clamp(0, W - 1)) * C + cc)
        elif op == "emb":
            ok = (Y >= 1) & (Y <= H) & (X >= 1) & (X <= W)
            v = torch.where(ok, _fetch(t, "dy", (((b * H + Y - 1) * W + X - 1) * C + cc) * ok), torch.zeros(()))
        elif op == "cadd":
            v = _fetch(t, "src", ((b * (H + 2) + Y + 1) * (W + 2) + X + 1) * C + cc)
            if g("res"):
                v = v + _fetch(t, "res", it)
            if g("relu"):
                v = v.clamp(min=0)
        else:      # padb: rows ascending, then columns ascending
            y0, y1 = torch.where(Y == 0, 0, Y + 1), torch.where(Y == H - 1, H + 1, Y + 1)
            x0, x1 = torch.where(X == 0, 0, X + 1), torch.where(X == W - 1, W + 1, X + 1)
            v = torch.zeros(it.shape)
            for a in range(3):
                for bb in range(3):
                    yy, xx = y0 + a, x0 + bb
                    ok = (yy <= y1) & (xx <= x1)
                    if defect == "corner_counted_once":
                        ok &= ~(((yy == 0) | (yy == H + 1)) & ((xx == 0) | (xx == W + 1)))
                    v = v + torch.where(ok, _fetch(t, "dy", (((b * (H + 2) + yy) * (W + 2) + xx) * C + cc) * ok), torch.zeros(()))
        _emit(bufs, t, outputs(w)[0], it, v)


def model(w, t, defect=None, store=True):
    """The kernels' arithmetic in float32 torch on CPU tensors, every operand fetched from and every result stored into the flat banded
    buffers by the kernels' index arithmetic; stores rounded to the output dtype (`store=False`: kept in float32).  `defect`: one of
    DEFECTS.  Returns {output: the flat buffer after the launch} for `results` / `bands_ok`."""
    assert defect is None or (w["op"] in DEFECTS[defect] and (defect not in HALFPIX_ONLY or w["rule"] == "hp")), (defect, w["name"])
    bufs = {n: t[n + "_buf"].clone() if store else t[n + "_buf"].to(torch.float32, copy=True) for n in outputs(w)}
    {"bl": _model_bl, "blb": _model_blb, "c1": _model_c1, "c1b": _model_c1b}.get(w["op"], _model_moves)(w, t, bufs, defect)
    return bufs


# ------------------------------------------------------------------------------------------ launching (the GPU test file and the child)
def launch(lib, w, t, stream, **over):
    "One call of the witness's entry point on the case's buffers; the status.  `over` replaces arguments by name."
    p = lambda n: over.get(n, t[n].data_ptr() if n in t else None)      # noqa: E731
    g = lambda k: over.get(k, w.get(k))      # noqa: E731
    code, op = over.get("dtype", CODE[w["dt"]]), w["op"]
    if op in ("bl", "blb"):
        a, b = (p("src"), p("dst")) if op == "bl" else (p("dy"), p("dx"))
        sfx = "" if op == "bl" else "_bwd"
        if g("entry") == "resize":
            return getattr(lib, "uc_resize_bilinear_nhwc" + sfx)(a, b, code, g("B"), g("Hi"), g("Wi"), g("C"), g("Ho"), g("Wo"), int(g("rule") == "ac"), stream)
        return getattr(lib, "uc_bilinear_nhwc" + sfx)(a, b, code, g("B"), g("Hi"), g("Wi"), g("C"), g("Ho"), g("Wo"), g("ch"), g("cw"), stream)
    if op == "c1":
        return lib.uc_conv1x1_to4(p("feat"), code, p("w"), p("bias"), p("out"), g("npix"), g("Cin"), stream)
    if op == "c1b":
        return lib.uc_conv1x1_to4_bwd(p("feat"), code, p("w"), p("dout"), p("dfeat"), p("dw"), p("db"), g("npix"), g("Cin"), g("relu"), stream)
    if op in ("sc", "ga"):
        return getattr(lib, "uc_convt_scatter" if op == "sc" else "uc_convt_gather")(p("src"), p("dst"), code, g("B"), g("h"), g("w"), g("k"), g("C"), stream)
    if op == "di":
        return lib.uc_dilate_nhwc(p("src"), p("dst"), code, g("B"), g("h"), g("w"), g("H"), g("W"), g("C"), g("s"), stream)
    if op == "ps":
        return lib.uc_pixel_shuffle(p("src"), code, p("dst"), g("B"), g("h"), g("w"), g("P"), g("C"), stream)
    if op == "im":
        return lib.uc_im2col_t(p("src"), p("dst"), code, g("B"), g("H"), g("W"), g("Cin"), g("stride"), g("relu"), g("ld"), stream)
    if op == "pad":
        return lib.uc_replicate_pad_nhwc(p("src"), p("dst"), code, g("B"), g("H"), g("W"), g("C"), stream)
    if op == "padb":
        return lib.uc_replicate_pad_nhwc_bwd(p("dy"), p("dx"), code, g("B"), g("H"), g("W"), g("C"), stream)
    if op == "emb":
        return lib.uc_crop_embed_nhwc(p("dy"), p("dst"), code, g("B"), g("H"), g("W"), g("C"), stream)
    return lib.uc_crop_add_nhwc(p("src"), p("res") if g("res") else None, p("dst"), code, g("B"), g("H"), g("W"), g("C"), g("relu"), stream)


def run_on_device(lib, w, family, device, plan=None, chunk=1 << 15):
    """Launch the witness on one input family and measure everything: {route: the driver's line for the pointers the launch got (None:
    no plan), status, bands, worst: {output: err / bound}, over: elements over the bound, first: the text of the first failure}."""
    t = make_case(w, family, device, seed=seed_of(w))
    line = plan([driver_row(w, t["bias"].data_ptr() if "bias" in t else None)])[0] if plan is not None and planned(w) else None
    status = launch(lib, w, t, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rec = dict(name=w["name"], family=family, route=line, status=status, bands=bands_ok(w, t), worst={}, over=0, first=None, case=t)
    got = results(w, t)
    label = f"{w['name']} ({family}): {route(w)}"

    def one(o, g, ref, bnd, at=""):
        worst, bad, _ = ratio(g, ref, bnd)
        rec["worst"][o] = max(rec["worst"].get(o, 0.0), worst)
        rec["over"] += bad
        if bad and rec["first"] is None:
            try:
                check(label + at, o, g.reshape(-1, g.shape[-1]), ref.reshape(-1, ref.shape[-1]), bnd.reshape(-1, bnd.shape[-1]))
            except AssertionError as e:
                rec["first"] = str(e)
    if w["op"] == "c1" and w["big"]:      # the reference in row chunks
        for r0 in range(0, w["npix"], chunk):
            r1 = min(w["npix"], r0 + chunk)
            one("out", got["out"][r0:r1], *reference_c1(w, t["feat"][r0:r1], t["w"], t["bias"]), at=f" rows {r0}..")
    else:
        ref = reference(w, t)
        for o in outputs(w):
            one(o, got[o], *ref[o])
        rec["ref"] = ref
    return rec


def bilinear_child():
    "The child of the UC_BILINEAR_ROWS2 tests: asserts the knob, runs its bilinear forward witnesses, prints one JSON line per witness."
    import ctypes
    import tempfile

    from uniception_amd import _lib
    lib = _lib.load()
    rows2 = int(os.environ["UC_BILINEAR_ROWS2"])
    v = ctypes.c_int(-99)
    assert lib.uc_tuning_get(b"bilinear_rows2", ctypes.byref(v)) == 0 and v.value == rows2, (v.value, rows2)
    device = torch.device("cuda")
    with tempfile.TemporaryDirectory() as tmp:
        plan = build_driver(tmp)
        for n in knob_witnesses(rows2):
            w = WITNESSES[n]
            for family in FAMILIES:
                rec = run_on_device(lib, w, family, device, plan)
                print(json.dumps(dict(name=n, family=family, route=rec["route"], status=rec["status"], bands=rec["bands"], over=rec["over"],
                                      worst=rec["worst"]["dst"], first=rec["first"], bits=_bits_hex(rec["case"]["dst"]))), flush=True)


def _bits_hex(x):
    "A digest of a tensor's bits: whether R = 2, R = 4 and the one-row kernel agree bit for bit is printed, not asserted."
    import hashlib
    return hashlib.sha1(x.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:16]


if __name__ == "__main__":
    if "--bilinear-child" in sys.argv:
        bilinear_child()
        sys.exit(0)
    print(f"{len(WITNESSES)} witnesses ({len(SMALL)} small x {len(FAMILIES)} input families, {len(BIG)} big), {len({route(w) for w in WITNESSES.values()})} routes")
    for n, w in WITNESSES.items():
        print(f"  {n:44s} [{route(w)}]" + (f"  plan [{expected_plan(w)}]" if planned(w) else ""))
