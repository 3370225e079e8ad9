"""Route audit of uc_layernorm / uc_layernorm_twin (uniception_amd/csrc/rope_norm.hip) and uc_layernorm_bwd (csrc/train.hip): routes, witness
shapes, operands inside guard bands, the fp64 reference, the per-element bound and a CPU model of the kernel arithmetic that can be given the
defects these kernels can have.

ROUTES.  A route is everything that selects device code: (direction, kernel, nv, nt, x dtype, y / dy dtype, twin, dres).  The kernel, nv and
nt come from uniception_amd/csrc/layernorm_plan.h (checked through tests/layernorm_plan_driver.cpp), the dtypes pick the template instance,
twin and dres are run-time branches inside every kernel.
  forward   exact (nv 1 2 3 4 6 8, nt 0 | 1) | vec | scalar      x f32 | bf16 -> y f32 | bf16, twin (a bf16 copy of y) on | off
  backward  wide (nv 1 2 3 4 6 8) | c64 | generic                x (= dres = dx) f32 | bf16, dy f32 | bf16, dres on | off, twin (dx_bf16, fp32
                                                                 stream only) on | off; c64 has neither dres nor twin

WITNESSES (`WITNESSES`, built by the loops below them; `python -m tests.layernorm_routes` prints the table).  Each is the smallest shape
that still exercises what its kernel can get wrong.
  forward, rows in {1, 5, 9} (four rows per workgroup: one ragged workgroup, two, three), rotated over the combinations:
    exact    every nv x 4 dtype pairs x twin on / off
    vec      C = 4 (one lane), 64 (a quarter wave of one chunk), 80, 96 (the qk-norm widths), 100, 1280 and 1792 (multiples of 256 without
             an exact instance: the fall-through), 2044 (the last chunk partial); 4 dtype pairs each, twin alternating
    scalar   C = 1, 67, 2052 (above the register cap); C = 768 with x, y, the twin (2 bytes: `% 8`), gamma or beta one element off
    nt       the size policy alone reaches it (tests never set UC_LN_NT): rows = the smallest value with rows * C * sizeof(x) > 128 MiB and
             rows % 4 == 1; fp32 x: every nv x {f32, bf16} y; bf16 x: C = 256 x both.  14 launches, twin off, inputs drawn on the device,
             reference on the device in row chunks.
  backward (grid caps parsed from layernorm_plan.h, `PLAN`):
    wide     every nv x 4 (x, dy) pairs x dres on / off x twin on / off (fp32 stream) at rows 1 and 13 (two workgroups, the second ragged);
             per nv one pair with dres (and twin) at rows = cap + 3 (2048 waves: three of them take a second, software-pipelined row)
             and at rows = 2 * cap + 5 (five waves take three rows)
    c64      rows 1, 3, 18 (ragged four-row groups) and cap + 7 (second grid-stride iteration) x 4 pairs
    generic  C = 64 with dres / with twin (must not plan to c64); C = 1, 67, 80, 96, 1280, 2052; C = 768 with x, dy, dres, dx, the twin or
             gamma one element off (the vector kernels would do misaligned 16-byte accesses)

INPUTS (`make_case`).  Families, all four on every small witness, the first on the big ones (nt, cap, the 16391-row c64):
    wide    x ~ N(0.5, 3^2)
    offset  x ~ 100 + N(0, 1): cancellation in mean and variance
    tiny    x ~ 1e-3 N(0, 1): the variance equals eps = 1e-6, so a missing or misplaced eps shows
    const   wide, with row rows // 2 constant: y of that row is beta, within the bound
gamma ~ 1 + 0.2 N(0, 1), beta ~ 0.1 N(0, 1), dy ~ N(0, 1), dres ~ N(0, 1); operands are rounded to their storage dtype first and the
reference sees the rounded values.  Every buffer is a slice of a larger one: inputs lie between bands of NaN (an over-read that reaches a sum
shows), outputs start as NaN (an element never written shows) between bands of SENTINEL that must be untouched afterwards; dgamma / dbeta
start at a non-zero prefill because the contract is `+=`.

REFERENCE: the expressions of include/uc_hip.h in float64.
BOUND per element, the form and constants of tests/gemm_routes.py (u_out = U_OUT: 2^-24 / 2^-8 for an fp32 / bf16 store):
    c = (|x| + |mean|) rstd                                  |xhat| formed on absolute values: x - mean cancels, its rounding error does not
    y      : u_out |ref| + 8 sqrt(C) 2^-24 ( |gamma| c + |beta| )
    dx     : u_out |ref| + 8 sqrt(C) 2^-24 ( rstd ( |a| + mean|a| + c mean(|a| c) ) + |dres| ),   a = dy gamma
    dgamma : 2^-24 |ref| + 8 sqrt(rows + C) 2^-24 sum_r |dy| c
    dbeta  : 2^-24 |ref| + 8 sqrt(rows) 2^-24 sum_r |dy|
dgamma / dbeta are compared as target - prefill.  Every atomic add onto the target rounds at the size of the running value, which the
prefill dominates, so the prefill adds 8 sqrt(n_add) 2^-24 |prefill| in the same random-walk form: n_add = the global atomic adds per
column = the grid of the wide / c64 kernels (one per workgroup), rows for the generic kernel (one per element).  A bf16 twin has the
bound of a bf16 store.

MODEL (`model`): float32 torch on the CPU, two-pass mean / variance, then the stated expressions, every operand fetched from the flat
banded buffer by the kernels' index arithmetic, so a defect of the addressing (`DEFECTS`) reads what the device would read.
The model stays at or under half the bound in front of the store, where the bound has fp32's u_out (`unstored`).  A bf16 store is one
correct rounding, and u_out = 2^-8 is exactly its worst case (a value just above a power of two), so behind a bf16 store a correct result
reaches 0.99 of the bound by the rounding alone; there the model is held to the bound itself.
"""
import math
import os
import re
import shutil
import subprocess

import torch

from tests.gemm_routes import BF16, F32, ROOT, U_OUT

EPS = 1e-6
GUARD = 64            # band elements in front of and behind every buffer: a multiple of 8, so every dtype's slice stays 16-byte aligned
SENTINEL = -6144.0    # exact in bf16
FAMILIES = ("wide", "offset", "tiny", "const")
DT = {"f": torch.float32, "b": torch.bfloat16}
CODE = {"f": F32, "b": BF16}
BYTES = {"f": 4, "b": 2}
PAIRS = (("f", "f"), ("f", "b"), ("b", "b"), ("b", "f"))      # forward: (x, y); backward: (x stream, dy)
NVS = (1, 2, 3, 4, 6, 8)
ROWS3 = (1, 5, 9)
NT_BYTES = 128 << 20


def _plan_constants():
    "The integer constants of layernorm_plan.h (grid caps, rows per workgroup): read, not retyped."
    text = open(os.path.join(ROOT, "uniception_amd", "csrc", "layernorm_plan.h")).read()
    return {k: int(v) for k, v in re.findall(r"static constexpr int (UC_LN_\w+) = (\d+);", text)}


PLAN = _plan_constants()
WIDE_CAP = PLAN["UC_LN_BWD_WIDE_GRID_CAP"] * PLAN["UC_LN_BWD_WIDE_ROWS_PER_WG"]      # rows one pass of the wide kernel covers
C64_CAP = PLAN["UC_LN_BWD_C64_GRID_CAP"] * PLAN["UC_LN_BWD_C64_ROWS_PER_WG"]


def nt_rows(C, x_bytes):
    "The smallest rows with rows * C * x_bytes > 128 MiB and rows % 4 == 1."
    r = NT_BYTES // (C * x_bytes) + 1
    return r + (1 - r) % 4


def _fwd(kernel, nv, x, y, twin, rows, C, nt=0, mis=None, big=False):
    name = f"f_{kernel}{nv or ''}{'_nt' if nt else ''}_{x}{y}_t{twin}_r{rows}_c{C}" + (f"_mis-{mis}" if mis else "")
    return dict(name=name, dir="fwd", kernel=kernel, nv=nv, nt=nt, x=x, o=y, twin=twin, dres=0, rows=rows, C=C, mis=mis, big=big or bool(nt))


def _bwd(kernel, nv, x, dy, dres, twin, rows, C, mis=None, big=False):
    assert not (twin and x == "b")
    name = f"b_{kernel}{nv or ''}_{x}{dy}_d{dres}_t{twin}_r{rows}_c{C}" + (f"_mis-{mis}" if mis else "")
    return dict(name=name, dir="bwd", kernel=kernel, nv=nv, nt=0, x=x, o=dy, twin=twin, dres=dres, rows=rows, C=C, mis=mis, big=big)


def _witnesses():
    out = []
    # ---- forward
    for i, nv in enumerate(NVS):
        for k, (x, y) in enumerate(PAIRS):
            for twin in (0, 1):
                out.append(_fwd("exact", nv, x, y, twin, ROWS3[(2 * i + 2 * k + twin) % 3], 256 * nv))
    for j, C in enumerate((4, 64, 80, 96, 100, 1280, 1792, 2044)):
        for k, (x, y) in enumerate(PAIRS):
            out.append(_fwd("vec", 0, x, y, (j + k) % 2, ROWS3[(j + k) % 3], C))
    for j, (C, mis) in enumerate(((1, None), (67, None), (2052, None), (768, "x"), (768, "twin"), (768, "y"), (768, "gamma"), (768, "beta"))):
        for k, (x, y) in enumerate(PAIRS):
            out.append(_fwd("scalar", 0, x, y, 1 if mis == "twin" else (j + k) % 2, ROWS3[(j + k) % 3], C, mis=mis))
    for nv in NVS:
        for y in "fb":
            out.append(_fwd("exact", nv, "f", y, 0, nt_rows(256 * nv, 4), 256 * nv, nt=1))
    for y in "bf":
        out.append(_fwd("exact", 1, "b", y, 0, nt_rows(256, 2), 256, nt=1))
    # ---- backward
    for i, nv in enumerate(NVS):
        for x, dy in PAIRS:
            for dres in (0, 1):
                for twin in ((0, 1) if x == "f" else (0,)):
                    for rows in (1, 13):
                        out.append(_bwd("wide", nv, x, dy, dres, twin, rows, 256 * nv))
        x, dy = PAIRS[i % 4]
        for rows in (WIDE_CAP + 3, 2 * WIDE_CAP + 5):
            out.append(_bwd("wide", nv, x, dy, 1, int(x == "f"), rows, 256 * nv, big=True))
    for x, dy in PAIRS:
        for rows in (1, 3, 18):
            out.append(_bwd("c64", 0, x, dy, 0, 0, rows, 64))
        out.append(_bwd("c64", 0, x, dy, 0, 0, C64_CAP + 7, 64, big=True))
    for x, dy in PAIRS:
        out.append(_bwd("generic", 0, x, dy, 1, 0, 5, 64))
    for dy in "fb":
        out.append(_bwd("generic", 0, "f", dy, 0, 1, 5, 64))
    for j, C in enumerate((1, 67, 80, 96, 1280, 2052)):
        for k, (x, dy) in enumerate(PAIRS):
            out.append(_bwd("generic", 0, x, dy, (j + k) % 2, int(x == "f" and (j + k // 2) % 2 == 0), ROWS3[(j + k) % 3], C))
    for x, dy, dres, twin, mis in (("f", "f", 0, 0, "x"), ("b", "b", 0, 0, "x"), ("f", "b", 0, 0, "dy"), ("b", "f", 0, 0, "dy"), ("f", "f", 1, 0, "dres"),
                                   ("b", "b", 1, 0, "dres"), ("f", "b", 0, 0, "dx"), ("b", "f", 1, 0, "dx"), ("f", "f", 1, 1, "twin"),
                                   ("f", "b", 1, 1, "gamma"), ("b", "b", 0, 0, "gamma")):
        out.append(_bwd("generic", 0, x, dy, dres, twin, 9, 768, mis=mis))
    names = [w["name"] for w in out]
    assert len(set(names)) == len(names)
    return {w["name"]: w for w in out}


WITNESSES = _witnesses()
NAMES = list(WITNESSES)
SMALL = [n for n in NAMES if not WITNESSES[n]["big"]]
BIG = [n for n in NAMES if WITNESSES[n]["big"]]


def route(w):
    if w["dir"] == "fwd":
        return f"fwd {w['kernel']} nv{w['nv']} nt{w['nt']} {w['x']}->{w['o']} twin{w['twin']}"
    return f"bwd {w['kernel']} nv{w['nv']} x {w['x']} dy {w['o']} dres{w['dres']} twin{w['twin']}"


def plan_key(w):
    "(direction, kernel, nv, nt): what the plans decide."
    return (w["dir"], w["kernel"], w["nv"], w["nt"])


def outputs(w):
    if w["dir"] == "fwd":
        return ("y", "twin") if w["twin"] else ("y",)
    return ("dx",) + (("twin",) if w["twin"] else ()) + ("dgamma", "dbeta")


# ------------------------------------------------------------------------------------------ plan driver
def build_driver(tmpdir):
    "Compile tests/layernorm_plan_driver.cpp with the system C++ compiler into tmpdir; returns run(rows) -> plan lines."
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed to build tests/layernorm_plan_driver.cpp"
    exe = os.path.join(str(tmpdir), "layernorm_plan_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "uniception_amd", "csrc"),
                           os.path.join(ROOT, "tests", "layernorm_plan_driver.cpp"), "-o", exe])

    def run(rows):
        lines = [" ".join(f"{k}={v}" for k, v in row.items()) for row in rows]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return run


BASE = 1 << 20      # a placeholder address, aligned for everything


def driver_row(w, ptrs=None):
    "The launch of the witness as a driver row; `ptrs`: real addresses {buffer: address}, else placeholders with the witness's misalignment."
    def p(name):
        if ptrs is not None:
            return ptrs.get(name, 0)
        elem = 4 if name in ("gamma", "beta") else 2 if name == "twin" else BYTES[w["o"]] if name in ("y", "dy") else BYTES[w["x"]]
        return BASE + (elem if w["mis"] == name else 0)
    row = dict(dir=w["dir"], rows=w["rows"], C=w["C"], x_bytes=BYTES[w["x"]], x=p("x"), gamma=p("gamma"), twin=p("twin") if w["twin"] else 0)
    if w["dir"] == "fwd":
        row.update(y=p("y"), beta=p("beta"))
    else:
        row.update(dy_bytes=BYTES[w["o"]], dy=p("dy"), dx=p("dx"), dres=p("dres") if w["dres"] else 0)
    return row


def expected_plan(w):
    "The plan line of the witness, the grid worked here from PLAN."
    if w["dir"] == "fwd":
        per = PLAN["UC_LN_FWD_ROWS_PER_WG"]
        return f"fwd {w['kernel']} {w['nv']} {w['nt']} {per} {-(-w['rows'] // per)}"
    per, cap = {"wide": (PLAN["UC_LN_BWD_WIDE_ROWS_PER_WG"], PLAN["UC_LN_BWD_WIDE_GRID_CAP"]),
                "c64": (PLAN["UC_LN_BWD_C64_ROWS_PER_WG"], PLAN["UC_LN_BWD_C64_GRID_CAP"]),
                "generic": (PLAN["UC_LN_BWD_GENERIC_ROWS_PER_WG"], 1 << 62)}[w["kernel"]]
    return f"bwd {w['kernel']} {w['nv']} {per} {min(cap, -(-w['rows'] // per))}"


def n_atomic_adds(w):
    "Global atomic adds per dgamma / dbeta column: one per workgroup (wide, c64), one per row (generic)."
    return w["rows"] if w["kernel"] == "generic" else int(expected_plan(w).split()[-1])


# ------------------------------------------------------------------------------------------ operands
def _banded(n, dtype, device, band, fill, off=0):
    "(buffer, start, the n elements from start): `band` everywhere, `fill` (a tensor, or a value) inside."
    buf = torch.full((GUARD + n + GUARD + 8,), band, dtype=dtype, device=device)
    start = GUARD + off
    view = buf[start:start + n]
    view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
    return buf, start, view


def bands_untouched(buf, start, n, band=SENTINEL):
    a, b = buf[:start], buf[start + n:]
    if band != band:
        return bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())
    return bool((a == band).all()) and bool((b == band).all())


def make_case(w, family, device, seed=0):
    """Seeded operands and output buffers of a witness on `device`: t[name] is the [rows, C] / [C] view, t[name + "_buf"] the flat banded
    buffer and t[name + "_at"] the view's first element in it.  A buffer named by w["mis"] starts one element later."""
    assert family in FAMILIES
    g = torch.Generator(device=device).manual_seed(7000 + seed)
    rows, C = w["rows"], w["C"]
    nan = float("nan")

    def randn(*shape):
        return torch.randn(*shape, generator=g, device=device)

    x = {"wide": lambda: 0.5 + 3.0 * randn(rows, C), "offset": lambda: 100.0 + randn(rows, C), "tiny": lambda: 1e-3 * randn(rows, C),
         "const": lambda: 0.5 + 3.0 * randn(rows, C)}[family]()
    if family == "const":
        x[rows // 2] = x[rows // 2, 0].clone()
    t = {"const_row": rows // 2 if family == "const" else None}

    def put(name, dtype, band, fill, shape):
        buf, at, view = _banded(math.prod(shape), dtype, device, band, fill, off=int(w["mis"] == name))
        t[name + "_buf"], t[name + "_at"], t[name] = buf, at, view.view(*shape)

    put("x", DT[w["x"]], nan, x.to(DT[w["x"]]).flatten(), (rows, C))
    del x
    put("gamma", torch.float32, nan, 1.0 + 0.2 * randn(C), (C,))
    if w["dir"] == "fwd":
        put("beta", torch.float32, nan, 0.1 * randn(C), (C,))
        put("y", DT[w["o"]], SENTINEL, nan, (rows, C))
    else:
        put("dy", DT[w["o"]], nan, randn(rows, C).to(DT[w["o"]]).flatten(), (rows, C))
        if w["dres"]:
            put("dres", DT[w["x"]], nan, randn(rows, C).to(DT[w["x"]]).flatten(), (rows, C))
        put("dx", DT[w["x"]], SENTINEL, nan, (rows, C))
        t["pre_g"], t["pre_b"] = 0.5 + torch.rand(C, generator=g, device=device), -0.5 - torch.rand(C, generator=g, device=device)
        put("dgamma", torch.float32, SENTINEL, t["pre_g"], (C,))
        put("dbeta", torch.float32, SENTINEL, t["pre_b"], (C,))
    if w["twin"]:
        put("twin", torch.bfloat16, SENTINEL, nan, (rows, C))
    return t


# ------------------------------------------------------------------------------------------ reference and bound
ACC = 8.0 * 2.0 ** -24


def _stats(x):
    mean = x.mean(1, keepdim=True)
    rstd = (((x - mean) ** 2).mean(1, keepdim=True) + EPS).rsqrt()
    return mean, rstd, (x.abs() + mean.abs()) * rstd


def reference_fwd(w, x, gamma, beta):
    "{output: (ref, bound)} in float64 of the rows x given (the whole witness, or a chunk of its rows)."
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean, rstd, c = _stats(x)
    y = (x - mean) * rstd * gamma + beta
    acc = ACC * math.sqrt(w["C"]) * (gamma.abs() * c + beta.abs())
    out = {"y": (y, U_OUT[CODE[w["o"]]] * y.abs() + acc)}
    if w["twin"]:
        out["twin"] = (y, U_OUT[BF16] * y.abs() + acc)
    return out


def reference_bwd(w, t):
    "{output: (ref, bound)} in float64; dgamma / dbeta are what the launch adds to the prefill."
    x, gamma, dy = t["x"].double(), t["gamma"].double(), t["dy"].double()
    rows, C = w["rows"], w["C"]
    mean, rstd, c = _stats(x)
    xhat, a = (x - mean) * rstd, dy * gamma
    dx = rstd * (a - a.mean(1, keepdim=True) - xhat * (a * xhat).mean(1, keepdim=True))
    s = rstd * (a.abs() + a.abs().mean(1, keepdim=True) + c * (a.abs() * c).mean(1, keepdim=True))
    if w["dres"]:
        dx = dx + t["dres"].double()
        s = s + t["dres"].double().abs()
    acc = ACC * math.sqrt(C) * s
    out = {"dx": (dx, U_OUT[CODE[w["x"]]] * dx.abs() + acc)}
    if w["twin"]:
        out["twin"] = (dx, U_OUT[BF16] * dx.abs() + acc)
    pre = ACC * math.sqrt(n_atomic_adds(w))
    dg, db = (dy * xhat).sum(0), dy.sum(0)
    out["dgamma"] = (dg, 2.0 ** -24 * dg.abs() + ACC * math.sqrt(rows + C) * (dy.abs() * c).sum(0) + pre * t["pre_g"].double().abs())
    out["dbeta"] = (db, 2.0 ** -24 * db.abs() + ACC * math.sqrt(rows) * dy.abs().sum(0) + pre * t["pre_b"].double().abs())
    return out


def unstored(ref, bnd, code):
    "The bound in front of a store of dtype `code`: the store's own rounding u_out |ref| replaced by fp32's."
    return bnd - (U_OUT[code] - U_OUT[F32]) * ref.abs()


def reference(w, t):
    return reference_fwd(w, t["x"], t["gamma"], t["beta"]) if w["dir"] == "fwd" else reference_bwd(w, t)


def results(w, t):
    "{output: tensor} of what a launch left in the case's buffers; dgamma / dbeta as target - prefill in float64."
    out = {o: t[o] for o in outputs(w) if o not in ("dgamma", "dbeta")}
    if w["dir"] == "bwd":
        out["dgamma"], out["dbeta"] = t["dgamma"].double() - t["pre_g"].double(), t["dbeta"].double() - t["pre_b"].double()
    return out


def ratio(got, ref, bnd):
    "(largest err / bound, elements over the bound or NaN, flat index of the worst); an element with bound 0 must be exact."
    err = (got.double() - ref).abs()
    nan = torch.isnan(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    r = torch.where(nan, torch.full_like(r, float("inf")), r)
    if r.numel() == 0:
        return 0.0, 0, 0
    worst, at = r.flatten().max(0)
    worst, at, bad = torch.stack([worst, at.to(worst.dtype), (r > 1.0).sum().to(worst.dtype)]).tolist()      # one device synchronisation
    return worst, int(bad), int(at)


def check(label, name, got, ref, bnd):
    "Zero elements over the bound, or an AssertionError naming the route, the count, the worst ratio and its (row, column)."
    worst, bad, at = ratio(got, ref, bnd)
    if bad == 0:
        return worst
    cols = ref.shape[-1]
    r, c = (at // cols, at % cols) if ref.dim() > 1 else (0, at)
    raise AssertionError(f"route [{label}] output {name}: {bad} of {ref.numel()} elements over the bound, worst err / bound {worst:.4g} at "
                         f"(row {r}, col {c}): got {float(got.flatten()[at]):.9g} ref {float(ref.flatten()[at]):.9g} bound {float(bnd.flatten()[at]):.3g}")


# ------------------------------------------------------------------------------------------ model
# defect -> the directions it belongs to
DEFECTS = {"last_vec_unwritten": ("fwd", "bwd"), "last_vec_from_next_row": ("fwd", "bwd"), "inv_c_minus_1": ("fwd", "bwd"), "eps_dropped": ("fwd", "bwd"),
           "gamma_shift4": ("fwd", "bwd"), "beta_shift4": ("fwd",), "mean_from_full_chunks": ("fwd", "bwd"), "dres_not_added": ("bwd",),
           "s2_without_gamma": ("bwd",), "dgamma_missing_last_row": ("bwd",), "twin_from_x": ("fwd",)}


def _fetch(t, name, idx):
    flat = t[name + "_buf"].float()
    return flat[(t[name + "_at"] + idx).clamp(0, flat.numel() - 1)]


def model(w, t, defect=None, store=True):
    """The kernels' arithmetic in float32 torch on CPU tensors: two-pass mean / variance, then the expressions of include/uc_hip.h, stores
    rounded to the output dtype (`store=False`: kept in float32, the value in front of the store), dgamma / dbeta added to the prefill.
    `defect`: one of DEFECTS.  {output: tensor} as `results`."""
    assert defect is None or w["dir"] in DEFECTS[defect]
    ydt, xdt, tdt = (DT[w["o"]], DT[w["x"]], torch.bfloat16) if store else (torch.float32,) * 3
    rows, C = w["rows"], w["C"]
    col = torch.arange(C)
    idx = torch.arange(rows)[:, None] * C + col[None]
    last = col >= C - 4
    xi = idx + C * last[None] if defect == "last_vec_from_next_row" else idx
    x = _fetch(t, "x", xi)
    gamma = _fetch(t, "gamma", col + (4 if defect == "gamma_shift4" else 0))
    inv = torch.tensor(1.0) / (C - 1 if defect == "inv_c_minus_1" else C)
    eps = 0.0 if defect == "eps_dropped" else EPS
    mean = (x[:, :256 * (C // 256)] if defect == "mean_from_full_chunks" else x).sum(1, keepdim=True) * inv
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) * inv + eps)
    nan = float("nan")
    if w["dir"] == "fwd":
        beta = _fetch(t, "beta", col + (4 if defect == "beta_shift4" else 0))
        o = d * rstd * gamma + beta
        out = {"y": o.to(ydt)}
        if w["twin"]:
            out["twin"] = (x if defect == "twin_from_x" else o).to(tdt)
        if defect == "last_vec_unwritten":
            for v in out.values():
                v[:, last] = nan
        return out
    dy = _fetch(t, "dy", idx + C * last[None] if defect == "last_vec_from_next_row" else idx)
    xhat, a = d * rstd, dy * gamma
    s1 = a.sum(1, keepdim=True) * inv
    s2 = ((dy if defect == "s2_without_gamma" else a) * xhat).sum(1, keepdim=True) * inv
    o = rstd * (a - s1 - xhat * s2)
    if w["dres"] and defect != "dres_not_added":
        o = o + _fetch(t, "dres", idx)
    out = {"dx": o.to(xdt)}
    if w["twin"]:
        out["twin"] = o.to(tdt)
    if defect == "last_vec_unwritten":
        for v in out.values():
            v[:, last] = nan
    n = rows - 1 if defect == "dgamma_missing_last_row" else rows
    dg = t["pre_g"] + (dy * xhat)[:n].sum(0)
    db = t["pre_b"] + dy.sum(0)
    out["dgamma"], out["dbeta"] = dg.double() - t["pre_g"].double(), db.double() - t["pre_b"].double()
    return out


if __name__ == "__main__":
    print(f"{len(WITNESSES)} witnesses ({len(SMALL)} small x {len(FAMILIES)} input families, {len(BIG)} big), "
          f"{len({route(w) for w in WITNESSES.values()})} routes, {len({plan_key(w) for w in WITNESSES.values()})} (direction, kernel, nv, nt)")
    for n, w in WITNESSES.items():
        print(f"  {n:44s} rows {w['rows']:7d} C {w['C']:5d}  [{route(w)}]")
