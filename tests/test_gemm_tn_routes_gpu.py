"""GPU: every uc_gemm_tn route (tests/gemm_tn_routes.py, checked on the CPU by tests/test_gemm_tn_routes.py) is launched at its witness
shape through ops.gemm_tn on operands that live inside NaN, proven to have taken its kernel — the uc_gemm_tn_desc the wrapper passed goes
to the plan driver — and every slab, the slab sum and the colsum are compared element by element with the fp64 reference under the derived
bound; the guard bands around the slabs and the colsum stay untouched.  uc_splitk_reduce by itself: bitwise against the sequential fp32
sum in slab order.  References run on the device in torch's fp64."""
import pytest
import torch

from tests import gemm_tn_routes as R

pytestmark = pytest.mark.gpu

GUARD = 4096          # NaN floats in front of and behind every output this file allocates (a multiple of 4: the outputs stay 16-byte aligned)
DRIVER_FIELDS = "A lda B ldb T I J conv_B conv_H conv_W conv_Cin conv_stride relu_b C colsum_a colsum_atomic split_k".split()


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("gemm_tn_routes_gpu"))


def _guarded(n, dev):
    "(buffer, the n floats in its middle): NaN everywhere."
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guards_untouched(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def _spy(lib, captured):
    real = lib.uc_gemm_tn

    def spy(desc_ref, stream):
        d = desc_ref._obj
        captured.append({f: int(getattr(d, f) or 0) for f in DRIVER_FIELDS})
        return real(desc_ref, stream)
    return real, spy


@pytest.mark.parametrize("name", R.NAMES)
def test_route_against_fp64(gpu, plan, name):
    from uniception_amd import _lib, ops
    w = R.WITNESSES[name]
    label = f"{name}: {R.route(w)}"
    seed = R.NAMES.index(name)
    t = R.make_operands(w, gpu, seed=seed)
    sk, I, J = w["split_k"], w["I"], w["J"]
    slab_buf, slabs = _guarded(sk * I * J, gpu)
    kw = dict(split_k=sk, out=slabs.view(sk, I, J))
    if w["conv"]:
        kw["conv"] = (w["conv"][4], bool(w["relu_b"]))
    pre = cs_buf = cs = None
    if w["colsum"] == "slabs":
        cs_buf, cs = _guarded(sk * I, gpu)
        kw.update(colsum=True, colsum_out=cs.view(sk, I))
    elif w["colsum"] == "atomic":
        pre = R.prefill(w, gpu, seed=seed)
        cs_buf, cs = _guarded(I, gpu)
        cs.copy_(pre)
        kw["colsum_into"] = cs

    lib = _lib.load()
    captured = []
    real, spy = _spy(lib, captured)
    lib.uc_gemm_tn = spy
    try:
        res = ops.gemm_tn(t["A"], t["B"], **kw)
    finally:
        lib.uc_gemm_tn = real
    torch.cuda.synchronize()

    # the launch took the route: the descriptor the wrapper passed -> the plan driver
    assert len(captured) == 1
    d = captured[0]
    line = plan([d])[0]
    assert " ".join(line.split()[:7]) == R.expected_plan(w), f"the launch took [{line}], the witness stands for [{R.expected_plan(w)}]"
    assert (d["relu_b"], d["colsum_a"] != 0, d["colsum_atomic"], d["lda"], d["ldb"]) == \
        (w["relu_b"], w["colsum"] != "none", int(w["colsum"] == "atomic"), w["lda"], w["ldb"])
    assert d["C"] == slabs.data_ptr() and (cs is None or d["colsum_a"] == cs.data_ptr())
    out = res[0] if w["colsum"] == "slabs" else res
    assert out.data_ptr() == slabs.data_ptr() and out.shape == (sk, I, J)

    # every element was written (empty slices too), nothing around them
    assert bool(torch.isfinite(slabs).all()), f"[{label}]: {int((~torch.isfinite(slabs)).sum())} slab elements are not finite"
    assert _guards_untouched(slab_buf, sk * I * J), f"[{label}]: the guard band around the slabs was written"
    if cs is not None:
        assert bool(torch.isfinite(cs).all()), f"[{label}]: {int((~torch.isfinite(cs)).sum())} colsum elements are not finite"
        assert _guards_untouched(cs_buf, cs.numel()), f"[{label}]: the guard band around the colsum was written"
    # the operands are as they were
    assert bool(torch.isnan(t["A_buf"][w["T"]:]).all()) and not bool(torch.isnan(t["A"]).any())

    ref = R.reference(w, t, pre)
    tile = R.TILE[w["kernel"]]
    worst = {}
    for s in range(sk):
        worst["slabs"] = max(worst.get("slabs", 0.0), R.ratio(out[s], ref["slabs"][0][s], ref["slabs"][1][s])[0])
    dw = ops.splitk_reduce(out)
    worst["dW"] = R.ratio(dw, *ref["dW"])[0]
    if w["colsum"] == "slabs":
        worst["colsum_slabs"] = R.ratio(cs.view(sk, I), *ref["colsum_slabs"])[0]
        worst["colsum"] = R.ratio(cs.view(sk, I).double().sum(0), *ref["colsum"])[0]
    elif w["colsum"] == "atomic":
        worst["colsum"] = R.ratio(cs.double() - pre.double(), *ref["colsum"])[0]
    print(f"{name}: largest err / bound {({k: round(v, 4) for k, v in worst.items()})}")
    for s in range(sk):
        R.check(label, f"slab {s}", out[s], ref["slabs"][0][s], ref["slabs"][1][s], tile)
    R.check(label, "dW", dw, *ref["dW"], tile)
    if w["colsum"] == "slabs":
        R.check(label, "colsum slabs", cs.view(sk, I), *ref["colsum_slabs"], (1, tile[0]))
    elif w["colsum"] == "atomic":
        R.check(label, "colsum (target - prefill)", (cs.double() - pre.double())[None], ref["colsum"][0][None], ref["colsum"][1][None], (1, tile[0]))


# (split_k, accumulate, rows of the slabs, r0, r1, N): n = (r1 - r0) * N floats out of slabs of rows * N
REDUCE_CASES = [(1, False, 40, 0, 40, 52), (1, True, 40, 2, 39, 52), (2, False, 40, 2, 39, 52), (2, True, 40, 0, 40, 52), (7, False, 40, 2, 39, 52),
                (7, True, 40, 2, 39, 52), (2, True, 8176, 2, 8173, 1028)]


@pytest.mark.parametrize("sk,accumulate,rows,r0,r1,N", REDUCE_CASES, ids=[f"sk{c[0]}_acc{int(c[1])}_rows{c[3]}-{c[4]}of{c[2]}_N{c[5]}" for c in REDUCE_CASES])
def test_splitk_reduce_is_the_sequential_fp32_sum(gpu, sk, accumulate, rows, r0, r1, N):
    """uc_splitk_reduce only adds, in slab order: out (+)= ws[0] + ws[1] + ..., so it equals the sequential fp32 sum bit for bit.  The form
    autograd._wgrad's sink path uses: a row range ws[:, r0:r1] of every slab (slab stride above n, start inside the slab, NaN in the rows
    outside the range), += into a live buffer, a NaN guard around out; n = 1924 is no multiple of 1024, n = 8171 * 1028 lies above
    8192 * 256 * 4 (the grid-stride loop's second pass)."""
    from uniception_amd import ops
    g = torch.Generator(device=gpu).manual_seed(sk * 1000 + rows + int(accumulate))
    n = (r1 - r0) * N
    assert n % 4 == 0 and (r0 * N) % 4 == 0 and (n % 1024 != 0) and (rows < 8000 or n > 8192 * 256 * 4)
    ws = torch.full((sk, rows, N), float("nan"), dtype=torch.float32, device=gpu)
    ws[:, r0:r1] = torch.randn(sk, r1 - r0, N, generator=g, device=gpu)
    buf, out = _guarded(n, gpu)
    out.copy_(torch.randn(n, generator=g, device=gpu))       # live values: kept with accumulate, overwritten without
    want = out.clone().view(r1 - r0, N) if accumulate else torch.zeros(r1 - r0, N, device=gpu)
    for s in range(sk):
        want = want + ws[s, r0:r1]
    got = ops.splitk_reduce(ws[:, r0:r1], out=out.view(r1 - r0, N), accumulate=accumulate)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{int((got.view(torch.int32) != want.view(torch.int32)).sum())} of {n} elements differ"
    assert _guards_untouched(buf, n), "the guard band around out was written"
    assert bool(torch.isnan(ws[:, :r0]).all()) and bool(torch.isnan(ws[:, r1:]).all())
