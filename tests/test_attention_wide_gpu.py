"""GPU: every kernel of the head_dim > 64 attention path (tests/attention_wide_routes.py WITNESSES) is launched at its witness shape through
ops.attention / ops.attention_bwd, proven to have taken that kernel — the descriptor the wrapper passed goes to the plan driver — and
compared element by element with the fp64 reference under the derived bound.  Then: the refusals (before any launch), and the backward's
bit reproducibility."""
import pytest
import torch

from tests import attention_wide_routes as R

pytestmark = pytest.mark.gpu

NAMES = list(R.WITNESSES)
_REPORT = {}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    yield R.build_driver(tmp_path_factory.mktemp("attention_wide_gpu"))
    for name, line in _REPORT.items():      # (shown with -s: the table of DESIGN.md section 14)
        print(f"  {name:18s} {line}")


def _route(plan, fn, captured):
    assert len(captured) == 1, f"{len(captured)} launches"
    line = plan([captured[0]])[0]
    return R.route_of(fn, line), line


@pytest.mark.parametrize("name", NAMES)
def test_witness_against_fp64(gpu, plan, name):
    from uniception_amd import ops
    w = R.WITNESSES[name]
    t = R.make_operands(w, w["shape"], seed=R.SEEDS[name])
    p, zones = R.place(w, t, gpu)
    scale = w["D"] ** -0.5
    bf = w["dtype"] == R.BF16
    bwd = w["fn"] == "bwd"
    with R.spy("uc_attention_fwd", R.FWD_FIELDS) as cap:
        ops.attention(p["q"], p["k"], ops.vt_pack(p["v"]) if bf else p["v"], scale, v_packed=bf, out=p["out"], lse=p["lse"])
        fwd_route, fwd_line = _route(plan, "fwd", cap)
    want_fwd = w["route"] if not bwd else (f"bf16_{w['D']}" if bf else "f32_96")
    assert fwd_route == want_fwd, f"the launch took [{fwd_route}] ({fwd_line}), the witness stands for [{want_fwd}]"
    got = {"O": p["out"], "LSE": p["lse"]}
    if bwd:
        with R.spy("uc_attention_bwd", R.BWD_FIELDS) as cap:
            ops.attention_bwd(p["q"], p["k"], p["v"], p["out"], p["do"], p["lse"], scale, out=(p["dq"], p["dk"], p["dv"]))
            bwd_route, bwd_line = _route(plan, "bwd", cap)
        assert bwd_route == w["route"], f"the launch took [{bwd_route}] ({bwd_line}), the witness stands for [{w['route']}]"
        got.update(dQ=p["dq"], dK=p["dk"], dV=p["dv"])
    torch.cuda.synchronize()

    for n, x in got.items():
        assert bool(torch.isfinite(x).all()), f"[{w['route']}] ({name}): {n} has {int((~torch.isfinite(x)).sum())} non-finite elements"
    ref = R.reference(w, t, scale, dev=gpu)
    worst = {}
    for n in got:
        x = R.ratio(got[n], *ref[n])
        print(f"{name}: {n} worst err / bound {float(x.max()):.3f}")
        worst[n] = R.check(f"{w['route']} ({name})", n, got[n], *ref[n])
    _REPORT[name] = " ".join(f"{n} {v:.3f}" for n, v in worst.items())
    for zone, z in zones.items():
        assert bool(torch.isnan(z).all()), f"[{w['route']}] ({name}): {zone} was written ({int((~torch.isnan(z)).sum())} elements)"


def _operands(gpu, D, dtype, B=1, H=2, Nq=40, Nk=40):
    g = torch.Generator().manual_seed(11)
    q, k, v, do = (torch.randn(B, n, H, D, generator=g).to(dtype).to(gpu) for n in (Nq, Nk, Nk, Nq))
    return q, k, v, do


@pytest.mark.parametrize("dtype,D,what", [(torch.bfloat16, 112, "head_dim"), (torch.float32, 100, "head_dim"), (torch.bfloat16, 80, "dropout"),
                                          (torch.bfloat16, 96, "rope"), (torch.bfloat16, 72, "head_dim"), (torch.float32, 80, "dropout")])
def test_refusals_come_before_any_launch_and_name_the_head_dim(gpu, dtype, D, what):
    """The C entry points are called directly (the wrappers' own checks aside): status != 0, the message names the head_dim, and the
    outputs — NaN before the call — are untouched."""
    import ctypes as C
    from uniception_amd import _lib, ops
    lib = _lib.load()
    q, k, v, do = _operands(gpu, D, dtype)
    B, N, H, _ = q.shape
    out = torch.full_like(q, float("nan"))
    lse = torch.full((B, H, N), float("nan"), device=gpu)
    bf = dtype == torch.bfloat16
    vt = torch.zeros((B, H, D, 64), dtype=dtype, device=gpu) if bf else v
    d = _lib.AttnDesc()
    d.dtype, d.v_layout = ops._dt(dtype), ops.UC_V_PACKED_T if bf else ops.UC_V_ROWMAJOR
    d.B, d.H, d.Nq, d.Nk, d.D = B, H, N, N, D
    d.Q, d.K, d.V, d.O = q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()
    d.q_sb, d.q_sn, d.q_sh = q.stride(0), q.stride(1), q.stride(2)
    d.k_sb, d.k_sn, d.k_sh = k.stride(0), k.stride(1), k.stride(2)
    d.v_sb, d.v_sn, d.v_sh = (0, 0, 0) if bf else (v.stride(0), v.stride(1), v.stride(2))
    d.o_sb, d.o_sn, d.o_sh = out.stride(0), out.stride(1), out.stride(2)
    d.scale, d.lse = D ** -0.5, lse.data_ptr()
    if what == "dropout":
        d.drop_p, d.seed = 0.25, 7
    if what != "rope":      # (the forward descriptor has no RoPE field)
        status = lib.uc_attention_fwd(C.byref(d), None)
        msg = lib.uc_last_error().decode()
        assert status != 0 and (f"head_dim {D}" in msg or f"got {D}" in msg), msg
    # the backward with the same fault
    dq, dk, dv = (torch.full_like(x, float("nan")) for x in (q, k, v))
    delta = torch.empty((B * H, 2, 128), dtype=torch.float32, device=gpu)
    pos = torch.zeros((B * N, 2), dtype=torch.int64, device=gpu)
    b = _lib.AttnBwdDesc()
    b.dtype, b.B, b.H, b.Nq, b.Nk, b.D = ops._dt(dtype), B, H, N, N, D
    lse0 = torch.zeros((B, H, N), device=gpu)
    b.Q, b.K, b.V, b.O, b.dO, b.LSE = q.data_ptr(), k.data_ptr(), v.data_ptr(), do.data_ptr(), do.data_ptr(), lse0.data_ptr()
    b.dQ, b.dK, b.dV, b.delta = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
    for pre, x in (("q", q), ("k", k), ("v", v), ("o", do), ("dq", dq), ("dk", dk), ("dv", dv)):
        for i, s in enumerate(("sb", "sn", "sh")):
            setattr(b, f"{pre}_{s}", x.stride(i))
    b.scale = D ** -0.5
    if what == "dropout":
        b.drop_p, b.seed = 0.25, 7
    if what == "rope":
        b.rope_qpos, b.rope_kpos, b.rope_base, b.rope_f0 = pos.data_ptr(), pos.data_ptr(), 100.0, 1.0
    status = lib.uc_attention_bwd(C.byref(b), None)
    msg = lib.uc_last_error().decode()
    assert status != 0 and (f"head_dim {D}" in msg or f"got {D}" in msg), msg
    torch.cuda.synchronize()
    for x in (out, lse, dq, dk, dv):
        assert bool(torch.isnan(x).all()), "a refused call wrote an output"


@pytest.mark.parametrize("D", [80, 96])
def test_the_backward_gives_the_same_bits_on_every_call(gpu, D):
    from uniception_amd import ops
    q, k, v, do = _operands(gpu, D, torch.bfloat16, B=2, H=3, Nq=200, Nk=150)
    scale = D ** -0.5
    lse = torch.empty((2, 3, 200), dtype=torch.float32, device=gpu)
    o = ops.attention(q, k, ops.vt_pack(v), scale, v_packed=True, lse=lse)
    a = ops.attention_bwd(q, k, v, o, do, lse, scale)
    b = ops.attention_bwd(q, k, v, o, do, lse, scale)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(bool(torch.isfinite(x).all()) for x in a)
