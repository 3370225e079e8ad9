"""GPU: every attention route (tests/attention_routes.py WITNESSES, checked against the plan on the CPU by tests/test_attention_routes.py)
is launched at its witness shape through ops.attention / ops.attention_bwd, proven to have taken that route — the descriptor the
wrapper passed goes to the plan driver with the device's CU count and the live knobs — and compared element by element with the fp64
reference under the derived bound.  Order of the assertions: the route, every output finite, every element inside the bound (a failure
names the element and its 64-row and 128-row tiles), every guard band and unused fused slot still NaN."""
import pytest
import torch

from tests import attention_routes as R

pytestmark = pytest.mark.gpu

NAMES = list(R.WITNESSES)
_REPORT = {}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    yield R.build_driver(tmp_path_factory.mktemp("attention_routes_gpu"))
    for name, line in _REPORT.items():      # (shown with -s: the table of the module docstring of tests/attention_routes.py)
        print(f"  {name:26s} {line}")


def _route(plan, ops, fn, captured):
    assert len(captured) == 1, f"{len(captured)} launches"
    line = plan([{**captured[0], **R.live_knobs(ops)}])[0]
    return R.route_of(fn, line), line


@pytest.mark.parametrize("name", NAMES)
def test_route_against_fp64(gpu, plan, name):
    from uniception_amd import ops
    w = R.WITNESSES[name]
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    shape = R.shape_for(w, cus)
    B, H, Nq, Nk = shape
    t = R.make_operands(w, shape, seed=R.SEEDS[name])
    p, zones = R.place(w, t, gpu)
    scale = w["D"] ** -0.5
    bf = w["dtype"] == R.BF16
    bwd = w["fn"] == "bwd"
    dropout = (w["drop"], R.DROP_SEED) if w["drop"] else None
    mask = ops.attention_drop_mask(B, H, Nq, Nk, w["drop"], R.DROP_SEED, gpu) if w["drop"] else None
    v_arg = ops.vt_pack(p["v"]) if bf else p["v"]

    # the forward (a backward witness: under the default knobs, whichever kernel that is; its LSE error enters the bound)
    with R.knobs_set(ops, {} if bwd else w["knobs"]), R.spy("uc_attention_fwd", R.FWD_FIELDS) as cap:
        ops.attention(p["q"], p["k"], v_arg, scale, v_packed=bf, out=p["out"], lse=p["lse"], dropout=dropout)
        fwd_route, fwd_line = _route(plan, ops, "fwd", cap)
    if not bwd:
        assert fwd_route == w["route"], f"the launch took [{fwd_route}] ({fwd_line}), the witness stands for [{w['route']}]"
    got = {"O": p["out"], "LSE": p["lse"]}
    if bwd:
        with R.knobs_set(ops, w["knobs"]), R.spy("uc_attention_bwd", R.BWD_FIELDS) as cap:
            ops.attention_bwd(p["q"], p["k"], p["v"], p["out"], p["do"], p["lse"], scale, out=(p["dq"], p["dk"], p["dv"]),
                              rope=p.get("rope"), dropout=dropout)
            bwd_route, bwd_line = _route(plan, ops, "bwd", cap)
        assert bwd_route == w["route"], f"the launch took [{bwd_route}] ({bwd_line}), the witness stands for [{w['route']}]"
        got.update(dQ=p["dq"], dK=p["dk"], dV=p["dv"])
    torch.cuda.synchronize()

    for n, x in got.items():
        assert bool(torch.isfinite(x).all()), f"route [{w['route']}] ({name}): {n} has {int((~torch.isfinite(x)).sum())} non-finite elements"
    ref, flagged = R.reference(w, t, scale, mask, fwd_requant=fwd_route in R.REQUANT_FWD, dev=gpu)
    worst = {n: R.check(f"{w['route']} ({name})", n, got[n], *ref[n]) for n in got}
    _REPORT[name] = f"fwd {fwd_route:12s} " + " ".join(f"{n} {v:.3f}" for n, v in worst.items())
    if w["seam"]:      # the first and the last (batch, head): an item of the first wave of workgroups and one picked up at a seam
        for b, h in ((0, 0), (B - 1, H - 1)):
            for n in got:
                sl = (slice(b, b + 1), slice(h, h + 1)) if n == "LSE" else (slice(b, b + 1), slice(None), slice(h, h + 1))
                R.check(f"{w['route']} ({name}) batch {b} head {h}", n, got[n][sl], ref[n][0][sl], ref[n][1][sl])
    if w["fixup"]:
        b, q, h, _ = R.spike_position(w, shape)
        assert bool(flagged[b, h, q]), "the spiked row stays inside the persistent kernel's score range: no block for attn_bf16_fixup_kernel"
        assert int(flagged.sum()) == 1
        words = p["out"].contiguous().view(torch.int32)
        assert not bool((words == 0x7fc57fc5).any()), "a sentinel of the persistent kernel is left in O"
    else:
        assert not bool(flagged.any())
    for zone, z in zones.items():
        assert bool(torch.isnan(z).all()), f"route [{w['route']}] ({name}): {zone} was written ({int((~torch.isnan(z)).sum())} elements)"


def test_role_split_is_bitwise_the_eight_wave_kernel_on_their_witness(gpu, plan):
    "rs8 == dma8 to the bit (O and LSE) at the witness both are checked against fp64 on."
    from uniception_amd import ops
    w = R.WITNESSES["dma8"]
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    shape = R.shape_for(w, cus)
    t = R.make_operands(w, shape, seed=R.SEEDS["dma8"])
    outs, routes = {}, {}
    for rs in (0, 1):
        p, _ = R.place(w, t, gpu)
        with R.knobs_set(ops, {"role_split": rs}), R.spy("uc_attention_fwd", R.FWD_FIELDS) as cap:
            ops.attention(p["q"], p["k"], ops.vt_pack(p["v"]), 0.125, v_packed=True, out=p["out"], lse=p["lse"])
            routes[rs] = _route(plan, ops, "fwd", cap)[0]
        outs[rs] = (p["out"], p["lse"])
    assert routes == {0: "dma8", 1: "rs8"}, routes
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
