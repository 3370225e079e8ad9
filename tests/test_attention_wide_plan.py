"""CPU: the plan of every attention launch with head_dim > 64 (uniception_amd/csrc/attention_plan.h, through
tests/attention_plan_driver.cpp built with the system compiler: the one plan and the one driver of every head_dim) — each GPU witness of
tests/attention_wide_routes.py and the Pixio H/16 and 5B/16 shapes at 256 x 256 and 512 x 512 pinned line by line, the head dims without
a kernel refused with their reason — and the self-check of the per-element bound those witnesses are held to: a CPU emulation of exactly
the roundings the wide kernels perform stays inside it, each seeded fault leaves it.  (The rules of the served set, one row on each side:
FWD_RULES / BWD_RULES of tests/test_attention_plan.py.)"""
import pytest

from tests import attention_wide_routes as R


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("attention_wide_plan"))


WITNESS_PLANS = {
    "fwd80_ragged": "bf16_80 2 3 2 256 0 0", "fwd80_whole_tile": "bf16_80 2 3 2 256 0 0", "fwd80_tiny": "bf16_80 1 1 1 256 0 0",
    "fwd96_ragged": "bf16_96 2 3 2 256 0 0", "fwd96_whole_tile": "bf16_96 2 3 2 256 0 0", "fwd96_tiny": "bf16_96 1 1 1 256 0 0",
    "bwd80_ragged": "dq80 12 dkv80 6", "bwd80_two_tiles": "dq80 8 dkv80 8",
    "bwd96_ragged": "dq96 12 dkv96 6", "bwd96_two_tiles": "dq96 8 dkv96 8",
    "f32_fwd_72": "f32_96 2 2 2 128 0 0", "f32_fwd_80": "f32_96 2 2 2 128 0 0", "f32_fwd_96": "f32_96 2 2 2 128 0 0",
    "f32_bwd_80": "f32_dq96 2,2,2 f32_dkv96 1,2,2 128 3", "f32_bwd_96": "f32_dq96 2,2,2 f32_dkv96 1,2,2 128 3",
}
MODEL_PLANS = {
    "pixio_h16_256": ("bf16_80 3 16 32 256 0 0", "dq80 1536 dkv80 1536"), "pixio_h16_512": ("bf16_80 9 16 32 256 0 0", "dq80 4608 dkv80 4608"),
    "pixio_5b16_256": ("bf16_96 3 32 32 256 0 0", "dq96 3072 dkv96 3072"), "pixio_5b16_512": ("bf16_96 9 32 32 256 0 0", "dq96 9216 dkv96 9216"),
}


def test_every_witness_has_its_pinned_plan_and_every_kernel_a_witness(plan):
    assert set(WITNESS_PLANS) == set(R.WITNESSES)
    names = sorted(R.WITNESSES)
    for n, line in zip(names, plan([R.driver_row(R.WITNESSES[n]) for n in names])):
        assert line == WITNESS_PLANS[n], (n, line)
        assert R.route_of(R.WITNESSES[n]["fn"], line) == R.WITNESSES[n]["route"], n
    routes = {w["route"] for w in R.WITNESSES.values()}
    assert routes == set(R.FWD_KERNELS) | {f"{a} {b}" for a, b in zip(R.DQ_KERNELS, R.DKV_KERNELS)}


def test_the_pixio_shapes_have_their_pinned_plans(plan):
    for n, (fwd, bwd) in MODEL_PLANS.items():
        assert tuple(plan(list(R.model_rows(n)))) == (fwd, bwd), n


# head dims without a kernel are refused with their reason; head_dim 64, which the wide plan of old did not own, now gets its 64-wide plan
OUTSIDE = {(R.BF16, 112): "refused bf16_head_dim", (R.BF16, 72): "refused bf16_head_dim", (R.BF16, 128): "refused bf16_head_dim",
           (R.F32, 100): "refused f32_head_dim", (R.BF16, 64): "dma4 1 1 1 256 1 0", (R.F32, 64): "f32_64 1 1 1 128 0 0"}


@pytest.mark.parametrize("dtype,D", [(R.BF16, 112), (R.BF16, 72), (R.BF16, 128), (R.F32, 100), (R.BF16, 64), (R.F32, 64)])
def test_head_dims_outside_the_wide_path_are_refused(plan, dtype, D):
    w = R._w("fwd", "", (1, 1, 5, 3), dtype=dtype, D=D)
    assert plan([R.driver_row(w)]) == [OUTSIDE[dtype, D]]
    assert plan([R.driver_row({**w, "fn": "bwd"})])[0].split()[0] == ("refused" if D != 64 else "dq32" if dtype == R.BF16 else "f32_dq64")


# ------------------------------------------------------------------------------------------ the bound, without a GPU
EMU = [n for n, w in R.WITNESSES.items() if w["dtype"] == R.BF16]


def _run(name, fault=None):
    w = R.WITNESSES[name]
    t = R.make_operands(w, w["shape"], seed=R.SEEDS[name])
    scale = w["D"] ** -0.5
    o, lse = R.emulate_fwd(w, t, scale, fault)
    got = {"O": o, "LSE": lse}
    if w["fn"] == "bwd":
        got["dQ"], got["dK"], got["dV"] = R.emulate_bwd(w, t, o, lse, scale)
    ref = R.reference(w, t, scale)
    return {n: (got[n], *ref[n]) for n in ref}


@pytest.mark.parametrize("name", EMU)
def test_the_emulated_roundings_stay_inside_the_bound(name):
    res = _run(name)
    worst = {n: R.check(name, n, *res[n]) for n in res}
    print(name, {n: round(v, 3) for n, v in worst.items()})
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("fault", R.FAULTS)
@pytest.mark.parametrize("name", ["fwd80_ragged", "fwd96_ragged"])
def test_a_seeded_fault_leaves_the_bound(name, fault):
    res = _run(name, fault)
    over = {n: int((R.ratio(*res[n]) > 1.0).sum()) for n in ("O", "LSE")}
    print(f"fault [{fault}] on [{name}]: elements over the bound {over}")
    assert any(over.values()), f"fault [{fault}] on [{name}] stays inside the bound of every output"
