"""bench.py --dump-outputs on the host: what a caller of the timed step receives, written as float32 .npy files, whole within the
byte budget and beyond it a seeded sample of rows that is the same from run to run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _forward_like(B=2, H=8, W=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    res1 = {"pts3d": torch.randn(B, H, W, 3, generator=g), "conf": torch.rand(B, H, W, 1, generator=g) + 1}
    res2 = {"pts3d_in_other_view": torch.randn(B, H, W, 3, generator=g), "conf": torch.rand(B, H, W, 1, generator=g) + 1}
    return res1, res2


def test_step_outputs_names_what_the_caller_receives():
    out = _forward_like()
    arrs = bench.step_outputs(out, "fwd")
    assert sorted(arrs) == ["view1_conf", "view1_pts3d", "view2_conf", "view2_pts3d_in_other_view"]
    assert arrs["view2_pts3d_in_other_view"] is out[1]["pts3d_in_other_view"]
    loss = torch.tensor([1.5])
    assert bench.step_outputs(({"pts3d": loss},), "train") == {"loss": loss}


def test_dump_within_budget_writes_everything_in_float32(tmp_path):
    out = _forward_like()
    arrs = bench.step_outputs(out, "fwd")
    arrs["view1_conf"] = arrs["view1_conf"].double()
    bench.dump_outputs(arrs, str(tmp_path))
    for name, t in arrs.items():
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.float().numpy())


def test_dump_beyond_budget_is_a_fixed_sample_of_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    arrs = bench.step_outputs(_forward_like(B=4, H=16, W=16), "fwd")
    total_in = sum(t.numel() for t in arrs.values()) * 4
    assert total_in > 4 * 4096
    info = bench.dump_outputs(arrs, str(tmp_path / "a"))
    bench.dump_outputs(arrs, str(tmp_path / "b"))
    written = 0
    for name, t in arrs.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)                  # same arguments, same sample
        rows = t.reshape(-1, t.shape[-1]).numpy()
        assert a.shape[1] == t.shape[-1] and 0 < a.shape[0] < rows.shape[0]
        assert info[name]["rows_written"] == a.shape[0] and info[name]["rows"] == rows.shape[0]
        # every written row is a row of the output, in ascending order of position
        pos = [int(np.flatnonzero((rows == r).all(axis=1))[0]) for r in a]
        assert pos == sorted(pos) and len(set(pos)) == len(pos)
        written += a.nbytes
    assert written <= 4096
    # views of one shape keep the same rows (pts3d and conf of one pixel stay together)
    p = np.load(tmp_path / "a" / "view1_pts3d.npy")
    c = np.load(tmp_path / "a" / "view1_conf.npy")
    rows_p = arrs["view1_pts3d"].reshape(-1, 3).numpy()
    rows_c = arrs["view1_conf"].reshape(-1, 1).numpy()
    ip = [int(np.flatnonzero((rows_p == r).all(axis=1))[0]) for r in p]
    ic = [int(np.flatnonzero((rows_c == r).all(axis=1))[0]) for r in c]
    assert ip == ic


def test_plain_and_full_are_separate_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    args = bench.parse()
    assert args.steps == 4 and args.warmup == 2 and args.full is False and args.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "d"
