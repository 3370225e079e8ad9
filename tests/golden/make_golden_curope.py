"""Golden vectors of the reference's own curope CPU loop (`rope_2d` on CPU tensors runs `rope_2d_cpu`, curope.cpp:11-46), so that
the two RoPE checks against it run without the reference's source tree:

    python -m oracle.build_ref && python -B tests/golden/make_golden_curope.py

Needs oracle/_ref/curope_ref.so (oracle/build_ref.py compiles it from the reference's curope.cpp).  Writes
tests/golden/curope_ref.npz: per case the input tokens [B, N, H, D], the positions [B, N, 2] and the reference's forward (fwd = +1)
and inverse (fwd = -1) rotations of them.  The cases and seeds are those of tests/test_oracle_golden.py (`oracle/...`, seed 3) and
tests/test_ops_gpu.py (`ops/...`, seed 4).  Data only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.curope_cases import CASES, make_inputs  # noqa: E402


def main():
    from oracle import build_ref
    ref = build_ref.load()
    if ref is None:
        raise SystemExit("oracle/_ref/curope_ref.so is not built: run `python -m oracle.build_ref` where the reference is present")
    store = {}
    for group in CASES:
        for key, t, pos in make_inputs(group):
            store[f"{key}/t"] = t.numpy()
            store[f"{key}/pos"] = pos.numpy()
            for tag, fwd in (("fwd", 1.0), ("inv", -1.0)):
                want = t.clone()
                ref.rope_2d(want, pos, 100.0, fwd)
                store[f"{key}/{tag}"] = want.numpy()
    out = os.path.join(HERE, "curope_ref.npz")
    np.savez_compressed(out, **store)
    print(f"wrote {out}: {len(store)} arrays")


if __name__ == "__main__":
    main()
