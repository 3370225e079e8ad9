"""Inputs of the RoPE checks against the reference's curope CPU loop (tests/golden/curope_ref.npz, make_golden_curope.py)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "curope_ref.npz")

# group -> (generator seed, [B, N, H, D] shapes, drawn in this order from one generator)
CASES = {
    "oracle": (3, ((2, 35, 3, 64), (1, 128, 2, 32))),   # tests/test_oracle_golden.py
    "ops": (4, ((2, 77, 3, 64), (1, 200, 2, 32))),      # tests/test_ops_gpu.py
}


def make_inputs(group):
    "Yields (key, tokens [B, N, H, D] fp32, positions [B, N, 2] int64) of one group, seeded as the tests always drew them."
    seed, shapes = CASES[group]
    g = torch.Generator().manual_seed(seed)
    for (B, N, H, D) in shapes:
        t = torch.randn(B, N, H, D, generator=g)
        pos = torch.randint(0, 64, (B, N, 2), generator=g)
        yield f"{group}/{B}x{N}x{H}x{D}", t, pos


def load(group):
    "Yields (key, tokens, positions, {fwd: the reference's rotation}) of one group from the committed fixture."
    z = np.load(GOLDEN)
    seed, shapes = CASES[group]
    for (B, N, H, D) in shapes:
        key = f"{group}/{B}x{N}x{H}x{D}"
        yield (key, torch.from_numpy(z[f"{key}/t"]), torch.from_numpy(z[f"{key}/pos"]),
               {1.0: torch.from_numpy(z[f"{key}/fwd"]), -1.0: torch.from_numpy(z[f"{key}/inv"])})
