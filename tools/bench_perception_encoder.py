"""Times the Perception Encoder on the HIP path, bf16 inference (engine.precision("bf16"), torch.no_grad), 32 images:
    PE-Core-L14-336 at 336 x 336 (577 tokens, 24 blocks)       PE-Lang-L14-448 at 448 x 448 (1025 tokens, 23 blocks)
and, for comparison, the DINOv2-L/14 encoder of the same tree at the same two sizes (577 / 1025 tokens, 24 blocks): the same block
shape (width 1024, 16 heads of 64, LayerScale, erf-GELU) without RoPE, with its own token assembly.  Weights are the initialisation
(timing does not depend on them).

    python tools/bench_perception_encoder.py [--batch 32] [--reps 10] [--warmup 3] [--rounds 3]

Method: every model is warmed up at its size first; then `rounds` rounds in one process, the four (model, size) pairs alternating inside
every round, `reps` forwards each with device events around each forward; per pair the median of each round, then the median over
the rounds and the spread (max - min of the round medians) — the noise a difference has to exceed.  ms_per_block divides by the
number of blocks, which is what compares a 23-block with a 24-block tower at equal tokens.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uniception_amd import engine  # noqa: E402
from uniception_amd.models.encoders import DINOv2Encoder, PerceptionEncoder, ViTEncoderInput  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_perception_encoder.py needs a HIP device: nothing is measured without one")
    torch.manual_seed(0)
    dino = DINOv2Encoder(name="dinov2", size="large").cuda().eval()
    towers = {
        "pe_core_l14_336": (PerceptionEncoder(name="pe", size="large", checkpoint_type="core").cuda().eval(), "perception_encoder", 336),
        "pe_lang_l14_448": (PerceptionEncoder(name="pe", size="large", checkpoint_type="lang").cuda().eval(), "perception_encoder", 448),
        "dinov2_l14_336": (dino, "dinov2", 336),
        "dinov2_l14_448": (dino, "dinov2", 448),
    }
    runs = {}
    for key, (model, norm, size) in towers.items():
        x = ViTEncoderInput(image=torch.randn(a.batch, 3, size, size, device="cuda"), data_norm_type=norm)

        def forward(model=model, x=x):
            with torch.no_grad(), engine.precision("bf16"):
                return model(x).features
        runs[key] = forward
        for _ in range(a.warmup):
            forward()
    torch.cuda.synchronize()
    med = {k: [] for k in runs}
    for r in range(a.rounds):
        order = list(runs) if r % 2 == 0 else list(runs)[::-1]
        for key in order:
            med[key].append(statistics.median(timed(runs[key], a.reps)))
    res = {"batch": a.batch, "device": torch.cuda.get_device_name(0), "precision": "bf16", "reps": a.reps, "rounds": a.rounds}
    for key, (model, _, size) in towers.items():
        blocks = len(model.model.transformer.resblocks) if key.startswith("pe_") else len(model.model.blocks)
        tokens = (size // 14) ** 2 + 1
        ms = statistics.median(med[key])
        res[key] = {"tokens": tokens, "blocks": blocks, "ms": ms, "spread_ms": max(med[key]) - min(med[key]), "ms_per_block": ms / blocks,
                    "images_per_s": a.batch / (ms * 1e-3)}
    for size in (336, 448):
        pe, dn = res[f"pe_{'core' if size == 336 else 'lang'}_l14_{size}"], res[f"dinov2_l14_{size}"]
        res[f"pe_over_dinov2_per_block_{size}"] = pe["ms_per_block"] / dn["ms_per_block"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
