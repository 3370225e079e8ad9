"""Times the head_dim 80 / 96 attention kernels (csrc/attention_wide.hip), bf16, 32 images, at the Pixio shapes:
    H/16 at 256 x 256 and 512 x 512 (264 / 1032 tokens, 16 heads of 80)        5B/16 at 256 x 256 (264 tokens, 32 heads of 96)
forward and forward + backward, against F.scaled_dot_product_attention in bf16 on the same tensors (what a user of this model on this
GPU would otherwise run) and, for scale, against this library's head_dim-64 kernels at the shape with the same H D (H/16: 20 heads of
64; 5B/16: 48 heads of 64).  Then the whole PixioEncoder H/16 forward at 256 x 256, bf16, per block and per image.

    python tools/bench_attention_wide.py [--batch 32] [--reps 10] [--warmup 3] [--rounds 3] [--out profiles/attention_wide_bench.json]

Method (tools/bench_perception_encoder.py): every candidate is warmed up first; then `rounds` rounds in one process, the candidates of a
shape alternating inside every round, `reps` calls each with device events around each call; per candidate the median of each round,
then the median over the rounds and the spread (max - min of the round medians).  The wide forward includes its uc_vt_pack, as the
sub-layer runs it.  tflops counts 4 N^2 D FLOPs per (batch, head) forward and 2.5 x that for the backward; mfma_peak_fraction divides by
the dense bf16 peak given with --peak-tflops (default 2500).  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uniception_amd import engine, ops  # noqa: E402
from uniception_amd.models.encoders import ViTEncoderInput  # noqa: E402
from uniception_amd.models.encoders.pixio import pixio_vith16  # noqa: E402

SHAPES = {"pixio_h16_256": (264, 16, 80), "pixio_h16_512": (1032, 16, 80), "pixio_5b16_256": (264, 32, 96)}


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


def candidates(B, N, H, D):
    "{name: callable} for one shape: (ours, sdpa) x (fwd, fwd + bwd); q, k, v are slots of one fused [B, N, 3, H, D] buffer"
    g = torch.Generator(device="cuda").manual_seed(N + D)
    qkv = torch.randn(B, N, 3, H, D, device="cuda", generator=g).bfloat16()
    do = torch.randn(B, N, H, D, device="cuda", generator=g).bfloat16()
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    scale = D ** -0.5
    lse = torch.empty((B, H, N), dtype=torch.float32, device="cuda")
    dqkv = torch.empty_like(qkv)

    def ours_fwd():
        return ops.attention(q, k, ops.vt_pack(v), scale, v_packed=True, lse=lse)

    def ours_fwd_bwd():
        o = ours_fwd()
        ops.attention_bwd(q, k, v, o, do, lse, scale, out=(dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]))

    leaf = qkv.clone().requires_grad_(True)

    def sdpa_fwd():
        with torch.no_grad():
            t = qkv.permute(2, 0, 3, 1, 4)
            return F.scaled_dot_product_attention(t[0], t[1], t[2])

    def sdpa_fwd_bwd():
        leaf.grad = None
        t = leaf.permute(2, 0, 3, 1, 4)
        F.scaled_dot_product_attention(t[0], t[1], t[2]).backward(do.permute(0, 2, 1, 3))

    return {"ours_fwd": ours_fwd, "ours_fwd_bwd": ours_fwd_bwd, "sdpa_fwd": sdpa_fwd, "sdpa_fwd_bwd": sdpa_fwd_bwd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--peak-tflops", type=float, default=2500.0)
    ap.add_argument("--out", default=os.path.join("profiles", "attention_wide_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_wide.py needs a HIP device: nothing is measured without one")
    res = {"batch": a.batch, "device": torch.cuda.get_device_name(0), "precision": "bf16", "reps": a.reps, "rounds": a.rounds,
           "peak_tflops": a.peak_tflops}
    for name, (N, H, D) in SHAPES.items():
        runs = {f"d{D}_{k}": f for k, f in candidates(a.batch, N, H, D).items()}
        H64 = H * D // 64
        runs.update({f"d64_{k}": f for k, f in candidates(a.batch, N, H64, 64).items() if k.startswith("ours")})
        for f in runs.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        med = {k: [] for k in runs}
        for r in range(a.rounds):
            for key in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
                med[key].append(statistics.median(timed(runs[key], a.reps)))
        entry = {"tokens": N, "heads": H, "head_dim": D, "heads_of_64": H64}
        fwd_flops = 4.0 * N * N * D * H * a.batch
        for key, m in med.items():
            ms = statistics.median(m)
            tf = fwd_flops * (3.5 if key.endswith("fwd_bwd") else 1.0) / (ms * 1e-3) / 1e12
            entry[key] = {"ms": ms, "spread_ms": max(m) - min(m), "tflops": tf, "mfma_peak_fraction": tf / a.peak_tflops}
        for kind in ("fwd", "fwd_bwd"):
            entry[f"ours_over_sdpa_{kind}"] = entry[f"d{D}_ours_{kind}"]["ms"] / entry[f"d{D}_sdpa_{kind}"]["ms"]
            entry[f"wide_over_d64_{kind}"] = entry[f"d{D}_ours_{kind}"]["ms"] / entry[f"d64_ours_{kind}"]["ms"]
        res[name] = entry
        del runs
        torch.cuda.empty_cache()

    model = pixio_vith16().cuda().eval()
    x = ViTEncoderInput(image=torch.randn(a.batch, 3, 256, 256, device="cuda"), data_norm_type="pixio")

    def forward():
        with torch.no_grad(), engine.precision("bf16"):
            return model(x).features
    for _ in range(a.warmup):
        forward()
    torch.cuda.synchronize()
    m = [statistics.median(timed(forward, a.reps)) for _ in range(a.rounds)]
    ms = statistics.median(m)
    res["pixio_vith16_256_forward"] = {"tokens": 264, "blocks": len(model.blocks), "ms": ms, "spread_ms": max(m) - min(m),
                                       "ms_per_block": ms / len(model.blocks), "ms_per_image": ms / a.batch, "images_per_s": a.batch / (ms * 1e-3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
