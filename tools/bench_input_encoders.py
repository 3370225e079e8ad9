"""Times the three non-image input encoders at their default sizes (518 x 518 pixels, patch 14: a 37 x 37 grid; B = 8; bf16 on the
HIP path under engine.precision("bf16")), forward and forward + backward, and uc_ln_pe_ln against the composition it replaces
(uc_layernorm, a torch add of the position table, uc_layernorm) on rows [16 * 1369, 1024].

    python tools/bench_input_encoders.py [--batch 8] [--size 518] [--reps 50] [--warmup 10] [--rounds 5]

Encoders: the median of `reps` launches after `warmup` launches, device events around each launch.
Fused against composed: `rounds` rounds in the same process, the two forms alternating inside every round (reps launches each, device
events around each launch, after a warm-up of both); per form the median of each round, then the median over the rounds and the
spread (max - min of the round medians) — the run-to-run noise a difference has to exceed.  Both forms are checked against each
other first (fp32 rows, the same formula: rel-L2 below 1e-6).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uniception_amd import engine, ops  # noqa: E402
from uniception_amd.models.encoders import (DenseRepresentationEncoder, EncoderGlobalRepInput, GlobalRepresentationEncoder,  # noqa: E402
                                            PatchEmbedder, ViTEncoderNonImageInput)


def timed(fn, reps, warmup):
    "per-launch milliseconds of `reps` launches after `warmup` launches (device events around each launch)"
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def bench_encoder(model, make_input, reps, warmup):
    model = model.cuda()

    def forward():
        with torch.no_grad(), engine.precision("bf16"):
            return model.eval()(make_input(False))

    def forward_backward():
        for p in model.parameters():
            p.grad = None
        with engine.precision("bf16"):
            out = model.train()(make_input(True)).features
            out.backward(cot)

    with torch.no_grad(), engine.precision("bf16"):
        cot = torch.randn_like(model(make_input(False)).features)
    return {"forward_ms": statistics.median(timed(forward, reps, warmup)),
            "forward_backward_ms": statistics.median(timed(forward_backward, reps, warmup))}


def bench_ln_pe_ln(rows_b, n, c, x_dtype, reps, warmup, rounds):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    x = (0.5 + torch.randn(rows_b * n, c, device=dev, generator=g)).to(x_dtype)
    pe = torch.randn(n, c, device=dev, generator=g)
    g1, b1, g2, b2 = (1 + 0.1 * torch.randn(c, device=dev, generator=g), 0.1 * torch.randn(c, device=dev, generator=g),
                      1 + 0.1 * torch.randn(c, device=dev, generator=g), 0.1 * torch.randn(c, device=dev, generator=g))

    def fused():
        return ops.ln_pe_ln(x, rows_b, n, (g1, b1, 1e-6), pe, (g2, b2, 1e-6), torch.float32)

    def composed():
        t = ops.layernorm(x, g1, b1, 1e-6, torch.float32)
        t = (t.view(rows_b, n, c) + pe).view(rows_b * n, c)
        return ops.layernorm(t, g2, b2, 1e-6, torch.float32)

    a, b = fused().double(), composed().double()
    diff = float((a - b).norm() / b.norm())
    assert diff < 1e-6, f"fused and composed forms disagree: rel-L2 {diff:.3e}"
    timed(fused, 0, warmup)
    timed(composed, 0, warmup)
    med = {"fused": [], "composed": []}
    for r in range(rounds):
        order = (("fused", fused), ("composed", composed)) if r % 2 == 0 else (("composed", composed), ("fused", fused))
        for name, fn in order:
            med[name].append(statistics.median(timed(fn, reps, 2)))
    res = {"rows": rows_b * n, "C": c, "x_dtype": str(x_dtype).replace("torch.", ""), "rel_l2_fused_vs_composed": diff}
    for name, v in med.items():
        res[name + "_ms"] = statistics.median(v)
        res[name + "_spread_ms"] = max(v) - min(v)
    res["composed_over_fused"] = res["composed_ms"] / res["fused_ms"]
    # one pass: x read once, y written once (fp32); the composition reads and writes the rows three times
    bytes_fused = rows_b * n * c * (x.element_size() + 4) + n * c * 4
    res["fused_GBps"] = bytes_fused / (res["fused_ms"] * 1e-3) / 1e9
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_encoders.py needs a HIP device: nothing is measured without one")
    B, S = a.batch, a.size
    torch.manual_seed(0)
    res = {"batch": B, "size": S, "device": torch.cuda.get_device_name(0)}

    def spatial(c):
        x = torch.randn(B, c, S, S, device="cuda")
        return lambda grad: ViTEncoderNonImageInput(data=x.detach().requires_grad_(grad))

    xg = torch.randn(B, 3, device="cuda")
    res["dense_rep_encoder"] = bench_encoder(DenseRepresentationEncoder(name="d", in_chans=3, input_size_for_pe=S), spatial(3), a.reps, a.warmup)
    res["patch_embedder"] = bench_encoder(PatchEmbedder(name="p", in_chans=3, input_size=S), spatial(3), a.reps, a.warmup)
    res["global_rep_encoder"] = bench_encoder(GlobalRepresentationEncoder(name="g", in_chans=3),
                                              lambda grad: EncoderGlobalRepInput(data=xg.detach().requires_grad_(grad)), a.reps, a.warmup)
    n = (S // 14) ** 2
    res["ln_pe_ln_fp32_rows"] = bench_ln_pe_ln(16, n, 1024, torch.float32, a.reps, a.warmup, a.rounds)
    res["ln_pe_ln_bf16_rows"] = bench_ln_pe_ln(16, n, 1024, torch.bfloat16, a.reps, a.warmup, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
