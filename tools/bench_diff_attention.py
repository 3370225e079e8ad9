"""Times the fused differential-attention forward (uc_diff_attention_fwd) against the composed alternative on today's plain kernels:
two uc_attention_fwd launches on Q / K zero-padded to head_dim 64 over the same packed V, then the elementwise combine
(a = A1 - lambda A2, RMSNorm, scale) as PyTorch elementwise passes.

    python tools/bench_diff_attention.py [--bh 384] [--n 1024] [--reps 50]

bf16, B*H = 32*12, N = 1024, Q/K head_dim 32 by default.  Every timing is the median of `reps` launches after `warmup` launches,
measured with device events around each launch; the composed path's padding of Q / K and the packing of V are outside the timed region
(both paths get their operands ready-made)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uniception_amd import ops  # noqa: E402


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, N, hd = a.batch, a.heads, a.n, 32
    g = torch.Generator(device="cpu").manual_seed(0)
    q = torch.randn(B, N, 2 * H, hd, generator=g).to(dev, torch.bfloat16)
    k = torch.randn(B, N, 2 * H, hd, generator=g).to(dev, torch.bfloat16)
    v = torch.randn(B, N, H, 2 * hd, generator=g).to(dev, torch.bfloat16)
    w = torch.ones(2 * hd, device=dev)
    vt = ops.vt_pack(v)
    lam, eps, c, scale = 0.37, 1e-5, 0.64, hd ** -0.5
    out = torch.empty(B, N, H, 2 * hd, device=dev, dtype=torch.bfloat16)

    def fused():
        ops.diff_attention(q, k, vt, scale, lam, w, eps, c, out=out, v_packed=True)

    qp = [torch.zeros(B, N, H, 64, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    kp = [torch.zeros(B, N, H, 64, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    for i in range(2):
        qp[i][..., :hd] = q[:, :, i * H:(i + 1) * H]
        kp[i][..., :hd] = k[:, :, i * H:(i + 1) * H]
    o = [torch.empty(B, N, H, 64, device=dev, dtype=torch.bfloat16) for _ in range(2)]

    def attn_only():
        ops.attention(qp[0], kp[0], vt, scale, v_packed=True, out=o[0])
        ops.attention(qp[1], kp[1], vt, scale, v_packed=True, out=o[1])

    def composed():
        attn_only()
        x = o[0] - lam * o[1]
        n = (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)).to(torch.bfloat16) * w.to(torch.bfloat16)
        return n * c

    res = dict(shape=dict(B=B, H=H, N=N, hd=hd), fused_ms=median_ms(fused, a.warmup, a.reps),
               two_attention_launches_ms=median_ms(attn_only, a.warmup, a.reps), composed_ms=median_ms(composed, a.warmup, a.reps))
    res["composed_over_fused"] = res["composed_ms"] / res["fused_ms"]
    ref = composed().float()
    res["max_abs_diff_vs_composed"] = float((out.float() - ref).abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
