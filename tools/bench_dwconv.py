"""Micro-benchmark of the DINOv3 ConvNeXt kernels (csrc/dwconv.hip); a tool, not part of bench.py.

    python tools/bench_dwconv.py [--batch 8] [--reps 20] [--warmup 3] [--rounds 5] [--out profiles/dinov3_convnext_dwconv.json]

uc_dwconv7x7_nhwc, uc_dwconv7x7_nhwc_wgrad and uc_patch2_gather_nhwc at the four stage maps of the large size for a 512 x 512 image
(128x128x192, 64x64x384, 32x32x768, 16x16x1536), batch 8, in bf16 and f32.  Per kernel and shape: the time; the bytes the kernel has to
move (computed from the shape: forward reads x and writes y, the weight gradient reads x and dy, the gather reads x and writes the
rows; weights, bias and the workspace are left out) over that time, and its ratio to the 6.29 TB/s copy rate of the MI355X; for the
forward also 49 FMAs per output element over the time, against the 78.6 T FMA/s of the fp32 vector pipe (256 CUs x 4 SIMDs x
32 lanes x 2.4 GHz), and the same depthwise convolution through torch.nn.functional.conv2d(groups=C) on a channels-last tensor of
the same dtype (tools may compare against torch; the package may not call it), with the rel-L2 distance between the two outputs.

Method: the operands rotate through a ring of buffers larger than the 256 MiB last-level cache, so a call does not find its input
there from the call before; everything is warmed up; then `rounds` rounds in one process, the candidates alternating inside every
round (order reversed every other round), `reps` calls each with device events around each call; per candidate the median of each
round, then the median over the rounds and the spread (max - min of the round medians) — the noise a difference has to exceed."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uniception_amd import ops  # noqa: E402

STAGES = [(128, 128, 192), (64, 64, 384), (32, 32, 768), (16, 16, 1536)]
COPY_TB_S = 6.29
VALU_FMA_S = 256 * 4 * 32 * 2.4e9
RING_BYTES = 640 << 20


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


def alternate(runs, reps, warmup, rounds):
    for fn in runs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    med = {k: [] for k in runs}
    for r in range(rounds):
        for key in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
            med[key].append(statistics.median(timed(runs[key], reps)))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in med.items()}


class Ring:
    "calls fn(i) with i walking round n slots"

    def __init__(self, n, fn):
        self.n, self.fn, self.i = n, fn, 0

    def __call__(self):
        self.i = (self.i + 1) % self.n
        return self.fn(self.i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dwconv.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = a.batch
    rec = {"device": torch.cuda.get_device_name(0), "batch": B, "reps": a.reps, "rounds": a.rounds, "copy_rate_TB_s": COPY_TB_S,
           "valu_fma_per_s": VALU_FMA_S, "ring_bytes": RING_BYTES, "results": []}
    for dtype, dname in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        for H, W, C in STAGES:
            n = B * H * W * C
            nbytes = 2 * n * dtype.itemsize                                # one map read + one map written (or two read)
            slots = max(2, -(-RING_BYTES // nbytes))
            xs = [torch.randn(B, H, W, C, device=dev).to(dtype) for _ in range(slots)]
            dys = [torch.randn(B, H, W, C, device=dev).to(dtype) for _ in range(slots)]
            w = torch.randn(C, 1, 7, 7, device=dev)
            bias = torch.randn(C, device=dev)
            w49 = w.reshape(C, 49).t().contiguous()
            wt = w.to(dtype).contiguous(memory_format=torch.channels_last)
            bt = bias.to(dtype)
            xt = [x.permute(0, 3, 1, 2) for x in xs]                       # NCHW-shaped channels-last views of the same storage
            ws = torch.empty(max(1, ops._lib.load().uc_dwconv7x7_nhwc_wgrad_ws_bytes(B, H, W, C) // 4), device=dev)
            runs = {
                "uc_dwconv7x7_nhwc": Ring(slots, lambda i: ops.dwconv7x7_nhwc(xs[i], w49, bias)),
                "torch_conv2d_groups_channels_last": Ring(slots, lambda i: torch.nn.functional.conv2d(xt[i], wt, bt, padding=3, groups=C)),
                "uc_dwconv7x7_nhwc_wgrad": Ring(slots, lambda i: ops.dwconv7x7_nhwc_wgrad(xs[i], dys[i], ws=ws)),
                "uc_patch2_gather_nhwc": Ring(slots, lambda i: ops.patch2_gather_nhwc(xs[i])),
            }
            t = alternate(runs, a.reps, a.warmup, a.rounds)
            ours = ops.dwconv7x7_nhwc(xs[0], w49, bias).float()
            theirs = torch.nn.functional.conv2d(xt[0], wt, bt, padding=3, groups=C).permute(0, 2, 3, 1).float()
            row = {"dtype": dname, "shape": [B, H, W, C], "bytes_moved": nbytes, "ring_slots": slots,
                   "rel_l2_vs_torch": float((ours - theirs).norm() / theirs.norm())}
            for key, (ms, spread) in t.items():
                row[key] = {"ms": ms, "spread_ms": spread, "TB_per_s": nbytes / (ms * 1e-3) / 1e12, "of_copy_rate": nbytes / (ms * 1e-3) / 1e12 / COPY_TB_S}
            for key in ("uc_dwconv7x7_nhwc", "torch_conv2d_groups_channels_last"):
                row[key]["of_valu_fma_peak"] = 49 * n / (t[key][0] * 1e-3) / VALU_FMA_S
            row["ours_over_torch_time"] = t["uc_dwconv7x7_nhwc"][0] / t["torch_conv2d_groups_channels_last"][0]
            rec["results"].append(row)
            print(json.dumps(row), flush=True)
            del xs, dys, xt
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
