"""Times MoGeConvFeature in the reference's own example configuration (patch 14, features [1024, 768, 768, 768], dim_out [2, 1],
defaults otherwise) on 37 x 37 patches (518 x 518 pixels), forward and forward + backward, in bf16 on the HIP path
(uniception_amd.models.prediction_heads.MoGeConvFeature under engine.precision("bf16")) against the SAME nn layers (the module's own
Conv2d / ConvTranspose2d / GroupNorm objects, so the same weights) run by PyTorch under torch.autocast(bfloat16) on the same GPU.

    python tools/bench_moge_head.py [--batch 8] [--grid 37] [--reps 50]

Every timing is the median of `reps` launches after `warmup` launches, measured with device events around each launch.  Prints one
JSON line with the four medians (ms) and the two ratios torch / hip (> 1: the HIP path is faster).

Share of the forward spent in the pad / crop passes and in GroupNorm — from a kernel trace taken in a run of its own (no counters):

    rocprofv3 --kernel-trace --stats -d /tmp/moge_prof -o moge -- python tools/bench_moge_head.py --forward-only 5
    python tools/bench_moge_head.py --stats /tmp/moge_prof/moge_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uniception_amd import engine  # noqa: E402
from uniception_amd.models.prediction_heads import (MoGeConvFeature, PredictionHeadLayeredInput, ResidualConvBlock,  # noqa: E402
                                                    normalized_view_plane_uv)

DIMS = [1024, 768, 768, 768]


def torch_forward(head, feats, shape):
    "the head's layers called by PyTorch itself, in the order of the published architecture (microsoft/MoGe v1 decoder)"
    img_h, img_w = shape

    def uv_cat(x):
        uv = normalized_view_plane_uv(width=x.shape[-1], height=x.shape[-2], aspect_ratio=img_w / img_h, dtype=x.dtype, device=x.device)
        return torch.cat([x, uv.permute(2, 0, 1).unsqueeze(0).expand(x.shape[0], -1, -1, -1)], dim=1)

    def run(layer, x):
        return layer.skip_connection(x) + layer.layers(x) if isinstance(layer, ResidualConvBlock) else layer(x)

    x = torch.stack([proj(f) for proj, f in zip(head.projects, feats)], dim=1).sum(dim=1)
    for block in head.upsample_blocks:
        x = uv_cat(x)
        for layer in block:
            x = run(layer, x)
    x = uv_cat(F.interpolate(x, (img_h, img_w), mode="bilinear", align_corners=False))
    outs = []
    for block in head.output_block:
        y = x
        for layer in block:
            y = run(layer, y.clone() if isinstance(layer, nn.ReLU) else y)
        outs.append(y)
    return torch.cat(outs, dim=1)


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


def stats_shares(path):
    "shares of the total kernel time per family, from rocprofv3's <name>_kernel_stats.csv"
    # (first match wins: the scatter of the transposed convolution before the GEMM / convolution family, whose patterns it contains)
    fam = {"group_norm": ("gn_",), "pad_crop": ("replicate_pad", "crop_add", "crop_embed"), "resize": ("resize_halfpix",),
           "scatter": ("convt_scatter",), "gemm_conv": ("gemm", "conv")}
    tot, acc = 0.0, dict.fromkeys(fam, 0.0)
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
            tot += ns
            for k, pats in fam.items():
                if any(p in name for p in pats):
                    acc[k] += ns
                    break
    return {"total_ms": round(tot / 1e6, 3), **{k + "_share": round(v / tot, 4) for k, v in acc.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--grid", type=int, default=37)
    ap.add_argument("--patch", type=int, default=14)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--forward-only", type=int, default=0, help="run this many HIP forwards and exit (for a kernel trace)")
    ap.add_argument("--stats", default=None, help="print the kernel-time shares of a rocprofv3 kernel_stats.csv and exit")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(stats_shares(a.stats)))
        return
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    head = MoGeConvFeature(patch_size=a.patch, num_features=4, input_feature_dims=DIMS, dim_out=[2, 1]).to(dev).train()
    shape = (a.grid * a.patch, a.grid * a.patch)
    feats = [torch.randn(a.batch, d, a.grid, a.grid, device=dev) for d in DIMS]
    cot = torch.randn(a.batch, 3, *shape, device=dev)

    def hip_fwd():
        with torch.no_grad(), engine.head_precision("follow"), engine.precision("bf16"):
            return head(PredictionHeadLayeredInput(list_features=feats, target_output_shape=shape)).decoded_channels

    def ref_fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return torch_forward(head, feats, shape)

    def hip_train():
        for p in head.parameters():
            p.grad = None
        xs = [f.detach().requires_grad_(True) for f in feats]
        with engine.precision("bf16"):
            (head(PredictionHeadLayeredInput(list_features=xs, target_output_shape=shape)).decoded_channels * cot).sum().backward()

    def ref_train():
        for p in head.parameters():
            p.grad = None
        xs = [f.detach().requires_grad_(True) for f in feats]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = torch_forward(head, xs, shape)
        (out.float() * cot).sum().backward()

    if a.forward_only:
        for _ in range(a.forward_only):
            hip_fwd()
        torch.cuda.synchronize()
        return
    ref = ref_fwd().float()
    diff = float((hip_fwd() - ref).norm() / ref.norm())
    del ref
    res = {"batch": a.batch, "grid": a.grid, "patch": a.patch, "image": list(shape), "warmup": a.warmup, "reps": a.reps, "rel_l2_hip_vs_torch": diff}
    for name, fh, ft in (("forward", hip_fwd, ref_fwd), ("forward_backward", hip_train, ref_train)):
        h, t = median_ms(fh, a.warmup, a.reps), median_ms(ft, a.warmup, a.reps)
        res[f"{name}_hip_ms"], res[f"{name}_torch_ms"], res[f"{name}_torch_over_hip"] = round(h, 4), round(t, 4), round(t / h, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
