"""Times the Cosmos family on the HIP path in bf16 at 512 x 512 pixels, batch 1: the CosmosEncoder(patch_size=8) forward, the
CosmosFeature(1024, 1, 8) forward (under the default head policy: fp16 maps in inference) and forward + backward (bf16), and the wide
single-head attention at the 4096 pixels those maps have.

    python tools/bench_cosmos.py [--size 512] [--warmup 10] [--reps 50] [--out profiles/cosmos_bench.json]

Every module timing is the median of `reps` calls after `warmup` calls, measured with device events around each call (a call is many
launches, 1.7 - 9 ms).  The new streaming kernels run 8 - 30 us per launch at these maps, too short for events around one launch (which
would also time the allocation of the output): their times come from a kernel trace, taken in runs of their own (no counters):

    rocprofv3 --kernel-trace --stats -f csv -d /tmp/cosmos_prof -o kernels -- python tools/bench_cosmos.py --trace-run kernels
    python tools/bench_cosmos.py --stats /tmp/cosmos_prof/kernels_kernel_stats.csv --out profiles/cosmos_stream_kernels.json
    rocprofv3 --kernel-trace --stats -f csv -d /tmp/cosmos_prof -o encoder -- python tools/bench_cosmos.py --trace-run encoder
    python tools/bench_cosmos.py --stats /tmp/cosmos_prof/encoder_kernel_stats.csv --out profiles/cosmos_encoder_p8_forward_kernel_stats.json

(--trace-run kernels_bwd -> profiles/cosmos_stream_kernels_bwd.json and --trace-run head -> profiles/cosmos_feature_p8_forward_kernel_stats.json
likewise).  --stats keeps the library's kernels (names cut at the argument list), adds PyTorch's and the runtime's up
as one row, groups the rows into steps (3x3 convolutions, attention, GroupNorm, ...) and, for a `kernels` trace, divides the bytes each
streaming step has to move — each input read once per pass over it, each output written once, computed from the shapes here — by the
sum of the average kernel times of that step.  Prints one JSON line."""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TRACE_REPS = 20
# step -> kernel-name prefixes (first match wins).  The 3x3 convolutions are the implicit-GEMM instantiations (sixth template argument 1).
STEPS = [
    ("attention_softmax", ("softmax_rows",)),
    ("transpose", ("transpose64",)),
    ("group_norm", ("gn_",)),
    ("haar", ("haar_",)),
    ("down_up_sample", ("down2_", "upsample2_")),
    ("convert_layout", ("convert", "nchw_to_nhwc", "nhwc_to_nchw")),
    ("gemm_and_conv", ("gemm", "conv")),
]


def stream_bytes(S):
    "step -> (kernel-name substrings whose average times add up to one call, bytes one call has to move) at the maps of an S x S run, bf16"
    h4, h8 = S // 4, S // 8
    img, coef64, coef48 = 3 * S * S * 4, h4 * h4 * 64 * 2, h4 * h4 * 48 * 2
    m256, m512, n = h4 * h4 * 256 * 2, h8 * h8 * 512 * 2, h8 * h8
    return {
        "haar_patch": (("haar_patch_kernel",), img + coef64),
        "haar_unpatch": (("haar_unpatch_kernel",), coef48 + img),
        "group_norm_silu": (("gn_stats_partial_kernel", "gn_stats_finalize_kernel", "gn_apply_kernel"), 3 * m256),            # x twice, y once
        "group_norm_silu_bwd": (("gn_bwd_partial_kernel", "gn_bwd_finalize_kernel", "gn_bwd_params_kernel", "gn_bwd_apply_kernel"), 5 * m256),
        "down2_gather": (("down2_gather_kernel",), m256 + 9 * m256 // 4),
        "down2_gather_bwd": (("down2_gather_bwd_kernel",), m256 + 9 * m256 // 4),
        "upsample2": (("upsample2_kernel",), 5 * m512),
        "upsample2_bwd": (("upsample2_bwd_kernel",), 5 * m512),
        "softmax_rows": (("softmax_rows_kernel",), n * n * 6),
        "softmax_rows_bwd": (("softmax_rows_bwd_kernel",), n * n * 8),
    }


def short_name(name):
    name = name[5:] if name.startswith("void ") else name
    return name.split("(")[0]


def stats(path, S):
    rows, other_ns, other_calls = [], 0.0, 0
    with open(path) as f:
        for r in csv.DictReader(f):
            name, calls, ns = short_name(r["Name"]), int(r["Calls"]), float(r["TotalDurationNs"])
            if name.startswith(("at::", "__amd_rocclr")) or "at::native" in name:
                other_ns, other_calls = other_ns + ns, other_calls + calls
            else:
                rows.append({"kernel": name, "calls": calls, "total_us": round(ns / 1e3, 1), "average_us": round(ns / calls / 1e3, 2)})
    total = sum(r["total_us"] for r in rows) + other_ns / 1e3
    steps = dict.fromkeys([s for s, _ in STEPS] + ["torch_and_runtime"], 0.0)
    steps["torch_and_runtime"] = other_ns / 1e3
    for r in rows:
        conv = r["kernel"].startswith("gemm_bf16_glds_kernel") and r["kernel"].split(",")[5].strip() == "1" if r["kernel"].count(",") >= 5 else False
        step = "conv3x3" if conv else next((s for s, pats in STEPS if r["kernel"].startswith(pats)), "other")
        steps[step] = steps.get(step, 0.0) + r["total_us"]
        r["share"] = round(r["total_us"] / total, 4)
    res = {"source": os.path.basename(path), "total_kernel_ms": round(total / 1e3, 3),
           "step_shares": {k: round(v / total, 4) for k, v in steps.items() if v}, "kernels": sorted(rows, key=lambda r: -r["total_us"]),
           "torch_and_runtime": {"calls": other_calls, "total_us": round(other_ns / 1e3, 1)}}
    rates = {}
    for step, (subs, nbytes) in stream_bytes(S).items():
        hit = [[r for r in rows if r["kernel"].startswith(sub + "<") or r["kernel"] == sub] for sub in subs]
        if all(len(h) == 1 and h[0]["calls"] >= TRACE_REPS for h in hit):       # (one instantiation of each, run as the timed step)
            us = sum(h[0]["average_us"] for h in hit)
            rates[step] = {"kernel_us": round(us, 2), "mbytes": round(nbytes / 1e6, 3), "gb_per_s": round(nbytes / us / 1e3, 1)}
    if rates:
        res["stream_rates"] = rates
    return res


def median_ms(fn, warmup, reps):
    import torch
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
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--trace-run", choices=["encoder", "head", "kernels", "kernels_bwd"], default=None,
                    help=f"run {TRACE_REPS} forwards of a module, or {TRACE_REPS} launches of every new streaming kernel (kernels_bwd: of their adjoints "
                         "/ backwards, which share kernel names with nothing else), and exit: for a kernel trace")
    ap.add_argument("--stats", default=None, help="summarise a rocprofv3 <name>_kernel_stats.csv and exit")
    a = ap.parse_args()
    S = a.size

    def emit(res):
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    if a.stats:
        emit(stats(a.stats, S))
        return

    import torch
    from uniception_amd import autograd, engine, ops
    from uniception_amd.models.encoders import CosmosEncoder, ViTEncoderInput
    from uniception_amd.models.prediction_heads import CosmosFeature, PredictionHeadInput
    assert torch.cuda.is_available(), "bench_cosmos needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    bf = torch.bfloat16
    img = torch.randn(1, 3, S, S, device=dev).clamp_(-1, 1)
    feat = torch.randn(1, 1024, S // 8, S // 8, device=dev)

    def encoder():
        enc = CosmosEncoder(name="cosmos", patch_size=8).to(dev).eval()

        def fwd():
            with torch.no_grad(), engine.precision("bf16"):
                return enc(ViTEncoderInput(image=img, data_norm_type="cosmos")).features
        return fwd

    def head():
        m = CosmosFeature(1024, 1, 8).to(dev).train()
        cot = torch.randn(1, 1, S, S, device=dev)

        def fwd():          # the default head policy: fp16 maps next to a bf16 transformer in inference
            with torch.no_grad(), engine.precision("bf16"):
                return m(PredictionHeadInput(last_feature=feat))[0].decoded_channels

        def train():
            for p in m.parameters():
                p.grad = None
            x = feat.detach().requires_grad_(True)
            with engine.precision("bf16"):
                (m(PredictionHeadInput(last_feature=x))[0].decoded_channels * cot).sum().backward()
        return fwd, train

    if a.trace_run in ("encoder", "head"):
        fn = encoder() if a.trace_run == "encoder" else head()[0]
        for _ in range(TRACE_REPS):
            fn()
        torch.cuda.synchronize()
        return
    if a.trace_run:
        h4, n, C = S // 4, (S // 8) ** 2, 512
        coef = torch.randn(1, h4, h4, 64, device=dev).to(bf)
        x256 = (torch.randn(1, h4, h4, 256, device=dev) + 0.5).to(bf)
        x512 = torch.randn(1, S // 8, S // 8, 512, device=dev).to(bf)
        g, b = torch.ones(256, device=dev), torch.zeros(256, device=dev)
        s = torch.randn(n, n, device=dev)
        if a.trace_run == "kernels":
            fns = [lambda: ops.haar_patch(img, bf, 64), lambda: ops.haar_unpatch(coef, 3), lambda: ops.group_norm_silu_nhwc(x256, g, b, 32, 1e-6),
                   lambda: ops.down2_gather(x256), lambda: ops.upsample2_nhwc(x512), lambda: ops.softmax_rows(s, C ** -0.5, bf)]
        else:
            y, mean, rstd = ops.group_norm_silu_nhwc(x256, g, b, 32, 1e-6)
            rows, up, p = ops.down2_gather(x256), ops.upsample2_nhwc(x512), ops.softmax_rows(s, C ** -0.5, bf)
            fns = [lambda: ops.group_norm_silu_nhwc_bwd(y, x256, mean, rstd, g, b), lambda: ops.down2_gather_bwd(rows, 1, h4, h4),
                   lambda: ops.upsample2_nhwc_bwd(up), lambda: ops.softmax_rows_bwd(p, s, n, C ** -0.5)]
        torch.cuda.synchronize()
        for fn in fns:
            for _ in range(TRACE_REPS):
                fn()
        torch.cuda.synchronize()
        return

    res = {"size": S, "dtype": "bf16", "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    t = lambda fn: round(median_ms(fn, a.warmup, a.reps), 4)      # noqa: E731
    res["encoder_p8_forward_ms"] = t(encoder())
    fwd, train = head()
    with torch.no_grad(), engine.precision("bf16"):
        res["feature_head_policy"] = f"{engine.head_dtype_name()} ({engine.head_dtype()} maps in inference, bf16 in training)"
    res["feature_1024_1_p8_forward_ms"] = t(fwd)
    res["feature_1024_1_p8_forward_backward_ms"] = t(train)
    del fwd, train
    N, C = (S // 8) ** 2, 512
    qkv = torch.randn(N, 3 * C, device=dev).to(bf)
    do = torch.randn(N, C, device=dev).to(bf)

    def attn_fwd():
        with torch.no_grad(), engine.precision("bf16"):
            return autograd.wide_attention(qkv, 1, N, C ** -0.5)

    def attn_train():
        x = qkv.detach().requires_grad_(True)
        with engine.precision("bf16"):
            autograd.wide_attention(x, 1, N, C ** -0.5).backward(do)
    fms = t(attn_fwd)
    res["wide_attention"] = {"pixels": N, "channels": C, "forward_ms": fms, "forward_backward_ms": t(attn_train),
                             "forward_tflops": round(4.0 * N * N * C / (fms * 1e-3) / 1e12, 2)}
    emit(res)


if __name__ == "__main__":
    main()
