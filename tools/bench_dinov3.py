"""Times the DINOv3 encoder's new pieces on the HIP path (bf16, torch.no_grad); a tool, not part of bench.py.

    python tools/bench_dinov3.py [--batch 64] [--pairs 16] [--reps 20] [--warmup 3] [--rounds 5] [--out-dir DIR]

1. uc_rope_axial on the q | k views of a packed [batch, 1024 + 5, 3, 16, 64] bf16 projection (ViT-L at 512 x 512: one launch, prefix
   tokens skipped), and in the same run uc_rope2d on the same bytes (two launches, q then k, every token) — both are one read and one
   write of the same buffer, so uc_rope2d is the yardstick.  GB/s counts the bytes each kernel has to move (read + write of the rotated
   tokens), computed from the shapes.
2. The DINOv3-L forward at 512 x 512 in pairs/s (a pair = two images; 24 blocks, 1029 tokens, the rotation as a pass of its own) and,
   next to it, the CroCo ViT-L encoder of the same tree at the same size (1024 tokens, RoPE-2D fused into the QKV GEMM's epilogue):
   the number a fused axial epilogue has to beat.  Weights are the initialisation (timing does not depend on them).

Method: everything is warmed up first; then `rounds` rounds in one process, the candidates alternating inside every round (order
reversed every other round), `reps` calls each with device events around each call; per candidate the median of each round, then the
median over the rounds and the spread (max - min of the round medians) — the noise a difference has to exceed.  Prints two JSON lines
and, with --out-dir, writes them to dinov3_rope.json / dinov3_forward.json there."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uniception_amd import engine, ops  # noqa: E402
from uniception_amd.models.encoders import CroCoEncoder, DINOv3Encoder, ViTEncoderInput  # noqa: E402
from uniception_amd.models.libs.dinov3.rope import RoPEAxial  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64, help="images of the kernel measurement")
    ap.add_argument("--pairs", type=int, default=16, help="image pairs of the forward measurement")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out-dir", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dinov3.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    common = {"device": torch.cuda.get_device_name(0), "precision": "bf16", "reps": a.reps, "rounds": a.rounds}

    # ---- 1. the kernel next to uc_rope2d -------------------------------------------------------------------------------
    B, gh, gw, prefix, H, D = a.batch, 32, 32, 5, 16, 64
    N = prefix + gh * gw
    qkv = torch.randn(B, N, 3, H, D, device=dev).to(torch.bfloat16)
    q, k = qkv[:, :, 0], qkv[:, :, 1]
    bound = RoPEAxial(D).bind(prefix, gh, gw, dev)
    pos = torch.zeros(B, N, 2, dtype=torch.int64, device=dev)
    p = torch.arange(gh * gw, device=dev)
    pos[:, prefix:, 0], pos[:, prefix:, 1] = p // gw, p % gw

    def axial():
        bound.rotate_(q, k)

    def rope2d():
        ops.rope_2d_(q, pos, 100.0, 1.0)
        ops.rope_2d_(k, pos, 100.0, 1.0)

    t = alternate({"uc_rope_axial": axial, "uc_rope2d": rope2d}, a.reps, a.warmup, a.rounds)
    nbytes = {"uc_rope_axial": 2 * B * (N - prefix) * 2 * H * D * 2, "uc_rope2d": 2 * B * N * 2 * H * D * 2}      # read + write, q and k, 2 bytes
    rope = dict(common, shape={"batch": B, "tokens": N, "prefix": prefix, "heads": H, "head_dim": D, "operands": "q | k of a packed qkv"})
    for key, (ms, spread) in t.items():
        rope[key] = {"ms": ms, "spread_ms": spread, "bytes": nbytes[key], "GB_per_s": nbytes[key] / (ms * 1e-3) / 1e9,
                     "launches": 1 if key == "uc_rope_axial" else 2}
    rope["axial_over_rope2d_time"] = t["uc_rope_axial"][0] / t["uc_rope2d"][0]
    print(json.dumps(rope))

    # ---- 2. the forward next to the fused-epilogue CroCo encoder --------------------------------------------------------
    del qkv, q, k
    n_img = 2 * a.pairs
    dino = DINOv3Encoder(name="dinov3_l", size="large").to(dev).eval()
    croco = CroCoEncoder(name="croco_l", data_norm_type="croco", img_size=(512, 512)).to(dev).eval()
    img = torch.randn(n_img, 3, 512, 512, device=dev)
    xd, xc = ViTEncoderInput(image=img, data_norm_type="dinov3"), ViTEncoderInput(image=img, data_norm_type="croco")

    def f_dino():
        with torch.no_grad(), engine.precision("bf16"):
            return dino(xd).features

    def f_croco():
        with torch.no_grad(), engine.precision("bf16"):
            return croco(xc).features

    t = alternate({"dinov3_l16_512": f_dino, "croco_l16_512_fused_rope": f_croco}, max(3, a.reps // 4), a.warmup, a.rounds)
    fwd = dict(common, pairs=a.pairs, images=n_img, size=512)
    for key, (ms, spread) in t.items():
        fwd[key] = {"tokens": 1029 if key.startswith("dinov3") else 1024, "blocks": 24, "ms": ms, "spread_ms": spread, "pairs_per_s": a.pairs / (ms * 1e-3)}
    fwd["dinov3_over_croco_time"] = t["dinov3_l16_512"][0] / t["croco_l16_512_fused_rope"][0]
    print(json.dumps(fwd))
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
        for name, rec in (("dinov3_rope.json", rope), ("dinov3_forward.json", fwd)):
            with open(os.path.join(a.out_dir, name), "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
