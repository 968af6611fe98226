#!/usr/bin/env python3
"""Time and accuracy of ops.lpips (csrc/jt_lpips.hip) on one GPU, with seeded random weights (no trained weight file is part of
this repository).  For an 800 x 800 pair and for V = 8 pairs: ms of every convolution and pool of the batch of 2 V pictures
(device events around back-to-back calls, after a warm-up, median of rounds), the FLOP/s of each convolution against the
157.3 TFLOP/s fp32-matrix peak of the chip, and the whole ops.lpips call.  Then the accuracy figures of
tests/test_gpu_lpips.py::test_lpips_end_to_end: kernel and stock fp32 CPU ops against the fp64 evaluation of the definition.
Writes profiles/lpips.txt (or --out).
usage: python tools/lpips_bench.py [--reps 10] [--rounds 5] [--out profiles/lpips.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TFLOPS = 157.3


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def median_ms(fn, reps, rounds):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return statistics.median(timed(fn, reps) for _ in range(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lpips_bench.py measures on the GPU: none is visible")
    from joint_tensorf_amd import lpips, ops
    from tests.lpips_ref import lpips_ref, noisy_pairs, random_weights
    from tests.test_gpu_lpips import E2E_CASES
    dev = "cuda:0"
    torch.cuda.set_device(0)
    host = random_weights(0)
    weights = lpips.pack(*host, device=dev)
    lines = ["ops.lpips on %s, seeded random weights; device events around %d back-to-back calls, median of %d rounds"
             % (torch.cuda.get_device_name(0), args.reps, args.rounds), ""]
    H = W = 800
    sizes = lpips.feature_sizes(H, W)
    for V in (1, 8):
        B = 2 * V
        lines.append("V = %d (%d pictures of %d x %d per launch)" % (V, B, H, W))
        gen = torch.Generator().manual_seed(V)
        h, w, total_conv = H, W, 0.0
        for l, (_, cout, cin, k, stride, pad) in enumerate(lpips.LAYERS):
            if l in (1, 2):
                x = torch.randn(B, cin, h, w, generator=gen).to(dev)
                ms = median_ms(lambda: ops.max_pool_3x3s2(x), args.reps, args.rounds)
                lines.append("  pool%d  [%d, %d, %d, %d]: %8.3f ms" % (l, B, cin, h, w, ms))
                h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            x = torch.randn(B, cin, h, w, generator=gen).to(dev)
            oh, ow = sizes[l]
            flop = 2.0 * cin * k * k * cout * B * oh * ow
            ms = median_ms(lambda: ops.conv2d_relu(x, weights.conv[l], weights.bias[l], k, stride, pad), args.reps, args.rounds)
            total_conv += ms
            lines.append("  conv%d  %3d -> %3d %2dx%-2d on %3d x %-3d (K = %4d, %7d pixels): %8.3f ms  %6.2f GFLOP  %6.1f TFLOP/s = "
                         "%4.1f %% of %.1f" % (l + 1, cin, cout, k, k, h, w, cin * k * k, B * oh * ow, ms, flop / 1e9,
                                                 flop / ms / 1e9, 100 * flop / ms / 1e9 / PEAK_TFLOPS, PEAK_TFLOPS))
            h, w = oh, ow
        pred, target = (t.to(dev) for t in noisy_pairs(V, H, W, 0.1, seed=V))
        ms = median_ms(lambda: ops.lpips(pred, target, weights), max(2, args.reps // 2), args.rounds)
        lines.append("  convolutions together %.3f ms; ops.lpips (scale, 5 conv, 2 pool, 5 head, finish, allocation): %.3f ms = "
                     "%.3f ms per pair" % (total_conv, ms, ms / V))
        lines.append("")
    lines.append("accuracy (the cases of tests/test_gpu_lpips.py::test_lpips_end_to_end), relative to the fp64 evaluation on the CPU:")
    worst, stock = 0.0, 0.0
    for k, (h, w, V, noise) in enumerate(E2E_CASES):
        pred, target = noisy_pairs(V, h, w, noise, seed=200 + k)
        ref, _ = lpips_ref(pred, target, host)
        f32, _ = lpips_ref(pred, target, host, dtype=torch.float32)
        got = ops.lpips(pred.to(dev), target.to(dev), weights).cpu()
        rel, rel32 = float(((got - ref).abs() / ref).max()), float(((f32.double() - ref).abs() / ref).max())
        worst, stock = max(worst, rel), max(stock, rel32)
        lines.append("  %3dx%-3d V=%d noise=%.2f lpips %.6f..%.6f | kernel %.2e | stock fp32 %.2e"
                     % (h, w, V, noise, float(ref.min()), float(ref.max()), rel, rel32))
    lines.append("  largest: kernel %.2e, stock fp32 %.2e; the test allows min(8 x stock, 1e-5) = %.2e"
                 % (worst, stock, min(8 * stock, 1e-5)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
