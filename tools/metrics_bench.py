#!/usr/bin/env python3
"""Time of ops.ssim (csrc/jt_metrics.hip: two launches, fp64) on one GPU next to the stock-op fp32 formulation it replaces
(five grouped conv2d calls + the element-wise formula, tests/ssim_ref.py), measured in the same process with device events,
the two alternating, after a warm-up of every shape.  Shapes: one Blender frame, opt.optim.test_batch's 32 frames, one LLFF frame.
Prints one JSON line.
usage: python tools/metrics_bench.py [--reps 50] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 800, 800), (32, 800, 800), (1, 378, 504)]


def timed(fn, reps):
    """ms per call: `reps` back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/metrics_bench.py measures on the GPU: none is visible")
    from joint_tensorf_amd import ops
    from tests.ssim_ref import ssim_ref, smooth_pairs
    dev = "cuda:0"
    torch.cuda.set_device(0)
    rows = []
    for V, H, W in SHAPES:
        pred, target = smooth_pairs(1, H, W, 0.05, seed=1)
        pred = pred.to(dev).expand(V, 3, H, W).contiguous()
        target = target.to(dev).expand(V, 3, H, W).contiguous()
        reps = max(4, args.reps // V)

        def kernel():
            return ops.ssim(pred, target)

        def kernel_map():
            return ops.ssim(pred, target, return_map=True)

        def stock():
            return ssim_ref(pred, target, dtype=torch.float32, device=dev)[0]
        got, base = kernel(), stock()          # warm-up of both (code objects, MIOpen's choice of algorithm) and a sanity check
        kernel_map()
        for _ in range(3):
            kernel(), stock()
        torch.cuda.synchronize()
        assert float((got - base.double()).abs().max()) < 1e-3, (got, base)
        t = {"kernel": [], "kernel_with_map": [], "stock_fp32": []}
        for _ in range(args.rounds):           # alternating: what else runs on the machine hits both alike
            t["kernel"].append(timed(kernel, reps))
            t["stock_fp32"].append(timed(stock, reps))
            t["kernel_with_map"].append(timed(kernel_map, reps))
        row = {"views": V, "image": [H, W], "reps": reps, "rounds": args.rounds,
               "bytes_read": 2 * V * 3 * H * W * 4}
        for k, v in t.items():
            row[k + "_ms"] = statistics.median(v)
            row[k + "_ms_min_max"] = [min(v), max(v)]
        row["kernel_GBps_of_input"] = row["bytes_read"] / (row["kernel_ms"] * 1e-3) / 1e9
        row["speedup_over_stock_fp32"] = row["stock_fp32_ms"] / row["kernel_ms"]
        rows.append(row)
    print(json.dumps({"tool": "metrics_bench", "device": torch.cuda.get_device_name(0),
                      "timing": "device events around back-to-back calls (launch overhead of the host included), median of rounds",
                      "ssim": rows}))


if __name__ == "__main__":
    main()
