#!/usr/bin/env python3
"""Where the waves of k_shade_scatter spend their time, and how far apart its workgroups end (profiling build:
   python tools/build_variant.py sstamp -DJT_SCATTER_STAMP=1
   JT_LIB_PATH=joint_tensorf_amd/lib/variants/sstamp.so [JT_SCATTER_CLAIM=0|1] python tools/stamp_scatter.py)
Runs the default bench workload (10 steps) and prints the table of profiles/scatter_pass_skew.txt."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RING, WGS = 32, 256


def main():
    import torch  # noqa: F401
    from joint_tensorf_amd import _lib
    sys.argv = ["bench.py", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--no-probe", "--no-torch-baseline", "--no-extras"]
    import runpy
    fn = _lib.lib.jt_debug_read_scatter_stamps
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    try:
        runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
    except SystemExit:
        pass
    n = 24 + RING * WGS * 4
    out = (ctypes.c_ulonglong * n)()
    assert fn(out, n) == 0
    acc = [int(out[i]) for i in range(24)]
    waves, launches, batches = max(acc[16], 1), max(acc[17], 1), acc[18]
    tot = sum(acc[:16])
    print("JT_SCATTER_CLAIM=%s: %d launches, %d waves, %.1f batches per wave and pass; s_memtime ticks per wave and launch: %.0f"
          % (os.environ.get("JT_SCATTER_CLAIM", "(default)"), launches, waves // launches, batches / (3.0 * waves), tot / waves))
    rows = [("set-up in front of the plane loop", [0])]
    for name, k in (("basis image, line reset (to the barrier)", 1), ("batch loop", 2), ("wait at the pass-end barrier", 3),
                    ("line flush", 4), ("dBasis slab sum", 5)):
        rows.append((name, [k, k + 5, k + 10]))
    for name, ks in rows:
        v = [acc[k] / waves for k in ks]
        print("  %-44s %9.0f  %5.2f %%   %s" % (name, sum(v), 100.0 * sum(acc[k] for k in ks) / tot,
                                               "planes " + " ".join("%.0f" % x for x in v) if len(ks) > 1 else ""))
    # the workgroups' pass ends, on the device-wide 100 MHz clock: what the last pass end of a workgroup lacks to the launch's last
    slots = []
    for s in range(RING):
        wg = []
        for b in range(WGS):
            w = [int(out[24 + (s * WGS + b) * 4 + j]) for j in range(4)]
            if w[0] and w[3] > w[0]:
                wg.append(w)
        if len(wg) >= 8:
            slots.append(wg)
    if not slots:
        return
    idle_all, idle_label, dur, per_label = [], [], [], [[] for _ in range(8)]
    for wg in slots:
        t0, t1 = min(w[0] for w in wg), max(w[3] for w in wg)
        dur.append((t1 - t0) * 0.01)
        g = min(len(wg), 8)
        lab_end = [max(w[3] for i, w in enumerate(wg) if i % g == x) for x in range(g)]
        for i, w in enumerate(wg):
            idle_all.append((t1 - w[3]) * 0.01)
            idle_label.append((lab_end[i % g] - w[3]) * 0.01)
        for x in range(g):
            per_label[x].append((lab_end[x] - t0) * 0.01)
    mean = lambda v: sum(v) / max(len(v), 1)
    d = mean(dur)
    print("workgroup pass ends over %d recorded launches of %d workgroups (100 MHz device clock, us):" % (len(slots), len(slots[0])))
    print("  launch, first workgroup start to last pass end   mean %8.1f   min %8.1f   max %8.1f" % (d, min(dur), max(dur)))
    print("  a workgroup's last pass end before the launch's last                mean %6.1f  (%4.2f %% of the launch)   max %6.1f"
          % (mean(idle_all), 100.0 * mean(idle_all) / d, max(idle_all)))
    print("  ... before the last of its own XCD label                            mean %6.1f  (%4.2f %% of the launch)   max %6.1f"
          % (mean(idle_label), 100.0 * mean(idle_label) / d, max(idle_label)))
    print("  last pass end of each XCD label after the launch's start, mean: " + " ".join("%.1f" % mean(v) for v in per_label if v))


if __name__ == "__main__":
    main()
