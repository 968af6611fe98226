#!/usr/bin/env python3
"""Cost of the mesh export on one GPU, stage by stage: the `bench.py --scene blobs` field (final 400^3 grid, twelve baked blobs)
on a --res^3 lattice -- lattice evaluation (dense_alpha_lattice), k_mesh_count, the caller's scan (popcount + two cumsums), the
host read of the totals, k_mesh_emit, and the PLY write.  Device stages are timed with device events after a warm-up call, the
median of --reps; for the two kernels the algorithmic bytes (from the shapes) over the kernel time are set against the chip's
copy roof.  usage: python tools/mesh_bench.py [--res 400] [--reps 9] [--level 0.005] [--no-cap] [--out DIR]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_ROOF_TBS = 6.29     # measured copy roof of the MI355X


def timed(fn, reps):
    """median device time of fn() in ms over `reps` calls after one warm-up call, and the last result"""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--level", type=float, default=0.005)
    ap.add_argument("--no-cap", action="store_true")
    ap.add_argument("--out", default=None, help="directory for mesh.ply (default: a temporary one)")
    args = ap.parse_args()
    sys.argv = [sys.argv[0]]
    import bench
    from joint_tensorf_amd import mesh_io, ops
    from joint_tensorf_amd.options import make_options
    from joint_tensorf_amd.synthetic import bake_blobs
    dev = "cuda:0"
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    np.random.seed(0)
    opt = make_options("bat_blender_VM", device=dev)
    stage, it0 = bench.stage_setup(opt, -1)
    opt.nerf.n_rays = opt.train_schedule.n_rays_rest
    model = bench.build_model(opt, it0, int(opt.data.num_views))
    tf = model.graph.nerf.tensorf
    bake_blobs(tf, n_blobs=12, seed=0)
    tf.kernel_density = None
    res = (args.res,) * 3
    with torch.no_grad():
        t_lattice, vol = timed(lambda: tf.dense_alpha_lattice(res), args.reps)
        lo, hi = tf.aabb[0].tolist(), tf.aabb[1].tolist()
        if not args.no_cap:
            vol, lo, hi = ops.cap_lattice(vol, lo, hi)
        n = vol.numel()
        t_count, (flags, tris) = timed(lambda: ops.mesh_count(vol, args.level), args.reps)
        t_scan, (vo, to, totals) = timed(lambda: ops.mesh_offsets(flags, tris), args.reps)
        t0 = time.perf_counter()
        nv, nt = (int(v) for v in totals.tolist())
        t_read = (time.perf_counter() - t0) * 1e3
        t_emit, (V, T) = timed(lambda: ops.mesh_emit(vol, args.level, lo, hi, flags, vo, to, nv, nt), args.reps)
        t_whole, _ = timed(lambda: ops.mesh_from_lattice(vol, args.level, lo, hi), args.reps)
    out_dir = args.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    ply = []
    for _ in range(3):
        t0 = time.perf_counter()
        path = mesh_io.write_ply(os.path.join(out_dir, "mesh.ply"), V, T, mesh_io.mesh_comments(args.level, vol.shape, lo, hi, "world"))
        ply.append((time.perf_counter() - t0) * 1e3)
    # algorithmic bytes: the lattice read once and two bytes written per point; the lattice, the flags and both offsets read once
    # and the mesh written once
    b_count = n * (4 + 2)
    b_emit = n * (4 + 1 + 8 + 8) + nv * 12 + nt * 12

    def roof(nbytes, ms):
        tbs = nbytes / (ms * 1e-3) / 1e12
        return "%.3f GB over %.3f ms = %.2f TB/s = %.0f %% of the %.2f TB/s copy roof" % (nbytes / 1e9, ms, tbs, 100 * tbs / COPY_ROOF_TBS, COPY_ROOF_TBS)
    print("mesh export, bench.py --scene blobs field (factor grid %s), lattice %s%s, level %g: %d vertices, %d triangles"
          % (tf.gridSize.tolist(), list(res), "" if args.no_cap else " + zeros shell = %s" % list(vol.shape), args.level, nv, nt))
    print("device events, one warm-up call, median of %d" % args.reps)
    print("  lattice evaluation (dense_alpha_lattice)  %9.3f ms" % t_lattice)
    print("  k_mesh_count                              %9.3f ms   %s" % (t_count, roof(b_count, t_count)))
    print("  scan (byte popcount + two int64 cumsums)  %9.3f ms" % t_scan)
    print("  host read of the two totals               %9.3f ms   (wall clock, once)" % t_read)
    print("  k_mesh_emit                               %9.3f ms   %s" % (t_emit, roof(b_emit, t_emit)))
    print("  mesh_from_lattice, all of the above       %9.3f ms" % t_whole)
    print("  write_ply (%.1f MB, host, wall clock)     %9.3f ms   (median of 3, incl. the device-to-host copy)"
          % (os.path.getsize(path) / 1e6, statistics.median(ply)))


if __name__ == "__main__":
    main()
