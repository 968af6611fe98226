#!/usr/bin/env python3
"""Cost of what the surface export adds to the mesh export on one GPU: the `bench.py --scene blobs` field (final 400^3 grid, twelve
baked blobs) on a --res^3 lattice -- the connected components of the opacity lattice (ops.lattice_components: sweeps taken, with
and without the pointer-jumping launch), the size count, the keep rule, and the two attribute passes over the mesh's vertices
(point_normals, point_colors).  Device stages are timed with device events after a warm-up call, the median of --reps; the
component loop reads its flags on the host and is timed by the wall clock around a synchronised call.
usage: python tools/mesh_surface_bench.py [--res 400] [--reps 5] [--level 0.005]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mesh_bench import timed  # noqa: E402


def wall(fn, reps):
    """median wall-clock time of a synchronised fn() in ms over `reps` calls after one warm-up call, and the last result"""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=float, default=0.005)
    args = ap.parse_args()
    sys.argv = [sys.argv[0]]
    import bench
    from joint_tensorf_amd import ops
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
    tf.kernel_density = tf.kernel_color = None
    res = (args.res,) * 3
    with torch.no_grad():
        vol = tf.dense_alpha_lattice(res)
        t_comp, labels = wall(lambda: ops.lattice_components(vol, args.level), args.reps)
        with_jump = dict(ops.last_components_stats)
        t_plain, plain = wall(lambda: ops.lattice_components(vol, args.level, jump=False), args.reps)
        without_jump = dict(ops.last_components_stats)
        assert torch.equal(labels, plain)
        t_every1, _ = wall(lambda: ops.lattice_components(vol, args.level, check_every=1), args.reps)
        t_sizes, (roots, counts) = timed(lambda: ops.component_sizes(labels), args.reps)
        t_keep, (kept_vol, kept, dropped) = wall(lambda: ops.keep_components(vol, args.level, keep_largest=1), args.reps)
        mesh = tf.extract_mesh(res=res, level=args.level)
        t_normals, (nrm, bad) = wall(lambda: tf.point_normals(mesh.vertices), args.reps)
        view = torch.where((nrm == 0).all(-1, keepdim=True), nrm.new_tensor([0.0, 0.0, -1.0]), -nrm)
        t_colors, _ = timed(lambda: tf.point_colors(mesh.vertices, view), args.reps)
        t_all, full = wall(lambda: tf.extract_mesh(res=res, level=args.level, keep_largest=1, normals=True, colors=True), args.reps)
        t_base, _ = wall(lambda: tf.extract_mesh(res=res, level=args.level), args.reps)
    order = torch.sort(counts, descending=True).values.tolist()
    print("surface export, bench.py --scene blobs field (factor grid %s), lattice %s, level %g" % (tf.gridSize.tolist(), list(res), args.level))
    print("  inside points %d of %d; %d components, sizes %s%s" % (int(counts.sum()), vol.numel(), len(order), order[:8],
                                                                 " ..." if len(order) > 8 else ""))
    print("one warm-up call, median of %d" % args.reps)
    print("  lattice_components (sweep + jump, flags read every 8)   %9.3f ms   %s" % (t_comp, with_jump))
    print("  lattice_components without pointer jumping             %9.3f ms   %s" % (t_plain, without_jump))
    print("  lattice_components, flags read after every sweep       %9.3f ms" % t_every1)
    print("  component_sizes (k_component_sizes + nonzero)          %9.3f ms" % t_sizes)
    print("  keep_components(keep_largest=1), all of the above      %9.3f ms   kept %d, dropped %d" % (t_keep, kept, dropped))
    print("  point_normals over %8d vertices                    %9.3f ms   %d degenerate" % (mesh.vertices.shape[0], t_normals, bad))
    print("  point_colors over %8d vertices                     %9.3f ms" % (mesh.vertices.shape[0], t_colors))
    print("  extract_mesh, defaults                                 %9.3f ms   %d vertices, %d triangles"
          % (t_base, mesh.vertices.shape[0], mesh.triangles.shape[0]))
    print("  extract_mesh(keep_largest=1, normals, colors)          %9.3f ms   %d vertices, %d triangles"
          % (t_all, full.vertices.shape[0], full.triangles.shape[0]))
    print("  ops.COMPONENTS_MAX_SWEEPS = %d" % ops.COMPONENTS_MAX_SWEEPS)


if __name__ == "__main__":
    main()
