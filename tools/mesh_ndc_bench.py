#!/usr/bin/env python3
"""The forward-facing scene as a world-space mesh, measured on one GPU: trains the synthetic LLFF scene of the README's

  python tools/converge.py --config bat_llff_VM_MLP --views 40 --image-size 240 --graph --llff-baseline 0.3 --gt-z-range 0.35,0.6 \\
         --gt-stairs 8 --gt-blobs 6 --gt-blob-radius 0.15,0.35

run (the same build and training, in process), extracts the NDC mesh with normals and colours, times ops.ndc_to_world and
ops.compact_mesh on it (device events after a warm-up call: the median of --reps event pairs, each round 20 back-to-back calls) and exports it with --frame.space=world,
--preview.views and --preview.check: triangles kept / beyond / far and the means of report.json.  The factor grid of the last stage
(771 x 859 x 771) is beyond the 2^27 lattice points the extractor takes, so the lattice is the factor grid divided by --shrink per
axis.  usage: python tools/mesh_ndc_bench.py [--compress 10] [--shrink 2] [--max-depth 40] [--reps 9] [--out DIR]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, reps, inner=20):
    """median device time of ONE fn() in ms: `reps` event pairs after one warm-up call, each round `inner` back-to-back calls (a
    single call of some ten microseconds is below what an event pair round a Python call resolves); and the last result"""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compress", type=float, default=10.0)
    ap.add_argument("--shrink", type=int, default=2)
    ap.add_argument("--max-depth", type=float, default=40.0)
    ap.add_argument("--views", type=int, default=8, help="preview views")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import converge
    scene = argparse.Namespace(config="bat_llff_VM_MLP", compress=a.compress, image_size=240, views=40, test_views=4, gt_res=128,
                               n_voxel_final=0, n_rays=0, noise=None, max_iter=0, test_iter=0, seed=0, graph=True, output_path=None,
                               novel_views=0, llff_baseline=0.3, llff_focus=0.0, gt_z_range="0.35,0.6", gt_wall=0.0, gt_stairs=8,
                               gt_stairs_near=0.0, gt_blobs=6, llff_zspread=0.0, gt_blob_radius="0.15,0.35")
    torch.cuda.set_device(0)
    opt, model = converge.build(scene)
    t0 = time.perf_counter()
    model.train(opt)
    torch.cuda.synchronize()
    tf = model.graph.nerf.tensorf
    grid = tf.gridSize.tolist()
    res = [max(2, g // a.shrink) for g in grid]
    print("forward-facing scene trained in %.0f s (%d iterations, compress %g): factor grid %s, mesh lattice %s, level 0.005, capped"
          % (time.perf_counter() - t0, model.it, a.compress, grid, res), flush=True)
    out_dir = a.out or tempfile.mkdtemp(prefix="mesh_ndc_")
    measure(model, opt, res, a, os.path.join(out_dir, "trained"))
    # the scene itself: the ground-truth field the supervising views were rendered from, seen from the cameras the run recovered
    from joint_tensorf_amd import synthetic
    _, gt = synthetic.gt_scene_for(opt, seed=int(opt.get("seed", 0)))
    gt.se3_refine = model.graph.se3_refine
    model.graph = gt
    print("the scene's own field (the ground truth the views were rendered from), factor grid %s = mesh lattice, level 0.005, capped; "
          "cameras: the trained run's" % (gt.nerf.tensorf.gridSize.tolist(),), flush=True)
    measure(model, opt, None, a, os.path.join(out_dir, "ground_truth"))


def measure(model, opt, res, a, out_dir):
    from joint_tensorf_amd import ops
    from joint_tensorf_amd.options import Opt
    tf = model.graph.nerf.tensorf
    sx, sy, near = model.ndc_frame(opt)
    with torch.no_grad():
        mesh = tf.extract_mesh(res=res, level=0.005, cap=True, normals=True, colors=True)
        nv, nt = mesh.vertices.shape[0], mesh.triangles.shape[0]
        print("NDC mesh: %d vertices, %d triangles; NDC map near %r sx %r sy %r" % (nv, nt, near, sx, sy))
        print("device events, one warm-up call, median of %d event pairs round 20 back-to-back calls each; ms per call" % a.reps)
        for limit in (None, a.max_depth):
            t_un, (world, wn, status) = timed(lambda: ops.ndc_to_world(mesh.vertices, sx, sy, near, normals=mesh.normals, max_depth=limit), a.reps)
            t_co, (v, t, n, c, (beyond, far)) = timed(lambda: ops.compact_mesh(world, mesh.triangles, status, normals=wn, colors=mesh.colors),
                                                      a.reps)
            # 12 B read + 12 B written per vertex and as much again for the normals, one status byte
            print("  max_depth %-6s ops.ndc_to_world (positions + normals) %8.3f ms  %6.0f GB/s | ops.compact_mesh (count, 2 scans, read, emit) "
                  "%8.3f ms | triangles kept %d beyond %d far %d; vertices kept %d of %d; depth %.3f .. %.1f"
                  % (limit, t_un, nv * 49 / t_un / 1e6, t_co, t.shape[0], beyond, far, v.shape[0], nv, float(v[:, 2].min()),
                     float(v[:, 2].max())))
    opt.mesh = Opt(dict(res=res, level=0.005, cap=True))
    opt.surface = Opt(dict(keep_largest=None, min_points=None, normals=True, colors=True))
    opt.preview = Opt(dict(views=a.views, size=None, shade="color", check=True, cull=False))
    for limit in (None, a.max_depth):
        opt.frame = Opt(dict(space="world", max_depth=limit))
        t0 = time.perf_counter()
        out = model.export_scene(opt, os.path.join(out_dir, "limit_%s" % limit))
        torch.cuda.synchronize()
        print("export --frame.space=world --frame.max_depth=%s --surface.normals=true --surface.colors=true --preview.views=%d "
              "--preview.check=true: %.1f s wall; %d vertices, %d triangles, dropped beyond %d far %d"
              % (limit, a.views, time.perf_counter() - t0, out.n_vertices, out.n_triangles, out.unwarp.n_dropped_beyond,
                 out.unwarp.n_dropped_far))
        print("  " + out.preview.summary)
        print("  report.json mean: " + json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in out.preview.means.items()}))


if __name__ == "__main__":
    main()
