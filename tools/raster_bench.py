#!/usr/bin/env python3
"""Cost of looking at an exported mesh on one GPU, call by call: the `bench.py --scene blobs` field (final 400^3 grid, twelve baked
blobs) meshed on a --res^3 lattice and drawn at --size x --size from the cameras of the novel-view turn round the scene box, one
view per call and eight -- jt_raster_project, the z-buffer fill, jt_raster_draw, jt_raster_resolve (with three colour channels),
ops.rasterize as a whole, and for context the volume render of one of the views (render_by_slices, eval mode).  Device events
after a warm-up call, the median of --reps.  usage: python tools/raster_bench.py [--res 400] [--size 800] [--reps 9] [--cull]"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--level", type=float, default=0.005)
    ap.add_argument("--cull", action="store_true")
    args = ap.parse_args()
    sys.argv = [sys.argv[0]]
    import bench
    from joint_tensorf_amd import mesh_io, novel_views, ops
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
    H = W = args.size
    with torch.no_grad():
        mesh = tf.extract_mesh(res=args.res, level=args.level, colors=True)
        V, T, colors = mesh.vertices, mesh.triangles, mesh.colors
        nv, nt = V.shape[0], T.shape[0]
        pose = novel_views.around_bbox(opt.data.scene_bbox, n=8).to(dev)
        focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)          # the field of view of the Blender image sets
        intr = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], device=dev).repeat(8, 1, 1)
        proj = mesh_io.projection_matrices(pose, intr).contiguous()
        print("mesh preview, bench.py --scene blobs field (factor grid %s), lattice %d^3, level %g: %d vertices, %d triangles, "
              "%d x %d pixels%s" % (tf.gridSize.tolist(), args.res, args.level, nv, nt, H, W, ", back faces culled" if args.cull else ""))
        print("device events, one warm-up call, median of %d; ms per VIEW" % args.reps)
        for n_views in (1, 8):
            P = proj[:n_views].contiguous()
            t_proj, screen = timed(lambda: ops.raster_project(V, P), args.reps)
            t_fill, _ = timed(lambda: torch.full((n_views, H, W), -1, device=dev, dtype=torch.int64), args.reps)
            t_draw, (zbuf, status) = timed(lambda: ops.raster_draw(screen, T, H, W, args.cull), args.reps)
            t_draw -= t_fill                                              # raster_draw allocates and fills its z-buffer
            t_res, (tri, depth, out) = timed(lambda: ops.raster_resolve(zbuf, screen, T, colors, 1.0), args.reps)
            t_all, r = timed(lambda: ops.rasterize(V, T, P, H, W, attrs=colors, cull=args.cull, background=1.0, views_per_call=8),
                             args.reps)
            counts = r.status_counts.sum(0).tolist()
            covered = float((r.tri >= 0).float().mean())
            print("  %d view%s per call" % (n_views, "" if n_views == 1 else "s"))
            print("    jt_raster_project                 %9.3f ms" % (t_proj / n_views))
            print("    z-buffer fill (8 B per pixel)     %9.3f ms" % (t_fill / n_views))
            print("    jt_raster_draw                    %9.3f ms   %.0f M triangles/s" % (t_draw / n_views, nt * n_views / t_draw / 1e3))
            print("    jt_raster_resolve, 3 channels     %9.3f ms" % (t_res / n_views))
            print("    ops.rasterize, all of the above   %9.3f ms   (with the status counts)" % (t_all / n_views))
            print("    triangles per view: %s; %.1f %% of the pixels covered"
                  % (", ".join("%s %d" % (s, c // n_views) for s, c in zip(ops.RASTER_STATUS, counts)), 100 * covered))
        # the volume render of the first view, for context
        model.graph.eval()
        opt.H, opt.W = H, W
        intr_inv = torch.linalg.inv(intr[:1])
        t_field, ret = timed(lambda: model.graph.render_by_slices(opt, pose[:1], intr_inv=intr_inv, intr=intr[:1]), max(3, args.reps // 3))
        print("  volume render of view 0 (render_by_slices)  %9.3f ms   opacity >= 0.5 on %.1f %% of the pixels"
              % (t_field, 100 * float((ret.opacity >= 0.5).float().mean())))


if __name__ == "__main__":
    main()
