#!/usr/bin/env python3
"""Cost and effect of simplifying an exported mesh on one GPU (ops.simplify_mesh; csrc/jt_simplify.hip): the `bench.py --scene
blobs` field (final 400^3 grid, twelve baked blobs) meshed on a --res^3 lattice with its normals, as tools/raster_bench.py has it,
then clustered in cells of K = 2, 4, 8 lattice spacings.  Per K the stages are timed separately -- jt_simplify_keys; the stable
sort, the scan and the host read of the cluster count; the index arrays; jt_simplify_clusters; jt_simplify_triangles; the
compaction (two cumsums, the host read, jt_mesh_filter_emit) -- with device events round a synchronised call (the stages with
a host read wait for it inside the pair), one warm-up call, the median of --reps; then ops.simplify_mesh as a whole by the wall
clock.  The effect is reported the way `--preview.check` scores a mesh: drawn at --size x --size from the eight cameras of the
novel-view turn round the scene box against the volume render of the same cameras -- IoU of the covered pixels with the
field's opacity >= 0.5, and the median depth difference where the field is solid (opacity >= 0.99) -- for the unsimplified mesh
and for every K.  It reports; it judges nothing.
usage: python tools/mesh_simplify_bench.py [--res 400] [--size 400] [--reps 9] [--cells 2,4,8]"""
import argparse
import math
import os
import statistics
import sys
import time

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


def walled(fn, reps):
    """median wall time of a synchronised fn() in ms"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--level", type=float, default=0.005)
    ap.add_argument("--cells", default="2,4,8", help="cell edges K in lattice spacings")
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
        t_extract = walled(lambda: tf.extract_mesh(res=args.res, level=args.level), max(3, args.reps // 3))
        mesh = tf.extract_mesh(res=args.res, level=args.level, normals=True)
        V, T, N = mesh.vertices, mesh.triangles, mesh.normals
        nv, nt = V.shape[0], T.shape[0]
        print("mesh simplification, bench.py --scene blobs field (factor grid %s), lattice %s (capped), level %g: %d vertices, %d "
              "triangles; extract_mesh, defaults %.3f ms (wall)" % (tf.gridSize.tolist(), list(mesh.shape), args.level, nv, nt, t_extract))
        # the field at the eight cameras, once
        pose = novel_views.around_bbox(opt.data.scene_bbox, n=8).to(dev)
        focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)          # the field of view of the Blender image sets
        intr = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], device=dev).repeat(8, 1, 1)
        proj = mesh_io.projection_matrices(pose, intr).contiguous()
        intr_inv = torch.linalg.inv(intr)
        model.graph.eval()
        opt.H, opt.W = H, W
        field = []
        for j in range(8):
            ret = model.graph.render_by_slices(opt, pose[j:j + 1], intr_inv=intr_inv[j:j + 1], intr=intr[j:j + 1])
            field.append((ret.opacity.view(H, W).clone(), (ret.depth.view(H, W) + float(tf.near_far[0]) - 0.05).clone()))

        def score(vertices, triangles):
            """(mean IoU, mean of the per-view median |depth difference|) over the eight views, as preview_scene's report has them"""
            drawn = ops.rasterize(vertices, triangles, proj, H, W, views_per_call=8)
            ious, depths = [], []
            for j, (opacity, depth_f) in enumerate(field):
                m, f = drawn.tri[j] >= 0, opacity >= 0.5
                union = (m | f).sum()
                ious.append(float((m & f).sum() / union) if int(union) else 1.0)
                solid = m & (opacity >= 0.99)
                if int(solid.sum()):
                    depths.append(float((drawn.depth[j] - depth_f)[solid].abs().median()))
            return sum(ious) / len(ious), (sum(depths) / len(depths) if depths else float("nan"))
        iou0, depth0 = score(V, T)
        spacing = (mesh.hi[0] - mesh.lo[0]) / (mesh.shape[0] - 1)
        print("device events round each stage, one warm-up call, median of %d; ms.  IoU / median depth difference: 8 views of %d x %d "
              "against the volume render (a lattice spacing is %.4f)" % (args.reps, H, W, spacing))
        print("  unsimplified                         %8d vertices %8d triangles   IoU %.4f   depth %.5f" % (nv, nt, iou0, depth0))
        for K in (float(k) for k in args.cells.split(",")):
            cells = [int(math.ceil((n - 1) / K)) for n in mesh.shape]
            none = cells[0] * cells[1] * cells[2]
            t_keys, keys = timed(lambda: ops.simplify_keys(V, mesh.lo, mesh.hi, cells), args.reps)

            def segments():
                seg = ops.simplify_segments(keys, none)
                return seg[:4] + tuple(int(v) for v in seg[4].tolist())
            t_sort, (order, head, cid, valid, nc, n_valid) = timed(segments, args.reps)
            t_index, (seg_start, cluster) = timed(lambda: ops.simplify_index(order, head, cid, valid, nc, n_valid), args.reps)
            t_clusters, (c_pos, c_nrm, c_cnt) = timed(lambda: ops.simplify_clusters(V, N, order, seg_start), args.reps)
            t_tris, (tri, keep, cause, used) = timed(lambda: ops.simplify_triangles(T, cluster, nc), args.reps)
            t_compact, (v, t, n, c, (n_invalid, n_collapsed)) = timed(lambda: ops.simplify_compact(c_pos, c_nrm, c_cnt, tri, keep, cause, used),
                                                                      args.reps)
            t_all = walled(lambda: ops.simplify_mesh(V, T, N, mesh.lo, mesh.hi, cells), args.reps)
            iou, depth = score(v, t)
            total = t_keys + t_sort + t_index + t_clusters + t_tris + t_compact
            print("  K = %g, cells %s: %d clusters, members per cluster mean %.1f max %d" % (K, cells, nc, nv / nc, int(c_cnt.max())))
            print("    jt_simplify_keys                    %9.3f ms" % t_keys)
            print("    stable sort, scan, host read        %9.3f ms" % t_sort)
            print("    seg_start and cluster (scatters)    %9.3f ms" % t_index)
            print("    jt_simplify_clusters                %9.3f ms" % t_clusters)
            print("    jt_simplify_triangles               %9.3f ms" % t_tris)
            print("    compaction (2 scans, read, emit)    %9.3f ms" % t_compact)
            print("    sum of the stages                   %9.3f ms   ops.simplify_mesh, wall %9.3f ms" % (total, t_all))
            print("    out                                 %8d vertices %8d triangles   IoU %.4f   depth %.5f   (invalid %d, collapsed %d)"
                  % (v.shape[0], t.shape[0], iou, depth, n_invalid, n_collapsed))


if __name__ == "__main__":
    main()
