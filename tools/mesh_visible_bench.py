#!/usr/bin/env python3
"""Cost and effect of exporting only the surface the cameras see on one GPU (ops.triangle_visibility / grow_triangles /
select_triangles, extract_mesh(visible=); csrc/jt_visible.hip): the `bench.py --scene blobs` field (final 400^3 grid, twelve baked
blobs) meshed on a --res^3 lattice as the other mesh tools have it, plain and simplified in cells of K lattice spacings, seen
from a turn of --views cameras round the scene box (novel_views.around_bbox) at --size x --size.  Every second camera DECIDES
what is seen; the others only judge the result.

Per mesh the stages are timed separately with device events round a synchronised call, one warm-up call, the median of --reps:
project + draw and the tally in both forms (one atomic per run of a wave, one per pixel: JT_VISIBLE_RUNS) for one slab of eight
views, the fold of that slab, one ring of growth, the selection; then the whole decision over all deciding views by the wall
clock.  The effect: triangle and vertex counts and the atlas size at S = 8 before and after, and what `--preview.check` reports
-- iou, depth_abs_median, coverage_mesh against the volume render -- before and after, from --judge of the deciding cameras and
from --judge of the others.  It reports; it judges nothing.
usage: python tools/mesh_visible_bench.py [--res 400] [--size 800] [--views 100] [--judge 8] [--reps 9] [--cells 0,4] [--grow 1]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, default=100, help="cameras of the turn; every second one decides")
    ap.add_argument("--judge", type=int, default=8, help="cameras of each kind the check is made from")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--level", type=float, default=0.005)
    ap.add_argument("--cells", default="0,4", help="cell edges K in lattice spacings; 0: the plain mesh")
    ap.add_argument("--grow", type=int, default=1)
    args = ap.parse_args()
    sys.argv = [sys.argv[0]]
    import bench
    from mesh_simplify_bench import timed, walled
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
    slab = 8

    def spaced(idx, k):
        k = min(k, len(idx))
        return [idx[int(round(i * (len(idx) - 1) / max(k - 1, 1)))] for i in range(k)]
    with torch.no_grad():
        pose = novel_views.around_bbox(opt.data.scene_bbox, n=args.views).to(dev)
        focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)          # the field of view of the Blender image sets
        intr = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], device=dev).repeat(args.views, 1, 1)
        proj = mesh_io.projection_matrices(pose, intr).contiguous()
        deciding, others = list(range(0, args.views, 2)), list(range(1, args.views, 2))
        judges = {"deciding": spaced(deciding, args.judge), "other": spaced(others, args.judge)}
        intr_inv = torch.linalg.inv(intr)
        model.graph.eval()
        opt.H, opt.W = H, W
        field = {}
        for j in sorted(set(judges["deciding"] + judges["other"])):
            ret = model.graph.render_by_slices(opt, pose[j:j + 1], intr_inv=intr_inv[j:j + 1], intr=intr[j:j + 1])
            field[j] = (ret.opacity.view(H, W).clone(), (ret.depth.view(H, W) + float(tf.near_far[0]) - 0.05).clone())

        def check(V, T, idx):
            """means over the cameras idx of coverage_mesh, iou and depth_abs_median as preview_scene's report has them"""
            drawn = ops.rasterize(V, T, proj[idx].contiguous(), H, W, views_per_call=slab)
            cov, iou, dep = [], [], []
            for k, j in enumerate(idx):
                opacity, depth_f = field[j]
                m, f = drawn.tri[k] >= 0, opacity >= 0.5
                union = (m | f).sum()
                solid = m & (opacity >= 0.99)
                cov.append(float(m.float().mean()))
                iou.append(float((m & f).sum() / union) if int(union) else 1.0)
                if int(solid.sum()):
                    dep.append(float((drawn.depth[k] - depth_f)[solid].abs().median()))
            return sum(cov) / len(cov), sum(iou) / len(iou), sum(dep) / len(dep) if dep else float("nan")

        def atlas(nt):
            try:
                lay = ops.texture_layout(nt, 8)
                return "%d x %d" % (lay.width, lay.height)
            except ValueError:
                return "beyond the 16384-texel limit"
        print("visible surface, bench.py --scene blobs field (factor grid %s), lattice %d^3 (capped), level %g; a turn of %d cameras at "
              "%d x %d, %d deciding, %d judging of each kind; grow %d" % (tf.gridSize.tolist(), args.res, args.level, args.views, H, W,
                                                                       len(deciding), len(judges["deciding"]), args.grow))
        print("device events round each stage, one warm-up call, median of %d; ms" % args.reps)
        P = proj[deciding].contiguous()
        for K in (float(k) for k in args.cells.split(",")):
            mesh = tf.extract_mesh(res=args.res, level=args.level, normals=True, **({"simplify": K} if K else {}))
            V, T, N = mesh.vertices, mesh.triangles, mesh.normals
            nv, nt = V.shape[0], T.shape[0]
            print("  %s: %d vertices, %d triangles, atlas at S = 8: %s" % ("K = %g" % K if K else "plain", nv, nt, atlas(nt)))
            Ps = P[:slab].contiguous()
            t_draw, (screen, (zbuf, status)) = timed(lambda: (lambda s: (s, ops.raster_draw(s, T, H, W)))(ops.raster_project(V, Ps)), args.reps)
            os.environ.pop("JT_VISIBLE_RUNS", None)
            t_runs, pix = timed(lambda: ops.visible_tally(zbuf, nt), args.reps)
            os.environ["JT_VISIBLE_RUNS"] = "0"
            t_plain, pix_plain = timed(lambda: ops.visible_tally(zbuf, nt), args.reps)
            os.environ.pop("JT_VISIBLE_RUNS", None)
            assert torch.equal(pix, pix_plain)
            t_fill, _ = timed(lambda: torch.zeros(Ps.shape[0], nt, device=dev, dtype=torch.int32), args.reps)
            views = torch.zeros(nt, device=dev, dtype=torch.int32)
            pixels = torch.zeros(nt, device=dev, dtype=torch.int64)
            t_fold, _ = timed(lambda: ops.visible_fold(pix, 1, views, pixels), args.reps)
            t_all = walled(lambda: ops.triangle_visibility(V, T, P, H, W, views_per_call=slab), max(3, args.reps // 3))
            vis = ops.triangle_visibility(V, T, P, H, W, views_per_call=slab)
            seen = (vis.views >= 1).to(torch.uint8)
            t_grow, kept = timed(lambda: ops.grow_triangles(T, nv, seen, args.grow), args.reps)
            t_select, out = timed(lambda: ops.select_triangles(V, T, kept, normals=N), args.reps)
            v2, t2 = out[0], out[1]
            covered = int((pix.sum(0) > 0).sum())
            print("    one slab of %d views:" % Ps.shape[0])
            print("      jt_raster_project + jt_raster_draw    %9.3f ms   (the z-buffer fill included)" % t_draw)
            print("      jt_visible_tally, one add per run     %9.3f ms   (the fill of pix included: %.3f ms)" % (t_runs, t_fill))
            print("      jt_visible_tally, one add per pixel   %9.3f ms   (likewise; %d triangles win a pixel in the slab)" % (t_plain, covered))
            print("      jt_visible_fold                       %9.3f ms" % t_fold)
            print("    all %d deciding views, ops.triangle_visibility, wall    %9.3f ms" % (P.shape[0], t_all))
            print("    grow, %d ring(s)                         %9.3f ms" % (args.grow, t_grow))
            print("    select_triangles                        %9.3f ms   (one host read)" % t_select)
            print("    seen %d, kept %d of %d triangles (%.1f %%), %d of %d vertices; atlas at S = 8: %s"
                  % (int(seen.sum()), t2.shape[0], nt, 100.0 * t2.shape[0] / nt, v2.shape[0], nv, atlas(t2.shape[0])))
            for kind in ("deciding", "other"):
                before, after = check(V, T, judges[kind]), check(v2, t2, judges[kind])
                print("    %-8s cameras %s: coverage_mesh %.5f -> %.5f, iou %.5f -> %.5f, depth_abs_median %.5f -> %.5f"
                      % (kind, judges[kind], before[0], after[0], before[1], after[1], before[2], after[2]))


if __name__ == "__main__":
    main()
