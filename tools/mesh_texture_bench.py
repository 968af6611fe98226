#!/usr/bin/env python3
"""Cost and effect of texturing an exported mesh on one GPU (TensorVMSplit.bake_texture; csrc/jt_texture.hip, and
jt_raster_resolve_texture in csrc/jt_raster.hip): the `bench.py --scene blobs` field (final 400^3 grid, twelve baked blobs) meshed
on a --res^3 lattice with its normals, as tools/mesh_simplify_bench.py has it, simplified in cells of K = 4, 8 lattice spacings,
then textured with blocks of S = 8, 16 texels.  Per (K, S) the stages of the bake are timed separately over the whole atlas --
jt_texture_texels; the shading (point_colors: the record-free appearance kernel, in slabs of 2^20 points); jt_texture_pack -- and
the textured resolve per --size x --size view beside the plain attribute resolve, with device events round a synchronised call,
one warm-up call, the median of --reps; then bake_texture as a whole by the wall clock.  The effect is reported the way
`--preview.check` scores colours: psnr_color over the pixels both cover, the mesh drawn from the eight cameras of the novel-view
turn round the scene box against the volume render of the same cameras -- once with the vertex colours of the simplified mesh,
once with its texture.  It reports; it judges nothing.
usage: python tools/mesh_texture_bench.py [--res 400] [--size 800] [--reps 9] [--cells 4,8] [--blocks 8,16]"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--level", type=float, default=0.005)
    ap.add_argument("--cells", default="4,8", help="cell edges K in lattice spacings")
    ap.add_argument("--blocks", default="8,16", help="block edges S in texels")
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
    n_views = 8
    with torch.no_grad():
        full = tf.extract_mesh(res=args.res, level=args.level, normals=True)
        print("mesh texturing, bench.py --scene blobs field (factor grid %s), lattice %s (capped), level %g: %d vertices, %d triangles "
              "before simplification" % (tf.gridSize.tolist(), list(full.shape), args.level, full.vertices.shape[0], full.triangles.shape[0]))
        # the field at the eight cameras, once
        pose = novel_views.around_bbox(opt.data.scene_bbox, n=n_views).to(dev)
        focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)          # the field of view of the Blender image sets
        intr = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], device=dev).repeat(n_views, 1, 1)
        proj = mesh_io.projection_matrices(pose, intr).contiguous()
        intr_inv = torch.linalg.inv(intr)
        model.graph.eval()
        opt.H, opt.W = H, W
        white = 1.0 if bool(opt.nerf.setbg_opaque) else 0.0
        field = []
        for j in range(n_views):
            ret = model.graph.render_by_slices(opt, pose[j:j + 1], intr_inv=intr_inv[j:j + 1], intr=intr[j:j + 1])
            field.append((ret.opacity.view(H, W).clone(), ret.rgb.view(H, W, 3).clone()))

        def psnr(drawn):
            """mean over the views of psnr_color as preview_scene's report has it: over pixels the mesh covers and the field
            renders with opacity >= 0.5"""
            vals = []
            for j, (opacity, rgb) in enumerate(field):
                both = (drawn.tri[j] >= 0) & (opacity >= 0.5)
                if int(both.sum()):
                    mse = ((drawn.attrs[j] - rgb)[both] ** 2).mean().clamp(min=1e-10)
                    vals.append(float(-10 * torch.log10(mse)))
            return sum(vals) / len(vals) if vals else float("nan")
        print("device events round each stage, one warm-up call, median of %d; ms.  psnr_color: %d views of %d x %d against the volume "
              "render, over pixels both cover" % (args.reps, n_views, H, W))
        for K in (float(k) for k in args.cells.split(",")):
            mesh = tf.extract_mesh(res=args.res, level=args.level, normals=True, colors=True, simplify=K)
            V, T, N = mesh.vertices, mesh.triangles, mesh.normals
            nv, nt = V.shape[0], T.shape[0]
            t_vertex_resolve, drawn = timed(lambda: ops.rasterize(V, T, proj, H, W, attrs=mesh.colors, background=white,
                                                                  views_per_call=n_views), args.reps)
            psnr_vertex = psnr(drawn)
            screen = ops.raster_project(V, proj)
            zbuf, _ = ops.raster_draw(screen, T, H, W)
            t_plain, _ = timed(lambda: ops.raster_resolve(zbuf, screen, T, mesh.colors, white), args.reps)
            print("  K = %g: %d vertices, %d triangles; vertex colours: psnr_color %.2f dB; jt_raster_resolve (3 attributes) %.3f ms per "
                  "view, ops.rasterize %.3f ms per view" % (K, nv, nt, psnr_vertex, t_plain / n_views, t_vertex_resolve / n_views))
            for S in (int(s) for s in args.blocks.split(",")):
                lay = ops.texture_layout(nt, S)
                t_texels, (xyz, dirs, valid) = timed(lambda: ops.texture_texels(V, T, N, lay), args.reps)
                t_shade, rgb = timed(lambda: tf.point_colors(xyz, dirs), max(3, args.reps // 3))
                atlas = torch.zeros(lay.height, lay.width, 3, device=dev, dtype=torch.uint8)
                t_pack, _ = timed(lambda: ops.texture_pack(rgb, valid, lay, atlas), args.reps)
                t_bake = walled(lambda: tf.bake_texture(V, T, N, block=S), max(3, args.reps // 3))
                tex = tf.bake_texture(V, T, N, block=S)
                assert torch.equal(tex.atlas, atlas)
                t_resolve, _ = timed(lambda: ops.raster_resolve_texture(zbuf, screen, T, tex.atlas, lay, white), args.reps)
                drawn = ops.rasterize(V, T, proj, H, W, texture=(tex.atlas, lay), background=white, views_per_call=n_views)
                print("    S = %d: atlas %d x %d (%d blocks in %d columns, %.1f MB, %d texels shaded)"
                      % (S, lay.width, lay.height, lay.n_blocks, lay.cols, 3e-6 * lay.width * lay.height, lay.n_entries))
                print("      jt_texture_texels                   %9.3f ms" % t_texels)
                print("      shading (point_colors, slabs)       %9.3f ms   %.1f M texels / s" % (t_shade, 1e-3 * lay.n_entries / t_shade))
                print("      jt_texture_pack                     %9.3f ms" % t_pack)
                print("      sum of the stages                   %9.3f ms   bake_texture, wall %9.3f ms" % (t_texels + t_shade + t_pack, t_bake))
                print("      jt_raster_resolve_texture           %9.3f ms per %d x %d view" % (t_resolve / n_views, H, W))
                print("      psnr_color                          %9.2f dB   (vertex colours %.2f dB)" % (psnr(drawn), psnr_vertex))


if __name__ == "__main__":
    main()
