#!/usr/bin/env python3
"""Cost and effect of exporting the surface fused from rendered depth maps on one GPU (mesh_ops.fusion_integrate / fusion_lattice /
mesh_from_fused_lattice, extract_mesh(fusion=); csrc/jt_fusion.hip): the `bench.py --scene blobs` field (final 400^3 grid, twelve
baked blobs) on a --res^3 lattice as the other mesh tools have it, seen from a turn of --views cameras round the scene box
(novel_views.around_bbox).  25 / 50 / 100 of them, evenly spaced, are rendered at 800 x 800 and at 400 x 400 (Model.fusion_depth)
and fused in slabs of eight views.

Timed with device events round a synchronised call, one warm-up call, the median of --reps: the depth render per view, the
integration per slab, the finish, the cell mask, the extraction with the cell rule.  The integration's achieved voxel-views per
second stand against its two floors: the bytes it must move (the state, read and written once per call, and the slab's depth and
opacity maps) over the HBM rate, and its vector instructions over the vector rate.  Then what `--preview.check` reports -- iou,
depth_abs_median, colour PSNR against the volume render, triangle counts -- for the level-set mesh and the fused mesh side by
side, each with and without the visible-surface stage over all fused cameras, from --judge cameras of the turn.  It reports; it
judges nothing.
usage: python tools/mesh_fusion_bench.py [--res 400] [--views 100] [--judge 8] [--reps 5] [--sizes 800,400] [--counts 25,50,100]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_RATE = 6.29e12              # bytes / s: the measured float4 copy rate of the part
VECTOR_RATE = 256 * 4 * 16 * 2.4e9      # fp32 vector instructions x lanes / s: 256 CUs, 4 SIMDs of 16 lanes, 2.4 GHz
# vector instructions of one (lattice point, view) pair on the longest path of k_fusion_integrate (in frame, a surface, inside the
# band), counted in the gfx950 assembly: 3 x 5 for the projection, 3 IEEE divisions of 11, 9 compares and selects, 13 of
# conversion and addressing, 5 for the distance, the clamp and the two sums
VECTOR_INSTRUCTIONS = 75
# what the resource-usage remarks of the compiler say of k_fusion_integrate and k_fusion_finish (hipcc --offload-arch=gfx950 -O3
# -Rpass-analysis=kernel-resource-usage): VGPRs, SGPRs, scratch bytes per lane, LDS bytes, waves per SIMD
RESOURCES = {"k_fusion_integrate": (27, 42, 0, 0, 8), "k_fusion_finish": (12, 15, 0, 0, 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--views", type=int, default=100, help="cameras of the turn")
    ap.add_argument("--judge", type=int, default=8, help="cameras the check is made from")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=float, default=0.005)
    ap.add_argument("--sizes", default="800,400")
    ap.add_argument("--counts", default="25,50,100")
    ap.add_argument("--trunc", type=float, default=4.0)
    args = ap.parse_args()
    sys.argv = [sys.argv[0]]
    import bench
    from mesh_simplify_bench import timed
    from joint_tensorf_amd import mesh_io, mesh_ops, novel_views, ops
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
    slab, res = 8, args.res
    n_points = res ** 3

    def spaced(n, k):
        k = min(k, n)
        return sorted(set(int(round(i * (n - 1) / max(k - 1, 1))) for i in range(k)))
    print("depth-map fusion, bench.py --scene blobs field (factor grid %s), lattice %d^3 (capped), trunc %g spacings; a turn of %d "
          "cameras, %s of them fused in slabs of %d; device events round each stage, one warm-up call, median of %d; ms"
          % (tf.gridSize.tolist(), res, args.trunc, args.views, args.counts, slab, args.reps))
    for name, (vgpr, sgpr, scratch, lds, waves) in RESOURCES.items():
        print("  %-20s %d VGPRs, %d SGPRs, scratch %d B / lane, LDS %d B, %d waves / SIMD" % (name, vgpr, sgpr, scratch, lds, waves))
    with torch.no_grad():
        model.graph.eval()
        pose = novel_views.around_bbox(opt.data.scene_bbox, n=args.views).to(dev)
        lo, hi = tf.aabb[0].tolist(), tf.aabb[1].tolist()
        trunc = args.trunc * sum((hi[a] - lo[a]) / (res - 1) for a in range(3)) / 3.0
        fused_by_size = {}
        for size in (int(s) for s in args.sizes.split(",")):
            H = W = size
            focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)          # the field of view of the Blender image sets
            intr = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], device=dev).repeat(args.views, 1, 1)
            intr_inv = torch.linalg.inv(intr)
            proj = mesh_io.projection_matrices(pose, intr).contiguous()
            model.fusion_depth(opt, pose[:1], intr[:1], intr_inv[:1], H, W)          # (warm-up)
            torch.cuda.synchronize()
            maps, ms = [], []
            for j in range(args.views):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                maps.append(model.fusion_depth(opt, pose[j:j + 1], intr[j:j + 1], intr_inv[j:j + 1], H, W))
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            depth, opacity = torch.stack([m[0] for m in maps]), torch.stack([m[1] for m in maps])
            del maps
            print("  %d x %d: depth render (render_by_slices + the depth undone) %.2f ms per view, median of %d views; %.1f ms for all"
                  % (H, W, float(np.median(ms)), args.views, sum(ms)))
            for count in (int(c) for c in args.counts.split(",")):
                idx = spaced(args.views, count)
                d, o, P = depth[idx].contiguous(), opacity[idx].contiguous(), proj[idx].contiguous()
                slabs = [(d[v:v + slab], o[v:v + slab], P[v:v + slab]) for v in range(0, len(idx), slab)]
                state = mesh_ops.fusion_state((res,) * 3, dev)
                per_slab = []
                for s in slabs:
                    if s[0].shape[0] == slab:
                        scratch_state = (state[0].clone(), state[1].clone())
                        per_slab.append(timed(lambda: mesh_ops.fusion_integrate(scratch_state, *s, lo, hi, trunc), args.reps)[0])
                    mesh_ops.fusion_integrate(state, *s, lo, hi, trunc)
                t_slab = float(np.median(per_slab))
                t_finish, (vol, seen) = timed(lambda: mesh_ops.fusion_lattice(state, 1), args.reps)
                t_cells, _ = timed(lambda: mesh_ops.fused_cells(seen), args.reps)
                cap_vol, cap_lo, cap_hi = mesh_ops.cap_lattice(vol, lo, hi)
                cap_seen = torch.nn.functional.pad(seen, (1,) * 6, value=1)
                t_extract, (v, t, n_tris) = timed(lambda: mesh_ops.mesh_from_fused_lattice(cap_vol, cap_seen, 0.5, cap_lo, cap_hi), args.reps)
                t_plain, _ = timed(lambda: mesh_ops.mesh_from_lattice(cap_vol, 0.5, cap_lo, cap_hi), args.reps)
                pairs = n_points * slab
                bytes_moved = n_points * 16 + slab * H * W * 8
                floor_hbm, floor_vec = bytes_moved / HBM_RATE * 1e3, pairs * VECTOR_INSTRUCTIONS / VECTOR_RATE * 1e3
                print("    %3d views: integrate %.3f ms per slab of %d (min %.3f, max %.3f over %d slabs) = %.1f G voxel-views / s"
                      % (len(idx), t_slab, slab, min(per_slab), max(per_slab), len(per_slab), pairs / t_slab * 1e-6))
                print("               floors per slab: %.3f ms for %.0f MB over HBM at %.2f TB/s, %.3f ms for %d vector instructions per pair "
                      "at %.1f T / s (every pair on the longest path): the %s floor is the higher one, the kernel reaches %.0f %% of it"
                      % (floor_hbm, bytes_moved * 1e-6, HBM_RATE * 1e-12, floor_vec, VECTOR_INSTRUCTIONS, VECTOR_RATE * 1e-12,
                         "vector" if floor_vec > floor_hbm else "HBM", 100 * max(floor_hbm, floor_vec) / t_slab))
                print("               finish %.3f ms, cell mask %.3f ms, extraction with the cell rule %.3f ms (without: %.3f ms); "
                      "%d points seen of %d, %d triangles emitted, %d unobserved"
                      % (t_finish, t_cells, t_extract, t_plain, int(seen.sum()), n_points, n_tris[0], n_tris[1]))
                if count == max(int(c) for c in args.counts.split(",")):
                    fused_by_size[size] = dict(depth=d, opacity=o, proj=P, H=H, W=W, trunc=args.trunc)
                del state, vol, seen, cap_vol, cap_seen
            del depth, opacity
        # ---- the preview report, level set and fused side by side ----
        size = max(fused_by_size)
        fusion = fused_by_size[size]
        H = W = size
        focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)
        intr = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], device=dev).repeat(args.views, 1, 1)
        intr_inv = torch.linalg.inv(intr)
        proj = mesh_io.projection_matrices(pose, intr).contiguous()
        judges = [j + 1 for j in spaced(args.views - 1, args.judge)]                  # (off the fused cameras where not all are fused)
        field = {}
        opt.H, opt.W = H, W
        for j in judges:
            ret = model.graph.render_by_slices(opt, pose[j:j + 1], intr_inv=intr_inv[j:j + 1], intr=intr[j:j + 1])
            field[j] = (ret.opacity.view(H, W).clone(), (ret.depth.view(H, W) + float(tf.near_far[0]) - 0.05).clone(),
                        ret.rgb.view(H, W, 3).clone())
        white = 1.0 if bool(opt.nerf.setbg_opaque) else 0.0

        def check(mesh):
            drawn = ops.rasterize(mesh.vertices, mesh.triangles, proj[judges].contiguous(), H, W, attrs=mesh.colors, background=white,
                                  views_per_call=slab)
            iou, dep, psnr = [], [], []
            for k, j in enumerate(judges):
                opacity, depth_f, rgb = field[j]
                m, f = drawn.tri[k] >= 0, opacity >= 0.5
                union, solid, both = (m | f).sum(), m & (opacity >= 0.99), m & f
                iou.append(float((m & f).sum() / union) if int(union) else 1.0)
                if int(solid.sum()):
                    dep.append(float((drawn.depth[k] - depth_f)[solid].abs().median()))
                if int(both.sum()):
                    psnr.append(float(-10 * torch.log10(((drawn.attrs[k] - rgb)[both] ** 2).mean().clamp(min=1e-10))))
            mean = lambda x: sum(x) / len(x) if x else float("nan")                   # noqa: E731
            return mean(iou), mean(dep), mean(psnr)
        print("  preview check from %d cameras of the turn at %d x %d (means): iou, depth_abs_median, colour PSNR against the volume "
              "render" % (len(judges), H, W))
        visible = dict(proj=fusion["proj"], H=H, W=W)
        for label, kw in (("level set %g" % args.level, dict(level=args.level)), ("fused, %d views" % fusion["proj"].shape[0], dict(fusion=fusion))):
            for vis in (False, True):
                mesh = tf.extract_mesh(res=res, normals=True, colors=True, **kw, **({"visible": visible} if vis else {}))
                iou, dep, psnr = check(mesh)
                print("    %-22s %-22s %9d vertices %9d triangles  iou %.5f  depth_abs_median %.5f  psnr_color %.2f dB%s"
                      % (label, "--visible.views=all" if vis else "", mesh.vertices.shape[0], mesh.triangles.shape[0], iou, dep, psnr,
                         "" if mesh.fused is None else "  (seen %d, unobserved %d)" % (mesh.fused[7], mesh.fused[9])))
                del mesh


if __name__ == "__main__":
    main()
