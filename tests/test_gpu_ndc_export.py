"""`python -m joint_tensorf_amd.export --frame.*` in process on a small bat_llff_VM_MLP model: the mesh of a forward-facing scene
carried from NDC to the frame of its cameras, previewed and checked there; and the export untouched without a `--frame.*` option."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES = [15, 14, 13]
REPORT_KEYS = ("coverage_mesh", "coverage_field", "iou", "depth_abs_median", "psnr_color", "disparity_abs_median")
STATUS = ("drawn", "near", "guard", "empty", "culled")
SURFACE = ["--surface.normals=true", "--surface.colors=true"]
PREVIEW = ["--preview.views=2", "--preview.size=[40,40]", "--preview.check=true"]
_CACHE = {}


def _export_args(tmp_path_factory):
    """a small forward-facing model trained for a few iterations, opaque blobs and a back wall that reaches the far face baked into its
    density (NDC fractions of the box), its checkpoint and the arguments that export it (built once for this module)"""
    if not _CACHE:
        from joint_tensorf_amd import synthetic
        from tests.test_gpu_metrics import _trained_small_model
        from tests.test_lifecycle import _small_opt
        root = str(tmp_path_factory.mktemp("ndc_export"))
        opt = _small_opt("bat_llff_VM_MLP", device=DEV, output_path=root, max_iter=3,
                         data=dict(image_size=[32, 32], num_views=3, num_test_views=2, synthetic=True),
                         train_schedule=dict(n_voxel_init=2200, n_rays_init=90, n_rays_rest=90, upsample_iters=[10 ** 9]),
                         nerf=dict(n_rays=90), freq=dict(scalar=2, val=100, ckpt=100))
        m = _trained_small_model(opt)
        with torch.no_grad():
            synthetic.bake_blobs(m.graph.nerf.tensorf, n_blobs=4, seed=2, z_range=(0.3, 0.6))
            synthetic.bake_wall(m.graph.nerf.tensorf, axis_frac=0.96)        # reaches the far face: a far cap, behind infinity
        ckpt = m.save_checkpoint(opt, ep=0, it=3, latest=True)
        _CACHE["root"] = root
        _CACHE["args"] = ["--yaml=bat_llff_VM_MLP", "--load=%s" % ckpt, "--device=%s" % DEV, "--mesh.res=%s" % json.dumps(RES),
                          "--data.image_size=[32,32]", "--train_schedule.n_voxel_init=2200", "--train_schedule.upsample_iters=[1000000000]",
                          "--data.synthetic=true", "--data.num_views=3", "--data.num_test_views=2"]
    return _CACHE["root"], _CACHE["args"]


def _restored_model(args, extra=()):
    """what export.main builds before it exports: (options, model) of the checkpoint"""
    from joint_tensorf_amd import export
    from joint_tensorf_amd.model import bat_hip
    opt = export.build_options(args + list(extra) + ["--output_path=unused"])
    m = bat_hip.Model(opt)
    m.load_dataset(opt, eval_split="test", train_split="train")
    m.build_networks(opt)
    m.restore_checkpoint(opt)
    return opt, m


def _own_world_mesh(args, max_depth=None):
    """extract_mesh's NDC mesh un-warped and compacted by the test: sx, sy from the data set's intrinsics, n from the options"""
    from joint_tensorf_amd import ops
    if ("own", max_depth) not in _CACHE:
        opt, m = _restored_model(args)
        with torch.no_grad():
            ndc = m.graph.nerf.tensorf.extract_mesh(res=RES, level=0.005, cap=True, normals=True, colors=True)
        intr = m.train_data.all.intr[0]
        sx, sy, near = float(intr[0, 0] / intr[0, 2]), float(intr[1, 1] / intr[1, 2]), float(opt.arch.ndc_near_plane)
        assert (sx, sy, near) == (float(np.float32(25.6) / np.float32(16)),) * 2 + (1.0,)
        world, wn, status = ops.ndc_to_world(ndc.vertices, sx, sy, near, normals=ndc.normals, max_depth=max_depth)
        _CACHE[("own", max_depth)] = (ndc, (sx, sy, near)) + tuple(ops.compact_mesh(world, ndc.triangles, status, normals=wn, colors=ndc.colors))
    return _CACHE[("own", max_depth)]


def _world_export(tmp_path_factory):
    from joint_tensorf_amd import export
    root, args = _export_args(tmp_path_factory)
    if "world" not in _CACHE:
        _CACHE["world"] = export.main(args + SURFACE + PREVIEW + ["--frame.space=world", "--output_path=%s" % os.path.join(root, "world")])
    return _CACHE["world"]


def test_world_export_with_preview_and_check(tmp_path_factory, capsys):
    from PIL import Image
    from joint_tensorf_amd import eval_io, mesh_io, ops
    root, args = _export_args(tmp_path_factory)
    out_dir = os.path.join(root, "world")
    fresh = "world" not in _CACHE
    out = _world_export(tmp_path_factory)
    assert not fresh or "preview of 2 views at 40 x 40" in capsys.readouterr().out
    assert sorted(os.listdir(out_dir)) == ["cameras.json", "mesh.ply", "preview", "report.json"]
    ply = mesh_io.read_ply_attributes(out.mesh)
    cams = mesh_io.read_cameras(out.cameras)
    ndc, (sx, sy, near), v, t, n, c, (n_beyond, n_far) = _own_world_mesh(args)
    assert "space world" in ply["comments"] and "space ndc" not in ply["comments"] and cams["space"] == "world"
    assert "unwarp near %r sx %r sy %r" % (near, sx, sy) in ply["comments"]
    assert "dropped beyond %d far %d" % (n_beyond, n_far) in ply["comments"] and n_beyond > 0 and n_far == 0
    assert out.unwarp.n_dropped_beyond == n_beyond and out.n_triangles == t.shape[0] == ndc.triangles.shape[0] - n_beyond > 0
    # bit for bit what the test's own un-warp and compaction give
    assert (ply["vertices"] == v.cpu().numpy()).all() and (ply["triangles"] == t.cpu().numpy()).all()
    assert (ply["normals"] == n.cpu().numpy()).all() and (ply["colors"] == mesh_io.quantise_colors(c)).all()
    assert np.isfinite(ply["vertices"]).all() and ply["vertices"][:, 2].min() > 0
    # the pictures: that mesh through the unchanged rasteriser under the cameras of cameras.json
    views = out.preview.views
    assert views == [0, 2]
    pose = torch.tensor([cams["views"][i]["pose"] for i in views], device=DEV)
    intr = torch.tensor([cams["views"][i]["intr"] for i in views], device=DEV)
    proj = mesh_io.projection_matrices(pose, intr, size=(40, 40), image_size=cams["image_size"])
    drawn = ops.rasterize(v, t, proj, 40, 40, attrs=c, background=0.0)
    report = json.load(open(out.preview.report))
    for j, i in enumerate(views):
        png = np.asarray(Image.open(os.path.join(out_dir, "preview", "mesh_%d.png" % i)))
        assert png.shape == (40, 40, 3) and (png == eval_io.to_uint8(drawn.attrs[j].permute(2, 0, 1)).numpy()).all()
        covered = drawn.tri[j] >= 0
        assert report["views"][j]["coverage_mesh"] == float(covered.float().mean()) > 0.2
        assert not png[~covered.cpu().numpy()].any()
        assert Image.open(os.path.join(out_dir, "preview", "field_%d.png" % i)).size == (40, 40)
    # the report: six keys, finite and in range; every triangle accounted for
    assert report["n_triangles"] == out.n_triangles and [r["idx"] for r in report["views"]] == views
    for row in report["views"] + [report["mean"]]:
        for k in REPORT_KEYS:
            assert k in row and isinstance(row[k], float) and math.isfinite(row[k]), (k, row)
        assert 0.0 <= row["iou"] <= 1.0 and 0.0 <= row["coverage_mesh"] <= 1.0 and 0.0 <= row["coverage_field"] <= 1.0
        assert row["depth_abs_median"] >= 0.0 and row["disparity_abs_median"] >= 0.0
        assert tuple(row["triangles"]) == STATUS and sum(row["triangles"].values()) == pytest.approx(out.n_triangles)
    for k in REPORT_KEYS:
        assert report["mean"][k] == pytest.approx(sum(r[k] for r in report["views"]) / 2)
    print("\n[ndc export] " + out.preview.summary)


def test_max_depth_drops_the_background(tmp_path_factory):
    from joint_tensorf_amd import export, mesh_io
    root, args = _export_args(tmp_path_factory)
    full = _own_world_mesh(args)
    limit = float(np.median(full[2][:, 2].cpu().numpy()))
    out = export.main(args + ["--frame.space=world", "--frame.max_depth=%r" % limit, "--output_path=%s" % os.path.join(root, "near")])
    v, t, comments = mesh_io.read_ply(out.mesh)
    _, _, v2, t2, _, _, (n_beyond, n_far) = _own_world_mesh(args, max_depth=limit)
    assert 0 < len(t) < full[3].shape[0] and n_far > 0 and "dropped beyond %d far %d" % (n_beyond, n_far) in comments
    assert (v == v2.cpu().numpy()).all() and (t == t2.cpu().numpy()).all() and v[:, 2].max() <= limit
    assert out.get("preview", None) is None and sorted(os.listdir(os.path.dirname(out.mesh))) == ["cameras.json", "mesh.ply"]


def test_without_a_frame_option_nothing_changes(tmp_path_factory, tmp_path):
    from joint_tensorf_amd import export, mesh_io
    root, args = _export_args(tmp_path_factory)
    plain_dir = os.path.join(root, "plain")
    plain = export.main(args + SURFACE + ["--output_path=%s" % plain_dir])
    comments = mesh_io.read_ply_attributes(plain.mesh)["comments"]
    assert "space ndc" in comments and not any(c.startswith(("unwarp", "dropped")) for c in comments)
    assert mesh_io.read_cameras(plain.cameras)["space"] == "ndc" and plain.get("unwarp", None) is None
    # Model.export_scene on options that have never heard of the group
    opt, m = _restored_model(args, SURFACE)
    del opt["frame"]
    direct = os.path.join(root, "direct")
    m.export_scene(opt, direct)
    named = export.main(args + SURFACE + ["--frame.space=ndc", "--output_path=%s" % os.path.join(root, "named")])
    for name in ("mesh.ply", "cameras.json"):
        want = open(os.path.join(plain_dir, name), "rb").read()
        assert open(os.path.join(direct, name), "rb").read() == want, name
        assert open(os.path.join(os.path.dirname(named.mesh), name), "rb").read() == want, name
    # the NDC mesh itself is still not previewed
    with pytest.raises(SystemExit) as e:
        export.main(args + ["--preview.views=2", "--output_path=%s" % tmp_path])
    assert "ndc" in str(e.value).lower() and "--frame.space=world" in str(e.value) and os.listdir(str(tmp_path)) == []
    with pytest.raises(ValueError):
        m.preview_scene(export.build_options(args + ["--preview.views=2", "--output_path=unused"]), str(tmp_path))
    assert os.listdir(str(tmp_path)) == []


def test_preview_scene_extracts_and_unwarps_by_itself(tmp_path_factory, tmp_path):
    """Model.preview_scene with mesh=None on a world-frame NDC scene: the pictures of the export's own preview"""
    root, args = _export_args(tmp_path_factory)
    world = _world_export(tmp_path_factory)
    opt, m = _restored_model(args, ["--preview.views=2", "--preview.size=[40,40]", "--frame.space=world"])
    out = m.preview_scene(opt, str(tmp_path))
    assert out.views == [0, 2] and out.report is None
    for i in out.views:
        a = open(os.path.join(str(tmp_path), "preview", "mesh_%d.png" % i), "rb").read()
        assert a == open(os.path.join(world.preview.directory, "mesh_%d.png" % i), "rb").read()


def test_world_on_a_world_scene_changes_nothing(tmp_path_factory):
    from joint_tensorf_amd import export
    from tests.test_gpu_preview import _export_args as blender_args
    root, args, data = blender_args(tmp_path_factory)
    a = export.main(args + data + SURFACE + ["--output_path=%s" % os.path.join(root, "frame_none")])
    b = export.main(args + data + SURFACE + ["--frame.space=world", "--output_path=%s" % os.path.join(root, "frame_world")])
    assert b.get("unwarp", None) is None
    for name in ("mesh.ply", "cameras.json"):
        assert open(os.path.join(os.path.dirname(a.mesh), name), "rb").read() == open(os.path.join(os.path.dirname(b.mesh), name), "rb").read()
