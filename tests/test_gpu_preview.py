"""`python -m joint_tensorf_amd.export --preview.*` in process on a small trained model: the pictures of the mesh from its training
cameras (Model.preview_scene -> ops.rasterize), the check against the volume render (report.json), and the export itself
untouched by any of it."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES = [15, 14, 13]
REPORT_KEYS = ("coverage_mesh", "coverage_field", "iou", "depth_abs_median", "psnr_color")
STATUS = ("drawn", "near", "guard", "empty", "culled")
_CACHE = {}


def _export_args(tmp_path_factory):
    """the scene of tests/test_gpu_mesh.py::test_export_end_to_end: a small model trained for a few iterations, opaque blobs baked
    into its density, its checkpoint and the arguments that export it (built once for this module)"""
    if not _CACHE:
        from joint_tensorf_amd import synthetic
        from tests.test_gpu_metrics import _trained_small_model
        from tests.test_lifecycle import _small_opt
        root = str(tmp_path_factory.mktemp("preview"))
        opt = _small_opt(device=DEV, output_path=root, max_iter=5, camera=dict(noise=0.15),
                         freq=dict(scalar=2, val=100, ckpt=100), optim=dict(test_iter=3))
        m = _trained_small_model(opt)
        with torch.no_grad():
            synthetic.bake_blobs(m.graph.nerf.tensorf, n_blobs=5, seed=2)
        ckpt = m.save_checkpoint(opt, ep=0, it=5, latest=True)
        _CACHE["root"] = root
        _CACHE["args"] = ["--yaml=bat_blender_VM", "--load=%s" % ckpt, "--device=%s" % DEV, "--mesh.res=%s" % json.dumps(RES),
                          "--data.image_size=[32,32]", "--train_schedule.n_voxel_init=1000", "--train_schedule.n_voxel_final=4096",
                          "--train_schedule.upsample_iters=[2,50]", "--camera.noise=0.15"]
        _CACHE["data"] = ["--data.synthetic=true", "--data.num_views=3", "--data.num_test_views=2"]
    return _CACHE["root"], _CACHE["args"], _CACHE["data"]


def test_preview_with_check(tmp_path_factory, capsys):
    from joint_tensorf_amd import export
    root, args, data = _export_args(tmp_path_factory)
    out_dir = os.path.join(root, "with_preview")
    out = export.main(args + data + ["--output_path=%s" % out_dir, "--preview.views=2", "--preview.size=[40,40]",
                                     "--preview.check=true"])
    assert "preview of 2 views at 40 x 40" in capsys.readouterr().out
    views = out.preview.views
    assert views == [0, 2] and out.preview.report == os.path.join(out_dir, "report.json")     # evenly spaced over the three
    from PIL import Image
    for i in views:
        for kind in ("mesh", "field"):
            img = Image.open(os.path.join(out_dir, "preview", "%s_%d.png" % (kind, i)))
            assert img.size == (40, 40) and img.mode == "RGB"
    assert sorted(os.listdir(os.path.join(out_dir, "preview"))) == sorted("%s_%d.png" % (k, i) for k in ("mesh", "field") for i in views)
    assert sorted(os.listdir(out_dir)) == ["cameras.json", "mesh.ply", "preview", "report.json"]
    report = json.load(open(out.preview.report))
    assert report["size"] == [40, 40] and report["shade"] == "color" and report["n_triangles"] == out.n_triangles > 0
    assert [r["idx"] for r in report["views"]] == views
    for row in report["views"] + [report["mean"]]:
        for k in REPORT_KEYS:
            assert k in row and isinstance(row[k], float) and math.isfinite(row[k]), (k, row)
        assert 0.0 <= row["iou"] <= 1.0 and 0.0 <= row["coverage_mesh"] <= 1.0 and 0.0 <= row["coverage_field"] <= 1.0
        assert row["depth_abs_median"] >= 0.0
        assert tuple(row["triangles"]) == STATUS
        assert sum(row["triangles"].values()) == pytest.approx(out.n_triangles)              # drawn and dropped: every one
    for row in report["views"]:
        assert all(isinstance(v, int) for v in row["triangles"].values()) and row["triangles"]["culled"] == 0
    for k in REPORT_KEYS:
        assert report["mean"][k] == pytest.approx(sum(r[k] for r in report["views"]) / 2)
    print("\n[preview] " + out.preview.summary)
    _CACHE["with_preview"] = out_dir


def test_export_is_untouched_by_the_preview(tmp_path_factory):
    """without a --preview.* option: the same mesh.ply and cameras.json, byte for byte, and no preview directory"""
    from joint_tensorf_amd import export
    root, args, data = _export_args(tmp_path_factory)
    with_dir = _CACHE.get("with_preview")
    if with_dir is None:
        with_dir = os.path.join(root, "with_preview_again")
        export.main(args + data + ["--output_path=%s" % with_dir, "--preview.views=2", "--preview.size=[40,40]", "--preview.check=true"])
    plain_dir = os.path.join(root, "plain")
    plain = export.main(args + data + ["--output_path=%s" % plain_dir])
    assert sorted(os.listdir(plain_dir)) == ["cameras.json", "mesh.ply"] and plain.get("preview", None) is None
    for name in ("mesh.ply", "cameras.json"):
        assert open(os.path.join(plain_dir, name), "rb").read() == open(os.path.join(with_dir, name), "rb").read(), name


def test_other_shades_cull_and_all_views(tmp_path_factory):
    from joint_tensorf_amd import export
    from PIL import Image
    root, args, data = _export_args(tmp_path_factory)
    out_dir = os.path.join(root, "normals")
    out = export.main(args + data + ["--output_path=%s" % out_dir, "--preview.views=all", "--preview.shade=normal", "--preview.cull=true"])
    assert out.preview.views == [0, 1, 2] and out.preview.report is None
    assert sorted(os.listdir(os.path.join(out_dir, "preview"))) == ["mesh_0.png", "mesh_1.png", "mesh_2.png"]
    assert Image.open(os.path.join(out_dir, "preview", "mesh_1.png")).size == (32, 32)          # the image set's size
    out_dir = os.path.join(root, "depth")
    out = export.main(args + data + ["--output_path=%s" % out_dir, "--preview.views=1", "--preview.shade=depth", "--preview.check=true"])
    assert out.preview.views == [0] and Image.open(os.path.join(out_dir, "preview", "mesh_0.png")).mode == "L"
    report = json.load(open(out.preview.report))
    assert report["views"][0]["psnr_color"] is None and report["mean"]["psnr_color"] is None      # no colours were drawn


def test_preview_refusals(tmp_path_factory, tmp_path):
    """no image set: no cameras.json, nothing to look from; an NDC scene: not drawn yet.  Both before any GPU work."""
    from joint_tensorf_amd import export
    root, args, data = _export_args(tmp_path_factory)
    with pytest.raises(SystemExit) as e:
        export.main(args + ["--output_path=%s" % tmp_path, "--preview.views=2"])
    assert "image set" in str(e.value) and "cameras.json" in str(e.value)
    with pytest.raises(SystemExit) as e:
        export.main(["--yaml=bat_llff_VM_MLP", "--load=%s" % args[1].split("=", 1)[1], "--device=%s" % DEV, "--data.synthetic=true",
                     "--output_path=%s" % tmp_path, "--preview.views=2"])
    assert "ndc" in str(e.value).lower()
    assert os.listdir(str(tmp_path)) == []
