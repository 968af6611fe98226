"""The host side of the evaluation stage (no GPU): the novel-view camera paths against the reference's generators, the SSIM
reference the device kernel is held to, the writers of quant.txt / quant_pose.txt / the PNGs, and the two SSIM entry points of
the C ABI."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.ssim_ref import PARITY_CASES, parity_inputs, smooth_pairs, ssim_ref, taps_fp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# the tolerances of tests/test_gpu_metrics.py::test_ssim_parity (derived there)
TOL_PIXEL, TOL_VIEW = 2.0 ** -23, 1e-9


def test_novel_view_poses_equal_the_reference_generators():
    """joint_tensorf_amd.novel_views against tests/golden/novel_poses.npz (camera.py:368-402 recorded by tools/make_eval_golden.py):
    1e-6 absolute on fp32 entries of magnitude <= 4 produced by the same torch trigonometric calls."""
    from joint_tensorf_amd import novel_views
    from joint_tensorf_amd.options import load_options
    d = np.load(os.path.join(GOLDEN, "novel_poses.npz"))
    bbox = d["bbox.scene_bbox"].tolist()
    assert bbox == [float(v) for v in load_options("bat_blender_VM").data.scene_bbox]
    assert float(d["bbox.scale_b"]) != 1.0 and float(d["llff.scale_b"]) != 1.0
    anchor = torch.from_numpy(d["llff.anchor"])
    assert float((anchor[:, :3] - torch.eye(3)).abs().max()) > 0.1 and float(anchor[:, 3].abs().min()) > 0.1
    got = {
        "bbox.poses_1": novel_views.around_bbox(bbox, n=120, scale=1),
        "bbox.poses_b": novel_views.around_bbox(bbox, n=120, scale=torch.from_numpy(d["bbox.scale_b"])),
        "llff.poses_1": novel_views.around_pose(anchor, n=60, scale=1),
        "llff.poses_b": novel_views.around_pose(anchor, n=60, scale=torch.from_numpy(d["llff.scale_b"])),
    }
    for k, v in got.items():
        assert v.dtype == torch.float32 and tuple(v.shape) == d[k].shape == ((120 if k.startswith("bbox") else 60), 3, 4)
        assert np.abs(d[k]).max() <= 4.0
        err = np.abs(v.numpy() - d[k]).max()
        print("%s: max |ours - reference| = %.2e" % (k, err))
        assert err <= 1e-6, (k, err)
    # a lower frame count walks the same circle more coarsely: every n-th pose of the full path
    np.testing.assert_allclose(novel_views.around_bbox(bbox, n=12, scale=1).numpy(), d["bbox.poses_1"][::10], atol=1e-6)


def test_ssim_ref_window_and_sanity():
    g = taps_fp32()
    assert g.dtype == torch.float32 and g.shape == (11,) and abs(float(g.double().sum()) - 1.0) < 1e-6
    assert torch.equal(g, g.flip(0)) and abs(float(g[5]) - 0.26601171493530273) < 1e-12
    pred, target = smooth_pairs(2, 37, 53, 0.1, seed=7)
    one, one_map = ssim_ref(target, target.clone())
    assert one.dtype == torch.float64 and torch.equal(one, torch.ones(2, dtype=torch.float64))     # exactly 1.0
    assert torch.equal(one_map, torch.ones_like(one_map))
    a, am = ssim_ref(pred, target)
    b, bm = ssim_ref(target, pred)
    assert torch.equal(a, b) and torch.equal(am, bm)                                                # symmetric
    assert 0.3 < float(a.min()) and float(a.max()) < 0.99                                           # and not trivially 1


def test_the_border_rule_is_pinned_by_the_parity_tolerances():
    """On the input set of the GPU parity test, SSIM with replicate padding differs from the zero-padded definition by more than
    100 x that test's tolerances, per view and per pixel: a kernel with another border rule cannot pass it.  (Computed, not
    assumed.  The identical and the all-zero pair are 1 under any border rule and are left out.)"""
    n = 0
    for label, pred, target in parity_inputs():
        if label in ("identical", "all-zero"):
            continue
        if pred.shape[0] > 3:                       # the border effect of a view does not depend on how many views ride along
            pred, target = pred[:3], target[:3]
        z, zm = ssim_ref(pred, target)
        r, rm = ssim_ref(pred, target, padding="replicate")
        dv, dp = float((z - r).abs().min()), float((zm - rm).abs().amax(dim=(1, 2, 3)).min())
        print("%-28s replicate vs zero padding: per view >= %.2e, per pixel (max over the map) >= %.2e" % (label, dv, dp))
        assert dv > 100 * TOL_VIEW and dp > 100 * TOL_PIXEL, (label, dv, dp)
        n += 1
    assert n == len(PARITY_CASES) + 1


def test_quant_files_parse_back_to_the_same_floats(tmp_path):
    from joint_tensorf_amd import eval_io
    rng = np.random.default_rng(0)
    psnr = [float(v) for v in rng.uniform(5, 40, 7)] + [float(np.float32(31.4159))]
    ssim = [float(v) for v in rng.uniform(0, 1, 7)] + [1.0]
    err_R = [float(np.float32(v)) for v in rng.uniform(0, 0.1, 5)]
    err_t = [float(np.float32(v)) for v in rng.uniform(0, 0.5, 5)]
    eval_io.write_quant(str(tmp_path), psnr, ssim)
    eval_io.write_quant_pose(str(tmp_path), torch.tensor(err_R), torch.tensor(err_t))
    lines = open(os.path.join(str(tmp_path), "quant.txt")).read().splitlines()
    assert len(lines) == 8
    for i, ln in enumerate(lines):
        f = ln.split(" ")
        assert len(f) == 4 and int(f[0]) == i and float(f[1]) == psnr[i] and float(f[2]) == ssim[i]
        assert f[3] == "nan" and math.isnan(float(f[3]))
        assert ln == "{} {} {} {}".format(i, psnr[i], ssim[i], float("nan"))      # the reference's formatting of floats
    lines = open(os.path.join(str(tmp_path), "quant_pose.txt")).read().splitlines()
    assert len(lines) == 5
    for i, ln in enumerate(lines):
        f = ln.split(" ")
        assert len(f) == 3 and int(f[0]) == i and float(f[1]) == err_R[i] and float(f[2]) == err_t[i]


def test_view_pngs_hold_floor_of_clamped_times_255(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from joint_tensorf_amd import eval_io
    H, W = 13, 21
    gen = torch.Generator().manual_seed(3)
    rgb = torch.rand(3, H, W, generator=gen) * 1.4 - 0.2        # values on both sides of [0, 1]
    gt = torch.rand(3, H, W, generator=gen)
    depth = torch.rand(1, H, W, generator=gen) * 3.0            # inverse depths above 1: clamped, not wrapped
    rgb[0, 0, :4] = torch.tensor([0.0, 1.0, 0.5, 254.5 / 255])
    assert eval_io.write_view_pngs(os.path.join(str(tmp_path), "test_view"), 4, rgb=rgb, rgb_GT=gt, depth=depth)
    for name, src, mode in (("rgb", rgb, "RGB"), ("rgb_GT", gt, "RGB"), ("depth", depth, "L")):
        im = Image.open(os.path.join(str(tmp_path), "test_view", "%s_4.png" % name))
        assert im.size == (W, H) and im.mode == mode
        want = torch.floor(src.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).numpy()
        got = np.asarray(im).reshape(H, W, -1)
        np.testing.assert_array_equal(got, want, err_msg=name)
    assert float(depth.max()) > 1 and np.asarray(Image.open(os.path.join(str(tmp_path), "test_view", "depth_4.png"))).max() == 255
    # only what is handed over is written (the novel-view frames have no ground truth)
    eval_io.write_view_pngs(os.path.join(str(tmp_path), "novel_view"), 0, rgb=rgb, depth=depth)
    assert sorted(os.listdir(os.path.join(str(tmp_path), "novel_view"))) == ["depth_0.png", "rgb_0.png"]


def test_normalized_invdepth():
    from joint_tensorf_amd import eval_io
    from joint_tensorf_amd.options import Opt
    m = torch.tensor([[0.05, 1.0, 6.0]])
    plain = Opt(camera=dict(ndc=False))
    assert eval_io.normalized_invdepth(plain, m) is m
    ndc = Opt(camera=dict(ndc=True), nerf=dict(depth=dict(range=[1.0, 7.0])))
    np.testing.assert_allclose(eval_io.normalized_invdepth(ndc, m).numpy(), [[0.0, 0.95 / 5.95, 1.0]], rtol=1e-6)


def test_ssim_entry_points_agree_across_header_binding_and_library():
    from joint_tensorf_amd import _lib
    src = open(os.path.join(ROOT, "include", "jt_render.h")).read()
    assert _lib.header_version() == _lib.JT_ABI_VERSION == _lib.lib.jt_version() >= 1205
    protos = {"jt_ssim_forward": ("int", 11), "jt_ssim_workspace_bytes": ("size_t", 4)}
    for name, (ret, n_args) in protos.items():
        m = re.search(r"^(\w+)\s+%s\(([^;]*)\);" % name, src, flags=re.M)
        assert m, "%s is not declared in include/jt_render.h" % name
        assert m.group(1) == ret and len(m.group(2).split(",")) == n_args
        res, args = _lib.SIGNATURES[name]
        assert len(args) == n_args and res is (ctypes.c_int if ret == "int" else ctypes.c_size_t)
        assert hasattr(_lib.lib, name)
    assert "model/nerf.py:550" in src[src.index("SSIM of n_views"):src.index("int jt_ssim_forward")]
    # the workspace: one fp64 partial sum per 32 x 16 tile, channel and view
    ws = _lib.lib.jt_ssim_workspace_bytes
    assert ws(1, 3, 800, 800) == 25 * 50 * 3 * 8 and ws(32, 3, 200, 200) == 7 * 13 * 96 * 8 and ws(1, 1, 1, 1) == 8
    assert ws(0, 3, 8, 8) == 0 and ws(1, 3, 0, 8) == 0


def test_ssim_forward_refuses_bad_arguments_without_a_gpu():
    """null pointers, empty shapes and a short workspace come back as JT_ERR_ARG, 2^31 elements as JT_ERR_UNSUPPORTED, before
    anything touches a device (this test runs where there is none)."""
    from joint_tensorf_amd import _lib
    f = _lib.lib.jt_ssim_forward
    buf = (ctypes.c_double * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    JT_ERR_ARG, JT_ERR_UNSUPPORTED = 1, 2
    assert f(None, p, 1, 3, 8, 8, p, None, p, 8192, None) == JT_ERR_ARG
    assert f(p, None, 1, 3, 8, 8, p, None, p, 8192, None) == JT_ERR_ARG
    assert f(p, p, 1, 3, 8, 8, None, None, p, 8192, None) == JT_ERR_ARG
    assert f(p, p, 1, 3, 8, 8, p, None, None, 8192, None) == JT_ERR_ARG
    for shape in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8)):
        assert f(p, p, *shape, p, None, p, 8192, None) == JT_ERR_ARG, shape
    assert f(p, p, 1, 3, 8, 8, p, None, p, 3 * 8 - 1, None) == JT_ERR_ARG            # workspace one byte short
    assert f(p, p, 32, 3, 4800, 4800, p, None, p, 1 << 40, None) == JT_ERR_UNSUPPORTED   # 2.2e9 elements
