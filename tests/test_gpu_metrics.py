"""The evaluation stage on the GPU: ops.ssim (csrc/jt_metrics.hip) against the fp64 stock-op evaluation of its definition
(tests/ssim_ref.py), its reproducibility and graph safety, and Model.evaluate_full / Model.generate_videos_synthesis with the
files they leave behind (model/nerf.py:525-627, model/bat.py:240-263)."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden_util import Fixture
from tests.ssim_ref import parity_inputs, smooth_pairs, ssim_ref
from tests.test_gpu_eval import _model
from tests.test_lifecycle import _small_opt

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Per pixel: the map is the fp32 rounding of a value in [-1, 1] whose fp64 evaluation differs from the reference's only by the
# order of its sums: half an fp32 ulp of 1 plus that difference stays below 2^-23.  Per view: N * 2^-53 for the mean of N <=
# 1.92 M terms (about 2.1e-10) plus about 3e-12 from the moment sums after the division by C2: below 1e-9.
TOL_PIXEL, TOL_VIEW = 2.0 ** -23, 1e-9


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _to_bytes(img):
    """the stated pixel rule, written out: clamp to [0, 1], times 255, truncated.  [C, H, W] -> [H, W, C] uint8"""
    return torch.floor(img.detach().float().cpu().clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).numpy()


def test_ssim_parity():
    from joint_tensorf_amd import ops
    lo, hi = 1.0, 0.0
    for label, pred, target in parity_inputs():
        ref, ref_map = ssim_ref(pred, target)
        f32, f32_map = ssim_ref(pred, target, dtype=torch.float32)
        got, got_map = ops.ssim(pred.to(DEV), target.to(DEV), return_map=True)
        alone = ops.ssim(pred.to(DEV), target.to(DEV))
        assert got.dtype == torch.float64 and got.shape == (pred.shape[0],) and got.is_cuda
        assert got_map.dtype == torch.float32 and got_map.shape == pred.shape
        assert torch.equal(alone, got)                                    # the map is an extra output, not another path
        dv = (got.cpu() - ref).abs()
        dp = (got_map.cpu().double() - ref_map).abs().amax(dim=(1, 2, 3))
        dv32 = (f32.double() - ref).abs()
        dp32 = (f32_map.double() - ref_map).abs().amax(dim=(1, 2, 3))
        print("%-28s ssim %.6f..%.6f | kernel - fp64: view %.2e pixel %.2e | stock fp32 - fp64: view %.2e pixel %.2e"
              % (label, float(ref.min()), float(ref.max()), float(dv.max()), float(dp.max()), float(dv32.max()), float(dp32.max())))
        assert float(dp.max()) <= TOL_PIXEL, (label, float(dp.max()))
        assert float(dv.max()) <= TOL_VIEW, (label, float(dv.max()))
        # at least as close to fp64 as the stock fp32 formulation, on every view of every case
        assert bool((dp <= dp32).all()) and bool((dv <= dv32).all()), (label, dp, dp32, dv, dv32)
        if "noise" in label:
            lo, hi = min(lo, float(ref.min())), max(hi, float(ref.max()))
        elif label in ("identical", "all-zero"):
            assert torch.equal(got.cpu(), torch.ones_like(ref)) and torch.equal(ref, torch.ones_like(ref))
    assert lo <= 0.3 and hi >= 0.99, (lo, hi)            # the cases span bad to nearly perfect pictures


def test_ssim_is_reproducible_in_both_modes():
    from joint_tensorf_amd import ops
    from joint_tensorf_amd._lib import lib
    pred, target = (t.to(DEV) for t in smooth_pairs(3, 200, 200, 0.05, seed=5))
    out = {}
    prev = lib.jt_set_deterministic(0)
    try:
        for mode in (0, 1):
            lib.jt_set_deterministic(mode)
            a, am = ops.ssim(pred, target, return_map=True)
            b, bm = ops.ssim(pred, target, return_map=True)
            assert torch.equal(a, b) and torch.equal(am, bm), mode
            out[mode] = (a, am)
    finally:
        lib.jt_set_deterministic(prev)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])      # one summation order
    assert 0.3 < float(out[0][0].min()) < 0.99


def test_ssim_is_graph_safe():
    """no host synchronisation and no allocation outside the stream-ordered allocator: captured once, replayed on new contents of
    the same buffers (single stream, no parallel branches)"""
    from joint_tensorf_amd import ops
    p0, t0 = (t.to(DEV) for t in smooth_pairs(2, 96, 80, 0.05, seed=11))
    p1, t1 = (t.to(DEV) for t in smooth_pairs(2, 96, 80, 0.3, seed=12))
    pred, target = p0.clone(), t0.clone()
    ops.ssim(pred, target, return_map=True)             # (warm-up: module load outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, out_map = ops.ssim(pred, target, return_map=True)
    graph.replay()
    torch.cuda.synchronize()
    e0, e0_map = ops.ssim(p0, t0, return_map=True)
    assert torch.equal(out, e0) and torch.equal(out_map, e0_map)
    pred.copy_(p1)
    target.copy_(t1)
    graph.replay()
    torch.cuda.synchronize()
    e1, e1_map = ops.ssim(p1, t1, return_map=True)
    assert torch.equal(out, e1) and torch.equal(out_map, e1_map)
    assert not torch.equal(e0, e1)


def _eval_views(fx, n=2):
    from joint_tensorf_amd.options import Opt
    return [Opt(idx=torch.arange(1, device=DEV), pose=fx.t("in.test_pose", DEV), intr=fx.t("in.intr", DEV),
                intr_inv=fx.t("in.intr_inv", DEV), image=fx.t("in.test_image", DEV)) for _ in range(n)]


def test_evaluate_full_reports_ssim_and_writes_the_result_files(tmp_path):
    """the fixture and model of tests/test_gpu_eval.py::test_evaluate_full_runs_end_to_end"""
    pytest.importorskip("PIL")
    from joint_tensorf_amd._lib import lib
    fx = Fixture("blender_test_optim")
    opt, model = _model(fx)
    H, W = fx.meta["H"], fx.meta["W"]
    opt.output_path = str(tmp_path)
    views = _eval_views(fx)
    np.random.seed(0)
    res = model.evaluate_full(opt, views, fx.t("in.pose_gt", DEV))
    g = model.graph
    assert len(res.ssim_per_view) == len(res.psnr_per_view) == len(res.views) == 2
    for i, r in enumerate(res.views):
        want = float(ssim_ref(r.rgb_map, views[i].image)[0][0])
        print("view %d: ssim %.12f (fp64 reference %.12f), psnr %.6f" % (i, res.ssim_per_view[i], want, res.psnr_per_view[i]))
        assert abs(res.ssim_per_view[i] - want) <= 1e-9 and isinstance(r.ssim, float) and r.ssim == res.ssim_per_view[i]
        # PSNR exactly as before: the expression evaluate_view has always used
        assert res.psnr_per_view[i] == -10 * g.MSE_loss(r.rgb_map, r.var.image).log10().item()
        assert r.invdepth_map_normalized.shape == (1, 1, H, W)
    assert res.ssim == float(np.mean(res.ssim_per_view)) or abs(res.ssim - np.mean(res.ssim_per_view)) < 1e-15
    assert abs(res.psnr - np.mean(res.psnr_per_view)) < 1e-12
    # the files
    lines = open(os.path.join(str(tmp_path), "quant.txt")).read().splitlines()
    assert len(lines) == 2
    for i, ln in enumerate(lines):
        f = ln.split(" ")
        assert int(f[0]) == i and float(f[1]) == res.psnr_per_view[i] and float(f[2]) == res.ssim_per_view[i]
        assert math.isnan(float(f[3])) and len(f) == 4
    lines = open(os.path.join(str(tmp_path), "quant_pose.txt")).read().splitlines()
    assert len(lines) == res.R_error.shape[0] == 3
    for i, ln in enumerate(lines):
        f = ln.split(" ")
        assert int(f[0]) == i and float(f[1]) == res.R_error[i].item() and float(f[2]) == res.t_error[i].item()
    for i, r in enumerate(res.views):
        for name, src in (("rgb", r.rgb_map[0]), ("rgb_GT", views[i].image[0]), ("depth", r.invdepth_map_normalized[0])):
            a = _png(os.path.join(str(tmp_path), "test_view", "%s_%d.png" % (name, i)))
            assert a.shape[:2] == (H, W)
            np.testing.assert_array_equal(a.reshape(H, W, -1), _to_bytes(src), err_msg="%s_%d" % (name, i))
    # opt.optim.test_batch = 2: both views optimised in one batch; SSIM per view equals the serial evaluation's.  The two
    # trajectories are bit-identical where the gradient sums are order-independent (JT_DETERMINISTIC, as
    # test_batched_test_time_optim_reproduces_the_serial_trajectories runs them): the same poses, the same renders, the same SSIM
    prev = lib.jt_set_deterministic(1)
    try:
        opt.output_path = None
        np.random.seed(0)
        serial = model.evaluate_full(opt, _eval_views(fx), fx.t("in.pose_gt", DEV))
        opt.optim.test_batch = 2
        np.random.seed(0)
        batched = model.evaluate_full(opt, _eval_views(fx), fx.t("in.pose_gt", DEV))
    finally:
        lib.jt_set_deterministic(prev)
    print("serial", serial.ssim_per_view, "batched", batched.ssim_per_view, "default mode", res.ssim_per_view)
    assert batched.ssim_per_view == serial.ssim_per_view


def _trained_small_model(opt):
    from joint_tensorf_amd.model import bat_hip
    torch.manual_seed(0)
    np.random.seed(0)
    m = bat_hip.Model(opt)
    m.load_dataset(opt, eval_split="test", train_split="train")
    m.build_networks(opt)
    m.setup_optimizer(opt)
    m.train(opt)
    return m


def test_novel_views_are_rendered_and_written(tmp_path):
    pytest.importorskip("PIL")
    from joint_tensorf_amd import novel_views
    opt = _small_opt(device=DEV, output_path=str(tmp_path), max_iter=5, camera=dict(noise=0.15),
                     freq=dict(scalar=2, val=100, ckpt=100), optim=dict(test_iter=3))
    m = _trained_small_model(opt)
    g = m.graph
    assert m.generate_videos_synthesis(opt) is None
    novel = os.path.join(str(tmp_path), "novel_view")
    names = sorted(os.listdir(novel))
    assert len(names) == 240 and all(("rgb_%d.png" % i) in names and ("depth_%d.png" % i) in names for i in range(120))
    # frame 0: the sliced eval render at pose 0 of the path that tests/test_eval_outputs.py holds to the reference's generator
    with torch.no_grad():
        pose, pose_GT = m.get_all_training_poses(opt)
        _, sim3 = m.prealign_cameras(opt, pose, pose_GT)
        scale = sim3.s1 / sim3.s0
        assert abs(float(scale) - 1.0) > 1e-4                            # the noisy poses make the alignment non-trivial
        pose0 = novel_views.around_bbox(opt.data.scene_bbox, n=120, scale=scale)[0].to(DEV)
        first = m.test_loader[0]
        ret = g.render_by_slices(opt, pose0[None], intr_inv=first["intr_inv"][:1].to(DEV), intr=first["intr"][:1].to(DEV))
        rgb = ret.rgb.view(opt.H, opt.W, 3).permute(2, 0, 1)
        inv = (1 / (ret.depth / ret.opacity + 1e-10)).view(1, opt.H, opt.W)
    a = _png(os.path.join(novel, "rgb_0.png"))
    assert a.shape == (32, 32, 3)
    np.testing.assert_array_equal(a, _to_bytes(rgb))
    d = _png(os.path.join(novel, "depth_0.png"))
    assert d.shape == (32, 32)
    np.testing.assert_array_equal(d[:, :, None], _to_bytes(torch.nan_to_num(inv, nan=0.0)))
    assert a.std() > 0                                                  # a picture, not a constant
    # opt.eval_novel_views lowers the frame count
    opt.output_path = os.path.join(str(tmp_path), "few")
    opt.eval_novel_views = 6
    assert m.generate_videos_synthesis(opt) is None
    assert len(os.listdir(os.path.join(opt.output_path, "novel_view"))) == 12
    # without an output path: no file, no render
    before = sorted(os.listdir(str(tmp_path)))
    calls = []
    orig = g.render_by_slices

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    g.render_by_slices = spy
    try:
        opt.output_path = None
        assert m.generate_videos_synthesis(opt) is None
    finally:
        g.render_by_slices = orig
    assert calls == [] and sorted(os.listdir(str(tmp_path))) == before


def test_novel_views_of_an_llff_model(tmp_path):
    pytest.importorskip("PIL")
    opt = _small_opt("bat_llff_VM_MLP", device=DEV, output_path=str(tmp_path), max_iter=3,
                     data=dict(image_size=[30, 40], num_views=3, num_test_views=2, synthetic=True),
                     train_schedule=dict(n_voxel_init=2200, n_rays_init=90, n_rays_rest=90, upsample_iters=[10 ** 9]),
                     nerf=dict(n_rays=90), freq=dict(scalar=2, val=100, ckpt=100))
    m = _trained_small_model(opt)
    assert opt.camera.ndc and m.generate_videos_synthesis(opt) is None
    names = sorted(os.listdir(os.path.join(str(tmp_path), "novel_view")))
    assert len(names) == 120 and all(("rgb_%d.png" % i) in names and ("depth_%d.png" % i) in names for i in range(60))
    assert _png(os.path.join(str(tmp_path), "novel_view", "rgb_59.png")).shape == (30, 40, 3)
    assert _png(os.path.join(str(tmp_path), "novel_view", "depth_59.png")).shape == (30, 40)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_rank_evaluation_gathers_ssim(tmp_path):
    """gloo on one device, as tests/test_gpu_dist.py: every rank renders every second view; both return the complete per-view
    lists, equal to the single process's, and rank 0 alone writes quant.txt."""
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "eval_dist_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    r0 = torch.load(os.path.join(str(tmp_path), "eval_rank0.pt"))
    r1 = torch.load(os.path.join(str(tmp_path), "eval_rank1.pt"))
    assert (r0["n_own_views"], r1["n_own_views"]) == (2, 1)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import eval_dist_worker as W
    opt, model, views, pose_gt = W.build(os.path.join(str(tmp_path), "one_process"))
    np.random.seed(0)
    one = model.evaluate_full(opt, views, pose_gt)
    assert len(one.ssim_per_view) == 3 and all(0.0 < s < 1.0 for s in one.ssim_per_view)
    for r in (r0, r1):
        assert r["ssim_per_view"] == one.ssim_per_view and r["psnr_per_view"] == one.psnr_per_view
        assert r["ssim"] == one.ssim
    # written once, by rank 0 (the line count and the floats are the gathered ones; a second writer would have raced)
    assert outs[0].count("SSIM:") == 1 and outs[1].count("SSIM:") == 0
    two = os.path.join(str(tmp_path), "two_ranks")
    lines = open(os.path.join(two, "quant.txt")).read().splitlines()
    assert [float(ln.split(" ")[2]) for ln in lines] == one.ssim_per_view
    assert lines == open(os.path.join(str(tmp_path), "one_process", "quant.txt")).read().splitlines()
    assert sorted(os.listdir(os.path.join(two, "test_view"))) == sorted(
        "%s_%d.png" % (n, i) for n in ("rgb", "rgb_GT", "depth") for i in range(3))
