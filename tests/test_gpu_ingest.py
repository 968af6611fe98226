"""The picture preprocessing of the dataset loaders on the GPU: ops.image_ingest (csrc/jt_ingest.hip) against the host path
(Pillow's LANCZOS resize, to_tensor, the composite in torch: datasets.preprocess_image_host) with torch.equal; the native
Blender loader on the device against the reference's fixture; reproducibility and graph safety; and the entry point
`python -m joint_tensorf_amd.train` end to end on a Blender-format directory written from rendered views."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dataset_scenes
from tests.test_datasets import SIZE_PAIRS, check_blender_against_fixture, pictures_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(img, H, W, bg):
    from joint_tensorf_amd.datasets import preprocess_image_host
    from joint_tensorf_amd.options import Opt
    return preprocess_image_host(Opt(data=dict(bgcolor=bg)), img, H, W)


@pytest.mark.parametrize("src,dst", SIZE_PAIRS + [((64, 48, 4), (64, 48)), ((64, 48, 3), (64, 48))],
                         ids=lambda v: "x".join(map(str, v)))
def test_image_ingest_equals_the_host_path(src, dst):
    """test 7: every size pair (both passes, one-axis cases, an enlargement, equal sizes, the Blender and the LLFF ratio, ratio 10),
    generator content and uniform random bytes, bgcolor 1, 0.5 and None"""
    from joint_tensorf_amd import ops
    (h, w, c), (H, W) = src, dst
    for kind, img in zip(("generator", "random"), pictures_for(h, w, c)):
        x = torch.from_numpy(img)[None].to(DEV)
        for bg in (1, 0.5, None):
            out = torch.full((1, 3, H, W), -7.0, device=DEV)
            assert ops.image_ingest(x, out, H, W, bg) is out
            want = host(img, H, W, bg)
            diff = (out[0].cpu() != want)
            print(src, dst, kind, "bgcolor", bg, "differing values:", int(diff.sum()), "of", diff.numel())
            assert torch.equal(out[0].cpu(), want), (kind, bg, int(diff.sum()))


def test_a_batch_lands_in_its_slots_and_nowhere_else():
    """800 x 800 x 4 -> 400 x 400, eight pictures written into the middle of a twelve-slot resident tensor"""
    from joint_tensorf_amd import ops
    imgs = np.stack([dataset_scenes.picture(800, 800, 4, view=k) for k in range(7)]
                    + [np.random.default_rng(5).integers(0, 256, (800, 800, 4), dtype=np.uint8)])
    resident = torch.full((12, 3, 400, 400), -7.0, device=DEV)
    ops.image_ingest(torch.from_numpy(imgs).to(DEV), resident[2:10], 400, 400, 1)
    got = resident.cpu()
    assert bool((got[:2] == -7.0).all()) and bool((got[10:] == -7.0).all())
    for k in range(8):
        assert torch.equal(got[2 + k], host(imgs[k], 400, 400, 1)), k


def test_bad_arguments_are_refused():
    from joint_tensorf_amd import _lib, ops
    lib = _lib.lib
    x = torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1, 3, 4, 4, device=DEV)
    tab = torch.zeros(16, 4, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1024, dtype=torch.int32, device=DEV)
    ok = lambda c, h=8, w=8, H=4, W=4, n=1: lib.jt_image_ingest(x.data_ptr(), n, h, w, c, tab.data_ptr(), 14, tab.data_ptr(), 14, H, W, 0,
                                                               0.0, out.data_ptr(), ws.data_ptr(), 4096, None)
    for c in (0, 1, 2, 5):
        assert ok(c) == 1 and lib.jt_image_ingest_workspace_bytes(1, 8, 8, c, 4, 4) == 0
    assert ok(4, h=0) == 1 and ok(4, w=0) == 1 and ok(4, H=0) == 1 and ok(4, W=0) == 1 and ok(4, n=0) == 1
    assert lib.jt_image_ingest(None, 1, 8, 8, 4, tab.data_ptr(), 14, tab.data_ptr(), 14, 4, 4, 0, 0.0, out.data_ptr(), ws.data_ptr(), 4096, None) == 1
    assert lib.jt_image_ingest(x.data_ptr(), 1, 8, 8, 4, None, 0, tab.data_ptr(), 14, 4, 4, 0, 0.0, out.data_ptr(), ws.data_ptr(), 4096, None) == 1
    assert lib.jt_image_ingest(x.data_ptr(), 1, 8, 8, 4, tab.data_ptr(), 14, tab.data_ptr(), 14, 4, 4, 0, 0.0, out.data_ptr(), ws.data_ptr(), 8, None) == 1
    assert lib.jt_image_ingest_workspace_bytes(3, 8, 8, 4, 4, 4) == 3 * 8 * 4 * 4 and lib.jt_image_ingest_workspace_bytes(3, 8, 8, 4, 4, 8) == 0
    with pytest.raises(ValueError):
        ops.image_ingest(x.float(), out, 4, 4)
    with pytest.raises(ValueError):
        ops.image_ingest(x, out[:, :, :, :2], 4, 2)
    with pytest.raises(_lib.JtError):
        ops.image_ingest(x.cpu(), out, 4, 4)


def test_native_blender_loader_on_the_device_equals_the_reference(tmp_path):
    """test 8: decode -> pinned buffer -> device -> ops.image_ingest fills `.all` with the tensors the reference collates"""
    check_blender_against_fixture(tmp_path, DEV)


def test_loader_batches_give_the_same_set(tmp_path, monkeypatch):
    """a set that does not fit one upload goes through several batches of the same staging buffers"""
    from joint_tensorf_amd import datasets
    from tests.test_datasets import blender_opt
    dataset_scenes.write_blender_set(tmp_path, splits={"train": 5}, size=96)
    whole = datasets.BlenderDataset(blender_opt(tmp_path, device=DEV, image_size=[40, 40]), split="train").all.image
    monkeypatch.setattr(datasets._FileDataset, "BATCH_BYTES", 2 * 96 * 96 * 4)
    parts = datasets.BlenderDataset(blender_opt(tmp_path, device=DEV, image_size=[40, 40]), split="train").all.image
    host_set = datasets.BlenderDataset(blender_opt(tmp_path, device="cpu", image_size=[40, 40]), split="train").all.image
    assert torch.equal(whole, parts) and torch.equal(whole.cpu(), host_set)


def test_same_answer_twice_and_from_a_replayed_graph():
    """test 9: the entry point is a pure launch sequence: run to run the same bits, and captured into a graph and replayed twice"""
    from joint_tensorf_amd import ops
    a = np.stack([dataset_scenes.picture(302, 403, 4, view=k) for k in range(3)])
    b = np.random.default_rng(9).integers(0, 256, a.shape, dtype=np.uint8)
    x = torch.from_numpy(a).to(DEV)
    out = torch.full((3, 3, 48, 64), -7.0, device=DEV)
    first = ops.image_ingest(x, out, 48, 64, 0.5).clone()        # (also the warm-up: code object, tables)
    second = ops.image_ingest(x, torch.empty_like(out), 48, 64, 0.5)
    assert torch.equal(first, second)
    assert torch.equal(first.cpu(), torch.stack([host(p, 48, 64, 0.5) for p in a]))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.image_ingest(x, out, 48, 64, 0.5)
    out.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    x.copy_(torch.from_numpy(b))
    graph.replay()
    torch.cuda.synchronize()
    want = torch.stack([host(p, 48, 64, 0.5) for p in b])
    assert torch.equal(out.cpu(), want) and not torch.equal(out, first)


# ---- test 10: end to end ---------------------------------------------------------------------------------------------------------

RAW, SIZE = 128, 64
SMALL_RUN = ["--yaml=bat_blender_VM", "--data.scene=blobs", "--data.image_size=[%d,%d]" % (SIZE, SIZE),
             "--train_schedule.n_voxel_init=1000", "--train_schedule.n_voxel_final=4096", "--train_schedule.n_rays_init=256",
             "--train_schedule.n_rays_rest=256", "--nerf.n_rays=256", "--optim.test_iter=3"]


def write_rendered_blender_set(root, n_train=5, n_test=2):
    """views of synthetic.make_gt_scene's field from the evaluation renderer at 128 x 128, quantised with eval_io.to_uint8, as a
    Blender-format directory: transforms_{train,val,test}.json + RGBA PNGs (already composited over white: alpha 255 everywhere).
    Returns {split: (uint8 [n, 128, 128, 4], meta)}."""
    from joint_tensorf_amd import eval_io
    from joint_tensorf_amd.options import make_options
    from joint_tensorf_amd.synthetic import make_rendered_views
    opt = make_options("bat_blender_VM", device=DEV, data=dict(image_size=[RAW, RAW], gt_res=64))
    f = 0.5 * RAW / math.tan(0.5 * 0.69)                                   # synthetic.make_views' focal length
    out, pics, metas = {}, {}, {}
    for split, n, seed in (("train", n_train, 0), ("val", n_test, 1000), ("test", n_test, 1000)):
        views = make_rendered_views(opt, n, seed=seed, device=DEV, scene_seed=0)
        rgb = torch.stack([eval_io.to_uint8(im) for im in views.image])                       # [n, 128, 128, 3]
        pics[split] = torch.cat([rgb, torch.full_like(rgb[..., :1], 255)], dim=-1).numpy()
        frames = []
        for i in range(n):
            # world-to-camera [R | t] (camera looking along +z) -> the camera-to-world matrix of a Blender file (looking along -z):
            # data/blender.py:86-91 inverts compose([diag(1, -1, -1), raw])
            R, t = views.pose[i, :, :3].double().cpu().numpy(), views.pose[i, :, 3].double().cpu().numpy()
            m = np.eye(4)
            m[:3, :3] = R.T @ np.diag([1.0, -1.0, -1.0])
            m[:3, 3] = -R.T @ t
            frames.append({"file_path": "./%s/r_%d" % (split, i), "transform_matrix": m.tolist()})
        metas[split] = {"camera_angle_x": 2 * math.atan(0.5 * RAW / f), "frames": frames}
        out[split] = (pics[split], metas[split])
    dataset_scenes.write_blender_set(root, scene="blobs", splits={"train": n_train, "val": n_test, "test": n_test}, pictures=pics)
    for split, meta in metas.items():       # (write_blender_set wrote its own cameras: replace them with the rendered views')
        with open(os.path.join(str(root), "blobs", "transforms_%s.json" % split), "w") as fh:
            json.dump(meta, fh)
    return out


def views_from(pictures, meta):
    """the `var` layout from the pictures and camera file of one split, the existing way: Pillow on the host for the pictures
    (datasets.preprocess_image_host), the loaders' camera conventions for the rest"""
    from joint_tensorf_amd import datasets
    n = len(pictures)
    image = torch.stack([host(p, SIZE, SIZE, 1) for p in pictures])
    pose = torch.stack([datasets.BlenderDataset.parse_raw_camera(torch.tensor(f["transform_matrix"], dtype=torch.float32))
                        for f in meta["frames"]])
    focal = 0.5 * RAW / np.tan(0.5 * meta["camera_angle_x"])
    intr = torch.tensor([[focal, 0, RAW / 2], [0, focal, RAW / 2], [0, 0, 1]]).float()
    intr[0] *= SIZE / RAW
    intr[1] *= SIZE / RAW
    return dict(idx=torch.arange(n), image=image, pose=pose, intr=intr[None].repeat(n, 1, 1),
                intr_inv=intr.inverse()[None].repeat(n, 1, 1))


def test_entry_point_trains_on_a_blender_directory(tmp_path):
    sets = write_rendered_blender_set(tmp_path / "sets")
    out = tmp_path / "out"
    # the schedule of bat_blender_VM divided by 4000: 10 iterations, the first upsampling at iteration 2, nothing else in reach
    cmd = [sys.executable, "-m", "joint_tensorf_amd.train"] + SMALL_RUN + [
        "--data.root=%s" % (tmp_path / "sets"), "--output_path=%s" % out, "--compress=4000",
        "--train_schedule.upsample_iters=[8000,200000]", "--train_schedule.update_alphamask_iters=[800000,1600000]"]
    run = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=420,
                         env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    text = run.stdout.decode(errors="replace")
    print(text[-6000:])
    assert run.returncode == 0
    assert "opt.data.dataset_class = joint_tensorf_amd.datasets.BlenderDataset" in text and "SYNTHETIC NOISE" not in text
    for name in ("quant.txt", "quant_pose.txt", "model.ckpt"):
        assert (out / name).exists(), name
    rows = [line.split() for line in (out / "quant.txt").read_text().splitlines()]
    assert len(rows) == 2 and all(math.isfinite(float(r[1])) for r in rows)        # one finite PSNR per test view
    assert len((out / "quant_pose.txt").read_text().splitlines()) == 5

    # ---- the files feed the engine the pictures they hold: same seed, same schedule, the views handed over as tensors ---------
    from joint_tensorf_amd import train
    from joint_tensorf_amd._lib import lib
    from joint_tensorf_amd.model import bat_hip
    argv = SMALL_RUN + ["--data.root=%s" % (tmp_path / "sets"), "--output_path=%s" % (tmp_path / "out_a"), "--max_iter=8",
                        "--train_schedule.upsample_iters=[2,50]", "--train_graph!"]
    prev = lib.jt_set_deterministic(1)
    try:
        a = train.main(argv)
        assert type(a.train_data).__name__ == "BlenderDataset" and a.it == 8
        opt = train.build_options(argv)
        opt.output_path = str(tmp_path / "out_b")
        os.makedirs(opt.output_path)
        opt.data.train_views = views_from(*sets["train"])
        opt.data.test_views = views_from(*sets["val"])
        torch.manual_seed(int(opt.seed))
        np.random.seed(int(opt.seed))
        b = bat_hip.Model(opt)
        b.load_dataset(opt, train_split="train")
        assert type(b.train_data).__name__ == "DictDataset"
        b.build_networks(opt)
        b.setup_optimizer(opt)
        b.restore_checkpoint(opt)
        b.setup_visualizer(opt)
        b.train(opt)
    finally:
        lib.jt_set_deterministic(prev)
    for key in ("image", "pose", "intr", "intr_inv", "idx"):
        assert torch.equal(a.train_data.all[key], b.train_data.all[key]), key
    sd_a, sd_b = a.graph.state_dict(), b.graph.state_dict()
    assert set(sd_a) == set(sd_b) and len(sd_a) > 10
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    assert float(a.graph.se3_refine.weight.abs().sum()) > 0
