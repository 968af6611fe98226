"""The native dataset loaders (joint_tensorf_amd/datasets.py) without a GPU: the host path against what the reference's
loaders made of the same closed-form image sets (tests/golden/dataset_blender.npz, dataset_llff_cameras.npz, recorded by
tools/make_dataset_golden.py), the host coefficient tables of the device kernel against Pillow, data.load's precedence, the
command-line override parser and the guards."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import dataset_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# (h, w, c) -> (H, W): the size pairs the ingest arithmetic is pinned at (tests/test_gpu_ingest.py runs the kernel on the same list)
SIZE_PAIRS = [((800, 800, 4), (400, 400)), ((800, 800, 3), (400, 400)), ((302, 403, 3), (48, 64)), ((302, 403, 4), (48, 64)),
              ((97, 131, 4), (200, 150)), ((378, 504, 3), (60, 80)), ((120, 200, 4), (60, 200)), ((120, 200, 4), (120, 100)),
              ((50, 70, 3), (7, 9)), ((33, 21, 4), (1, 1)), ((800, 800, 4), (80, 80)), ((128, 128, 4), (64, 64)),
              ((3024, 4032, 3), (480, 640))]


def blender_opt(root, device="cpu", **data):
    from joint_tensorf_amd.options import make_options
    d = dict(root=str(root), scene="shapes", image_size=[80, 80], bgcolor=1)
    d.update(data)
    return make_options("bat_blender_VM", device=device, data=d)


def llff_opt(root, device="cpu", **data):
    from joint_tensorf_amd.options import make_options
    d = dict(root=str(root), scene="arc", image_size=[480, 640])
    d.update(data)
    return make_options("bat_llff_VM_MLP", device=device, data=d)


def check_blender_against_fixture(root, device):
    """test 1 / test 8: every split of the native loader equals the reference's collated tensors"""
    from joint_tensorf_amd import datasets
    fx = np.load(os.path.join(GOLDEN, "dataset_blender.npz"))
    metas = dataset_scenes.write_blender_set(root)
    for split, subset, n in (("train", None, 3), ("val", 2, 2), ("test", None, 2)):
        # the camera files the generator writes are the ones the fixture was recorded from
        assert metas[split]["camera_angle_x"] == float(fx[split + ".camera_angle_x"])
        assert np.array_equal(np.array([f["transform_matrix"] for f in metas[split]["frames"]]), fx[split + ".transform_matrix"])
        opt = blender_opt(root, device=device)
        ds = datasets.BlenderDataset(opt, split=split, subset=subset)
        assert len(ds) == n and ds.all.image.device.type == torch.device(device).type
        assert (ds.raw_H, ds.raw_W) == (800, 800)
        for key in ("image", "idx", "pose", "intr", "intr_inv"):
            got, want = ds.all[key].cpu(), torch.from_numpy(fx["%s.%s" % (split, key)])
            assert got.dtype == want.dtype and got.shape == want.shape, (split, key, got.dtype, got.shape)
            print(split, key, "max abs difference", float((got.double() - want.double()).abs().max()))
            assert torch.equal(got, want), (split, key)
        assert torch.equal(ds.get_all_camera_poses(opt), ds.all.pose)
        batch = ds.setup_loader(opt)[1]
        assert batch["image"].shape == (1, 3, 80, 80) and int(batch["idx"][0]) == 1


def test_blender_loader_equals_the_reference(tmp_path):
    check_blender_against_fixture(tmp_path, "cpu")


def test_blender_held_out_subsets_and_size_check(tmp_path):
    """subset=None on the held-out splits applies the reference yaml's val_sub 10 / test_sub 200; the raw size comes from the
    files (another size than 800 gives the intrinsics of THAT size), and a file of another size than the first is an error"""
    from joint_tensorf_amd import datasets
    dataset_scenes.write_blender_set(tmp_path, splits={"train": 2, "val": 12}, size=40, channels=4)
    opt = blender_opt(tmp_path, image_size=[20, 20])
    assert datasets.BLENDER_HELD_OUT_SUBSET == {"val": 10, "test": 200}
    assert len(datasets.BlenderDataset(opt, split="val")) == 10 and len(datasets.BlenderDataset(opt, split="val", subset=11)) == 11
    tr = datasets.BlenderDataset(opt, split="train")
    assert len(tr) == 2 and (tr.raw_H, tr.raw_W) == (40, 40)
    focal = 0.5 * 40 / np.tan(0.5 * tr.meta["camera_angle_x"]) * 0.5
    np.testing.assert_allclose(tr.all.intr[0].numpy(), [[focal, 0, 10], [0, focal, 10], [0, 0, 1]], rtol=1e-6)
    from PIL import Image
    Image.fromarray(dataset_scenes.picture(40, 44, 4)).save(str(tmp_path / "shapes" / "train" / "r_1.png"))
    with pytest.raises(ValueError, match="40 x 44"):
        datasets.BlenderDataset(opt, split="train")
    with pytest.raises(FileNotFoundError):
        datasets.BlenderDataset(blender_opt(tmp_path, scene="nowhere"), split="train")


def test_llff_cameras_equal_the_reference(tmp_path):
    """test 2: cameras, split sizes, the zero-split error at 9 views, the size-mismatch error"""
    from joint_tensorf_amd import datasets
    fx = np.load(os.path.join(GOLDEN, "dataset_llff_cameras.npz"))
    pb = dataset_scenes.write_llff_set(tmp_path, flat=True)
    assert np.array_equal(pb, fx["poses_bounds"])
    for split, n in (("train", 11), ("val", 1)):
        opt = llff_opt(tmp_path)
        ds = datasets.LLFFDataset(opt, split=split)
        assert len(ds) == n and ds.all.image.shape == (n, 3, 480, 640) and (ds.raw_H, ds.raw_W) == (3024, 4032)
        for key in ("pose", "intr", "intr_inv"):
            got, want = ds.all[key], torch.from_numpy(fx["%s.%s" % (split, key)])
            assert got.dtype == want.dtype and got.shape == want.shape
            print(split, key, "max abs difference", float((got.double() - want.double()).abs().max()))
            assert torch.equal(got, want), (split, key)
        assert torch.equal(ds.get_all_camera_poses(opt), torch.from_numpy(fx[split + ".all_camera_poses"]))
        assert torch.equal(ds.all.idx, torch.arange(n))
        # a flat picture of value v stays flat: v / 255
        first = 0 if split == "train" else 11
        assert torch.equal(ds.all.image[0], torch.full((3, 480, 640), 16 * first % 256, dtype=torch.float32).div(255))
    assert len(datasets.LLFFDataset(llff_opt(tmp_path), split="test")) == 1          # val and test are the same split
    assert len(datasets.LLFFDataset(llff_opt(tmp_path), split="train", subset=4)) == 4


def test_llff_zero_split_and_size_mismatch_are_errors(tmp_path):
    from joint_tensorf_amd import datasets
    small = dataset_scenes.llff_poses_bounds(n=9, h=30, w=40)
    dataset_scenes.write_llff_set(tmp_path, scene="nine", poses_bounds=small)
    with pytest.raises(ValueError, match="no held-out view"):        # int(9 * 0.1) = 0: the reference's train split would be empty
        datasets.LLFFDataset(llff_opt(tmp_path, scene="nine", image_size=[15, 20]), split="train")
    ds = datasets.LLFFDataset(llff_opt(tmp_path, scene="nine", image_size=[15, 20], val_ratio=0.25), split="train")
    assert len(ds) == 7 and ds.all.image.shape == (7, 3, 15, 20)
    dataset_scenes.write_llff_set(tmp_path, scene="wrong", poses_bounds=dataset_scenes.llff_poses_bounds(n=10, h=30, w=40), size=(30, 44))
    with pytest.raises(ValueError, match=r"30 x 44, poses_bounds.npy states 30 x 40"):
        datasets.LLFFDataset(llff_opt(tmp_path, scene="wrong", image_size=[15, 20]), split="train")
    dataset_scenes.write_llff_set(tmp_path, scene="short", poses_bounds=dataset_scenes.llff_poses_bounds(n=10, h=30, w=40), n_files=8)
    with pytest.raises(ValueError, match="8 files"):
        datasets.LLFFDataset(llff_opt(tmp_path, scene="short", image_size=[15, 20]), split="train")


# ---- test 3: the tables the kernel reads, through a numpy evaluation of its arithmetic, against Pillow ---------------------------

def ingest_numpy(img, H, W):
    """csrc/jt_ingest.hip's integer arithmetic in numpy, from the tables jt_image_ingest is handed: uint8 [h, w, c] -> uint8 [H, W, c]"""
    from joint_tensorf_amd.datasets import PRECISION_BITS, resample_table

    def one_pass(x, n_out, axis):
        x = np.moveaxis(x, axis, 0).astype(np.int32)
        tab, taps = resample_table(x.shape[0], n_out)
        assert tab.dtype == np.int32 and tab.shape == (2 + taps, n_out)
        out = np.empty((n_out,) + x.shape[1:], np.int32)
        for o in range(n_out):
            first, n = int(tab[0, o]), int(tab[1, o])
            assert 0 <= first and 1 <= n <= taps and first + n <= x.shape[0]
            acc = np.tensordot(tab[2:2 + n, o], x[first:first + n], axes=(0, 0)).astype(np.int32) + np.int32(1 << (PRECISION_BITS - 1))
            out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
        return np.moveaxis(out.astype(np.uint8), 0, axis)

    h, w, c = img.shape
    if (h, w) == (H, W):
        return img
    x = img
    if c == 4:
        a = x[..., 3:4].astype(np.int32)
        t = x[..., :3].astype(np.int32) * a + 128
        x = np.concatenate([((t >> 8) + t) >> 8, a], -1).astype(np.uint8)
    if w != W:
        x = one_pass(x, W, 1)
    if h != H:
        x = one_pass(x, H, 0)
    if c == 4:
        a, col = x[..., 3:4].astype(np.int32), x[..., :3].astype(np.int32)
        un = np.where((a == 255) | (a == 0), col, np.minimum(255, 255 * col // np.maximum(a, 1)))
        x = np.concatenate([un, a], -1).astype(np.uint8)
    return x


def pictures_for(h, w, c):
    """the generator's picture and one of uniform random bytes"""
    rnd = np.random.default_rng(h * 7 + w * 3 + c).integers(0, 256, (h, w, c), dtype=np.uint8)
    return [dataset_scenes.picture(h, w, c, view=1), rnd]


@pytest.mark.parametrize("src,dst", SIZE_PAIRS + [((64, 48, 4), (64, 48)), ((64, 48, 3), (64, 48))],
                         ids=lambda v: "x".join(map(str, v)))
def test_coefficient_tables_reproduce_pillow(src, dst):
    from PIL import Image
    (h, w, c), (H, W) = src, dst
    for img in pictures_for(h, w, c)[:1 if h * w > 10 ** 6 else 2]:
        want = np.asarray(Image.fromarray(img).resize((W, H), Image.LANCZOS))
        got = ingest_numpy(img, H, W)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())


def test_tap_counts_are_what_the_kernel_is_documented_for():
    from joint_tensorf_amd.datasets import resample_table
    assert resample_table(800, 400)[1] == 12 and resample_table(4032, 640)[1] == 38 and resample_table(3024, 480)[1] == 38
    assert resample_table(800, 80)[1] == 60 and resample_table(97, 200)[1] <= 7
    tab, taps = resample_table(800, 400)
    assert abs(int(tab[2:, 200].sum()) - (1 << 22)) <= taps        # weights sum to one in 2^22 fixed point, up to their rounding


# ---- test 4: data.load precedence -------------------------------------------------------------------------------------------------

def _forget_data_modules(monkeypatch):
    for k in [k for k in sys.modules if k == "data" or k.startswith("data.")]:
        monkeypatch.delitem(sys.modules, k)


def test_data_load_precedence(tmp_path, monkeypatch, capsys):
    from joint_tensorf_amd import data as jdata
    from tests.test_lifecycle import _small_opt
    _forget_data_modules(monkeypatch)
    dataset_scenes.write_blender_set(tmp_path / "sets", splits={"train": 2, "val": 1}, size=24)
    # 1. opt.data.synthetic set: as before, whatever root says
    opt = _small_opt(data=dict(image_size=[12, 12], num_views=3, synthetic=True, root=str(tmp_path / "sets"), scene="shapes"))
    assert type(jdata.load(opt, "train")).__name__ == "SyntheticDataset"
    # 3. no loader module, root set: the native loader
    opt = _small_opt(data=dict(image_size=[12, 12], num_views=3, synthetic=False, root=str(tmp_path / "sets"), scene="shapes"))
    ds = jdata.load(opt, "train")
    assert type(ds).__name__ == "BlenderDataset" and opt.data.dataset_class == "joint_tensorf_amd.datasets.BlenderDataset"
    assert len(ds) == 2 and ds.all.image.shape == (2, 3, 12, 12)
    assert "SYNTHETIC NOISE" not in capsys.readouterr().out
    # ... and a bad path raises instead of falling back
    opt.data.scene = "nowhere"
    with pytest.raises(FileNotFoundError):
        jdata.load(opt, "train")
    # 4. no loader module, no root: the noise scene with the warning of before
    opt = _small_opt(data=dict(image_size=[12, 12], num_views=3, num_test_views=2, synthetic=False))
    assert not opt.data.get("root", None)
    ds = jdata.load(opt, "train")
    assert type(ds).__name__ == "SyntheticDataset" and opt.data.dataset_class.endswith("SyntheticDataset")
    out = capsys.readouterr().out
    assert "joint_tensorf_amd: WARNING -- no dataset loader `data.blender` on the path" in out and "SYNTHETIC NOISE" in out
    # 2. a reference-style data.blender module on the path wins over the native loader, root or no root
    pkg = tmp_path / "data"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "blender.py").write_text("class Dataset:\n    def __init__(self, opt, split='train', subset=None):\n        self.split = split\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    _forget_data_modules(monkeypatch)
    opt = _small_opt(data=dict(image_size=[12, 12], num_views=3, synthetic=False, root=str(tmp_path / "sets"), scene="shapes"))
    ds = jdata.load(opt, "val")
    assert type(ds).__module__ == "data.blender" and ds.split == "val" and opt.data.dataset_class == "data.blender.Dataset"
    # (popped, not monkeypatch.delitem: its undo would put the stand-in module back for every later test of the process,
    #  and tests/test_gpu_ingest.py's in-process training run would load it in place of the native loader)
    for k in [k for k in sys.modules if k == "data" or k.startswith("data.")]:
        del sys.modules[k]


def test_native_loader_needs_a_known_dataset(tmp_path, monkeypatch):
    from joint_tensorf_amd import data as jdata
    from tests.test_lifecycle import _small_opt
    _forget_data_modules(monkeypatch)
    opt = _small_opt(data=dict(image_size=[12, 12], synthetic=False, root=str(tmp_path), dataset="iphone", scene="x"))
    with pytest.raises(ValueError, match="no native loader"):
        jdata.load(opt, "train")


# ---- test 5: the override parser ---------------------------------------------------------------------------------------------------

def test_override_parser():
    from joint_tensorf_amd import options
    over = options.parse_overrides(["--data.image_size=[40,40]", "--optim.lr_pose=1.e-3", "--data.bgcolor=null", "--data.root=/sets",
                                    "--max_iter=200", "--camera.noise!", "--optim.lr=1e-3", "--data.scene=", "--tb"])
    assert over.data.image_size == [40, 40] and all(isinstance(v, int) for v in over.data.image_size)
    assert over.optim.lr_pose == 1e-3 and isinstance(over.optim.lr_pose, float) and over.optim.lr == 1e-3
    assert over.data.bgcolor is None and "bgcolor" in over.data and over.data.root == "/sets" and over.data.scene is None
    assert over.max_iter == 200 and over.camera.noise is False and over.tb is True
    opt = options.load_options("bat_blender_VM")
    lr_before = opt.optim.lr_pose
    options.apply_overrides(opt, options.parse_overrides(["--data.image_size=[40,40]", "--optim.lr_pose=2.5e-3", "--data.bgcolor=null",
                                                          "--output_path=/out"]))
    assert opt.data.image_size == [40, 40] and opt.optim.lr_pose == 2.5e-3 != lr_before and opt.data.bgcolor is None
    assert opt.data.scene == "lego" and opt.output_path == "/out"          # untouched keys stay
    with pytest.raises(KeyError, match="unknown option --optimm"):
        options.apply_overrides(opt, options.parse_overrides(["--optimm.lr_pose=1.e-3"]))
    with pytest.raises(ValueError):
        options.parse_overrides(["data.root=/sets"])
    with pytest.raises(ValueError, match="twice"):
        options.parse_overrides(["--data.root=/a", "--data.root=/b"])


def test_entry_point_builds_its_options():
    from joint_tensorf_amd import train
    opt = train.build_options(["--yaml=bat_blender_VM", "--data.root=/sets", "--data.scene=chair", "--output_path=/out",
                               "--data.image_size=[64,64]", "--compress=100"])
    assert opt.data.root == "/sets" and opt.data.scene == "chair" and (opt.H, opt.W) == (64, 64) and opt.max_iter == 400
    assert opt.device == "cuda:0" and "compress" not in opt and opt.yaml == "bat_blender_VM"
    with pytest.raises(SystemExit):
        train.build_options(["--data.root=/sets"])
    with pytest.raises(KeyError):
        train.build_options(["--yaml=bat_blender_VM", "--steps=5"])


def test_yaml_copies_carry_the_loader_keys():
    from joint_tensorf_amd.options import load_options
    b, l = load_options("bat_blender_VM"), load_options("bat_llff_VM_MLP")
    assert b.data.root is None and b.data.num_workers == 4 and b.data.bgcolor == 1
    assert l.data.val_ratio == 0.1 and l.data.num_workers == 4
    assert "val_sub" not in b.data and "test_sub" not in b.data       # those would clip the synthetic sets' held-out views


# ---- test 6: the guards -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("data", [dict(center_crop=0.5), dict(augment=dict(hflip=True)), dict(image_size=[None, None])],
                         ids=["center_crop", "augment", "image_size"])
def test_unbuilt_options_are_refused(tmp_path, data):
    from joint_tensorf_amd import datasets
    from joint_tensorf_amd.options import load_options
    dataset_scenes.write_blender_set(tmp_path, splits={"train": 1}, size=16)
    opt = load_options("bat_blender_VM")
    opt.device = "cpu"
    opt.data.update(dict(root=str(tmp_path), scene="shapes", image_size=[8, 8]))
    opt.data.update(data)
    with pytest.raises(NotImplementedError):
        datasets.BlenderDataset(opt, split="train")
    with pytest.raises(NotImplementedError):
        datasets.LLFFDataset(opt, split="train")


def test_decode_threads_follow_the_affinity_mask(monkeypatch):
    from joint_tensorf_amd import datasets
    from joint_tensorf_amd.options import Opt
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: {0, 1, 2})
    monkeypatch.setattr(os, "cpu_count", lambda: 512)
    assert datasets.n_decode_threads(Opt(data=dict(num_workers=8))) == 3
    assert datasets.n_decode_threads(Opt(data=dict(num_workers=2))) == 2


def test_package_does_not_import_the_oracle():
    for name in ("datasets.py", "train.py", "data.py"):
        src = open(os.path.join(ROOT, "joint_tensorf_amd", name)).read()
        assert "oracle" not in src, name
