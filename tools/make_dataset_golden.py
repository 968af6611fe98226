#!/usr/bin/env python3
"""Record what the reference's dataset loaders (data/base.py, data/blender.py, data/llff.py) make of the closed-form image
sets of tests/dataset_scenes.py: tests/golden/dataset_blender.npz and tests/golden/dataset_llff_cameras.npz.

Runs ONLY where the reference checkout exists (tools/make_golden.py: REF), with that tool's stand-ins for the reference's
non-arithmetic imports.  Two of them are answered here instead of stubbed out: `imageio.imread` by PIL (decode the file,
hand back the array), and torchvision's `to_tensor`, which is not installed: the stand-in states its documented rule for an
8-bit PIL picture -- HWC bytes -> CHW fp32 divided by 255 -- and nothing else of it.  The fixtures are data only: the
tensors the reference's `prefetch_all_data` collates, its camera tensors, and the generator's camera files.

Re-run:  python tools/make_dataset_golden.py [--out tests/golden]"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden  # noqa: E402  (the stub-import mechanism and the reference's location)
from tests import dataset_scenes  # noqa: E402


def to_tensor(pic):
    """torchvision.transforms.functional.to_tensor on an 8-bit PIL picture, by its documented rule: HWC bytes in [0, 255] ->
    CHW fp32 in [0, 1], divided by 255"""
    a = np.asarray(pic)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def imread(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im).copy()


def import_loaders():
    make_golden._install_stubs()
    sys.modules["torchvision.transforms.functional"].to_tensor = to_tensor
    sys.modules["imageio"].imread = imread
    import types
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            m = types.ModuleType("tqdm")
            m.tqdm = lambda it, **k: it
            sys.modules["tqdm"] = m
    sys.path.insert(0, make_golden.REF)
    cwd = os.getcwd()
    os.chdir(make_golden.REF)
    import data.blender as blender
    import data.llff as llff
    os.chdir(cwd)
    return blender, llff


def ref_opt(dataset, root, scene, image_size, **data):
    d = dict(dataset=dataset, root=root, scene=scene, image_size=list(image_size), num_workers=4, preload=False,
             augment={}, center_crop=None, bgcolor=None, val_ratio=0.1)
    d.update(data)
    return make_golden.EasyDict(dict(data=d, H=image_size[0], W=image_size[1], batch_size=1, device="cpu"))


def collated(ds, opt):
    ds.prefetch_all_data(opt)
    return {k: ds.all[k].numpy() for k in ("idx", "image", "pose", "intr", "intr_inv")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    blender, llff = import_loaders()
    with tempfile.TemporaryDirectory() as tmp:
        # ---- Blender: 3 train / 3 val / 2 test frames at 800 x 800 RGBA -> 80 x 80 over white, val_sub 2 ---------------------
        metas = dataset_scenes.write_blender_set(tmp)
        opt = ref_opt("blender", tmp, "shapes", (80, 80), bgcolor=1, val_sub=2)
        out = {}
        for split, subset in (("train", None), ("val", 2), ("test", None)):
            ds = blender.Dataset(opt, split=split, subset=subset)
            for k, v in collated(ds, opt).items():
                out["%s.%s" % (split, k)] = v
            out["%s.camera_angle_x" % split] = np.float64(metas[split]["camera_angle_x"])
            out["%s.transform_matrix" % split] = np.array([f["transform_matrix"] for f in metas[split]["frames"]], np.float64)
        np.savez_compressed(os.path.join(args.out, "dataset_blender.npz"), **out)
        print("dataset_blender.npz:", {k: v.shape for k, v in out.items()})
        # ---- LLFF cameras: 12 views, 3024 x 4032, val_ratio 0.1; preload false: the reference opens no picture for these ---
        pb = dataset_scenes.llff_poses_bounds()
        base = os.path.join(tmp, "arc")
        os.makedirs(os.path.join(base, "images"))
        np.save(os.path.join(base, "poses_bounds.npy"), pb)
        for k in range(len(pb)):
            open(os.path.join(base, "images", "image%03d.png" % k), "w").close()     # names only
        opt = ref_opt("llff", tmp, "arc", (480, 640))
        out = {"poses_bounds": pb}
        for split in ("train", "val"):
            ds = llff.Dataset(opt, split=split)
            cams = [ds.preprocess_camera(opt, *ds.get_camera(opt, i)) for i in range(len(ds))]
            out["%s.intr_inv" % split] = torch.stack([c[0] for c in cams]).numpy()
            out["%s.pose" % split] = torch.stack([c[1] for c in cams]).numpy()
            out["%s.intr" % split] = torch.stack([c[2] for c in cams]).numpy()
            out["%s.all_camera_poses" % split] = ds.get_all_camera_poses(opt).numpy()
        np.savez_compressed(os.path.join(args.out, "dataset_llff_cameras.npz"), **out)
        print("dataset_llff_cameras.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
