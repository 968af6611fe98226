"""Native loaders of the two image-set layouts the BAT yamls train on: Blender (`nerf_synthetic/<scene>`) and LLFF
(`nerf_llff_data/<scene>`).  They restate the reference's loaders (data/base.py, data/blender.py, data/llff.py: camera
parsing, file decoding, `preprocess_image`, `preprocess_camera`) with PIL as the only decoder, have the interface of
data.DictDataset and fill `.all` (idx int64 [N], image fp32 [N,3,H,W], pose fp32 [N,3,4], intr / intr_inv fp32 [N,3,3])
directly on `opt.device`.

The picture preprocessing -- `PIL.Image.resize((W, H), LANCZOS)`, `to_tensor`, the Blender composite over
`opt.data.bgcolor` -- runs on the device (ops.image_ingest, csrc/jt_ingest.hip) and is equal bit for bit to the host ops:
decoded bytes -> pinned host buffer -> device -> kernel, in batches, so the fp32 set is never staged on the host.  On a
CPU device the reference's own op sequence runs (Pillow, the division, the composite in torch); that path is what the
GPU path is tested against, not a second implementation of the resampling."""
import json
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .data import DictDataset
from .options import Opt

# `val_sub: 10` / `test_sub: 200` of options/tensorf_blender_VM.yaml:98-99: how many held-out Blender views the reference
# evaluates.  Not in this package's yamls (Model.load_dataset hands those keys to the synthetic sets as `subset`, and a
# default there would clip runs that ask for more held-out views): BlenderDataset applies them when it is given subset=None.
BLENDER_HELD_OUT_SUBSET = {"val": 10, "test": 200}

PRECISION_BITS = 32 - 8 - 2     # of Pillow's 8-bit resampling: weights are 2^22 fixed point


# ---- the resampling tables (host, double precision) ------------------------------------------------------------------------------

def _lanczos(x):
    """Pillow's LANCZOS kernel, a = 3: sinc(x) sinc(x / 3) on [-3, 3), sinc(x) = sin(pi x) / (pi x)"""
    if not (-3.0 <= x < 3.0):
        return 0.0
    if x == 0.0:
        return 1.0
    a, b = x * math.pi, (x / 3.0) * math.pi
    return (math.sin(a) / a) * (math.sin(b) / b)


_TABLES = {}


def resample_coeffs(n_in, n_out):
    """The coefficients of one axis of `PIL.Image.resize(..., LANCZOS)` on 8-bit pictures, from n_in to n_out samples:
    (first [n_out] int32, count [n_out] int32, weights [n_out, taps] int32, zero beyond count).  For output index x, in double
    precision: scale = n_in / n_out, fs = max(scale, 1), support = 3 fs, center = (x + 0.5) scale, the window
    [max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n_in)), weights L((i + first - center + 0.5) / fs)
    divided by their sum and rounded to 2^22 fixed point half away from zero.  One output byte is then
    clamp((2^21 + sum_i k_i in[first + i]) >> 22, 0, 255)."""
    key = (int(n_in), int(n_out))
    if key not in _TABLES:
        n_in, n_out = key
        scale = n_in / n_out
        fs = max(scale, 1.0)
        support = 3.0 * fs
        taps = int(math.ceil(support)) * 2 + 1
        first = np.zeros(n_out, np.int32)
        count = np.zeros(n_out, np.int32)
        weights = np.zeros((n_out, taps), np.int32)
        ss = 1.0 / fs
        one = float(1 << PRECISION_BITS)
        for x in range(n_out):
            center = (x + 0.5) * scale
            x0 = max(int(center - support + 0.5), 0)
            n = min(int(center + support + 0.5), n_in) - x0
            w = [_lanczos((i + x0 - center + 0.5) * ss) for i in range(n)]
            total = 0.0
            for v in w:
                total += v
            if total != 0.0:
                w = [v / total for v in w]
            first[x], count[x] = x0, n
            weights[x, :n] = [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in w]   # (int() truncates)
        used = max(int(count.max()), 1)
        _TABLES[key] = (first, count, np.ascontiguousarray(weights[:, :used]))
    return _TABLES[key]


def resample_table(n_in, n_out):
    """resample_coeffs in the layout jt_image_ingest reads (include/jt_render.h): int32 [2 + taps, n_out], row 0 the first source
    index, row 1 the tap count, row 2 + i the weight of tap i.  Returns (table, taps)."""
    first, count, weights = resample_coeffs(n_in, n_out)
    return np.ascontiguousarray(np.concatenate([first[None], count[None], weights.T], axis=0).astype(np.int32)), weights.shape[1]


# ---- pose algebra (camera.py:11-57), fp32 torch, the reference's order of products ------------------------------------------------

def _pose(R, t):
    return torch.cat([R, t[..., None]], dim=-1)


def pose_invert(pose):
    """camera.py:34-40"""
    R, t = pose[..., :3], pose[..., 3:]
    R_inv = R.transpose(-1, -2)
    return _pose(R_inv, (-R_inv @ t)[..., 0])


def pose_compose(pose_list):
    """camera.py:42-57: x -> poseN(... pose2(pose1(x)))"""
    new = pose_list[0]
    for p in pose_list[1:]:
        R_a, t_a = new[..., :3], new[..., 3:]
        R_b, t_b = p[..., :3], p[..., 3:]
        new = _pose(R_b @ R_a, (R_b @ t_a + t_b)[..., 0])
    return new


def _pose_flip():
    """camera.pose(R=diag(1, -1, -1)) (data/blender.py:87): an integer rotation beside a float translation, fp32 after the cat"""
    R = torch.diag(torch.tensor([1, -1, -1]))
    return _pose(R, torch.zeros(R.shape[:-1]))


# ---- decoding and preprocessing ------------------------------------------------------------------------------------------------

def n_decode_threads(opt):
    """opt.data.num_workers threads, capped by the CPUs this process may run on (never os.cpu_count(): a container or a
    job slot usually owns a fraction of the machine)"""
    return max(1, min(int(opt.data.get("num_workers", 4) or 1), len(os.sched_getaffinity(0))))


def decode(path):
    """one file -> uint8 [h, w, c] as the decoder leaves it (the reference: PIL.Image.fromarray(imageio.imread(path)))"""
    from PIL import Image
    with Image.open(path) as im:
        im.load()
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGBA" if "A" in im.getbands() or "transparency" in im.info else "RGB")
        return np.asarray(im)


def preprocess_image_host(opt, array, H, W):
    """data/base.py:92-107 + data/blender.py:71-76 with the reference's own ops: Pillow's LANCZOS resize, to_tensor (HWC bytes
    -> CHW fp32 divided by 255), the composite over opt.data.bgcolor for a picture with alpha.  -> fp32 [3, H, W]"""
    from PIL import Image
    image = Image.fromarray(array).resize((W, H), Image.LANCZOS)
    image = torch.from_numpy(np.asarray(image).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    rgb, mask = image[:3], image[3:]
    bg = opt.data.get("bgcolor", None)
    if mask.shape[0] and bg is not None:
        rgb = rgb * mask + bg * (1 - mask)
    return rgb


def _check_supported(opt):
    """what these loaders do not build, in the style of the guards of tensorf_repr.py"""
    if opt.data.get("center_crop", None) is not None:
        raise NotImplementedError("data.center_crop is not built (None in every BAT yaml)")
    if opt.data.get("augment", None):
        raise NotImplementedError("data.augment is not built (empty in every BAT yaml)")
    size = opt.data.get("image_size", None)
    if size is None or len(size) != 2 or any(v is None for v in size):
        raise NotImplementedError("data.image_size must name a height and a width (both BAT yamls do)")


class _FileDataset(DictDataset):
    """what the two layouts share: the guards, the resident `.all`, batched decoding and ingest"""

    # decoded bytes of one upload: a batch is at most this large (a 3024 x 4032 x 3 picture is 36.6 MB)
    BATCH_BYTES = 256 << 20

    def __init__(self, opt, split):
        _check_supported(opt)
        self.opt, self.split = opt, split
        self.H, self.W = (int(v) for v in opt.data.image_size)
        self.all = None

    def _finish(self, opt, files, intr, pose):
        """files: the pictures of this split; intr [3,3] / pose [N,3,4] raw -> self.all on opt.device"""
        n = len(files)
        self.list = list(range(n))
        intr_inv, intr = self._preprocess_camera(intr)
        image = self._load_images(opt, files)
        dev = opt.device
        self.all = Opt(dict(idx=torch.arange(n, dtype=torch.int64, device=dev), image=image,
                                  pose=pose.to(torch.float32).to(dev), intr=intr[None].repeat(n, 1, 1).to(dev),
                                  intr_inv=intr_inv[None].repeat(n, 1, 1).to(dev)))

    def _preprocess_camera(self, intr):
        """data/base.py:109-119 without a crop: the intrinsics rows scaled to the training size, the inverse in fp32"""
        intr = intr.clone()
        intr[0] *= self.W / self.raw_W
        intr[1] *= self.H / self.raw_H
        return intr.inverse().to(torch.float32), intr

    def _check_size(self, array, path):
        raise NotImplementedError

    def _load_images(self, opt, files):
        n, H, W = len(files), self.H, self.W
        on_device = torch.device(opt.device).type != "cpu"
        out = torch.empty(n, 3, H, W, dtype=torch.float32, device=opt.device)
        if n == 0:
            return out
        with ThreadPoolExecutor(max_workers=n_decode_threads(opt)) as pool:
            if not on_device:
                def one(i):
                    a = decode(files[i])
                    self._check_size(a, files[i])
                    out[i] = preprocess_image_host(opt, a, H, W)
                list(pool.map(one, range(n)))
                return out
            from . import ops
            first = decode(files[0])
            self._check_size(first, files[0])
            h, w, c = first.shape
            per = max(1, min(n, self.BATCH_BYTES // first.nbytes))
            pinned = torch.empty(per, h, w, c, dtype=torch.uint8).pin_memory()
            staged = torch.empty(per, h, w, c, dtype=torch.uint8, device=opt.device)
            view = pinned.numpy()

            def one(job):
                slot, i = job
                a = first if i == 0 else decode(files[i])
                self._check_size(a, files[i])
                if a.shape != (h, w, c):
                    raise ValueError("%s decodes to %s, the first picture of the split to %s" % (files[i], a.shape, (h, w, c)))
                view[slot] = a
            for lo in range(0, n, per):
                hi = min(lo + per, n)
                list(pool.map(one, [(i - lo, i) for i in range(lo, hi)]))
                staged[:hi - lo].copy_(pinned[:hi - lo], non_blocking=True)
                ops.image_ingest(staged[:hi - lo], out[lo:hi], H, W, opt.data.get("bgcolor", None))
                torch.cuda.current_stream().synchronize()   # the pinned buffer is refilled next
        return out

    def prefetch_all_data(self, opt):
        return None     # resident since construction (`preload: true` in both BAT yamls)

    def get_all_camera_poses(self, opt):
        return self.all.pose


class BlenderDataset(_FileDataset):
    """data/blender.py:19-91: <root>/<scene>/transforms_<split>.json, frames in file order, pictures <file_path>.png."""

    def __init__(self, opt, split="train", subset=None):
        super().__init__(opt, split)
        self.root = opt.data.root or "data/blender"
        self.path = "{}/{}".format(self.root, opt.data.scene)
        with open("{}/transforms_{}.json".format(self.path, split)) as f:
            self.meta = json.load(f)
        frames = self.meta["frames"]
        if subset is None:
            subset = BLENDER_HELD_OUT_SUBSET.get(split, None)
        if subset:
            frames = frames[:int(subset)]
        if not frames:
            raise ValueError("%s/transforms_%s.json lists no frames" % (self.path, split))
        self.frames = frames
        files = ["{}/{}.png".format(self.path, f["file_path"]) for f in frames]
        # The reference hard-codes raw_H, raw_W = 800, 800 without looking at the files (data/blender.py:20).  Here the raw size is
        # that of the first decoded file and every file of the split has to agree (_check_size): identical on every real Blender
        # set, and a set rendered at another size gets right intrinsics instead of silently wrong ones.
        self.raw_H, self.raw_W = decode(files[0]).shape[:2]
        self.focal = 0.5 * self.raw_W / np.tan(0.5 * self.meta["camera_angle_x"])
        intr = torch.tensor([[self.focal, 0, self.raw_W / 2], [0, self.focal, self.raw_H / 2], [0, 0, 1]]).float()
        pose = torch.stack([self.parse_raw_camera(torch.tensor(f["transform_matrix"], dtype=torch.float32)) for f in frames])
        self._finish(opt, files, intr, pose)

    def _check_size(self, array, path):
        if array.shape[:2] != (self.raw_H, self.raw_W):
            raise ValueError("%s is %d x %d, the first picture of the split %d x %d" % ((path,) + array.shape[:2] + (self.raw_H, self.raw_W)))

    @staticmethod
    def parse_raw_camera(pose_raw):
        """data/blender.py:86-91"""
        pose = pose_invert(pose_compose([_pose_flip(), pose_raw[:3]]))
        assert not pose.isnan().any()
        return pose


class LLFFDataset(_FileDataset):
    """data/llff.py:19-142: <root>/<scene>/poses_bounds.npy [N,17] and images/ in sorted order; the last int(N * val_ratio)
    entries are the val / test split, the rest train."""

    def __init__(self, opt, split="train", subset=None):
        super().__init__(opt, split)
        self.root = opt.data.root or "data/llff"
        self.path = "{}/{}".format(self.root, opt.data.scene)
        self.path_image = "{}/images".format(self.path)
        names = sorted(os.listdir(self.path_image))
        poses_raw, bounds = self.parse_cameras_and_bounds(np.load("{}/poses_bounds.npy".format(self.path)))
        if len(names) != len(poses_raw):
            raise ValueError("%s holds %d files, poses_bounds.npy %d cameras" % (self.path_image, len(names), len(poses_raw)))
        entries = list(zip(names, poses_raw, bounds))
        n_val = int(len(entries) * opt.data.val_ratio)
        if n_val == 0:
            # the reference's list[:-0] would make the TRAIN split empty here (data/llff.py:29-31)
            raise ValueError("data.val_ratio %g of %d views leaves no held-out view: raise it to at least %g"
                             % (opt.data.val_ratio, len(entries), 1.0 / max(len(entries), 1)))
        entries = entries[:-n_val] if split == "train" else entries[-n_val:]
        if subset:
            entries = entries[:int(subset)]
        if not entries:
            raise ValueError("the %s split of %s is empty" % (split, self.path))
        self.entries, self.bounds = entries, torch.stack([e[2] for e in entries])
        intr = torch.tensor([[self.focal, 0, self.raw_W / 2], [0, self.focal, self.raw_H / 2], [0, 0, 1]]).float()
        pose = torch.stack([self.parse_raw_camera(e[1]) for e in entries])
        self._finish(opt, ["{}/{}".format(self.path_image, e[0]) for e in entries], intr, pose)

    def _check_size(self, array, path):
        # (the reference asserts 3024 x 4032, data/llff.py:20,53; here the files must have the size poses_bounds.npy states)
        if array.shape[:2] != (self.raw_H, self.raw_W):
            raise ValueError("%s is %d x %d, poses_bounds.npy states %d x %d" % ((path,) + array.shape[:2] + (self.raw_H, self.raw_W)))

    def parse_cameras_and_bounds(self, array):
        """data/llff.py:43-61; [N,17] = [R | t | (h, w, focal)] row-major 3 x 5, then near, far"""
        data = torch.tensor(array, dtype=torch.float32)
        cam_data = data[:, :-2].view([-1, 3, 5])
        poses_raw = cam_data[..., :4]
        poses_raw[..., 0], poses_raw[..., 1] = poses_raw[..., 1], -poses_raw[..., 0]   # (:51, on views of `data`, as there)
        raw_H, raw_W, self.focal = cam_data[0, :, -1]
        self.raw_H, self.raw_W = int(raw_H), int(raw_W)
        bounds = data[:, -2:]
        scale = 1. / (bounds.min() * 0.75)
        poses_raw[..., 3] *= scale
        bounds *= scale
        return self.center_camera_poses(poses_raw), bounds

    @staticmethod
    def center_camera_poses(poses):
        """data/llff.py:82-97, the new form"""
        center = poses[..., 3].mean(dim=0)
        vz = torch.nn.functional.normalize(poses[..., 2].mean(dim=0), dim=0)
        vy_hat = poses[..., 1].mean(dim=0)
        vx = torch.nn.functional.normalize(torch.linalg.cross(vy_hat, vz), dim=0)
        vy = torch.linalg.cross(vz, vx)
        pose_avg = torch.stack([vx, vy, vz, center], dim=-1)[None]
        return pose_compose([poses, pose_invert(pose_avg)])

    @staticmethod
    def parse_raw_camera(pose_raw):
        """data/llff.py:137-142"""
        flip = _pose_flip()
        return pose_compose([flip, pose_invert(pose_compose([flip, pose_raw[:3]]))])


NATIVE = {"blender": BlenderDataset, "llff": LLFFDataset}
