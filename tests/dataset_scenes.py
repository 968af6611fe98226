"""Closed-form image sets for the dataset loaders' tests and for tools/make_dataset_golden.py: pictures are integer
formulas of x, y, channel and view index (no random-number library between the tool that records the fixtures and the
test that reads them: both produce identical bytes), cameras are closed-form look-at matrices.  The alpha channel has a
hard-edged disc, a soft ramp and isolated partially transparent pixels: the three kinds of content the premultiplied
resampling of an RGBA picture treats differently."""
import json
import math
import os

import numpy as np

BLENDER_SPLITS = {"train": 3, "val": 3, "test": 2}     # views per split of the recorded set
BLENDER_RAW = 800
LLFF_VIEWS, LLFF_H, LLFF_W = 12, 3024, 4032


def picture(h, w, c, view=0):
    """uint8 [h, w, c]: smooth gradients, a high-frequency lattice and hard edges in the colour; c = 4 adds the alpha channel"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    out = np.empty((h, w, c), np.uint8)
    for ch in range(3):
        smooth = (x * (2 + ch) + y * (3 - ch) + 40 * view) // 5
        lattice = ((x * 7 + y * 13 + ch * 29 + view * 11) * (x + 3 * y + 1)) % 61
        edge = 90 * (((x // (9 + ch)) + (y // (14 - ch)) + view) % 2)
        out[..., ch] = (smooth + lattice + edge) % 256
    if c == 4:
        r2 = (2 * x - w + 1) ** 2 + (2 * y - h + 1) ** 2                     # (2 r)^2 about the picture centre
        alpha = np.where(r2 * 9 < 4 * min(h, w) ** 2, 255, 0)                 # hard-edged disc of radius min(h, w) / 3
        ramp = np.clip((x - w // 8) * 255 // max(w // 3, 1), 0, 255)          # soft ramp across a third of the width
        alpha = np.where(y * 4 < h, ramp, alpha)                              # ... over the top quarter
        partial = (x * 7 + y * 13 + view * 5) % 97 == 0                       # isolated partial pixels
        alpha = np.where(partial, (x * 31 + y * 17 + view * 3) % 256, alpha)
        out[..., 3] = alpha
    return out


def look_at_matrix(k):
    """camera-to-world 4 x 4 of view k: on a sphere of radius 4, looking at the origin (the Blender sets' convention: the camera
    looks along its -z)"""
    theta, phi = 2 * math.pi * (0.13 * k + 0.05), 0.3 + 0.1 * k
    p = 4.0 * np.array([math.cos(theta) * math.cos(phi), math.sin(theta) * math.cos(phi), math.sin(phi)])
    z = p / np.linalg.norm(p)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, p
    return m


def blender_meta(split, n, first_view=0, camera_angle_x=0.6911112070083618):
    return {"camera_angle_x": camera_angle_x,
            "frames": [{"file_path": "./%s/r_%d" % (split, i), "rotation": 0.0125,
                        "transform_matrix": look_at_matrix(first_view + i).tolist()} for i in range(n)]}


def write_blender_set(root, scene="shapes", splits=None, size=BLENDER_RAW, channels=4, pictures=None):
    """<root>/<scene>/transforms_<split>.json + <split>/r_<i>.png.  `pictures`: {split: uint8 [n, h, w, c]} instead of the
    generator's.  Returns {split: meta}."""
    from PIL import Image
    splits = dict(BLENDER_SPLITS if splits is None else splits)
    base = os.path.join(str(root), scene)
    metas, first = {}, 0
    for split, n in splits.items():
        os.makedirs(os.path.join(base, split), exist_ok=True)
        metas[split] = blender_meta(split, n, first_view=first)
        with open(os.path.join(base, "transforms_%s.json" % split), "w") as f:
            json.dump(metas[split], f)
        for i in range(n):
            a = picture(size, size, channels, view=first + i) if pictures is None else np.asarray(pictures[split][i])
            Image.fromarray(a).save(os.path.join(base, split, "r_%d.png" % i), compress_level=1)
        first += n
    return metas


def llff_poses_bounds(n=LLFF_VIEWS, h=LLFF_H, w=LLFF_W, focal=3260.526333):
    """[n, 17] float64: [R | t | (h, w, focal)] row-major 3 x 5, near, far -- forward-facing cameras on a small arc"""
    out = np.zeros((n, 17))
    for k in range(n):
        a, b = 0.04 * (k - n / 2), 0.03 * math.sin(0.9 * k)
        Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
        R = Ry @ Rx
        t = np.array([0.35 * (k - n / 2), 0.2 * math.cos(0.7 * k), 0.05 * k])
        m = np.concatenate([R, t[:, None], np.array([[h], [w], [focal]], dtype=np.float64)], axis=1)
        out[k, :15] = m.reshape(-1)
        out[k, 15:] = 1.2 + 0.05 * k, 9.0 + 0.3 * k
    return out


def write_llff_set(root, scene="arc", poses_bounds=None, n_files=None, size=None, channels=3, flat=False):
    """<root>/<scene>/poses_bounds.npy + images/image<k>.png; `size` (h, w) of the files (default: what poses_bounds states);
    `flat`: pictures of one colour each (a 3024 x 4032 picture of the generator's takes seconds to encode, a flat one does not:
    for tests that read the cameras)"""
    from PIL import Image
    pb = llff_poses_bounds() if poses_bounds is None else poses_bounds
    base = os.path.join(str(root), scene)
    os.makedirs(os.path.join(base, "images"), exist_ok=True)
    np.save(os.path.join(base, "poses_bounds.npy"), pb)
    h, w = (int(pb[0, 4]), int(pb[0, 9])) if size is None else size
    for k in range(len(pb) if n_files is None else n_files):
        a = np.full((h, w, channels), 16 * k % 256, np.uint8) if flat else picture(h, w, channels, view=k)
        Image.fromarray(a).save(os.path.join(base, "images", "image%03d.png" % k), compress_level=1)
    return pb
