#!/usr/bin/env python3
"""Record the reference's two novel-view pose generators (camera.py:368-402) to tests/golden/novel_poses.npz.

Runs ONLY where the reference checkout exists (tools/make_golden.py: REF), with that tool's stand-ins for the reference's
non-arithmetic imports.  The fixture is data only -- the inputs handed to the generators and the pose arrays they returned --
and is what joint_tensorf_amd/novel_views.py is held to (tests/test_eval_outputs.py).  Re-run:
    python tools/make_eval_golden.py  [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden  # noqa: E402  (the stub-import mechanism and the reference's location)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    out_dir = os.path.abspath(args.out)
    from joint_tensorf_amd.options import load_options
    bbox = [float(v) for v in load_options("bat_blender_VM").data.scene_bbox]
    make_golden._install_stubs()
    sys.path.insert(0, make_golden.REF)
    cwd = os.getcwd()
    os.chdir(make_golden.REF)
    try:
        import camera
    finally:
        os.chdir(cwd)
    opt = make_golden.EasyDict(device="cpu", data=dict(scene_bbox=bbox))
    # scales as evaluate_full hands them over: 1 (no alignment) and a 0-dim fp32 tensor (sim3.s1 / sim3.s0)
    s_bbox, s_llff = torch.tensor(1.23, dtype=torch.float32), torch.tensor(0.83, dtype=torch.float32)
    # a non-trivial anchor: a rotation about a skew axis and an offset camera (camera.lie: the reference's own exponential map)
    w = torch.tensor([0.31, -0.42, 0.17])
    anchor = camera.pose(R=camera.lie.so3_to_SO3(w), t=torch.tensor([0.4, -0.25, 3.1])).float()
    arrays = {
        "bbox.scene_bbox": np.asarray(bbox, np.float32),
        "bbox.scale_b": s_bbox.numpy(),
        "bbox.poses_1": camera.get_novel_view_around_bbox(opt, N=120, scale=1).numpy(),
        "bbox.poses_b": camera.get_novel_view_around_bbox(opt, N=120, scale=s_bbox).numpy(),
        "llff.anchor": anchor.numpy(),
        "llff.scale_b": s_llff.numpy(),
        "llff.poses_1": camera.get_novel_view_poses(opt, anchor, N=60, scale=1).numpy(),
        "llff.poses_b": camera.get_novel_view_poses(opt, anchor, N=60, scale=s_llff).numpy(),
    }
    for k, v in arrays.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    path = os.path.join(out_dir, "novel_poses.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
