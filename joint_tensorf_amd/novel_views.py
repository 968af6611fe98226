"""Camera paths of the novel-view videos (Model.generate_videos_synthesis, model/nerf.py:574-620): host code in fp32 torch,
held to the reference's two generators by tests/golden/novel_poses.npz (tools/make_eval_golden.py records it).

Poses are [N, 3, 4] world-to-camera [R | t], the layout of every pose of this package.  Both paths are evaluated on the
HOST whatever the training device is: the frames of a run do not depend on a device's trigonometric functions."""
import math

import torch


def _rot(angle, axis):
    """rotation by `angle` [...] about a coordinate axis -> [..., 3, 3]  (camera.py:220-229)"""
    a = torch.as_tensor(angle, dtype=torch.float32)
    c, s, o, i = a.cos(), a.sin(), torch.zeros_like(a), torch.ones_like(a)
    rows = {"X": ((i, o, o), (o, c, -s), (o, s, c)),
            "Y": ((c, o, s), (o, i, o), (-s, o, c)),
            "Z": ((c, -s, o), (s, c, o), (o, o, i))}[axis]
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2)


def _compose(first, then):
    """x -> then(first(x)) for [..., 3, 4] poses  (camera.py:50-57)"""
    R = then[..., :3] @ first[..., :3]
    t = then[..., :3] @ first[..., 3:] + then[..., 3:]
    return torch.cat([R, t], dim=-1)


def _scalar(scale):
    return torch.as_tensor(scale).detach().to("cpu", torch.float32).reshape(())


def around_bbox(scene_bbox, n=120, scale=1):
    """camera.py:380-402 (Blender): a full turn about the vertical axis of the scene box, at 0.6 box diagonals from its centre
    line and a tenth of the box height above it, pitched down to look at the centre."""
    bbox = torch.tensor([float(v) for v in scene_bbox], dtype=torch.float32).view(2, 3)
    scale = _scalar(scale)
    diag = torch.norm(bbox[0] - bbox[1])
    theta = torch.arange(n) / n * 2 * math.pi
    dist = diag * 0.6 * scale
    height = (bbox[1, 1] - bbox[0, 1]).abs() * 0.1 * scale
    R = _rot(torch.atan(height / dist), "X") @ _rot(theta, "Y") @ _rot(torch.full_like(theta, math.pi / 2), "X")
    t = torch.stack([torch.zeros_like(theta), torch.full_like(theta, float(height)), torch.full_like(theta, float(dist))], dim=-1)
    return torch.cat([R, t[..., None]], dim=-1)


def around_pose(pose_anchor, n=60, scale=1):
    """camera.py:368-378 (LLFF): a small circular oscillation (sin 0.05 either way) about a point 4 scaled units in front of
    the anchor camera, pulled 0.2 scaled units towards it."""
    anchor = pose_anchor.detach().to("cpu", torch.float32)
    scale = _scalar(scale)      # (an fp32 tensor: 3.8 * scale rounds as the reference's tensor product does)
    theta = torch.arange(n) / n * 2 * math.pi
    R = _rot((theta.cos() * 0.05).asin(), "Y") @ _rot((theta.sin() * 0.05).asin(), "X")
    rot = torch.cat([R, torch.zeros(n, 3, 1)], dim=-1)

    def shift(z):
        return torch.cat([torch.eye(3), torch.tensor([[0.0], [0.0], [float(z)]])], dim=-1)
    oscillation = _compose(_compose(shift(-4.0 * scale), rot), shift(3.8 * scale))
    return _compose(oscillation, anchor[None])
