"""Meshes taken in the NDC box of a forward-facing scene, carried to world space (ops.ndc_to_world, ops.compact_mesh) and drawn by
the unchanged rasteriser: a plane against its analytic world plane, and a lattice of blobs against tests/ndc_ref.py.  No model."""
import math

import numpy as np
import pytest
import torch

from tests import ndc_ref as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
LO, HI = [-1.5, -1.67, -2.0], [1.5, 1.67, 1.0]          # the LLFF scene box (configs/bat_llff_VM_MLP.yaml)
NEAR = 1.0
H, W = 20, 24
SX, SY = 1.25, 1.5                                      # fx = sx cx = 15, fy = sy cy = 15
# a xn + b yn + c zn + d = 0: over the box zn = -0.25 -+ 0.55, inside [-1, 0.5]; inside (vol > 0) is the FAR side, so a camera
# sees the plane first and the cap closes the solid behind it (its far face at zn = 1.5: behind infinity)
PLANE = (0.2, -0.15, 1.0, 0.25)


def _lattice_coords(shape, lo, hi):
    """the fp32 coordinates csrc/jt_mesh.hip gives the lattice points: lo (1 - s) + hi s with s = float(i) / float(n - 1)"""
    out = []
    for a in range(3):
        s = np.arange(shape[a], dtype=np.float32) / np.float32(shape[a] - 1)
        out.append(np.float32(lo[a]) * (np.float32(1) - s) + np.float32(hi[a]) * s)
    return out


def _cameras():
    t = np.array([0.1, -0.05, 0.03])
    a = math.radians(5.0)
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    poses = np.stack([np.concatenate([np.eye(3), np.zeros((3, 1))], 1), np.concatenate([np.eye(3), t[:, None]], 1),
                      np.concatenate([R, t[:, None]], 1)])
    K = np.array([[SX * W / 2, 0, W / 2], [0, SY * H / 2, H / 2], [0, 0, 1.0]])
    return poses, K


def _analytic(pose, K):
    """(depth [H, W] along the camera axis of the ray through every pixel centre to the world plane, its gradient per pixel
    |ds/dpx| + |ds/dpy|, the NDC point [H, W, 3] of the hit), fp64"""
    a, b, c, d = PLANE
    nw, D = np.array([a * SX, b * SY, c + d]), 2 * NEAR * c
    R, t = pose[:, :3], pose[:, 3]
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    dirs = np.stack([(px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1], np.ones_like(px)], -1)
    m = R @ nw                                            # nw . R^T v = (R nw) . v
    num, den = D + m @ t, dirs @ m
    s = num / den
    grad = np.abs(num / den ** 2) * (abs(m[0] / K[0, 0]) + abs(m[1] / K[1, 1]))
    hit = (s[..., None] * dirs - t) @ R                   # R^T (s d - t)
    return s, grad, N.forward(hit, SX, SY, NEAR)


@pytest.mark.parametrize("cap", [False, True])
def test_plane_is_drawn_where_the_world_plane_is(cap):
    from joint_tensorf_amd import mesh_io, ops
    shape = (9, 8, 7)
    a, b, c, d = PLANE
    X, Y, Z = np.meshgrid(*[v.astype(np.float64) for v in _lattice_coords(shape, LO, HI)], indexing="ij")
    vol = torch.from_numpy((a * X + b * Y + c * Z + d).astype(np.float32)).to(DEV)
    lo, hi = LO, HI
    if cap:
        vol, lo, hi = ops.cap_lattice(vol, lo, hi)
    v_ndc, tri = ops.mesh_from_lattice(vol, 0.0, lo, hi)
    world, _, status = ops.ndc_to_world(v_ndc, SX, SY, NEAR)
    v, t, _, _, (n_beyond, n_far) = ops.compact_mesh(world, tri, status)
    zn_tri = v_ndc[:, 2][tri.long()]
    behind = int((zn_tri >= 1.0).any(-1).sum())
    # the far cap (and what hangs on it) lies at zn = 1 + one lattice spacing: counted beyond, every one of them, and not drawn
    assert n_far == 0 and n_beyond == behind and (behind > 0) == cap and t.shape[0] == tri.shape[0] - behind > 0
    assert bool(torch.isfinite(v).all()) and float(v[:, 2].min()) > 0.0
    if cap:
        far_face = int((zn_tri > 1.0).all(-1).sum())
        assert far_face >= 2 * (shape[0] - 1) * (shape[1] - 1)       # the whole far face of the box is closed there
    poses, K = _cameras()
    proj = mesh_io.projection_matrices(torch.from_numpy(poses).float().to(DEV), torch.from_numpy(K).float().to(DEV).expand(3, 3, 3))
    drawn = ops.rasterize(v, t, proj, H, W)
    covered = (drawn.tri >= 0).cpu().numpy()
    depth = drawn.depth.cpu().numpy().astype(np.float64)
    cell = (np.array(HI) - np.array(LO)) / (np.array(shape) - 1)
    for j in range(3):
        s, grad, hit = _analytic(poses[j], K)
        inner = ((hit >= np.array(LO) + cell) & (hit <= np.array(HI) - cell)).all(-1) & (s > 0)
        outer = ~((hit >= np.array(LO) - cell) & (hit <= np.array(HI) + cell)).all(-1) | ~(s > 0)
        assert inner.mean() >= 1 / 3, inner.mean()
        assert covered[j][inner].all() and not covered[j][outer].any(), (j, (~covered[j][inner]).sum(), covered[j][outer].sum())
        # vertex snapping moves the interpolated depth to that of a point at most 1/512 pixel away per axis; the fp32 chain from
        # the lattice to 1/w adds 2^-18 relative
        bound = grad / 512 + 2.0 ** -18 * np.abs(s)
        err = np.abs(depth[j] - s)[covered[j]]
        print("\n[ndc plane] cap %s view %d: %d of %d pixels covered (%d must be), depth error at most %.3g of the bound"
              % (cap, j, covered[j].sum(), H * W, inner.sum(), (err / bound[covered[j]]).max()))
        assert (err <= bound[covered[j]]).all(), (j, (err / bound[covered[j]]).max())


_BLOBS = {}


def _blob_mesh():
    """a 15 x 14 x 13 lattice of Gaussian blobs in NDC coordinates, capped, meshed at 0.3: one blob crosses the far face"""
    if not _BLOBS:
        from joint_tensorf_amd import ops
        shape = (15, 14, 13)
        X, Y, Z = np.meshgrid(*[v.astype(np.float64) for v in _lattice_coords(shape, LO, HI)], indexing="ij")
        centres = [(-0.6, 0.5, -1.2, 0.45), (0.5, -0.6, -0.3, 0.5), (0.2, 0.7, 0.4, 0.4), (-0.5, -0.4, 0.9, 0.5), (0.9, 0.3, -1.6, 0.35)]
        vol = sum(np.exp(-((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) / (2 * s * s)) for cx, cy, cz, s in centres)
        vol, lo, hi = ops.cap_lattice(torch.from_numpy(vol.astype(np.float32)).to(DEV), LO, HI)
        v, t = ops.mesh_from_lattice(vol, 0.3, lo, hi)
        rng = np.random.default_rng(7)
        nrm = rng.normal(size=(v.shape[0], 3))
        nrm = torch.from_numpy((nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)).to(DEV)
        col = torch.from_numpy(rng.uniform(0, 1, (v.shape[0], 3)).astype(np.float32)).to(DEV)
        _BLOBS.update(v=v, t=t, nrm=nrm, col=col)
    return _BLOBS["v"], _BLOBS["t"], _BLOBS["nrm"], _BLOBS["col"]


def _run(max_depth):
    from joint_tensorf_amd import ops
    v, t, nrm, col = _blob_mesh()
    world, wn, status = ops.ndc_to_world(v, SX, SY, NEAR, normals=nrm, max_depth=max_depth)
    return (world, wn, status) + tuple(ops.compact_mesh(world, t, status, normals=wn, colors=col))


def _median_limit():
    """a depth limit at the median vertex depth: half way from the median of the distinct fp32 depths to the next one, so that
    no vertex sits within rounding of it and fp32 and fp64 decide alike"""
    v = _blob_mesh()[0].cpu().numpy().astype(np.float64)
    z = np.unique(N.inverse(v[v[:, 2] < 1.0], SX, SY, NEAR)[:, 2].astype(np.float32))
    k = len(z) // 2
    limit = float(np.float32(0.5 * (float(z[k]) + float(z[k + 1]))))
    assert z[k] < limit < z[k + 1] and (z[k + 1] - z[k]) > 64 * 2.0 ** -24 * limit
    return limit


@pytest.mark.parametrize("limited", [False, True])
def test_blob_lattice_compaction(limited):
    v, t, nrm, col = _blob_mesh()
    max_depth = _median_limit() if limited else None
    world, wn, status, v2, t2, n2, c2, (n_beyond, n_far) = _run(max_depth)
    nt = t.shape[0]
    assert nt > 500 and t2.shape[0] + n_beyond + n_far == nt and n_beyond > 0 and (n_far > 0) == limited and t2.shape[0] > 100
    # the reference's filter on the reference's statuses: exactly these triangles and vertices, in this order
    vq = v.cpu().numpy().astype(np.float64)
    _, _, want_status = N.unwarp(vq, SX, SY, NEAR, max_depth=max_depth)
    assert (status.cpu().numpy() == want_status).all()
    rv, rt, rn, rc, dropped = N.compact(world.cpu().numpy(), t.cpu().numpy(), want_status, normals=wn.cpu().numpy(), colors=col.cpu().numpy())
    assert dropped == (n_beyond, n_far)
    assert t2.dtype == torch.int32 and (t2.cpu().numpy() == rt).all()                 # kept triangles keep their relative order
    assert (v2.cpu().numpy() == rv).all() and (n2.cpu().numpy() == rn).all() and (c2.cpu().numpy() == rc).all()    # bit for bit
    # every id in range, every vertex referenced
    ids = t2.cpu().numpy()
    assert ids.min() == 0 and ids.max() == v2.shape[0] - 1 and len(np.unique(ids)) == v2.shape[0]
    # winding: the fp64 world face normal against J^T of the NDC face normal at the centroid
    keep, _ = N.filter_triangles(t.cpu().numpy(), want_status)
    tri_ndc = vq[t.cpu().numpy()[keep]]
    tri_world = N.inverse(tri_ndc, SX, SY, NEAR)
    fn_ndc = np.cross(tri_ndc[:, 1] - tri_ndc[:, 0], tri_ndc[:, 2] - tri_ndc[:, 0])
    fn_world = np.cross(tri_world[:, 1] - tri_world[:, 0], tri_world[:, 2] - tri_world[:, 0])
    carried = N.normal_to_world(tri_ndc.mean(1), fn_ndc, SX, SY)
    assert ((fn_world * carried).sum(-1) > 0).all()
    # and the result is the kept triangles' own corners
    assert (v2.cpu().numpy()[ids] == world.cpu().numpy()[t.cpu().numpy()[keep]]).all()
    # two runs give the same bits
    again = _run(max_depth)
    for a, b in zip((world, wn, status, v2, t2, n2, c2), again[:7]):
        assert torch.equal(a, b)
    assert again[7] == (n_beyond, n_far)
    print("\n[ndc blobs] limit %r: %d triangles = %d kept + %d beyond + %d far; %d of %d vertices used"
          % (max_depth, nt, t2.shape[0], n_beyond, n_far, v2.shape[0], v.shape[0]))


def test_compaction_without_attributes_and_with_nothing_left():
    from joint_tensorf_amd import ops
    v, t, nrm, col = _blob_mesh()
    world, _, status = ops.ndc_to_world(v, SX, SY, NEAR)
    v2, t2, n2, c2, dropped = ops.compact_mesh(world, t, status)
    full = _run(None)
    assert n2 is None and c2 is None and torch.equal(v2, full[3]) and torch.equal(t2, full[4]) and dropped == full[7]
    v3, t3, n3, c3, dropped = ops.compact_mesh(world, t, torch.ones_like(status), normals=nrm)
    assert tuple(v3.shape) == (0, 3) and tuple(t3.shape) == (0, 3) and tuple(n3.shape) == (0, 3) and c3 is None
    assert dropped == (t.shape[0], 0)
