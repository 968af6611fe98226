"""tests/fusion_ref.py -- the NumPy float32 statement of the depth-map fusion contract (include/jt_render.h: "Depth-map fusion")
-- against an analytic plane and hand-made single observations, on the CPU.  tests/test_gpu_fusion.py holds the kernels to it
bit for bit."""
import numpy as np

from tests import fusion_ref as FR
from tests import mesh_ref as MR

F = np.float32


def test_plane_symbols_exist():
    """the feature under test: the package exposes the fusion entry points this reference states"""
    from joint_tensorf_amd import _lib, mesh_ops
    assert "jt_fusion_integrate" in _lib.SIGNATURES and "jt_fusion_finish" in _lib.SIGNATURES
    for name in ("fusion_state", "fusion_integrate", "fusion_lattice", "mesh_from_fused_lattice"):
        assert name in mesh_ops.__all__


def test_analytic_plane():
    depth, opacity, proj, trunc = FR.plane_scene()
    lo, hi = FR.PLANE_BOX
    acc, count, lattice, seen = FR.fuse(FR.PLANE_SHAPE, depth, opacity, proj, lo, hi, trunc)
    z = FR.coords(FR.PLANE_SHAPE, lo, hi)[2].astype(np.float64)[None, None, :]
    # some points are outside every frame or occluded for every view, most are seen
    assert 0 < int((seen == 0).sum()) < seen.size // 2
    assert (count.max(), count.min()) == (3, 0)
    # points more than trunc below the plane are occluded for every camera: never seen
    assert not seen[:, :, z[0, 0] - FR.PLANE_Z < -trunc].any()
    want = 0.5 * (1 - np.minimum((z - FR.PLANE_Z) / float(F(trunc)), 1.0))
    # e_L of plane_bound(): 0.5 (5 u / T + (V + 1) u + u) < 6 u
    err = np.abs(lattice.astype(np.float64) - want)[seen != 0]
    print("\n[plane] lattice error at most %.2f u" % (err.max() / 2.0 ** -24))
    assert err.max() <= 6 * 2.0 ** -24
    assert (lattice[seen == 0] == 0).all()
    # ---- the extraction and the cell rule ----
    V, T, owner = MR.reference_mesh(lattice, 0.5, lo, hi, return_cells=True)
    keep = FR.keep_triangles(owner, seen)
    assert 0 < keep.sum() < len(T)                                   # the sheets at unseen points are there, and go
    v, t = FR.select(V, T, keep)
    assert len(t) == keep.sum() > 0 and len(v) > 0
    bound = FR.plane_bound()
    dz = np.abs(v[:, 2] - FR.PLANE_Z)
    print("[plane] %d of %d triangles kept, %d vertices, |z - 0.1| at most %.2f u, bound %.0f u"
          % (len(t), len(T), len(v), dz.max() / 2.0 ** -24, bound / 2.0 ** -24))
    assert dz.max() <= bound
    # what was dropped is not on the plane: the rule removed sheets, not surface
    cells = FR.seen_cells(seen).reshape(-1)
    n = FR.PLANE_SHAPE
    flat = (np.arange(n[0] - 1)[:, None, None] * n[1] + np.arange(n[1] - 1)[None, :, None]) * n[2] + np.arange(n[2] - 1)[None, None, :]
    full = np.zeros(n[0] * n[1] * n[2], dtype=bool)
    full[flat.reshape(-1)] = cells
    assert full[owner[keep]].all() and not full[owner[~keep]].any()


# ---- hand cases: the lattice point [0, 0, 0] of a 2 x 2 x 2 lattice sits at `point`; proj = rows (1, 0, 0, 0), (0, 1, 0, 0),
# (0, 0, 0, w): u = x / w, v = y / w and the depth along the axis is w, whatever the point ----------------------------------------
H, W = 3, 4


def _observe(point, w, d=None, a=None, trunc=0.5, min_opacity=0.5, carve=True, near=1e-3, image=None, min_views=1, views=1):
    lo = tuple(float(c) for c in point)
    hi = tuple(c + 8.0 for c in lo)                                   # (the other seven points: outside the frame, or anywhere)
    proj = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, w]], dtype=F)[None].repeat(views, 0)
    depth = np.full((views, H, W), d if d is not None else 1.0, dtype=F) if image is None else np.asarray(image, dtype=F)[None]
    opacity = np.full((views, H, W), 1.0 if a is None else a, dtype=F)
    acc, count, lattice, seen = FR.fuse((2, 2, 2), depth, opacity, proj, lo, hi, trunc, min_opacity, carve, near, min_views)
    return float(acc[0, 0, 0]), int(count[0, 0, 0]), float(lattice[0, 0, 0]), int(seen[0, 0, 0])


def test_behind_and_at_the_near_plane():
    assert _observe((1.5, 1.5, 0.0), -1.0, d=1.0)[:2] == (0.0, 0)                           # behind the camera
    near = F(1e-3)
    assert _observe((0.0, 0.0, 0.0), float(near), d=float(near))[:2] == (0.0, 0)            # w == near: skipped
    acc, count, _, _ = _observe((0.0, 0.0, 0.0), float(np.nextafter(near, F(1))), d=float(near))
    assert count == 1                                                                       # just beyond it: observed


def test_frame_edges_and_nearest_pixel():
    image = np.arange(H * W, dtype=F).reshape(H, W) + F(10)           # every pixel its own depth: 10 + row W + col
    # u == W exactly is outside, the float below it reads the last column; likewise v and H
    assert _observe((float(W), 0.5, 0.0), 1.0, image=image)[1] == 0
    below = float(np.nextafter(F(W), F(0)))
    acc, count, _, _ = _observe((below, 1.5, 0.0), 1.0, image=image, trunc=100.0)
    assert count == 1 and acc == float((image[1, W - 1] - F(1)) / F(100))
    assert _observe((0.5, float(H), 0.0), 1.0, image=image)[1] == 0
    assert _observe((-1e-6, 0.5, 0.0), 1.0, image=image)[1] == 0
    # u = 2.999: column 2, not 3 (no rounding to the nearest integer: centres are at half-integers)
    acc, count, _, _ = _observe((2.999, 0.001, 0.0), 1.0, image=image, trunc=100.0)
    assert count == 1 and acc == float((image[0, 2] - F(1)) / F(100))
    # -0.0 is inside: 0 <= -0
    assert _observe((-0.0, 0.5, 0.0), 1.0, image=image, trunc=100.0)[1] == 1


def test_rays_without_a_surface():
    p = (1.5, 1.5, 0.0)
    for d in (np.nan, np.inf, 0.0, -1.0):
        assert _observe(p, 2.0, d=d)[:2] == (1.0, 1)                                        # carve: seen empty
        assert _observe(p, 2.0, d=d, carve=False)[:2] == (0.0, 0)
    a_below = float(np.nextafter(F(0.5), F(0)))
    assert _observe(p, 2.0, d=2.0, a=a_below)[:2] == (1.0, 1)
    assert _observe(p, 2.0, d=2.0, a=a_below, carve=False)[:2] == (0.0, 0)
    assert _observe(p, 2.0, d=2.0, a=0.5)[:2] == (0.0, 1)                                   # at min_opacity: a surface, s = 0
    assert _observe(p, 2.0, d=2.0, a=np.nan)[:2] == (1.0, 1)                                # a NaN opacity is no surface


def test_truncation():
    p = (1.5, 1.5, 0.0)
    assert _observe(p, 2.0, d=1.5, trunc=0.5)[:3] == (-1.0, 1, 1.0)                         # s == -trunc: kept, t == -1, deep inside
    assert _observe(p, 2.0, d=float(np.nextafter(F(1.5), F(0))), trunc=0.5)[:2] == (0.0, 0)  # the float below: occluded
    assert _observe(p, 2.0, d=2.5, trunc=0.5)[:3] == (1.0, 1, 0.0)                          # s == trunc
    assert _observe(p, 2.0, d=30.0, trunc=0.5)[:3] == (1.0, 1, 0.0)                         # clamped
    assert _observe(p, 2.0, d=2.125, trunc=0.5)[:3] == (0.25, 1, 0.375)


def test_min_views():
    p = (1.5, 1.5, 0.0)
    assert _observe(p, 2.0, d=2.0, min_views=1)[2:] == (0.5, 1)
    assert _observe(p, 2.0, d=2.0, min_views=2)[2:] == (0.0, 0)
    assert _observe(p, 2.0, d=2.125, min_views=2, views=2) == (0.5, 2, 0.375, 1)
    assert _observe(p, -2.0, d=2.0)[2:] == (0.0, 0)                                         # never observed: 0, unseen
