"""tests/visible_ref.py, the NumPy statement of csrc/jt_visible.hip, on cases small enough to work out by hand, and the
nested-cube scene of tests/test_gpu_visible.py through tests/raster_ref.py: what the GPU test expects of it is established here,
without a GPU."""
import numpy as np

from tests import raster_ref as R
from tests import visible_ref as VR


def test_tally_by_hand():
    tri = np.array([[[0, 0, 1], [-1, 2, 2]], [[2, 2, 2], [2, 5, -1]]])            # two views of 2 x 3; 5 is no triangle of 3
    views, pixels = VR.tally(tri, 3)
    assert views.dtype == np.int32 and pixels.dtype == np.int64
    assert views.tolist() == [1, 1, 2] and pixels.tolist() == [2, 1, 6]
    assert VR.tally(tri, 3, min_pixels=2)[0].tolist() == [1, 0, 2]                # exactly min_pixels counts
    assert VR.tally(tri, 3, min_pixels=3)[0].tolist() == [0, 0, 1]
    assert VR.tally(tri, 3, min_pixels=5)[0].tolist() == [0, 0, 0]
    assert VR.tally(tri, 3, min_pixels=5)[1].tolist() == [2, 1, 6]                # the pixel sums do not depend on it
    views, pixels = VR.tally(np.full((2, 3, 3), -1), 4)
    assert not views.any() and not pixels.any()
    # slabs of views compose
    a, b = VR.tally(tri[:1], 3), VR.tally(tri[1:], 3)
    assert (a[0] + b[0]).tolist() == [1, 1, 2] and (a[1] + b[1]).tolist() == [2, 1, 6]


def test_grow_on_a_strip():
    nv, T = VR.strip(10)
    seed = np.zeros(len(T), dtype=np.uint8)
    seed[0] = 1
    assert VR.grow(T, nv, seed, 0).tolist() == seed.tolist()
    # triangle k = (k, k + 1, k + 2) shares a vertex with k - 2 .. k + 2: a ring reaches two triangles further
    assert VR.grow(T, nv, seed, 1).tolist() == [1, 1, 1] + [0] * 7 + [0, 0]
    assert VR.grow(T, nv, seed, 2).tolist() == [1, 1, 1, 1, 1] + [0] * 5 + [0, 0]
    assert VR.grow(T, nv, seed, 20).tolist() == [1] * 10 + [0, 0]                 # the two bad triangles never enter
    # a bad triangle that IS in the input set stays (its bits are the caller's) but flags nothing
    bad = np.zeros(len(T), dtype=np.uint8)
    bad[10] = 1
    assert VR.grow(T, nv, bad, 3).tolist() == bad.tolist()
    assert VR.grow(T, nv, np.uint8([0, 0, 0, 0, 0, 7, 0, 0, 0, 0, 0, 0]), 1).tolist() == [0, 0, 0, 1, 1, 7, 1, 1, 0, 0, 0, 0]


def test_select_by_hand():
    V = np.arange(18, dtype=np.float32).reshape(6, 3)
    N, C = V + 100, V + 200
    T = np.int32([[0, 1, 2], [2, 3, 4], [3, 4, 5], [0, 5, 6], [1, 1, 4]])         # triangle 3 names a vertex out of range
    v, t, n, c, dropped = VR.select(V, T, [1, 0, 1, 1, 0], N, C)
    assert dropped == 3 and t.dtype == np.int32
    assert v.tolist() == V[[0, 1, 2, 3, 4, 5]].tolist() and t.tolist() == [[0, 1, 2], [3, 4, 5]]
    v, t, n, c, dropped = VR.select(V, T, [0, 0, 1, 0, 1], N, C)
    assert dropped == 3 and v.tolist() == V[[1, 3, 4, 5]].tolist() and t.tolist() == [[1, 2, 3], [0, 0, 2]]
    assert n.tolist() == N[[1, 3, 4, 5]].tolist() and c.tolist() == C[[1, 3, 4, 5]].tolist()
    v, t, n, c, dropped = VR.select(V, T[:3], [1, 1, 1])
    assert dropped == 0 and n is None and c is None and v.tobytes() == V.tobytes() and t.tobytes() == T[:3].tobytes()
    v, t, n, c, dropped = VR.select(V, T, [0] * 5, N)
    assert v.shape == (0, 3) and t.shape == (0, 3) and n.shape == (0, 3) and c is None and dropped == 5


def test_look_at_is_the_rasteriser_tests_construction():
    from tests.test_gpu_raster import _look_at
    for eye in VR.CUBE_EYES:
        want = _look_at(eye, (0.0, 0.0, 0.0), VR.CUBE_FOCAL, VR.CUBE_H, VR.CUBE_W)[0]
        assert VR.look_at(eye, (0.0, 0.0, 0.0), VR.CUBE_FOCAL, VR.CUBE_H, VR.CUBE_W).tobytes() == want.tobytes()


def test_nested_cubes_through_the_reference_rasteriser():
    """what tests/test_gpu_visible.py relies on: all 24 triangles are drawn in every view, every outer triangle wins between 21
    and 93 pixels in exactly two views, no inner triangle wins one, and no pixel is a near tie -- so the device's fp32 depth
    cannot pick another winner than fp64 does"""
    V, T = VR.nested_cubes()
    assert V.shape == (16, 3) and T.shape == (24, 3) and T[:12].max() == 7 and T[12:].min() == 8
    H, W = VR.CUBE_H, VR.CUBE_W
    assert (H * W) % 64 != 0
    screens = R.project(V, VR.cube_views())
    tri = []
    for s in screens:
        ref = R.rasterize(s, T, H, W)
        assert (ref["status"] == R.DRAWN).all()
        assert not R.near_ties(ref).any()
        tri.append(ref["tri"])
    tri = np.stack(tri)
    views, pixels = VR.tally(tri, 24)
    assert views.tolist() == [2] * 12 + [0] * 12 and not pixels[12:].any()
    per_view = np.stack([VR.tally(tri[v:v + 1], 24)[1] for v in range(4)])
    won = per_view[:, :12][per_view[:, :12] > 0]
    assert len(won) == 24 and won.min() == 21 and won.max() == 93
    assert VR.tally(tri, 24, min_pixels=21)[0].tolist() == views.tolist()
    assert VR.tally(tri, 24, min_pixels=94)[0].tolist() == [0] * 24
    (v, t, _, _, dropped), seen, kept = VR.visible_mesh(tri, V, T, min_views=1, rings=1)
    assert seen.tolist() == kept.tolist() == [1] * 12 + [0] * 12                  # the cubes share no vertex: a ring adds nothing
    assert dropped == 12 and v.tobytes() == V[:8].tobytes() and t.tobytes() == T[:12].tobytes()
    (v, t, _, _, dropped), seen, kept = VR.visible_mesh(tri, V, T, min_views=3)
    assert dropped == 24 and v.shape == (0, 3) and t.shape == (0, 3)
