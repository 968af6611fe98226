"""The three simplification entry points (include/jt_render.h: jt_simplify_keys / jt_simplify_clusters / jt_simplify_triangles)
refuse bad arguments before anything launches: no GPU needed."""
import ctypes


def _box(*v):
    return (ctypes.c_float * 3)(*v)


def _cells(*v):
    return (ctypes.c_int * 3)(*v)


def test_simplify_entry_points_refuse_bad_arguments_without_a_gpu():
    """JT_ERR_ARG (1) for a NULL pointer, a count below 1, a cell count outside 1 .. 2^20, hi <= lo, a non-finite box or a bad
    lambda; JT_ERR_UNSUPPORTED (2) at 2^31 vertices or triangle corners.  Nothing here reaches a kernel."""
    from joint_tensorf_amd import _lib
    L, p = _lib.lib, 64                     # p: a non-NULL pointer that is never dereferenced on these paths
    lo, hi, cells = _box(0, 0, 0), _box(1, 1, 1), _cells(4, 4, 4)
    inf, nan, big = float("inf"), float("nan"), 3.0e38
    # ---- keys ----
    assert L.jt_simplify_keys(None, 8, lo, hi, cells, p, None) == 1
    assert L.jt_simplify_keys(p, 8, None, hi, cells, p, None) == 1
    assert L.jt_simplify_keys(p, 8, lo, None, cells, p, None) == 1
    assert L.jt_simplify_keys(p, 8, lo, hi, None, p, None) == 1
    assert L.jt_simplify_keys(p, 8, lo, hi, cells, None, None) == 1
    assert L.jt_simplify_keys(p, 0, lo, hi, cells, p, None) == 1
    assert L.jt_simplify_keys(p, 8, lo, hi, _cells(4, 0, 4), p, None) == 1
    assert L.jt_simplify_keys(p, 8, lo, hi, _cells(4, 4, (1 << 20) + 1), p, None) == 1
    assert L.jt_simplify_keys(p, 8, lo, _box(1, 0, 1), cells, p, None) == 1               # hi == lo on an axis
    assert L.jt_simplify_keys(p, 8, lo, _box(1, -1, 1), cells, p, None) == 1
    assert L.jt_simplify_keys(p, 8, lo, _box(1, inf, 1), cells, p, None) == 1
    assert L.jt_simplify_keys(p, 8, _box(nan, 0, 0), hi, cells, p, None) == 1
    assert L.jt_simplify_keys(p, 8, _box(-big, 0, 0), _box(big, 1, 1), cells, p, None) == 1   # the fp32 extent overflows
    assert L.jt_simplify_keys(p, 1 << 31, lo, hi, cells, p, None) == 2
    assert L.jt_simplify_keys(None, 1 << 31, lo, hi, cells, p, None) == 1                 # argument errors come first
    # ---- clusters ----
    ok = [p, p, 8, p, p, 2, 0.0625, p, p, p, None]
    for i in (0, 1, 3, 4, 7, 8, 9):
        bad = list(ok)
        bad[i] = None
        assert L.jt_simplify_clusters(*bad) == 1, i
    assert L.jt_simplify_clusters(p, p, 0, p, p, 2, 0.0625, p, p, p, None) == 1
    assert L.jt_simplify_clusters(p, p, 8, p, p, 0, 0.0625, p, p, p, None) == 1
    assert L.jt_simplify_clusters(p, p, 8, p, p, 9, 0.0625, p, p, p, None) == 1            # more clusters than vertices
    for lam in (0.0, -1.0, inf, nan):
        assert L.jt_simplify_clusters(p, p, 8, p, p, 2, lam, p, p, p, None) == 1, lam
    assert L.jt_simplify_clusters(p, p, 1 << 31, p, p, 2, 0.0625, p, p, p, None) == 2
    # ---- triangles ----
    ok = [p, 8, p, 8, 2, p, p, p, p, None]
    for i in (0, 2, 5, 6, 7, 8):
        bad = list(ok)
        bad[i] = None
        assert L.jt_simplify_triangles(*bad) == 1, i
    assert L.jt_simplify_triangles(p, 0, p, 8, 2, p, p, p, p, None) == 1
    assert L.jt_simplify_triangles(p, 8, p, 0, 2, p, p, p, p, None) == 1
    assert L.jt_simplify_triangles(p, 8, p, 8, 0, p, p, p, p, None) == 1
    assert L.jt_simplify_triangles(p, 8, p, 8, 9, p, p, p, p, None) == 1
    assert L.jt_simplify_triangles(p, 8, p, 1 << 31, 2, p, p, p, p, None) == 2
    assert L.jt_simplify_triangles(p, 715827883, p, 8, 2, p, p, p, p, None) == 2           # ceil(2^31 / 3) triangles
    assert L.jt_simplify_triangles(p, 715827882, None, 8, 2, p, p, p, p, None) == 1


def test_ops_refuses_bad_shapes_before_any_launch():
    import pytest
    import torch
    from joint_tensorf_amd import ops
    V, T, N = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    box = ((0, 0, 0), (1, 1, 1))
    for args in ((V[:, :2], T, N, *box, 2), (V, T.long(), N, *box, 2), (V, T, N[:3], *box, 2), (V, T, None, *box, 2),
                 (V, T, N, (0, 0), (1, 1, 1), 2), (V, T, N, *box, 0), (V, T, N, *box, (2, 2)), (V, T, N, *box, (1 << 20) + 1),
                 (V, T, N, *box, 2.5), (V, T, N, *box, True)):
        with pytest.raises(ValueError):
            ops.simplify_mesh(*args)
    for lam in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.simplify_mesh(V, T, N, *box, 2, regular=lam)
    assert ops.simplify_cells(3) == [3, 3, 3] and ops.simplify_cells((1, 2, 1 << 20)) == [1, 2, 1 << 20]
    out = ops.simplify_mesh(V[:0], T, N[:0], *box, 2)                                      # an empty mesh: nothing launched
    assert [tuple(o.shape) for o in out[:4]] == [(0, 3), (0, 3), (0, 3), (0,)] and out[4] == (0, 0)
