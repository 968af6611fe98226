"""The contract of csrc/jt_visible.hip in NumPy (include/jt_render.h: "Visible surface"): integers only, so every comparison with
the device is exact.

The tally's input is a WINNER buffer tri [V, H, W] (the nearest triangle per pixel, -1 where none): in the GPU tests the device's
own, ops.rasterize(...).tri -- tests/test_gpu_raster.py::test_depth_order tolerates up to four near-tie pixels between the NumPy
rasteriser and the device, so a rasteriser restatement would not isolate the new kernels.  The CPU tests feed it
tests/raster_ref.py's winners."""
import numpy as np


def tally(tri, nt, min_pixels=1):
    """(views [nt] int32: the views in which the triangle wins at least min_pixels pixels, pixels [nt] int64: the pixels it wins
    over all views) of tri [V, H, W]; an entry outside [0, nt) is no winner"""
    tri = np.asarray(tri).astype(np.int64)
    views = np.zeros(nt, dtype=np.int32)
    pixels = np.zeros(nt, dtype=np.int64)
    for v in range(tri.shape[0]):
        w = tri[v].ravel()
        w = w[(w >= 0) & (w < nt)]
        count = np.bincount(w, minlength=nt).astype(np.int64)
        views += (count >= min_pixels).astype(np.int32)
        pixels += count
    return views, pixels


def in_range(triangles, nv):
    """[nt] bool: the three ids lie in [0, nv)"""
    t = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < nv)).all(axis=1)


def grow(triangles, nv, visible, rings):
    """visible [nt] uint8 grown by `rings` rings of vertex neighbours: per ring, flag the vertices of the triangles of the set
    whose ids are in range, then visible | (ids in range and a flag on one of them).  rings = 0: the input's bits."""
    t = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    ok = in_range(t, nv)
    cur = np.array(visible, dtype=np.uint8)
    for _ in range(int(rings)):
        flag = np.zeros(nv, dtype=bool)
        flag[t[ok & (cur != 0)].ravel()] = True
        touched = np.zeros(len(t), dtype=bool)
        touched[ok] = flag[t[ok]].any(axis=1)
        cur = cur | touched.astype(np.uint8)
    return cur


def select(vertices, triangles, keep, normals=None, colors=None):
    """(vertices', triangles' int32 with remapped ids, normals' or None, colors' or None, n_dropped): the triangles with keep != 0
    and ids in range, in order, and the vertices they name, in order; empty results are [0, 3]"""
    V = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    k = (np.asarray(keep).reshape(-1) != 0) & in_range(t, len(V))
    used = np.zeros(len(V), dtype=bool)
    used[t[k].ravel()] = True
    remap = np.cumsum(used) - 1
    T = remap[t[k]].astype(np.int32).reshape(-1, 3)

    def rows(a):
        return None if a is None else np.asarray(a, dtype=np.float32).reshape(-1, 3)[used]
    return V[used], T, rows(normals), rows(colors), int(len(t) - k.sum())


def visible_mesh(tri, vertices, triangles, min_views=1, min_pixels=1, rings=1, normals=None, colors=None):
    """the whole rule on a winner buffer: seen = views >= min_views, kept = grow(seen, rings), select(kept); returns (select's
    result, seen, kept)"""
    views, _ = tally(tri, len(triangles), min_pixels)
    seen = (views >= min_views).astype(np.uint8)
    kept = grow(triangles, len(vertices), seen, rings)
    return select(vertices, triangles, kept, normals, colors), seen, kept


# ---- the nested-cube scene of tests/test_visible_ref.py and tests/test_gpu_visible.py -----------------------------------------
CUBE_EYES = ((3.1, 2.2, 1.7), (-2.9, -2.4, 1.9), (2.3, -3.0, -2.1), (-2.2, 3.1, -1.8))
CUBE_FOCAL, CUBE_H, CUBE_W = 28.0, 33, 70


def cube(half, first=0):
    """(vertices [8, 3] fp32, triangles [12, 3] int32 wound so that the right-hand normal points outwards) of the cube
    [-half, half]^3; vertex i = (x, y, z) bits (i >> 2, i >> 1, i) & 1"""
    V = np.array([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)], dtype=np.float32) * (2 * half) - half
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]     # -x +x -y +y -z +z
    T = []
    for a, b, c, d in quads:
        T += [(a, b, c), (a, c, d)]
    T = np.array(T, dtype=np.int32)
    n = np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
    assert (np.einsum("ij,ij->i", n, V[T].mean(1)) > 0).all()                # outward
    return V, T + first


def nested_cubes():
    """an outer cube of half-size 1 and an inner one of half-size 0.5, 12 outward-wound triangles each, outer first"""
    Vo, To = cube(1.0)
    Vi, Ti = cube(0.5, first=8)
    return np.concatenate([Vo, Vi]), np.concatenate([To, Ti])


def look_at(eye, target, focal, H, W):
    """proj [3, 4] fp32 of a camera at `eye` looking at `target`, x right, y down, z forward: the construction of
    tests/test_gpu_raster.py::_look_at"""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]])
    return (K @ np.concatenate([Rm, -(Rm @ eye)[:, None]], 1)).astype(np.float32)


def cube_views():
    return np.stack([look_at(e, (0.0, 0.0, 0.0), CUBE_FOCAL, CUBE_H, CUBE_W) for e in CUBE_EYES])


def strip(n=10):
    """(nv, triangles [n + 2, 3] int32): a strip of n triangles sharing edges -- triangle k = (k, k + 1, k + 2) -- plus one
    triangle with an id of -1 and one with an id of nv"""
    nv = n + 2
    T = [[k, k + 1, k + 2] for k in range(n)] + [[0, 1, -1], [1, 2, nv]]
    return nv, np.array(T, dtype=np.int32)
