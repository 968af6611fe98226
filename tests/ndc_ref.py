"""The contract of the NDC un-warp (include/jt_render.h: "NDC meshes in world space") in NumPy fp64: the forward map of the ray
generator, its inverse, the normal transform, the vertex status and the triangle filter.  Nothing here is shared with the product.

    forward:  xn = sx x / z,  yn = sy y / z,  zn = 1 - 2 n / z
    inverse:  u = 1 - zn,  z = 2 n / u,  x = xn z / sx,  y = yn z / sy          (u > 0)
    normals:  (sx nx, sy ny, u nz - xn nx - yn ny), normalised; (0, 0, 0) stays (0, 0, 0)
    status:   1 (beyond) for a non-finite coordinate, u <= 0 or a non-finite result; else 2 (far) for max_depth > 0 and z > max_depth;
              else 0 (kept).  A vertex that is not kept is all zeros.
    filter:   a triangle is kept iff its three ids are in range and their statuses 0; a dropped one counts once, as beyond when an id
              is out of range or a vertex is beyond, else as far."""
import numpy as np

KEPT, BEYOND, FAR = 0, 1, 2


def forward(p, sx, sy, near):
    p = np.asarray(p, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([sx * x / z, sy * y / z, 1.0 - 2.0 * near / z], -1)


def inverse(q, sx, sy, near):
    """world points of NDC points q [..., 3]; u <= 0 gives what the arithmetic gives (inf, nan, negative z): see status"""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = 1.0 - q[..., 2]
        z = 2.0 * near / u
        return np.stack([q[..., 0] * z / sx, q[..., 1] * z / sy, z], -1)


def normal_to_world(q, normals, sx, sy):
    """J^T of the forward map applied to NDC normals at NDC points q, scaled by the positive z, then normalised"""
    q, n = np.asarray(q, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    v = np.stack([sx * n[..., 0], sy * n[..., 1], (1.0 - q[..., 2]) * n[..., 2] - q[..., 0] * n[..., 0] - q[..., 1] * n[..., 1]], -1)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((v * v).sum(-1, keepdims=True))
    ok = np.isfinite(length) & (length > 0)
    return np.where(ok, v / np.where(ok, length, 1.0), 0.0)


def status(q, sx, sy, near, max_depth=None):
    q = np.asarray(q, dtype=np.float64)
    w = inverse(q, sx, sy, near)
    with np.errstate(invalid="ignore"):
        beyond = ~np.isfinite(q).all(-1) | ~(1.0 - q[..., 2] > 0) | ~np.isfinite(w).all(-1)
        far = np.zeros_like(beyond) if max_depth is None or not max_depth > 0 else w[..., 2] > max_depth
    return np.where(beyond, BEYOND, np.where(far, FAR, KEPT)).astype(np.uint8)


def unwarp(q, sx, sy, near, normals=None, max_depth=None):
    """(world [n, 3] fp64, world normals [n, 3] fp64 or None, status [n] uint8) with zeros where a vertex is not kept"""
    st = status(q, sx, sy, near, max_depth)
    kept = (st == KEPT)[..., None]
    with np.errstate(invalid="ignore"):
        world = np.where(kept, inverse(q, sx, sy, near), 0.0)
        nrm = None if normals is None else np.where(kept, normal_to_world(q, normals, sx, sy), 0.0)
    return world, nrm, st


def filter_triangles(triangles, st, n_vertices=None):
    """(keep [nt] bool, cause [nt] uint8: 0 kept, 1 beyond, 2 far) of triangles [nt, 3] under vertex statuses st [nv]"""
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    st = np.asarray(st)
    nv = len(st) if n_vertices is None else int(n_vertices)
    in_range = (T >= 0) & (T < nv)
    s = np.where(in_range, st[np.clip(T, 0, max(nv - 1, 0))], BEYOND)
    beyond = (s == BEYOND).any(-1)
    far = (s == FAR).any(-1) & ~beyond
    keep = ~beyond & ~far
    return keep, np.where(keep, KEPT, np.where(beyond, BEYOND, FAR)).astype(np.uint8)


def compact(vertices, triangles, st, normals=None, colors=None):
    """(vertices', triangles' int32, normals' or None, colors' or None, (n_dropped_beyond, n_dropped_far)): kept triangles in their
    order with remapped ids, the vertices they name in their order"""
    V, T = np.asarray(vertices), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    keep, cause = filter_triangles(T, st, len(V))
    used = np.zeros(len(V), dtype=bool)
    used[T[keep].reshape(-1)] = True
    remap = np.cumsum(used) - 1
    pick = (lambda a: None if a is None else np.asarray(a)[used])
    return (V[used], remap[T[keep]].astype(np.int32).reshape(-1, 3), pick(normals), pick(colors),
            (int((cause == BEYOND).sum()), int((cause == FAR).sum())))
