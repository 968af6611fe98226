"""The contract of csrc/jt_raster.hip in NumPy: int64 edge functions with the top-left rule, fp64 for q, depth and attributes.

A `screen` array is [nv, 4] = (x, y, 1/w, w) of ONE view, as jt_raster_project writes it.  x is the column, y the row; the pixel of
column i and row j has its centre at (i + 0.5, j + 0.5).  The GPU tests hand the kernel's own fp32 `screen` to `rasterize`, so
the projection's rounding cannot move a snap; `project` is the fp64 statement of that first step."""
import numpy as np

SUB = 256                      # sub-pixels per pixel
GUARD = 1 << 22                # |snapped coordinate| beyond this drops the triangle
DRAWN, NEAR, GUARD_BAND, EMPTY, CULLED = range(5)
ORTHO = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.float32)      # (x, y) = (vx, vy), w = 1, exactly
PERSP = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)      # (x, y) = (vx, vy) / vz, w = vz


def project(vertices, proj, near=1e-3):
    """fp64 `screen` [V, nv, 4] of fp32 vertices [nv, 3] under fp32 proj [V, 3, 4]; 1/w = 0 (and x = y = 0) for a non-finite vertex
    or w < near"""
    v = np.asarray(vertices, dtype=np.float64)
    P = np.asarray(proj, dtype=np.float64).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        h = np.einsum("vrc,nc->vnr", P[:, :, :3], v) + P[:, None, :, 3]
        w = h[..., 2]
        ok = np.isfinite(v).all(-1)[None] & (w >= near)
        out = np.zeros(h.shape[:2] + (4,))
        out[..., 3] = w
        safe = np.where(ok, w, 1.0)
        out[..., 0] = np.where(ok, h[..., 0] / safe, 0.0)
        out[..., 1] = np.where(ok, h[..., 1] / safe, 0.0)
        out[..., 2] = np.where(ok, 1.0 / safe, 0.0)
    return out


def snap(screen):
    """(X, Y int64 sub-pixel coordinates, inside: within the guard band) of a screen array; the snap is rintf(x * 256) in fp32"""
    with np.errstate(all="ignore"):
        f = np.rint(np.asarray(screen, dtype=np.float32)[..., :2] * np.float32(SUB))
        inside = (np.abs(f) <= GUARD).all(-1)                  # False for a NaN
        xy = np.where(inside[..., None], f, 0).astype(np.int64)
    return xy[..., 0], xy[..., 1], inside


def edge_values(X, Y, tri, px, py):
    """int64 edge values b[3] (b[k] weighs vertex k; inside-positive after orientation) at the centres of pixels (px, py), the
    signed area and the top-left biases: (b [3, ...], area, bias [3])"""
    x = [int(X[k]) for k in tri]
    y = [int(Y[k]) for k in tri]
    area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    sign = 1 if area > 0 else -1
    cx = SUB * np.asarray(px, dtype=np.int64) + SUB // 2
    cy = SUB * np.asarray(py, dtype=np.int64) + SUB // 2
    b, bias = [], []
    for k in range(3):
        u, v = (k + 1) % 3, (k + 2) % 3
        dx, dy = sign * (x[v] - x[u]), sign * (y[v] - y[u])
        b.append(sign * ((x[v] - x[u]) * (cy - y[u]) - (y[v] - y[u]) * (cx - x[u])))
        bias.append(0 if (dy < 0 or (dy == 0 and dx > 0)) else 1)      # a left edge points up the screen, a top edge right
    return np.stack(b), area, bias


def triangle_status(X, Y, inside, q, tri, cull):
    i = [int(k) for k in tri]
    if not all(0 <= k < len(X) for k in i) or not all(q[k] > 0 and np.isfinite(q[k]) for k in i):
        return NEAR
    if not all(inside[k] for k in i):
        return GUARD_BAND
    area = (X[i[1]] - X[i[0]]) * (Y[i[2]] - Y[i[0]]) - (Y[i[1]] - Y[i[0]]) * (X[i[2]] - X[i[0]])
    if area == 0:
        return EMPTY
    if cull and area > 0:
        return CULLED
    return DRAWN


def rasterize(screen, triangles, H, W, cull=False, attrs=None, background=0.0, snapped=None):
    """One view.  Returns a dict: tri [H, W] int64 (-1: none; largest q wins, the lower index at equal q), q [H, W] fp64 (0: none),
    second [H, W] fp64: the runner-up's q (0: no second triangle covers the pixel), cover [H, W]: how many drawn triangles cover
    it, status [nt], depth [H, W] (1 / q, inf: none) and out [H, W, C] fp64 when attrs [nv, C] are given.  snapped = (X, Y):
    the sub-pixel integers themselves instead of the snap of screen's x and y (screen then gives 1/w only)."""
    screen = np.asarray(screen)
    X, Y, inside = snap(screen)
    if snapped is not None:
        X, Y = (np.asarray(a, dtype=np.int64) for a in snapped)
        inside = (np.abs(X) <= GUARD) & (np.abs(Y) <= GUARD)
    q = screen[:, 2].astype(np.float64)
    nt = len(triangles)
    win = np.full((H, W), -1, dtype=np.int64)
    best, second = np.zeros((H, W)), np.zeros((H, W))
    cover = np.zeros((H, W), dtype=np.int64)
    status = np.zeros(nt, dtype=np.uint8)
    C = 0 if attrs is None else np.asarray(attrs).shape[1]
    out = np.empty((H, W, C))
    out[:] = np.broadcast_to(np.asarray(background, dtype=np.float64), (C,)) if C else 0
    for t in range(nt):
        tri = [int(k) for k in triangles[t]]
        status[t] = triangle_status(X, Y, inside, q, tri, cull)
        if status[t] != DRAWN:
            continue
        xs, ys = [int(X[k]) for k in tri], [int(Y[k]) for k in tri]
        x0, x1 = max(-((SUB // 2 - min(xs)) // SUB), 0), min((max(xs) - SUB // 2) // SUB, W - 1)
        y0, y1 = max(-((SUB // 2 - min(ys)) // SUB), 0), min((max(ys) - SUB // 2) // SUB, H - 1)
        if x1 < x0 or y1 < y0:
            continue
        py, px = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        b, area, bias = edge_values(X, Y, tri, px, py)
        hit = (b[0] >= bias[0]) & (b[1] >= bias[1]) & (b[2] >= bias[2])
        bq = [b[k].astype(np.float64) * q[tri[k]] for k in range(3)]
        qq = (bq[0] + bq[1] + bq[2]) / b.sum(0).astype(np.float64)
        sub = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        cover[sub] += hit
        wins = hit & (qq > best[sub])                         # strictly: an earlier (lower) index keeps an equal q
        second[sub] = np.where(wins, best[sub], np.where(hit, np.maximum(second[sub], qq), second[sub]))
        best[sub] = np.where(wins, qq, best[sub])
        win[sub] = np.where(wins, t, win[sub])
        if C:
            a = np.asarray(attrs, dtype=np.float64)
            val = sum(bq[k][..., None] * a[tri[k]] for k in range(3)) / (bq[0] + bq[1] + bq[2])[..., None]
            out[sub] = np.where(wins[..., None], val, out[sub])
    with np.errstate(divide="ignore"):
        depth = np.where(win >= 0, 1.0 / np.where(win >= 0, best, 1.0), np.inf)
    res = dict(tri=win, q=best, second=second, cover=cover, status=status, depth=depth)
    if C:
        res["out"] = out
    return res


def near_ties(ref, rel=1e-5):
    """pixels where the winner and the runner-up lie within `rel` of each other: where fp32 may pick the other one"""
    return (ref["second"] > 0) & (ref["q"] - ref["second"] < rel * ref["q"])


# ---- the scenes of tests/test_gpu_raster.py (and of the near-tie cap in tests/test_raster_ref.py) ---------------------------
def lift(points):
    """vertices [n, 3] fp32 for PERSP from rows (x, y, w): (x w, y w, w)"""
    p = np.asarray(points, dtype=np.float64)
    return np.stack([p[:, 0] * p[:, 2], p[:, 1] * p[:, 2], p[:, 2]], -1).astype(np.float32)


def flat(points, z=0.0):
    """vertices [n, 3] fp32 for ORTHO from rows (x, y)"""
    p = np.asarray(points, dtype=np.float32)
    return np.concatenate([p, np.full((len(p), 1), z, dtype=np.float32)], -1)


FAN_CENTRE = (16.5, 16.5)       # exactly a pixel centre of the 32 x 32 image


def fan_scene():
    ring = [(27.25, 15.0), (25.0, 25.5), (16.5, 29.0), (6.0, 24.75), (3.5, 16.5), (7.75, 6.25), (17.0, 3.0), (26.0, 7.5)]
    V = flat([FAN_CENTRE] + ring)
    T = np.array([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)], dtype=np.int32)
    return dict(vertices=V, triangles=T, proj=ORTHO, H=32, W=32)


def one_triangle_scene():
    return dict(vertices=flat([(2.3, 1.7), (13.1, 5.2), (4.9, 14.6)]), triangles=np.array([[0, 1, 2]], dtype=np.int32),
                proj=ORTHO, H=16, W=16)


def big_triangle_scene():
    """every vertex off the 24 x 40 image and inside the guard band; the image is covered in part"""
    return dict(vertices=flat([(-30.0, 10.0), (100.0, -10.0), (10.0, 120.0)]), triangles=np.array([[0, 1, 2]], dtype=np.int32),
                proj=ORTHO, H=24, W=40)


def mixed_scene(seed=0, n=130, big=(5, 70)):
    """130 triangles in 32 x 32: two cover the screen, the rest are sub-pixel to 6 pixels across; triangle t lies at constant
    depth w = 2 + 0.01 t, so neighbours in depth differ by 0.3 % in q and more"""
    g = np.random.default_rng(seed)
    pts, T = [], []
    for t in range(n):
        w = 2.0 + 0.01 * t
        if t in big:
            xy = np.array([(-40.0, -45.0), (110.0, -38.0), (-42.0, 105.0)]) + (3.0 if t == big[1] else 0.0)
            if t == big[1]:
                xy = xy[::-1]                                 # the other winding
        else:
            size = 0.3 + 5.7 * g.random()
            xy = 1.0 + 30.0 * g.random(2) + size * (g.random((3, 2)) - 0.5)
        T.append([len(pts), len(pts) + 1, len(pts) + 2])
        pts += [(x, y, w) for x, y in xy]
    return dict(vertices=lift(pts), triangles=np.array(T, dtype=np.int32), proj=PERSP, H=32, W=32)


def layers_scene():
    """two parallel layers, two triangles each: the nearer one (w = 2, submitted second) hides part of the farther (w = 3)"""
    far = [(2.2, 3.1, 3.0), (20.7, 2.4, 3.0), (21.3, 19.8, 3.0), (1.6, 20.5, 3.0)]
    near = [(9.4, 8.3, 2.0), (23.1, 9.9, 2.0), (22.2, 23.6, 2.0), (8.7, 22.1, 2.0)]
    return dict(vertices=lift(far + near), triangles=np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.int32),
                proj=PERSP, H=24, W=24)


def duplicate_scene():
    """one triangle, tilted in depth, submitted twice: once with shared vertex ids, once with a copy of the vertices"""
    tri = [(3.3, 2.1, 1.5), (28.6, 9.4, 2.5), (9.2, 27.7, 4.0)]
    return dict(vertices=lift(tri + tri), triangles=np.array([[0, 1, 2], [0, 1, 2], [3, 4, 5]], dtype=np.int32), proj=PERSP,
                H=32, W=32)


def crossing_scene():
    """two triangles through each other: one recedes to the right, the other to the left"""
    a = [(2.3, 3.9, 1.2), (29.1, 14.2, 3.4), (3.8, 28.4, 1.3)]
    b = [(28.7, 2.6, 1.1), (30.2, 29.3, 1.25), (1.9, 16.3, 3.7)]
    return dict(vertices=lift(a + b), triangles=np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32), proj=PERSP, H=32, W=32)


COVERAGE_SCENES = dict(one=one_triangle_scene, fan=fan_scene, big=big_triangle_scene, mixed=mixed_scene)
DEPTH_SCENES = dict(layers=layers_scene, duplicate=duplicate_scene, crossing=crossing_scene)
MAX_NEAR_TIES = 4
