"""The depth-map fusion contract of include/jt_render.h (jt_fusion_integrate / jt_fusion_finish) and the cell rule of
mesh_ops.mesh_from_fused_lattice, written out in NumPy float32, operation by operation in the order the header states: every
NumPy float32 operation is rounded on its own, as every operation of the kernels is, so the kernels have to reproduce these
bits.  Nothing here is shared with the kernels.  The scenes of the CPU and the GPU tests live here too, so both use the same."""
import numpy as np

F = np.float32


def coords(shape, lo, hi):
    """per axis the fp32 lattice positions P(i) = lo (1 - s) + hi s, s = float(i) / float(n - 1): jt_mesh_emit's"""
    out = []
    for a in range(3):
        s = np.arange(shape[a]).astype(F) / F(shape[a] - 1)
        out.append(F(lo[a]) * (F(1) - s) + F(hi[a]) * s)
    return out


def integrate(acc, count, depth, opacity, proj, lo, hi, trunc, min_opacity=0.5, carve=True, near=1e-3):
    """the views of depth / opacity [V, H, W] fp32 under proj [V, 3, 4] fp32, in ascending order, added into acc fp32 / count int32
    [nx, ny, nz] (updated in place and returned)"""
    assert acc.dtype == F and count.dtype == np.int32 and acc.shape == count.shape
    depth, opacity, proj = np.asarray(depth, dtype=F), np.asarray(opacity, dtype=F), np.asarray(proj, dtype=F)
    V, H, W = depth.shape
    trunc, min_opacity, near = F(trunc), F(min_opacity), F(near)
    ax = coords(acc.shape, lo, hi)
    x, y, z = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
    with np.errstate(all="ignore"):
        for view in range(V):
            p = proj[view]
            xw = ((p[0, 0] * x + p[0, 1] * y) + p[0, 2] * z) + p[0, 3]
            yw = ((p[1, 0] * x + p[1, 1] * y) + p[1, 2] * z) + p[1, 3]
            w = ((p[2, 0] * x + p[2, 1] * y) + p[2, 2] * z) + p[2, 3]
            xw, yw, w = (np.broadcast_to(a, acc.shape).astype(F) for a in (xw, yw, w))
            u, v = xw / w, yw / w
            frame = (w > near) & (u >= F(0)) & (u < F(W)) & (v >= F(0)) & (v < F(H))          # a NaN fails every test
            col = np.where(frame, u, F(0)).astype(np.int64)                                    # (int)u: towards zero
            row = np.where(frame, v, F(0)).astype(np.int64)
            d, a = depth[view][row, col], opacity[view][row, col]
            surface = np.isfinite(d) & (d > F(0)) & (a >= min_opacity)
            s = d - w
            t = s / trunc
            t = np.where(t > F(1), F(1), t)
            add_t = frame & surface & ~(s < -trunc)
            add_1 = frame & ~surface & bool(carve)
            acc[...] = np.where(add_t, acc + t, np.where(add_1, acc + F(1), acc))
            count[...] = count + (add_t | add_1).astype(np.int32)
    return acc, count


def state(shape):
    return np.zeros(shape, dtype=F), np.zeros(shape, dtype=np.int32)


def finish(acc, count, min_views=1):
    """(lattice fp32, seen uint8)"""
    ok = count >= min_views
    with np.errstate(all="ignore"):
        lattice = np.where(ok, F(0.5) * (F(1) - acc / count.astype(F)), F(0)).astype(F)
    return lattice, ok.astype(np.uint8)


def fuse(shape, depth, opacity, proj, lo, hi, trunc, min_opacity=0.5, carve=True, near=1e-3, min_views=1):
    acc, count = integrate(*state(shape), depth, opacity, proj, lo, hi, trunc, min_opacity, carve, near)
    return (acc, count) + finish(acc, count, min_views)


def seen_cells(seen):
    """bool [nx - 1, ny - 1, nz - 1]: the cells whose eight corners are all seen, indexed by their minimum corner"""
    s = np.asarray(seen) != 0
    out = np.ones(tuple(n - 1 for n in s.shape), dtype=bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                out &= s[dx:s.shape[0] - 1 + dx, dy:s.shape[1] - 1 + dy, dz:s.shape[2] - 1 + dz]
    return out


def keep_triangles(owner, seen):
    """bool [nt]: the triangles whose owner cell (flat index of its minimum corner, tests/mesh_ref.py's return_cells) has eight
    seen corners"""
    n = np.asarray(seen).shape
    owner = np.asarray(owner, dtype=np.int64)
    i, j, k = owner // (n[1] * n[2]), owner // n[2] % n[1], owner % n[2]
    return seen_cells(seen)[i, j, k]


def select(V, T, keep):
    """the kept triangles and the vertices they name, in order, ids remapped"""
    T = np.asarray(T)[np.asarray(keep, dtype=bool)]
    used = np.zeros(len(V), dtype=bool)
    used[T.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return np.asarray(V)[used], remap[T]


def mean_spacing(shape, lo, hi):
    return sum((float(hi[a]) - float(lo[a])) / (shape[a] - 1) for a in range(3)) / 3.0


# ---- the analytic plane ------------------------------------------------------------------------------------------------------
PLANE_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
PLANE_SHAPE = (9, 11, 13)
PLANE_Z = 0.1
PLANE_HW = (20, 24)
# (height h, x offset, y offset): the cameras look straight down -z from (ox, oy, h); every h is an fp32 number below 4
PLANE_CAMERAS = ((2.0, 0.0, 0.0), (2.5, 0.3, -0.2), (3.0, -0.25, 0.15))
PLANE_FOCAL = 20.0


def plane_scene():
    """(depth [3, H, W], opacity [3, H, W], proj [3, 3, 4], trunc in world units): constant depth maps d = h - 0.1 of the plane
    z = 0.1 seen from straight above; the third row of every proj is (0, 0, -1, h), so w = h - z.  With a focal length of 20 the
    frame covers |x - ox| < 0.6 w, |y - oy| < 0.5 w: lattice points near the top of the box fall outside every frame."""
    H, W = PLANE_HW
    K = np.array([[PLANE_FOCAL, 0, W / 2], [0, PLANE_FOCAL, H / 2], [0, 0, 1.0]])
    proj, depth = [], []
    for h, ox, oy in PLANE_CAMERAS:
        Rt = np.array([[1.0, 0, 0, -ox], [0, -1.0, 0, oy], [0, 0, -1.0, h]])
        proj.append(K @ Rt)
        depth.append(np.full((H, W), F(h) - F(PLANE_Z), dtype=F))
    proj = np.stack(proj).astype(F)
    assert all(tuple(p[2]) == (0.0, 0.0, -1.0, F(h)) for p, (h, _, _) in zip(proj, PLANE_CAMERAS))
    trunc = 4.0 * mean_spacing(PLANE_SHAPE, *PLANE_BOX)
    return np.stack(depth), np.ones((3, H, W), dtype=F), proj, trunc


def plane_bound():
    """The bound on |vertex z - 0.1| of the plane scene, in absolute terms, derived from the rounded operations between a depth map
    and a vertex.  u = 2^-24 is the unit roundoff: an fp32 result r carries an error of at most u |r| (half an ulp).  T = trunc,
    V = 3 views, Z the fp32 lattice coordinate the kernel forms (|Z| <= 1), h <= 3.
      w = fl(h - Z): the products by 0 and -1 and the sums with 0 are exact; one rounding of a number below 4:      2 u
      d = fl32(h - 0.1), a number below 4 (in [2, 4) half an ulp is 2 u):                                           2 u
      s = fl(d - w), |s| < 2:                                                                                          u
        so s = (Z - 0.1) + e_s with |e_s| <= 5 u.
      t = fl(s / T): relative u; the sum over at most V views: V - 1 roundings, relative u each; the division by the count:
        relative u.  With |t| <= 1 the mean is m = (Z - 0.1) / T + e_m with |e_m| <= 5 u / T + (V + 1) u.
      1 - m is rounded once (below 2: u), the product by 0.5 is exact: L = 0.5 (1 - (Z - 0.1) / T) + e_L, |e_L| <= 0.5 (e_m + u).
    L is linear in Z with slope -0.5 / T, so whatever edge is cut (only edges from the layer z = 0 to the layer z = 1/6 are: L
    is 0.56 and 0.46 there, far from 0.5 on the scale of e_L) an error e_L of its two ends moves the crossing by at most
    2 T e_L = 5 u + T (V + 2) u along z.
    The extraction then interpolates: t' = (0.5 - L_a) / (L_b - L_a) -- the numerator is exact (Sterbenz), the denominator and the
    quotient are rounded, relative 2 u of t' <= 1 -- and z = Z_a + t' (Z_b - Z_a): the difference and the product are rounded,
    relative u each of at most the spacing 1/6, and the sum, below 1/4, by u / 4:  (4 / 6 + 1 / 4) u < u.
    tests/mesh_ref.py interpolates in fp64 but between ITS lattice positions, which are the fp32 box carried through fp64: they
    differ from Z by the roundings of s (u / 2), 1 - s (u / 2 and the u / 2 it inherits... at most u in all for lo (1 - s)), hi s
    (u / 2) and the sum (u / 2): 2 u.
    In all (5 + T (V + 2) + 1 + 2) u: 12.2 u for T = 0.822, rounded up to whole units."""
    T = F(plane_scene()[3])
    return float(np.ceil(5 + float(T) * (len(PLANE_CAMERAS) + 2) + 1 + 2)) * 2.0 ** -24


# ---- the sphere seen by five cameras, one of them inside the box ---------------------------------------------------------------
SPHERE_BOX = ((-1.0, -1.2, -0.9), (1.0, 1.1, 1.3))
SPHERE_SHAPE = (9, 12, 17)
SPHERE_HW = (28, 20)
SPHERE_EYES = ((3.1, 0.4, 0.6), (-2.2, 2.4, 0.9), (0.3, -3.0, -1.2), (-0.6, 0.5, 3.4), (0.85, -0.9, 1.1))     # (the last: inside)
SPHERE_CENTRE, SPHERE_RADIUS = (0.05, -0.1, 0.15), 0.55


def look_at(eye, target, focal, H, W):
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]])
    return K, np.concatenate([Rm, -(Rm @ eye)[:, None]], 1)


def sphere_scene(seed=5):
    """(depth [5, H, W], opacity [5, H, W], proj [5, 3, 4], trunc): the camera-axis depth of a sphere at the pixel centres with
    seeded noise, opacity 1 on it and 0.02 beside it, and on top of that holes (opacity below 0.5 on the sphere), opacities of
    exactly 0.5, a NaN and an inf depth"""
    H, W = SPHERE_HW
    rng = np.random.default_rng(seed)
    depth, opacity, proj = [], [], []
    c = np.asarray(SPHERE_CENTRE)
    for eye in SPHERE_EYES:
        K, Rt = look_at(eye, SPHERE_CENTRE, 16.0, H, W)
        proj.append(K @ Rt)
        px = np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), -1)                   # [H, W, 2]
        dirs_c = np.concatenate([(px - K[:2, 2]) / K[0, 0], np.ones((H, W, 1))], -1)             # camera frame, third component 1
        dirs = dirs_c @ Rt[:, :3]                                                                # world
        o = np.asarray(eye) - c
        a_, b_, c_ = (dirs ** 2).sum(-1), 2 * dirs @ o, o @ o - SPHERE_RADIUS ** 2
        disc = b_ ** 2 - 4 * a_ * c_
        hit = disc > 0
        t = np.where(hit, (-b_ - np.sqrt(np.maximum(disc, 0))) / (2 * a_), 0.0)                  # the parameter IS the camera-axis depth
        d = np.where(hit, t + rng.normal(0, 0.01, (H, W)), 0.0)
        a = np.where(hit, 1.0, 0.02)
        holes = rng.random((H, W)) < 0.08
        a = np.where(holes & hit, 0.3, a)
        a[rng.integers(H), rng.integers(W)] = 0.5
        depth.append(d.astype(F))
        opacity.append(a.astype(F))
    depth, opacity = np.stack(depth), np.stack(opacity)
    depth[1, H // 2, W // 2], opacity[1, H // 2, W // 2] = np.nan, 1.0
    depth[2, H // 2, W // 2 - 1], opacity[2, H // 2, W // 2 - 1] = np.inf, 1.0
    trunc = 2.0 * mean_spacing(SPHERE_SHAPE, *SPHERE_BOX)
    return depth, opacity, np.stack(proj).astype(F), trunc
