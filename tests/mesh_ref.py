"""The mesh extraction contract of include/jt_render.h (jt_mesh_count / jt_mesh_emit), written out in NumPy and fp64: marching
tetrahedra on the Kuhn triangulation of every lattice cell.  Nothing here is shared with the kernels: the winding of every
(permutation, case) pair is derived at import time from the tetrahedron's ideal geometry (edge midpoints in the unit cube), never
from a computed vertex position, and the kernels' hand-written case table has to agree with it.

reference_mesh(vol, level, lo, hi) -> vertices [nv, 3] float64, triangles [nt, 3] int64, in the order the contract fixes: vertices
by owner point (flat index, z fastest) and edge kind, triangles by cell (flat index of its minimum corner) and permutation.
topology(V, T) -> what the tests ask of a surface.  Analytic fields for the tests live here too, so that the CPU and the GPU tests
use the same lattices."""
import itertools

import numpy as np

# edge kinds, bit 0..6 of the flags byte: the offset from the owner to the upper end
KIND_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
KIND_OF_OFFSET = {d: k for k, d in enumerate(KIND_OFFSETS)}
PERMS = tuple(itertools.permutations(range(3)))


def tet_corners(perm):
    """corner offsets c0..c3 of the tetrahedron of permutation (a, b, c)"""
    a, b, _ = perm
    c1 = [0, 0, 0]
    c1[a] = 1
    c2 = list(c1)
    c2[b] = 1
    return ((0, 0, 0), tuple(c1), tuple(c2), (1, 1, 1))


def _edge(u, w):
    return (u, w) if u < w else (w, u)


def _case_triangles(perm, inside):
    """triangles of one tetrahedron as triples of tetrahedron edges (u, w), u < w; `inside`: four bools in corner order"""
    ins = [q for q in range(4) if inside[q]]
    out = [q for q in range(4) if not inside[q]]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1 or len(out) == 1:
        q = ins[0] if len(ins) == 1 else out[0]
        x, y, z = [r for r in range(4) if r != q]
        tris = [(_edge(q, x), _edge(q, y), _edge(q, z))]
    else:
        (i0, i1), (o0, o1) = ins, out
        a, b, c, d = _edge(i0, o0), _edge(i0, o1), _edge(i1, o1), _edge(i1, o0)
        tris = [(a, b, c), (a, c, d)]
    # orientation from the ideal geometry: midpoints of the edges in the unit cube; the normal of the first triangle must point
    # from the inside corners' centroid to the outside corners'
    C = np.array(tet_corners(perm), dtype=np.float64)

    def mid(e):
        return 0.5 * (C[e[0]] + C[e[1]])
    p0, p1, p2 = (mid(e) for e in tris[0])
    normal = np.cross(p1 - p0, p2 - p0)
    s = float(normal @ (C[out].mean(axis=0) - C[ins].mean(axis=0)))
    assert abs(s) > 1e-9
    if s < 0:
        tris = [(t[0], t[2], t[1]) for t in tris]
    return tris


CASES = {(perm, case): _case_triangles(perm, [bool(case >> q & 1) for q in range(4)]) for perm in PERMS for case in range(16)}


def _as_box(lo, hi):
    return (np.asarray(lo, dtype=np.float32).astype(np.float64).reshape(3),
            np.asarray(hi, dtype=np.float32).astype(np.float64).reshape(3))


def reference_mesh(vol, level, lo, hi, return_cells=False):
    """vol [nx, ny, nz] float32.  With return_cells also the flat index of the owning cell of every triangle."""
    vol = np.asarray(vol)
    assert vol.dtype == np.float32 and vol.ndim == 3 and min(vol.shape) >= 2
    n = vol.shape
    level = float(np.float32(level))
    assert np.isfinite(level)
    lo, hi = _as_box(lo, hi)
    inside = vol > np.float32(level)                      # strict: a NaN is outside
    v64 = vol.astype(np.float64)
    axes = [np.array([lo[a] * (1 - i / (n[a] - 1)) + hi[a] * (i / (n[a] - 1)) for i in range(n[a])]) for a in range(3)]
    vid, V = {}, []
    with np.errstate(all="ignore"):
        for p in itertools.product(range(n[0]), range(n[1]), range(n[2])):
            for k, d in enumerate(KIND_OFFSETS):
                q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                if q[0] >= n[0] or q[1] >= n[1] or q[2] >= n[2] or inside[p] == inside[q]:
                    continue
                t = (level - v64[p]) / (v64[q] - v64[p])
                t = 0.5 if np.isnan(t) else min(max(t, 0.0), 1.0)
                vid[(p, k)] = len(V)
                V.append([axes[a][p[a]] + t * (axes[a][q[a]] - axes[a][p[a]]) for a in range(3)])
    T, cells = [], []
    for p in itertools.product(range(n[0] - 1), range(n[1] - 1), range(n[2] - 1)):
        flat = (p[0] * n[1] + p[1]) * n[2] + p[2]
        for perm in PERMS:
            C = tet_corners(perm)
            pts = [(p[0] + c[0], p[1] + c[1], p[2] + c[2]) for c in C]
            case = sum(int(inside[pts[q]]) << q for q in range(4))
            for tri in CASES[(perm, case)]:
                T.append([vid[(pts[u], KIND_OF_OFFSET[tuple(C[w][a] - C[u][a] for a in range(3))])] for u, w in tri])
                cells.append(flat)
    V = np.array(V, dtype=np.float64).reshape(-1, 3)
    T = np.array(T, dtype=np.int64).reshape(-1, 3)
    return (V, T, np.array(cells, dtype=np.int64)) if return_cells else (V, T)


def cap(vol, lo, hi):
    """one layer of zeros round the lattice, the box grown by one lattice spacing per side (fp32 box, as extract_mesh makes it)"""
    vol = np.asarray(vol, dtype=np.float32)
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    unit = (hi - lo) / (np.array(vol.shape, dtype=np.float32) - np.float32(1))
    return np.pad(vol, 1), lo - unit, hi + unit


def topology(V, T):
    """dict(closed, oriented, euler, volume, boundary): closed = every undirected edge lies in exactly two triangles; oriented =
    every directed edge occurs once and its reverse once; euler = V - E + F over the vertices the triangles use; volume = the
    signed volume (positive for outward normals); boundary = the undirected edges that lie in one triangle only."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.int64).reshape(-1, 3)
    directed, undirected = {}, {}
    for a, b, c in T.tolist():
        for u, w in ((a, b), (b, c), (c, a)):
            directed[(u, w)] = directed.get((u, w), 0) + 1
            key = (u, w) if u < w else (w, u)
            undirected[key] = undirected.get(key, 0) + 1
    closed = len(T) > 0 and all(c == 2 for c in undirected.values())
    oriented = len(T) > 0 and all(c == 1 and directed.get((w, u), 0) == 1 for (u, w), c in directed.items())
    p = V[T] if len(T) else np.zeros((0, 3, 3))
    volume = float(np.einsum("ni,ni->n", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
    return dict(closed=closed, oriented=oriented, euler=len(np.unique(T)) - len(undirected) + len(T), volume=volume,
                boundary=sorted(e for e, c in undirected.items() if c == 1))


def rotations_of(tris):
    """a sorted list of triangles, each rotated to start at its smallest id: equal for equal sets of oriented triangles"""
    out = []
    for t in np.asarray(tris).reshape(-1, 3).tolist():
        i = t.index(min(t))
        out.append(tuple(t[i:] + t[:i]))
    return sorted(out)


# ---- the lattices of the tests -------------------------------------------------------------------------------------------
BOX_LO, BOX_HI = (-1.0, -1.2, -0.9), (1.0, 1.1, 1.3)


def lattice_points(shape, lo=BOX_LO, hi=BOX_HI):
    """[nx, ny, nz, 3] float64 positions of the lattice P_axis(i) = lo (1 - s) + hi s over the fp32 box"""
    lo, hi = _as_box(lo, hi)
    ax = [lo[a] * (1 - np.arange(shape[a]) / (shape[a] - 1)) + hi[a] * (np.arange(shape[a]) / (shape[a] - 1)) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


def sphere_field(shape, centre, radius, lo=BOX_LO, hi=BOX_HI):
    """radius - |x - centre|: positive inside, a distance function"""
    return (radius - np.linalg.norm(lattice_points(shape, lo, hi) - np.asarray(centre), axis=-1)).astype(np.float32)


def torus_field(shape, major=0.6, minor=0.25, z0=0.2, lo=BOX_LO, hi=BOX_HI):
    x = lattice_points(shape, lo, hi)
    ring = np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) - major
    return (minor - np.sqrt(ring ** 2 + (x[..., 2] - z0) ** 2)).astype(np.float32)


def two_spheres_field(shape, r=0.3, lo=BOX_LO, hi=BOX_HI):
    x = lattice_points(shape, lo, hi)
    d = np.minimum(np.linalg.norm(x - np.array([0.5, 0, 0]), axis=-1), np.linalg.norm(x - np.array([-0.5, 0, 0]), axis=-1))
    return (r - d).astype(np.float32)


def integer_sphere_field():
    """4 - |x|^2 on the integer lattice [-3, 3]^3: six lattice points (+-2 on an axis) have the value 0 exactly"""
    g = np.arange(-3, 4, dtype=np.float64)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1)
    return (4.0 - (x ** 2).sum(-1)).astype(np.float32), (-3.0, -3.0, -3.0), (3.0, 3.0, 3.0)


def cell_configuration(config):
    """the 4 x 4 x 4 lattice of -1 with the eight corners of its middle cell set to +1 where bit (dx | dy << 1 | dz << 2) of
    `config` is set"""
    vol = -np.ones((4, 4, 4), dtype=np.float32)
    for m in range(8):
        if config >> m & 1:
            vol[1 + (m & 1), 1 + (m >> 1 & 1), 1 + (m >> 2 & 1)] = 1.0
    return vol


def uniform_lattice(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)
