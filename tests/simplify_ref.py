"""The mesh simplification contract of include/jt_render.h (jt_simplify_keys / jt_simplify_clusters / jt_simplify_triangles and
the compaction that follows), written out in NumPy: fp32 scalars for the keys, Python floats (IEEE fp64, every operation rounded
on its own) in Python loops for the cluster sums, a stable argsort.  Nothing here is shared with the kernels; the order of
operations is the header's, so the kernels have to agree with it bit for bit.

simplify(V, T, N, lo, hi, cells, lam, variant) -> (V' [nv', 3] float32, T' [nt', 3] int64, N' [nv', 3] float32, counts' [nv'] int64,
(n_dropped_invalid, n_collapsed), members: per output vertex the ids of the input vertices it replaces).  variant "mean" places
a vertex at fp32(c), the mean of its members, for comparison.  Analytic lattices with their normals live here too, so that the
CPU and the GPU tests use the same meshes."""
import math

import numpy as np

from tests import mesh_ref as R

REGULAR = 1.0 / 16.0
MAX_CELLS = 1 << 20


def cell_keys(V, lo, hi, cells):
    """keys [n] int64: four fp32 operations per axis, each rounded once; cx cy cz for a vertex with a non-finite coordinate"""
    V = np.asarray(V, dtype=np.float32).reshape(-1, 3)
    lo, hi = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(hi, dtype=np.float32).reshape(3)
    cx, cy, cz = (int(c) for c in cells)
    idx = []
    with np.errstate(all="ignore"):
        for a, c in enumerate((cx, cy, cz)):
            d = (V[:, a] - lo[a]).astype(np.float32)
            w = np.float32(hi[a] - lo[a])
            s = (d / w).astype(np.float32)
            f = (s * np.float32(c)).astype(np.float32)
            i = np.where(f >= np.float32(c), c - 1, np.where(f < 0, 0, np.floor(np.where(np.isfinite(f), f, 0))))
            idx.append(i.astype(np.int64))
    keys = (idx[0] * cy + idx[1]) * cz + idx[2]
    return np.where(np.isfinite(V).all(axis=1), keys, cx * cy * cz)


def representative(P, Nrm, lam, variant="qef"):
    """position [3] float32, normal [3] float32 of a cluster with members P [m, 3] float32, Nrm [m, 3] float32, in member order"""
    m = len(P)
    s = [0.0, 0.0, 0.0]
    for p in P:
        for a in range(3):
            s[a] = s[a] + float(p[a])
    c = [s[a] / float(m) for a in range(3)]
    a00 = a01 = a02 = a11 = a12 = a22 = 0.0
    b = [0.0, 0.0, 0.0]
    sn = [0.0, 0.0, 0.0]
    for p, nf in zip(P, Nrm):
        d = [float(p[a]) - c[a] for a in range(3)]
        n = [float(v) for v in nf] if np.isfinite(nf).all() else [0.0, 0.0, 0.0]
        e = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
        a00 = a00 + n[0] * n[0]
        a01 = a01 + n[0] * n[1]
        a02 = a02 + n[0] * n[2]
        a11 = a11 + n[1] * n[1]
        a12 = a12 + n[1] * n[2]
        a22 = a22 + n[2] * n[2]
        for a in range(3):
            b[a] = b[a] + n[a] * e
            sn[a] = sn[a] + n[a]
    r = float(np.float32(lam)) * float(m)
    a00, a11, a22 = a00 + r, a11 + r, a22 + r
    k00 = a11 * a22 - a12 * a12
    k01 = a02 * a12 - a01 * a22
    k02 = a01 * a12 - a02 * a11
    k11 = a00 * a22 - a02 * a02
    k12 = a01 * a02 - a00 * a12
    k22 = a00 * a11 - a01 * a01
    det = (a00 * k00 + a01 * k01) + a02 * k02
    with np.errstate(all="ignore"):
        x = [np.float64((k00 * b[0] + k01 * b[1]) + k02 * b[2]) / np.float64(det),
             np.float64((k01 * b[0] + k11 * b[1]) + k12 * b[2]) / np.float64(det),
             np.float64((k02 * b[0] + k12 * b[1]) + k22 * b[2]) / np.float64(det)]
        if variant == "mean":
            x = [0.0, 0.0, 0.0]
        pos = np.array([np.float32(np.float64(c[a]) + np.float64(x[a])) for a in range(3)], dtype=np.float32)
        pos = np.fmin(np.fmax(pos, P.min(axis=0)), P.max(axis=0)).astype(np.float32)
        length = np.sqrt(np.float64((sn[0] * sn[0] + sn[1] * sn[1]) + sn[2] * sn[2]))
        if length > 0 and np.isfinite(length):
            nrm = np.array([np.float32(np.float64(sn[a]) / length) for a in range(3)], dtype=np.float32)
        else:
            nrm = np.zeros(3, dtype=np.float32)
    return pos, nrm


def simplify(V, T, Nrm, lo, hi, cells, lam=REGULAR, variant="qef"):
    V = np.asarray(V, dtype=np.float32).reshape(-1, 3)
    Nrm = np.asarray(Nrm, dtype=np.float32).reshape(-1, 3)
    T = np.asarray(T, dtype=np.int64).reshape(-1, 3)
    cells = [int(cells)] * 3 if np.isscalar(cells) else [int(c) for c in cells]
    assert len(cells) == 3 and all(1 <= c <= MAX_CELLS for c in cells) and len(Nrm) == len(V)
    assert lam > 0 and math.isfinite(lam)
    n, none = len(V), cells[0] * cells[1] * cells[2]
    keys = cell_keys(V, lo, hi, cells)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    cluster = np.full(n, -1, dtype=np.int64)
    members, pos, nrm = [], [], []
    starts = [q for q in range(n) if ks[q] < none and (q == 0 or ks[q] != ks[q - 1])]
    n_valid = int((ks < none).sum())
    for j, q in enumerate(starts):
        end = starts[j + 1] if j + 1 < len(starts) else n_valid
        ids = order[q:end]
        assert (np.diff(ids) > 0).all()                        # stable: ascending vertex id
        cluster[ids] = j
        p, nn = representative(V[ids], Nrm[ids], lam, variant)
        members.append(ids)
        pos.append(p)
        nrm.append(nn)
    nc = len(starts)
    keep, used = np.zeros(len(T), dtype=bool), np.zeros(nc, dtype=bool)
    Tc = np.full((len(T), 3), -1, dtype=np.int64)
    n_invalid = n_collapsed = 0
    for t, ids in enumerate(T.tolist()):
        cl = [int(cluster[i]) if 0 <= i < n else -1 for i in ids]
        Tc[t] = cl
        if min(cl) < 0:
            n_invalid += 1
        elif cl[0] == cl[1] or cl[1] == cl[2] or cl[0] == cl[2]:
            n_collapsed += 1
        else:
            keep[t] = True
            used[cl] = True
    remap = np.cumsum(used) - 1
    sel = np.flatnonzero(used)
    Vo = np.array([pos[j] for j in sel], dtype=np.float32).reshape(-1, 3)
    No = np.array([nrm[j] for j in sel], dtype=np.float32).reshape(-1, 3)
    counts = np.array([len(members[j]) for j in sel], dtype=np.int64)
    To = remap[Tc[keep]].reshape(-1, 3)
    return Vo, To, No, counts, (n_invalid, n_collapsed), [members[j] for j in sel]


def cells_for(shape, K):
    """cells per axis for a cell of K lattice spacings on a lattice of `shape` points: ceil((points - 1) / K)"""
    return [int(math.ceil((int(s) - 1) / float(K))) for s in shape]


def edge_balance(T):
    """True iff every directed edge of triangles T occurs as often as its reverse"""
    count = {}
    for a, b, c in np.asarray(T, dtype=np.int64).reshape(-1, 3).tolist():
        for u, w in ((a, b), (b, c), (c, a)):
            count[(u, w)] = count.get((u, w), 0) + 1
    return all(count.get((w, u), 0) == k for (u, w), k in count.items())


def signed_volume(V, T):
    return R.topology(np.asarray(V, dtype=np.float64), T)["volume"]


# ---- the meshes of the tests: capped lattices of tests/mesh_ref.py, with analytic normals --------------------------------
SPHERE_CENTRE, SPHERE_RADIUS = (0.1, -0.05, 0.2), 0.7
CUBE_CENTRE, CUBE_HALF = (0.05, -0.1, 0.15), 0.55


def _unit(g):
    length = np.linalg.norm(g, axis=-1, keepdims=True)
    return np.where(length > 0, g / np.where(length > 0, length, 1.0), 0.0)


def sphere_lattice():
    """(capped lattice, lo, hi, level, normals(points) -> [n, 3] float64): the 20^3 sphere"""
    vol = R.sphere_field((20, 20, 20), SPHERE_CENTRE, SPHERE_RADIUS)
    vol, lo, hi = R.cap(vol, R.BOX_LO, R.BOX_HI)
    return vol, lo, hi, 0.0, lambda x: _unit(x - np.asarray(SPHERE_CENTRE))


def torus_lattice(major=0.6, minor=0.25, z0=0.2):
    vol = R.torus_field((24, 22, 20), major, minor, z0)
    vol, lo, hi = R.cap(vol, R.BOX_LO, R.BOX_HI)

    def normals(x):
        rho = np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2)
        ring = np.stack([x[:, 0] / rho * major, x[:, 1] / rho * major, np.full(len(x), z0)], -1)
        return _unit(x - ring)
    return vol, lo, hi, 0.0, normals


def cube_lattice():
    """an axis-aligned cube as the field half - max|x - centre|; normals are the face normals (the axis of the largest offset)"""
    x = R.lattice_points((20, 20, 20)) - np.asarray(CUBE_CENTRE)
    vol = (CUBE_HALF - np.abs(x).max(-1)).astype(np.float32)
    vol, lo, hi = R.cap(vol, R.BOX_LO, R.BOX_HI)

    def normals(p):
        d = p - np.asarray(CUBE_CENTRE)
        axis = np.abs(d).argmax(-1)
        out = np.zeros_like(d)
        out[np.arange(len(d)), axis] = np.sign(d[np.arange(len(d)), axis])
        return out
    return vol, lo, hi, 0.0, normals


LATTICES = {"sphere": sphere_lattice, "torus": torus_lattice, "cube": cube_lattice}
