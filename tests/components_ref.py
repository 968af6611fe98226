"""The connected-component contract of include/jt_render.h (jt_components_* / ops.lattice_components, ops.keep_components) written
out in NumPy: a union-find over the mesh's own connectivity.  Two lattice points are adjacent iff both are inside (v > level; a NaN
is outside) and they differ by + or - one of the seven edge kinds of tests/mesh_ref.py -- 14 neighbours.  A point's label is the
smallest flat index (z fastest) of its component, -1 outside: a unique fixed point, so the kernels must give these bits."""
import numpy as np

from tests.mesh_ref import KIND_OFFSETS

OFFSETS = tuple(KIND_OFFSETS) + tuple((-a, -b, -c) for a, b, c in KIND_OFFSETS)


def labels(vol, level):
    """vol [nx, ny, nz] float32 -> int32 [nx, ny, nz]"""
    vol = np.asarray(vol)
    assert vol.dtype == np.float32 and vol.ndim == 3
    nx, ny, nz = vol.shape
    inside = (vol > np.float32(level)).reshape(-1)
    parent = np.arange(inside.size)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    idx = np.arange(inside.size).reshape(nx, ny, nz)
    for dx, dy, dz in KIND_OFFSETS:                     # every undirected edge once: from the owner to its upper end
        a = idx[:nx - dx, :ny - dy, :nz - dz].reshape(-1)
        b = idx[dx:, dy:, dz:].reshape(-1)
        both = inside[a] & inside[b]
        for p, q in zip(a[both].tolist(), b[both].tolist()):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)       # the smaller index stays the root: the root is the component's minimum
    out = np.full(inside.size, -1, dtype=np.int32)
    for p in np.flatnonzero(inside).tolist():
        out[p] = find(p)
    return out.reshape(nx, ny, nz)


def sizes(lab):
    """(roots ascending, counts) of a label array"""
    roots, counts = np.unique(lab[lab >= 0], return_counts=True)
    return roots, counts


def keep_components(vol, level, keep_largest=None, min_points=None, fill=0.0):
    """ops.keep_components: (vol', kept, dropped); ties under keep_largest go to the smaller label"""
    vol = np.asarray(vol, dtype=np.float32)
    if keep_largest is None and min_points is None:
        return vol, None, None
    if not fill <= level:
        raise ValueError("fill exceeds level")
    lab = labels(vol, level)
    roots, counts = sizes(lab)
    keep = np.ones(len(roots), dtype=bool)
    if keep_largest is not None:
        order = sorted(range(len(roots)), key=lambda i: (-int(counts[i]), int(roots[i])))
        keep[:] = False
        keep[order[:keep_largest]] = True
    if min_points is not None:
        keep &= counts >= min_points
    out = vol.copy()
    out[np.isin(lab, roots[~keep])] = np.float32(fill)
    return out, int(keep.sum()), int((~keep).sum())
