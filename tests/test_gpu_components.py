"""Connected components of a lattice on the GPU (csrc/jt_components.hip through ops.lattice_components / ops.keep_components)
against the NumPy union-find of tests/components_ref.py.  The result is a unique fixed point (the smallest flat index of every
component), so every comparison is torch.equal: no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from tests import components_ref as C
from tests import mesh_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu_labels(vol, level, **kw):
    from joint_tensorf_amd import ops
    lab = ops.lattice_components(torch.from_numpy(np.ascontiguousarray(vol)).to(DEV), level, **kw)
    assert lab.is_cuda and lab.dtype == torch.int32 and tuple(lab.shape) == tuple(vol.shape)
    return lab.cpu()


def _check(vol, level, label=""):
    want = torch.from_numpy(C.labels(vol, level))
    got = _gpu_labels(vol, level)
    assert torch.equal(got, want), (label, int((got != want).sum()))
    return got


def test_all_255_cell_configurations():
    for config in range(1, 256):
        _check(R.cell_configuration(config), 0.0, "configuration %d" % config)


@pytest.mark.parametrize("level,n_components", [(0.8, 544), (0.6, 276), (0.5, 156)])
def test_random_lattices(level, n_components):
    from joint_tensorf_amd import ops
    vol = R.uniform_lattice((33, 20, 17), seed=5)
    lab = _check(vol, level, "uniform at %g" % level)
    roots, counts = ops.component_sizes(lab.to(DEV))
    want_roots, want_counts = C.sizes(lab.numpy())
    print("level %g: %d components, the largest of %d points, %s" % (level, len(want_roots), want_counts.max(), ops.last_components_stats))
    assert len(want_roots) == n_components
    assert np.array_equal(roots.cpu().numpy(), want_roots) and np.array_equal(counts.cpu().numpy(), want_counts)
    if level == 0.5:
        assert want_counts.max() == 2325


def _edge_shapes():
    from joint_tensorf_amd.ops import COMPONENTS_TILE as t
    shapes = [(2, 2, 2), (t, t, t)]
    for axis in range(3):
        for n in (t - 1, t + 1, 2 * t - 1, 2 * t, 2 * t + 1):
            s = [t + 1, t, t - 1]
            s[axis] = n
            shapes.append(tuple(s))
    return list(dict.fromkeys(shapes))


@pytest.mark.parametrize("shape", _edge_shapes(), ids=lambda s: "x".join(str(v) for v in s))
def test_tile_edges(shape):
    """one below, at and one above the tile edge (and two tiles) on each axis; dense enough that components cross tile faces"""
    vol = R.uniform_lattice(shape, seed=sum(shape))
    for level in (0.4, 0.0):
        _check(vol, level, "%s at %g" % (shape, level))


def test_uniform_and_nan_lattices():
    inside = _gpu_labels(np.ones((9, 17, 10), dtype=np.float32), 0.0)
    assert bool((inside == 0).all())                                         # one component, its smallest index
    assert bool((_gpu_labels(-np.ones((9, 17, 10), dtype=np.float32), 0.0) == -1).all())
    assert bool((_gpu_labels(np.full((5, 9, 8), np.nan, dtype=np.float32), 0.0) == -1).all())
    vol = np.full((5, 9, 8), np.nan, dtype=np.float32)
    vol[4, 8, 7] = vol[0, 0, 0] = 1.0
    lab = _gpu_labels(vol, 0.0)
    assert lab[4, 8, 7] == 5 * 9 * 8 - 1 and lab[0, 0, 0] == 0 and int((lab >= 0).sum()) == 2


def _snakes():
    """a one-point-wide path through a 17 x 17 x 9 lattice: along x in the rows y = 0, 4, 8, 12, 16, joined at alternating ends, in
    the layers z = 0, 4, 8, joined at the path's end -- it crosses tile faces dozens of times; and a second one, the same shape
    moved by two points in y and z (rows 2, 6, 10, 14 of the layers 2 and 6), that never touches it (no two of their points
    are closer than two lattice steps on some axis)"""
    vol = -np.ones((17, 17, 9), dtype=np.float32)

    def snake(rows, layers):
        where_y = rows[0]
        for li, z in enumerate(layers):
            order = rows if li % 2 == 0 else rows[::-1]
            x_end = 0
            for ri, y in enumerate(order):
                vol[:, y, z] = 1.0
                if ri + 1 < len(order):
                    # the joint at alternating ends of the rows
                    x_end = 16 if (ri % 2 == 0) else 0
                    a, b = sorted((y, order[ri + 1]))
                    vol[x_end, a:b + 1, z] = 1.0
            where_y = order[-1]
            if li + 1 < len(layers):
                x_last = 16 if (len(order) % 2 == 1) else 0
                vol[x_last, where_y, z:layers[li + 1] + 1] = 1.0
    snake([0, 4, 8, 12, 16], [0, 4, 8])
    snake([2, 6, 10, 14], [2, 6])
    return vol


def test_snakes():
    from joint_tensorf_amd import ops
    vol = _snakes()
    want = C.labels(vol, 0.0)
    assert len(C.sizes(want)[0]) == 2                                         # the reference itself: two snakes that never touch
    got = _gpu_labels(vol, 0.0)
    stats = dict(ops.last_components_stats)
    no_jump = _gpu_labels(vol, 0.0, jump=False)
    print("snakes: %d + %d points; with pointer jumping %s, without %s"
          % (tuple(C.sizes(want)[1]) + (stats, dict(ops.last_components_stats))))
    assert torch.equal(got, torch.from_numpy(want)) and torch.equal(no_jump, got)
    assert stats["converged_at"] > 1
    with pytest.raises(RuntimeError, match="17 x 17 x 9.*1 sweeps"):
        _gpu_labels(vol, 0.0, max_sweeps=1)
    # the flags are read once per `check_every` sweeps: any batch size ends at the same labels
    assert torch.equal(_gpu_labels(vol, 0.0, check_every=1), got) and torch.equal(_gpu_labels(vol, 0.0, check_every=3), got)


def test_two_runs_give_the_same_bits():
    vol = R.uniform_lattice((33, 20, 17), seed=5)
    assert torch.equal(_gpu_labels(vol, 0.5), _gpu_labels(vol, 0.5))


def _three_spheres(shape=(25, 12, 12)):
    x = R.lattice_points(shape)
    big = R.two_spheres_field(shape, r=0.3)
    small = (0.17 - np.linalg.norm(x - np.array([0.0, 0.75, 0.9]), axis=-1)).astype(np.float32)
    return big, small


def test_keep_components_on_spheres():
    from joint_tensorf_amd import ops
    big, small = _three_spheres()
    vol = np.maximum(big, small)
    lab = C.labels(vol, 0.0)
    roots, counts = C.sizes(lab)
    n_small = int((small > 0).sum())
    print("spheres: labels %s, points %s" % (roots.tolist(), counts.tolist()))
    assert len(roots) == 3 and sorted(counts.tolist()) == sorted([n_small, counts.max(), counts.max()]) and 0 < n_small < counts.max()
    dvol = torch.from_numpy(vol).to(DEV)
    fill = -0.25
    # keep_largest = 2: the mesh of the two big spheres' points alone, `fill` elsewhere inside, to the bit
    out, kept, dropped = ops.keep_components(dvol, 0.0, keep_largest=2, fill=fill)
    want = np.where((small > 0) & (vol > 0), np.float32(fill), vol)
    assert (kept, dropped) == (2, 1) and np.array_equal(out.cpu().numpy(), want)
    got = ops.mesh_from_lattice(out, 0.0, R.BOX_LO, R.BOX_HI)
    ref = ops.mesh_from_lattice(torch.from_numpy(want).to(DEV), 0.0, R.BOX_LO, R.BOX_HI)
    assert got[0].shape[0] > 50 and torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    t = R.topology(got[0].cpu().numpy(), got[1].cpu().numpy())
    assert t["closed"] and t["oriented"] and t["euler"] == 4
    # min_points at the exact size of the small sphere (it stays) and one above (it goes)
    out, kept, dropped = ops.keep_components(dvol, 0.0, min_points=n_small, fill=fill)
    assert (kept, dropped) == (3, 0) and torch.equal(out, dvol)
    out, kept, dropped = ops.keep_components(dvol, 0.0, min_points=n_small + 1, fill=fill)
    assert (kept, dropped) == (2, 1) and np.array_equal(out.cpu().numpy(), want)
    # the two equal spheres tie under keep_largest = 1: the one with the smaller label stays
    out, kept, dropped = ops.keep_components(dvol, 0.0, keep_largest=1, fill=fill)
    first = roots[counts == counts.max()].min()
    assert (kept, dropped) == (1, 2) and np.array_equal(out.cpu().numpy(), np.where((lab == first) | (lab < 0), vol, np.float32(fill)))
    # both tests at once; and the reference's own statement of the rule agrees throughout
    for kw in (dict(keep_largest=3, min_points=n_small + 1), dict(keep_largest=1, min_points=int(counts.max()) + 1), dict(min_points=1)):
        out, kept, dropped = ops.keep_components(dvol, 0.0, fill=fill, **kw)
        rv, rk, rd = C.keep_components(vol, 0.0, fill=fill, **kw)
        assert (kept, dropped) == (rk, rd) and np.array_equal(out.cpu().numpy(), rv), kw
    with pytest.raises(ValueError):
        ops.keep_components(dvol, 0.0, keep_largest=1, fill=0.1)
    with pytest.raises(ValueError):
        ops.lattice_components(dvol.double(), 0.0)
