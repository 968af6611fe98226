"""The mesh simplification without a GPU: the NumPy statement of its contract (tests/simplify_ref.py) on the capped analytic
lattices of tests/mesh_ref.py -- what the GPU tests then hold the kernels to, bit for bit -- and the option parsing of
`python -m joint_tensorf_amd.export --simplify.cell=K`."""
import numpy as np
import pytest

from tests import mesh_ref as R
from tests import simplify_ref as S

_MESHES = {}


def _mesh(name):
    """(V float32, T, N float32, lo, hi, lattice shape) of a lattice of simplify_ref.LATTICES, computed once"""
    if name not in _MESHES:
        vol, lo, hi, level, normals = S.LATTICES[name]()
        V, T = R.reference_mesh(vol, level, lo, hi)
        V = V.astype(np.float32)
        _MESHES[name] = (V, T, normals(V.astype(np.float64)).astype(np.float32), lo, hi, vol.shape)
    return _MESHES[name]


def test_the_lattices_are_closed_surfaces():
    V, T, N, lo, hi, shape = _mesh("sphere")
    assert shape == (22, 22, 22) and len(V) == 2134
    for name, euler in (("sphere", 2), ("torus", 0), ("cube", 2)):
        V, T, N, lo, hi, shape = _mesh(name)
        t = R.topology(V, T)
        assert t["closed"] and t["oriented"] and t["euler"] == euler and t["volume"] > 0, (name, t)
        assert np.allclose(np.linalg.norm(N, axis=1), 1.0, atol=1e-6) and S.edge_balance(T)


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("name", ["sphere", "torus", "cube"])
def test_reference_properties(name, K):
    V, T, N, lo, hi, shape = _mesh(name)
    cells = S.cells_for(shape, K)
    Vo, To, No, counts, (n_invalid, n_collapsed), members = S.simplify(V, T, N, lo, hi, cells)
    Vm, Tm, _, _, _, _ = S.simplify(V, T, N, lo, hi, cells, variant="mean")
    vol_in, vol_qef, vol_mean = S.signed_volume(V, T), S.signed_volume(Vo, To), S.signed_volume(Vm, Tm)
    print("%s K=%d cells %s: %d / %d -> %d / %d, volume %.4f, qef %.4f, mean %.4f, largest cluster %d"
          % (name, K, cells, len(V), len(T), len(Vo), len(To), vol_in, vol_qef, vol_mean, counts.max()))
    assert 0 < len(Vo) < len(V) and 0 < len(To) < len(T)
    assert n_invalid == 0 and n_collapsed == len(T) - len(To) and np.array_equal(Tm, To)
    assert S.edge_balance(To)                                   # every directed edge as often as its reverse
    assert (To[:, 0] != To[:, 1]).all() and (To[:, 1] != To[:, 2]).all() and (To[:, 0] != To[:, 2]).all()
    assert To.min() == 0 and To.max() == len(Vo) - 1 and len(np.unique(To)) == len(Vo)
    assert counts.sum() <= len(V) and [len(m) for m in members] == counts.tolist()
    for j, ids in enumerate(members):                           # inside the bounding box of what it replaces
        assert (Vo[j] >= V[ids].min(axis=0)).all() and (Vo[j] <= V[ids].max(axis=0)).all(), (name, K, j)
    assert np.isfinite(Vo).all() and np.isfinite(No).all()
    assert abs(vol_qef - vol_in) < abs(vol_mean - vol_in), (vol_in, vol_qef, vol_mean)


def test_keys_clamp_and_skip_non_finite_vertices():
    lo, hi = np.float32([0, 0, 0]), np.float32([1, 2, 4])
    V = np.float32([[0, 0, 0], [1, 2, 4], [-5, 1, 1], [0.5, 9, 1], [0.25, 0.5, 1.0], [np.nan, 0, 0], [0, np.inf, 0]])
    keys = S.cell_keys(V, lo, hi, (4, 4, 4))
    assert keys.tolist() == [0, 63, (0 * 4 + 2) * 4 + 1, (2 * 4 + 3) * 4 + 1, (1 * 4 + 1) * 4 + 1, 64, 64]
    assert S.cell_keys(V, lo, hi, (1, 1, 1)).tolist() == [0, 0, 0, 0, 0, 1, 1]


def test_single_members_zero_normals_and_dropped_triangles():
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    V = np.float32([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.12, 0.1, 0.16], [np.nan, 0.5, 0.5]])
    N = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1]])
    T = np.array([[0, 1, 2], [3, 1, 2], [0, 3, 1], [0, 1, 4], [0, 1, 7]])
    Vo, To, No, counts, drops, members = S.simplify(V, T, N, lo, hi, 2)
    assert drops == (2, 1) and counts.tolist() == [2, 1, 1] and To.tolist() == [[0, 2, 1], [0, 2, 1]]
    mean = ((V[0].astype(np.float64) + V[3].astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(Vo[0], mean) and np.array_equal(No[0], np.zeros(3, np.float32))       # zero normals: the mean
    assert np.array_equal(Vo[1], V[2]) and np.array_equal(Vo[2], V[1])                          # single members: exact
    assert np.array_equal(No[1], N[2]) and np.array_equal(No[2], N[1])


def test_export_option_parsing():
    from joint_tensorf_amd import export
    base = ["--yaml=bat_blender_VM"]
    assert export.build_options(base).simplify.cell is None
    assert export.build_options(base + ["--simplify.cell=3"]).simplify.cell == 3.0
    assert export.build_options(base + ["--simplify.cell=2.5"]).simplify.cell == 2.5
    for bad in ("0.5", "0", "-2", "true", "nan", "inf", "[2,2,2]", "wide"):
        with pytest.raises(SystemExit):
            export.build_options(base + ["--simplify.cell=%s" % bad])
    with pytest.raises(SystemExit):
        export.build_options(base + ["--simplify=3"])
    with pytest.raises(KeyError):
        export.build_options(base + ["--simplify.cells=3"])
