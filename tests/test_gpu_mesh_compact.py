"""The one compaction of joint_tensorf_amd/mesh_ops.py through its three callers -- compact_mesh, select_triangles and
simplify_compact -- on a mesh written out by hand: 12 vertices, 20 triangles.  Copies and integers only: every comparison is
of bits.  The selection rule is tests/visible_ref.py's; what the vertex statuses make of a triangle is include/jt_render.h's
jt_mesh_filter_count, restated below."""
import numpy as np
import pytest
import torch

from tests import visible_ref as VR

DEV = "cuda"
NV = 12
# vertices 10 and 11 are named by no triangle; triangle 7 has an id of 12, triangle 8 one of -1
TRIANGLES = np.array([[0, 1, 2], [1, 2, 4], [2, 4, 6], [0, 2, 3], [3, 5, 6], [4, 5, 6], [6, 8, 9], [0, 12, 1], [2, -1, 4], [8, 9, 0],
                      [7, 8, 9], [1, 4, 6], [5, 8, 9], [9, 8, 6], [0, 4, 8], [7, 0, 1], [2, 6, 9], [1, 0, 9], [5, 1, 2], [4, 2, 0]],
                     dtype=np.int32)
# two vertices beyond (1), one far (2); triangle 4 = (3, 5, 6) touches both kinds
STATUS = np.zeros(NV, dtype=np.uint8)
STATUS[[3, 7]] = 1
STATUS[5] = 2
_REF = {}


def _mesh():
    rng = np.random.default_rng(5)
    V, N, C = (rng.standard_normal((NV, 3)).astype(np.float32) for _ in range(3))
    V[2, 1], C[9, 0] = -0.0, np.inf                                   # bits a comparison of values would not tell apart
    return V, N, C


def _cause(triangles, status):
    """jt_mesh_filter_count's cause [nt] uint8: 0 kept, else the first that applies of 1 (an id out of range, a vertex beyond)
    and 2 (a vertex far)"""
    ok = VR.in_range(triangles, len(status))
    st = status[np.clip(triangles, 0, len(status) - 1)]
    beyond = ~ok | (st == 1).any(1)
    return np.where(beyond, 1, np.where((st == 2).any(1), 2, 0)).astype(np.uint8)


def _reference():
    """the expected arrays, computed once and checked against what the mesh was written to give"""
    if not _REF:
        V, N, C = _mesh()
        cause = _cause(TRIANGLES, STATUS)
        keep = (cause == 0).astype(np.uint8)
        used = np.zeros(NV, dtype=np.uint8)
        used[TRIANGLES[keep != 0].ravel()] = 1
        assert TRIANGLES.shape == (20, 3) and not np.isin([10, 11], TRIANGLES).any()
        assert np.flatnonzero(cause == 1).tolist() == [3, 4, 7, 8, 10, 15] and np.flatnonzero(cause == 2).tolist() == [5, 12, 18]
        assert cause[4] == 1 and set(STATUS[TRIANGLES[4]]) == {0, 1, 2}   # the mixed triangle: once, as beyond
        assert np.flatnonzero(used).tolist() == [0, 1, 2, 4, 6, 8, 9]
        want = VR.select(V, TRIANGLES, keep, N, C)
        assert want[0].shape == (7, 3) and want[1].shape == (11, 3) and want[4] == 9 and want[1].max() == 6
        _REF.update(V=V, N=N, C=C, cause=cause, keep=keep, used=used, want=want)
    return _REF


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is None:
            assert g is None
            continue
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


def _empty(out, with_attrs):
    assert [tuple(o.shape) for o in out[:2]] == [(0, 3), (0, 3)] and out[1].dtype == torch.int32
    for o in out[2:4]:
        assert tuple(o.shape) == (0, 3) if with_attrs else o is None


def test_the_reference_is_what_the_mesh_was_written_to_give():
    _reference()


@pytest.mark.gpu
def test_compact_mesh():
    from joint_tensorf_amd import ops
    r = _reference()
    out = ops.compact_mesh(_dev(r["V"]), _dev(TRIANGLES), _dev(STATUS), _dev(r["N"]), _dev(r["C"]))
    _same_bits(out[:4], r["want"][:4])
    assert out[4] == (6, 3)
    out = ops.compact_mesh(_dev(r["V"]), _dev(TRIANGLES), _dev(STATUS), colors=_dev(r["C"]))
    _same_bits(out[:4], r["want"][:2] + (None, r["want"][3]))


@pytest.mark.gpu
def test_select_triangles():
    from joint_tensorf_amd import ops
    r = _reference()
    V, N, C = _dev(r["V"]), _dev(r["N"]), _dev(r["C"])
    out = ops.select_triangles(V, _dev(TRIANGLES), _dev(r["keep"]), N, C)
    _same_bits(out[:4], r["want"][:4])
    assert out[4] == 20 - out[1].shape[0] == 9
    # the mesh minus its unused vertices and bad triangles, all kept: the input's bits
    clean = VR.select(r["V"], TRIANGLES, np.ones(20, dtype=np.uint8), r["N"], r["C"])
    assert clean[0].shape == (10, 3) and clean[1].shape == (18, 3)
    out = ops.select_triangles(_dev(clean[0]), _dev(clean[1]), torch.ones(18, device=DEV, dtype=torch.bool), _dev(clean[2]), _dev(clean[3]))
    _same_bits(out[:4], clean[:4])
    assert out[4] == 0


@pytest.mark.gpu
def test_nothing_kept():
    from joint_tensorf_amd import ops
    r = _reference()
    V, T, N = _dev(r["V"]), _dev(TRIANGLES), _dev(r["N"])
    zeros = torch.zeros(20, device=DEV, dtype=torch.uint8)
    for attrs in ((), (N, _dev(r["C"]))):
        out = ops.select_triangles(V, T, zeros, *attrs)
        _empty(out, bool(attrs))
        assert out[4] == 20
        out = ops.compact_mesh(V, T, torch.full((NV,), 2, device=DEV, dtype=torch.uint8), *attrs)
        _empty(out, bool(attrs))
        assert out[4] == (2, 18)                                        # the two bad ids are beyond, the rest far


@pytest.mark.gpu
def test_simplify_compact():
    """the clusters are the mesh's vertices, tri its triangles; keep, cause and used as jt_simplify_triangles would leave them"""
    from joint_tensorf_amd import ops
    r = _reference()
    c_cnt = np.arange(1, NV + 1, dtype=np.int32) * 3
    c_pos, c_nrm, tri = _dev(r["V"]), _dev(r["N"]), _dev(TRIANGLES)
    out = ops.simplify_compact(c_pos, c_nrm, _dev(c_cnt), tri, _dev(r["keep"]), _dev(r["cause"]), _dev(r["used"]))
    sel = ops.select_triangles(c_pos, tri, _dev(r["keep"]), c_nrm)
    _same_bits(out[:3], tuple(a.cpu().numpy() for a in sel[:3]))
    _same_bits(out[:3], r["want"][:3])
    assert out[3].dtype == torch.int32 and out[3].cpu().numpy().tolist() == c_cnt[r["used"] != 0].tolist()
    assert out[4] == (6, 3)
    zeros = torch.zeros(20, device=DEV, dtype=torch.uint8)
    out = ops.simplify_compact(c_pos, c_nrm, _dev(c_cnt), tri, zeros, torch.ones_like(zeros), torch.zeros(NV, device=DEV, dtype=torch.uint8))
    assert out == (None, None, None, None, (20, 0))
