"""jt_mesh_unwarp_ndc (ops.ndc_to_world) against tests/ndc_ref.py evaluated in fp64 on the same fp32 inputs.

The bounds are derived, not measured.  Positions: u = 1 - zn is one correctly rounded operation (exact for zn in [0.5, 2], Sterbenz),
z = 2n / u a second, xn z a third and the division by sx a fourth: (1 + 2^-24)^4 - 1 < 8 * 2^-24 relative, per component.  Normals:
fewer than sixteen roundings from the inputs to a component of the unit vector, and the cancelling terms of the third component are
bounded by |xn|, |yn| <= 2 times the first two: 2^-20 absolute."""
import numpy as np
import pytest
import torch

from tests import ndc_ref as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
LO, HI = np.array([-1.5, -1.67, -2.0]), np.array([1.5, 1.67, 1.0])      # the LLFF scene box (configs/bat_llff_VM_MLP.yaml)
POS_REL, NRM_ABS = 8 * 2.0 ** -24, 2.0 ** -20
NEAR = 1.0
MAX_DEPTH = 8.0
# zn = 1: infinity; just behind it; u = 2^-23; a NaN and an inf coordinate; z exactly MAX_DEPTH (u = 1/4: z = 8) and the next zn
# above it (u = 1/4 - 2^-24: z = 8 + 2^-19 in fp32 and fp64 alike)
EDGES = np.array([[0.3, -0.4, 1.0], [0.3, -0.4, 1.0 + 2.0 ** -20], [0.3, -0.4, 1.0 - 2.0 ** -23], [np.nan, 0.1, 0.2],
                  [0.1, np.inf, 0.2], [0.1, 0.2, -np.inf], [0.5, -0.5, 0.75], [0.5, -0.5, 0.75 + 2.0 ** -24]], dtype=np.float32)
EDGE_STATUS = [1, 1, 2, 1, 1, 1, 0, 2]
EDGE_STATUS_NO_LIMIT = [1, 1, 0, 1, 1, 1, 0, 0]


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(LO, HI, (n, 3)).astype(np.float32)
    k = min(n, len(EDGES))
    if n > 1:
        q[:k] = EDGES[:k]
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    if n > 16:
        nrm[9] = 0.0                                                    # a degenerate normal stays (0, 0, 0)
    sx, sy = (float(np.float32(v)) for v in rng.uniform(0.5, 2.0, 2))
    return q, nrm, sx, sy


def _check(q, nrm, sx, sy, max_depth):
    from joint_tensorf_amd import ops
    want_w, want_n, want_s = N.unwarp(q.astype(np.float64), sx, sy, NEAR, normals=nrm.astype(np.float64), max_depth=max_depth)
    if max_depth is not None:
        # the limit is compared with the fp32 z: no random point may sit within the position bound of it (the edge rows are exact)
        z = N.inverse(q.astype(np.float64), sx, sy, NEAR)[len(EDGES):, 2]
        assert not (np.abs(z - max_depth) <= 2 * POS_REL * max_depth).any()
    tq, tn = torch.from_numpy(q).to(DEV), torch.from_numpy(nrm).to(DEV)
    world, normals, status = ops.ndc_to_world(tq, sx, sy, NEAR, normals=tn, max_depth=max_depth)
    assert world.dtype == torch.float32 and normals.dtype == torch.float32 and status.dtype == torch.uint8
    assert tuple(world.shape) == tuple(normals.shape) == q.shape and tuple(status.shape) == (len(q),)
    w, nn, st = world.cpu().numpy(), normals.cpu().numpy(), status.cpu().numpy()
    assert (st == want_s).all(), np.nonzero(st != want_s)
    gone = st != 0
    assert (w[gone] == 0).all() and (nn[gone] == 0).all()               # zeros, not the arithmetic's inf / nan
    err = np.abs(w.astype(np.float64) - want_w)
    print("\n[ndc unwarp] n %d max_depth %r: kept %d beyond %d far %d; position error %.3g of the bound, normal error %.3g of the bound"
          % (len(q), max_depth, (st == 0).sum(), (st == 1).sum(), (st == 2).sum(),
             (err / (POS_REL * np.maximum(np.abs(want_w), 1e-300))).max(), np.abs(nn - want_n).max() / NRM_ABS))
    assert (err <= POS_REL * np.abs(want_w)).all()
    assert np.abs(nn.astype(np.float64) - want_n).max() <= NRM_ABS
    # two runs give the same bits; and the positions do not depend on whether normals travel along
    world2, normals2, status2 = ops.ndc_to_world(tq, sx, sy, NEAR, normals=tn, max_depth=max_depth)
    assert torch.equal(world, world2) and torch.equal(normals, normals2) and torch.equal(status, status2)
    world3, none, status3 = ops.ndc_to_world(tq, sx, sy, NEAR, max_depth=max_depth)
    assert none is None and torch.equal(world, world3) and torch.equal(status, status3)
    return st


@pytest.mark.parametrize("max_depth", [MAX_DEPTH, None])
def test_tail_block_against_fp64(max_depth):
    q, nrm, sx, sy = _inputs(4099, seed=0)
    st = _check(q, nrm, sx, sy, max_depth)
    assert st[:len(EDGES)].tolist() == (EDGE_STATUS if max_depth is not None else EDGE_STATUS_NO_LIMIT)
    assert (st == 0).sum() > 1000 and (max_depth is None or (st == 2).sum() > 100)


def test_one_ulp_above_the_limit():
    """the vertex at z = 8 under a limit one ulp below 8: far; under 8 itself it was kept (EDGE_STATUS[6])"""
    from joint_tensorf_amd import ops
    below = float(np.nextafter(np.float32(MAX_DEPTH), np.float32(0)))
    q = torch.from_numpy(EDGES[6:7]).to(DEV)
    assert ops.ndc_to_world(q, 1.25, 0.75, NEAR, max_depth=below)[2].tolist() == [2]
    world, _, st = ops.ndc_to_world(q, 1.25, 0.75, NEAR, max_depth=MAX_DEPTH)
    f = np.float32                                          # xn z is exact here, the division by sx or sy the one rounding
    assert st.tolist() == [0] and world.tolist() == [[float(f(4.0) / f(1.25)), float(f(-4.0) / f(0.75)), 8.0]]


def test_a_single_vertex():
    q, nrm, sx, sy = _inputs(1, seed=3)
    assert _check(q, nrm, sx, sy, None).tolist() == [0]


def test_argument_errors():
    from joint_tensorf_amd import _lib, ops
    L = _lib.lib
    v = torch.zeros(4, 3, device=DEV)
    w, nrm, st = torch.empty_like(v), torch.empty_like(v), torch.empty(4, device=DEV, dtype=torch.uint8)
    p = _lib.ptr
    good = dict(vertices=p(v), normals=p(v), n=4, sx=1.0, sy=1.0, near=1.0, max_depth=0.0, world=p(w), wn=p(nrm), status=p(st))

    def call(**kw):
        a = dict(good, **kw)
        return L.jt_mesh_unwarp_ndc(a["vertices"], a["normals"], a["n"], a["sx"], a["sy"], a["near"], a["max_depth"], a["world"], a["wn"],
                                    a["status"], None)
    assert call() == 0
    for bad in (dict(vertices=None), dict(world=None), dict(status=None), dict(wn=None), dict(n=0), dict(n=-1), dict(sx=0.0),
                dict(sx=-1.0), dict(sx=float("inf")), dict(sx=float("nan")), dict(sy=0.0), dict(sy=float("inf")), dict(sy=float("nan")),
                dict(near=0.0), dict(near=-1.0), dict(near=float("inf")), dict(near=float("nan")), dict(max_depth=float("nan"))):
        assert call(**bad) == 1, bad
    assert call(normals=None, wn=None) == 0                            # no normals: neither array is touched
    assert call(n=1 << 31) == 2
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.ndc_to_world(v[:0], 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        ops.ndc_to_world(v, 1.0, 1.0, 1.0, normals=v[:2])
    with pytest.raises(ValueError):
        ops.ndc_to_world(v, 1.0, 1.0, 1.0, max_depth=0.0)
    with pytest.raises(_lib.JtError):
        ops.ndc_to_world(v, 0.0, 1.0, 1.0)
    # the compaction entries
    tri = torch.zeros(2, 3, device=DEV, dtype=torch.int32)
    b = torch.zeros(4, device=DEV, dtype=torch.uint8)
    o = torch.zeros(4, device=DEV, dtype=torch.int64)
    assert L.jt_mesh_filter_count(None, 2, p(st), 4, p(b), p(b), p(b), None) == 1
    assert L.jt_mesh_filter_count(p(tri), 0, p(st), 4, p(b), p(b), p(b), None) == 1
    assert L.jt_mesh_filter_count(p(tri), 2, p(st), 0, p(b), p(b), p(b), None) == 1
    assert L.jt_mesh_filter_count(p(tri), 1 << 30, p(st), 4, p(b), p(b), p(b), None) == 2
    assert L.jt_mesh_filter_emit(p(v), None, None, 4, p(tri), 2, p(b), p(b), p(o), None, 1, 1, p(w), None, None, p(tri), None) == 1
    assert L.jt_mesh_filter_emit(p(v), None, None, 4, p(tri), 2, p(b), p(b), p(o), p(o), 5, 1, p(w), None, None, p(tri), None) == 1
    assert L.jt_mesh_filter_emit(p(v), p(v), None, 4, p(tri), 2, p(b), p(b), p(o), p(o), 1, 1, p(w), None, None, p(tri), None) == 1
    assert L.jt_mesh_filter_emit(p(v), None, None, 4, p(tri), 2, p(b), p(b), p(o), p(o), 0, 0, None, None, None, None, None) == 0
    torch.cuda.synchronize()
