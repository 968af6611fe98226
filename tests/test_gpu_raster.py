"""The device rasteriser (csrc/jt_raster.hip through ops.raster_project / raster_draw / raster_resolve and ops.rasterize) against the
NumPy statement of its contract, tests/raster_ref.py.  Every case hands the GPU's own fp32 `screen` to the reference, so the
projection's rounding cannot move a snap: coverage and status are then compared bit for bit.

U = 2^-24 is one fp32 rounding (half an ulp, relative).  The bounds, each a count of roundings:
  projection  x = fl(xw / w) with xw, w three fmaf each: |dx| <= U (3 Sx / |w| + |x| (3 Sw / |w| + 1)), S the sum of the absolute
              terms of the row; 1/w: |dq| <= U q (3 Sw / |w| + 1); w: 3 U Sw -- all times (1 + 2^-10) for the second order.
  depth       q = fl(num / fl(sum b)), num three roundings over positive terms, the b conversions one each: 6 U, and 1 / q one more:
              8 U depth is asserted.
  attributes  out = fmaf(l1, a1 - a0, fmaf(l2, a2 - a0, a0)), l_k = fl(w_k / den): w_k two roundings, den four, the quotient one, the
              difference one: 8 U |a_k - a0| per term; each fmaf one rounding of a value between the attributes: 2 U max |a|.
              With D = max a - min a over the mesh: (16 D + 2 max |a|) U (1 + 2^-10).  A constant has a_k - a0 = 0: it is exact."""
import numpy as np
import pytest
import torch

from tests import mesh_ref as M
from tests import raster_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SLACK = 1 + 2.0 ** -10


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _run(scene, cull=False, attrs=None, background=0.0, near=1e-3):
    """the three calls on one scene (every view of scene["proj"]): numpy arrays of everything they wrote"""
    from joint_tensorf_amd import ops
    V, T = _dev(scene["vertices"], np.float32), _dev(scene["triangles"], np.int32)
    P = _dev(np.asarray(scene["proj"], dtype=np.float32).reshape(-1, 3, 4))
    screen = ops.raster_project(V, P, near)
    zbuf, status = ops.raster_draw(screen, T, scene["H"], scene["W"], cull)
    tri, depth, out = ops.raster_resolve(zbuf, screen, T, None if attrs is None else _dev(attrs, np.float32), background)
    assert tri.dtype == torch.int32 and depth.dtype == torch.float32 and status.dtype == torch.uint8 and zbuf.dtype == torch.int64
    return dict(screen=screen.cpu().numpy(), zbuf=zbuf.cpu().numpy(), status=status.cpu().numpy(), tri=tri.cpu().numpy(),
                depth=depth.cpu().numpy(), out=None if out is None else out.cpu().numpy())


def _reference(scene, got, view=0, cull=False, attrs=None, background=0.0):
    return R.rasterize(got["screen"][view], scene["triangles"], scene["H"], scene["W"], cull=cull, attrs=attrs, background=background)


def test_projection():
    """screen = (x, y, 1/w, w) of 1 000 random vertices under 3 views against fp64, within the bound of the module docstring"""
    from joint_tensorf_amd import ops
    g = np.random.default_rng(0)
    v = (2 * g.random((1000, 3)) - 1).astype(np.float32)
    proj = []
    for k in range(3):
        Q = np.linalg.qr(g.standard_normal((3, 3)))[0]
        Q = Q * np.sign(np.linalg.det(Q))
        K = np.array([[60.0 + 10 * k, 0, 24.0], [0, 55.0, 20.0 + k], [0, 0, 1]])
        proj.append(K @ np.concatenate([Q, np.array([[0.1 * k], [-0.2], [4.0]])], 1))      # |Q v| <= sqrt(3) < 4: w > 2
    proj = np.asarray(proj, dtype=np.float32)
    got = ops.raster_project(_dev(v), _dev(proj), 1e-3).cpu().numpy().astype(np.float64)
    want = R.project(v, proj)
    assert got.shape == want.shape == (3, 1000, 4) and (want[..., 3] > 2).all()
    P, v64 = proj.astype(np.float64), v.astype(np.float64)
    S = np.einsum("vrc,nc->vnr", np.abs(P[:, :, :3]), np.abs(v64)) + np.abs(P[:, None, :, 3])          # [3, 1000, 3]
    w = np.abs(want[..., 3])
    bound = np.stack([U * (3 * S[..., 0] / w + np.abs(want[..., 0]) * (3 * S[..., 2] / w + 1)),
                      U * (3 * S[..., 1] / w + np.abs(want[..., 1]) * (3 * S[..., 2] / w + 1)),
                      U * want[..., 2] * (3 * S[..., 2] / w + 1), 3 * U * S[..., 2]], -1) * SLACK
    err = np.abs(got - want)
    for c, name in enumerate(("x", "y", "1/w", "w")):
        print("projection %s: largest error %.3e, its bound %.3e, worst error / bound %.3f"
              % (name, err[..., c].max(), bound[..., c].flat[err[..., c].argmax()], (err[..., c] / bound[..., c]).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize("name", sorted(R.COVERAGE_SCENES))
def test_coverage_bit_for_bit(name):
    """one triangle in 16 x 16; the fan in 32 x 32; one triangle larger than a 24 x 40 image with every vertex off screen (the
    cooperative path, the clipped box, H != W); 130 triangles, two of them full-screen (large and small in one wave, a count that
    is no multiple of 64): `tri` and `status` equal the reference's, both windings"""
    scene = R.COVERAGE_SCENES[name]()
    for flip in (False, True):
        s = dict(scene, triangles=np.ascontiguousarray(scene["triangles"][:, ::-1]) if flip else scene["triangles"])
        got = _run(s)
        ref = _reference(s, got)
        assert R.near_ties(ref).sum() == 0
        assert np.array_equal(got["status"][0], ref["status"]), name
        assert np.array_equal(got["tri"][0], ref["tri"]), (name, int((got["tri"][0] != ref["tri"]).sum()))
        assert (ref["tri"] >= 0).sum() > 0
        assert np.array_equal(np.isinf(got["depth"][0]), ref["tri"] < 0) and (got["zbuf"][0][ref["tri"] < 0] == -1).all()
    if name == "fan":
        assert ref["cover"].max() == 1 and got["tri"][0][16, 16] >= 0
    if name == "big":
        assert 0 < (got["tri"][0] >= 0).sum() < 24 * 40


@pytest.mark.parametrize("name", sorted(R.DEPTH_SCENES))
def test_depth_order(name):
    """two parallel layers, the same triangle submitted twice (and once more as a copy), two triangles through each other.  `tri`
    may differ from the reference only where its best and second-best q lie within 1e-5 relative, at no more than 4 pixels of a
    scene; the copies of one triangle tie exactly and the lowest index has to win everywhere."""
    scene = R.DEPTH_SCENES[name]()
    got = _run(scene)
    ref = _reference(scene, got)
    assert np.array_equal(got["status"][0], ref["status"]) and (ref["status"] == R.DRAWN).all()
    differ = got["tri"][0] != ref["tri"]
    if name == "duplicate":
        assert not differ.any() and set(np.unique(got["tri"][0])) == {-1, 0}
        assert (ref["cover"][ref["tri"] >= 0] == 3).all()
        return
    ties = R.near_ties(ref)
    print("%s: %d covered pixels, %d near ties, %d pixels differ" % (name, int((ref["tri"] >= 0).sum()), int(ties.sum()), int(differ.sum())))
    assert ties.sum() <= R.MAX_NEAR_TIES
    assert not (differ & ~ties).any()
    overlap = ref["cover"] == 2
    assert overlap.sum() > 20
    # layers: the nearer layer (triangles 2, 3) hides the farther wherever both lie; crossing: each wins on its own side
    assert set(np.unique(ref["tri"][overlap])) == ({0, 1} if name == "crossing" else {2, 3})
    ok = ~ties & (ref["tri"] >= 0)
    assert (np.abs(got["depth"][0][ok] - ref["depth"][ok]) <= 8 * U * ref["depth"][ok]).all()


def _tilted_quad():
    K = np.array([[30.0, 0, 16.0], [0, 30.0, 16.0], [0, 0, 1]])
    proj = (K @ np.eye(3, 4)).astype(np.float32)
    V = np.array([(-1.0, -1.0, 2.0), (1.2, -0.9, 2.5), (1.1, 1.0, 5.0), (-0.9, 1.1, 4.0)], dtype=np.float32)
    return dict(vertices=V, triangles=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), proj=proj, H=32, W=32)


def test_attributes():
    """a quad tilted in depth carrying (world x, a constant): perspective-correct against fp64 within the module docstring's bound,
    the constant to 1 ulp; the background, depth = +inf and tri = -1 where nothing was drawn"""
    scene = _tilted_quad()
    const = np.float32(0.7)
    attrs = np.stack([scene["vertices"][:, 0], np.full(4, const)], -1).astype(np.float32)
    bg = (-2.0, 0.25)
    got = _run(scene, attrs=attrs, background=bg)
    ref = _reference(scene, got, attrs=attrs, background=bg)
    assert np.array_equal(got["tri"][0], ref["tri"]) and R.near_ties(ref).sum() == 0
    hit = ref["tri"] >= 0
    assert 100 < hit.sum() < 32 * 32
    a = attrs[:, 0].astype(np.float64)
    bound = (16 * (a.max() - a.min()) + 2 * np.abs(a).max()) * U * SLACK
    err = np.abs(got["out"][0][..., 0] - ref["out"][..., 0])[hit].max()
    print("attribute error %.3e (bound %.3e)" % (err, bound))
    assert err <= bound
    # perspective-correct, not screen-linear: the two differ by far more than the bound somewhere on this quad
    span = got["out"][0][..., 0][hit]
    assert span.min() < -0.5 and span.max() > 0.5
    assert (np.abs(got["out"][0][..., 1][hit] - const) <= np.spacing(const)).all()
    assert (got["out"][0][~hit] == np.float32(bg)).all()
    assert np.isposinf(got["depth"][0][~hit]).all() and (got["tri"][0][~hit] == -1).all()
    assert (np.abs(got["depth"][0][hit] - ref["depth"][hit]) <= 8 * U * ref["depth"][hit]).all()
    assert 2.0 <= got["depth"][0][hit].min() and got["depth"][0][hit].max() <= 5.0


def _dropped_scene():
    """triangle 0 (positive screen area: a back face) and 1 (the same, reversed: a front face) are visible; the rest must go"""
    nan = float("nan")
    pts = [(2, 2, 1), (10, 2, 1), (2, 10, 1),                       # 0-2   the visible triangle
           (5, 5, 1), (6, 6, 1), (7, 7, 1),                         # 3-5   collinear: zero area
           (5.0001, 5, 1), (5.0002, 5.0001, 1), (5.0003, 5, 1),     # 6-8   collapses when snapped
           (3, 3, -1), (9, 3, -1), (3, 9, -1),                      # 9-11  behind the camera
           (4, 12, -0.5),                                           # 12    with 0, 1: straddles near
           (20000, 4, 1),                                           # 13    with 0, 2: beyond the guard band (16 384 pixels)
           (4, 4, 1e-4)]                                            # 14    with 0, 1: in front of the camera, nearer than near
    V = R.lift(pts)
    V = np.concatenate([V, np.array([[nan, 1.0, 1.0], [1.0, 1.0, np.inf]], dtype=np.float32)])      # 15, 16: not finite
    T = np.array([[0, 1, 2], [0, 2, 1], [3, 4, 5], [6, 7, 8], [9, 10, 11], [0, 1, 12], [0, 13, 2], [0, 1, 14], [0, 1, 15],
                  [16, 1, 2]], dtype=np.int32)
    want = [R.DRAWN, R.DRAWN, R.EMPTY, R.EMPTY, R.NEAR, R.NEAR, R.GUARD_BAND, R.NEAR, R.NEAR, R.NEAR]
    return dict(vertices=V, triangles=T, proj=R.PERSP, H=16, W=16), want


def test_dropped_geometry():
    from joint_tensorf_amd import ops
    scene, want = _dropped_scene()
    for cull in (False, True):
        got = _run(scene, cull=cull)
        ref = _reference(scene, got, cull=cull)
        expect = [R.CULLED] + want[1:] if cull else want
        assert list(got["status"][0]) == expect == list(ref["status"]), cull
        assert np.array_equal(got["tri"][0], ref["tri"])
        assert set(np.unique(got["tri"][0])) == ({-1, 1} if cull else {-1, 0})       # equal q: the lower index, unless it is culled
    # none of the dropped ones writes a pixel: alone, and the culled one alone
    only = dict(scene, triangles=scene["triangles"][2:])
    got = _run(only)
    assert list(got["status"][0]) == want[2:] and (got["zbuf"] == -1).all() and (got["tri"] == -1).all()
    got = _run(dict(scene, triangles=scene["triangles"][:1]), cull=True)
    assert list(got["status"][0]) == [R.CULLED] and (got["zbuf"] == -1).all()
    # the counts of ops.rasterize: [V, 5] int64 on the device, summing to the triangle count
    for cull, counts in ((False, [2, 5, 1, 2, 0]), (True, [1, 5, 1, 2, 1])):
        r = ops.rasterize(_dev(scene["vertices"]), _dev(scene["triangles"]), _dev(scene["proj"][None]), 16, 16, cull=cull)
        assert r.status_counts.device.type == torch.device(DEV).type and r.status_counts.dtype == torch.int64 and r.attrs is None
        assert r.status_counts.tolist() == [counts] and sum(counts) == len(scene["triangles"])


def _three_views():
    scene = R.mixed_scene(seed=3)
    views = [np.array([[s, 0, tx], [0, s, ty], [0, 0, 1]]) @ R.PERSP.astype(np.float64)
             for s, tx, ty in ((1.0, 0.0, 0.0), (0.8, 3.5, -1.25), (1.3, -6.0, -4.5))]
    return dict(scene, proj=np.asarray(views, dtype=np.float32))


def test_batching_and_determinism():
    """V = 3 in one call equals three single-view calls bit for bit, whatever views_per_call; two runs give the same z-buffer"""
    from joint_tensorf_amd import ops
    scene = _three_views()
    attrs = np.random.default_rng(5).random((len(scene["vertices"]), 3)).astype(np.float32)
    whole = _run(scene, attrs=attrs, background=0.5)
    again = _run(scene, attrs=attrs, background=0.5)
    assert np.array_equal(whole["zbuf"], again["zbuf"]) and (whole["tri"] >= 0).sum() > 2000
    for v in range(3):
        one = _run(dict(scene, proj=scene["proj"][v]), attrs=attrs, background=0.5)
        for k in ("screen", "zbuf", "status", "tri", "depth", "out"):
            assert np.array_equal(one[k][0], whole[k][v]), (v, k)
        assert np.array_equal(whole["tri"][v], _reference(scene, whole, view=v)["tri"])
    assert not np.array_equal(whole["tri"][0], whole["tri"][1])
    V, T, P, A = _dev(scene["vertices"]), _dev(scene["triangles"]), _dev(scene["proj"]), _dev(attrs)
    runs = [ops.rasterize(V, T, P, 32, 32, attrs=A, background=0.5, views_per_call=n) for n in (1, 2, 8)]
    for r in runs:
        assert np.array_equal(r.tri.cpu().numpy(), whole["tri"]) and np.array_equal(r.depth.cpu().numpy(), whole["depth"])
        assert np.array_equal(r.attrs.cpu().numpy(), whole["out"])
        assert r.status_counts.tolist() == [np.bincount(whole["status"][v], minlength=5).tolist() for v in range(3)]
    assert whole["status"].shape == (3, 130) and (whole["status"][0] == R.DRAWN).sum() > 120


def _look_at(eye, target, focal, H, W):
    """(proj [3, 4] fp32, R [3, 3], eye) of a camera at `eye` looking at `target`: x right, y down, z forward"""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]])
    return (K @ np.concatenate([Rm, -(Rm @ eye)[:, None]], 1)).astype(np.float32), Rm, eye


def test_sphere():
    """mesh_ref.sphere_field on a 24^3 lattice through ops.mesh_from_lattice, drawn at 48 x 48 from two poses.  With e the radial
    bound L^2 / (8 (r - L)) + 1e-5 of test_gpu_mesh.py::test_sphere: a pixel whose ray passes within r - e of the centre is covered,
    one beyond r + e is not, and on rays within 0.9 r of the centre (cosine of the incidence angle >= 0.43) the depth agrees with
    the analytic intersection within e / 0.43."""
    from joint_tensorf_amd import ops
    shape, c, r = (24, 24, 24), np.array((0.05, -0.03, 0.1)), 0.6
    vol = M.sphere_field(shape, c, r)
    V, T = ops.mesh_from_lattice(_dev(vol), 0.0, M.BOX_LO, M.BOX_HI)
    L = float(np.linalg.norm((np.array(M.BOX_HI) - np.array(M.BOX_LO)) / (np.array(shape) - 1)))
    e = L * L / (8 * (r - L)) + 1e-5
    H = W = 48
    focal = 100.0
    cams = [_look_at(c + np.array(d), c + np.array(o), focal, H, W)
            for d, o in (((3.2, 0.4, 0.9), (0.0, 0.0, 0.0)), ((-1.1, -2.9, -1.2), (0.03, -0.02, 0.04)))]
    drawn = ops.rasterize(V, T, _dev(np.stack([cam[0] for cam in cams])), H, W)
    culled = ops.rasterize(V, T, _dev(np.stack([cam[0] for cam in cams])), H, W, cull=True)
    counts = drawn.status_counts.cpu().numpy()
    # nothing is behind the camera or far off screen; a sliver may collapse when it is snapped
    assert (counts[:, 0] + counts[:, 3] == T.shape[0]).all() and (counts[:, 0] > 0.9 * T.shape[0]).all() and counts[:, [1, 2, 4]].sum() == 0
    jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    for v, (proj, Rm, eye) in enumerate(cams):
        # the rays the projection belongs to, from the fp32 matrix itself: d = M^-1 (x, y, 1) with M the left 3 x 3 block
        P = proj.astype(np.float64)
        Minv = np.linalg.inv(P[:, :3])
        o = -Minv @ P[:, 3]
        d = np.stack([ii, jj, np.ones_like(ii)], -1) @ Minv.T                      # unit depth along the camera axis: s is w
        oc = o - c
        A, B, C = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - r * r
        dist = np.linalg.norm(np.cross(np.broadcast_to(oc, d.shape), d), axis=-1) / np.sqrt(A)
        tri, depth = drawn.tri[v].cpu().numpy(), drawn.depth[v].cpu().numpy().astype(np.float64)
        inside, outside, core = dist <= r - e, dist >= r + e, dist <= 0.9 * r
        assert inside.sum() > 500 and outside.sum() > 500 and core.sum() > 400
        assert (tri[inside] >= 0).all() and (tri[outside] < 0).all()
        s = (-B - np.sqrt(np.where(core, B * B - 4 * A * C, 0.0))) / (2 * A)
        err = np.abs(depth - s)[core].max()
        print("view %d: %d pixels covered, depth error %.5f (bound %.5f)" % (v, int((tri >= 0).sum()), err, e / 0.43))
        assert err <= e / 0.43
        # a closed surface seen from outside turns about half its triangles away
        n_culled = int(culled.status_counts[v, 4])
        assert 0.3 * T.shape[0] < n_culled < 0.7 * T.shape[0] and int(culled.status_counts[v].sum()) == T.shape[0]
        # ... and what stays is the near side: the winding number of a closed oriented surface leaves one front face over every
        # pixel inside the outline
        middle = dist <= 0.5 * r
        assert (culled.tri[v].cpu().numpy()[middle] >= 0).all()
        assert (np.abs(culled.depth[v].cpu().numpy().astype(np.float64) - s)[middle] <= e / 0.43).all()
