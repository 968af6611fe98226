"""The visible-surface stage on the GPU (csrc/jt_visible.hip through ops.triangle_visibility / grow_triangles / select_triangles,
TensorVMSplit.extract_mesh(visible=), Model.export_scene and `python -m joint_tensorf_amd.export --visible.*`) against the NumPy
statement of its contract, tests/visible_ref.py.

Everything is integers and bits: nothing here has a tolerance.  The tally's reference input is the device's OWN winner buffer,
ops.rasterize(...).tri (tests/test_gpu_raster.py::test_depth_order tolerates near-tie pixels between the NumPy rasteriser and the
device; a rasteriser restatement would not isolate the new kernels), except for the nested cubes, where tests/test_visible_ref.py
shows on the CPU that there is no near tie and what every count must be."""
import json
import os

import numpy as np
import pytest
import torch

from tests import raster_ref as R
from tests import visible_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tally_forms(fn):
    """fn() with the tally adding once per run of a wave (the default) and once per pixel (JT_VISIBLE_RUNS=0, read at every call)"""
    old = os.environ.pop("JT_VISIBLE_RUNS", None)
    try:
        runs = fn()
        os.environ["JT_VISIBLE_RUNS"] = "0"
        plain = fn()
    finally:
        os.environ.pop("JT_VISIBLE_RUNS", None)
        if old is not None:
            os.environ["JT_VISIBLE_RUNS"] = old
    return runs, plain


def _visibility(V, T, P, H, W, **kw):
    from joint_tensorf_amd import ops
    vis = ops.triangle_visibility(_dev(V), _dev(T), _dev(P), H, W, **kw)
    assert vis.views.dtype == torch.int32 and vis.pixels.dtype == torch.int64 and vis.views.shape == vis.pixels.shape == (len(T),)
    return vis.views.cpu().numpy(), vis.pixels.cpu().numpy(), vis.status_counts.cpu().numpy()


# ---- nested cubes ------------------------------------------------------------------------------------------------------------
def test_nested_cubes():
    from joint_tensorf_amd import ops
    V, T = VR.nested_cubes()
    P, H, W = VR.cube_views(), VR.CUBE_H, VR.CUBE_W
    assert (H * W) % 64 != 0                                                      # waves straddle rows and views
    tri = ops.rasterize(_dev(V), _dev(T), _dev(P), H, W).tri.cpu().numpy()
    for form, (views, pixels, counts) in zip(("runs", "plain"), _tally_forms(lambda: _visibility(V, T, P, H, W))):
        print("\n[cubes, %s] views %s pixels %s" % (form, views.tolist(), pixels.tolist()))
        assert counts.tolist() == [[24, 0, 0, 0, 0]] * 4                          # all 24 are drawn in every view
        assert views.tolist() == [2] * 12 + [0] * 12
        assert np.array_equal(pixels, VR.tally(tri, 24)[1]) and not pixels[12:].any()
    assert _visibility(V, T, P, H, W, min_pixels=21)[0].tolist() == [2] * 12 + [0] * 12
    assert _visibility(V, T, P, H, W, min_pixels=94)[0].tolist() == [0] * 24      # sees nothing
    Vd, Td = _dev(V), _dev(T)
    opts = ops.visible_options(dict(proj=_dev(P), H=H, W=W, min_views=1))
    kept, seen = ops.visible_triangles(Vd, Td, opts)
    assert kept.tolist() == seen.tolist() == [1] * 12 + [0] * 12
    v, t, n, c, dropped = ops.select_triangles(Vd, Td, kept)
    assert dropped == 12 and n is None and c is None
    assert v.cpu().numpy().tobytes() == V[:8].tobytes() and t.cpu().numpy().tobytes() == T[:12].tobytes()    # the outer cube, in order
    kept, seen = ops.visible_triangles(Vd, Td, ops.visible_options(dict(proj=_dev(P), H=H, W=W, min_views=3)))
    v, t, n, c, dropped = ops.select_triangles(Vd, Td, kept, normals=Vd)
    assert dropped == 24 and tuple(v.shape) == tuple(t.shape) == tuple(n.shape) == (0, 3)
    assert v.dtype == torch.float32 and t.dtype == torch.int32


# ---- the tally against the reference ---------------------------------------------------------------------------------------------
def _three_views():
    """raster_ref.mixed_scene() under three cameras; the third looks past the edge of the two triangles that cover the screen"""
    scene = R.mixed_scene()
    views = [np.array([[s, 0, tx], [0, s, ty], [0, 0, 1]]) @ R.PERSP.astype(np.float64)
             for s, tx, ty in ((1.0, 0.0, 0.0), (0.8, 3.5, -1.25), (0.5, -10.0, -10.0))]
    return dict(scene, proj=np.asarray(views, dtype=np.float32))


def test_tally_equals_the_reference_however_the_views_are_batched():
    from joint_tensorf_amd import ops
    s = _three_views()
    V, T, P, H, W = s["vertices"], s["triangles"], s["proj"], s["H"], s["W"]
    tri = ops.rasterize(_dev(V), _dev(T), _dev(P), H, W).tri.cpu().numpy()
    assert len(T) == 130 and (tri < 0).sum() > 500 and (tri >= 0).sum() > 2000    # background pixels are present
    want_v, want_p = VR.tally(tri, len(T))
    assert want_p.sum() == (tri >= 0).sum() and 2 < (want_v > 0).sum() < len(T)
    for n in (1, 2, 8):
        for views, pixels, _ in _tally_forms(lambda: _visibility(V, T, P, H, W, views_per_call=n)):
            assert views.tobytes() == want_v.tobytes() and pixels.tobytes() == want_p.tobytes(), n
    # min_pixels exactly equal to a triangle's count in a view is counted, one more is not: the smallest count of at least 2
    per_view = np.stack([VR.tally(tri[v:v + 1], len(T))[1] for v in range(3)])
    k = int(per_view[per_view >= 2].min())
    v0, t = (int(x) for x in np.argwhere(per_view == k)[0])
    at_k, above = _visibility(V, T, P, H, W, min_pixels=k), _visibility(V, T, P, H, W, min_pixels=k + 1)
    print("\n[tally] triangle %d wins exactly %d pixels in view %d: views %d at min_pixels %d, %d at %d"
          % (t, k, v0, at_k[0][t], k, above[0][t], k + 1))
    for m, (views, pixels, _) in ((k, at_k), (k + 1, above)):
        assert views.tobytes() == VR.tally(tri, len(T), min_pixels=m)[0].tobytes() and pixels.tobytes() == want_p.tobytes()
        assert views[t] == (per_view[:, t] >= m).sum()
    assert at_k[0][t] == above[0][t] + (per_view[:, t] == k).sum() and at_k[0][t] >= 1


def test_one_triangle_over_two_whole_views():
    """one triangle covers every pixel of a 300 x 300 image in two consecutive views: 90000 winners per view (past 2^16), and the
    run of equal indices continues across the view boundary in memory (90000 is no multiple of 64) but must be split there"""
    V = R.flat([(-400.0, -300.0), (1000.0, -300.0), (-400.0, 1100.0)])
    T = np.array([[0, 1, 2]], dtype=np.int32)
    P = np.stack([R.ORTHO, R.ORTHO])
    assert 90000 % 64 != 0
    for views, pixels, counts in _tally_forms(lambda: _visibility(V, T, P, 300, 300)):
        assert counts.tolist() == [[1, 0, 0, 0, 0]] * 2
        assert pixels.tolist() == [180000] and views.tolist() == [2]
    assert _visibility(V, T, P, 300, 300, min_pixels=90000)[0].tolist() == [2]
    assert _visibility(V, T, P, 300, 300, min_pixels=90001)[0].tolist() == [0]


def test_tally_of_a_hand_made_buffer():
    """the kernel on a z-buffer written by the test: runs of every length over three views of 33 x 70, runs that continue across
    the view boundaries, empty pixels, and low words that are no triangle; and a buffer left all-ones"""
    from joint_tensorf_amd import ops
    rng = np.random.default_rng(11)
    Vn, H, W, nt = 3, 33, 70, 9
    n = Vn * H * W
    low = np.repeat(rng.integers(0, nt + 3, size=n), rng.integers(1, 150, size=n))[:n].astype(np.int64)    # nt .. nt + 2: no triangle
    low[H * W - 40:H * W + 40] = 4                                                # one run over the first boundary
    low[2 * H * W - 3:2 * H * W + 1] = nt + 1                                     # and a skipped one over the second
    high = rng.integers(0, 1 << 31, size=n).astype(np.int64)
    key = (high << 32) | low
    empty = rng.random(n) < 0.2
    key[empty] = -1
    key[100:300] = -1
    tri = np.where(empty | (np.arange(n) >= 100) & (np.arange(n) < 300), -1, low).reshape(Vn, H, W)
    want_v, want_p = VR.tally(tri, nt, min_pixels=5)
    assert want_p.sum() > 0 and (tri >= nt).any()
    zbuf = _dev(key.reshape(Vn, H, W))

    def run():
        pix = ops.visible_tally(zbuf, nt)
        views = torch.zeros(nt, device=DEV, dtype=torch.int32)
        pixels = torch.zeros(nt, device=DEV, dtype=torch.int64)
        ops.visible_fold(pix, 5, views, pixels)
        ops.visible_fold(pix, 5, views, pixels)                                   # in and out: a second call adds again
        return pix.cpu().numpy(), views.cpu().numpy(), pixels.cpu().numpy()
    for pix, views, pixels in _tally_forms(run):
        assert np.array_equal(pix, np.stack([VR.tally(tri[v:v + 1], nt)[1] for v in range(Vn)]).astype(np.int32))
        assert np.array_equal(views, 2 * want_v) and np.array_equal(pixels, 2 * want_p)
    blank = torch.full((2, 17, 31), -1, device=DEV, dtype=torch.int64)
    for pix in _tally_forms(lambda: ops.visible_tally(blank, 5).cpu().numpy()):
        assert pix.shape == (2, 5) and not pix.any()


# ---- grow --------------------------------------------------------------------------------------------------------------------
def test_grow_on_a_strip():
    from joint_tensorf_amd import ops
    nv, T = VR.strip(10)
    seed = np.zeros(len(T), dtype=np.uint8)
    seed[0] = 1
    for rings in (0, 1, 2, 20):
        got = ops.grow_triangles(_dev(T), nv, _dev(seed), rings)
        assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == VR.grow(T, nv, seed, rings).tobytes(), rings
        assert not got[10:].any()                                                 # the two bad triangles never enter
    assert ops.grow_triangles(_dev(T), nv, _dev(seed), 20).tolist() == [1] * 10 + [0, 0]
    assert ops.grow_triangles(_dev(T), nv, _dev(seed).bool(), 1).tolist() == [1, 1, 1] + [0] * 9
    bad = np.zeros(len(T), dtype=np.uint8)
    bad[10:] = 1                                                                  # ... and never flag a vertex
    assert ops.grow_triangles(_dev(T), nv, _dev(bad), 5).cpu().numpy().tobytes() == bad.tobytes() == VR.grow(T, nv, bad, 5).tobytes()
    odd = np.uint8([0, 0, 0, 0, 0, 7, 0, 0, 0, 0, 0, 0])                          # rings = 0 returns its input's bits
    assert ops.grow_triangles(_dev(T), nv, _dev(odd), 0).tolist() == odd.tolist()
    assert ops.grow_triangles(_dev(T), nv, _dev(odd), 1).cpu().numpy().tobytes() == VR.grow(T, nv, odd, 1).tobytes()
    # more than one workgroup
    rng = np.random.default_rng(3)
    Tb = rng.integers(0, 4000, size=(3001, 3)).astype(np.int32)
    Tb[17, 1], Tb[2999, 0] = -1, 4000
    sb = (rng.random(3001) < 0.01).astype(np.uint8)
    for rings in (1, 2):
        assert ops.grow_triangles(_dev(Tb), 4000, _dev(sb), rings).cpu().numpy().tobytes() == VR.grow(Tb, 4000, sb, rings).tobytes()


# ---- select ------------------------------------------------------------------------------------------------------------------
def test_select_on_a_soup():
    from joint_tensorf_amd import ops
    rng = np.random.default_rng(9)
    nv, nt = 700, 500
    V = rng.normal(size=(nv, 3)).astype(np.float32)
    N, C = rng.normal(size=(nv, 3)).astype(np.float32), rng.random((nv, 3)).astype(np.float32)
    T = rng.integers(0, nv, size=(nt, 3)).astype(np.int32)
    T[5, 2], T[77, 0] = nv, -2
    keep = (rng.random(nt) < 0.4).astype(np.uint8)
    keep[[5, 77]] = 1
    want = VR.select(V, T, keep, N, C)
    got = ops.select_triangles(_dev(V), _dev(T), _dev(keep), normals=_dev(N), colors=_dev(C))
    assert got[4] == want[4] == nt - int(keep.sum()) + 2 and 0 < len(want[0]) < nv
    assert np.array_equal(got[1].cpu().numpy(), want[1]) and got[1].dtype == torch.int32
    for g, w in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
        assert np.array_equal(_bits(g), _bits(w))
    again = ops.select_triangles(_dev(V), _dev(T), _dev(keep).bool(), normals=_dev(N), colors=_dev(C))
    assert all(torch.equal(a, b) for a, b in zip(got[:4], again[:4])) and again[4] == got[4]
    # all ones on a mesh without unused vertices: the input's bits
    Tu = np.concatenate([np.arange(nv - nv % 3, dtype=np.int32).reshape(-1, 3), [[nv - 3, nv - 2, nv - 1]]]).astype(np.int32)
    v, t, n, c, dropped = ops.select_triangles(_dev(V), _dev(Tu), torch.ones(len(Tu), device=DEV, dtype=torch.uint8), normals=_dev(N))
    assert dropped == 0 and c is None and t.cpu().numpy().tobytes() == Tu.tobytes()
    assert np.array_equal(_bits(v), _bits(V)) and np.array_equal(_bits(n), _bits(N))
    # all zeros: empties
    v, t, n, c, dropped = ops.select_triangles(_dev(V), _dev(T), torch.zeros(nt, device=DEV, dtype=torch.uint8), colors=_dev(C))
    assert dropped == nt and n is None and tuple(v.shape) == tuple(t.shape) == tuple(c.shape) == (0, 3)


# ---- invariance: what is culled was never in a picture ---------------------------------------------------------------------------
_SCENE = {}


def _blob_mesh():
    """the blob field of tests/test_gpu_simplify.py on a 17 x 19 x 23 lattice with its normals, and four cameras at 64 x 48, all
    on the +x side of it: the far side is in no picture"""
    if not _SCENE:
        from tests.test_gpu_simplify import _blob_scene
        tf = _blob_scene()
        mesh = tf.extract_mesh(res=(17, 19, 23), normals=True)
        H, W = 64, 48
        eyes = ((4.2, 0.6, 0.9), (3.6, -2.2, -0.4), (3.9, 1.8, -1.1), (2.9, -0.3, 2.6))
        P = np.stack([VR.look_at(e, (0.1, -0.1, 0.1), 90.0, H, W) for e in eyes])
        _SCENE.update(tf=tf, mesh=mesh, P=_dev(P), H=H, W=W)
    return _SCENE


@pytest.mark.parametrize("grow", [0, 1])
def test_culling_changes_no_pixel(grow):
    from joint_tensorf_amd import ops
    s = _blob_mesh()
    mesh, P, H, W = s["mesh"], s["P"], s["H"], s["W"]
    V, T, N = mesh.vertices, mesh.triangles, mesh.normals
    before = ops.rasterize(V, T, P, H, W, attrs=N)
    assert before.status_counts[:, 1:3].sum() == 0 and (before.tri >= 0).float().mean() > 0.1
    opts = ops.visible_options(dict(proj=P, H=H, W=W, min_views=1, min_pixels=1, grow=grow))
    kept, seen = ops.visible_triangles(V, T, opts)
    tri = before.tri.cpu().numpy()
    want_seen = (VR.tally(tri, T.shape[0])[0] >= 1).astype(np.uint8)
    assert seen.cpu().numpy().tobytes() == want_seen.tobytes()
    assert kept.cpu().numpy().tobytes() == VR.grow(T.cpu().numpy(), V.shape[0], want_seen, grow).tobytes()
    v, t, n, _, dropped = ops.select_triangles(V, T, kept, normals=N)
    print("\n[invariance] grow %d: %d of %d triangles seen, %d kept, %d dropped" % (grow, int(seen.sum()), T.shape[0], t.shape[0], dropped))
    assert dropped > 0 and t.shape[0] == T.shape[0] - dropped == int(kept.sum()) >= int(seen.sum()) > 0
    after = ops.rasterize(v, t, P, H, W, attrs=n)
    assert np.array_equal(_bits(after.depth), _bits(before.depth)) and np.array_equal(_bits(after.attrs), _bits(before.attrs))
    old = torch.nonzero(kept).view(-1).cpu().numpy()                              # new triangle index -> old
    new_tri = after.tri.cpu().numpy()
    assert np.array_equal(np.where(new_tri >= 0, old[np.maximum(new_tri, 0)], -1), tri)


# ---- extract_mesh(visible=) --------------------------------------------------------------------------------------------------------
def test_extract_mesh_culls_before_colours_and_texture():
    from joint_tensorf_amd import ops
    from tests.test_gpu_simplify import _blob_scene
    tf = _blob_scene(shaded=True)
    s = _blob_mesh()
    P, H, W = s["P"], s["H"], s["W"]
    res = (17, 19, 23)
    plain = tf.extract_mesh(res=res, normals=True)
    assert plain.visible is None
    again = tf.extract_mesh(res=res, normals=True, visible=None)
    assert again.visible is None and torch.equal(again.vertices, plain.vertices) and torch.equal(again.triangles, plain.triangles)
    assert torch.equal(again.normals, plain.normals)
    for grow in (0, 2):
        vis = dict(proj=P, H=H, W=W, grow=grow)
        kept, seen = ops.visible_triangles(plain.vertices, plain.triangles, ops.visible_options(vis))
        want = ops.select_triangles(plain.vertices, plain.triangles, kept, normals=plain.normals)
        mesh = tf.extract_mesh(res=res, normals=True, colors=True, texture=4, visible=vis)
        n_views, h, w, min_views, min_pixels, g, cull, nv_in, nt_in, n_seen, n_grown, n_dropped = mesh.visible
        assert (n_views, h, w, min_views, min_pixels, g, cull) == (4, H, W, 1, 1, grow, False)
        assert (nv_in, nt_in) == (plain.vertices.shape[0], plain.triangles.shape[0])
        assert n_seen == int(seen.sum()) <= n_grown == int(kept.sum()) and n_grown + n_dropped == nt_in and n_dropped == want[4] > 0
        assert torch.equal(mesh.vertices, want[0]) and torch.equal(mesh.triangles, want[1]) and torch.equal(mesh.normals, want[2])
        # colours and the atlas are evaluated on what is returned
        assert mesh.texture.layout.n_triangles == n_grown == mesh.triangles.shape[0]
        assert tuple(mesh.colors.shape) == tuple(mesh.vertices.shape) and mesh.vertices.shape[0] < nv_in
        zero = (want[2] == 0).all(-1, keepdim=True)
        assert torch.equal(mesh.colors, tf.point_colors(want[0], torch.where(zero, want[2].new_tensor([0.0, 0.0, -1.0]), -want[2])))
        assert mesh.n_degenerate_normals == int((want[2] == 0).all(-1).sum())
    # after simplify: the mask is decided on the simplified mesh
    simple = tf.extract_mesh(res=res, normals=True, simplify=2)
    mesh = tf.extract_mesh(res=res, normals=True, simplify=2, visible=dict(proj=P, H=H, W=W, grow=1, cull=True))
    assert mesh.simplified == simple.simplified and mesh.visible[6] is True
    assert mesh.visible[7:9] == (simple.vertices.shape[0], simple.triangles.shape[0]) and mesh.visible[10] == mesh.triangles.shape[0]
    # nothing is seen: an empty mesh, not an error
    none = tf.extract_mesh(res=res, normals=True, colors=True, texture=4, visible=dict(proj=P, H=H, W=W, min_pixels=H * W + 1))
    assert tuple(none.vertices.shape) == tuple(none.triangles.shape) == tuple(none.colors.shape) == (0, 3) and none.texture is None
    assert none.visible[9:] == (0, 0, plain.triangles.shape[0])
    with pytest.raises(ValueError):
        tf.extract_mesh(res=res, visible=dict(proj=P, H=H, W=W, min_views=0))


# ---- NDC ---------------------------------------------------------------------------------------------------------------------------
def test_ndc_mask_is_decided_on_the_world_space_copy():
    from joint_tensorf_amd import mesh_io, ops
    from tests import test_gpu_ndc_mesh as G
    v, t, _, _ = G._blob_mesh()
    poses, K = G._cameras()
    H, W = 4 * G.H, 4 * G.W
    proj = mesh_io.projection_matrices(torch.from_numpy(poses).float().to(DEV), torch.from_numpy(K).float().to(DEV).expand(3, 3, 3),
                                       size=(H, W), image_size=(G.H, G.W))
    world, _, status = ops.ndc_to_world(v, G.SX, G.SY, G.NEAR)
    bad = status != 0
    bad_tri = bad[t.long()].any(-1).cpu().numpy()
    assert 0 < bad_tri.sum() < len(bad_tri)                                       # the far cap lies behind infinity
    draw = torch.where(bad[:, None], torch.full_like(world, float("nan")), world)
    drawn = ops.rasterize(draw, t, proj, H, W)
    tri = drawn.tri.cpu().numpy()
    assert not np.isin(tri[tri >= 0], np.flatnonzero(bad_tri)).any()              # such a triangle is not drawn
    for grow in (0, 1, 3):
        kept, seen = ops.visible_triangles(v, t, ops.visible_options(dict(proj=proj, H=H, W=W, grow=grow, ndc=(G.SX, G.SY, G.NEAR))))
        want_seen = (VR.tally(tri, t.shape[0])[0] >= 1).astype(np.uint8)
        grown = VR.grow(t.cpu().numpy(), v.shape[0], want_seen, grow)
        assert seen.cpu().numpy().tobytes() == want_seen.tobytes() and want_seen.sum() > 0
        assert kept.cpu().numpy().tobytes() == (grown * ~bad_tri).astype(np.uint8).tobytes()
        assert not kept.cpu().numpy()[bad_tri].any()                              # never kept, however far the rings reach
    assert (grown.astype(bool) & bad_tri).any()                                   # (three rings do reach one)
    # the mask is applied to the mesh in the frame it lives in: the kept vertices are the NDC ones, bit for bit
    got = ops.select_triangles(v, t, kept)
    want = VR.select(v.cpu().numpy(), t.cpu().numpy(), kept.cpu().numpy())
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1].cpu().numpy(), want[1]) and got[4] == want[4] > 0


# ---- export_scene ---------------------------------------------------------------------------------------------------------------------
VISIBLE = ["--visible.views=all", "--visible.size=[48,40]", "--visible.grow=1"]


def test_export_with_and_without_visible(tmp_path_factory, tmp_path):
    from joint_tensorf_amd import export, mesh_io
    from tests.test_gpu_ndc_export import _restored_model
    from tests.test_gpu_preview import RES, _export_args
    root, args, data = _export_args(tmp_path_factory)
    # ---- without the option: the bytes of an export that never heard of it, twice ----
    a = export.main(args + data + ["--output_path=%s" % os.path.join(str(tmp_path), "a")])
    b = export.main(args + data + ["--output_path=%s" % os.path.join(str(tmp_path), "b")])
    assert a.get("visible", None) is None and open(a.mesh, "rb").read() == open(b.mesh, "rb").read()
    opt, m = _restored_model(args + data)
    assert "visible" not in opt and m.visible_arg(opt) == {}
    plain = m.graph.nerf.tensorf.extract_mesh(res=RES, level=0.005, cap=True)
    want_path = mesh_io.write_ply(os.path.join(str(tmp_path), "want.ply"), plain.vertices, plain.triangles,
                                  mesh_io.mesh_comments(plain.level, plain.shape, plain.lo, plain.hi, "world"))
    assert open(a.mesh, "rb").read() == open(want_path, "rb").read()
    assert not any(c.startswith("visible") for c in mesh_io.read_ply_attributes(a.mesh)["comments"])
    # ---- with it ----
    out = export.main(args + data + VISIBLE + ["--preview.views=2", "--preview.size=[40,40]", "--preview.check=true",
                                               "--output_path=%s" % os.path.join(str(tmp_path), "seen")])
    again = export.main(args + data + VISIBLE + ["--output_path=%s" % os.path.join(str(tmp_path), "seen_again")])
    assert open(out.mesh, "rb").read() == open(again.mesh, "rb").read() and out.visible == again.visible
    opt, m = _restored_model(args + data + VISIBLE)
    arg = m.visible_arg(opt)["visible"]
    assert tuple(arg["proj"].shape) == (3, 3, 4) and (arg["H"], arg["W"], arg["grow"], arg["ndc"]) == (48, 40, 1, None)
    mesh = m.graph.nerf.tensorf.extract_mesh(res=RES, level=0.005, cap=True, visible=arg)
    assert tuple(out.visible) == tuple(mesh.visible) and mesh.visible[:7] == (3, 48, 40, 1, 1, 1, False)
    got = mesh_io.read_ply_attributes(out.mesh)
    line = ("visible views %d size %d %d min_views %d min_pixels %d grow %d cull %d from %d %d seen %d grown %d dropped %d"
            % tuple(int(x) for x in mesh.visible))
    assert line in got["comments"]
    report = json.load(open(out.preview.report))
    assert report["visible"] == [int(x) for x in mesh.visible] and report["n_triangles"] == out.n_triangles == mesh.visible[10]
    assert mesh.visible[7:9] == (plain.vertices.shape[0], plain.triangles.shape[0])
    assert mesh.visible[9] <= mesh.visible[10] and mesh.visible[10] + mesh.visible[11] == mesh.visible[8] and mesh.visible[11] > 0
    assert np.array_equal(_bits(got["vertices"]), _bits(mesh.vertices)) and np.array_equal(got["triangles"], mesh.triangles.cpu().numpy())
    print("\n[export] " + line)


def test_export_refuses_visible_without_a_training_set(tmp_path_factory, tmp_path):
    from joint_tensorf_amd import checkpoint, export
    from joint_tensorf_amd.model import bat_hip
    from tests.test_gpu_preview import _export_args
    root, args, data = _export_args(tmp_path_factory)
    with pytest.raises(SystemExit) as e:
        export.main(args + ["--output_path=%s" % tmp_path, "--visible.views=2"])
    assert "image set" in str(e.value)
    opt = export.build_options(args + ["--visible.views=2", "--output_path=%s" % tmp_path])
    m = bat_hip.Model(opt)
    weight = checkpoint._load(opt.load, "cpu")["graph"].get("se3_refine.weight")
    m.build_networks(opt, n_views=1 if weight is None else int(weight.shape[0]))
    m.restore_checkpoint(opt)
    target = os.path.join(str(tmp_path), "never")
    with pytest.raises(ValueError) as e:
        m.export_scene(opt, target)
    assert "training set" in str(e.value) and not os.path.exists(target)
    assert not any("mesh.ply" in names for _, _, names in os.walk(str(tmp_path)))        # before any file is written
    for bad in (["--visible.grow=2"], ["--visible.views=-1"], ["--visible.views=2", "--visible.min_views=0"],
                ["--visible.views=2", "--visible.size=[0,4]"], ["--visible.views=2", "--visible.cull=1"]):
        with pytest.raises(SystemExit):
            export.build_options(args + bad)
    with pytest.raises(KeyError):
        export.build_options(args + ["--visible.rings=2"])


def test_ndc_export_stays_in_ndc_unless_carried_out(tmp_path_factory, tmp_path):
    """a camera.ndc scene: the mask is decided in world space and applied in NDC; with --texture.block the atlas is of the kept
    triangles; --frame.space=world carries the culled mesh out afterwards, and finds nothing left to drop behind infinity"""
    from joint_tensorf_amd import export, mesh_io
    from tests.test_gpu_ndc_export import _export_args
    root, args = _export_args(tmp_path_factory)
    vis = ["--visible.views=all", "--visible.size=[64,64]"]
    plain = export.main(args + ["--output_path=%s" % os.path.join(str(tmp_path), "plain")])
    ndc = export.main(args + vis + ["--texture.block=4", "--output_path=%s" % os.path.join(str(tmp_path), "ndc")])
    world = export.main(args + vis + ["--frame.space=world", "--output_path=%s" % os.path.join(str(tmp_path), "world")])
    p, a, w = mesh_io.read_ply_attributes(plain.mesh), mesh_io.read_ply_textured(ndc.mesh), mesh_io.read_ply_attributes(world.mesh)
    assert "space ndc" in a["comments"] and "space world" in w["comments"]
    assert tuple(ndc.visible) == tuple(world.visible) and ndc.visible[:3] == (3, 64, 64)
    n_seen, n_grown, n_dropped = ndc.visible[9:]
    assert 0 < n_seen <= n_grown == ndc.n_triangles and n_grown + n_dropped == plain.n_triangles and n_dropped > 0
    assert ndc.texture is not None and "texture block 4 atlas %d %d" % (ndc.texture.width, ndc.texture.height) in a["comments"]
    assert ndc.texture.width == mesh_io.texture_layout(n_grown, 4).width
    # in NDC: every written vertex is a vertex of the plain NDC export, bit for bit and in order
    all_rows, j = [r.tobytes() for r in _bits(p["vertices"])], 0
    for r in _bits(a["vertices"]):
        j = all_rows.index(r.tobytes(), j) + 1                                    # (a ValueError when it is not there, or out of order)
    assert 0 < len(a["vertices"]) < len(all_rows)
    # carried out: nothing at or beyond infinity was kept
    assert world.unwarp.n_dropped_beyond == 0 and world.n_triangles == n_grown and np.isfinite(w["vertices"]).all()
    assert plain.get("visible", None) is None
