"""Depth-map fusion on the GPU (csrc/jt_fusion.hip through mesh_ops.fusion_integrate / fusion_lattice / mesh_from_fused_lattice,
TensorVMSplit.extract_mesh(fusion=), Model.export_scene and `python -m joint_tensorf_amd.export --fusion.*`) against the NumPy
float32 statement of its contract, tests/fusion_ref.py: the state and the lattice bit for bit, the plane of
tests/test_fusion_ref.py within the bound derived there."""
import json
import os

import numpy as np
import pytest
import torch

from tests import fusion_ref as FR
from tests import mesh_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fuse(shape, depth, opacity, proj, lo, hi, trunc, slab=None, min_views=1, **kw):
    from joint_tensorf_amd import mesh_ops
    state = mesh_ops.fusion_state(shape, DEV)
    depth, opacity, proj = _dev(depth), _dev(opacity), _dev(proj)
    step = depth.shape[0] if slab is None else slab
    for v0 in range(0, depth.shape[0], step):
        mesh_ops.fusion_integrate(state, depth[v0:v0 + step], opacity[v0:v0 + step], proj[v0:v0 + step], lo, hi, trunc, **kw)
    return state + mesh_ops.fusion_lattice(state, min_views)


def _sphere():
    """the sphere scene and its reference states, computed once: {(carve, min_views): (sum, count, lattice, seen)}"""
    if "sphere" not in _CACHE:
        depth, opacity, proj, trunc = FR.sphere_scene()
        lo, hi = FR.SPHERE_BOX
        want = {}
        for carve in (True, False):
            acc, count = FR.integrate(*FR.state(FR.SPHERE_SHAPE), depth, opacity, proj, lo, hi, trunc, carve=carve)
            for mv in (1, 2):
                want[(carve, mv)] = (acc, count) + FR.finish(acc, count, mv)
        _CACHE["sphere"] = (depth, opacity, proj, trunc, want)
    return _CACHE["sphere"]


def _same(got, want):
    acc, count, lattice, seen = (g.cpu().numpy() for g in got)
    assert np.array_equal(_bits(acc), _bits(want[0])) and np.array_equal(count, want[1])
    assert np.array_equal(_bits(lattice), _bits(want[2])) and np.array_equal(seen, want[3]) and seen.dtype == np.uint8


@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("min_views", [1, 2])
def test_bit_for_bit_against_the_reference(carve, min_views):
    depth, opacity, proj, trunc, want = _sphere()
    lo, hi = FR.SPHERE_BOX
    w = want[(carve, min_views)]
    # the scene exercises every branch: points in front of and behind cameras, in and out of frames, carved, occluded, clamped
    # (with carve a point in all five frames counts five views; without, the sphere hides itself from at least one camera)
    assert 0 < (w[3] == 0).sum() < w[3].size and w[1].max() == (5 if carve else 4) and (w[2] > 0.5).any()
    assert (w[2][w[3] != 0] < 0.5).any()
    assert not np.isfinite(depth).all()
    _same(_fuse(FR.SPHERE_SHAPE, depth, opacity, proj, lo, hi, trunc, carve=carve, min_views=min_views), w)


@pytest.mark.parametrize("slab", [1, 2, 5])
def test_slabs_compose_to_the_bits_of_one_call(slab):
    depth, opacity, proj, trunc, want = _sphere()
    lo, hi = FR.SPHERE_BOX
    _same(_fuse(FR.SPHERE_SHAPE, depth, opacity, proj, lo, hi, trunc, slab=slab), want[(True, 1)])


def test_the_plane_through_the_kernels():
    """tests/test_fusion_ref.py's plane through jt_fusion_* and jt_mesh_*: the bound derived in fusion_ref.plane_bound covers the
    fp32 interpolation of jt_mesh_emit"""
    from joint_tensorf_amd import mesh_ops
    depth, opacity, proj, trunc = FR.plane_scene()
    lo, hi = FR.PLANE_BOX
    acc, count, lattice, seen = _fuse(FR.PLANE_SHAPE, depth, opacity, proj, lo, hi, trunc)
    want = FR.fuse(FR.PLANE_SHAPE, depth, opacity, proj, lo, hi, trunc)
    _same((acc, count, lattice, seen), want)
    v, t, (n_emitted, n_unobserved) = mesh_ops.mesh_from_fused_lattice(lattice, seen, 0.5, lo, hi)
    full_v, full_t = mesh_ops.mesh_from_lattice(lattice, 0.5, lo, hi)
    assert n_emitted == t.shape[0] > 0 and n_unobserved > 0 and n_emitted + n_unobserved == full_t.shape[0]
    dz = (v[:, 2].double() - FR.PLANE_Z).abs().max().item()
    print("\n[plane] %d of %d triangles kept, |z - 0.1| at most %.2f u, bound %.0f u"
          % (n_emitted, full_t.shape[0], dz / 2.0 ** -24, FR.plane_bound() / 2.0 ** -24))
    assert dz <= FR.plane_bound()
    # every kept triangle's owner cell is fully seen, recomputed from `seen`: the reference's owners, the reference's rule
    V, T, owner = MR.reference_mesh(want[2], 0.5, lo, hi, return_cells=True)
    keep = FR.keep_triangles(owner, want[3])
    assert np.array_equal(full_t.cpu().numpy(), T) and keep.sum() == n_emitted
    rv, rt = FR.select(full_v.cpu().numpy(), T, keep)
    assert np.array_equal(t.cpu().numpy(), rt) and np.array_equal(_bits(v), _bits(rv))
    # two calls: the same bits
    v2, t2, _ = mesh_ops.mesh_from_fused_lattice(lattice, seen, 0.5, lo, hi)
    assert torch.equal(v, v2) and torch.equal(t, t2)
    # everything unseen: nothing is emitted, not an error
    v0, t0, n0 = mesh_ops.mesh_from_fused_lattice(lattice, torch.zeros_like(seen), 0.5, lo, hi)
    assert tuple(v0.shape) == tuple(t0.shape) == (0, 3) and n0 == (0, full_t.shape[0])


def _blob_views():
    """the blob field of tests/test_gpu_simplify.py and six cameras round it at 40 x 40; the depth maps are those of its level-set
    mesh under the device rasteriser -- camera-axis depth where a triangle covers the pixel centre, opacity 1 there and 0 elsewhere"""
    if "blob" not in _CACHE:
        from joint_tensorf_amd import ops
        from tests.test_gpu_simplify import _blob_scene
        tf = _blob_scene(shaded=True)
        H = W = 40
        eyes = ((4.2, 0.6, 0.9), (-3.6, -2.2, -0.4), (0.3, 3.9, 1.1), (-0.9, -3.3, 2.6), (0.4, 0.2, 4.3), (1.0, -0.5, -4.0))
        P = _dev(np.stack([FR.look_at(e, (0.1, -0.1, 0.1), 40.0, H, W)[0] @ FR.look_at(e, (0.1, -0.1, 0.1), 40.0, H, W)[1]
                           for e in eyes]).astype(np.float32))
        level_set = tf.extract_mesh(res=40)
        drawn = ops.rasterize(level_set.vertices, level_set.triangles, P, H, W)
        covered = drawn.tri >= 0
        assert 0.02 < covered.float().mean() < 0.9
        _CACHE["blob"] = (tf, dict(depth=torch.where(covered, drawn.depth, torch.zeros_like(drawn.depth)), opacity=covered.float(), proj=P,
                                   H=H, W=W), level_set)
    return _CACHE["blob"]


def test_extract_mesh_with_and_without_fusion():
    tf, fusion, level_set = _blob_views()
    # ---- without: the bits of a call that never heard of the keyword ----
    plain = tf.extract_mesh(res=40, normals=True)
    again = tf.extract_mesh(res=40, normals=True, fusion=None)
    assert plain.fused is None and again.fused is None and plain.level == again.level == 0.005
    assert torch.equal(again.vertices, plain.vertices) and torch.equal(again.triangles, plain.triangles)
    assert torch.equal(again.normals, plain.normals) and torch.equal(plain.vertices, level_set.vertices)
    # ---- with ----
    mesh = tf.extract_mesh(res=40, normals=True, fusion=fusion)
    n_views, H, W, trunc, min_opacity, min_views, carve, n_seen, n_emitted, n_unobserved = mesh.fused
    assert (n_views, H, W, trunc, min_opacity, min_views, carve) == (6, 40, 40, 4.0, 0.5, 1, True)
    assert mesh.level == 0.5 and mesh.shape == (42, 42, 42) and mesh.triangles.shape[0] == n_emitted > 100 and 0 < n_seen <= 40 ** 3
    assert n_unobserved >= 0 and tuple(mesh.normals.shape) == tuple(mesh.vertices.shape)
    # the fused surface lies where the depth maps put it: within a lattice spacing or two of the level set it was rendered from
    lo, hi = torch.tensor(plain.lo, device=DEV), torch.tensor(plain.hi, device=DEV)
    assert ((mesh.vertices >= lo) & (mesh.vertices <= hi)).all()
    near = torch.cdist(mesh.vertices[::7], plain.vertices).min(1).values
    spacing = float(((hi - lo) / 41).max())
    print("\n[blob] fused %d triangles (%d unobserved dropped), level set %d; median distance to the level set %.3f spacings"
          % (n_emitted, n_unobserved, plain.triangles.shape[0], float(near.median()) / spacing))
    assert float(near.median()) < 2 * spacing
    # two runs: the same bits
    twice = tf.extract_mesh(res=40, normals=True, fusion=fusion)
    assert torch.equal(twice.vertices, mesh.vertices) and torch.equal(twice.triangles, mesh.triangles) and twice.fused == mesh.fused
    assert torch.equal(twice.normals, mesh.normals)
    # slabs, given as a generator: the same bits
    slabs = ((fusion["depth"][v:v + 4], fusion["opacity"][v:v + 4], fusion["proj"][v:v + 4]) for v in (0, 4))
    by_slab = tf.extract_mesh(res=40, normals=True, fusion=dict(slabs=slabs, H=40, W=40))
    assert torch.equal(by_slab.vertices, mesh.vertices) and torch.equal(by_slab.triangles, mesh.triangles) and by_slab.fused == mesh.fused
    # the fused lattice is what the ops make of the same maps
    from joint_tensorf_amd import mesh_ops
    vol, seen, n = tf.fused_lattice(40, mesh_ops.fusion_options(fusion))
    assert n == 6 and int(seen.sum()) == n_seen
    cap_vol, cap_lo, cap_hi = mesh_ops.cap_lattice(vol, tf.aabb[0].tolist(), tf.aabb[1].tolist())
    want = mesh_ops.mesh_from_fused_lattice(cap_vol, torch.nn.functional.pad(seen, (1,) * 6, value=1), 0.5, cap_lo, cap_hi)
    assert torch.equal(want[0], mesh.vertices) and torch.equal(want[1], mesh.triangles) and want[2] == (n_emitted, n_unobserved)
    # every later stage runs on it
    full = tf.extract_mesh(res=40, normals=True, colors=True, simplify=4, texture=4, keep_largest=1,
                           visible=dict(proj=fusion["proj"], H=40, W=40), fusion=fusion)
    assert full.fused[:8] == mesh.fused[:8] and full.level == 0.5 and full.n_components[0] == 1
    assert 0 < full.triangles.shape[0] < n_emitted and full.simplified is not None and full.visible is not None
    assert tuple(full.colors.shape) == tuple(full.vertices.shape) and full.texture.layout.n_triangles == full.triangles.shape[0]
    with pytest.raises(ValueError):
        tf.extract_mesh(res=40, level=0.5, fusion=fusion)
    with pytest.raises(ValueError):
        tf.extract_mesh(res=40, fusion=dict(fusion, min_views=0))


FUSION = ["--mesh.res=40", "--fusion.views=4", "--fusion.size=[40,40]"]


def test_export_with_and_without_fusion(tmp_path_factory, tmp_path):
    from joint_tensorf_amd import export, mesh_io
    from tests.test_gpu_ndc_export import _restored_model
    from tests.test_gpu_preview import _export_args
    root, args, data = _export_args(tmp_path_factory)
    args = [a for a in args if not a.startswith("--mesh.res")]
    # ---- without the option, before a fused export ran ----
    before = export.main(args + data + ["--mesh.res=40", "--output_path=%s" % os.path.join(str(tmp_path), "before")])
    assert before.get("fused", None) is None
    assert not any(c.startswith("fusion") for c in mesh_io.read_ply_attributes(before.mesh)["comments"])
    # ---- with it ----
    out = export.main(args + data + FUSION + ["--preview.views=2", "--preview.size=[40,40]", "--preview.check=true",
                                             "--output_path=%s" % os.path.join(str(tmp_path), "fused")])
    n_views, H, W, trunc, min_opacity, min_views, carve, n_seen, n_emitted, n_unobserved = out.fused
    assert (n_views, H, W, trunc, min_opacity, min_views, carve) == (3, 40, 40, 4.0, 0.5, 1, True)          # (the set has three views)
    got = mesh_io.read_ply_attributes(out.mesh)
    line = ("fusion views 3 size 40 40 trunc 4 min_opacity 0.5 min_views 1 carve 1 seen %d unobserved %d" % (n_seen, n_unobserved))
    assert line in got["comments"], got["comments"]
    assert out.n_triangles == n_emitted == len(got["triangles"]) > 0 and 0 < n_seen <= 40 ** 3
    assert any(c.startswith("level 0.5") or " level 0.5" in c for c in got["comments"]), got["comments"]
    report = json.load(open(out.preview.report))
    assert report["fused"] == [3, 40, 40, 4, 0.5, 1, 1, n_seen, n_emitted, n_unobserved] and report["n_triangles"] == n_emitted
    print("\n[export] " + line + "; preview: " + out.preview.summary)
    # the model's own path gives the same mesh
    opt, m = _restored_model(args + data + FUSION)
    arg = m.fusion_arg(opt)["fusion"]
    assert (arg["H"], arg["W"], arg["trunc"], arg["min_opacity"], arg["min_views"], arg["carve"]) == (40, 40, 4.0, 0.5, 1, True)
    mesh = m.graph.nerf.tensorf.extract_mesh(res=[40, 40, 40], cap=True, fusion=arg)
    assert tuple(mesh.fused) == tuple(out.fused)
    assert np.array_equal(_bits(got["vertices"]), _bits(mesh.vertices)) and np.array_equal(got["triangles"], mesh.triangles.cpu().numpy())
    assert (opt.H, opt.W) == (32, 32)                                                # (the renders put the size back)
    # ---- without it, after: byte for byte the export made before ----
    after = export.main(args + data + ["--mesh.res=40", "--output_path=%s" % os.path.join(str(tmp_path), "after")])
    assert open(after.mesh, "rb").read() == open(before.mesh, "rb").read() and after.get("fused", None) is None
    opt, m = _restored_model(args + data + ["--mesh.res=40"])
    assert "fusion" not in opt and m.fusion_arg(opt) == {}


def test_export_refuses_ndc_scenes_before_any_gpu_work(tmp_path_factory, tmp_path):
    from joint_tensorf_amd import export
    from tests.test_gpu_ndc_export import _export_args
    root, args = _export_args(tmp_path_factory)
    target = os.path.join(str(tmp_path), "never")
    with pytest.raises(SystemExit) as e:
        export.main(args + ["--fusion.views=2", "--output_path=%s" % target])
    assert "camera.ndc" in str(e.value) and not os.path.exists(target)
