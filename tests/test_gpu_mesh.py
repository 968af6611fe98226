"""Mesh extraction on the GPU (csrc/jt_mesh.hip through ops.mesh_from_lattice, TensorVMSplit.extract_mesh, Model.export_scene and
`python -m joint_tensorf_amd.export`) against the NumPy / fp64 statement of its contract, tests/mesh_ref.py, on the same fp32
lattice: equal counts, vertices in the same order and within COORD_ULPS * 2^-24 * max(|lo|, |hi|) per coordinate, and the triangles
of every cell equal as sets, modulo rotation.

The coordinate bound: three fp32 roundings in t (in [0, 1]), two in the lattice coordinate, two in the lerp, each at most half an
ulp of a magnitude that does not exceed the box: 3.5 ulp, doubled for slack and rounded up to 16 * 2^-24."""
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
COORD_ULPS = 16.0


def _gpu_mesh(vol, level, lo, hi):
    from joint_tensorf_amd import ops
    V, T = ops.mesh_from_lattice(torch.from_numpy(np.ascontiguousarray(vol)).to(DEV), level, lo, hi)
    assert V.is_cuda and T.is_cuda and V.dtype == torch.float32 and T.dtype == torch.int32
    assert V.dim() == 2 and V.shape[1] == 3 and T.dim() == 2 and T.shape[1] == 3
    return V.cpu().numpy(), T.cpu().numpy()


def _check(vol, level, lo, hi, label=""):
    """the GPU mesh of a lattice against the reference's; returns (V, T) of the GPU"""
    Vr, Tr, cells = R.reference_mesh(vol, level, lo, hi, return_cells=True)
    V, T = _gpu_mesh(vol, level, lo, hi)
    assert (len(V), len(T)) == (len(Vr), len(Tr)), (label, len(V), len(Vr), len(T), len(Tr))
    tol = COORD_ULPS * 2.0 ** -24 * float(max(np.abs(np.float32(lo)).max(), np.abs(np.float32(hi)).max()))
    err = float(np.abs(V.astype(np.float64) - Vr).max()) if len(V) else 0.0
    print("%s: %d vertices, %d triangles, coordinate error %.3e (bound %.3e)" % (label, len(V), len(T), err, tol))
    assert err <= tol, (label, err, tol)
    if len(T):
        assert T.min() >= 0 and T.max() < len(V)
        starts = np.flatnonzero(np.r_[True, cells[1:] != cells[:-1], True])
        for a, b in zip(starts[:-1], starts[1:]):
            assert R.rotations_of(T[a:b]) == R.rotations_of(Tr[a:b]), (label, int(cells[a]), T[a:b], Tr[a:b])
    return V, T


def test_all_255_cell_configurations():
    for config in range(1, 256):
        vol = R.cell_configuration(config)
        Vr, Tr, cells = R.reference_mesh(vol, 0.0, (0, 0, 0), (3, 3, 3), return_cells=True)
        V, T = _gpu_mesh(vol, 0.0, (0, 0, 0), (3, 3, 3))
        assert (len(V), len(T)) == (len(Vr), len(Tr)), config
        assert np.abs(V - Vr).max() <= COORD_ULPS * 2.0 ** -24 * 3.0, config
        starts = np.flatnonzero(np.r_[True, cells[1:] != cells[:-1], True])
        for a, b in zip(starts[:-1], starts[1:]):
            assert R.rotations_of(T[a:b]) == R.rotations_of(Tr[a:b]), (config, int(cells[a]))
        t = R.topology(V, T)
        assert t["closed"] and t["oriented"] and t["volume"] > 0, (config, t)


@pytest.mark.parametrize("shape", [(9, 11, 13), (12, 12, 12)])
def test_sphere(shape):
    c, radius = np.array((0.05, -0.03, 0.1)), 0.6
    V, T = _check(R.sphere_field(shape, c, radius), 0.0, R.BOX_LO, R.BOX_HI, "sphere %s" % (shape,))
    t = R.topology(V, T)
    assert t["closed"] and t["oriented"] and t["euler"] == 2 and t["volume"] > 0
    L = float(np.linalg.norm((np.array(R.BOX_HI) - np.array(R.BOX_LO)) / (np.array(shape) - 1)))
    err = float(np.abs(np.linalg.norm(V.astype(np.float64) - c, axis=1) - radius).max())
    print("radial error %.4f, bound %.4f" % (err, L * L / (8 * (radius - L)) + 1e-5))
    assert err <= L * L / (8 * (radius - L)) + 1e-5


def test_torus_and_two_spheres():
    V, T = _check(R.torus_field((14, 15, 9)), 0.0, R.BOX_LO, R.BOX_HI, "torus")
    t = R.topology(V, T)
    assert t["closed"] and t["oriented"] and t["euler"] == 0
    V, T = _check(R.two_spheres_field((13, 8, 8)), 0.0, R.BOX_LO, R.BOX_HI, "two spheres")
    t = R.topology(V, T)
    assert t["closed"] and t["oriented"] and t["euler"] == 4


def test_values_exactly_at_the_level():
    vol, lo, hi = R.integer_sphere_field()
    V, T = _check(vol, 0.0, lo, hi, "integer sphere")
    t = R.topology(V, T)
    assert t["closed"] and t["oriented"] and t["euler"] == 2 and t["volume"] > 0


def test_surface_cut_by_the_box_and_capped():
    from joint_tensorf_amd import ops
    f = R.sphere_field((8, 9, 7), (0, 0, 0.2), 1.3)
    V, T = _check(f, 0.0, R.BOX_LO, R.BOX_HI, "cut sphere")
    t = R.topology(V, T)
    assert not t["closed"] and len(t["boundary"]) > 0
    lo, hi = np.float32(R.BOX_LO), np.float32(R.BOX_HI)

    def on_face(v):
        return bool(((v == lo) | (v == hi)).any())
    assert all(on_face(V[a]) and on_face(V[b]) for a, b in t["boundary"])
    # the capping path: the zeros shell and the grown box as extract_mesh makes them
    clamped = np.clip(f, 0, 1)
    cv, clo, chi = ops.cap_lattice(torch.from_numpy(clamped).to(DEV), R.BOX_LO, R.BOX_HI)
    rv, rlo, rhi = R.cap(clamped, R.BOX_LO, R.BOX_HI)
    assert np.array_equal(cv.cpu().numpy(), rv)
    assert np.array_equal(np.float32(clo), rlo) and np.array_equal(np.float32(chi), rhi)
    for level in (0.5, 0.05):
        V, T = _check(cv.cpu().numpy(), level, clo, chi, "capped sphere at %g" % level)
        t = R.topology(V, T)
        assert t["closed"] and t["oriented"] and t["euler"] == 2 and t["volume"] > 0, (level, t)


@pytest.mark.parametrize("shape", [(5, 6, 70), (3, 2, 257), (2, 2, 2), (2, 3, 130)])
def test_launch_edges(shape):
    """the fastest axis across 64-lane and 256-thread boundaries, neighbours in the next workgroup, nearly every cell cut"""
    vol = R.uniform_lattice(shape, seed=sum(shape))
    V, T = _check(vol, 0.0, (-1.0, -2.0, -0.5), (1.5, 2.0, 3.0), "uniform %s" % (shape,))
    assert len(T) > 2 * (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)


def test_degenerate_and_refused_inputs():
    from joint_tensorf_amd import ops
    from joint_tensorf_amd._lib import JtError
    for value in (-1.0, 1.0):
        V, T = ops.mesh_from_lattice(torch.full((4, 5, 6), value, device=DEV), 0.0, (0, 0, 0), (1, 1, 1))
        assert tuple(V.shape) == (0, 3) and tuple(T.shape) == (0, 3) and V.dtype == torch.float32 and T.dtype == torch.int32
    nan = torch.full((3, 3, 3), float("nan"), device=DEV)
    assert ops.mesh_from_lattice(nan, 0.0, (0, 0, 0), (1, 1, 1))[0].shape[0] == 0           # NaN is outside, everywhere
    nan[1, 1, 1] = 1.0                                                                        # every t is NaN: midpoints
    V, T = ops.mesh_from_lattice(nan, 0.0, (0, 0, 0), (1, 1, 1))
    assert V.shape[0] == 14 and bool(((V == 0.25) | (V == 0.5) | (V == 0.75)).all())
    t = R.topology(V.cpu().numpy(), T.cpu().numpy())
    assert t["closed"] and t["oriented"] and t["euler"] == 2
    with pytest.raises(JtError):
        ops.mesh_from_lattice(torch.zeros(1, 4, 4, device=DEV), 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(JtError):
        ops.mesh_from_lattice(torch.zeros(4, 4, 4, device=DEV), float("nan"), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        ops.mesh_from_lattice(torch.zeros(4, 4, 4, device=DEV, dtype=torch.float64), 0.0, (0, 0, 0), (1, 1, 1))
    vol = torch.from_numpy(R.uniform_lattice((7, 9, 66), seed=1)).to(DEV)
    a, b = ops.mesh_from_lattice(vol, 0.1, (0, 0, 0), (1, 2, 3)), ops.mesh_from_lattice(vol, 0.1, (0, 0, 0), (1, 2, 3))
    assert a[0].shape[0] > 1000 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _blob_scene():
    from joint_tensorf_amd import synthetic, tensorf_repr
    torch.manual_seed(0)
    tf = tensorf_repr.TensorVMSplit([-1.0, -1.3, -0.8, 1.2, 1.1, 1.0], [20, 21, 19], DEV, density_n_comp=[8, 8, 8],
                                    appearance_n_comp=[4, 4, 4], app_dim=27, near_far=[2.0, 6.0], shadingMode="MLP_Fea", featureC=64)
    with torch.no_grad():
        synthetic.bake_blobs(tf, n_blobs=5, seed=2)
    return tf


def test_extract_mesh_of_a_model():
    from joint_tensorf_amd import ops
    tf = _blob_scene()
    res = (17, 19, 23)
    alpha = tf.getDenseAlpha(res)[0]
    lo, hi = tf.aabb[0].tolist(), tf.aabb[1].tolist()
    want_v, want_t = ops.mesh_from_lattice(alpha, 0.005, lo, hi)
    mesh = tf.extract_mesh(res=res, cap=False, slab_points=1000)                      # eight slabs, the last one short
    assert mesh.vertices.shape[0] > 100 and torch.equal(mesh.vertices, want_v) and torch.equal(mesh.triangles, want_t)
    assert mesh.shape == res and mesh.level == 0.005 and list(mesh.lo) == lo and list(mesh.hi) == hi
    one = tf.extract_mesh(res=res, cap=False)
    assert torch.equal(one.vertices, want_v) and torch.equal(one.triangles, want_t)
    # capped: closed whatever reaches the box, inside the grown box
    capped = tf.extract_mesh(res=res, cap=True, slab_points=1000)
    assert capped.shape == (19, 21, 25)
    V, T = capped.vertices.cpu().numpy(), capped.triangles.cpu().numpy()
    t = R.topology(V, T)
    print("blob scene: %d vertices, %d triangles, euler %d, volume %.4f" % (len(V), len(T), t["euler"], t["volume"]))
    assert t["closed"] and t["oriented"] and t["volume"] > 0
    unit = (np.float32(hi) - np.float32(lo)) / (np.float32(res) - np.float32(1))
    assert np.array_equal(np.float32(capped.lo), np.float32(lo) - unit) and np.array_equal(np.float32(capped.hi), np.float32(hi) + unit)
    assert (V >= np.float32(capped.lo)).all() and (V <= np.float32(capped.hi)).all()
    # the factor grid by default, one int for a cubic lattice
    assert tf.extract_mesh(cap=False).shape == (20, 21, 19) and tf.extract_mesh(res=9).shape == (11, 11, 11)
    with pytest.raises(ValueError):
        tf.extract_mesh(res=(4, 4))
    with pytest.raises(ValueError):
        tf.extract_mesh(res=1)


def test_export_end_to_end(tmp_path):
    """a small trained model, its checkpoint, and `python -m joint_tensorf_amd.export` run in process on it"""
    from joint_tensorf_amd import export, mesh_io, synthetic
    from tests.test_gpu_metrics import _trained_small_model
    from tests.test_lifecycle import _small_opt
    opt = _small_opt(device=DEV, output_path=str(tmp_path), max_iter=5, camera=dict(noise=0.15),
                     freq=dict(scalar=2, val=100, ckpt=100), optim=dict(test_iter=3))
    m = _trained_small_model(opt)
    tf = m.graph.nerf.tensorf
    with torch.no_grad():
        synthetic.bake_blobs(tf, n_blobs=5, seed=2)
    ckpt = m.save_checkpoint(opt, ep=0, it=5, latest=True)
    res = [15, 14, 13]
    args = ["--yaml=bat_blender_VM", "--load=%s" % ckpt, "--device=%s" % DEV, "--mesh.res=%s" % json.dumps(res),
            "--data.image_size=[32,32]", "--train_schedule.n_voxel_init=1000", "--train_schedule.n_voxel_final=4096",
            "--train_schedule.upsample_iters=[2,50]", "--camera.noise=0.15"]
    data = ["--data.synthetic=true", "--data.num_views=3", "--data.num_test_views=2"]
    out_dir = os.path.join(str(tmp_path), "export")
    out = export.main(args + data + ["--output_path=%s" % out_dir])
    # the mesh: what the field in memory gives without the blur state its last training forward left (a restored checkpoint has none)
    tf.kernel_density = None
    want = tf.extract_mesh(res=res, level=0.005, cap=True)
    V, T, comments = mesh_io.read_ply(os.path.join(out_dir, "mesh.ply"))
    assert out.mesh == os.path.join(out_dir, "mesh.ply") and (out.n_vertices, out.n_triangles) == (len(V), len(T))
    assert len(V) > 50 and np.array_equal(V, want.vertices.cpu().numpy()) and np.array_equal(T, want.triangles.cpu().numpy())
    assert "space world" in comments and "lattice 17 16 15" in comments and "level 0.005" in comments
    assert "box_lo %r %r %r" % tuple(want.lo) in comments and "box_hi %r %r %r" % tuple(want.hi) in comments
    t = R.topology(V, T)
    assert t["closed"] and t["oriented"] and t["volume"] > 0
    # the cameras: one entry per training view, in the frame of the mesh, with the alignment to the dataset's frame
    cams = mesh_io.read_cameras(os.path.join(out_dir, "cameras.json"))
    assert out.cameras == os.path.join(out_dir, "cameras.json")
    assert cams["space"] == "world" and cams["n_views"] == len(cams["views"]) == len(m.train_data) == 3
    assert cams["image_size"] == [32, 32] and [v["idx"] for v in cams["views"]] == [0, 1, 2]
    with torch.no_grad():
        pose, pose_GT = m.get_all_training_poses(opt)
        aligned, sim3 = m.prealign_cameras(opt, pose, pose_GT)
    got = np.array([v["pose"] for v in cams["views"]], dtype=np.float32)
    assert got.shape == (3, 3, 4) and np.abs(got - pose.cpu().numpy()).max() <= 4 * 2.0 ** -23 * max(1.0, float(pose.abs().max()))
    assert np.abs(got - pose_GT.cpu().numpy()).max() > 1e-3                          # the refined poses, not the dataset's
    np.testing.assert_allclose(np.array([v["pose_aligned"] for v in cams["views"]], dtype=np.float32), aligned.cpu().numpy(), atol=1e-5)
    np.testing.assert_array_equal(np.array([v["intr"] for v in cams["views"]], dtype=np.float32), m.train_data.all.intr.cpu().numpy())
    for k in ("t0", "t1", "s0", "s1", "R"):
        np.testing.assert_allclose(np.array(cams["sim3"][k], dtype=np.float32), torch.as_tensor(sim3[k]).cpu().numpy(), atol=1e-5, err_msg=k)
    # without an image set: the same mesh, no cameras
    bare_dir = os.path.join(str(tmp_path), "bare")
    bare = export.main(args + ["--output_path=%s" % bare_dir])
    assert bare.cameras is None and sorted(os.listdir(bare_dir)) == ["mesh.ply"]
    assert open(bare.mesh, "rb").read() == open(out.mesh, "rb").read()
