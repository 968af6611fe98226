"""Mesh simplification on the GPU (csrc/jt_simplify.hip through ops.simplify_mesh, TensorVMSplit.extract_mesh(simplify=),
Model.export_scene and `python -m joint_tensorf_amd.export --simplify.cell=K`) against the NumPy statement of its contract,
tests/simplify_ref.py, on the SAME fp32 inputs: the GPU's own mesh_from_lattice vertices plus fp32 normals.

Everything is compared exactly: counts, the order of the clusters, counts', the triangle integers, the two drop counts, and the
BITS of positions and normals.  The keys are four correctly rounded fp32 operations; positions and normals are fixed sequences of
correctly rounded fp64 additions, multiplications, divisions and one square root (contraction off), which IEEE 754 defines to the
bit -- NumPy on the host computes the same ones in the same order."""
import json
import os

import numpy as np
import pytest
import torch

from tests import simplify_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
_MESHES = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mesh(name):
    """(V float32 [nv, 3], T int32 [nt, 3], N float32 [nv, 3], lo, hi, lattice shape): the GPU's mesh of a lattice of
    simplify_ref.LATTICES with the analytic normals at its vertices, computed once and never modified"""
    if name not in _MESHES:
        from joint_tensorf_amd import ops
        vol, lo, hi, level, normals = S.LATTICES[name]()
        V, T = ops.mesh_from_lattice(torch.from_numpy(np.ascontiguousarray(vol)).to(DEV), level, lo.tolist(), hi.tolist())
        V, T = V.cpu().numpy(), T.cpu().numpy()
        _MESHES[name] = (V, T, normals(V.astype(np.float64)).astype(np.float32), lo, hi, vol.shape)
    return _MESHES[name]


def _gpu(V, T, N, lo, hi, cells, **kw):
    from joint_tensorf_amd import ops
    out = ops.simplify_mesh(torch.from_numpy(np.ascontiguousarray(V)).to(DEV), torch.from_numpy(np.ascontiguousarray(T)).to(DEV),
                            torch.from_numpy(np.ascontiguousarray(N)).to(DEV), [float(v) for v in lo], [float(v) for v in hi],
                            cells, **kw)
    Vo, To, No, Co, drops = out
    assert Vo.is_cuda and Vo.dtype == torch.float32 and To.dtype == torch.int32 and No.dtype == torch.float32 and Co.dtype == torch.int32
    assert Vo.dim() == 2 and Vo.shape[1] == 3 and To.dim() == 2 and To.shape[1] == 3 and No.shape == Vo.shape and Co.shape == Vo.shape[:1]
    return Vo.cpu().numpy(), To.cpu().numpy(), No.cpu().numpy(), Co.cpu().numpy(), tuple(drops)


def _check(V, T, N, lo, hi, cells, label="", **kw):
    """the GPU's simplification against the reference's, exactly; returns (gpu result, reference result)"""
    ref = S.simplify(V, T, N, lo, hi, cells, **({"lam": kw["regular"]} if "regular" in kw else {}))
    got = _gpu(V, T, N, lo, hi, cells, **kw)
    print("%s cells %s: %d / %d -> %d / %d, dropped %s, largest cluster %d"
          % (label, cells, len(V), len(T), len(got[0]), len(got[1]), got[4], got[3].max() if len(got[3]) else 0))
    assert (len(got[0]), len(got[1])) == (len(ref[0]), len(ref[1])), label
    assert got[4] == ref[4], (label, got[4], ref[4])
    assert np.array_equal(got[3], ref[3]), label                              # members per vertex, in cluster order
    assert np.array_equal(got[1], ref[1]), label                              # the triangle integers
    pos = _bits(got[0]) != _bits(ref[0])
    assert not pos.any(), (label, "positions", int(pos.sum()), got[0][pos.any(-1)][:4], ref[0][pos.any(-1)][:4])
    nrm = _bits(got[2]) != _bits(ref[2])
    assert not nrm.any(), (label, "normals", int(nrm.sum()), got[2][nrm.any(-1)][:4], ref[2][nrm.any(-1)][:4])
    return got, ref


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("name", ["sphere", "torus", "cube"])
def test_lattice_meshes_equal_the_reference_bit_for_bit(name, K):
    V, T, N, lo, hi, shape = _mesh(name)
    got, ref = _check(V, T, N, lo, hi, S.cells_for(shape, K), "%s K=%d" % (name, K))
    assert S.edge_balance(got[1]) and 0 < len(got[0]) < len(V)
    if (name, K) == ("sphere", 4):
        assert len(V) % 64 != 0 and ref[3].max() > 64                         # a cluster of more members than a wave has lanes


def test_two_runs_give_the_same_bits():
    V, T, N, lo, hi, shape = _mesh("torus")
    a, b = _gpu(V, T, N, lo, hi, S.cells_for(shape, 3)), _gpu(V, T, N, lo, hi, S.cells_for(shape, 3))
    assert len(a[0]) > 50
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4]


def _cloud(n, cells, seed):
    """a random soup: n vertices in [0, 1]^3 with one at the centre of each of the `cells` cells along x, unnormalised random
    normals, n random triangles"""
    rng = np.random.default_rng(seed)
    V = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    V[:cells, 0] = (np.arange(cells) + 0.5) / cells
    N = rng.normal(size=(n, 3)).astype(np.float32)
    T = rng.integers(0, n, size=(n, 3)).astype(np.int32)
    return V, T, N


def test_65_clusters_and_a_regulariser_of_its_own():
    V, T, N = _cloud(333, 65, seed=5)
    for lam in (S.REGULAR, 1.0 / 64.0, 3.0):
        got, ref = _check(V, T, N, (0, 0, 0), (1, 1, 1), (65, 1, 1), "65 cells, lambda %g" % lam, regular=lam)
    from joint_tensorf_amd import ops
    keys = ops.simplify_keys(torch.from_numpy(V).to(DEV), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (65, 1, 1)).cpu().numpy()
    assert len(np.unique(keys)) == 65 and np.array_equal(keys, S.cell_keys(V, (0, 0, 0), (1, 1, 1), (65, 1, 1)))
    _check(V, T, N, (0, 0, 0), (1, 1, 1), (3, 5, 7), "3 x 5 x 7 cells")


def test_one_cell_collapses_everything():
    V, T, N, lo, hi, shape = _mesh("cube")
    Vo, To, No, Co, drops = _gpu(V, T, N, lo, hi, (1, 1, 1))
    assert Vo.shape == (0, 3) and To.shape == (0, 3) and No.shape == (0, 3) and Co.shape == (0,) and drops == (0, len(T))
    assert Vo.dtype == np.float32 and To.dtype == np.int32


def test_finest_cells_return_the_mesh_itself():
    V, T, N, lo, hi, shape = _mesh("sphere")
    cells = (1 << 20,) * 3
    (Vo, To, No, Co, drops), ref = _check(V, T, N, lo, hi, cells, "2^20 cells")
    assert len(Vo) == len(V) and len(To) == len(T) and drops == (0, 0) and (Co == 1).all()
    keys = S.cell_keys(V, lo, hi, cells)
    perm = np.argsort(keys, kind="stable")                                    # output vertex j is input vertex perm[j]
    assert np.array_equal(_bits(Vo), _bits(V[perm]))                          # positions come back exactly
    assert np.abs(No - N[perm]).max() <= 2.0 ** -23                           # (a normal is normalised again, in fp64: one fp32 ulp)
    assert np.array_equal(perm[To], T)                                        # the triangles, unchanged under the permutation


def test_vertices_on_and_beyond_the_box():
    lo, hi = (-1.0, 0.0, 2.0), (1.0, 4.0, 3.0)
    V = np.float32([[-1, 0, 2], [1, 4, 3], [-7, 2, 2.5], [9, 2, 2.5], [0, -3, 2.5], [0, 40, 2.5], [0, 2, -1e30], [0, 2, 3e38],
                    [0.5, 1, 2.25], [-0.5, 3, 2.75]])
    N = np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]])
    T = np.int32([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 0, 5], [2, 3, 6], [1, 7, 9], [4, 8, 0], [2, 2, 5]])
    from joint_tensorf_amd import ops
    cells = (4, 4, 4)
    keys = ops.simplify_keys(torch.from_numpy(V).to(DEV), lo, hi, cells).cpu().numpy()
    want = [0, 63, (0 * 4 + 2) * 4 + 2, (3 * 4 + 2) * 4 + 2, (2 * 4 + 0) * 4 + 2, (2 * 4 + 3) * 4 + 2, (2 * 4 + 2) * 4 + 0,
            (2 * 4 + 2) * 4 + 3, (3 * 4 + 1) * 4 + 1, (1 * 4 + 3) * 4 + 3]
    assert keys.tolist() == want and np.array_equal(keys, S.cell_keys(V, lo, hi, cells))
    got, ref = _check(V, T, N, lo, hi, cells, "on and beyond the box")
    assert got[4] == (0, 1) and len(got[0]) == 10                            # every vertex a cluster of its own, returned exactly
    got, ref = _check(V, T, N, lo, hi, (2, 1, 2), "on and beyond the box, coarse")


def test_one_nan_vertex_drops_its_triangles_and_moves_nothing_else():
    V, T, N, lo, hi, shape = _mesh("sphere")
    cells = S.cells_for(shape, 3)
    base = _gpu(V, T, N, lo, hi, cells)
    bad = 1000
    Vn = V.copy()
    Vn[bad, 1] = np.nan
    got, ref = _check(Vn, T, N, lo, hi, cells, "one NaN vertex")
    touched = (T == bad).any(axis=1)
    assert touched.sum() >= 3 and got[4][0] == int(touched.sum())            # cause 1 comes first, and is counted
    assert got[4][0] + got[4][1] + len(got[1]) == len(T)
    # the cluster that lost the vertex has one member less; every other vertex keeps its bits
    keys = S.cell_keys(V, lo, hi, cells)
    assert len(got[0]) == len(base[0]) and got[3].sum() == base[3].sum() - 1
    changed = np.flatnonzero(got[3] != base[3])
    assert len(changed) == 1 and base[3][changed[0]] == (keys == keys[bad]).sum() == got[3][changed[0]] + 1
    same = np.ones(len(base[0]), dtype=bool)
    same[changed] = False
    assert np.array_equal(_bits(got[0])[same], _bits(base[0])[same]) and np.array_equal(_bits(got[2])[same], _bits(base[2])[same])


def test_zero_normals_give_the_mean():
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    V = np.float32([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.12, 0.1, 0.16], [0.31, 0.2, 0.05], [0.1, 0.1, 0.9]])
    N = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [np.nan, 1, 0], [0, 0, 1]])    # (a non-finite normal counts as zero)
    T = np.int32([[0, 1, 2], [3, 1, 5], [4, 2, 5], [0, 3, 1]])
    (Vo, To, No, Co, drops), ref = _check(V, T, N, lo, hi, 2, "zero normals")
    assert drops == (0, 1) and Co.tolist() == [3, 1, 1, 1]
    mean = (V[[0, 3, 4]].astype(np.float64).sum(axis=0) / 3.0).astype(np.float32)
    assert np.array_equal(_bits(Vo[0]), _bits(mean)) and not No[0].any()
    assert np.array_equal(_bits(Vo[1:]), _bits(V[[5, 2, 1]]))                 # clusters of one member: their vertex, exactly


def _blob_scene(shaded=False):
    """the small synthetic field of tests/test_gpu_mesh.py; shaded: with the appearance branch of tests/test_gpu_surface.py's, a
    shape the record-free appearance kernel of point_colors takes"""
    from joint_tensorf_amd import synthetic, tensorf_repr
    torch.manual_seed(0)
    app = dict(appearance_n_comp=[48, 48, 48], view_pe=2, fea_pe=2) if shaded else dict(appearance_n_comp=[4, 4, 4])
    tf = tensorf_repr.TensorVMSplit([-1.0, -1.3, -0.8, 1.2, 1.1, 1.0], [20, 21, 19], DEV, density_n_comp=[8, 8, 8],
                                    app_dim=27, near_far=[2.0, 6.0], shadingMode="MLP_Fea", featureC=64, **app)
    with torch.no_grad():
        synthetic.bake_blobs(tf, n_blobs=5, seed=2)
    return tf


@pytest.mark.parametrize("shaded", [False, True])
def test_extract_mesh_simplifies_its_own_output(shaded):
    from joint_tensorf_amd import ops
    tf = _blob_scene(shaded)
    res = (17, 19, 23)
    plain = tf.extract_mesh(res=res, normals=True, colors=shaded)
    assert plain.simplified is None and plain.vertices.shape[0] > 100
    again = tf.extract_mesh(res=res, normals=True, colors=shaded, simplify=None)
    assert torch.equal(again.vertices, plain.vertices) and torch.equal(again.triangles, plain.triangles)
    assert torch.equal(again.normals, plain.normals) and (not shaded or torch.equal(again.colors, plain.colors))
    for K in (2, 2.5):
        cells = S.cells_for(plain.shape, K)
        want = ops.simplify_mesh(plain.vertices, plain.triangles, plain.normals, plain.lo, plain.hi, cells)
        mesh = tf.extract_mesh(res=res, normals=True, colors=shaded, simplify=K)
        assert 0 < mesh.vertices.shape[0] < plain.vertices.shape[0]
        assert torch.equal(mesh.vertices, want[0]) and torch.equal(mesh.triangles, want[1]) and torch.equal(mesh.normals, want[2])
        assert mesh.simplified == (tuple(cells), plain.vertices.shape[0], plain.triangles.shape[0]) + tuple(want[4])
        assert (mesh.shape, mesh.lo, mesh.hi, mesh.level) == (plain.shape, plain.lo, plain.hi, plain.level)
        assert mesh.n_degenerate_normals == int((want[2] == 0).all(-1).sum())
        if shaded:
            # colours: the field at the representative, seen against its new normal
            zero = (want[2] == 0).all(-1, keepdim=True)
            col = tf.point_colors(want[0], torch.where(zero, want[2].new_tensor([0.0, 0.0, -1.0]), -want[2]))
            assert tuple(col.shape) == tuple(want[0].shape) and torch.equal(mesh.colors, col)
        else:
            assert mesh.colors is None
        # and against the reference, on the same inputs
        _check(plain.vertices.cpu().numpy(), plain.triangles.cpu().numpy(), plain.normals.cpu().numpy(), plain.lo, plain.hi, cells,
               "blob scene K=%g" % K)
    bare = tf.extract_mesh(res=res, simplify=2)                               # normals are formed whether asked for or not
    assert bare.normals is None and bare.colors is None and bare.n_degenerate_normals is None and bare.simplified is not None
    for bad in (0.5, 0, float("nan"), float("inf"), True, "2"):
        with pytest.raises(ValueError):
            tf.extract_mesh(res=res, simplify=bad)


def test_export_with_and_without_simplify(tmp_path):
    """`python -m joint_tensorf_amd.export` in process on a small trained model: without --simplify.* the bytes of write_ply of
    the plain mesh; with --simplify.cell=3 the simplified mesh, its comment, and a PLY that reads back"""
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
            "--train_schedule.upsample_iters=[2,50]", "--camera.noise=0.15", "--surface.normals=true"]
    tf.kernel_density = None                     # (a restored checkpoint has no blur state)
    plain = tf.extract_mesh(res=res, level=0.005, cap=True, normals=True)
    # ---- without the option: byte for byte what it was ----
    out = export.main(args + ["--output_path=%s" % os.path.join(str(tmp_path), "plain")])
    comments = mesh_io.mesh_comments(plain.level, plain.shape, plain.lo, plain.hi, "world") + ["normals degenerate %d" % plain.n_degenerate_normals]
    want_path = mesh_io.write_ply(os.path.join(str(tmp_path), "want.ply"), plain.vertices, plain.triangles, comments, normals=plain.normals)
    assert open(out.mesh, "rb").read() == open(want_path, "rb").read()
    assert out.get("simplified", None) is None and not any(c.startswith("simplify") for c in mesh_io.read_ply_attributes(out.mesh)["comments"])
    # ---- with it ----
    simple = tf.extract_mesh(res=res, level=0.005, cap=True, normals=True, simplify=3.0)
    out = export.main(args + ["--simplify.cell=3", "--output_path=%s" % os.path.join(str(tmp_path), "simple")])
    got = mesh_io.read_ply_attributes(out.mesh)
    cells = tuple(S.cells_for(plain.shape, 3))
    assert ("simplify cell 3 cells %d %d %d from %d %d collapsed %d"
            % (cells + (plain.vertices.shape[0], plain.triangles.shape[0], simple.simplified[4]))) in got["comments"]
    assert out.simplified == simple.simplified and simple.simplified[0] == cells
    assert (out.n_vertices, out.n_triangles) == (len(got["vertices"]), len(got["triangles"])) == (simple.vertices.shape[0], simple.triangles.shape[0])
    assert 0 < out.n_vertices < plain.vertices.shape[0]
    assert np.array_equal(_bits(got["vertices"]), _bits(simple.vertices.cpu().numpy()))
    assert np.array_equal(got["triangles"], simple.triangles.cpu().numpy())
    assert np.array_equal(_bits(got["normals"]), _bits(simple.normals.cpu().numpy()))
    assert "normals degenerate %d" % simple.n_degenerate_normals in got["comments"]
    # read_ply round-trips: positions and triangles written again give the same file
    again = mesh_io.write_ply(os.path.join(str(tmp_path), "again.ply"), got["vertices"], got["triangles"], got["comments"], normals=got["normals"])
    assert open(again, "rb").read() == open(out.mesh, "rb").read()
    assert S.edge_balance(got["triangles"])
    # ---- the preview and its check draw and score the simplified mesh; report.json says what it was simplified from ----
    data = ["--data.synthetic=true", "--data.num_views=3", "--data.num_test_views=2"]
    out = export.main(args + data + ["--simplify.cell=2", "--preview.views=2", "--preview.size=[40,40]", "--preview.check=true",
                                     "--output_path=%s" % os.path.join(str(tmp_path), "checked")])
    report = json.load(open(out.preview.report))
    assert report["simplified"] == [list(out.simplified[0])] + list(out.simplified[1:]) and out.simplified[0] == tuple(S.cells_for(plain.shape, 2))
    assert report["n_triangles"] == out.n_triangles == plain.triangles.shape[0] - out.simplified[3] - out.simplified[4] > 0
    assert 0.0 <= report["mean"]["iou"] <= 1.0
