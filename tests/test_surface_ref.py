"""What the surface export adds, checked without a GPU: the NumPy statement of the component contract (tests/components_ref.py) on
itself and against the mesh reference, the PLY layouts with normals and colours, the --surface.* options, and the refusals of the
new entry points."""
import numpy as np
import pytest

from tests import components_ref as C
from tests import mesh_ref as R


def _vol(points, shape=(4, 4, 4)):
    vol = -np.ones(shape, dtype=np.float32)
    for p in points:
        vol[p] = 1.0
    return vol


def test_connectivity_is_the_meshs_own():
    assert len(set(C.OFFSETS)) == 14 and (1, -1, 0) not in C.OFFSETS and (-1, -1, -1) in C.OFFSETS
    lab = C.labels(_vol([(1, 1, 1), (2, 2, 2)]), 0.0)                     # joined only by +x+y+z: one component
    assert lab[1, 1, 1] == lab[2, 2, 2] == (1 * 4 + 1) * 4 + 1 and (lab >= 0).sum() == 2
    lab = C.labels(_vol([(0, 1, 0), (1, 0, 0)]), 0.0)                     # (+x, -y) is no edge: two components
    assert lab[0, 1, 0] == 4 and lab[1, 0, 0] == 16
    lab = C.labels(_vol([(0, 0, 0), (1, 0, 0), (1, 1, 0), (3, 3, 3)]), 0.0)
    assert lab[1, 1, 0] == 0 and lab[3, 3, 3] == 63 and lab[2, 2, 2] == -1
    nan = np.full((3, 3, 3), np.nan, dtype=np.float32)
    assert (C.labels(nan, 0.0) == -1).all()


def _triangle_set(V, T):
    return sorted(tuple(V[t].reshape(-1).tolist()) for t in T)


@pytest.mark.parametrize("level,n_components", [(0.5, 20), (0.3, 10), (0.0, 3)])
def test_the_surface_splits_along_components(level, n_components):
    """the triangles of the per-component meshes, taken together, are the triangles of the whole mesh, coordinates equal to the bit"""
    vol = R.uniform_lattice((9, 8, 11), seed=1)
    lab = C.labels(vol, level)
    roots, counts = C.sizes(lab)
    V, T = R.reference_mesh(vol, level, R.BOX_LO, R.BOX_HI)
    whole = _triangle_set(V, T)
    parts = []
    for r in roots:
        Vr, Tr = R.reference_mesh(np.where((lab == r) | (lab < 0), vol, np.float32(-2.0)), level, R.BOX_LO, R.BOX_HI)
        assert len(Tr) > 0
        parts += _triangle_set(Vr, Tr)
    print("level %g: %d components (largest %d points), %d triangles" % (level, len(roots), counts.max(), len(whole)))
    assert len(roots) == n_components and sorted(parts) == whole
    # and the keep rule: the largest alone is the mesh of its own lattice
    kept, k, d = C.keep_components(vol, level, keep_largest=1, fill=-2.0)
    big = roots[np.lexsort((roots, -counts))[0]]
    assert (k, d) == (1, len(roots) - 1) and np.array_equal(kept, np.where((lab == big) | (lab < 0), vol, np.float32(-2.0)))


def test_keep_rule():
    vol = _vol([(0, 0, 0), (0, 0, 1), (2, 0, 0), (2, 0, 1), (0, 3, 3)], shape=(4, 4, 4))      # sizes 2, 2, 1; labels 0, 32, 15
    out, k, d = C.keep_components(vol, 0.0, keep_largest=1, fill=-5.0)
    assert (k, d) == (1, 2) and out[0, 0, 0] == 1 and out[2, 0, 0] == -5 and out[0, 3, 3] == -5           # the tie: the smaller label
    out, k, d = C.keep_components(vol, 0.0, min_points=2)
    assert (k, d) == (2, 1) and out[0, 3, 3] == 0 and out[2, 0, 1] == 1
    out, k, d = C.keep_components(vol, 0.0, keep_largest=3, min_points=3)
    assert (k, d) == (0, 3) and (out <= 0).all()
    assert C.keep_components(vol, 0.0)[0] is not None and C.keep_components(vol, 0.0)[1:] == (None, None)
    with pytest.raises(ValueError):
        C.keep_components(vol, 0.0, keep_largest=1, fill=0.5)


def test_keep_components_refuses_a_fill_above_the_level():
    import torch
    from joint_tensorf_amd import ops
    vol = torch.zeros(4, 4, 4)
    with pytest.raises(ValueError):
        ops.keep_components(vol, 0.0, keep_largest=1, fill=0.5)
    with pytest.raises(ValueError):
        ops.keep_components(vol, 0.0, keep_largest=0)
    with pytest.raises(ValueError):
        ops.keep_components(vol, 0.0, keep_largest=1, fill=float("nan"))
    out = ops.keep_components(vol, 0.0)                                   # nothing asked for: the lattice itself, nothing launched
    assert out[0] is vol and out[1:] == (None, None)


# ---- PLY ----------------------------------------------------------------------------------------------------------------------
def _mesh(seed=3, nv=50, nt=70):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((nv, 3)).astype(np.float32)
    T = rng.integers(0, nv, size=(nt, 3)).astype(np.int32)
    N = rng.standard_normal((nv, 3)).astype(np.float32)
    N[0] = 0.0
    Cc = rng.uniform(0, 1, size=(nv, 3)).astype(np.float32)
    return V, T, N, Cc


@pytest.mark.parametrize("with_n,with_c", [(False, False), (True, False), (False, True), (True, True)])
def test_ply_layouts_round_trip(tmp_path, with_n, with_c):
    from joint_tensorf_amd import mesh_io
    V, T, N, Cc = _mesh()
    path = mesh_io.write_ply(str(tmp_path / "m.ply"), V, T, ["space world", "components kept 1 dropped 4"],
                             normals=N if with_n else None, colors=Cc if with_c else None)
    got = mesh_io.read_ply_attributes(path)
    assert got["vertices"].tobytes() == V.tobytes() and np.array_equal(got["triangles"], T)
    assert got["comments"] == ["space world", "components kept 1 dropped 4"]
    assert (got["normals"] is not None) == with_n and (got["colors"] is not None) == with_c
    if with_n:
        assert got["normals"].dtype == np.float32 and got["normals"].tobytes() == N.tobytes()
    if with_c:
        assert got["colors"].dtype == np.uint8 and np.array_equal(got["colors"], np.floor(255.0 * Cc.astype(np.float64) + 0.5))
    head = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii").split("\n")
    props = [ln for ln in head if ln.startswith("property")]
    want = ["property float x", "property float y", "property float z"]
    want += ["property float nx", "property float ny", "property float nz"] if with_n else []
    want += ["property uchar red", "property uchar green", "property uchar blue"] if with_c else []
    assert props == want + ["property list uchar int vertex_indices"]
    if with_n or with_c:
        with pytest.raises(ValueError):
            mesh_io.read_ply(path)                                        # the three-tuple reader reads today's layout only
    else:
        plain = mesh_io.write_ply(str(tmp_path / "plain.ply"), V, T, ["space world", "components kept 1 dropped 4"])
        assert open(plain, "rb").read() == open(path, "rb").read()
        V2, T2, comments = mesh_io.read_ply(path)
        assert V2.tobytes() == V.tobytes() and np.array_equal(T2, T) and len(comments) == 2


def test_ply_plain_bytes_are_unchanged(tmp_path):
    """the file without attributes, byte for byte: header lines, 12 bytes per vertex, 13 per triangle"""
    from joint_tensorf_amd import mesh_io
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    T = np.array([[0, 1, 2]], dtype=np.int32)
    data = open(mesh_io.write_ply(str(tmp_path / "a.ply"), V, T, ["c"]), "rb").read()
    head = (b"ply\nformat binary_little_endian 1.0\ncomment c\nelement vertex 3\nproperty float x\nproperty float y\n"
            b"property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n")
    assert data == head + V.tobytes() + b"\x03" + T.tobytes()


def test_colour_quantisation_and_refusals(tmp_path):
    from joint_tensorf_amd import mesh_io
    q = mesh_io.quantise_colors(np.array([[0.0, 1.0, 0.5 / 255], [0.49999 / 255, 1.5 / 255, 254.5 / 255], [-0.2, 1.7, 0.999]]))
    assert q.dtype == np.uint8 and q.tolist() == [[0, 255, 1], [0, 2, 255], [0, 255, 255]]
    V, T, N, Cc = _mesh()
    bad = Cc.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        mesh_io.write_ply(str(tmp_path / "nan.ply"), V, T, colors=bad)
    with pytest.raises(ValueError):
        mesh_io.write_ply(str(tmp_path / "short.ply"), V, T, normals=N[:-1])
    with pytest.raises(ValueError):
        mesh_io.write_ply(str(tmp_path / "short.ply"), V, T, colors=Cc[:-1])
    path = mesh_io.write_ply(str(tmp_path / "cut.ply"), V, T, normals=N, colors=Cc)
    data = open(path, "rb").read()
    open(path, "wb").write(data[:-1])
    with pytest.raises(ValueError):
        mesh_io.read_ply_attributes(path)
    import torch
    path = mesh_io.write_ply(str(tmp_path / "t.ply"), torch.from_numpy(V), torch.from_numpy(T), normals=torch.from_numpy(N),
                             colors=torch.from_numpy(Cc))
    assert open(path, "rb").read() == data


# ---- options ------------------------------------------------------------------------------------------------------------------
def test_surface_option_parsing():
    from joint_tensorf_amd import export
    base = ["--yaml=bat_blender_VM", "--load=a.ckpt", "--output_path=out"]
    opt = export.build_options(base)
    assert dict(opt.mesh) == dict(res=None, level=0.005, cap=True)
    assert dict(opt.surface) == dict(keep_largest=None, min_points=None, normals=False, colors=False)
    opt = export.build_options(base + ["--surface.keep_largest=2", "--surface.min_points=50", "--surface.normals=true",
                                       "--surface.colors=true", "--mesh.res=32"])
    assert dict(opt.surface) == dict(keep_largest=2, min_points=50, normals=True, colors=True)
    assert dict(opt.mesh) == dict(res=[32, 32, 32], level=0.005, cap=True) and "surface" not in opt.mesh
    assert export.build_options(base + ["--surface.colors=true"]).surface.normals is False
    with pytest.raises(KeyError):
        export.build_options(base + ["--surface.colour=true"])
    for bad in (["--surface.keep_largest=0"], ["--surface.keep_largest=1.5"], ["--surface.min_points=-3"],
                ["--surface.normals=maybe"], ["--surface.colors=1"], ["--surface=3"]):
        with pytest.raises(SystemExit):
            export.build_options(base + bad)


# ---- entry points -------------------------------------------------------------------------------------------------------------
def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    """JT_ERR_ARG (1) for a NULL pointer, a size below 2 and a non-finite level, JT_ERR_UNSUPPORTED (2) above 2^27 points.  Nothing
    here reaches a kernel."""
    from joint_tensorf_amd import _lib, ops
    L, p = _lib.lib, 64                     # p: a non-NULL pointer that is never dereferenced on these paths
    assert ops.COMPONENTS_TILE == 8
    assert L.jt_components_init(None, 4, 4, 4, 0.0, p, None) == 1
    assert L.jt_components_init(p, 4, 4, 4, 0.0, None, None) == 1
    assert L.jt_components_init(p, 4, 1, 4, 0.0, p, None) == 1
    assert L.jt_components_init(p, 4, 4, 4, float("nan"), p, None) == 1
    assert L.jt_components_init(p, 4, 4, 4, float("-inf"), p, None) == 1
    assert L.jt_components_init(p, 512, 512, 513, 0.0, p, None) == 2
    assert L.jt_components_sweep(None, 4, 4, 4, p, 1, None) == 1
    assert L.jt_components_sweep(p, 4, 4, 4, None, 1, None) == 1
    assert L.jt_components_sweep(p, 4, 4, 1, p, 0, None) == 1
    assert L.jt_components_sweep(p, 513, 512, 512, p, 0, None) == 2
    assert L.jt_component_sizes(None, 4, 4, 4, p, None) == 1
    assert L.jt_component_sizes(p, 4, 4, 4, None, None) == 1
    assert L.jt_component_sizes(p, 1, 4, 4, p, None) == 1
    assert L.jt_component_sizes(p, 512, 513, 512, p, None) == 2
    # jt_density_gradient: a scene, factors with every density pointer, points and the gradient; feat may be NULL
    cfg = ops.RenderCfg(aabb=[-1, -1, -1, 1, 1, 1], plane_hw=[(8, 8)] * 3, line_len=[8] * 3, n_comp_density=16, n_comp_app=48,
                        step_size=0.01, near_far=(2.0, 6.0), distance_scale=25.0, density_shift=-10.0,
                        density_act=_lib.JT_ACT_SOFTPLUS, weight_thres=1e-4, n_samples=1, ndc=False, white_bg=False, app_dim=27,
                        mlp_kind=0, mlp_hidden=64, view_pe=2, fea_pe=2)
    fac = _lib.JtFactors()
    for i in range(3):
        fac.density_plane[i] = p
        fac.density_line[i] = p
    assert L.jt_density_gradient(None, fac, p, 5, p, p, None) == 1
    assert L.jt_density_gradient(cfg.scene(), None, p, 5, p, p, None) == 1
    assert L.jt_density_gradient(cfg.scene(), fac, None, 5, p, p, None) == 1
    assert L.jt_density_gradient(cfg.scene(), fac, p, 5, p, None, None) == 1
    assert L.jt_density_gradient(cfg.scene(), fac, p, -1, p, p, None) == 1
    assert L.jt_density_gradient(cfg.scene(), fac, p, 0, None, p, None) == 0            # no points: nothing launched
    fac.density_line[1] = None
    assert L.jt_density_gradient(cfg.scene(), fac, p, 5, p, p, None) == 1
    fac.density_line[1] = p
    cfg.n_comp_density = 6
    assert L.jt_density_gradient(cfg.scene(), fac, p, 5, p, p, None) == 2               # channels not a multiple of four
