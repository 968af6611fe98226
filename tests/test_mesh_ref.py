"""The mesh export without a GPU: the NumPy statement of the extraction contract (tests/mesh_ref.py) against analytic fields --
what the GPU tests then hold the kernels to --, the PLY and cameras.json writers, and the option parsing of
`python -m joint_tensorf_amd.export`."""
import json
import os
import re

import numpy as np
import pytest

from tests import mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _topo(vol, level, lo, hi):
    V, T = R.reference_mesh(vol, level, lo, hi)
    return V, T, R.topology(V, T)


def test_kernel_case_table_equals_the_derived_one():
    """csrc/jt_mesh.hip writes its 16 cases by hand for a positively oriented tetrahedron and swaps the last two corners of every
    triangle for an odd permutation; tests/mesh_ref.py derives every (permutation, case) from the ideal geometry.  The same
    triangles, up to rotation, in all 96 pairs."""
    src = open(os.path.join(ROOT, "joint_tensorf_amd", "csrc", "jt_mesh.hip")).read()
    body = src[src.index("kMeshCase[16] = {"):]
    body = body[:body.index("};")]
    entries = []
    for ln in body.splitlines()[1:]:
        ln = ln.split("//")[0].strip().rstrip(",")
        if not ln:
            continue
        if ln.startswith("0"):
            entries.append([])
            continue
        a = [int(v) for v in re.findall(r"\d+", ln[ln.index("("):])]
        entries.append([tuple(a[1 + 3 * t:4 + 3 * t]) for t in range(a[0])])
    assert len(entries) == 16
    edges = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for perm in R.PERMS:
        odd = sum(1 for i in range(3) for j in range(i + 1, 3) if perm[i] > perm[j]) & 1
        for case in range(16):
            mine = [tuple(edges[q] for q in t) for t in entries[case]]
            if odd:
                mine = [(t[0], t[2], t[1]) for t in mine]
            mine = sorted(tuple(t[t.index(min(t)):] + t[:t.index(min(t))]) for t in mine)
            ref = sorted(tuple(t[t.index(min(t)):] + t[:t.index(min(t))]) for t in R.CASES[(perm, case)])
            assert mine == ref, (perm, case, mine, ref)


def test_all_255_cell_configurations_are_closed_oriented_and_positive():
    for config in range(1, 256):
        V, T, t = _topo(R.cell_configuration(config), 0.0, (0, 0, 0), (3, 3, 3))
        assert t["closed"] and t["oriented"] and t["volume"] > 0, (config, t)
        assert len(V) and (V >= 0.5).all() and (V <= 2.5).all()          # midpoints of edges that touch the middle cell


@pytest.mark.parametrize("shape", [(9, 11, 13), (12, 12, 12)])
def test_sphere(shape):
    c, radius = np.array((0.05, -0.03, 0.1)), 0.6
    V, T, t = _topo(R.sphere_field(shape, c, radius), 0.0, R.BOX_LO, R.BOX_HI)
    assert t["closed"] and t["oriented"] and t["euler"] == 2 and t["volume"] > 0
    # linear interpolation of a field with |f''| <= 1 / (R - L) along an edge no longer than the cell's body diagonal L
    L = float(np.linalg.norm((np.array(R.BOX_HI) - np.array(R.BOX_LO)) / (np.array(shape) - 1)))
    err = float(np.abs(np.linalg.norm(V - c, axis=1) - radius).max())
    bound = L * L / (8 * (radius - L)) + 1e-5
    print("sphere %s: %d vertices, %d triangles, radial error %.4f (bound %.4f), volume %.4f" % (shape, len(V), len(T), err, bound, t["volume"]))
    assert err <= bound
    assert abs(t["volume"] - 4 / 3 * np.pi * radius ** 3) < 0.1 * 4 / 3 * np.pi * radius ** 3


def test_torus_and_two_spheres():
    _, _, t = _topo(R.torus_field((14, 15, 9)), 0.0, R.BOX_LO, R.BOX_HI)
    assert t["closed"] and t["oriented"] and t["euler"] == 0 and t["volume"] > 0
    _, _, t = _topo(R.two_spheres_field((13, 8, 8)), 0.0, R.BOX_LO, R.BOX_HI)
    assert t["closed"] and t["oriented"] and t["euler"] == 4 and t["volume"] > 0


def test_values_exactly_at_the_level():
    """six lattice points carry the level itself: vertices of several edges fall on one lattice point there and triangles
    degenerate -- a winding read off the positions would flip some of them"""
    vol, lo, hi = R.integer_sphere_field()
    assert int((vol == 0).sum()) == 6
    V, T, t = _topo(vol, 0.0, lo, hi)
    assert t["closed"] and t["oriented"] and t["euler"] == 2 and t["volume"] > 0
    areas = np.linalg.norm(np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]]), axis=1)
    assert (areas == 0).any()                             # the degenerate triangles are there


def test_surface_cut_by_the_box_and_capped():
    f = R.sphere_field((8, 9, 7), (0, 0, 0.2), 1.3)
    V, T, t = _topo(f, 0.0, R.BOX_LO, R.BOX_HI)
    assert not t["closed"] and len(t["boundary"]) > 0
    lo, hi = np.float32(R.BOX_LO).astype(np.float64), np.float32(R.BOX_HI).astype(np.float64)

    def on_face(v):
        return bool(((v == lo) | (v == hi)).any())
    assert all(on_face(V[a]) and on_face(V[b]) for a, b in t["boundary"])
    # 0.5 is the issue's level (the surface |x - c| = 0.8 stays inside the box); at 0.05 the box really cuts it
    for level in (0.5, 0.05):
        cv, clo, chi = R.cap(np.clip(f, 0, 1), R.BOX_LO, R.BOX_HI)
        assert cv.shape == (10, 11, 9) and (clo < lo).all() and (chi > hi).all()
        V, T, t = _topo(cv, level, clo, chi)
        assert t["closed"] and t["oriented"] and t["euler"] == 2 and t["volume"] > 0, (level, t)
        assert (V >= clo).all() and (V <= chi).all()


def test_reference_order_and_strictness():
    """vertices by owner point and kind, triangles by cell and permutation; inside is strictly above the level; NaN is outside"""
    vol = np.full((2, 2, 2), -1.0, dtype=np.float32)
    vol[0, 0, 0] = 1.0
    V, T, cells = R.reference_mesh(vol, 0.0, (0, 0, 0), (1, 1, 1), return_cells=True)
    assert len(V) == 7 and len(T) == 6 and (cells == 0).all()           # the seven edges of corner 0, one triangle per tetrahedron
    want = 0.5 * np.array(R.KIND_OFFSETS, dtype=np.float64)
    np.testing.assert_array_equal(V, want)
    assert [sorted(t) for t in T.tolist()] == [[0, 3, 6], [0, 4, 6], [1, 3, 6], [1, 5, 6], [2, 4, 6], [2, 5, 6]]
    vol[0, 0, 0] = 0.0                                                   # equal to the level: outside
    assert len(R.reference_mesh(vol, 0.0, (0, 0, 0), (1, 1, 1))[0]) == 0
    vol[0, 0, 0] = np.nan
    assert len(R.reference_mesh(vol, 0.0, (0, 0, 0), (1, 1, 1))[0]) == 0


# ---- files ---------------------------------------------------------------------------------------------------------------
def _roundtrip(tmp_path, V, T, comments=()):
    from joint_tensorf_amd import mesh_io
    path = mesh_io.write_ply(str(tmp_path / "m.ply"), V, T, comments)
    V2, T2, c2 = mesh_io.read_ply(path)
    assert V2.dtype == np.float32 and T2.dtype == np.int32 and V2.shape == (len(V), 3) and T2.shape == (len(T), 3)
    assert V2.tobytes() == np.asarray(V, dtype=np.float32).tobytes() and T2.tobytes() == np.asarray(T, dtype=np.int32).tobytes()
    assert c2 == [str(c) for c in comments]
    return path


def test_ply_round_trip(tmp_path):
    from joint_tensorf_amd import mesh_io
    _roundtrip(tmp_path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    path = _roundtrip(tmp_path, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32),
                      mesh_io.mesh_comments(0.005, (17, 19, 23), (-1, -1.5, -2), (1, 1.5, 2), "world"))
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    assert [ln for ln in lines if not ln.startswith("comment")][2:] == [
        "element vertex 3", "property float x", "property float y", "property float z", "element face 1",
        "property list uchar int vertex_indices"]
    assert "comment level 0.005" in lines and "comment lattice 17 19 23" in lines and "comment space world" in lines
    assert "comment box_lo -1.0 -1.5 -2.0" in lines and "comment box_hi 1.0 1.5 2.0" in lines
    assert len(body) == 3 * 12 + 13 and body[36] == 3
    rng = np.random.default_rng(3)
    nv, nt = 60000, 100000
    V = rng.standard_normal((nv, 3)).astype(np.float32)
    V[0, 0], V[1, 1] = np.float32(np.inf), np.float32(-0.0)
    _roundtrip(tmp_path, V, rng.integers(0, nv, size=(nt, 3)).astype(np.int32), ["space ndc"])
    with pytest.raises(ValueError):
        mesh_io.write_ply(str(tmp_path / "bad.ply"), V[:3], np.array([[0, 1, 3]]))
    with pytest.raises(ValueError):
        mesh_io.write_ply(str(tmp_path / "bad.ply"), V[:3], np.array([[0, 1, 2]]), ["two\nlines"])
    with pytest.raises(ValueError):
        mesh_io.mesh_comments(0.005, (2, 2, 2), (0, 0, 0), (1, 1, 1), "camera")


def test_ply_takes_tensors(tmp_path):
    import torch
    from joint_tensorf_amd import mesh_io
    V = torch.tensor([[0.1, 0.2, 0.3], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    T = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    V2, T2, _ = mesh_io.read_ply(mesh_io.write_ply(str(tmp_path / "t.ply"), V, T))
    assert np.array_equal(V2, V.numpy()) and np.array_equal(T2, T.numpy())


def test_cameras_json_round_trip(tmp_path):
    from joint_tensorf_amd import mesh_io
    rng = np.random.default_rng(5)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)        # noqa: E731
    cams = {"space": "world", "n_views": 2, "image_size": [30, 40],
            "sim3": {"t0": f32(3).tolist(), "t1": f32(3).tolist(), "s0": float(f32()), "s1": float(f32()), "R": f32(3, 3).tolist()},
            "views": [{"idx": i, "pose": f32(3, 4).tolist(), "intr": f32(3, 3).tolist(), "pose_aligned": f32(3, 4).tolist()}
                      for i in range(2)]}
    path = mesh_io.write_cameras(str(tmp_path / "cameras.json"), cams)
    assert mesh_io.read_cameras(path) == cams == json.load(open(path))
    back = np.array(mesh_io.read_cameras(path)["views"][1]["pose"], dtype=np.float32)
    assert back.tobytes() == np.array(cams["views"][1]["pose"], dtype=np.float32).tobytes()   # fp32 values survive the text


def test_export_option_parsing():
    from joint_tensorf_amd import export
    opt = export.build_options(["--yaml=bat_blender_VM", "--load=a.ckpt", "--output_path=out"])
    assert dict(opt.mesh) == dict(res=None, level=0.005, cap=True) and opt.load == "a.ckpt" and opt.output_path == "out"
    assert not export.has_dataset(opt) and (opt.H, opt.W) == tuple(opt.data.image_size)
    opt = export.build_options(["--yaml=bat_llff_VM_MLP", "--load=a.ckpt", "--output_path=out", "--mesh.res=[17,19,23]",
                                "--mesh.level=1.e-2", "--mesh.cap=false", "--data.root=/somewhere", "--data.scene=fern"])
    assert opt.mesh.res == [17, 19, 23] and opt.mesh.level == 0.01 and opt.mesh.cap is False
    assert export.has_dataset(opt) and opt.data.scene == "fern" and opt.camera.ndc
    assert export.build_options(["--yaml=bat_blender_VM", "--mesh.res=64"]).mesh.res == [64, 64, 64]
    assert export.has_dataset(export.build_options(["--yaml=bat_blender_VM", "--data.synthetic=true"]))
    for bad in (["--mesh.res=1"], ["--mesh.res=[4,4]"], ["--mesh.res=2.5"], ["--mesh.cap=maybe"], ["--mesh=3"]):
        with pytest.raises(SystemExit):
            export.build_options(["--yaml=bat_blender_VM"] + bad)
    with pytest.raises(KeyError):
        export.build_options(["--yaml=bat_blender_VM", "--mesh.resolution=64"])
    with pytest.raises(KeyError):
        export.build_options(["--yaml=bat_blender_VM", "--mehs.res=64"])
    with pytest.raises(SystemExit):
        export.build_options(["--mesh.res=64"])
    with pytest.raises(SystemExit):
        export.main(["--yaml=bat_blender_VM", "--output_path=out"])        # no checkpoint named: refused before any GPU work


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """JT_ERR_ARG (1) for a NULL pointer, a size below 2 and a non-finite level, JT_ERR_UNSUPPORTED (2) above 2^27 points or at 2^31
    vertices / triangle corners; an empty mesh is JT_OK without a launch.  Nothing here reaches a kernel."""
    import ctypes
    from joint_tensorf_amd import _lib
    L, p = _lib.lib, 64                     # p: a non-NULL pointer that is never dereferenced on these paths
    box = (ctypes.c_float * 3)(0, 0, 0)
    assert L.jt_mesh_count(None, 4, 4, 4, 0.0, p, p, None) == 1
    assert L.jt_mesh_count(p, 4, 4, 4, 0.0, None, p, None) == 1
    assert L.jt_mesh_count(p, 1, 4, 4, 0.0, p, p, None) == 1
    assert L.jt_mesh_count(p, 4, 4, 4, float("nan"), p, p, None) == 1
    assert L.jt_mesh_count(p, 4, 4, 4, float("inf"), p, p, None) == 1
    assert L.jt_mesh_count(p, 512, 512, 513, 0.0, p, p, None) == 2
    assert L.jt_mesh_emit(p, 4, 4, 1, 0.0, box, box, p, p, p, 1, 1, p, p, None) == 1
    assert L.jt_mesh_emit(p, 4, 4, 4, 0.0, None, box, p, p, p, 1, 1, p, p, None) == 1
    assert L.jt_mesh_emit(p, 4, 4, 4, 0.0, box, box, p, p, p, 1, 1, None, p, None) == 1
    assert L.jt_mesh_emit(p, 4, 4, 4, float("nan"), box, box, p, p, p, 1, 1, p, p, None) == 1
    assert L.jt_mesh_emit(p, 512, 512, 513, 0.0, box, box, p, p, p, 1, 1, p, p, None) == 2
    assert L.jt_mesh_emit(p, 4, 4, 4, 0.0, box, box, p, p, p, 1 << 31, 1, p, p, None) == 2
    assert L.jt_mesh_emit(p, 4, 4, 4, 0.0, box, box, p, p, p, 1, 715827883, p, p, None) == 2
    assert L.jt_mesh_emit(p, 4, 4, 4, 0.0, box, box, p, p, p, 0, 0, None, None, None) == 0
