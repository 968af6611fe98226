"""The texture atlas without a GPU: the layout (mesh_io.texture_layout / ops.texture_layout) against its definition and against the
property that makes it usable -- a viewer's bilinear filter never mixes the two triangles of a block and never leaves the block --
in exact rational arithmetic; the PLY / OBJ / MTL writers and their readers; and the exporter's options."""
from fractions import Fraction

import numpy as np
import pytest

from tests import texture_ref as X

BLOCKS = list(range(4, 14))
COUNTS = [1, 2, 3, 131]


@pytest.mark.parametrize("S", BLOCKS)
def test_layout_is_the_definition(S):
    from joint_tensorf_amd import mesh_io, ops
    for nt in COUNTS:
        lay, ref = mesh_io.texture_layout(nt, S), X.layout(nt, S)
        assert lay == ops.texture_layout(nt, S)
        assert (lay.block, lay.leg, lay.n_triangles, lay.n_blocks, lay.cols, lay.rows, lay.width, lay.height, lay.n_entries) == \
            (S, S - 3, nt, (nt + 1) // 2, ref["cols"], ref["rows"], ref["W"], ref["H"], ref["n_entries"])
        assert lay.cols * lay.cols >= lay.n_blocks > (lay.cols - 1) * (lay.cols - 1)          # the smallest such cols
        assert lay.rows * lay.cols >= lay.n_blocks > (lay.rows - 1) * lay.cols
        # every texel of a block has exactly one owner, and the two charts are each other's mirror image
        b, i, j, tri, ci, cj = X.entries(ref)
        assert len(b) == lay.n_entries and set(np.unique(tri - 2 * b)) <= {0, 1}
        lower = tri == 2 * b
        assert np.array_equal(lower, i + j <= S - 1)
        assert np.array_equal(ci, np.where(lower, i, S - 1 - i)) and np.array_equal(cj, np.where(lower, j, S - 1 - j))
        first = b == 0
        assert lower[first].sum() == S * (S + 1) // 2 and (~lower[first]).sum() == S * (S - 1) // 2
        assert ci.min() >= 0 and cj.min() >= 0 and (ci + cj)[lower].max() == S - 1 and (ci + cj)[~lower].max() == S - 2
        # entries and atlas pixels are in bijection (onto the pixels of the blocks in use)
        px, py = X.pixels(ref)
        assert px.min() == 0 and py.min() == 0 and px.max() < lay.width and py.max() == lay.height - 1
        flat = py * lay.width + px
        assert len(np.unique(flat)) == lay.n_entries
        e = b * S * S + j * S + i
        assert np.array_equal(e, np.arange(lay.n_entries))
        assert np.array_equal(px, (b % lay.cols) * S + i) and np.array_equal(py, (b // lay.cols) * S + j)
        # the corners: on texel centres, on the texels of barycentrics (0, 0), (1, 0), (0, 1) of the right chart
        uv = mesh_io.texture_uv(lay)
        assert uv.dtype == np.float32 and uv.shape == (nt, 3, 2) and np.array_equal(uv.astype(np.float64), X.uv(ref))
        assert np.array_equal(uv - np.floor(uv), np.full_like(uv, 0.5))
        owner = np.full((lay.height, lay.width), -1)
        owner[py, px] = tri
        chart = np.zeros((lay.height, lay.width, 2), dtype=np.int64)
        chart[py, px] = np.stack([ci, cj], -1)
        for t in range(nt):
            for k, want in enumerate(((0, 0), (S - 3, 0), (0, S - 3))):
                x, y = (int(v) for v in np.floor(uv[t, k]))
                assert owner[y, x] == t and tuple(chart[y, x]) == want, (t, k)


@pytest.mark.parametrize("S", BLOCKS)
def test_a_bilinear_filter_stays_inside_its_chart(S):
    """over a dense rational grid of barycentrics (corners and edges included): every texel that carries weight has chart
    coordinates i, j >= 0 and i + j <= S - 2 -- inside the block, and, mirrored, i + j >= S for the other chart: never shared"""
    n = 4 * (S - 3) + 3                                        # finer than the texels and not aligned with them
    seen = 0
    for grid in (n, S - 3):                                    # and the texel centres themselves
        for p in range(grid + 1):
            for q in range(grid + 1 - p):
                for (i, j) in X.footprint(S, Fraction(p, grid), Fraction(q, grid)):
                    assert i >= 0 and j >= 0 and i + j <= S - 2, (S, p, q, i, j)
                    assert (S - 1 - i) + (S - 1 - j) >= S
                    seen = max(seen, i + j)
    assert seen == S - 2                                       # the bound is met: S = L + 3 is the smallest block that works


def test_layout_refusals():
    from joint_tensorf_amd import mesh_io
    for bad in (3, 65, 2.5, True, "8", None):
        with pytest.raises(ValueError):
            mesh_io.texture_layout(10, bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            mesh_io.texture_layout(bad, 8)
    side = mesh_io.TEXTURE_MAX_SIDE // 8                       # 2048 blocks of 8 texels a side
    assert mesh_io.texture_layout(2 * side * side, 8).width == mesh_io.TEXTURE_MAX_SIDE
    with pytest.raises(ValueError) as e:
        mesh_io.texture_layout(2 * side * side + 1, 8)
    assert "smaller block" in str(e.value) and "--simplify.cell" in str(e.value)
    with pytest.raises(ValueError):
        mesh_io.texture_layout(2 * 256 * 256 + 1, 64)


def _mesh(seed=3, nt=7):
    V, N, T = X.soup(nt, seed)
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    return V, N.astype(np.float32), T


@pytest.mark.parametrize("with_normals,with_colors", [(False, False), (True, False), (True, True)])
def test_ply_round_trip_with_texcoords(tmp_path, with_normals, with_colors):
    from joint_tensorf_amd import mesh_io
    V, N, T = _mesh()
    lay = mesh_io.texture_layout(len(T), 6)
    uv = mesh_io.texture_uv(lay)
    C = np.random.default_rng(1).uniform(0, 1, size=V.shape)
    path = str(tmp_path / "mesh.ply")
    kw = dict(normals=N if with_normals else None, colors=C if with_colors else None)
    mesh_io.write_ply(path, V, T, ["one", "two"], texcoords=uv, texture_size=(lay.width, lay.height), **kw)
    got = mesh_io.read_ply_textured(path)
    assert np.array_equal(got["vertices"], V) and np.array_equal(got["triangles"], T)
    assert got["comments"] == ["one", "two", "TextureFile atlas.png"] and got["texture_file"] == "atlas.png"
    assert (got["normals"] is None) == (not with_normals) and (got["colors"] is None) == (not with_colors)
    if with_normals:
        assert np.array_equal(got["normals"], N)
    if with_colors:
        assert np.array_equal(got["colors"], mesh_io.quantise_colors(C))
    want = np.stack([uv[..., 0].astype(np.float64) / lay.width, 1.0 - uv[..., 1].astype(np.float64) / lay.height], -1).astype(np.float32)
    assert got["texcoords"].dtype == np.float32 and np.array_equal(got["texcoords"], want)
    assert got["texcoords"].min() > 0 and got["texcoords"].max() < 1
    head = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[-3:-1] == ["property list uchar int vertex_indices", "property list uchar float texcoord"]
    assert "comment TextureFile atlas.png" in head
    for old in (mesh_io.read_ply, mesh_io.read_ply_attributes):
        with pytest.raises(ValueError):
            old(path)                                          # the old readers read the old layouts, and say so
    with pytest.raises(ValueError):
        mesh_io.write_ply(path, V, T, texcoords=uv)                                   # pixel units need the atlas size
    with pytest.raises(ValueError):
        mesh_io.write_ply(path, V, T, texcoords=uv[:-1], texture_size=(lay.width, lay.height))
    with pytest.raises(ValueError):
        mesh_io.write_ply(path, V, T, texture_file="atlas.png")


def test_ply_without_texcoords_is_byte_for_byte_what_it_was(tmp_path):
    """the file of the same call, and the layout spelt out here: header lines, 12 / 24 / 27 bytes per vertex, 13 per face"""
    from joint_tensorf_amd import mesh_io
    V, N, T = _mesh()
    C = np.random.default_rng(1).uniform(0, 1, size=V.shape)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    for kw in (dict(), dict(normals=N), dict(normals=N, colors=C)):
        mesh_io.write_ply(a, V, T, ["c"], **kw)
        mesh_io.write_ply(b, V, T, ["c"], texcoords=None, texture_file=None, texture_size=None, **kw)
        data = open(a, "rb").read()
        assert data == open(b, "rb").read()
        props = ["property float x", "property float y", "property float z"]
        props += ["property float nx", "property float ny", "property float nz"] if "normals" in kw else []
        props += ["property uchar red", "property uchar green", "property uchar blue"] if "colors" in kw else []
        head = "\n".join(["ply", "format binary_little_endian 1.0", "comment c", "element vertex %d" % len(V)] + props
                         + ["element face %d" % len(T), "property list uchar int vertex_indices", "end_header"]) + "\n"
        rows = [V.astype("<f4")] + ([N.astype("<f4")] if "normals" in kw else [])
        body = b"".join(b"".join(r[i].tobytes() for r in rows) + (mesh_io.quantise_colors(C)[i].tobytes() if "colors" in kw else b"")
                        for i in range(len(V)))
        faces = b"".join(b"\x03" + T[t].astype("<i4").tobytes() for t in range(len(T)))
        assert data == head.encode("ascii") + body + faces
        assert np.array_equal(mesh_io.read_ply_attributes(a)["triangles"], T)


@pytest.mark.parametrize("with_normals", [False, True])
def test_obj_and_mtl_parse_back_to_the_same_floats(tmp_path, with_normals):
    from joint_tensorf_amd import mesh_io
    V, N, T = _mesh(seed=5, nt=9)
    V[0] = [1e-7, -3.4e38, 0.1]                                # values a short decimal does not hold
    lay = mesh_io.texture_layout(len(T), 5)
    uv = mesh_io.texture_uv(lay)
    path = str(tmp_path / "mesh.obj")
    obj, mtl = mesh_io.write_obj(path, V, T, uv, (lay.width, lay.height), normals=N if with_normals else None)
    assert obj == path and mtl == str(tmp_path / "mesh.mtl")
    got = mesh_io.read_obj(obj)
    assert got["mtllib"] == "mesh.mtl" and got["usemtl"] == "atlas" and mesh_io.read_mtl(mtl) == "atlas.png"
    assert "newmtl atlas" in open(mtl).read()
    assert np.array_equal(got["vertices"], V)
    assert (got["normals"] is None) if not with_normals else np.array_equal(got["normals"], N)
    want = np.stack([uv[..., 0].astype(np.float64) / lay.width, 1.0 - uv[..., 1].astype(np.float64) / lay.height], -1).astype(np.float32)
    assert np.array_equal(got["texcoords"], want.reshape(-1, 2))                    # one vt per corner
    assert np.array_equal(got["faces"][..., 0], T)
    assert np.array_equal(got["faces"][..., 1], np.arange(3 * len(T)).reshape(-1, 3))
    assert np.array_equal(got["faces"][..., 2], T if with_normals else np.full_like(T, -1))
    with pytest.raises(ValueError):
        mesh_io.write_obj(path, V, T, uv[:-1], (lay.width, lay.height))


@pytest.mark.parametrize("name", ["fan", "mixed"])
def test_the_sampling_scenes_have_few_near_ties(name):
    """tests/test_gpu_texture.py compares the sampled colour where the device's winner is the reference's, and asks for 99 % of
    the covered pixels: the reference alone must leave that many undisputed (no runner-up within 1e-5 of the winner), and its
    sample of a constant atlas is that constant"""
    from tests import raster_ref as R
    scene = dict(fan=R.fan_scene, mixed=R.mixed_scene)[name]()
    screen = R.project(scene["vertices"], scene["proj"][None])[0]
    lay = X.layout(len(scene["triangles"]), 4)
    atlas = np.full((lay["H"], lay["W"], 3), 51, dtype=np.uint8)
    ref = X.sample(screen, scene["triangles"], scene["H"], scene["W"], atlas, lay, background=0.0)
    covered = ref["tri"] >= 0
    ties = R.near_ties(ref) & covered
    assert covered.sum() > 400 and ties.sum() <= 0.01 * covered.sum(), (covered.sum(), ties.sum())
    assert np.abs(ref["out"][covered] - 0.2).max() < 1e-15 and (ref["out"][~covered] == 0).all()


BASE = ["--yaml=bat_blender_VM"]


def test_export_options():
    from joint_tensorf_amd import export
    assert export.TEXTURE_DEFAULTS == dict(block=None) and "texture" in export.PREVIEW_SHADES
    opt = export.build_options(BASE)
    assert opt.texture.block is None
    opt = export.build_options(BASE + ["--texture.block=8"])
    assert opt.texture.block == 8 and isinstance(opt.texture.block, int)
    opt = export.build_options(BASE + ["--texture.block=6", "--preview.views=2", "--preview.shade=texture", "--preview.check=true",
                                       "--simplify.cell=3"])
    assert opt.texture.block == 6 and opt.preview.shade == "texture" and opt.simplify.cell == 3.0
    for bad in ("3", "65", "2.5", "true", "abc"):
        with pytest.raises(SystemExit) as e:
            export.build_options(BASE + ["--texture.block=%s" % bad])
        assert "--texture.block" in str(e.value)
    with pytest.raises(KeyError):
        export.build_options(BASE + ["--texture.size=8"])
    with pytest.raises(SystemExit) as e:
        export.build_options(BASE + ["--preview.views=2", "--preview.shade=texture"])
    assert "--texture.block" in str(e.value)
    # a chart that is linear in NDC is not linear in world space: not together with the unwarp of a camera.ndc scene
    llff = ["--yaml=bat_llff_VM_MLP"]
    assert export.build_options(llff + ["--texture.block=8"]).texture.block == 8
    with pytest.raises(SystemExit) as e:
        export.build_options(llff + ["--texture.block=8", "--frame.space=world"])
    assert "--frame.space=world" in str(e.value) and "NDC" in str(e.value)
    assert export.build_options(BASE + ["--texture.block=8", "--frame.space=world"]).texture.block == 8     # already a world scene
