"""The texture atlas on the GPU (csrc/jt_texture.hip through ops.texture_texels / texture_pack, jt_raster_resolve_texture through
ops.rasterize(texture=), TensorVMSplit.bake_texture / extract_mesh(texture=), and `python -m joint_tensorf_amd.export
--texture.block=S`) against the NumPy statement of its contract, tests/texture_ref.py.

Texel positions, directions, validity and the packed bytes are compared BIT FOR BIT: they are fixed sequences of correctly rounded
fp32 / fp64 operations (contraction off), which IEEE 754 defines to the bit.  The one thing it leaves open is the sign and payload of
a NaN RESULT: the texels of the triangle with a NaN vertex must be NaN where the reference's are, and are not compared further.

The sampled colour is held to 1e-4 against the fp64 reference at pixels whose winner agrees.  That bound is derived, not measured:
the weights l are good to a few fp32 ulp, so s = l L with L <= 61 is off by at most about 1.5e-5 texels; texel values in [0, 1]
change by at most 1 per texel and axis, so the sample moves by at most 3e-5; the five fused operations add less than 1e-6; 1e-4 is
about three times the sum.  A constant atlas has q - p = 0 in every lerp and comes back exactly."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import raster_ref as R
from tests import texture_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
SAMPLE_TOL = 1e-4
_CACHE = {}


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gpu_texels(V, N, T, S, start=0, count=None):
    from joint_tensorf_amd import ops
    lay = ops.texture_layout(len(T), S)
    xyz, dirs, valid = ops.texture_texels(_dev(V, np.float32), _dev(T, np.int32), _dev(N, np.float32), lay, start, count)
    n = lay.n_entries - start if count is None else count
    assert xyz.dtype == dirs.dtype == torch.float32 and valid.dtype == torch.uint8
    assert tuple(xyz.shape) == tuple(dirs.shape) == (n, 3) and tuple(valid.shape) == (n,)
    return xyz.cpu().numpy(), dirs.cpu().numpy(), valid.cpu().numpy()


def _same_texels(got, ref, label):
    """bit for bit; a NaN of the reference must be a NaN (of any sign and payload) on the device"""
    assert np.array_equal(got[2], ref[2]), (label, "valid")
    nan = np.isnan(ref[0])
    assert np.array_equal(np.isnan(got[0]), nan), (label, "NaN positions")
    bad = (_bits(got[0]) != _bits(ref[0])) & ~nan
    assert not bad.any(), (label, "xyz", int(bad.sum()), got[0][bad.any(-1)][:4], ref[0][bad.any(-1)][:4])
    bad = _bits(got[1]) != _bits(ref[1])
    assert not bad.any(), (label, "dirs", int(bad.sum()), got[1][bad.any(-1)][:4], ref[1][bad.any(-1)][:4])


def _soup(nt, seed):
    """the random soup of texture_ref with one vertex id out of range, one zero normal sum and one NaN vertex (131 triangles)"""
    V, N, T = X.soup(nt, seed)
    if nt >= 100:
        T[7, 1] = len(V)                                       # out of range above
        T[9, 0] = -1                                           # and below
        a, b, c = T[20]
        N[a] = N[b] = N[c] = 0                                 # every interpolated normal of triangle 20 is zero
        a, b, c = T[40]
        N[b] = -N[a]                                           # the normal vanishes at one texel of an edge (a = 1/2 at even L)
        N[c] = N[a]
        V[T[60, 2], 1] = np.nan
        N[T[70, 0], 0] = np.inf
    return V, N, T


@pytest.mark.parametrize("S", [4, 5, 8])
@pytest.mark.parametrize("nt", [1, 2, 131])
def test_texels_equal_the_reference_bit_for_bit(nt, S):
    V, N, T = _soup(nt, seed=10 + nt)
    lay = X.layout(nt, S)
    ref = X.texels(V, N, T, lay)
    got = _gpu_texels(V, N, T, S)
    _same_texels(got, ref, "nt %d S %d" % (nt, S))
    n_invalid = int((ref[2] == 0).sum())
    print("nt %d S %d: atlas %d x %d, %d entries, %d invalid, %d NaN positions, %d fallback directions"
          % (nt, S, lay["W"], lay["H"], lay["n_entries"], n_invalid, int(np.isnan(ref[0]).any(-1).sum()),
             int((ref[1] == np.float32([0, 0, -1])).all(-1).sum())))
    if nt == 1:
        assert n_invalid == S * (S - 1) // 2                   # the empty upper half of the only block
    if nt == 131:
        assert lay["cols"] == 9 and lay["rows"] == 8 and lay["n_blocks"] == 66          # a non-square grid, a partial last row
        assert n_invalid > 2 * S * (S - 1) // 2 and np.isnan(ref[0]).any()
        assert (ref[1][ref[2] == 1] == np.float32([0, 0, -1])).all(-1).sum() >= S * (S - 1) // 2     # the zero normal sum
    # directions are unit vectors, corner texel 0 of every valid triangle is its vertex 0 exactly
    unit = np.linalg.norm(ref[1].astype(np.float64), axis=-1)
    assert np.abs(unit - 1).max() < 1e-6
    uv = X.uv(lay)
    for t in range(nt):
        if ((T[t] >= 0) & (T[t] < len(V))).all() and np.isfinite(V[T[t]]).all():       # (0 times a NaN edge is a NaN)
            x, y = (int(v) for v in np.floor(uv[t, 0]))
            e = ((y // S) * lay["cols"] + x // S) * S * S + (y % S) * S + x % S
            assert got[2][e] == 1 and np.array_equal(_bits(got[0][e]), _bits(V[T[t, 0]])), t


@pytest.mark.parametrize("S", [4, 8])
def test_slabs_compose_to_the_bits_of_one_call(S):
    V, N, T = _soup(131, seed=141)
    whole = _gpu_texels(V, N, T, S)
    n = len(whole[2])
    assert 100 % (S * S) != 0 and n % 100 != 0
    parts = [_gpu_texels(V, N, T, S, start, min(100, n - start)) for start in range(0, n, 100)]
    for k in range(3):
        joined = np.concatenate([p[k] for p in parts])
        assert joined.tobytes() == whole[k].tobytes(), k


def _pack_values(n, seed):
    g = np.random.default_rng(seed)
    rgb = g.uniform(-0.2, 1.2, size=(n, 3)).astype(np.float32)
    k = g.integers(0, 256, size=(n // 2, 3)).astype(np.float64)
    half = (k + g.choice([-0.5, 0.5], size=k.shape)) / 255.0                       # k/255 +- half a step, rounded to fp32
    rgb[: n // 2] = half.astype(np.float32)
    rgb[:3] = [[np.nan, 0.5, 1.0], [np.inf, -np.inf, 0.0], [-0.0, 1.0000001, 254.5 / 255]]
    rgb[3:6] = [np.nextafter(np.float32(0.5 / 255), np.float32(0)), np.float32(0.5 / 255), np.nextafter(np.float32(0.5 / 255), np.float32(1))]
    return rgb


@pytest.mark.parametrize("S,nt", [(4, 131), (8, 3)])
def test_pack_equals_the_reference_bit_for_bit(S, nt):
    from joint_tensorf_amd import ops
    lay, ref_lay = ops.texture_layout(nt, S), X.layout(nt, S)
    n = lay.n_entries
    rgb = _pack_values(n, seed=S)
    valid = (np.random.default_rng(1).random(n) < 0.8).astype(np.uint8)
    valid[:6] = 1
    want = X.pack(rgb, valid, ref_lay)
    assert want[..., 0].max() == 255 and (want == 0).any() and np.isnan(rgb).any()
    runs = []
    for _ in range(2):
        atlas = torch.zeros(lay.height, lay.width, 3, device=DEV, dtype=torch.uint8)
        out = ops.texture_pack(_dev(rgb), _dev(valid), lay, atlas)
        assert out is atlas
        runs.append(atlas.cpu().numpy())
    assert np.array_equal(runs[0], want) and runs[0].tobytes() == runs[1].tobytes()
    # invalid entries leave the (here: not zeroed) atlas alone, and slabs that are no multiple of S S compose
    atlas = torch.full((lay.height, lay.width, 3), 7, device=DEV, dtype=torch.uint8)
    for start in range(0, n, 100):
        ops.texture_pack(_dev(rgb[start:start + 100]), _dev(valid[start:start + 100]), lay, atlas, start)
    want7 = X.pack(rgb, valid, ref_lay, atlas=np.full((lay.height, lay.width, 3), 7, dtype=np.uint8))
    got7 = atlas.cpu().numpy()
    assert np.array_equal(got7, want7)
    px, py = X.pixels(ref_lay)
    assert (got7[py[valid == 0], px[valid == 0]] == 7).all()


def _scene(name):
    """the scene, its device tensors and the GPU's own fp32 screen (the reference is handed it: the projection cannot move a snap)"""
    if name not in _CACHE:
        from joint_tensorf_amd import ops
        scene = dict(fan=R.fan_scene, mixed=R.mixed_scene)[name]()
        V, T, P = _dev(scene["vertices"], np.float32), _dev(scene["triangles"], np.int32), _dev(scene["proj"][None], np.float32)
        screen = ops.raster_project(V, P, 1e-3)
        _CACHE[name] = (scene, V, T, P, screen.cpu().numpy()[0])
    return _CACHE[name]


@pytest.mark.parametrize("name", ["fan", "mixed"])
def test_a_constant_atlas_comes_back_exactly(name):
    from joint_tensorf_amd import ops
    scene, V, T, P, _ = _scene(name)
    H, W = scene["H"], scene["W"]
    lay = ops.texture_layout(T.shape[0], 5)
    byte = np.array([37, 128, 255], dtype=np.uint8)
    atlas = _dev(np.broadcast_to(byte, (lay.height, lay.width, 3)))
    bg = (0.25, 0.5, 0.75)
    got = ops.rasterize(V, T, P, H, W, texture=(atlas, lay), background=bg)
    plain = ops.rasterize(V, T, P, H, W)
    assert torch.equal(got.tri, plain.tri) and torch.equal(got.depth.view(torch.int32), plain.depth.view(torch.int32))
    assert torch.equal(got.status_counts, plain.status_counts) and plain.attrs is None
    covered = (got.tri >= 0).cpu().numpy()[0]
    out = got.attrs.cpu().numpy()[0]
    assert out.shape == (H, W, 3) and out.dtype == np.float32 and 0 < covered.sum() and (name != "fan" or covered.sum() < H * W)
    want = (byte.astype(np.float32) / np.float32(255)).astype(np.float32)
    assert np.array_equal(_bits(out[covered]), np.broadcast_to(_bits(want), out[covered].shape))
    assert np.array_equal(out[~covered], np.broadcast_to(np.float32(bg), out[~covered].shape))


@pytest.mark.parametrize("S", [4, 8])
@pytest.mark.parametrize("name", ["fan", "mixed"])
def test_a_random_atlas_is_sampled_within_the_bound(name, S):
    from joint_tensorf_amd import ops
    scene, V, T, P, screen = _scene(name)
    H, W, nt = scene["H"], scene["W"], len(scene["triangles"])
    lay, ref_lay = ops.texture_layout(nt, S), X.layout(nt, S)
    atlas = np.random.default_rng(S).integers(0, 256, size=(lay.height, lay.width, 3)).astype(np.uint8)
    ref = X.sample(screen, scene["triangles"], H, W, atlas, ref_lay, background=0.5)
    zbuf, _ = ops.raster_draw(_dev(screen[None]), T, H, W)
    tri, depth, out = ops.raster_resolve_texture(zbuf, _dev(screen[None]), T, _dev(atlas), lay, background=0.5)
    tri0, depth0, _ = ops.raster_resolve(zbuf, _dev(screen[None]), T)
    assert torch.equal(tri, tri0) and torch.equal(depth.view(torch.int32), depth0.view(torch.int32))
    tri, out = tri.cpu().numpy()[0], out.cpu().numpy()[0].astype(np.float64)
    covered = ref["tri"] >= 0
    same = covered & (tri == ref["tri"])
    err = np.abs(out - ref["out"])[same]
    print("%s S %d: %d covered pixels, %d compared (%.2f %%), largest error %.3e (bound %.1e)"
          % (name, S, covered.sum(), same.sum(), 100.0 * same.sum() / covered.sum(), err.max(), SAMPLE_TOL))
    assert same.sum() >= 0.99 * covered.sum()
    assert err.max() <= SAMPLE_TOL
    assert np.array_equal(out[~covered & (tri < 0)], np.full_like(out[~covered & (tri < 0)], 0.5))
    assert np.ptp(ref["out"][same]) > 0.2                       # the atlas was really sampled: not a constant


def _blob():
    if "blob" not in _CACHE:
        from tests.test_gpu_simplify import _blob_scene
        tf = _blob_scene(shaded=True)
        _CACHE["blob"] = (tf, tf.extract_mesh(res=(17, 19, 23), normals=True, colors=True))
    return _CACHE["blob"]


@pytest.mark.parametrize("S,slab", [(6, 1 << 20), (5, 4099)])
def test_bake_texture_equals_the_reference_pack_of_point_colors(S, slab):
    from joint_tensorf_amd import mesh_io
    tf, mesh = _blob()
    nt = int(mesh.triangles.shape[0])
    tex = tf.bake_texture(mesh.vertices, mesh.triangles, mesh.normals, block=S, slab_points=slab)
    lay = tex.layout
    assert lay == mesh_io.texture_layout(nt, S) and nt > 200
    assert lay.n_entries > 2 * slab or slab == 1 << 20         # the small slab: several of them, and no multiple of S S
    assert tex.atlas.dtype == torch.uint8 and tuple(tex.atlas.shape) == (lay.height, lay.width, 3) and tex.atlas.is_cuda
    assert tex.uv.dtype == torch.float32 and np.array_equal(tex.uv.cpu().numpy(), mesh_io.texture_uv(lay))
    ref_lay = X.layout(nt, S)
    xyz, dirs, valid = X.texels(mesh.vertices.cpu().numpy(), mesh.normals.cpu().numpy(), mesh.triangles.cpu().numpy(), ref_lay)
    rgb = tf.point_colors(_dev(xyz), _dev(dirs))
    want = X.pack(rgb.cpu().numpy(), valid, ref_lay)
    assert torch.equal(tex.atlas, _dev(want))
    assert len(np.unique(want)) > 4                            # a picture, not a constant
    # corner texels: the field at the vertex seen against its normal, as the vertex colours -- within one level of them
    corners = np.floor(tex.uv.cpu().numpy()).astype(np.int64)                   # [nt, 3, 2] (x, y)
    at_corner = want[corners[..., 1], corners[..., 0]].astype(np.int64)         # [nt, 3, 3]
    vertex = mesh_io.quantise_colors(mesh.colors).astype(np.int64)[mesh.triangles.cpu().numpy().astype(np.int64)]
    print("block %d: atlas %d x %d for %d triangles, corner texels differ from the vertex colours by at most %d levels"
          % (S, lay.width, lay.height, nt, np.abs(at_corner - vertex).max()))
    assert np.abs(at_corner - vertex).max() <= 1


def test_extract_mesh_bakes_last_and_changes_nothing_else():
    tf, mesh = _blob()
    again = tf.extract_mesh(res=(17, 19, 23), normals=True, colors=True, texture=None)
    assert again.texture is None and mesh.texture is None
    for a, b in zip(again, mesh):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    plain = tf.extract_mesh(res=(17, 19, 23), texture=6)
    assert plain.normals is None and plain.colors is None and plain.n_degenerate_normals is None     # computed, not returned
    assert torch.equal(plain.vertices, mesh.vertices) and torch.equal(plain.triangles, mesh.triangles)
    assert torch.equal(plain.texture.atlas, tf.bake_texture(mesh.vertices, mesh.triangles, mesh.normals, block=6).atlas)
    simple = tf.extract_mesh(res=(17, 19, 23), normals=True, texture=6, simplify=2)
    nt = int(simple.triangles.shape[0])
    assert 0 < nt < mesh.triangles.shape[0] and simple.simplified is not None
    assert simple.texture.layout.n_triangles == nt and tuple(simple.texture.uv.shape) == (nt, 3, 2)
    want = tf.bake_texture(simple.vertices, simple.triangles, simple.normals, block=6)
    assert torch.equal(simple.texture.atlas, want.atlas) and simple.texture.atlas.shape[0] < plain.texture.atlas.shape[0]
    for bad in (3, 65, 2.5, True, "8"):
        with pytest.raises(ValueError):
            tf.extract_mesh(res=(17, 19, 23), texture=bad)
        with pytest.raises(ValueError):
            tf.bake_texture(mesh.vertices, mesh.triangles, mesh.normals, block=bad)


def test_export_end_to_end(tmp_path_factory, capsys):
    from PIL import Image
    from joint_tensorf_amd import export, mesh_io
    from tests.test_gpu_preview import _export_args
    root, args, data = _export_args(tmp_path_factory)
    out_dir = os.path.join(root, "textured")
    out = export.main(args + data + ["--output_path=%s" % out_dir, "--texture.block=6", "--simplify.cell=3", "--surface.normals=true",
                                     "--preview.views=2", "--preview.size=[40,40]", "--preview.shade=texture", "--preview.check=true"])
    assert sorted(os.listdir(out_dir)) == ["atlas.png", "cameras.json", "mesh.mtl", "mesh.obj", "mesh.ply", "preview", "report.json"]
    lay = mesh_io.texture_layout(out.n_triangles, 6)
    assert (out.texture.block, out.texture.width, out.texture.height) == (6, lay.width, lay.height)
    img = Image.open(os.path.join(out_dir, "atlas.png"))
    assert img.size == (lay.width, lay.height) and img.mode == "RGB" and len(np.unique(np.asarray(img))) > 10
    ply = mesh_io.read_ply_textured(out.mesh)
    assert ply["texcoords"].shape == (out.n_triangles, 3, 2) and ply["texcoords"].min() >= 0 and ply["texcoords"].max() <= 1
    assert ply["normals"] is not None and ply["colors"] is None and ply["texture_file"] == "atlas.png"
    assert "texture block 6 atlas %d %d" % (lay.width, lay.height) in ply["comments"]
    want = mesh_io.texture_uv(lay).astype(np.float64)
    assert np.array_equal(ply["texcoords"], np.stack([want[..., 0] / lay.width, 1 - want[..., 1] / lay.height], -1).astype(np.float32))
    obj = mesh_io.read_obj(os.path.join(out_dir, "mesh.obj"))
    assert np.array_equal(obj["vertices"], ply["vertices"]) and np.array_equal(obj["normals"], ply["normals"])
    assert np.array_equal(obj["faces"][..., 0], ply["triangles"]) and np.array_equal(obj["texcoords"], ply["texcoords"].reshape(-1, 2))
    assert mesh_io.read_mtl(os.path.join(out_dir, "mesh.mtl")) == "atlas.png"
    report = json.load(open(out.preview.report))
    assert report["shade"] == "texture" and report["texture"] == {"block": 6, "atlas": [lay.width, lay.height], "file": "atlas.png"}
    assert report["simplified"] is not None and report["n_triangles"] == out.n_triangles
    for row in report["views"] + [report["mean"]]:
        for k in ("psnr_color", "psnr_vertex_color"):
            assert isinstance(row[k], float) and math.isfinite(row[k]), (k, row)
    for i in out.preview.views:
        assert Image.open(os.path.join(out_dir, "preview", "mesh_%d.png" % i)).mode == "RGB"
    print("\n[texture] " + out.preview.summary)
    # without a --texture.* option: the plain export's bytes, and none of the new files
    plain_dir, same_dir = os.path.join(root, "untextured"), os.path.join(root, "untextured_again")
    common = ["--simplify.cell=3", "--surface.normals=true"]
    export.main(args + data + ["--output_path=%s" % plain_dir] + common)
    assert sorted(os.listdir(plain_dir)) == ["cameras.json", "mesh.ply"]
    plain = mesh_io.read_ply_attributes(os.path.join(plain_dir, "mesh.ply"))
    assert np.array_equal(plain["vertices"], ply["vertices"]) and np.array_equal(plain["triangles"], ply["triangles"])
    assert not any(c.startswith(("texture", "TextureFile")) for c in plain["comments"])
    assert plain["comments"] == [c for c in ply["comments"] if not c.startswith(("texture", "TextureFile"))]
    data_plain = open(os.path.join(plain_dir, "mesh.ply"), "rb").read()
    assert b"texcoord" not in data_plain.split(b"end_header\n")[0]
    rewritten = mesh_io.write_ply(os.path.join(root, "rewritten.ply"), plain["vertices"], plain["triangles"], plain["comments"],
                                  normals=plain["normals"])
    assert open(rewritten, "rb").read() == data_plain           # positions, normals, 13-byte faces: the old layout, nothing else
    export.main(args + data + ["--output_path=%s" % same_dir] + common)
    assert open(os.path.join(plain_dir, "mesh.ply"), "rb").read() == open(os.path.join(same_dir, "mesh.ply"), "rb").read()


def test_export_refusals_before_any_gpu_work(tmp_path_factory, tmp_path):
    from joint_tensorf_amd import export
    from tests.test_gpu_preview import _export_args
    root, args, data = _export_args(tmp_path_factory)
    with pytest.raises(SystemExit) as e:
        export.main(args + data + ["--output_path=%s" % tmp_path, "--preview.views=2", "--preview.shade=texture"])
    assert "--texture.block" in str(e.value)
    with pytest.raises(SystemExit) as e:
        export.main(["--yaml=bat_llff_VM_MLP", "--load=%s" % args[1].split("=", 1)[1], "--device=%s" % DEV, "--data.synthetic=true",
                     "--output_path=%s" % tmp_path, "--texture.block=8", "--frame.space=world"])
    assert "--frame.space=world" in str(e.value)
    assert os.listdir(str(tmp_path)) == []
