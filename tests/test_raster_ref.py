"""The rasteriser's contract on the NumPy reference alone (tests/raster_ref.py), and what needs no device: the fill rule, shared
edges, the near-tie cap of the GPU tests' scenes, the entry points' argument checks, the projection matrices and the
--preview.* options."""
import numpy as np
import pytest

from tests import raster_ref as R


def _screen(xy, w=1.0):
    xy = np.asarray(xy, dtype=np.float32)
    s = np.zeros((len(xy), 4), dtype=np.float32)
    s[:, :2], s[:, 2], s[:, 3] = xy, 1.0 / w, w
    return s


def test_quads_split_along_either_diagonal_cover_their_union_once():
    """200 random convex quads of either winding, split along a-c and along b-d: a pixel whose centre lies strictly inside the
    snapped quad is covered exactly once, one strictly outside never, one on its boundary at most once -- and a vertex, an
    edge or the diagonal through a pixel centre (every fifth quad has half-integer corners) changes nothing about that"""
    g = np.random.default_rng(1)
    H = W = 24
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cx, cy = R.SUB * px + R.SUB // 2, R.SUB * py + R.SUB // 2
    for n in range(200):
        c = 6 + 12 * g.random(2)
        ang = (np.arange(4) + 0.15 + 0.7 * g.random(4)) * (np.pi / 2) + g.random() * 6       # one corner per quadrant of an
        quad = c + (2.0 + 8.0 * g.random(2)) * np.stack([np.cos(ang), np.sin(ang)], -1)        # ellipse: convex
        if n % 2:
            quad = quad[::-1]
        if n % 5 == 0:
            quad = np.rint(quad * 2) / 2
        screen = _screen(quad)
        X, Y, inside = R.snap(screen)
        assert inside.all()
        e = np.stack([(X[(k + 1) % 4] - X[k]) * (cy - Y[k]) - (Y[(k + 1) % 4] - Y[k]) * (cx - X[k]) for k in range(4)])
        e = e * int(np.sign(sum(X[k] * Y[(k + 1) % 4] - X[(k + 1) % 4] * Y[k] for k in range(4))))   # inside-positive
        strictly_in, strictly_out = (e > 0).all(0), (e < 0).any(0)
        assert strictly_in.sum() > 0
        for split in ([[0, 1, 2], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]]):
            ref = R.rasterize(screen, np.array(split), H, W)
            assert (ref["status"] == R.DRAWN).all()
            assert ref["cover"].max() <= 1, (n, split)
            assert (ref["cover"][strictly_in] == 1).all() and (ref["cover"][strictly_out] == 0).all(), (n, split)
            assert ((ref["tri"] >= 0) == (ref["cover"] == 1)).all()


def test_fan_round_a_pixel_centre_covers_every_pixel_once():
    s = R.fan_scene()
    ref = R.rasterize(R.project(s["vertices"], s["proj"])[0].astype(np.float32), s["triangles"], s["H"], s["W"])
    assert (ref["status"] == R.DRAWN).all() and ref["cover"].max() == 1
    assert ref["cover"][16, 16] == 1                                  # the pixel whose centre IS the shared vertex
    # the union is the octagon: a pixel strictly inside it is covered (the centre's pixel ring at least)
    assert (ref["cover"][10:23, 10:23] == 1).all()
    # the reversed fan (the other winding) covers exactly the same pixels
    rev = R.rasterize(R.project(s["vertices"], s["proj"])[0].astype(np.float32), s["triangles"][:, ::-1], s["H"], s["W"])
    assert np.array_equal(rev["cover"], ref["cover"])


def test_top_left_rule():
    """a vertex, a vertical left / right edge and a horizontal top / bottom edge exactly through pixel centres"""
    # the axis-aligned right triangle (2.5, 2.5), (6.5, 2.5), (2.5, 6.5): top edge y = 2.5, left edge x = 2.5, both through centres
    ref = R.rasterize(_screen([(2.5, 2.5), (6.5, 2.5), (2.5, 6.5)]), np.array([[0, 1, 2]]), 8, 8)
    got = {(x, y) for y, x in zip(*np.nonzero(ref["cover"]))}
    # centres (i + .5, j + .5) with i, j >= 2 (the top and the left edge are in) and strictly on this side of the hypotenuse x + y = 9
    want = {(i, j) for i in range(2, 8) for j in range(2, 8) if (i + 0.5) + (j + 0.5) < 9.0}
    assert got == want and (2, 2) in got and (6, 2) not in got and (2, 6) not in got
    # the mirror image (6.5, 6.5), (2.5, 6.5), (6.5, 2.5): its bottom edge y = 6.5 and right edge x = 6.5 are out, and the
    # hypotenuse, which bounds it on the left, is in: the centres ON x + y = 9 that the first triangle left out
    ref = R.rasterize(_screen([(6.5, 6.5), (2.5, 6.5), (6.5, 2.5)]), np.array([[0, 1, 2]]), 8, 8)
    got = {(x, y) for y, x in zip(*np.nonzero(ref["cover"]))}
    want = {(i, j) for i in range(2, 6) for j in range(2, 6) if (i + 0.5) + (j + 0.5) >= 9.0}
    assert got == want
    # together the two tile the square [2.5, 6.5)^2: 16 pixels, each once, the hypotenuse's pixels going to exactly one of them
    both = R.rasterize(_screen([(2.5, 2.5), (6.5, 2.5), (2.5, 6.5), (6.5, 6.5)]), np.array([[0, 1, 2], [3, 2, 1]]), 8, 8)
    assert both["cover"].max() == 1 and int(both["cover"].sum()) == 16 and (both["cover"][2:6, 2:6] == 1).all()
    # a lone vertex on a pixel centre: the apex (4.5, 1.5) of a triangle pointing up is the meeting of a left and a right edge: out;
    # the top-left corner of a square is the meeting of a top and a left edge: in
    up = R.rasterize(_screen([(4.5, 1.5), (7.5, 6.0), (1.5, 6.0)]), np.array([[0, 1, 2]]), 8, 8)
    assert up["cover"][1, 4] == 0 and up["cover"][2, 4] == 1
    # the same triangle given as its sub-pixel integers
    ints = R.rasterize(_screen([(0, 0)] * 3), np.array([[0, 1, 2]]), 8, 8, snapped=([1152, 1920, 384], [384, 1536, 1536]))
    assert np.array_equal(ints["cover"], up["cover"])
    # both windings give the same pixels
    flip =R.rasterize(_screen([(4.5, 1.5), (1.5, 6.0), (7.5, 6.0)]), np.array([[0, 1, 2]]), 8, 8)
    assert np.array_equal(flip["cover"], up["cover"])


def test_status_codes_and_cull():
    s = _screen([(1.0, 1.0), (5.0, 1.0), (1.0, 5.0), (3.0, 3.0), (2e4, 1.0)])
    s[3, 2] = 0.0                                                     # vertex 3: behind near
    T = np.array([[0, 1, 2], [0, 2, 1], [0, 1, 3], [0, 1, 4], [0, 1, 1], [0, 1, 7]])
    ref = R.rasterize(s, T, 8, 8)
    assert list(ref["status"]) == [R.DRAWN, R.DRAWN, R.NEAR, R.GUARD_BAND, R.EMPTY, R.NEAR]
    ref = R.rasterize(s, T, 8, 8, cull=True)
    assert list(ref["status"]) == [R.CULLED, R.DRAWN, R.NEAR, R.GUARD_BAND, R.EMPTY, R.NEAR]   # positive area: a back face


@pytest.mark.parametrize("name", sorted(R.COVERAGE_SCENES) + sorted(R.DEPTH_SCENES))
def test_near_tie_cap_of_the_gpu_scenes(name):
    """Where the reference's best and second-best q differ by less than 1e-5 relative an fp32 rasteriser may pick the other
    triangle; the GPU tests allow that at no more than MAX_NEAR_TIES pixels, and the scenes are built to stay below it: the
    coverage scenes (compared bit for bit) have none.  The duplicate scene ties everywhere BY CONSTRUCTION (the same triangle
    thrice) and is held to the lower index exactly instead; its cap is taken with the copies removed."""
    s = (R.COVERAGE_SCENES.get(name) or R.DEPTH_SCENES[name])()
    T = s["triangles"][:1] if name == "duplicate" else s["triangles"]
    screen = R.project(s["vertices"], s["proj"])[0].astype(np.float32)
    ref = R.rasterize(screen, T, s["H"], s["W"])
    n = int(R.near_ties(ref).sum())
    print("%s: %d triangles, %d covered pixels, %d near ties" % (name, len(T), int((ref["tri"] >= 0).sum()), n))
    assert (ref["tri"] >= 0).sum() > 0
    assert n <= (0 if name in R.COVERAGE_SCENES else R.MAX_NEAR_TIES)
    if name == "mixed":
        assert len(T) == 130 and (ref["status"] == R.DRAWN).all()
        big = [int(((ref_one["cover"]) > 0).sum()) for ref_one in
               (R.rasterize(screen, T[k:k + 1], s["H"], s["W"]) for k in (5, 70))]
        assert big == [s["H"] * s["W"]] * 2                            # the two that cover the screen
    if name == "big":
        assert 0 < (ref["tri"] >= 0).sum() < s["H"] * s["W"] and R.snap(screen)[2].all()
        off = (screen[:, 0] < 0) | (screen[:, 0] > s["W"]) | (screen[:, 1] < 0) | (screen[:, 1] > s["H"])
        assert off.all()                                               # every vertex off the image, inside the guard band


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """JT_ERR_ARG (1) for a NULL pointer, a size below 1 and a non-finite near; JT_ERR_UNSUPPORTED (2) when n_views * H * W or
    n_triangles reaches 2^31, H or W exceeds 16384 or there are more than 8 attributes.  Nothing here reaches a kernel."""
    import ctypes
    from joint_tensorf_amd import _lib
    L, p = _lib.lib, 64                     # p: a non-NULL pointer that is never dereferenced on these paths
    bg = (ctypes.c_float * 8)()
    assert L.jt_raster_project(None, 4, p, 1, 0.1, p, None) == 1
    assert L.jt_raster_project(p, 4, None, 1, 0.1, p, None) == 1
    assert L.jt_raster_project(p, 4, p, 1, 0.1, None, None) == 1
    assert L.jt_raster_project(p, 0, p, 1, 0.1, p, None) == 1
    assert L.jt_raster_project(p, 4, p, 0, 0.1, p, None) == 1
    assert L.jt_raster_project(p, 4, p, 1, float("nan"), p, None) == 1
    assert L.jt_raster_project(p, 4, p, 1, float("inf"), p, None) == 1

    def draw(screen=p, nv=4, tris=p, nt=2, V=1, H=8, W=8, zbuf=p, status=p):
        return L.jt_raster_draw(screen, nv, tris, nt, V, H, W, 0, zbuf, status, None)
    assert draw(screen=None) == 1 and draw(tris=None) == 1 and draw(zbuf=None) == 1 and draw(status=None) == 1
    assert draw(nv=0) == 1 and draw(nt=0) == 1 and draw(V=0) == 1 and draw(H=0) == 1 and draw(W=-3) == 1
    assert draw(nt=1 << 31) == 2 and draw(H=16385) == 2 and draw(W=16385) == 2
    assert draw(V=8, H=16384, W=16384) == 2 and draw(V=2, H=32768, W=32768) == 2

    def resolve(zbuf=p, screen=p, nv=4, tris=p, nt=2, V=1, H=8, W=8, attrs=p, C=3, background=bg, tri=p, depth=p, out=p):
        return L.jt_raster_resolve(zbuf, screen, nv, tris, nt, V, H, W, attrs, C, background, tri, depth, out, None)
    for k in ("zbuf", "screen", "tris", "attrs", "background", "tri", "depth", "out"):
        assert resolve(**{k: None}) == 1, k
    assert resolve(nv=0) == 1 and resolve(nt=0) == 1 and resolve(V=0) == 1 and resolve(H=0) == 1 and resolve(C=-1) == 1
    assert resolve(C=9) == 2 and resolve(nt=1 << 31) == 2 and resolve(W=16385) == 2 and resolve(V=8, H=16384, W=16384) == 2


def test_projection_matrices():
    torch = pytest.importorskip("torch")
    from joint_tensorf_amd import mesh_io
    g = torch.Generator().manual_seed(0)
    R3 = torch.linalg.qr(torch.randn(2, 3, 3, generator=g)).Q
    pose = torch.cat([R3, torch.randn(2, 3, 1, generator=g)], -1)
    intr = torch.tensor([[[50.0, 0, 16], [0, 40.0, 12], [0, 0, 1]]]).repeat(2, 1, 1)
    P = mesh_io.projection_matrices(pose, intr)
    assert tuple(P.shape) == (2, 3, 4) and torch.allclose(P, intr @ pose, atol=1e-5)
    # rendering at twice the width and half the height: x scales by 2, y by 1/2 (datasets.py's resize of the intrinsics)
    Ps = mesh_io.projection_matrices(pose, intr, size=(12, 64), image_size=(24, 32))
    want = torch.tensor([2.0, 0.5, 1.0])[None, :, None] * (intr @ pose)
    assert torch.allclose(Ps, want, atol=1e-5)
    assert torch.equal(mesh_io.projection_matrices(pose, intr, size=(24, 32), image_size=(24, 32)), P)
    with pytest.raises(ValueError):
        mesh_io.projection_matrices(pose, intr, size=(12, 64))            # a size without the size the intrinsics belong to
    with pytest.raises(ValueError):
        mesh_io.projection_matrices(pose[:1], intr)


def test_preview_option_parsing():
    from joint_tensorf_amd import export
    base = ["--yaml=bat_blender_VM", "--load=a.ckpt", "--output_path=out"]
    opt = export.build_options(base)
    assert dict(opt.preview) == dict(views=0, size=None, shade="color", check=False, cull=False)
    opt = export.build_options(base + ["--preview.views=3", "--preview.size=[40,48]", "--preview.shade=normal",
                                       "--preview.check=true", "--preview.cull=true"])
    assert dict(opt.preview) == dict(views=3, size=[40, 48], shade="normal", check=True, cull=True)
    assert export.build_options(base + ["--preview.views=all"]).preview.views == "all"
    assert export.build_options(base + ["--preview.views=1", "--preview.size=64"]).preview.size == [64, 64]
    for bad in (["--preview.views=-1"], ["--preview.views=2.5"], ["--preview.views=some"], ["--preview.size=[4]"],
                ["--preview.size=0"], ["--preview.size=[20000,4]"], ["--preview.shade=phong"], ["--preview.check=maybe"],
                ["--preview.cull=1"], ["--preview=2"], ["--preview.check=true"], ["--preview.shade=depth"]):
        with pytest.raises(SystemExit):
            export.build_options(base + bad)
    with pytest.raises(KeyError):
        export.build_options(base + ["--preview.view=2"])
