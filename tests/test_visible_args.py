"""The five visible-surface entry points (include/jt_render.h: jt_visible_tally / jt_visible_fold / jt_visible_mark /
jt_visible_spread / jt_mesh_select_count) refuse bad arguments before anything launches: no GPU needed."""


def test_visible_entry_points_refuse_bad_arguments_without_a_gpu():
    """JT_ERR_ARG (1) for a NULL pointer, a size or count below 1 or min_pixels < 1; JT_ERR_UNSUPPORTED (2) at 2^31 pixels,
    vertices or triangle corners; argument errors come first.  Nothing here reaches a kernel."""
    from joint_tensorf_amd import _lib
    L, p = _lib.lib, 64                     # p: a non-NULL pointer that is never dereferenced on these paths
    corners = 715827883                     # ceil(2^31 / 3) triangles
    # ---- tally ----
    assert L.jt_visible_tally(None, 2, 8, 8, 4, p, None) == 1
    assert L.jt_visible_tally(p, 2, 8, 8, 4, None, None) == 1
    for bad in ((0, 8, 8, 4), (2, 0, 8, 4), (2, 8, 0, 4), (2, 8, 8, 0), (-1, 8, 8, 4), (2, 8, 8, -3)):
        assert L.jt_visible_tally(p, *bad, p, None) == 1, bad
    assert L.jt_visible_tally(p, 2, 32768, 32768, 4, p, None) == 2                # 2^31 pixels
    assert L.jt_visible_tally(p, 32768, 256, 256, 4, p, None) == 2
    assert L.jt_visible_tally(p, 2, 8, 8, corners, p, None) == 2
    assert L.jt_visible_tally(None, 2, 32768, 32768, 4, p, None) == 1             # argument errors come first
    assert L.jt_visible_tally(p, 0, 32768, 32768, corners, p, None) == 1
    # ---- fold ----
    ok = [p, 2, 4, 1, p, p, None]
    for i in (0, 4, 5):
        bad = list(ok)
        bad[i] = None
        assert L.jt_visible_fold(*bad) == 1, i
    assert L.jt_visible_fold(p, 0, 4, 1, p, p, None) == 1
    assert L.jt_visible_fold(p, 2, 0, 1, p, p, None) == 1
    assert L.jt_visible_fold(p, 2, 4, 0, p, p, None) == 1                         # min_pixels < 1
    assert L.jt_visible_fold(p, 2, 4, -5, p, p, None) == 1
    assert L.jt_visible_fold(p, 2, corners, 1, p, p, None) == 2
    assert L.jt_visible_fold(p, 2, corners, 0, p, p, None) == 1
    assert L.jt_visible_fold(p, 2, corners - 1, 1, None, p, None) == 1
    # ---- mark, spread, select: (triangles, n_triangles, n_vertices, pointers ...) ----
    for fn, n_ptr in ((L.jt_visible_mark, 2), (L.jt_visible_spread, 3), (L.jt_mesh_select_count, 3)):
        ok = [p, 8, 6] + [p] * n_ptr + [None]
        for i in [0] + list(range(3, 3 + n_ptr)):
            bad = list(ok)
            bad[i] = None
            assert fn(*bad) == 1, (fn.__name__, i)
        assert fn(*(ok[:1] + [0] + ok[2:])) == 1
        assert fn(*(ok[:2] + [0] + ok[3:])) == 1
        assert fn(*(ok[:1] + [corners] + ok[2:])) == 2
        assert fn(*(ok[:2] + [1 << 31] + ok[3:])) == 2
        assert fn(*([None, corners] + ok[2:])) == 1
        assert fn(*(ok[:1] + [corners, 0] + ok[3:])) == 1


def test_ops_refuse_bad_shapes_before_any_launch():
    import pytest
    import torch
    from joint_tensorf_amd import ops
    V, T, P = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, 4)
    for args, kw in (((V[:, :2], T, P, 8, 8), {}), ((V, T.long(), P, 8, 8), {}), ((V, T, P[0], 8, 8), {}), ((V, T, P[:0], 8, 8), {}),
                     ((V[:0], T, P, 8, 8), {}), ((V, T[:0], P, 8, 8), {}), ((V, T, P, 0, 8), {}), ((V, T, P, 8, 0), {}),
                     ((V, T, P, 8, 8), dict(views_per_call=0)), ((V, T, P, 8, 8), dict(min_pixels=0)),
                     ((V, T, P, 8, 8), dict(min_pixels=1.5)), ((V, T, P, 8, 8), dict(min_pixels=True))):
        with pytest.raises(ValueError):
            ops.triangle_visibility(*args, **kw)
    vis = torch.ones(2, dtype=torch.uint8)
    for args in ((T.long(), 4, vis, 1), (T[:, :2], 4, vis, 1), (T, 4, vis[:1], 1), (T, 4, vis.float(), 1), (T, 4, vis, -1),
                 (T, 4, vis, 1.5), (T, 4, vis, True), (T, -1, vis, 1)):
        with pytest.raises(ValueError):
            ops.grow_triangles(*args)
    out = ops.grow_triangles(T[:0], 4, vis[:0], 3)                                # an empty mesh: nothing launched
    assert out.dtype == torch.uint8 and tuple(out.shape) == (0,)
    for args, kw in (((V[:, :2], T, vis), {}), ((V, T.long(), vis), {}), ((V, T, vis[:1]), {}), ((V, T, vis.int()), {}),
                     ((V, T, vis), dict(normals=V[:3])), ((V, T, vis), dict(colors=V[:, :2]))):
        with pytest.raises(ValueError):
            ops.select_triangles(*args, **kw)
    out = ops.select_triangles(V[:0], T, vis, normals=V[:0])
    assert [None if o is None else tuple(o.shape) for o in out[:4]] == [(0, 3), (0, 3), (0, 3), None] and out[4] == 2
    # extract_mesh's option block, checked before any work
    good = dict(proj=P, H=8, W=8)
    got = ops.visible_options(good)
    assert (got.min_views, got.min_pixels, got.grow, got.cull, got.ndc) == (1, 1, 1, False, None) and got.proj is P
    assert ops.visible_options(dict(good, ndc=(1.5, 2, 1), grow=0)).ndc == (1.5, 2.0, 1.0)
    for bad in (None, {}, dict(proj=P, H=8), dict(good, H=0), dict(good, W=2.5), dict(good, min_views=0), dict(good, min_pixels=0),
                dict(good, grow=-1), dict(good, grow=True), dict(good, ndc=(1, 1)), dict(good, ndc=(1, 0, 1)),
                dict(good, ndc=(1, float("nan"), 1)), dict(good, proj=P[0]), dict(good, rings=2)):
        with pytest.raises(ValueError):
            ops.visible_options(bad)


def test_export_option_group():
    """--visible.* of `python -m joint_tensorf_amd.export`: absent leaves no opt.visible at all; bad values are refused while
    the options are built, before any GPU work"""
    import pytest
    from joint_tensorf_amd import export
    base = ["--yaml=bat_blender_VM"]
    assert "visible" not in export.build_options(base) and "visible" not in export.build_options(base + ["--visible.views=0"])
    opt = export.build_options(base + ["--visible.views=all", "--visible.size=[600,800]", "--visible.min_views=2", "--visible.min_pixels=3",
                                       "--visible.grow=0", "--visible.cull=true"])
    assert dict(opt.visible) == dict(views="all", size=[600, 800], min_views=2, min_pixels=3, grow=0, cull=True)
    opt = export.build_options(["--yaml=bat_llff_VM_MLP", "--visible.views=5", "--visible.size=64", "--texture.block=8"])
    assert dict(opt.visible) == dict(views=5, size=[64, 64], min_views=1, min_pixels=1, grow=1, cull=False) and opt.texture.block == 8
    assert export.build_options(["--yaml=bat_llff_VM_MLP", "--visible.views=5", "--frame.space=world"]).frame.space == "world"
    for bad in (["--visible.grow=2"], ["--visible.views=-1"], ["--visible.views=1.5"], ["--visible.views=some"],
                ["--visible.views=2", "--visible.min_views=0"], ["--visible.views=2", "--visible.min_pixels=0.5"],
                ["--visible.views=2", "--visible.grow=-1"], ["--visible.views=2", "--visible.size=[0,4]"],
                ["--visible.views=2", "--visible.size=[4,4,4]"], ["--visible.views=2", "--visible.cull=1"], ["--visible=3"]):
        with pytest.raises(SystemExit):
            export.build_options(base + bad)
    with pytest.raises(KeyError):
        export.build_options(base + ["--visible.rings=2"])
