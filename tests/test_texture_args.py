"""The three texture entry points (include/jt_render.h: jt_texture_texels / jt_texture_pack / jt_raster_resolve_texture) refuse
bad arguments before anything launches: no GPU needed."""
import ctypes

import pytest


def test_texture_entry_points_refuse_bad_arguments_without_a_gpu():
    """JT_ERR_ARG (1) for a NULL pointer, a size or count below 1, a negative start, an entry range beyond the atlas, an atlas that
    is not cols x rows whole blocks or holds fewer charts than triangles; JT_ERR_UNSUPPORTED (2) for S outside 4 .. 64, an atlas
    side beyond 16384 and the 2^31 limits.  Argument errors come first.  Nothing here reaches a kernel."""
    from joint_tensorf_amd import _lib
    L, p = _lib.lib, 64                     # p: a non-NULL pointer that is never dereferenced on these paths
    # ---- texels: (vertices, normals, nv, triangles, nt, S, cols, start, count, xyz, dirs, valid, stream) ----
    ok = [p, p, 9, p, 5, 8, 2, 0, 3 * 64, p, p, p, None]
    for i in (0, 1, 3, 9, 10, 11):
        bad = list(ok)
        bad[i] = None
        assert L.jt_texture_texels(*bad) == 1, i
    for i, v in ((2, 0), (4, 0), (6, 0), (7, -1), (8, 0)):
        bad = list(ok)
        bad[i] = v
        assert L.jt_texture_texels(*bad) == 1, (i, v)
    for S in (3, 65, 0, -8):
        bad = list(ok)
        bad[5] = S
        assert L.jt_texture_texels(*bad) == 2, S
    assert L.jt_texture_texels(p, p, 9, p, 5, 8, 2, 1, 3 * 64, p, p, p, None) == 1            # one entry past the third block
    assert L.jt_texture_texels(p, p, 9, p, 5, 8, 2049, 0, 64, p, p, p, None) == 2             # 2049 blocks of 8: 16392 texels wide
    assert L.jt_texture_texels(p, p, 9, p, 2 * 2048 * 2048 + 1, 8, 2048, 0, 64, p, p, p, None) == 2      # a 2049th row of blocks
    assert L.jt_texture_texels(p, p, 1 << 31, p, 5, 8, 2, 0, 64, p, p, p, None) == 2
    assert L.jt_texture_texels(p, p, 9, p, 715827883, 4, 16384, 0, 64, p, p, p, None) == 2    # ceil(2^31 / 3) triangles
    n_blocks = (1 << 31) // (64 * 64)                                                          # 2^19 blocks of 64 x 64: 2^31 entries
    assert L.jt_texture_texels(p, p, 9, p, 2 * n_blocks, 64, 256, 0, 64, p, p, p, None) == 2
    assert L.jt_texture_texels(None, p, 1 << 31, p, 5, 3, 2, 0, 64, p, p, p, None) == 1       # argument errors come first
    assert L.jt_texture_texels(p, p, 9, p, 5, 65, 2, 0, 0, p, p, p, None) == 1
    # ---- pack: (rgb, valid, S, cols, start, count, atlas, H_atlas, W_atlas, stream) ----
    ok = [p, p, 8, 2, 0, 3 * 64, p, 16, 16, None]
    for i in (0, 1, 6):
        bad = list(ok)
        bad[i] = None
        assert L.jt_texture_pack(*bad) == 1, i
    for i, v in ((3, 0), (4, -1), (5, 0), (7, 0), (8, 0)):
        bad = list(ok)
        bad[i] = v
        assert L.jt_texture_pack(*bad) == 1, (i, v)
    for S in (3, 65):
        assert L.jt_texture_pack(p, p, S, 2, 0, 64, p, 2 * S, 2 * S, None) == 2, S
    assert L.jt_texture_pack(p, p, 8, 2, 0, 64, p, 16, 17, None) == 1                         # W_atlas is not cols S
    assert L.jt_texture_pack(p, p, 8, 2, 0, 64, p, 17, 16, None) == 1                         # H_atlas is no multiple of S
    assert L.jt_texture_pack(p, p, 8, 2, 1, 4 * 64, p, 16, 16, None) == 1                     # one entry past the atlas
    assert L.jt_texture_pack(p, p, 8, 2049, 0, 64, p, 16, 2049 * 8, None) == 2
    assert L.jt_texture_pack(p, p, 8, 2, 0, 64, p, 16392, 16, None) == 2
    assert L.jt_texture_pack(None, p, 3, 2, 0, 64, p, 16, 16, None) == 1
    # ---- resolve: (zbuf, screen, nv, triangles, nt, V, H, W, atlas, S, cols, H_atlas, W_atlas, background, tri, depth, out, stream) ----
    bg = (ctypes.c_float * 3)(0, 0, 0)
    ok = [p, p, 9, p, 5, 1, 4, 4, p, 8, 2, 16, 16, bg, p, p, p, None]
    assert L.jt_raster_resolve_texture(*(ok[:4] + [9] + ok[5:])) == 1                         # nine triangles, charts for eight
    for i in (0, 1, 3, 8, 13, 14, 15, 16):
        bad = list(ok)
        bad[i] = None
        assert L.jt_raster_resolve_texture(*bad) == 1, i
    for i in (2, 4, 5, 6, 7, 10, 11, 12):
        bad = list(ok)
        bad[i] = 0
        assert L.jt_raster_resolve_texture(*bad) == 1, i
    for S in (3, 65):
        bad = list(ok)
        bad[9], bad[11], bad[12] = S, 2 * S, 2 * S
        assert L.jt_raster_resolve_texture(*bad) == 2, S
    for i, v in ((4, 1 << 31), (5, 65536), (6, 16385), (7, 16385), (11, 16392), (12, 16392)):
        bad = list(ok)
        bad[i] = v
        assert L.jt_raster_resolve_texture(*bad) == 2, (i, v)
    assert L.jt_raster_resolve_texture(*(ok[:5] + [8, 16384, 16384] + ok[8:])) == 2           # n_views H W = 2^31
    assert L.jt_raster_resolve_texture(*(ok[:11] + [16, 17] + ok[13:])) == 1
    assert L.jt_raster_resolve_texture(*(ok[:11] + [17, 16] + ok[13:])) == 1
    assert L.jt_raster_resolve_texture(*([None] + ok[1:9] + [65] + ok[10:])) == 1


def test_ops_refuses_bad_shapes_before_any_launch():
    import torch
    from joint_tensorf_amd import ops
    V, T, N = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    lay = ops.texture_layout(2, 4)
    assert lay.n_entries == 16 and (lay.width, lay.height) == (4, 4)
    for args in ((V[:, :2], T, N, lay), (V, T.long(), N, lay), (V, T, N[:3], lay), (V, T[:1], N, lay), (V, T, N, lay, -1, 4),
                 (V, T, N, lay, 0, 0), (V, T, N, lay, 1, 16), (V, T, N, lay, 16)):
        with pytest.raises(ValueError):
            ops.texture_texels(*args)
    atlas, rgb, valid = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(16, 3), torch.ones(16, dtype=torch.uint8)
    for args in ((rgb[:, :2], valid, lay, atlas), (rgb, valid[:3], lay, atlas), (rgb, valid.float(), lay, atlas),
                 (rgb, valid, lay, atlas.float()), (rgb, valid, lay, atlas[:3]), (rgb, valid, lay, atlas, 1)):
        with pytest.raises(ValueError):
            ops.texture_pack(*args)
    P = torch.zeros(1, 3, 4)
    with pytest.raises(ValueError):
        ops.rasterize(V, T, P, 4, 4, attrs=N, texture=(atlas, lay))                           # attrs and texture exclude each other
    with pytest.raises(ValueError):
        ops.rasterize(V, T, P, 4, 4, texture=(atlas, ops.texture_layout(3, 4)))
    with pytest.raises(ValueError):
        ops.rasterize(V, T, P, 4, 4, texture=(atlas.float(), lay))
