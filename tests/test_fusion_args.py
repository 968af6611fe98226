"""Depth-map fusion refuses what it cannot do before anything launches: the two entry points (include/jt_render.h:
jt_fusion_integrate / jt_fusion_finish), the mesh_ops wrappers, extract_mesh(fusion=) and --fusion.* of the export.  No GPU needed."""
import pytest


def test_fusion_entry_points_refuse_bad_arguments_without_a_gpu():
    """JT_ERR_ARG (1) for a NULL pointer, a lattice axis below 2, n_views < 0, H or W < 1, a trunc that is not positive and finite,
    a NaN threshold, min_views < 1; JT_ERR_UNSUPPORTED (2) beyond 2^27 lattice points or at 2^31 pixels; n_views == 0 is JT_OK and
    launches nothing.  Nothing here reaches a kernel."""
    import ctypes
    from joint_tensorf_amd import _lib
    L, p = _lib.lib, 64                     # p: a non-NULL pointer that is never dereferenced on these paths
    box = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    lo, hi = (ctypes.cast(b, ctypes.c_void_p) for b in box)
    nan = float("nan")

    def call(depth=p, opacity=p, proj=p, V=2, H=8, W=8, nx=4, ny=4, nz=4, lo=lo, hi=hi, trunc=0.5, a=0.5, carve=1, near=1e-3, acc=p, count=p):
        return L.jt_fusion_integrate(depth, opacity, proj, V, H, W, nx, ny, nz, lo, hi, trunc, a, carve, near, acc, count, None)
    for bad in (dict(depth=None), dict(opacity=None), dict(proj=None), dict(lo=None), dict(hi=None), dict(acc=None), dict(count=None),
                dict(V=-1), dict(H=0), dict(W=0), dict(nx=1), dict(ny=1), dict(nz=0), dict(trunc=0.0), dict(trunc=-1.0),
                dict(trunc=float("inf")), dict(trunc=nan), dict(a=nan), dict(near=nan)):
        assert call(**bad) == 1, bad
    assert call(nx=513, ny=512, nz=512) == 2                                      # beyond 2^27 points
    assert call(V=2, H=32768, W=32768) == 2                                       # 2^31 pixels
    assert call(V=32768, H=256, W=256) == 2
    assert call(nx=513, ny=512, nz=512, acc=None) == 1                            # argument errors come first
    assert call(V=0, depth=None, opacity=None, proj=None) == 0                    # nothing to add: nothing launched
    assert call(V=0, acc=None) == 1
    ok = [p, p, 64, 1, p, p, None]
    for i in (0, 1, 4, 5):
        bad = list(ok)
        bad[i] = None
        assert L.jt_fusion_finish(*bad) == 1, i
    assert L.jt_fusion_finish(p, p, 0, 1, p, p, None) == 1
    assert L.jt_fusion_finish(p, p, 64, 0, p, p, None) == 1                       # min_views < 1
    assert L.jt_fusion_finish(p, p, (1 << 27) + 1, 1, p, p, None) == 2


def test_mesh_ops_refuse_bad_shapes_before_any_launch():
    import torch
    from joint_tensorf_amd import mesh_ops, ops
    assert ops.fusion_integrate is mesh_ops.fusion_integrate and ops.mesh_from_fused_lattice is mesh_ops.mesh_from_fused_lattice
    acc, count = mesh_ops.fusion_state((3, 4, 5), "cpu")
    assert acc.dtype == torch.float32 and count.dtype == torch.int32 and tuple(acc.shape) == tuple(count.shape) == (3, 4, 5)
    assert not acc.any() and not count.any()
    for shape in ((3, 4), (1, 4, 5), (3, 4, 5, 6)):
        with pytest.raises(ValueError):
            mesh_ops.fusion_state(shape, "cpu")
    d, a, P = torch.ones(2, 6, 8), torch.ones(2, 6, 8), torch.zeros(2, 3, 4)
    lo, hi = (-1, -1, -1), (1, 1, 1)
    good = ((acc, count), d, a, P, lo, hi, 0.5)
    for i, bad in ((0, acc), (0, (acc, count.float())), (0, (acc, count[:2])), (0, (acc[0], count[0])), (1, d[0]), (2, a[:1]), (3, P[:1]),
                   (3, P[0]), (4, (0, 0)), (6, 0.0), (6, -1.0), (6, float("inf")), (6, float("nan"))):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            mesh_ops.fusion_integrate(*args)
    for kw in (dict(min_opacity=float("nan")), dict(near=float("nan"))):
        with pytest.raises(ValueError):
            mesh_ops.fusion_integrate(*good, **kw)
    assert mesh_ops.fusion_integrate((acc, count), d[:0], a[:0], P[:0], lo, hi, 0.5)[0] is acc      # no views: nothing launched
    for mv in (0, 1.5, True, -1):
        with pytest.raises(ValueError):
            mesh_ops.fusion_lattice((acc, count), mv)
    # extract_mesh's option block, checked before any work
    opt = mesh_ops.fusion_options(dict(depth=d, opacity=a, proj=P, H=6, W=8))
    assert (opt.H, opt.W, opt.trunc, opt.min_opacity, opt.min_views, opt.carve) == (6, 8, 4.0, 0.5, 1, True) and len(opt.slabs) == 1
    gen = ((d, a, P) for _ in range(2))
    assert mesh_ops.fusion_options(dict(slabs=gen, H=6, W=8, trunc=2, min_opacity=1, min_views=2, carve=False)).slabs is gen
    base = dict(depth=d, opacity=a, proj=P, H=6, W=8)
    for bad in (None, {}, dict(depth=d, opacity=a, proj=P, H=6), dict(base, H=5), dict(base, W=0), dict(base, trunc=0), dict(base, trunc=-4),
                dict(base, trunc=float("nan")), dict(base, min_views=0), dict(base, min_views=1.5), dict(base, min_opacity=0),
                dict(base, min_opacity=1.5), dict(base, slabs=[(d, a, P)]), dict(H=6, W=8), dict(depth=d, opacity=a, H=6, W=8),
                dict(base, proj=P[:1]), dict(base, level=0.5)):
        with pytest.raises(ValueError):
            mesh_ops.fusion_options(bad)


def test_extract_mesh_refuses_a_level_with_fusion():
    """the fused surface is the level 0.5 of the fused lattice: a level passed with fusion is a ValueError, raised before the
    field is touched (`self` is never looked at)"""
    import torch
    from joint_tensorf_amd import tensorf_repr
    d, a, P = torch.ones(2, 6, 8), torch.ones(2, 6, 8), torch.zeros(2, 3, 4)
    with pytest.raises(ValueError) as e:
        tensorf_repr.TensorVMSplit.extract_mesh(None, res=8, level=0.5, fusion=dict(depth=d, opacity=a, proj=P, H=6, W=8))
    assert "level" in str(e.value)
    with pytest.raises(ValueError) as e:
        tensorf_repr.TensorVMSplit.extract_mesh(None, res=8, fusion=dict(depth=d, opacity=a, proj=P, H=6, W=8, trunc=0))
    assert "trunc" in str(e.value)
    assert tensorf_repr.Mesh._fields[-1] == "fused" and tensorf_repr.Mesh(*range(6)).fused is None


def test_export_option_group():
    """--fusion.* of `python -m joint_tensorf_amd.export`: absent leaves no opt.fusion at all; bad values, camera.ndc scenes and a
    --mesh.level are refused while the options are built, before any GPU work"""
    from joint_tensorf_amd import export
    from joint_tensorf_amd.options import Opt
    base = ["--yaml=bat_blender_VM"]
    assert "fusion" not in export.build_options(base) and "fusion" not in export.build_options(base + ["--fusion.views=0"])
    opt = export.build_options(base + ["--fusion.views=all", "--fusion.size=[400,400]", "--fusion.trunc=3", "--fusion.min_opacity=0.7",
                                       "--fusion.min_views=2", "--fusion.carve=false", "--fusion.views_per_call=4"])
    assert dict(opt.fusion) == dict(views="all", size=[400, 400], trunc=3.0, min_opacity=0.7, min_views=2, carve=False, views_per_call=4)
    opt = export.build_options(base + ["--fusion.views=5", "--fusion.size=64", "--visible.views=all", "--simplify.cell=4", "--texture.block=8"])
    assert dict(opt.fusion) == dict(views=5, size=[64, 64], trunc=4.0, min_opacity=0.5, min_views=1, carve=True, views_per_call=8)
    for bad in (["--fusion.trunc=2"], ["--fusion.views=-1"], ["--fusion.views=1.5"], ["--fusion.views=some"],
                ["--fusion.views=2", "--fusion.trunc=0"], ["--fusion.views=2", "--fusion.trunc=-1"], ["--fusion.views=2", "--fusion.min_views=0"],
                ["--fusion.views=2", "--fusion.min_opacity=0"], ["--fusion.views=2", "--fusion.min_opacity=1.01"],
                ["--fusion.views=2", "--fusion.size=[0,4]"], ["--fusion.views=2", "--fusion.carve=1"],
                ["--fusion.views=2", "--fusion.views_per_call=0"], ["--fusion.views=2", "--mesh.level=0.01"], ["--fusion=3"]):
        with pytest.raises(SystemExit):
            export.build_options(base + bad)
    with pytest.raises(KeyError):
        export.build_options(base + ["--fusion.bilinear=true"])
    with pytest.raises(SystemExit) as e:
        export.build_options(["--yaml=bat_llff_VM_MLP", "--fusion.views=2"])
    assert "camera.ndc" in str(e.value) and "not built" in str(e.value)
    # _check_fusion itself, on the group
    good = Opt(export.FUSION_DEFAULTS)
    good.views = 3
    export._check_fusion(good)
    for key, value in (("trunc", 0), ("min_views", 0), ("min_opacity", 0.0), ("min_opacity", 2), ("views", 0)):
        bad = Opt(export.FUSION_DEFAULTS)
        bad.views = 3
        bad[key] = value
        with pytest.raises(SystemExit):
            export._check_fusion(bad)
    with pytest.raises(SystemExit):
        export._check_fusion(good, ndc=True)
    # no image set: refused by main before a model is built
    with pytest.raises(SystemExit) as e:
        export.main(base + ["--fusion.views=2", "--load=nowhere.ckpt", "--output_path=nowhere"])
    assert "image set" in str(e.value)
