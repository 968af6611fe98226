"""The alpha mask's in-kernel test, mask_keep (csrc/jt_common.h), held to the pinned reference of tests/mask_ref.py on every
path that reads it: k_dense_alpha directly, sample_valid in k_march_fwd<false | true>, and the second decision of
k_march_bwd_scan<0 | 1 | 2>.  After the first updateAlphaMask + shrink every training step, evaluation render and
test-time pose step runs with a mask; the rest of the suite only meets one through a cubic 20^3 fixture at whole-tensor
tolerances.

1. test_dense_alpha_probe: a thin blender scene (P.build_scene, positive density factors; the unmasked one-step opacity at
   length 1 is asserted above 1e-3 everywhere in the box and positive everywhere, so alpha == 0 exactly iff the point was
   dropped), a hand-made non-cubic AlphaGridMask, ~22 800 points of the families of mask_ref.probe_points: (alpha > 0)
   equals mask_ref.keep on EVERY point, and a kept point has the unmasked run's value bit for bit.  Volumes: one set voxel
   at (1, 2, 3); all set but one; 40 % random.  Boxes: the scene's own (dims 7 x 5 x 19), and the post-shrink state (dims
   9 x 5 x 17 over the old, larger box with power-of-two pitches; the scene lies 1.75 / 1.375 / 3.25 cells inside it).
   Family counts (floors in mask_ref.FLOORS, counted from mask_ref.cells alone, also held on the CPU by
   tests/test_mask_ref.py): shrunk interior 12 651, node1 5 241, node2 1 200, node3 1 200, face_lo 2 091, face_hi 2 305,
   outside_near 1 308, outside_far 1 200, ulp 770; same 13 047, 5 433, 1 286, 496, 2 121, 2 408, 1 338, 1 200, 2 392.
2. The masked march: one iteration on GRID = [12, 9, 72], 84 rays of the mixed families (mask_ref.march_rays), S = 151,
   the post-shrink box with mask_ref.march_volume, judged by _check_row (training form; blender, llff, blender in
   deterministic mode) and _check_pose (pose-only form, both kinds, ops.POSE_MARCH_DERIVATIVES on and off) with their
   own bounds, imported: TOL_VAL, TOL_DEPTH, KAPPA with zero stray writes, DENSE_TOL, RAY_RTOL / RAY_ATOL.  The reference
   renders with the mask, its decision pinned to mask_ref.keep (pinned_ref._pinned_mask_sample).  Input conditions, from
   the reference side (mask_ref.march_census; counted: 6 726 in-box samples, 3 924 dropped, 2 802 kept, 28 rays with
   every sample dropped, 26 rays with a gap between two kept runs, 685 kept samples on a far node): >= 20 % dropped,
   >= 20 % kept, >= 4 all-dropped rays -- background out, every gradient exactly zero on both sides --, >= 8 gap rays,
   >= 1 kept far-node sample.
3. test_march_forward_direct: jt_march_forward itself: sigma_feat != 0 exactly at the kept samples, no dropped sample in
   the shade list.  test_blur_ignores_mask: with a blur active the mask is not consulted: values and (deterministic
   mode: order-independent sums) gradients equal the unmasked call bit for bit.

A BUG THESE ROWS FOUND, fixed with them: mask_keep took the fraction as `ix - floorf(ix)`, which the compiler contracts
into v_fma_f32(h, size - 1, -floor): the fraction of the UNROUNDED product.  Where ix rounds onto a node from above that
is a tiny positive number instead of 0, the upper corner counts, and a point the reference (grid_sample, which takes the
fraction of the rounded ix) drops is kept.  Against the library as it was: test_dense_alpha_probe[same-random] fails with
323 points kept that the reference drops (none the other way), [same-full-but-one] with 3 (the point on the cleared
voxel's node), and the masked getDenseAlpha added to test_alpha_mask_update_and_shrink_vs_golden with 28 of the 8 000
lattice points of the 20^3 fixture -- every lattice point of a mask update sits on a node of the previous mask.  The box
with 6, 4 and 18 cells makes the product round; the power-of-two box cannot show it, and its rows passed.  The fraction
is now add_rn(ix, -fl), the rounded one.

MEASURED on MI355X (all 16 tests green, 4.4 s of pytest for the file, no test above 2.4 s), worst over the seven masked
march rows next to the imported bound: per-element factor ratio density planes 15 (KAPPA 5 200), density lines 7 (2 400),
appearance lines 18 (8 000), appearance planes 5 339 (blender-det, app_plane.1; 1 597 blender, 122 llff; 120 000), no
stray write; basis / MLP gradients 6.0e-7 (DENSE_TOL 5e-5); every ray-gradient element within RAY_RTOL |t| with no
absolute term at all (RAY_ATOL 1e-6), training and pose-only form alike; rgb 1.5e-7, opacity 2.6e-7 (TOL_VAL 3e-5), depth
6.5e-7 (TOL_DEPTH 2e-4).  All 2 802 kept samples were shaded, 685 of them on a far node, in 45 of the 88 gather tiles.

DELIBERATE BREAKS, scratch builds that are not part of the repository, this file run against each:
  * the `w > 0.f` term dropped from mask_keep: 15 of 16 fail -- all six probe rows (kept though the reference drops: 59,
    3, 980 on the scene's box; 55, 1, 1 399 on the post-shrink box; single, full-but-one, random), every masked march row
    and both direct march rows (the samples of the rays along z sit on the mask's z node planes); only the blur row
    passes, as it must.  The golden test's masked getDenseAlpha fails as well.
  * the x and y entries of mask_dims swapped in RenderCfg.scene(): all 16 fail (the blur row on its last line, that the
    mask acts once the blur is off).  The cubic fixture of the golden test passes it, and so does fused-versus-staged,
    which compares two paths that read the same dims.
  * D.mask ignored in k_march_bwd_scan (sample_point in place of sample_valid, both passes): the blender rows fail --
    training form and deterministic mode with density-plane ratios of 4.3e6 - 3.4e7 and 576 - 7 840 stray writes per
    plane, pose-only with stored derivatives at 2.8e14 (the never-written dfeat_dn of dropped samples), regathering at
    4.3e-4 against RAY_ATOL 1e-6.  The llff rows pass it, and that is arithmetic, not a missing row: a dropped sample's
    stored feature is 0, the ReLU scene's density there is relu(0) = 0 with slope 0, so the backward's second decision
    cannot move anything; softplus(0 - 10) is positive, which is why both kinds run.
"""
import pytest
import torch

from tests import mask_ref as M
from tests import pinned_ref as P
from tests.test_gpu_pose_paths import APP_GAIN, FWD_GRAD, FWD_PLAIN, NOT_POSE, SCAN0, SCAN1, SCAN2, _check_pose
from tests.test_gpu_scatter_shapes import _check_row

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID = M.SCENE_GRID
S = 2 * (GRID[2] - 1) + 9     # 151
AABB = P.thin_box(GRID)


def _masked_scene(kind, vol, mask_aabb, app_gain=1.0):
    from joint_tensorf_amd.tensorf_repr import AlphaGridMask
    assert torch.equal(torch.tensor(AABB).view(2, 3), M.scene_box())
    tf = P.build_scene(kind, GRID, AABB, DEV)
    if app_gain != 1.0:
        with torch.no_grad():
            for p in list(tf.app_plane) + list(tf.app_line):
                p.mul_(app_gain)
    if vol is not None:
        tf.alphaMask = AlphaGridMask(DEV, mask_aabb, vol)
        # what the kernels are handed is what the reference computes from the box
        a = mask_aabb.float()
        assert torch.equal(tf.alphaMask.invgridSize.cpu(), 1.0 / (a[1] - a[0]) * 2)
        assert tf.alphaMask.gridSize.tolist() == [vol.shape[2], vol.shape[1], vol.shape[0]]
    return tf


# ---- 1. k_dense_alpha as the direct probe of mask_keep ------------------------------------------------------------------------
_PROBE = {}


def _probe(box):
    """the scene, the points of `box` and the unmasked run, computed once and left unchanged"""
    if box not in _PROBE:
        dims, maabb = M.mask_box(box)
        xyz = M.probe_points(dims, maabb)
        tf = _masked_scene("blender", None, None)
        a0 = tf.compute_alpha(xyz.to(DEV), 1.0).cpu()
        lo, hi = M.scene_box()
        in_scene = ((xyz >= lo) & (xyz <= hi)).all(1)
        assert int(in_scene.sum()) >= 2000      # (the scene is a small part of the post-shrink box: 3 226 of its points)
        assert float(a0[in_scene].min()) > 1e-3, float(a0[in_scene].min())
        assert bool((a0 > 0).all())      # softplus: a positive density beyond the scene box as well
        _PROBE[box] = (tf, dims, maabb, xyz, a0)
    return _PROBE[box]


@pytest.mark.parametrize("kind", ["single", "full-but-one", "random"])
@pytest.mark.parametrize("box", ["same", "shrunk"])
def test_dense_alpha_probe(box, kind):
    tf, dims, maabb, xyz, a0 = _probe(box)
    counts = M.family_counts(dims, maabb, xyz)
    for k in M.FAMILIES:
        assert counts[k] >= M.FLOORS[box][k], (box, k, counts)
    vol = M.volume(kind, dims)
    keep = M.keep(vol, maabb, xyz)
    from joint_tensorf_amd.tensorf_repr import AlphaGridMask
    tf.alphaMask = AlphaGridMask(DEV, maabb, vol)
    try:
        a1 = tf.compute_alpha(xyz.to(DEV), 1.0).cpu()
    finally:
        tf.alphaMask = None
    got = a1 > 0
    too_much, too_little = int((got & ~keep).sum()), int((~got & keep).sum())
    print("\n[mask] probe %s/%s: %d points, reference keeps %d; kernel keeps %d the reference drops, drops %d it keeps; %s"
          % (box, kind, xyz.shape[0], int(keep.sum()), too_much, too_little, counts))
    if too_much or too_little:
        fl, f = M.cells(vol.shape, maabb, xyz)
        bad = (got != keep).nonzero()[:6, 0]
        raise AssertionError((box, kind, too_much, too_little,
                              [(xyz[i].tolist(), fl[i].tolist(), f[i].tolist(), bool(keep[i])) for i in bad.tolist()]))
    assert torch.equal(a1[keep], a0[keep])          # the same kernel, the same arithmetic: bit for bit
    assert float(a1[~keep].abs().max()) == 0.0 if bool((~keep).any()) else True
    if kind == "full-but-one":                       # "any corner", not "all"
        fl, f = M.cells(vol.shape, maabb, xyz)
        inside = ((fl >= 0) & (fl < torch.tensor(dims) - 1)).all(1)
        lost = inside & ~got
        assert bool((f[lost] == 0).all()) and int(lost.sum()) <= 20    # only points ON the cleared voxel's node


# ---- 2. the masked march -----------------------------------------------------------------------------------------------------
_CENSUS = {}


def _march_inputs():
    if not _CENSUS:
        dims, maabb = M.mask_box("shrunk")
        vol = M.march_volume()
        o, d = M.march_rays()
        valid, kept, c = M.march_census(vol, maabb, o, d, S)
        assert c["dropped"] >= 0.2 * c["in_box"] and c["kept"] >= 0.2 * c["in_box"], c
        assert c["all_dropped"] >= 4 and c["gap_rays"] >= 8 and c["kept_far"] >= 1, c
        _CENSUS.update(vol=vol, maabb=maabb, o=o, d=d, valid=valid, kept=kept, counts=c)
    return _CENSUS


def _after(tag, hip, ref, pose):
    """what every masked row adds to its checker's bounds"""
    c = _march_inputs()
    valid, kept = c["valid"], c["kept"]
    print("   [mask] %s: %s" % (tag, c["counts"]))
    # no dropped sample was shaded
    assert not bool((hip["shade_mask"].cpu() & ~kept).any()), tag
    # rays that cross the box with every sample dropped: the background, and exactly zero gradients on both sides
    dead = valid.any(1) & ~kept.any(1)
    assert int(dead.sum()) >= 4
    for side in (hip, ref):
        assert float((side["rgb"].cpu()[dead].double() - 1.0).abs().max()) == 0.0, tag     # white background
        assert float(side["opacity"].cpu()[dead].abs().max()) == 0.0, tag
        assert float(side["g_o"].cpu()[dead].abs().max()) == 0.0 and float(side["g_d"].cpu()[dead].abs().max()) == 0.0, tag
    # and the mask matters: rays with kept samples have content
    assert float(ref["opacity"][kept.any(1)].max()) > 0.05


@pytest.mark.parametrize("row", ["blender", "llff", "blender-det"])
def test_masked_training_row(row):
    kind, det = row.split("-")[0], row.endswith("-det")
    c = _march_inputs()
    tf = _masked_scene(kind, c["vol"], c["maabb"])
    hip, ref = _check_row("mask-train-" + row, kind, GRID, AABB, c["o"], c["d"], S, det=det, expect=[SCAN0], long_line=False,
                          tf=tf)
    _after(row, hip, ref, False)
    # the footprint of the density factors is that of the kept samples: the reference's F is strictly smaller than
    # the unmasked one would be (x <= 4 mask cells holds no kept sample: the low-x texels of the line along x)
    assert not bool(ref["F"]["density_line.2"].all())


@pytest.mark.parametrize("stored", [True, False], ids=["stored", "regather"])
@pytest.mark.parametrize("kind", ["blender", "llff"])
def test_masked_pose_row(kind, stored):
    from joint_tensorf_amd import ops
    c = _march_inputs()
    tf = _masked_scene(kind, c["vol"], c["maabb"], app_gain=APP_GAIN)
    expect = [FWD_GRAD, SCAN2] if stored else [FWD_PLAIN, SCAN1]
    absent = NOT_POSE + ((SCAN1, SCAN0) if stored else (FWD_GRAD, SCAN2, SCAN0))
    keep = ops.POSE_MARCH_DERIVATIVES
    try:
        ops.POSE_MARCH_DERIVATIVES = stored
        hip, ref, _ = _check_pose("mask-pose-%s-%s" % (kind, "stored" if stored else "regather"), kind, GRID, AABB, c["o"],
                                  c["d"], S, expect=expect, absent=absent, tf=tf)
    finally:
        ops.POSE_MARCH_DERIVATIVES = keep
    _after("%s-%s" % (kind, stored), hip, ref, True)
    assert float(ref["g_o"].abs().max()) > 0.0


# ---- 3. the march's own outputs, and the blur ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blender", "llff"])
def test_march_forward_direct(kind):
    """jt_march_forward with the mask: sigma_feat is non-zero exactly at the kept samples (positive density factors) and
    exactly zero at the dropped ones; the shade list holds kept samples only, in ascending order"""
    from joint_tensorf_amd import ops
    from joint_tensorf_amd._lib import check, lib, ptr
    c = _march_inputs()
    tf = _masked_scene(kind, c["vol"], c["maabb"])
    o, d = c["o"].to(DEV).contiguous(), c["d"].to(DEV).contiguous()
    R = o.shape[0]
    rc = tf._render_cfg(S, False, True)
    assert rc.alpha_mask is not None
    scene = rc.scene()
    assert list(scene.mask_dims) == list(M.DIMS_SHRUNK)
    fac = ops._factors_struct([ops.factor_storage(p) for p in tf.density_plane], [ops.factor_storage(p) for p in tf.density_line],
                              [ops.factor_storage(p) for p in tf.app_plane], [ops.factor_storage(p) for p in tf.app_line],
                              rc.alpha_mask[0])
    f32 = dict(device=DEV, dtype=torch.float32)
    sf, w, tmin = torch.empty(R, S, **f32), torch.empty(R, S, **f32), torch.empty(R, **f32)
    cnt = torch.empty(R, device=DEV, dtype=torch.int32)
    off = torch.empty(R + 1, device=DEV, dtype=torch.int32)
    sidx = torch.empty(R, S, device=DEV, dtype=torch.int16)
    op, dep = torch.empty(R, **f32), torch.empty(R, **f32)
    check(lib.jt_march_forward(scene, fac, ptr(o), ptr(d), None, None, R, ptr(sf), ptr(w), ptr(tmin), ptr(cnt), ptr(off),
                               ptr(sidx), ptr(op), ptr(dep), None), "march")
    torch.cuda.synchronize()
    kept = c["kept"]
    sf, w, cnt, sidx = sf.cpu(), w.cpu(), cnt.cpu().long(), sidx.cpu().to(torch.int32) & 0xFFFF
    assert float(sf[~kept].abs().max()) == 0.0
    assert bool((sf[kept] != 0).all())
    assert float(w[~kept].abs().max()) == 0.0
    assert int(cnt.sum()) > 1000 and int(off[R]) == int(cnt.sum())
    for r in range(R):
        lst = sidx[r, :int(cnt[r])].long()
        assert bool(kept[r, lst].all()), r
        assert bool((lst[1:] > lst[:-1]).all()), r
        assert bool((w[r, lst] > 0).all()), r


def test_blur_ignores_mask():
    """with a blur active the mask is not consulted (batBase.py:76-82): the masked scene renders what the unmasked one does"""
    c = _march_inputs()
    tf = _masked_scene("blender", c["vol"], c["maabb"])
    mask = tf.alphaMask
    cr, co = P.cotangents(c["o"].shape[0], 3)
    got = {}
    with P.deterministic(True):      # order-independent gradient sums: two runs agree to the bit
        for name, m in (("masked", mask), ("plain", None), ("sharp", mask)):
            tf.alphaMask = m
            for p in tf.parameters():
                p.grad = None
            og, dg = c["o"].to(DEV).requires_grad_(True), c["d"].to(DEV).requires_grad_(True)
            blur = name != "sharp"
            out = tf(None, og, dg, white_bg=True, is_train=False, ndc_ray=False, N_samples=S,
                     c2f_parameter_density=0.1 if blur else None, c2f_parameter_color=0.1 if blur else None,
                     c2f_mode="uniform-gaussian" if blur else None, c2f_kernel_size=16 if blur else None)
            assert (tf.last_render_cfg.alpha_mask is None) == blur
            ((out[0] * cr.to(DEV).float()).sum() + (out[2] * co.to(DEV).float()).sum()).backward()
            torch.cuda.synchronize()
            got[name] = [t.detach().clone() for t in out] + [og.grad.clone(), dg.grad.clone()] + \
                        [p.grad.clone() for p in tf.parameters() if p.grad is not None]
    assert len(got["masked"]) == len(got["plain"]) > 10
    for a, b in zip(got["masked"], got["plain"]):
        assert torch.equal(a, b)
    # (and the mask does act once the blur is off: the all-dropped rays lose their content)
    dead = c["valid"].any(1) & ~c["kept"].any(1)
    assert float(got["sharp"][2].cpu()[dead].abs().max()) == 0.0 and float(got["masked"][2].cpu()[dead].max()) > 0.0
