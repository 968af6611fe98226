"""The pose-only backward -- a render in which only the rays want a gradient, what test-time pose optimisation runs -- held
to the pinned fp64 reference (tests/pinned_ref.py) on every kernel path it can take, element by element.

Such a render runs kernels the training step never uses: k_march_fwd<true> (the march that also stores d feature / d
coordinate), the appearance forward with its light record set, the chain k_shade_bwd<C, false, true[, true]> followed by
k_pose_gather<C, B16> in the scatter's place, and k_march_bwd_scan<2> (stored derivatives) or <1> (gathers again,
ops.POSE_MARCH_DERIVATIVES off); in deterministic mode the training-form kernels with their targets switched off.

Each row builds a thin scene (P.build_scene), runs one pose-only forward + backward under the profiler, runs the fp64
reference pinned to that run's own decisions (shading mask, ReLU words of the pose-only record set), asserts the kernels
it expects, and judges rgb / opacity / depth and every element of g_o and g_d with the bounds of
tests/test_gpu_scatter_shapes.py (imported, not restated): the pose path produces the training backward's ray gradients
and claims the same accuracy.  No parameter may receive a gradient, and no kernel may write past a buffer it was handed
(P.guard_band: 512 guard bytes behind every device buffer of the step; a partial last tile handled as a full one writes
up to 31 x 12 bytes past g_xyz, which nothing downstream ever reads).

The subject of most rows is k_pose_gather's choice, one ballot per wave and plane, between the nested interpolation
(every tap in range) and the masked form (grid_sample's zero padding), which a sample needs exactly when it sits on a far
node, floor(ix) == size - 1: at test time (no jitter) the first sample of every ray that enters through a `hi` face.  The
far-side / far-entry families of P.ray_set put samples there on purpose, and P.census counts, from the reference side
alone, the 32-entry tiles with and without such a sample, so that a row cannot pass by missing its subject.  Two facts
about the rows, both from the compositing, not from the kernels: the last sample of a ray has a zero interval, hence zero
weight, and is never shaded -- so an S = 1 row shades nothing (all gradients are exactly zero on both sides; it holds the
empty launch), S = 2 rows shade exactly the first sample (on far-entry rays: the far-node sample is the whole appearance
gradient), and in NDC the sample on z = +1 never reaches the gather (the far-side family does).

Measured on MI355X: all 55 rows green; the worst figures and the four deliberate breaks are recorded below the imports.
Wall time on MI355X, same session: this file 11 s (pytest 6.5 s, the grid-cap row 0.8 s of it);
tests/test_gpu_scatter_shapes.py 21 s (pytest 16.6 s)."""
import re
import time

import numpy as np
import pytest
import torch

from tests import pinned_ref as P
from tests.test_gpu_scatter_shapes import RAY_ATOL, RAY_RTOL, TOL_DEPTH, TOL_VAL, _ndc_setup

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Worst measured over the 55 rows (MI355X): every element of g_o and g_d within RAY_RTOL |t| + 8.9e-9 max |t| (c20-n31; most
# rows need no absolute term at all) against RAY_ATOL = 1e-6; rgb 2.4e-7, opacity 3.9e-7 (TOL_VAL 3e-5), depth 8.0e-7
# (TOL_DEPTH 2e-4); no ReLU word of the pose-only record set farther than 2e-5 from a tie; no guard byte touched.  The pose
# path keeps the training backward's bounds with room, so none is restated or widened here.
#
# What the rows catch -- the library rebuilt with one line broken (scratch builds, not part of the repository), whole file
# run against each; figures are the absolute term a row would need at RAY_RTOL, to be compared with 1e-6:
#   * `oor` forced to false in k_pose_gather (the nested form on far-node samples): 30 rows fail -- every mixed row, far-only
#     and S2 of all three instantiations (vm48 far-only 8.5e-4, vm48 S2 1.8e-3, c20 far-only 2.7e-2, c20 S2 1.8e-2), the
#     tile rows from 31 entries on (worst c20-n33 4.3e-2), chunks, grid cap, NDC; the interior-only rows stay green, as they
#     must.  Without APP_GAIN the vm48 far-only and mixed rows passed this break and vm48 S2 failed by 4e-6 only.
#   * the __shfl_xor(.., 32) sum of the lane halves dropped for the y axis: 48 rows fail, 7.8e-6 (march-blender-S2, a scene
#     without the gain) to 0.99 (c20-n1); the 7 that pass shade nothing or run no gather (S1 rows, deterministic mode).
#   * nlive replaced by 32: tile-n1 of both instantiations fails, on the guard band alone (359 bytes behind g_xyz [2, 3]
#     changed).  The dead lanes of a partial tile compute columns of their own and write entries past the shaded count,
#     which no consumer reads: no value moves, and the stray write only leaves g_xyz where 32 x tiles exceeds rays x
#     samples -- the one-entry row.  That is all a test can see of this break through the product path.
#   * the second and third planes of dfeat_dn swapped in k_march_bwd_scan<2>: 48 rows fail, 0.13 to 9.0 (the same 7 pass:
#     nothing shaded and no density gradient at S = 1, no stored derivatives in deterministic mode).

C48, C20 = "jt::ShadeCfg<48, 27, 64, 0>", "jt::ShadeCfg<20, 20, 32, 1>"
G48B, G48F, G20 = "k_pose_gather<%s, true>" % C48, "k_pose_gather<%s, false>" % C48, "k_pose_gather<%s, false>" % C20
CHAIN_B16 = "k_shade_bwd<%s, false, true, true>"      # the chain on the bf16 matrix cores (matrix-mode bit 2)
CHAIN_F32 = "k_shade_bwd<%s, false, true>"            # the fp32 chain (a trailing default `, false` is stripped: _names)
FWD_GRAD, FWD_PLAIN = "k_march_fwd<true>", "k_march_fwd<false>"
SCAN0, SCAN1, SCAN2 = "k_march_bwd_scan<0>", "k_march_bwd_scan<1>", "k_march_bwd_scan<2>"
NOT_POSE = ("k_shade_scatter", "k_march_bwd_walk")
OURS = ("k_pose_gather", "k_shade_bwd", "k_shade_scatter", "k_shade_fwd", "k_march_fwd", "k_march_bwd")

# id: (scene kind, kernel variant (tests/test_gpu_parity.py VARIANTS), gather instantiation, chain pattern)
GATHER = {
    "vm48-b16": ("blender", "mfma", G48B, CHAIN_B16 % C48),
    "vm48-fp32": ("blender", "mfma-split16-fp32chain", G48F, CHAIN_F32 % C48),   # matrix mode 3
    "c20": ("llff", "mfma", G20, CHAIN_B16 % C20),
}
GRID = [12, 9, 72]
S_FULL = 2 * (GRID[2] - 1) + 9    # 151: the 143 in-box samples of a ray along z, and past the far face
POSE_EXPECT = [FWD_GRAD, SCAN2]
# P.build_scene's appearance factors are 0.1 x randn: plane x line products of 0.01, and an appearance share of the ray
# gradient of a few thousandths -- the density path, whose factors are ~0.5, makes the rest.  Every row whose subject is
# the appearance gather (all but the density-side rows, which keep the scene as built) scales the appearance planes and
# lines by 10 (products x 100: basis outputs of order 1), so that the two paths weigh about the same and a wrong
# appearance slope is an O(1) error of the element, not a per-mille one.
APP_GAIN = 10.0


def _mixed(aabb, seed):
    """axial, oblique, grazing, far-side, far-entry rays and a few misses"""
    return P.ray_set(aabb, 8, 48, 16, n_miss=4, n_far_side=8, n_far_entry=8, seed=seed)


def _names(kernels):
    """this library's kernels among the profiled device kernels, without their argument lists; k_shade_bwd's defaulted
    last template argument is written out by some demanglers and not by others: `, true, false>` reads `, true>`"""
    out = set()
    for n in kernels:
        if any(k in n for k in OURS):
            n = n.split("(")[0]
            out.add(re.sub(r"(k_shade_bwd<.*, (?:true|false), true), false>$", r"\1>", n))
    return sorted(out)


def _ran(seen, what):
    return any(what in n for n in seen)


def _check_pose(tag, kind, grid, aabb, o, d, S, cd=16, variant="mfma", det=False, ndc=False, near_far=(0.5, 40.0),
                expect=(), absent=NOT_POSE, chunk=1 << 22, tf=None, app_gain=None):
    """one pose-only iteration against its pinned fp64 reference; returns (hip, ref, census).  app_gain scales the
    appearance planes and lines of the scene (None: APP_GAIN)"""
    from joint_tensorf_amd._lib import lib
    from tests.test_gpu_parity import kernel_variant
    t0 = time.time()
    if tf is None:
        tf = P.build_scene(kind, grid, aabb, DEV, cd=cd, near_far=near_far)
        if (APP_GAIN if app_gain is None else app_gain) != 1.0:
            with torch.no_grad():
                for p in list(tf.app_plane) + list(tf.app_line):
                    p.mul_(APP_GAIN if app_gain is None else app_gain)
    prev = lib.jt_set_deterministic(1 if det else 0)
    try:
        with kernel_variant(variant):
            hip = P.run_hip(tf, o, d, S, ndc=ndc, profile=True, pose_only=True)
    finally:
        lib.jt_set_deterministic(prev)
    t1 = time.time()
    ref = P.run_reference(tf, kind, hip, o, d, S, ndc=ndc, ray_only=True)
    _, far = P.far_node_samples(aabb, grid, near_far, o, d, S, ndc=ndc, device=DEV)
    cen = P.census(far, hip["shade_mask"], chunk)
    seen = _names(hip["kernels"])
    rays = {k: P.ray_atol(hip[k].cpu(), ref[k], RAY_RTOL) for k in ("g_o", "g_d")}
    vals = {k: float((hip[k].double().cpu() - ref[k]).abs().max()) for k in ("rgb", "opacity", "depth")}
    print("\n[pose] %s: grid %s, %d rays x %d samples, %d shaded; tiles per chunk %s: %d with a far-node sample, %d without "
          "(%d far-node entries)%s" % (tag, grid, o.shape[0], S, cen["shaded"], cen["tiles"], cen["far_tiles"],
                                      cen["plain_tiles"], cen["far_entries"],
                                      "; second profiled attempt" if hip["profile_attempts"] > 1 else ""))
    print("   kernels: " + "; ".join(seen))
    print("   ray atol at rtol %.0e: %s   max |g|: g_o %.2e g_d %.2e   values: %s   (%.1f s, %.1f s of it the HIP side)" % (
        RAY_RTOL, " ".join("%s %.1e" % kv for kv in rays.items()), float(ref["g_o"].abs().max()),
        float(ref["g_d"].abs().max()), " ".join("%s %.1e" % kv for kv in vals.items()), time.time() - t0, t1 - t0))
    assert hip["kernels"], "the profiler reported no device kernels"
    assert cen["shaded"] == int(hip["shade_mask"].sum())
    for k in expect:
        assert _ran(seen, k), (tag, "expected", k, seen)
    for k in absent:
        assert not _ran(seen, k), (tag, "unexpected", k, seen)
    # what the plan queries say this backward launches (tests/test_launch_plan.py checks them on the CPU) is what ran
    # (the appearance kernels are only required where a sample was shaded)
    from joint_tensorf_amd import ops
    from tests.test_launch_plan import missing_from, planned_kernels
    shade, march, _, _ = planned_kernels(kind, grid, S, o.shape[0], cd=cd, variant=variant, det=det, pose=True,
                                         stored=ops.POSE_MARCH_DERIVATIVES)
    planned = march + (shade if cen["shaded"] else [])
    assert not missing_from(planned, hip["kernels"]), (tag, planned, seen)
    assert hip["grads"] is None and hip["param_grads"] == 0, (tag, "a parameter received a gradient")
    assert not hip["overruns"], (tag, "a kernel wrote past its buffer (shape, bytes changed)", hip["overruns"])
    assert ref["relu"].get("max_abs", 0.0) <= 2e-5, ref["relu"]   # ReLU signs decided differently: near-ties only
    for key, tol in (("rgb", TOL_VAL), ("opacity", TOL_VAL), ("depth", TOL_DEPTH)):
        assert vals[key] <= tol, (tag, key, vals[key])
    assert torch.isfinite(hip["g_o"]).all() and torch.isfinite(hip["g_d"]).all(), tag
    if not all(v <= RAY_ATOL for v in rays.values()):
        # which rays, which axis: the worst elements (ray index, axis, got, reference)
        worst = []
        for k in ("g_o", "g_d"):
            dlt = ((hip[k].double().cpu() - ref[k]).abs() - RAY_RTOL * ref[k].abs()).flatten()
            for i in dlt.topk(min(6, dlt.numel())).indices.tolist():
                worst.append((k, i // 3, i % 3, float(hip[k].flatten()[i]), float(ref[k].flatten()[i])))
        raise AssertionError((tag, rays, worst))
    return hip, ref, cen


# ---- the three gather instantiations on the mixed ray set ---------------------------------------------------------------------
@pytest.mark.parametrize("row", list(GATHER) + ["vm48-fp32-mode0"])
def test_gather_mixed(row):
    """vm48-fp32-mode0: the fp32 matrix-core kernels throughout (matrix mode 0, `mfma-fp32`): the same gather and chain
    as vm48-fp32 behind the fp32 forward"""
    kind, variant, gather, chain = GATHER["vm48-fp32"] if row == "vm48-fp32-mode0" else GATHER[row]
    if row == "vm48-fp32-mode0":
        variant = "mfma-fp32"
    aabb = P.thin_box(GRID)
    o, d = _mixed(aabb, seed=7)
    _, _, cen = _check_pose(row + "-mixed", kind, GRID, aabb, o, d, S_FULL, variant=variant,
                            expect=[gather, chain] + POSE_EXPECT)
    assert cen["far_tiles"] >= 8 and cen["plain_tiles"] >= 8, cen


# ---- far-node rows --------------------------------------------------------------------------------------------------------
def _far_rays(aabb, which):
    if which == "far-only":     # 23 shaded samples per ray: every tile of 32 entries holds a ray's first sample or a far-side ray
        return P.ray_set(aabb, 0, 0, 0, n_far_side=16, n_far_entry=16, seed=11) + (24,)
    if which == "interior-only":
        # the bundle stops short of the far face (S = 100); of the oblique and grazing rays, those that enter through a `hi`
        # face have their first sample on it: only rays without any far-node sample stay (decided on the reference side)
        o, d = P.ray_set(aabb, 24, 48, 16, seed=12)
        _, far = P.far_node_samples(aabb, GRID, (0.5, 40.0), o, d, 100, device=DEV)
        keep = ~far.any(-1).any(-1)
        assert int(keep.sum()) >= 40
        return o[keep].contiguous(), d[keep].contiguous(), 100
    return P.ray_set(aabb, 0, 0, 0, n_far_entry=40, seed=13) + (int(which[1:]),)


@pytest.mark.parametrize("which", ["far-only", "interior-only", "S1", "S2"])
@pytest.mark.parametrize("row", list(GATHER))
def test_far_node(row, which):
    kind, variant, gather, chain = GATHER[row]
    aabb = P.thin_box(GRID)
    o, d, S = _far_rays(aabb, which)
    expect = ([gather, chain] if which != "S1" else []) + POSE_EXPECT
    hip, ref, cen = _check_pose("%s-%s" % (row, which), kind, GRID, aabb, o, d, S, variant=variant, expect=expect)
    if which == "far-only":
        assert cen["plain_tiles"] == 0 and cen["far_tiles"] >= 8, cen
    elif which == "interior-only":
        assert cen["far_tiles"] == 0 and cen["plain_tiles"] >= 8, cen
    elif which == "S1":   # the only sample is the last one: zero interval, zero weight, nothing shaded, no gradient at all
        assert cen["shaded"] == 0 and float(ref["g_o"].abs().max()) == 0.0 and float(hip["g_o"].abs().max()) == 0.0
    else:                 # the first sample of every ray, on the far node of z, and nothing else
        assert cen["shaded"] == 40 and cen["far_entries"] == 40, cen
        assert float(ref["g_o"].abs().max()) > 0.0


# ---- tile and grid arithmetic of k_pose_gather ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 1001])
@pytest.mark.parametrize("row", ["vm48-b16", "c20"])
def test_tile_arithmetic(row, n):
    """n shaded entries exactly: with S = 2 every ray that crosses the box shades its first sample and nothing else (n
    rays, a quarter of them far-entry rays); 1 001 = 7 rays along z x 143 in-box samples (window 960 .. 1 040)"""
    kind, variant, gather, chain = GATHER[row]
    aabb = P.thin_box(GRID)
    if n == 1001:
        o, d = P.ray_set(aabb, 4, 0, 0, n_far_side=2, n_far_entry=1, seed=n)
        S = S_FULL
    else:
        o, d = P.ray_set(aabb, n - n // 4, 0, 0, n_far_entry=n // 4, seed=n)
        S = 2
    _, _, cen = _check_pose("%s-n%d" % (row, n), kind, GRID, aabb, o, d, S, variant=variant,
                            expect=[gather, chain] + POSE_EXPECT)
    if n == 1001:
        assert 960 <= cen["shaded"] <= 1040, cen
    else:
        assert cen["shaded"] == n, cen
    assert cen["tiles"] == [(cen["shaded"] + 31) // 32]


def _many_rays(aabb, n):
    return P.ray_set(aabb, n - n // 5, 0, 0, n_far_side=n // 10, n_far_entry=n // 10, seed=n)


def test_several_chunks():
    """backward chunks of 2^16 entries: a full chunk, a second one and a partial third (chunk_start, the chunks' record blocks)"""
    from joint_tensorf_amd._lib import lib
    kind, variant, gather, chain = GATHER["c20"]
    aabb = P.thin_box(GRID)
    o, d = _many_rays(aabb, 1000)     # 1 000 rays x 143 in-box samples
    prev = lib.jt_shade_set_chunk_log2(16)
    try:
        assert lib.jt_shade_chunk_entries() == 1 << 16
        _, _, cen = _check_pose("c20-chunks", kind, GRID, aabb, o, d, S_FULL, variant=variant, chunk=1 << 16,
                                expect=[gather, chain] + POSE_EXPECT)
    finally:
        lib.jt_shade_set_chunk_log2(prev)
    assert cen["shaded"] > 2 * 65536 and cen["shaded"] < 3 * 65536, cen
    assert cen["tiles"][:2] == [2048, 2048] and len(cen["tiles"]) == 3 and 0 < cen["tiles"][2] < 2048, cen
    assert cen["far_tiles"] >= 8 and cen["plain_tiles"] >= 8, cen


def test_grid_cap():
    """more than 2 048 workgroups x 4 waves x 32 entries in one chunk: the tile loop of k_pose_gather takes a second trip"""
    from joint_tensorf_amd._lib import lib
    kind, variant, gather, chain = GATHER["c20"]
    aabb = P.thin_box(GRID)
    o, d = _many_rays(aabb, 2000)     # 2 000 rays x 143 in-box samples
    assert lib.jt_shade_chunk_entries() == 1 << 22
    _, _, cen = _check_pose("c20-gridcap", kind, GRID, aabb, o, d, S_FULL, variant=variant,
                            expect=[gather, chain] + POSE_EXPECT)
    assert cen["shaded"] > 262144 and len(cen["tiles"]) == 1, cen
    assert cen["far_tiles"] >= 8 and cen["plain_tiles"] >= 8, cen


# ---- density side: k_march_fwd<true> and k_march_bwd_scan<1 | 2> at the 64-sample chunk edges --------------------------------
def _density_row(tag, kind, S, cd):
    from joint_tensorf_amd import ops
    grid = [11, 9, 72]
    aabb = P.thin_box(grid)
    o, d = P.ray_set(aabb, 8, 16, 4, seed=S, n_far_side=4, n_far_entry=4)
    gather = GATHER["vm48-b16" if kind == "blender" else "c20"][2]
    tf = P.build_scene(kind, grid, aabb, DEV, cd=cd)     # (as built: no appearance gain, the density path dominates)
    keep = ops.POSE_MARCH_DERIVATIVES
    got = {}
    try:
        for stored in (True, False):
            ops.POSE_MARCH_DERIVATIVES = stored
            expect = [FWD_GRAD, SCAN2] if stored else [FWD_PLAIN, SCAN1]
            absent = NOT_POSE + ((SCAN1, SCAN0) if stored else (FWD_GRAD, SCAN2, SCAN0))
            if S > 1:
                expect = expect + [gather]
            hip, _, _ = _check_pose("%s-%s" % (tag, "stored" if stored else "regather"), kind, grid, aabb, o, d, S, cd=cd,
                                    expect=expect, absent=absent, tf=tf)
            got[stored] = hip
    finally:
        ops.POSE_MARCH_DERIVATIVES = keep
    for k in ("g_o", "g_d"):   # the two settings against each other: the bound of tests/test_gpu_edge.py
        a, b = got[True][k].cpu().numpy(), got[False][k].cpu().numpy()
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6 * float(np.abs(b).max()), err_msg="%s %s" % (tag, k))


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 127, 128, 129])
@pytest.mark.parametrize("kind", ["blender", "llff"])
def test_density_side_chunk_edges(kind, S):
    _density_row("march-%s-S%d" % (kind, S), kind, S, 16)


@pytest.mark.parametrize("kind", ["blender", "llff"])
def test_density_side_cd8(kind):
    _density_row("march-%s-cd8-S129" % kind, kind, 129, 8)


# ---- NDC rays -----------------------------------------------------------------------------------------------------------------
def test_c20_ndc():
    kind, variant, gather, chain = GATHER["c20"]
    S = 2 * (GRID[2] - 1) + 1
    aabb, o, d = _ndc_setup(GRID, (8, 16, 4, 0), seed=5, n_far_side=8)
    _, _, cen = _check_pose("c20-ndc", kind, GRID, aabb, o, d, S, variant=variant, ndc=True, near_far=(0.0, 1.0),
                            expect=[gather, chain] + POSE_EXPECT)
    assert cen["far_tiles"] >= 8 and cen["plain_tiles"] >= 8, cen


# ---- deterministic mode: the training-form kernels with their targets switched off ------------------------------------------
@pytest.mark.parametrize("row", ["vm48-b16", "c20"])
def test_deterministic(row):
    kind, variant, _, chain = GATHER[row]
    cfg = C48 if kind == "blender" else C20
    aabb = P.thin_box(GRID)
    o, d = _mixed(aabb, seed=9)
    expect = [chain, "k_shade_scatter<%s, true, " % cfg, "k_march_bwd_walk<16, true, ", FWD_PLAIN, SCAN0]
    runs = [_check_pose("det-%s-run%d" % (row, i), kind, GRID, aabb, o, d, S_FULL, variant=variant, det=True, expect=expect,
                        absent=("k_pose_gather", FWD_GRAD, SCAN1, SCAN2)) for i in range(2)]
    assert runs[0][2]["far_tiles"] >= 8 and runs[0][2]["plain_tiles"] >= 8
    for k in ("g_o", "g_d"):
        assert torch.equal(runs[0][0][k], runs[1][0][k]), (row, k, "two deterministic runs differ")
