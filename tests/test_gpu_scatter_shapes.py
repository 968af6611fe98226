"""Every LDS-budget branch of the two shape-dependent backward launchers, and the density backward scan at its 64-sample
chunk edges, held element by element to a pinned fp64 reference (tests/pinned_ref.py).

The appearance scatter (launch_shade_bwd, jt_shade.hip) and the density walk (jt_march_backward, jt_march.hip) pick
their kernel from the scene's longest line; the rest of the suite only reaches the branches its grids land on.  Each row
here is a thin scene -- the long axis (z) has L texels, the other two 9-12 -- placed at the last length that fits a
budget and the first that does not, with a bundle of rays along the long axis (entering through the end face), oblique
rays and grazing rays.  Each row asserts that its expected instantiation ran (torch.profiler, device kernel names) and
judges every factor gradient element: zero outside the reference footprint F, and |G - T| <= kappa 2^-24 M inside; and
every element of the ray gradients, which the density walk and the appearance chain write per ray.

Budget arithmetic (bytes; 160 KB = 163 840), ScatCfg<C> of jt_shade.hip, kRecWords = 20:
  scatter_lds(run, fl, sw) = 4 (BT + (fl & 1) L Ca + RED + sw (4 run (4 + 4 + 20) + 512))    (dBasis in the scatter)
  VM-48 (Ca 48, BT 1 344, RED 1 536): twelve waves, runs of 8, LDS line: 79 104 + 192 L <= 163 840  <=>  L <= 441;
      past it split 16 with eight waves, whose LDS line needs 85 248 + 192 L <= 163 840  <=>  L <= 409 -- so at L >= 442
      the default takes the global-atomic line path <.., false, 16, 8, 2>; with split 16 forced (no twelve-wave shape)
      the LDS line holds up to L = 409 and L = 410 is the global-atomic path.
  20 channels (Ca 20, BT 640, RED 640): sixteen waves while 152 576 + 80 L <= 163 840 (L <= 140), eight waves with
      the LDS line while 78 848 + 80 L <= 163 840 (L <= 1 062), the global-atomic path from L = 1 063.
  deterministic mode: no LDS line (FLAGS 2, DET true); the 20-channel scene keeps sixteen waves (152 576 <= 163 840).
Walk (jt_march.hip, shape()): records w x 5 376 bytes (8 waves 43 008, 16 waves 86 016), the line L Cd x 4 x lm bytes
(lm 2 doubles, 1 floats), the prefix table 4 n bytes when n <= 16 384 and it fits 158 KB = 161 792; eight waves only
when two workgroups fit (2 (b + 256) <= 163 840, b <= 81 664).  Cd 16, n = 1 000 (prefix 4 000 bytes):
  doubles 8w  47 008 + 128 L <= 81 664   <=> L <= 270     doubles 16w 90 016 + 128 L <= 161 792 <=> L <= 560
  floats 16w  90 016 +  64 L <= 161 792  <=> L <= 1 121   (floats 8w: 47 008 + 64 L <= 81 664 <=> L <= 541, never first)
  floats 16w without the prefix table: 86 016 + 64 L <= 161 792 <=> L <= 1 184;  then no LDS line, 8 waves.
  The prefix table is a runtime argument, not part of the kernel's name: rows 1 122 and 1 184 rest on this arithmetic
  (and on jt_march_backward_plan's prefix field, which tests/test_launch_plan.py holds to the row ids without a GPU).
  At L = 24: 16 384 rays keep the table (doubles, 16 waves: 86 016 + 3 072 + 65 536 <= 161 792); 16 385 rays have none
  and take doubles at eight waves (2 (46 080 + 256) <= 163 840).
  Cd 8: L = 24 doubles 8w; L = 1 185 floats 16w (doubles 16w: 86 016 + 75 840 > 161 792; floats 8w: 2 x 85 184 > 163 840).
Scan (k_march_bwd_scan): 4 waves x (2 Spad + Spad / 64) floats <= 163 840 bytes  <=>  Spad <= 5 056."""
import pytest
import torch

from tests import pinned_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"

# kappa per factor kind (|G - T| <= kappa 2^-24 M), ~4x the worst measured on MI355X.  All are above 2^12, and that is
# a finding, not a tolerance the kernels were fitted to: M is built from the exact upstream gradient |U| of each
# contribution, but the fp32 U of the product path carries the rounding of the sums that form it -- the compositing
# chain (dL/dalpha = G T - suffix / (1 - alpha)) for the density factors, basis^T GF over the app_dim rows and the MLP
# backward for the appearance factors -- relative to the magnitudes of their terms, not to |U|.  A texel reached only by
# samples whose U cancelled shows it.  Worst measured: density lines 596 and planes 1 291 (S = 5 056, where each long-line
# texel also sums thousands of contributions in fp32), appearance lines 1 971, appearance planes 29 133 (walk-L270,
# app_plane.1, a handful of texels; 300 - 900 on most rows).
# A lost, doubled or misplaced whole contribution is 2^24 x its share of M (the scatter built without the global-atomic
# line path's last flush fails vm48-L442 at 1.4e7 - 1.6e7 on every app line).
KAPPA = {"density_line": 2400.0, "density_plane": 5200.0, "app_line": 8000.0, "app_plane": 120000.0}
RAY_RTOL, RAY_ATOL = 1e-3, 1e-6   # ray gradients, element by element: |d| <= rtol |t| + atol max |t| (measured: every
                                  # element within 1e-3 |t| + 1e-9 max |t|)
DENSE_TOL = 5e-5                  # basis / MLP weight gradients: max |G - T| <= tol max |T| (measured: 7.9e-6)
TOL_VAL, TOL_DEPTH = 3e-5, 2e-4   # rgb / opacity, depth (test_gpu_fuzz.py)

SC48 = "k_shade_scatter<jt::ShadeCfg<48, 27, 64, 0>, "
SC20 = "k_shade_scatter<jt::ShadeCfg<20, 20, 32, 1>, "
WALK = "k_march_bwd_walk<"
SCAN = "k_march_bwd_scan<0>"

# id: (kind, L, Cd, rays (axial, oblique, grazing, missing), kernel variant, deterministic, ndc, expected kernel names)
APP = (32, 96, 32, 0)
WALK_RAYS = (24, 200, 32, 744)                          # n = 1 000 (the misses cost the reference nothing)
ROWS = {
    "vm48-L441": ("blender", 441, 16, APP, "mfma", False, False, [SC48 + "false, 8, 12, 3>"]),
    "vm48-L442": ("blender", 442, 16, APP, "mfma", False, False, [SC48 + "false, 16, 8, 2>"]),
    "vm48-split16-L409": ("blender", 409, 16, APP, "mfma-split16", False, False, [SC48 + "false, 16, 8, 3>"]),
    "vm48-split16-L410": ("blender", 410, 16, APP, "mfma-split16", False, False, [SC48 + "false, 16, 8, 2>"]),
    "c20-L140": ("llff", 140, 16, APP, "mfma", False, False, [SC20 + "false, 16, 16, 3>"]),
    "c20-L141": ("llff", 141, 16, APP, "mfma", False, False, [SC20 + "false, 16, 8, 3>"]),
    "c20-L1062": ("llff", 1062, 16, APP, "mfma", False, False, [SC20 + "false, 16, 8, 3>"]),
    "c20-L1063": ("llff", 1063, 16, APP, "mfma", False, False, [SC20 + "false, 16, 8, 2>"]),
    "c20-ndc-L1063": ("llff", 1063, 16, APP, "mfma", False, True, [SC20 + "false, 16, 8, 2>"]),
    "det-vm48-L442": ("blender", 442, 16, APP, "mfma", True, False, [SC48 + "true, 16, 8, 2>", WALK + "16, true, 0, 8>"]),
    "det-c20-L1063": ("llff", 1063, 16, APP, "mfma", True, False, [SC20 + "true, 16, 16, 2>", WALK + "16, true, 0, 8>"]),
    "walk-L270": ("llff", 270, 16, WALK_RAYS, "mfma", False, False, [WALK + "16, false, 2, 8>"]),
    "walk-L271": ("llff", 271, 16, WALK_RAYS, "mfma", False, False, [WALK + "16, false, 2, 16>"]),
    "walk-L560": ("llff", 560, 16, WALK_RAYS, "mfma", False, False, [WALK + "16, false, 2, 16>"]),
    "walk-L561": ("llff", 561, 16, WALK_RAYS, "mfma", False, False, [WALK + "16, false, 1, 16>"]),
    "walk-L1121": ("llff", 1121, 16, WALK_RAYS, "mfma", False, False, [WALK + "16, false, 1, 16>"]),
    "walk-L1122-noprefix": ("llff", 1122, 16, WALK_RAYS, "mfma", False, False, [WALK + "16, false, 1, 16>"]),
    "walk-L1184-noprefix": ("llff", 1184, 16, WALK_RAYS, "mfma", False, False, [WALK + "16, false, 1, 16>"]),
    "walk-L1185": ("llff", 1185, 16, WALK_RAYS, "mfma", False, False, [WALK + "16, false, 0, 8>"]),
    "walk-prefix-n16384": ("llff", 24, 16, (64, 1000, 64, 15256), "mfma", False, False, [WALK + "16, false, 2, 16>"]),
    "walk-noprefix-n16385": ("llff", 24, 16, (64, 1000, 64, 15257), "mfma", False, False, [WALK + "16, false, 2, 8>"]),
    "walk-cd8-L24": ("llff", 24, 8, WALK_RAYS, "mfma", False, False, [WALK + "8, false, 2, 8>"]),
    "walk-cd8-L1185": ("llff", 1185, 8, WALK_RAYS, "mfma", False, False, [WALK + "8, false, 1, 16>"]),
}
SHORT = (12, 9)   # the two short axes of a thin scene


def _ndc_setup(grid, rays, seed, n_far_side=0):
    """thin LLFF-style NDC box (z in [-1, 1] is the long axis) and rays from the z = -1 plane: a bundle along z (the
    first sample, t = near = 0, sits on the face), oblique rays, and rays grazing the long edges.  n_far_side: that many
    more rays along z (appended, from a generator of their own: the other rays do not move) with x = +hx or y = +hy
    (alternating) exactly -- every sample of such a ray is on that axis' far node; and the last sample (t = far = 1) of
    every ray along z lands on z = +1, the far node of the long axis."""
    hx, hy = 0.1, 0.08
    aabb = [-hx, -hy, -1.0, hx, hy, 1.0]
    g = torch.Generator().manual_seed(seed)
    na, no, ng = rays[:3]
    lo = torch.tensor([-hx, -hy])
    xy = [lo + 2 * torch.tensor([hx, hy]) * torch.rand(na + no, 2, generator=g)]
    e = torch.where(torch.rand(ng, 2, generator=g) < 0.5, -1.0, 1.0) * torch.tensor([hx, hy])
    xy.append(e + 0.005 * torch.randn(ng, 2, generator=g))
    xy = torch.cat(xy)
    o = torch.cat([xy, -torch.ones(na + no + ng, 1)], -1)
    dxy = torch.cat([torch.zeros(na, 2), 0.15 * torch.randn(no + ng, 2, generator=g)])
    d = torch.cat([dxy, 2.0 * torch.ones(na + no + ng, 1)], -1)
    if n_far_side:
        gf = torch.Generator().manual_seed(seed + 7919)
        xy = lo + 2 * torch.tensor([hx, hy]) * torch.rand(n_far_side, 2, generator=gf)
        xy[0::2, 0] = hx
        xy[1::2, 1] = hy
        o = torch.cat([o, torch.cat([xy, -torch.ones(n_far_side, 1)], -1)])
        d = torch.cat([d, torch.tensor([0.0, 0.0, 2.0]).expand(n_far_side, 3)])
    return aabb, o.float().contiguous(), d.float().contiguous()


def _check_row(tag, kind, grid, aabb, o, d, S, cd=16, variant="mfma", det=False, ndc=False, expect=(), near_far=(0.5, 40.0),
               long_line=True, tf=None):
    """tf: a prepared scene of `kind` on `grid` (tests/test_gpu_mask_edges.py hands one with an alpha mask set) instead of
    the one P.build_scene makes"""
    import time
    from joint_tensorf_amd._lib import lib
    from tests.test_gpu_parity import kernel_variant
    t0 = time.time()
    if tf is None:
        tf = P.build_scene(kind, grid, aabb, DEV, cd=cd, near_far=near_far)
    prev = lib.jt_set_deterministic(1 if det else 0)
    try:
        with kernel_variant(variant):
            hip = P.run_hip(tf, o, d, S, ndc=ndc, profile=True)
    finally:
        lib.jt_set_deterministic(prev)
    ref = P.run_reference(tf, kind, hip, o, d, S, ndc=ndc)
    seen = sorted(n for n in hip["kernels"] if any(k in n for k in ("k_shade_scatter", "k_march_bwd_walk", "k_march_bwd_scan")))
    print("\n[shapes] %s: grid %s, %d rays x %d samples, %d shaded; kernels%s: %s" % (
        tag, grid, o.shape[0], S, int(hip["shade_mask"].sum()),
        " (second profiled attempt: the first trace lacked this library's kernels)" if hip["profile_attempts"] > 1 else "",
        "; ".join(n.split("(")[0] for n in seen)))
    assert hip["kernels"], "the profiler reported no device kernels"
    for k in expect:
        assert any(k in n for n in seen), (tag, k, seen)
    # what the plan queries say this backward launches (tests/test_launch_plan.py checks them on the CPU) is what ran
    from tests.test_launch_plan import missing_from, planned_kernels
    shade, march, _, _ = planned_kernels(kind, grid, S, o.shape[0], cd=cd, variant=variant, det=det)
    planned = march + (shade if int(hip["shade_mask"].sum()) else [])
    assert not missing_from(planned, hip["kernels"]), (tag, planned, sorted(hip["kernels"]))
    rep = ref["relu"]
    assert rep.get("max_abs", 0.0) <= 2e-5, rep   # ReLU signs the fp64 reference decides differently: near-ties only
    for key, tol in (("rgb", TOL_VAL), ("opacity", TOL_VAL), ("depth", TOL_DEPTH)):
        err = float((hip[key].double().cpu() - ref[key]).abs().max())
        assert err <= tol, (tag, key, err)
    bad = []
    line = "   kappa:"
    for n in P.FACTORS:
        stray, ratio, at = P.factor_errors(hip["grads"][n].cpu(), ref["T"][n], ref["M"][n], ref["F"][n])
        fam = n.split(".")[0]
        line += " %s %.0f%s" % (n.replace("_plane", "P").replace("_line", "L").replace("density", "d").replace("app", "a"),
                                ratio, "" if not stray else " (%d STRAY)" % stray)
        if stray or not ratio <= KAPPA[fam]:
            bad.append((n, stray, ratio, at))
    print(line)
    dense = {n: P.max_rel(hip["grads"][n].cpu(), ref["T"][n]) for n in P.DENSE}
    # (the reference takes the product path's tap cells: a sample on a texel node has the same slope on both sides)
    rays = {k: P.ray_atol(hip[k].cpu(), ref[k], RAY_RTOL) for k in ("g_o", "g_d")}
    print("   dense max-rel: " + " ".join("%s %.1e" % kv for kv in dense.items()) +
          "   ray atol at rtol %.0e: %s   (%.1f s)" % (RAY_RTOL, " ".join("%s %.1e" % kv for kv in rays.items()),
                                                       time.time() - t0))
    if long_line:  # every texel of the long line (line 0: along z) is in the footprint
        assert ref["F"]["density_line.0"].all() and ref["F"]["app_line.0"].all(), tag
    assert not bad, (tag, bad)
    assert all(v <= DENSE_TOL for v in dense.values()), (tag, dense)
    assert all(v <= RAY_ATOL for v in rays.values()), (tag, rays)
    return hip, ref


@pytest.mark.parametrize("row", list(ROWS))
def test_branch_row(row):
    kind, L, cd, rays, variant, det, ndc, expect = ROWS[row]
    grid = [SHORT[0], SHORT[1], L]
    if ndc:
        aabb, o, d = _ndc_setup(grid, rays, seed=L)
        S, near_far = 2 * (L - 1) + 1, (0.0, 1.0)
    else:
        aabb = P.thin_box(grid)
        o, d = P.ray_set(aabb, *rays[:3], n_miss=rays[3], seed=L)
        S, near_far = 2 * (L - 1) + 9, (0.5, 40.0)
    assert o.shape[0] == sum(rays)
    _check_row(row, kind, grid, aabb, o, d, S, cd=cd, variant=variant, det=det, ndc=ndc, expect=expect, near_far=near_far)


# The backward scan handles a ray's samples 64 at a time and carries the transmittance across chunks through LDS: S at
# the chunk edges, on a scene whose long axis holds more than 129 samples of the axial bundle
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 127, 128, 129])
@pytest.mark.parametrize("kind", ["blender", "llff"])
def test_scan_chunk_edges(kind, S):
    grid = [11, 9, 72]
    aabb = P.thin_box(grid)
    o, d = P.ray_set(aabb, 8, 16, 4, seed=S)
    _check_row("scan-%s-S%d" % (kind, S), kind, grid, aabb, o, d, S, expect=[SCAN], long_line=False)


def test_scan_chunk_edge_ndc():
    grid = [11, 9, 72]
    aabb, o, d = _ndc_setup(grid, (8, 16, 4, 0), seed=3)
    _check_row("scan-ndc-S65", "llff", grid, aabb, o, d, 65, ndc=True, expect=[SCAN], near_far=(0.0, 1.0), long_line=False)


def test_scan_largest_s():
    """S = 5 056: the largest S whose per-wave arrays fit the scan's LDS (Spad = 5 056), on a few rays along a line of
    2 528 texels (every sample of the bundle in the box, the last one past the far face)"""
    grid = [8, 8, 2528]
    aabb = P.thin_box(grid)
    o, d = P.ray_set(aabb, 4, 2, 0, seed=5)
    hip, ref = _check_row("scan-S5056", "blender", grid, aabb, o, d, 5056, expect=[SCAN])
    assert int(hip["shade_mask"][:4].sum()) >= 4 * 5000
