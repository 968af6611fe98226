"""k_pose_fused (csrc/jt_fused.hip), the single-launch render + loss + backward-to-the-rays kernel of test-time pose
optimisation, held to the pinned fp64 reference (tests/pinned_ref.py) ray by ray, at the edges of its hand-made control
flow: the fill of a workgroup's eight ray slots, shaded counts at the 32-sample tile edges of the pooled tile list, S at
the 64-sample chunk and slot-carving edges, a second round over the same slots, rays of several views in one workgroup,
NDC rays, a black background, an alpha mask, the loss accumulator's protocol across launches of different grid sizes and
the sample count at which the kernel's LDS is full.  tests/test_gpu_fused.py compares the kernel with the staged path on
300 - 500 comfortable rays and judges the gradient summed into d loss / d se3; one wrong ray in hundreds moves that sum
by parts in 10^4.  Here every element of g_o and g_d is judged.

Every row runs one launch through ops.render_pose_fused on a freshly zeroed workspace (P.run_fused), reads the kernel's own
discrete decisions back from its scratch slots (the rank array and the ReLU sign words, P.decode_fused_scratch, laid out
by jt_pose_fused_scratch_layout) and runs the fp64 reference pinned to them, differentiating loss_scale * sum (clamp(rgb)
- target)^2.  Judged per row (judge): every element of g_o and g_d (RAY_RTOL |t| + RAY_ATOL max |t|), of rgb, opacity
(TOL_VAL) and depth (TOL_DEPTH) -- the bounds of tests/test_gpu_scatter_shapes.py, imported --, sqerr per ray within
2 TOL_VAL sum_c |rgb_c - target_c| + 3 TOL_VAL^2, the loss against loss_scale x the fp64 sum of the kernel's own sqerr
within n 2^-24 (n = rounds + 8 waves + workgroups additions of non-negative terms), no ReLU word farther than 2e-5 from
a tie, no guard byte touched, the two head words of the workspace zero after the launch, every word behind the last slot
the launch's workgroups own still zero, and the census the row is about, from the scratch and from the reference side.

Condition, asserted from the reference alone: every ray with shaded samples has its reference colour in [1e-5, 1 - 1e-5]
in all three channels, so the clamp's gate (v >= 0 && v <= 1 in the kernel, torch's closed-interval clamp in the
reference) is decided alike in fp32 and fp64.

The LDS limit.  launch_fused needs, per workgroup, C::LDS_FLOATS * 4 (the MLP in LDS) + 8 waves * 2 * 16 * 64 * 4 = 65 536
(sin / cos stashes) + 8 * Sp * 2 (shaded-sample lists, Sp = S rounded up to 64) + sizeof(FusedTabs) = 268 bytes, at most
160 KB = 163 840:
  blender (ShadeCfg<48, 27, 64>): LDS_FLOATS = 32*145 + 64*151 + 64*65 + 64*4 + 64 + 64 + 4 = 18 852 -> 75 408 bytes;
      16 Sp <= 163 840 - 75 408 - 65 536 - 268 = 22 628 -> Sp <= 1 414 -> Sp = 1 408 = 22 * 64: S_max = 1 408
  llff (ShadeCfg<20, 20, 32>):    LDS_FLOATS = 32*61 + 32*101 + 32*33 + 44*4 + 32 + 32 + 4 = 6 484 -> 25 936 bytes;
      16 Sp <= 163 840 - 25 936 - 65 536 - 268 = 72 100 -> Sp <= 4 506 -> Sp = 4 480 = 70 * 64: S_max = 4 480
(tests/test_host_logic.py::test_fused_probe_knows_the_lds_limit holds the probe to both sides of these without a GPU).

Measured on MI355X: all 46 rows green, this file 3.2 s of pytest wall time (the slowest row 1.1 s, the first: it loads the
libraries; no other above 0.4 s).  Worst over all rows: every element of g_o within RAY_RTOL |t| + 2.6e-8 max |t|, of g_d
within RAY_RTOL |t| + 1.6e-8 max |t| (RAY_ATOL = 1e-6; most rows need no absolute term at all); rgb 2.4e-7, opacity 3.6e-7
(TOL_VAL = 3e-5); depth 9.5e-7 (TOL_DEPTH = 2e-4); sqerr 0.0061 of its bound; loss 0.20 of n 2^-24; no ReLU sign of the
scratch differs from the fp64 reference's own (max_abs 0); no guard byte touched; head words and the workspace behind the
launch's slots zero in every row.  The imported bounds hold with room: none is restated or widened."""
import time

import pytest
import torch

from tests import mask_ref as M
from tests import pinned_ref as P
from tests.test_gpu_pose_paths import APP_GAIN, GRID, S_FULL
from tests.test_gpu_scatter_shapes import RAY_ATOL, RAY_RTOL, TOL_DEPTH, TOL_VAL, _ndc_setup
from tests.test_host_logic import FUSED_S_MAX

pytestmark = pytest.mark.gpu
DEV = "cuda"

# What the rows catch -- libjt_fused.so rebuilt with one line of k_pose_fused broken (scratch builds, not part of the
# repository; each break changes arithmetic or an index inside the ray's own slot, or which view's image is read -- no
# address leaves the workspace, the lattice or the images), the whole file run against each.  Figures: the absolute term a
# row would need at RAY_RTOL for (g_o, g_d), to be compared with 1e-6.
#   * the final sum's ntile one short (the last tile's position gradients are left out): 39 of 46 rows fail -- every row
#     that shades anything, 9.7e-4 (the masked row) to 0.13 (black-llff); only the two S = 1 rows, which shade nothing, and
#     the rows that judge no launch pass.  The smallest failures are a thousand times the bound; in d loss / d se3 of
#     tests/test_gpu_fused.py a single such ray would be parts in 10^4.
#   * the chunk partial rows addressed with S / 32 instead of Sp / 32 (the D1 sums land in rows D2 overwrites): 27 rows
#     fail, 0.16 to 1.1 -- every row with S = 151 but the masked one, S = 2 and S = 63 (one chunk row, at tile row 0 / 1),
#     the second round (S = 16); the rows where S / 32 == Sp / 32 or no ray shades more than 32 floor(S / 32) samples pass
#     (S = 64, 65, 128, 129, both LDS rows, ndc-S65; in the masked row no ray keeps more than 128 samples).
#   * queue[1] not reset after D2: the two second-round rows fail and nothing else does -- round two pops from a queue that
#     is already past the pool, no tile's backward runs and the composited colours left in the partial rows are summed as
#     gradients: g_o of rays 2048 .. 2056 is 0.08 - 0.09 against references of 1e-4 (1.3 and 13 x max |t|); the copies also
#     differ from their originals bit-wise.
#   * the image's view taken from the slot index, b * 8 + w, instead of the ray (clamped to the views present; the lattice
#     index still from the ray): the four views rows fail -- sqerr 2e4 to 4.5e4 times its bound, g_o / g_d 0.77 to 4.3 --
#     and no other row does (one view: view 0 either way).  The literal form of this break -- the lattice index from the
#     wrong view as well -- reads ray_idx out of range and is not to be run.

MARGIN = 1e-5            # the clamp tie margin
KINDS = ["blender", "llff"]
STEP = P.UNIT * 0.5      # sample spacing of a thin scene at step_ratio 0.5


def build(kind, dev, near_far=(0.5, 40.0), aabb=None, masked=False):
    """the thin scene of the rows, with the appearance gain of tests/test_gpu_pose_paths.py"""
    aabb = P.thin_box(GRID) if aabb is None else aabb
    tf = P.build_scene(kind, GRID, aabb, dev, near_far=near_far)
    with torch.no_grad():
        for p in list(tf.app_plane) + list(tf.app_line):
            p.mul_(APP_GAIN)
    if masked:
        from joint_tensorf_amd.tensorf_repr import AlphaGridMask
        tf.alphaMask = AlphaGridMask(dev, M.mask_box("shrunk")[1], M.march_volume())
    return tf


def mixed(n, seed):
    """n >= 12 rays of every family of P.ray_set in a fixed scattered order (ray 0 is one of the bundle along z)"""
    aabb = P.thin_box(GRID)
    k = n - 7
    na = max(1, k // 5)
    ng = k // 5
    o, d = P.ray_set(aabb, na, k - na - ng, ng, n_miss=2, n_far_side=2, n_far_entry=3, seed=seed)
    perm = torch.cat([torch.zeros(1, dtype=torch.long),
                      1 + torch.randperm(n - 1, generator=torch.Generator().manual_seed(seed))])
    return o[perm].contiguous(), d[perm].contiguous()


def counted_rays():
    """eight rays along +z that hold 0 (miss), 0 (in the box, S-limited), 1, 31, 32, 33, 65 and 143 shaded samples at
    S = S_FULL.  k samples: the ray starts so close to the box that its march begins at t = near = 0.5, placed so that
    samples 0 .. k - 1 lie in the box, the last of them half a step before the far face.  S-limited: the ray starts more
    than `far` = 40 before the box, so its march begins at t = far, placed so that the last sample alone, number
    S_FULL - 1, lies in the box (half a step behind the near face; every coordinate involved is exact in fp32): it is
    in the box, its interval is zero, its weight is zero, it is not shaded.  The miss passes beside the box."""
    aabb = P.thin_box(GRID)
    lo_z, hi_z = aabb[2], aabb[5]
    o, d = P.ray_set(aabb, 8, 0, 0, seed=41)
    for r, k in zip((2, 3, 4, 5, 6), (1, 31, 32, 33, 65)):
        o[r, 2] = hi_z - 0.5 - (k - 0.5) * STEP
    o[0, 0] = aabb[3] + 3 * P.UNIT
    o[1, 2] = lo_z - 40.0 - (S_FULL - 1.5) * STEP
    return o.contiguous(), d.contiguous(), [0, 0, 1, 31, 32, 33, 65, 143]


def pixels(rpv, views, seed, idx=None):
    """a small random image per view and the lattice's pixels, pixel 0 and pixel HW - 1 among them"""
    g = torch.Generator().manual_seed(seed)
    H, W = 3, (rpv + 8) // 3
    image = torch.rand(views, 3, H, W, generator=g)
    if idx is None:
        idx = torch.randperm(H * W, generator=g)[:rpv]
        idx[int(torch.randint(rpv, (1,), generator=g))] = 0
        if rpv > 1:
            free = (idx != 0).nonzero()[:, 0]
            idx[free[int(torch.randint(free.numel(), (1,), generator=g))]] = H * W - 1
    target = image.view(views, 3, H * W)[:, :, idx].permute(0, 2, 1).reshape(views * rpv, 3).double()
    return image, idx.long(), target


FIG = {}     # worst figure per judged quantity over the rows of this session (printed by the last row to run)


def judge(tag, hip, ref, target):
    """every bound of the module docstring on one launch; returns the figures"""
    R = target.shape[0]
    lay = hip["layout"]
    rays = {k: P.ray_atol(hip[k].cpu(), ref[k], RAY_RTOL) for k in ("g_o", "g_d")}
    vals = {k: float((hip[k].double().cpu() - ref[k]).abs().max()) for k in ("rgb", "opacity", "depth")}
    sq_err = (hip["sqerr"].double().cpu() - ref["sqerr"]).abs()
    sq_bound = 2 * TOL_VAL * (ref["rgb"] - target).abs().sum(-1) + 3 * TOL_VAL ** 2
    sq_ratio = float((sq_err / sq_bound).max())
    scale32 = float(torch.tensor(hip["loss_scale"], dtype=torch.float32))
    want = scale32 * float(hip["sqerr"].double().sum())
    rounds = -(-R // (lay["blocks"] * lay["waves"]))
    n = rounds + lay["waves"] + lay["blocks"]
    loss_rel = abs(float(hip["loss"]) - want) / want if want > 0 else abs(float(hip["loss"]))
    words = hip["ws"].view(torch.int32)
    head = words[:2].cpu().tolist()
    tail = words[lay["head"] + lay["blocks"] * lay["waves"] * lay["slot"]:]
    dirty = int((tail != 0).sum())
    shaded = hip["count"] > 0
    lo = float(ref["rgb"][shaded].min()) if bool(shaded.any()) else 0.5
    hi = float(ref["rgb"][shaded].max()) if bool(shaded.any()) else 0.5
    fig = dict(g_o=rays["g_o"], g_d=rays["g_d"], sqerr=sq_ratio, loss=loss_rel / (n * P.EPS32),
               relu=ref["relu"].get("max_abs", 0.0), **vals)
    for k, v in fig.items():
        FIG[k] = max(FIG.get(k, 0.0), v)
    print("\n[fused] %s: %d rays, S %d (Sp %d), %d workgroups, %d round(s), %d shaded in %d tiles (per ray %s%s)" % (
        tag, R, hip["shade_mask"].shape[1], lay["Sp"], lay["blocks"], rounds, int(hip["count"].sum()),
        int(((hip["count"] + 31) // 32).sum()), hip["count"][:12].tolist(), " ..." if R > 12 else ""))
    print("   ray atol at rtol %.0e: g_o %.1e g_d %.1e (max |g| %.2e %.2e)  rgb %.1e opacity %.1e depth %.1e  sqerr %.2f of its "
          "bound  loss %.2f of %d x 2^-24  relu %.1e  colours of shaded rays in [%.4f, %.6f]" % (
              RAY_RTOL, rays["g_o"], rays["g_d"], float(ref["g_o"].abs().max()), float(ref["g_d"].abs().max()), vals["rgb"],
              vals["opacity"], vals["depth"], sq_ratio, fig["loss"], n, fig["relu"], lo, hi))
    # conditions (from the reference alone)
    assert lo >= MARGIN and hi <= 1 - MARGIN, (tag, "a shaded ray's reference colour is within the clamp tie margin", lo, hi)
    assert ref["rgb"].shape[0] == hip["rgb"].shape[0] == R and ref["g_o"].shape == hip["g_o"].shape == (R, 3)
    # the launch's own bookkeeping
    assert not hip["overruns"], (tag, "a kernel wrote past its buffer (shape, bytes changed)", hip["overruns"])
    assert head == [0, 0], (tag, "loss accumulator / arrival counter not left zeroed", head)
    assert dirty == 0, (tag, "words written behind the launch's last slot", dirty)
    assert ref["relu"].get("max_abs", 0.0) <= 2e-5, ref["relu"]
    # values
    for key, tol in (("rgb", TOL_VAL), ("opacity", TOL_VAL), ("depth", TOL_DEPTH)):
        assert vals[key] <= tol, (tag, key, vals[key])
    assert sq_ratio <= 1.0, (tag, "sqerr", sq_ratio, int((sq_err / sq_bound).argmax()))
    assert loss_rel <= n * P.EPS32, (tag, "loss", float(hip["loss"]), want, loss_rel, n)
    assert torch.isfinite(hip["g_o"]).all() and torch.isfinite(hip["g_d"]).all(), tag
    if not all(v <= RAY_ATOL for v in rays.values()):
        worst = []
        for k in ("g_o", "g_d"):
            dlt = ((hip[k].double().cpu() - ref[k]).abs() - RAY_RTOL * ref[k].abs()).flatten()
            for i in dlt.topk(min(6, dlt.numel())).indices.tolist():
                worst.append((k, i // 3, i % 3, float(hip[k].flatten()[i]), float(ref[k].flatten()[i])))
        raise AssertionError((tag, rays, worst))
    return fig


def check(tag, kind, tf, o, d, S, views=1, ndc=False, white=True, idx=None, seed=0):
    """one launch on a fresh workspace against its pinned reference; returns (hip, ref, valid [R, S] of the reference side)"""
    t0 = time.time()
    R = o.shape[0]
    rpv = R // views
    image, idx, target = pixels(rpv, views, seed, idx)
    hip = P.run_fused(tf, o, d, S, image, idx, rpv, ndc=ndc, white=white)
    t1 = time.time()
    ref = P.run_reference(tf, kind, hip, o, d, S, ndc=ndc, white=white, ray_only=True, loss=(target, hip["loss_scale"]))
    valid, _ = P.far_node_samples(tf.aabb.view(-1).tolist(), GRID, [float(tf.near_far[0]), float(tf.near_far[1])], o, d, S,
                                  ndc=ndc, device=DEV)
    judge(tag, hip, ref, target)
    # census, both sides: nothing is shaded outside the box, and a ray's count is what its slot's rank array says
    assert not bool((hip["shade_mask"] & ~valid).any()), tag
    assert hip["layout"]["blocks"] == min(256, (R + 7) // 8) and hip["layout"]["waves"] == 8
    print("   (%.1f s, %.1f s of it the launch and its decoding)" % (time.time() - t0, t1 - t0))
    return hip, ref, valid


# ---- workgroup fill ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("kind", KINDS)
def test_workgroup_fill(kind, R):
    """a single active wave, a partial and a full workgroup, a second workgroup with one ray (seven inactive waves that
    meet every barrier and pop from a pool that may be empty), a third"""
    o, d = mixed(17, seed=3)
    o, d = o[:R].contiguous(), d[:R].contiguous()
    hip, ref, valid = check("fill-%s-R%d" % (kind, R), kind, build(kind, DEV), o, d, S_FULL, seed=R)
    assert hip["layout"]["blocks"] == {1: 1, 7: 1, 8: 1, 9: 2, 17: 3}[R]
    assert int(hip["count"][0]) == 143 == int(valid[0].sum())       # the ray along z: all its in-box samples
    assert float(ref["g_o"].abs().max()) > 0.0


# ---- shaded counts at the tile edges, one workgroup -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_tile_edges(kind):
    o, d, counts = counted_rays()
    hip, ref, valid = check("tiles-%s" % kind, kind, build(kind, DEV), o, d, S_FULL, seed=5)
    assert hip["layout"]["blocks"] == 1
    assert hip["count"].tolist() == counts, hip["count"].tolist()
    # the reference side's in-box samples: the S-limited ray's one is the last of the row
    assert valid.sum(1).tolist() == [0, 1] + counts[2:] and bool(valid[1, S_FULL - 1]), valid.sum(1).tolist()
    # the pooled tile list: owners with 0, 1, 2, 3 and 5 tiles, first tiles that repeat
    assert ((hip["count"] + 31) // 32).tolist() == [0, 0, 1, 1, 1, 2, 3, 5]
    for r in (0, 1):     # nothing shaded and no weight: the background, and no gradient on either side
        for side in (hip, ref):
            assert float(side["g_o"][r].abs().max()) == 0.0 == float(side["g_d"][r].abs().max()), r
    assert float(ref["g_o"][2].abs().max()) > 0.0


# ---- S at the chunk and slot edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 128, 129])
@pytest.mark.parametrize("kind", KINDS)
def test_sample_count_edges(kind, S):
    o, d = mixed(24, seed=S)
    hip, ref, valid = check("S-%s-%d" % (kind, S), kind, build(kind, DEV), o, d, S, seed=S)
    assert hip["layout"]["Sp"] == {1: 64, 2: 64, 63: 64, 64: 64, 65: 128, 128: 128, 129: 192}[S]
    crossing = valid.any(1)
    assert int(crossing.sum()) >= 18
    if S == 1:   # the only sample is the last one: zero interval, zero weight -- nothing shaded, no gradient, the background
        assert int(hip["count"].sum()) == 0
        for side in (hip, ref):
            assert float(side["g_o"].abs().max()) == 0.0 and float(side["g_d"].abs().max()) == 0.0
        _, _, target = pixels(24, 1, S)
        assert torch.equal(hip["rgb"].cpu(), torch.ones(24, 3))
        want = float(((1.0 - target) ** 2).sum()) / 72
        assert abs(float(hip["loss"]) - want) <= 1e-6 * want
    else:        # the rays along z shade every sample but the last
        assert int(hip["count"][0]) == S - 1 and int(hip["count"].max()) == S - 1
        assert float(ref["g_o"].abs().max()) > 0.0
    if S in (65, 129):   # one live lane in the last 64-sample chunk, and it is in the box
        assert bool(valid[0, S - 1])


# ---- a second round over the same slots ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_second_round(kind):
    """2 048 + 9 rays: 256 workgroups; in round two wave 0 of workgroups 0 .. 8 alone is active and reuses the slots of
    rays 0 .. 8.  Ray 2 048 + b is a copy of ray b with the same pixel, so the decisions rays 0 .. 8 lost with their slots
    are those of their copies, and a copy must come out bit for bit as its original did: a queue counter not reset, a table
    not rewritten or scratch carried over from round one shows there."""
    S = 16
    aabb = P.thin_box(GRID)
    o, d = P.ray_set(aabb, 256, 1200, 400, n_miss=64, n_far_side=64, n_far_entry=64, seed=21)
    perm = torch.randperm(2048, generator=torch.Generator().manual_seed(21))
    o, d = o[perm], d[perm]
    o, d = torch.cat([o, o[:9]]).contiguous(), torch.cat([d, d[:9]]).contiguous()
    g = torch.Generator().manual_seed(22)
    HW = 3 * ((2057 + 8) // 3)
    idx = torch.randint(HW, (2057,), generator=g)
    idx[100], idx[200] = 0, HW - 1
    idx[2048:] = idx[:9]
    hip, ref, valid = check("round2-%s" % kind, kind, build(kind, DEV), o, d, S, idx=idx, seed=23)
    assert hip["layout"]["blocks"] == 256 and o.shape[0] > 256 * 8
    slots = P.fused_slot_of(hip["layout"], 2057)
    assert torch.equal(slots[2048:], slots[:9]) and slots[:9].tolist() == [8 * b for b in range(9)]
    assert int((hip["count"][:9] > 0).sum()) >= 5 and int(hip["count"].max()) == S - 1
    for k in ("rgb", "depth", "opacity", "sqerr", "g_o", "g_d"):
        assert torch.equal(hip[k][2048:], hip[k][:9]), (k, "a second-round copy differs from its first-round original")
    assert float(hip["g_o"][:9].abs().max()) > 0.0


# ---- several views ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_views(kind, views):
    """13 rays per view: ray -> (view, lattice point) -> pixel under the ray order scattered over the workgroups; every
    view has its own image"""
    rpv = 13
    o, d = mixed(rpv * views, seed=30 + views)
    hip, ref, _ = check("views-%s-%d" % (kind, views), kind, build(kind, DEV), o, d, S_FULL, views=views, seed=views)
    blocks = hip["layout"]["blocks"]
    per_block = [{(w * blocks + b) // rpv for w in range(8) if w * blocks + b < rpv * views} for b in range(blocks)]
    assert all(len(v) >= 2 for v in per_block), per_block     # every workgroup holds rays of different views
    image, idx, _ = pixels(rpv, views, views)
    assert 0 in idx.tolist() and image.shape[2] * image.shape[3] - 1 in idx.tolist()
    assert not torch.equal(image[0], image[1])


# ---- NDC ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [65, 151])
def test_ndc(S):
    """llff kind on NDC rays with far-side rays: the shared zvals row and the gnorm term of g_d"""
    aabb, o, d = _ndc_setup(GRID, (8, 16, 4, 0), seed=5, n_far_side=8)
    tf = build("llff", DEV, near_far=(0.0, 1.0), aabb=aabb)
    hip, ref, valid = check("ndc-S%d" % S, "llff", tf, o, d, S, ndc=True, seed=S)
    assert bool(valid[:8].all()) and int(hip["count"][:8].min()) >= S - 2
    assert float(ref["g_d"].abs().max()) > 0.0


# ---- black background ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_black_background(kind):
    o, d = mixed(24, seed=51)
    hip, ref, valid = check("black-%s" % kind, kind, build(kind, DEV), o, d, S_FULL, white=False, seed=51)
    miss = ~valid.any(1)
    assert int(miss.sum()) >= 2 and float(hip["rgb"].cpu()[miss].abs().max()) == 0.0
    assert float(ref["g_o"].abs().max()) > 0.0


# ---- alpha mask ------------------------------------------------------------------------------------------------------------------------
def test_alpha_mask():
    """the masked scene of tests/test_gpu_mask_edges.py's march rows (post-shrink box, M.march_volume) and their rays"""
    vol, (_, maabb) = M.march_volume(), M.mask_box("shrunk")
    o, d = M.march_rays()
    tf = build("blender", DEV, masked=True)
    hip, ref, valid = check("mask", "blender", tf, o, d, S_FULL, seed=61)
    _, kept, c = M.march_census(vol, maabb, o, d, S_FULL)
    assert c["dropped"] >= 0.2 * c["in_box"] and c["kept"] >= 0.2 * c["in_box"] and c["all_dropped"] >= 4, c
    assert not bool((hip["shade_mask"] & ~kept).any())      # no dropped sample was shaded
    assert int(hip["count"].sum()) >= 0.9 * c["kept"]
    dead = valid.any(1) & ~kept.any(1)                     # crossing the box with every sample dropped: the background
    assert int(hip["count"][dead].sum()) == 0 and float(hip["g_o"].cpu()[dead].abs().max()) == 0.0


# ---- the accumulator protocol -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_accumulator_protocol(kind):
    """the same inputs launched twice on one workspace, then once more after a launch with another number of rays (another
    grid size, hence another arrival count): every output of a repeat is bit-equal to the first"""
    tf = build(kind, DEV)
    o, d = mixed(24, seed=71)
    image, idx, target = pixels(24, 1, 71)
    o2, d2 = mixed(41, seed=72)
    image2, idx2, target2 = pixels(41, 1, 72)
    first = P.run_fused(tf, o, d, S_FULL, image, idx, 24)
    ref = P.run_reference(tf, kind, first, o, d, S_FULL, ray_only=True, loss=(target, first["loss_scale"]))
    judge("acc-%s-first" % kind, first, ref, target)
    again = P.run_fused_again(tf, o, d, S_FULL, image, idx, 24)
    other = P.run_fused_again(tf, o2, d2, S_FULL, image2, idx2, 41)
    ref2 = P.run_reference(tf, kind, other, o2, d2, S_FULL, ray_only=True, loss=(target2, other["loss_scale"]))
    judge("acc-%s-other" % kind, other, ref2, target2)      # (on a used workspace: its head was left zeroed)
    third = P.run_fused_again(tf, o, d, S_FULL, image, idx, 24)
    assert first["layout"]["blocks"] == 3 and other["layout"]["blocks"] == 6
    for name, run in (("second", again), ("after another R", third)):
        assert not run["overruns"] and run["ws"].view(torch.int32)[:2].cpu().tolist() == [0, 0], name
        for k in ("rgb", "depth", "opacity", "sqerr", "loss", "g_o", "g_d"):
            assert torch.equal(run[k], first[k]), (name, k)
        assert torch.equal(run["shade_mask"], first["shade_mask"]), name


# ---- the LDS limit ---------------------------------------------------------------------------------------------------------------------
def _lds_rays():
    return P.ray_set(P.thin_box(GRID), 4, 4, 0, seed=81)


@pytest.mark.parametrize("kind", KINDS)
def test_lds_limit_last_supported(kind):
    """S_max (module docstring): 4 rays along z + 4 oblique, held like any row; samples past the far face are invalid"""
    from joint_tensorf_amd import ops
    o, d = _lds_rays()
    S = FUSED_S_MAX[kind]
    try:
        hip, ref, valid = check("lds-%s-S%d" % (kind, S), kind, build(kind, DEV), o, d, S, seed=81)
    finally:
        ops._WS.pop((DEV + ":0", "pose_fused"), None)     # (gigabytes at this S)
        ops._WS.pop((DEV, "pose_fused"), None)
    assert hip["layout"]["Sp"] == S
    assert hip["count"][:4].tolist() == [143] * 4 and int(valid[:4, 143:].sum()) == 0
    assert float(ref["g_o"].abs().max()) > 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_lds_limit_first_unsupported(kind):
    """the first S whose Sp does not fit: the probe answers 0, a direct call is refused (JT_ERR_UNSUPPORTED, rc = 2,
    before any launch: the output buffer keeps its fill) and the model's render_test_fused returns None"""
    import ctypes
    from joint_tensorf_amd import ops
    from joint_tensorf_amd._lib import JtError, fused_lib
    S = FUSED_S_MAX[kind] + 1
    tf = build(kind, DEV)
    cfg = tf._render_cfg(S, False, True)
    assert fused_lib().jt_pose_fused_workspace_bytes(ctypes.byref(cfg.scene())) == 0
    assert P.fused_layout(cfg.scene(), 8) is None
    o, d = _lds_rays()
    image, idx, _ = pixels(8, 1, 82)
    guard = P.guard_band()
    with guard, pytest.raises(JtError, match=r"jt_pose_fused failed: unsupported shape \(rc=2\)"):
        ops.render_pose_fused(cfg, o.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True), None, image.to(DEV),
                              idx.to(DEV), 8, list(tf.density_plane), list(tf.density_line), list(tf.app_plane),
                              list(tf.app_line), tf.basis_mat.weight, tf.renderModule.weights())
    torch.cuda.synchronize()
    assert not guard.violations()


@pytest.mark.parametrize("config,kind", [("bat_blender_VM", "blender"), ("bat_llff_VM_MLP", "llff")])
def test_scene_past_the_lds_limit_takes_the_staged_path(config, kind):
    """test-time optimisation with opt.optim.test_fused set on a scene whose sample count is past the limit: the staged
    path renders (no fused_render_loss) and the pose receives a gradient, instead of an error from the launch"""
    from joint_tensorf_amd import ops
    from joint_tensorf_amd.options import Opt
    from tests.test_gpu_fused import _scene
    hw, grid, dens = ((48, 48), 20 ** 3, 22.0) if kind == "blender" else ((36, 48), 9000, 1.0)
    opt, model, var = _scene(config, 1, hw, grid, 64, dens)
    g = model.graph
    g.nerf.n_samples = FUSED_S_MAX[kind] + 1
    opt.optim.test_fused = True
    se3 = (0.02 * torch.randn(1, 6, device=DEV)).requires_grad_(True)
    v = Opt(dict(var))
    v.se3_refine_test = se3
    frozen = [p for p in g.parameters() if p.requires_grad]
    for p in frozen:
        p.requires_grad_(False)
    try:
        v.pose_refine_test = ops.train_pose(se3, None, torch.eye(3, 4, device=DEV))
        assert g.render_test_fused(opt, var.pose, v) is None
        assert g.nerf.tensorf._pose_fused_ok is False
        v = g.forward(opt, v, mode="test-optim")
        assert v.get("fused_render_loss") is None
        loss = model.summarize_loss(opt, v, g.compute_loss(opt, v, mode="test-optim"))
        loss.all.backward()
    finally:
        for p in frozen:
            p.requires_grad_(True)
    assert torch.isfinite(se3.grad).all() and float(se3.grad.abs().max()) > 0.0


def test_worst_figures():
    """prints the worst figure of every judged quantity over the rows that ran before it in this session"""
    print("\n[fused] worst over the session: " + "  ".join("%s %.3g" % kv for kv in sorted(FIG.items())))
