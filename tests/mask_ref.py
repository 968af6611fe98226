"""Pinned reference of the alpha mask's decision, AlphaGridMask.sample_alpha(xyz) > 0 on a 0/1 volume, which the
kernels take in mask_keep (csrc/jt_common.h): pure torch on the CPU.

grid_sample (trilinear, align_corners=True, zero padding) of a 0/1 volume is positive iff one of the eight corners of
the sample's cell is inside the volume, is set, and carries a non-zero weight.  As tests/pinned_ref.py pins the sample
geometry (_axis32), the normalised coordinate g and the texel coordinate ix are the fp32 VALUES of AlphaGridMask's own
expression -- (xyz - aabb[0]) * invgridSize - 1 with invgridSize = 1 / (aabb[1] - aabb[0]) * 2, then
((g + 1) * 0.5) * (size - 1), every operation separately rounded, which fp32 torch on the CPU is -- while floor(ix) and
the fraction f = ix - floor(ix) are taken as exact numbers (the subtraction is done in fp64, where it is exact for every
|ix| < 2^28) and everything after them is set logic: along an axis the lower corner floor(ix) counts iff 1 - f != 0,
the upper corner floor(ix) + 1 iff f != 0.  With an exact f in [0, 1) the lower corner always counts and the upper one
counts off the node planes only.

No fp32 weight product of the kernel can underflow to zero where the exact weight is non-zero, for any size >= 2 (a
size of 1 has ix == 0 identically): g is the rounded result of (...) - 1, hence a multiple of 2^-24 wherever |g + 1| <
1/2, so a non-zero g + 1 is at least 2^-24 in magnitude, h = (g + 1) * 0.5 at least 2^-25 (exact), and the rounded
ix = h (size - 1) at least 2^-25.  For 0 < ix < 1 the fraction is ix itself; for ix >= 1 it is a multiple of
ulp(ix) >= 2^-23; for -1 < ix < 0, the one negative cell with a corner in range, the fp32 fraction ix + 1 is at least
1/2 (and may round to 1: that zeroes the weight of corner -1, which is out of range anyway).  1 - f of an fp32 f < 1 is
at least 2^-24.  Every factor of a non-zero weight is therefore >= 2^-25 and the product of three >= 2^-75, far above
the smallest normal fp32 number 2^-126: `w > 0` in fp32 is `w != 0` exactly."""
import torch


def cells(shape_zyx, aabb, xyz):
    """(floor(ix) [N, 3] int64, f [N, 3] float64) per axis (x, y, z) of points xyz [N, 3] in a mask volume of shape
    [Z, Y, X] over the box aabb [2, 3]: the fp32 values of AlphaGridMask's expression, floor and fraction exact"""
    aabb = aabb.detach().float().cpu()
    xyz = xyz.detach().float().cpu()
    size = torch.tensor([shape_zyx[2], shape_zyx[1], shape_zyx[0]])
    inv = 1.0 / (aabb[1] - aabb[0]) * 2                 # AlphaGridMask.invgridSize
    g = (xyz - aabb[0]) * inv - 1                       # AlphaGridMask.normalize_coord: three rounded fp32 operations
    ix = ((g + 1.0) * 0.5) * (size - 1).float()         # grid_sample's unnormalise, align_corners=True
    assert g.dtype == torch.float32 and ix.dtype == torch.float32
    fl = torch.floor(ix)
    f = ix.double() - fl.double()
    return fl.long(), f


def keep(volume, aabb, xyz):
    """bool [N]: the mask volume [Z, Y, X] (0/1) over aabb [2, 3] keeps the points xyz [N, 3]"""
    vol = volume.detach().cpu().reshape(volume.shape[-3:]) > 0
    Z, Y, X = vol.shape
    size = (X, Y, Z)
    i0, f = cells(vol.shape, aabb, xyz)
    counts = ((1.0 - f) != 0, f != 0)                   # per axis: the lower / upper corner carries weight
    out = torch.zeros(i0.shape[0], dtype=torch.bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ok = torch.ones_like(out)
                idx = []
                for a, da in enumerate((dx, dy, dz)):
                    c = i0[:, a] + da
                    ok &= (c >= 0) & (c < size[a]) & counts[da][:, a]
                    idx.append(c.clamp(0, size[a] - 1))
                out |= ok & vol[idx[2], idx[1], idx[0]]
    return out


# ---- the hand-made masks and point families of tests/test_gpu_mask_edges.py (checked on the CPU by tests/test_mask_ref.py) ----
SCENE_GRID = [12, 9, 72]          # the thin scene of tests/test_gpu_pose_paths.py: texel pitch 1 / 128 on every axis
DIMS_SAME = (7, 5, 19)            # (X, Y, Z) of the mask that shares the scene's box: 6, 4 and 18 cells, pitches not exact
DIMS_SHRUNK = (9, 5, 17)          # (X, Y, Z) of the post-shrink mask: 8, 4 and 16 cells of 1/64, 1/32, 1/16 -- every node
#                                   coordinate, the normalised coordinate and ix of a node are exact in fp32
SHRUNK_LO = (-18 / 256, -19 / 256, -123 / 256)
SHRUNK_PITCH = (1 / 64, 1 / 32, 1 / 16)


def scene_box():
    h = [(g - 1) / 256 for g in SCENE_GRID]
    return torch.tensor([[-h[0], -h[1], -h[2]], h], dtype=torch.float32)


def mask_box(which):
    """(dims (X, Y, Z), aabb [2, 3] fp32).  `same`: the scene's box.  `shrunk`: the state after shrink -- the old, larger
    box; the scene box lies strictly inside it, 1.75 / 0.75 (x), 1.375 / 0.625 (y) and 3.25 / 3.875 (z) mask cells from
    its lo / hi faces, with texel pitches that are powers of two"""
    if which == "same":
        return DIMS_SAME, scene_box()
    lo = torch.tensor(SHRUNK_LO, dtype=torch.float64)
    hi = lo + torch.tensor([(n - 1) * p for n, p in zip(DIMS_SHRUNK, SHRUNK_PITCH)], dtype=torch.float64)
    return DIMS_SHRUNK, torch.stack([lo, hi]).float()


def volume(kind, dims, seed=0):
    """0/1 volume [Z, Y, X]: `single` one set voxel at (x, y, z) = (1, 2, 3); `full-but-one` all set but (3, 1, 8);
    `random` about 40 % set"""
    X, Y, Z = dims
    if kind == "single":
        v = torch.zeros(Z, Y, X)
        v[3, 2, 1] = 1.0
    elif kind == "full-but-one":
        v = torch.ones(Z, Y, X)
        v[8, 1, 3] = 0.0
    else:
        v = (torch.rand(Z, Y, X, generator=torch.Generator().manual_seed(seed)) < 0.4).float()
    return v


def march_volume(seed=0):
    """the volume [Z, Y, X] of the masked march rows, over the `shrunk` box (the scene spans mask cells 1.75 .. 7.25 in x,
    1.375 .. 3.375 in y, 3.25 .. 12.125 in z): nothing set at x <= 4 -- a ray along z through the low-x part of the scene
    has every sample dropped --, two slabs z in {3, 4} and {9 .. 13} with an empty stretch between them -- a ray along z
    through the high-x part keeps two runs with a gap of three cells, 96 samples, between them --, and one in eight of the
    set voxels cleared at random"""
    X, Y, Z = DIMS_SHRUNK
    v = torch.zeros(Z, Y, X)
    v[[3, 4, 9, 10, 11, 12, 13], :, 5:] = 1.0
    hole = torch.rand(Z, Y, X, generator=torch.Generator().manual_seed(seed)) < 0.125
    return v * (~hole).float()


def march_rays(seed=5):
    """about 80 rays of the mixed families of pinned_ref.ray_set on the thin scene"""
    from tests import pinned_ref as P
    return P.ray_set(scene_box().view(-1).tolist(), 24, 28, 12, n_miss=4, n_far_side=8, n_far_entry=8, seed=seed)


def march_census(vol, mask_aabb, o, d, S, near_far=(0.5, 40.0), step_ratio=0.5):
    """From the reference side alone (the oracle's fp32 sampler on the CPU, keep() and pinned_ref's far-node test): valid
    [R, S] (in the scene box), kept [R, S] (valid and kept by the mask), and the counts the masked rows assert --
    in-box samples, dropped and kept among them, rays that cross the box with every sample dropped, rays with a dropped
    stretch between two kept runs, kept samples on a far node of a factor"""
    from oracle import tensorf_oracle as O
    from tests import pinned_ref as P
    aabb = scene_box().view(-1).tolist()
    cfg = P.scene_cfg(aabb, SCENE_GRID, list(near_far), "llff", step_ratio, 1e-7, "cpu")
    pts, _, valid = O.sample_ray(cfg, o.float(), d.float(), S)
    kept = valid.clone()
    kept[valid] = keep(vol, mask_aabb, pts[valid])
    _, far = P.far_node_samples(aabb, SCENE_GRID, near_far, o, d, S, step_ratio=step_ratio)
    gaps = 0
    for r in range(valid.shape[0]):
        k = kept[r].nonzero()[:, 0]
        if k.numel() >= 2 and bool((valid[r] & ~kept[r])[int(k[0]):int(k[-1])].any()):
            gaps += 1
    n = int(valid.sum())
    return valid, kept, dict(in_box=n, dropped=n - int(kept.sum()), kept=int(kept.sum()),
                             all_dropped=int((valid.any(1) & ~kept.any(1)).sum()), gap_rays=gaps,
                             kept_far=int((far.any(-1) & kept).sum()))


FAMILIES = ("interior", "node1", "node2", "node3", "face_lo", "face_hi", "outside_near", "outside_far", "ulp")


def probe_points(dims, aabb, seed=0, n_interior=12000, n_each=1200):
    """about 20 000 points [N, 3] fp32 around a mask of `dims` over `aabb`: random interior points; points on mask nodes
    along one, two and three axes; points on the lo and hi faces; points outside the box, less than one cell and one to
    three cells away; points one fp32 ulp either side of a node plane.  Node coordinates are formed in fp64 and rounded:
    exact for the power-of-two box, within an ulp of the node otherwise (family_counts says where they landed)."""
    g = torch.Generator().manual_seed(seed)
    size = torch.tensor(dims)
    lo, hi = aabb[0].double(), aabb[1].double()
    pitch = (hi - lo) / (size - 1)

    def inside(n):
        return lo + (hi - lo) * torch.rand(n, 3, generator=g, dtype=torch.float64)

    def node(n):
        return lo + pitch * torch.floor(torch.rand(n, 3, generator=g, dtype=torch.float64) * size)

    def axes(n, k):
        """[n, 3] bool with exactly k axes chosen per row"""
        order = torch.rand(n, 3, generator=g).argsort(1)
        return order < k

    out = [inside(n_interior)]
    for k in (1, 2, 3):
        out.append(torch.where(axes(n_each, k), node(n_each), inside(n_each)))
    out.append(torch.where(axes(n_each, 1), lo.expand(n_each, 3), inside(n_each)))
    out.append(torch.where(axes(n_each, 1), hi.expand(n_each, 3), inside(n_each)))
    for a, b in ((0.05, 0.95), (1.05, 3.0)):
        u = (a + (b - a) * torch.rand(n_each, 3, generator=g, dtype=torch.float64)) * pitch
        side = torch.rand(n_each, 3, generator=g) < 0.5
        out.append(torch.where(axes(n_each, 1), torch.where(side, lo - u, hi + u), inside(n_each)))
    p = torch.cat(out).float()
    nd = node(2 * n_each).float()
    up = torch.rand(2 * n_each, 3, generator=g) < 0.5
    near = torch.nextafter(nd, torch.where(up, torch.tensor(float("inf")), torch.tensor(float("-inf"))))
    p = torch.cat([p, torch.where(axes(2 * n_each, 1), near, inside(2 * n_each).float())])
    return p.contiguous()


def family_counts(dims, aabb, xyz):
    """how many of the points sit where each family is meant to put them, from cells() alone"""
    size = torch.tensor(dims)
    fl, f = cells((dims[2], dims[1], dims[0]), aabb, xyz)
    in_rng = (fl >= 0) & (fl <= size - 1) & ~((fl == size - 1) & (f > 0))
    on = (f == 0) & in_rng
    n_on = on.sum(1)
    all_in = in_rng.all(1)
    near_out = ((fl == -1) & (f > 0)) | ((fl == size - 1) & (f > 0))
    far_out = (fl < -1) | ((fl == -1) & (f == 0)) | (fl >= size)
    d = torch.minimum(f, 1 - f)
    return dict(interior=int((all_in & (n_on == 0)).sum()), node1=int((all_in & (n_on == 1)).sum()),
                node2=int((all_in & (n_on == 2)).sum()), node3=int((all_in & (n_on == 3)).sum()),
                face_lo=int((on & (fl == 0)).any(1).sum()), face_hi=int((on & (fl == size - 1)).any(1).sum()),
                outside_near=int((near_out.any(1) & ~far_out.any(1)).sum()), outside_far=int(far_out.any(1).sum()),
                ulp=int(((d > 0) & (d < 1e-4)).any(1).sum()))


# Lower bounds per family, by construction for `shrunk` (1 200 points generated per family, 2 400 for ulp, every node exact).
# `same` has inexact pitches: a rounded node coordinate may miss f == 0 (its lo faces, xyz - lo == 0, are exact), so its node
# floors are below what was generated.  The ulp family counts the points whose fraction is within 1e-4 of a node and not on
# it: a point one ulp from a node plane often lands ON the node, because xyz - aabb[0] and the - 1 of the normalisation
# round the ulp away -- those count as node points, which is what the kernel sees as well.
# Counted (seed 0): shrunk interior 12 651, node1 5 241, node2 1 200, node3 1 200, face_lo 2 091, face_hi 2 305,
# outside_near 1 308, outside_far 1 200, ulp 770; same 13 047, 5 433, 1 286, 496, 2 121, 2 408, 1 338, 1 200, 2 392.
FLOORS = {
    "shrunk": dict(interior=10000, node1=1000, node2=1000, node3=1000, face_lo=1000, face_hi=1000, outside_near=1000,
                   outside_far=1000, ulp=500),
    "same": dict(interior=10000, node1=1000, node2=1000, node3=400, face_lo=1000, face_hi=1000, outside_near=1000,
                 outside_far=1000, ulp=500),
}
