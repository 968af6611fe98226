"""The float LDS line of the backward scatters and of the density walk (RecWalker, LDSL == 1) summed without the LDS float
atomic (joint_tensorf_amd/csrc/jt_lds_sum.h), under ray sets chosen to make the line sums collide.

Every scene is a thin scene of tests/test_gpu_scatter_shapes.py at a length that selects one float-line shape (its budget
arithmetic is in that module's docstring); each row asserts that the expected instantiation ran and judges, through that
module's own _check_row, every element of every factor gradient (zero outside the footprint, |G - T| <= kappa 2^-24 M inside,
the imported KAPPA), every element of the ray gradients (RAY_*) and the dense gradients (DENSE_TOL) against the pinned fp64
reference of tests/pinned_ref.py.

Ray sets:
  fan      256 rays in ONE plane of constant long-axis coordinate, half a texel between two nodes of the long line, fanned over
           the cross-section: every sample of every wave of every workgroup lands on the same two texels of the long line
           (~ 5 000 contributions each), and on the two short lines (12 and 9 cells) that everything shares anyway.
  repeat   one oblique ray 64 times back to back: the four groups of an instruction and the neighbouring waves flush
           identical addresses at the same time; the ray crosses about half of the long axis before it leaves through a
           side, ~ 19 000 samples whose short-line texels take 2 000 - 4 000 contributions each.
  axial    a bundle of 48 rays along the long axis over its first 50 texels, samples half a texel apart: a line cell is left
           every second step.
All three put more than 1 024 shaded samples (two workgroups of the sixteen-wave shape with runs of 16) and more than 16 wave
items per plane of the walk on the device.  The walk rows are padded with rays that miss the box to the 1 000 rays at which
tests/test_gpu_scatter_shapes.py places the walk's shapes (the prefix table is part of the budget).

(The two 20-channel scatter shapes keep the float atomic on their line -- the compare-and-swap sum measured slower there,
profiles/lds_line_sum.txt section 8 -- so their rows hold the parent's form and the plain coordinate-gradient stores; the
VM-48 shapes and the two walk shapes run the compare-and-swap sum.)

What a broken sum looks like: a flush that is lost or doubled is 2^24 x its share of M.  Built with a one-round
compare-and-swap and no fallback in every kernel (a failed swap drops the addend), all eighteen rows fail at kappa 8e5 - 1e7
on the app / density lines (profiles/lds_line_sum.txt section 7); the parent's float-atomic build and this one stay below a
quarter of KAPPA per kind on every row (same section)."""
import math

import pytest
import torch

from tests import pinned_ref as P
from tests.test_gpu_scatter_shapes import SC20, SC48, SHORT, WALK, _check_row

pytestmark = pytest.mark.gpu

# id: (kind, L, Cd, kernel variant, rays in all (0: no padding), expected kernel)
SCENES = {
    "vm48-L441": ("blender", 441, 16, "mfma", 0, SC48 + "false, 8, 12, 3>"),
    "vm48-split16-L409": ("blender", 409, 16, "mfma-split16", 0, SC48 + "false, 16, 8, 3>"),
    "c20-L140": ("llff", 140, 16, "mfma", 0, SC20 + "false, 16, 16, 3>"),
    "c20-L141": ("llff", 141, 16, "mfma", 0, SC20 + "false, 16, 8, 3>"),
    "walk-L561": ("llff", 561, 16, "mfma", 1000, WALK + "16, false, 1, 16>"),
    "walk-cd8-L1185": ("llff", 1185, 8, "mfma", 1000, WALK + "8, false, 1, 16>"),
}
RAYSETS = ("fan", "repeat", "axial")
N_FAN, N_REPEAT, N_AXIAL = 256, 64, 48
S_AXIAL = 101   # samples of an axial ray: the first 50 texels of the long axis


def _misses(aabb, n, seed):
    if n <= 0:
        return torch.zeros(0, 3), torch.zeros(0, 3)
    return P.ray_set(aabb, 0, 0, 0, n_miss=n, seed=seed)


def make_rays(which, grid, aabb, n_total):
    """(origins, directions, samples per ray) of a ray set on the thin scene `grid`"""
    L = grid[2]
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])
    g = torch.Generator().manual_seed(1000 + L)
    if which == "fan":
        # z0: half a texel past node L // 2 (exact in fp32: a multiple of UNIT / 2), d_z = 0: every sample has z == z0
        z0 = float(lo[2]) + (L // 2 + 0.5) * P.UNIT
        tgt = lo + (hi - lo) * torch.rand(N_FAN, 3, generator=g)
        phi = 2 * math.pi * torch.rand(N_FAN, generator=g)
        d = torch.stack([torch.cos(phi), torch.sin(phi), torch.zeros(N_FAN)], -1)
        o = tgt - 3.0 * d
        o[:, 2] = z0
        S = 40   # the cross-section's diagonal is 13.6 texels = 28 samples
    elif which == "repeat":
        # enters through the z = lo face a third of the way in from the (lo, lo) corner, leaves through the x = hi side
        # after (2 / 3) 11 / 0.05 = 147 z texels ... or through the far face when the line is shorter
        d1 = torch.tensor([0.05, 0.03, 1.0])
        d1 = d1 / d1.norm()
        e = lo + (hi - lo) * torch.tensor([0.33, 0.31, 0.0])
        o1 = e - 3.0 * d1
        o, d = o1[None].repeat(N_REPEAT, 1), d1[None].repeat(N_REPEAT, 1)
        S = 2 * min(L - 1, 160) + 9
    else:
        # (the first 50 texels of the long axis only.  A ray along z puts ALL its samples on one cell of the plane across it;
        #  with 24 rays over the whole axis the PARENT's density planes reach kappa 1 633 on vm48-split16-L409 -- one texel,
        #  1 445 - 1 581 at 65 - 201 samples per ray too -- above a quarter of KAPPA; with 48 rays and 101 samples it is 78
        #  (profiles/lds_line_sum.txt).  The line sums do not need the length.)
        o, d = P.ray_set(aabb, N_AXIAL, 0, 0, seed=1000 + L)
        S = S_AXIAL
    mo, md = _misses(aabb, n_total - o.shape[0], seed=2000 + L)
    return torch.cat([o, mo]).float().contiguous(), torch.cat([d, md]).float().contiguous(), S


@pytest.mark.parametrize("rays", RAYSETS)
@pytest.mark.parametrize("scene", list(SCENES))
def test_line_sum_row(scene, rays):
    kind, L, cd, variant, n_total, expect = SCENES[scene]
    grid = [SHORT[0], SHORT[1], L]
    aabb = P.thin_box(grid)
    o, d, S = make_rays(rays, grid, aabb, n_total)
    hip, ref = _check_row("%s-%s" % (scene, rays), kind, grid, aabb, o, d, S, cd=cd, variant=variant, expect=[expect],
                          long_line=False)
    shaded = int(hip["shade_mask"].sum())
    assert shaded > 1024, (scene, rays, shaded)   # two workgroups of every scatter shape
    # "several thousand contributions per contended texel", from the shaded count: every sample of the fan adds to both of its
    # two long-line texels; every sample of the repeat set adds to two cells of each short line, so 2 shaded / cells is the
    # MEAN per cell of a short line if the ray touched all of its cells (it touches fewer: a lower bound)
    if rays == "fan":
        assert shaded >= 3000, (scene, shaded)
    if rays == "repeat":
        assert 2 * shaded / max(SHORT) >= 2000, (scene, shaded)
    if rays == "fan":   # all of it on two texels of the long line (line 0, [1, C, L, 1])
        for fam in ("density_line.0", "app_line.0"):
            assert int(ref["F"][fam][0].any(0).sum()) == 2, (scene, fam)
