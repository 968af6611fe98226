"""tests/mask_ref.py checked on the CPU: keep() against the oracle's grid_sample in fp32 and fp64 where all three must agree
(off the node planes), against hand-worked answers where they need not (nodes, faces, outside), and the inputs of
tests/test_gpu_mask_edges.py -- the point families of the k_dense_alpha probe, the conditions of the masked march rows --
counted from the reference side alone, so that the GPU rows cannot lose their subject unnoticed."""
import pytest
import torch

from oracle import tensorf_oracle as O
from tests import mask_ref as M
from tests import pinned_ref as P


def _off_node_points(dims, aabb, n, seed):
    """points whose texel coordinate is k + u on every axis, k from two cells outside to one past the far node, u in
    [1e-3, 1 - 1e-3]: at least 1e-3 of a cell from every node plane"""
    g = torch.Generator().manual_seed(seed)
    size = torch.tensor(dims)
    k = torch.floor(torch.rand(n, 3, generator=g, dtype=torch.float64) * (size + 2)) - 2
    u = 1e-3 + (1 - 2e-3) * torch.rand(n, 3, generator=g, dtype=torch.float64)
    lo, hi = aabb[0].double(), aabb[1].double()
    return (lo + (k + u) * (hi - lo) / (size - 1)).float()


@pytest.mark.parametrize("box", ["same", "shrunk"])
@pytest.mark.parametrize("kind", ["single", "full-but-one", "random"])
def test_keep_agrees_with_grid_sample_off_the_nodes(box, kind):
    dims, aabb = M.mask_box(box)
    vol = M.volume(kind, dims)
    xyz = _off_node_points(dims, aabb, 20000, seed=3)
    fl, f = M.cells(vol.shape, aabb, xyz)
    assert float(torch.minimum(f, 1 - f).min()) > 5e-4          # (fp32 rounding of the coordinate: well below 1e-3 of a cell)
    k = M.keep(vol, aabb, xyz)
    k32 = O.alpha_mask_sample((vol, aabb), xyz) > 0
    k64 = O.alpha_mask_sample((vol.double(), aabb.double()), xyz.double()) > 0
    assert torch.equal(k, k32) and torch.equal(k, k64)
    assert 0 < int(k.sum()) < k.numel() or kind == "full-but-one"
    if kind == "full-but-one":   # "any corner", not "all": nothing inside the volume's reach is dropped
        inside = ((fl >= -1) & (fl <= torch.tensor(dims) - 1)).all(1)
        assert bool(k[inside].all()) and not bool(k[~inside].any())


def test_keep_hand_worked_nodes_faces_outside():
    """a 3 x 2 x 5 (X, Y, Z) volume over the box (0, 0, 0) .. (2, 1, 4): ix is the coordinate itself"""
    aabb = torch.tensor([[0.0, 0.0, 0.0], [2.0, 1.0, 4.0]])
    one = torch.zeros(5, 2, 3)
    one[3, 0, 1] = 1.0          # the voxel (x, y, z) = (1, 0, 3)
    cases = [
        ((1.0, 0.0, 3.0), True),     # on the node itself: fractions 0, 0, 0, the lower corner is the voxel
        ((0.5, 0.5, 2.5), True),     # interior: upper x, lower y, upper z
        ((1.5, 0.5, 3.5), True),     # interior: the lower corner on every axis
        ((2.0, 0.0, 3.0), False),    # node plane x = 2: only the corner x = 2 carries weight
        ((0.0, 0.0, 3.0), False),    # node plane x = 0: the upper corner x = 1 has weight 0
        ((0.001, 0.0, 3.0), True),   # ... and a non-zero one just beside it
        ((1.0, 0.0, 2.0), False),    # node plane z = 2: the upper corner z = 3 has weight 0
        ((1.0, 0.0, 4.0), False),    # the hi face of z: floor == size - 1, corner 4 unset, corner 5 out of range
        ((1.0, 1.0, 3.0), False),    # the hi face of y: corner y = 1 unset, y = 2 out of range
        ((1.0, 0.999, 3.0), True),
        ((1.0, -0.5, 3.0), True),    # outside, less than a cell: floor == -1, the upper corner y = 0 is the voxel
        ((1.0, -1.0, 3.0), False),   # outside, exactly one cell: fraction 0
        ((1.0, -1.5, 3.0), False),   # outside, more than a cell: both corners out of range
        ((1.0, 0.0, 3.999), True),
        ((3.0, 0.0, 3.0), False),
    ]
    xyz = torch.tensor([c[0] for c in cases])
    assert M.keep(one, aabb, xyz).tolist() == [c[1] for c in cases]
    full = torch.ones(5, 2, 3)
    cases = [
        ((2.0, 1.0, 4.0), True),     # the hi corner: the lower corner on every axis is the last voxel
        ((2.5, 1.0, 4.0), True),     # outside past hi, less than a cell: floor == size - 1, the lower corner is in range
        ((3.0, 1.0, 4.0), False),    # outside past hi, exactly one cell: floor == size
        ((2.5, 1.5, 4.5), True),
        ((-0.5, -0.5, -0.5), True),  # outside below lo on all axes, less than a cell: the upper corners (0, 0, 0)
        ((-1.0, 0.5, 2.0), False),   # exactly one cell below lo: floor == -1, fraction 0
        ((0.0, 0.0, 0.0), True),     # the lo corner
        ((1.0, 0.5, -2.5), False),
    ]
    xyz = torch.tensor([c[0] for c in cases])
    assert M.keep(full, aabb, xyz).tolist() == [c[1] for c in cases]
    # a transposed volume or a reversed dims order answers differently: the voxel (1, 0, 3) is not (3, 0, 1)
    assert not bool(M.keep(one.permute(2, 1, 0).contiguous(), torch.tensor([[0.0, 0.0, 0.0], [4.0, 1.0, 2.0]]),
                           torch.tensor([[1.0, 0.0, 1.5]])).any())


def test_fraction_is_exact_and_weights_cannot_underflow():
    """the facts mask_ref's docstring argues: the fp64 fraction reproduces ix exactly, and the smallest non-zero factor of a
    weight over all probe points is far above 2^-42 (a product of three stays normal in fp32)"""
    for box in ("same", "shrunk"):
        dims, aabb = M.mask_box(box)
        xyz = M.probe_points(dims, aabb)
        fl, f = M.cells((dims[2], dims[1], dims[0]), aabb, xyz)
        assert bool(((f >= 0) & (f < 1)).all())
        a32, x32 = aabb.float(), xyz.float()
        ix = (((x32 - a32[0]) * (1.0 / (a32[1] - a32[0]) * 2) - 1 + 1.0) * 0.5) * (torch.tensor(dims) - 1).float()
        assert torch.equal((fl.double() + f), ix.double())
        w = torch.cat([f[f > 0], (1 - f)[f < 1]])
        assert float(w.min()) >= 2.0 ** -25


@pytest.mark.parametrize("box", ["same", "shrunk"])
def test_probe_families_hold_their_floors(box):
    dims, aabb = M.mask_box(box)
    xyz = M.probe_points(dims, aabb)
    assert 19000 <= xyz.shape[0] <= 24000
    got = M.family_counts(dims, aabb, xyz)
    for k in M.FAMILIES:
        assert got[k] >= M.FLOORS[box][k], (box, k, got)
    # the single voxel sits at three different coordinates and the volumes are not cubic: a transposition changes the answer
    assert len(set(dims)) == 3
    vol = M.volume("single", dims)
    k = M.keep(vol, aabb, xyz)
    assert 100 <= int(k.sum()) <= 1000, int(k.sum())
    # the full volume with one voxel cleared drops nothing inside the box -- but a point exactly on the cleared voxel's
    # node (fraction 0 on all three axes: that voxel is the only corner with weight)
    fl, f = M.cells(vol.shape, aabb, xyz)
    inside = ((fl >= 0) & (fl < torch.tensor(dims) - 1)).all(1)
    lost = inside & ~M.keep(M.volume("full-but-one", dims), aabb, xyz)
    assert int(inside.sum()) >= 10000 and int(lost.sum()) <= 20
    assert bool((f[lost] == 0).all()) and bool((fl[lost] == torch.tensor([3, 1, 8])).all())


def test_shrunk_box_holds_the_scene_off_its_nodes():
    dims, aabb = M.mask_box("shrunk")
    scene = M.scene_box()
    assert bool((aabb[0] < scene[0]).all() and (scene[1] < aabb[1]).all())
    cells_lo = (scene[0].double() - aabb[0].double()) / torch.tensor(M.SHRUNK_PITCH, dtype=torch.float64)
    cells_hi = (aabb[1].double() - scene[1].double()) / torch.tensor(M.SHRUNK_PITCH, dtype=torch.float64)
    assert cells_lo.tolist() == [1.75, 1.375, 3.25] and cells_hi.tolist() == [0.75, 0.625, 3.875]
    # power-of-two pitches: ix of every node is the node's index, exactly
    idx = torch.stack(torch.meshgrid(*[torch.arange(n) for n in dims], indexing="ij"), -1).view(-1, 3)
    nodes = (aabb[0].double() + idx * torch.tensor(M.SHRUNK_PITCH, dtype=torch.float64)).float()
    fl, f = M.cells((dims[2], dims[1], dims[0]), aabb, nodes)
    assert torch.equal(fl, idx) and float(f.abs().max()) == 0.0


def test_march_row_conditions():
    """what tests/test_gpu_mask_edges.py's masked march rows count on, from the reference side: shares of dropped and kept
    samples, rays with every sample dropped, rays with a gap between two kept runs, kept samples on a far node"""
    dims, aabb = M.mask_box("shrunk")
    vol = M.march_volume()
    assert tuple(vol.shape) == (dims[2], dims[1], dims[0])
    o, d = M.march_rays()
    assert 70 <= o.shape[0] <= 90
    valid, kept, c = M.march_census(vol, aabb, o, d, 151)
    print("\n[mask] march rows: %d rays, %s" % (o.shape[0], c))
    assert c["dropped"] >= 0.2 * c["in_box"] and c["kept"] >= 0.2 * c["in_box"], c
    assert c["all_dropped"] >= 4 and c["gap_rays"] >= 8 and c["kept_far"] >= 1, c
    # the pinned reference renders with this decision: the oracle's own mask call, patched as reference() patches it
    cfg = P.scene_cfg(M.scene_box().view(-1).tolist(), M.SCENE_GRID, [0.5, 40.0], "llff", 0.5, 1e-7, "cpu")
    pts, _, v = O.sample_ray(cfg, o, d, 151)
    assert torch.equal(P._pinned_mask_sample((vol, aabb), pts[v].double()) > 0, kept[v])
