"""The element-wise gradient criterion of tests/test_gpu_scatter_shapes.py checked on the oracle alone (CPU, fp64): the
magnitude M bounds the reference gradient, the reference gradient is zero outside the footprint F, and a single lost or
misplaced sample contribution -- the failure of branch-specific scatter code -- is caught element by element, at the
kappa the GPU module enforces, where the norm-wise check of test_gpu_fuzz.py (3e-3 of the tensor's largest element) lets
it pass; on a scene with a long line, most single contributions are caught (the rest are below kappa 2^-24 of their
texel)."""
import torch

from oracle import tensorf_oracle as O
from tests import pinned_ref as P
from tests.test_gpu_scatter_shapes import KAPPA as KAPPA_GPU

KAPPA = max(KAPPA_GPU.values())   # the largest kappa tests/test_gpu_scatter_shapes.py holds the kernels to
FUZZ_TOL = 3e-3         # test_gpu_fuzz.py: max |G - T| <= 3e-3 max |T|


def _scene_params(seed, grid):
    cd, ca, app_dim, hid = 4, 6, 5, 16
    g = torch.Generator().manual_seed(seed)
    dt = torch.float64
    sigma = 1.5 / (25.0 * (grid[2] - 1) * P.UNIT)
    a = ((10.0 + float(torch.log(torch.expm1(torch.tensor(sigma, dtype=dt))))) / (3 * cd)) ** 0.5
    p = dict(density_plane=[], density_line=[], app_plane=[], app_line=[])
    for i in range(3):
        m0, m1 = O.MAT_MODE[i]
        v = O.VEC_MODE[i]
        p["density_plane"].append(a * (0.5 + torch.rand(1, cd, grid[m1], grid[m0], generator=g, dtype=dt)))
        p["density_line"].append(a * (0.5 + torch.rand(1, cd, grid[v], 1, generator=g, dtype=dt)))
        p["app_plane"].append(0.3 * torch.randn(1, ca, grid[m1], grid[m0], generator=g, dtype=dt))
        p["app_line"].append(0.3 * torch.randn(1, ca, grid[v], 1, generator=g, dtype=dt))
    p["basis"] = 0.3 * torch.randn(app_dim, 3 * ca, generator=g, dtype=dt)
    n_in = app_dim + 3 + 2 * 2 * app_dim + 2 * 2 * 3  # MLP_Fea: [f, d, PE(f), PE(d)] with fea_pe = view_pe = 2
    p["mlp"] = dict(w1=0.3 * torch.randn(hid, n_in, generator=g, dtype=dt), b1=0.1 * torch.randn(hid, generator=g, dtype=dt),
                    w2=0.3 * torch.randn(hid, hid, generator=g, dtype=dt), b2=0.1 * torch.randn(hid, generator=g, dtype=dt),
                    w3=0.3 * torch.randn(3, hid, generator=g, dtype=dt), b3=0.1 * torch.randn(3, generator=g, dtype=dt))
    for _, v in O.flat_params(p):
        v.requires_grad_(True)
    return p


def _scene(seed=0, grid=(6, 5, 11), rays=(6, 12, 4)):
    grid = list(grid)
    aabb = P.thin_box(grid)
    p = _scene_params(seed, grid)
    cfg = P.scene_cfg(aabb, grid, [0.5, 40.0], "blender", 0.5, 1e-7, "cpu", torch.float64)
    o, d = P.ray_set(aabb, *rays, seed=seed)
    S = 2 * grid[2] + 6
    ref = P.reference(cfg, p, o, d, S, P.cotangents(o.shape[0], seed), keep=True)
    return grid, ref


def _fuzz_passes(G, T):
    return float((G - T).abs().max()) <= FUZZ_TOL * float(T.abs().max()) + 1e-10


def test_magnitude_bounds_gradient_and_footprint_holds_it():
    grid, ref = _scene()
    for n in P.FACTORS:
        T, M, F = ref["T"][n], ref["M"][n], ref["F"][n]
        assert (T.abs() <= M * (1 + 1e-12)).all(), n
        assert (M[~F] == 0).all() and (T[~F] == 0).all(), n
        assert F.any(), n
        # the exact gradient passes its own criterion with kappa 0, and writes nothing outside F
        assert P.factor_errors(T, T, M, F)[:2] == (0, 0.0), n
    # the bundle along the long axis enters through the end face: every texel of the long line is in the footprint
    assert ref["F"]["density_line.0"].all() and ref["F"]["app_line.0"].all()
    assert ref["T"]["density_line.0"].shape[2] == grid[2]


def _one_contribution(ref, name):
    """one sample's contribution c to one texel of factor `name` with |c| below the norm-wise tolerance and above the
    element-wise bound at twice KAPPA: (texel index, neighbour index along the line, c)"""
    T, M = ref["T"][name], ref["M"][name]
    tmax = float(T.abs().max())
    for n, factor, out, U in ref["samples"]:
        if n != name:
            continue
        for p in range(out.shape[1]):
            if not bool((U[:, p] != 0).any()):
                continue
            gout = torch.zeros_like(out)
            gout[:, p] = U[:, p]
            c = torch.autograd.grad(out, factor, grad_outputs=gout, retain_graph=True)[0].flatten()
            ok = (c.abs() > 0) & (c.abs() <= 0.9 * FUZZ_TOL * tmax) & (c.abs() > 2 * KAPPA * P.EPS32 * M.flatten())
            if ok.any():
                k = int(ok.nonzero()[0])
                nb = k + 1 if (k + 1) % T.shape[2] != 0 else k - 1   # the next texel along the line, same channel
                return k, nb, float(c[k])
    raise AssertionError("no small contribution found for %s" % name)


def test_lost_or_moved_contribution_is_caught_elementwise_only():
    _, ref = _scene()
    for name in ("density_line.0", "app_line.0"):
        T, M, F = ref["T"][name], ref["M"][name], ref["F"][name]
        k, nb, c = _one_contribution(ref, name)
        lost = T.clone().flatten()
        lost[k] -= c
        lost = lost.view_as(T)
        moved = lost.clone().flatten()
        moved[nb] += c
        moved = moved.view_as(T)
        for G in (lost, moved):
            assert _fuzz_passes(G, T), name   # the norm-wise check does not see it
            stray, ratio, _ = P.factor_errors(G, T, M, F)
            assert stray > 0 or ratio > KAPPA, (name, ratio)
        # the texel that lost it fails on its own
        assert P.factor_errors(lost, T, M, F)[1] > 2 * KAPPA * 0.99


def test_stray_write_outside_footprint_is_caught():
    _, ref = _scene()
    hit = False
    for name in P.FACTORS:
        T, M, F = ref["T"][name], ref["M"][name], ref["F"][name]
        if F.all():
            continue
        G = T.clone()
        G[~F] = 1e-30 * float(T.abs().max() + 1)
        assert _fuzz_passes(G, T)
        assert P.factor_errors(G, T, M, F)[0] == int((~F).sum())
        hit = True
    assert hit, "every factor's footprint is complete: no stray write to test"


def test_single_contributions_of_a_long_line_are_caught():
    """every single-sample contribution of a random subset, removed on its own, on a scene whose long line has 160
    texels and whose texels each sum the contributions of many samples: the element-wise check, at the kappa of the
    factor's family, catches most of them.  The ones it misses are below kappa 2^-24 of their texel's magnitude: samples
    whose upstream gradient is orders of magnitude below the texel's other samples' (deep in a ray, grazing)."""
    _, ref = _scene(seed=1, grid=(12, 9, 160), rays=(16, 24, 8))
    g = torch.Generator().manual_seed(3)
    for name in ("density_line.0", "app_line.0", "density_plane.1", "app_plane.1"):
        M = ref["M"][name].flatten()
        kappa = KAPPA_GPU[name.split(".")[0]]
        caught = total = 0
        for n, factor, out, U in ref["samples"]:
            if n != name:
                continue
            live = (U != 0).any(0).nonzero()[:, 0]
            for p in live[torch.randperm(live.numel(), generator=g)[:40]].tolist():
                gout = torch.zeros_like(out)
                gout[:, p] = U[:, p]
                c = torch.autograd.grad(out, factor, grad_outputs=gout, retain_graph=True)[0].flatten()
                for k in (c != 0).nonzero()[:, 0].tolist():
                    total += 1
                    caught += int(abs(float(c[k])) > kappa * P.EPS32 * float(M[k]))
        print("\n[checker] %s: %d of %d single contributions caught at kappa %g" % (name, caught, total, kappa))
        assert total >= 100, (name, total)
        # (measured: 82 %, 86 %, 87 % and 88 %; the misses are contributions below kappa 2^-24 of their texel)
        assert caught >= (0.4 if name.startswith("app_plane") else 0.75) * total, (name, caught, total)


# ---- the far-node ray families of tests/test_gpu_pose_paths.py, on the fp32 oracle alone ------------------------------------
# A sample on a far node (floor(ix) == size - 1) is where the pose gather must take the masked form of the interpolation; the
# GPU rows count on these rays to put samples there.  If thin_box, UNIT or the families change so that the samples slip off
# the nodes, these cases fail here -- the GPU rows would only lose their subject.
def test_far_node_families_leave_existing_rays_alone():
    for grid, rays, seed in (([12, 9, 72], (8, 16, 4, 3), 72), ([11, 9, 72], (8, 16, 4, 0), 63)):
        aabb = P.thin_box(grid)
        o0, d0 = P.ray_set(aabb, *rays[:3], n_miss=rays[3], seed=seed)
        o1, d1 = P.ray_set(aabb, *rays[:3], n_miss=rays[3], seed=seed, n_far_side=6, n_far_entry=5)
        n = sum(rays)
        assert o1.shape[0] == n + 11 and torch.equal(o1[:n], o0) and torch.equal(d1[:n], d0)
    from tests.test_gpu_scatter_shapes import _ndc_setup
    _, o0, d0 = _ndc_setup([12, 9, 72], (8, 16, 4, 0), seed=3)
    _, o1, d1 = _ndc_setup([12, 9, 72], (8, 16, 4, 0), seed=3, n_far_side=6)
    assert o1.shape[0] == 34 and torch.equal(o1[:28], o0) and torch.equal(d1[:28], d0)


def test_far_side_and_far_entry_rays_sit_on_far_nodes():
    for grid, in_box in (([12, 9, 72], 2288), ([12, 9, 200], 6384), ([11, 9, 72], 2288)):
        aabb = P.thin_box(grid)
        S = 2 * (grid[2] - 1) + 9
        o, d = P.ray_set(aabb, 0, 0, 0, seed=1, n_far_side=16)
        valid, far = P.far_node_samples(aabb, grid, (0.5, 40.0), o, d, S)
        assert int(valid.sum()) == in_box and (valid.sum(1) == in_box // 16).all(), grid
        for k in range(16):   # alternating: x == hi (the 11- or 10-cell axis), y == hi (the 8-cell axis)
            assert bool(far[k, :, k % 2][valid[k]].all()), (grid, k)
            assert int(far[k, :, 2].sum()) == 1   # and the one sample on the far end face
        o, d = P.ray_set(aabb, 0, 0, 0, seed=1, n_far_entry=16)
        valid, far = P.far_node_samples(aabb, grid, (0.5, 40.0), o, d, S)
        assert int(valid.sum()) == in_box, grid
        assert bool(far[:, 0, 2].all()) and (far.any(-1).sum(1) == 1).all(), grid   # the first sample, and no other
        # every full-length ray of the axial bundle ends on the far node of the long axis: one far-node sample per ray
        o, d = P.ray_set(aabb, 8, 0, 0, seed=1)
        _, far = P.far_node_samples(aabb, grid, (0.5, 40.0), o, d, S)
        assert (far.any(-1).sum(1) == 1).all(), grid
        # ... and none when S ends the bundle before the far face
        _, far = P.far_node_samples(aabb, grid, (0.5, 40.0), o, d, 100)
        assert not bool(far.any()), grid


def test_ndc_far_side_rays_sit_on_far_nodes():
    from tests.test_gpu_scatter_shapes import _ndc_setup
    for grid in ([12, 9, 72], [12, 9, 1063]):
        S = 2 * (grid[2] - 1) + 1
        aabb, o, d = _ndc_setup(grid, (8, 0, 0, 0), seed=3, n_far_side=16)
        valid, far = P.far_node_samples(aabb, grid, (0.0, 1.0), o, d, S, ndc=True)
        assert bool(valid.all()), grid
        for k in range(16):
            assert bool(far[8 + k, :, k % 2].all()), (grid, k)
        assert bool(far[:, -1, 2].all()), grid    # t = far = 1: z = +1
        assert int(far[:8].any(-1).sum()) == 8, grid   # the plain bundle: that last sample only


def test_census_counts_tiles_per_chunk():
    far = torch.zeros(3, 100, dtype=torch.bool)
    mask = torch.zeros(3, 100, dtype=torch.bool)
    mask[0, :70] = True      # entries 0 .. 69
    mask[2, 10:100] = True   # entries 70 .. 159
    far[0, 5] = True         # entry 5: tile 0
    far[1, 7] = True         # not shaded: no entry
    far[2, 10] = True        # entry 70: tile 2 of one chunk; entry 6 = tile 0 of the second chunk of 64
    far[2, 99] = True        # entry 159: the last tile
    c = P.census(far, mask)
    assert c == dict(shaded=160, tiles=[5], far_tiles=3, plain_tiles=2, far_entries=3), c
    c = P.census(far, mask, chunk=64)
    assert c == dict(shaded=160, tiles=[2, 2, 1], far_tiles=3, plain_tiles=2, far_entries=3), c
    c = P.census(far[..., None].expand(3, 100, 3), torch.zeros_like(mask))
    assert c == dict(shaded=0, tiles=[], far_tiles=0, plain_tiles=0, far_entries=0), c


# ---- the additions for the single-launch pose kernel (tests/test_gpu_pose_fused_edges.py) -------------------------------------
def test_loss_form_equals_cotangent_form():
    """d / d rays of loss_scale * sum (clamp(rgb) - target)^2 is the cotangent form with cot = 2 loss_scale (rgb - target)
    taken from the reference's own rgb (no ray that meets the scene has a colour on the clamp's ends), and nothing on the opacity"""
    grid = [6, 5, 11]
    aabb = P.thin_box(grid)
    o, d = P.ray_set(aabb, 6, 12, 4, seed=0)
    S = 2 * grid[2] + 6
    R = o.shape[0]
    p = _scene_params(0, grid)
    for _, v in O.flat_params(p):
        v.requires_grad_(False)
    cfg = P.scene_cfg(aabb, grid, [0.5, 40.0], "blender", 0.5, 1e-7, "cpu", torch.float64)
    target = torch.rand(R, 3, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    scale = 1.0 / (3 * R)
    a = P.reference(cfg, p, o, d, S, None, ray_only=True, loss=(target, scale))
    hit = a["opacity"] > 0      # (a ray that misses is the background, exactly 1, and has no gradient in either form)
    assert int(hit.sum()) >= 12 and float(a["rgb"][hit].min()) > 0.0 and float(a["rgb"][hit].max()) < 1.0
    cot = (2 * scale * (a["rgb"] - target), torch.zeros(R, dtype=torch.float64))
    b = P.reference(cfg, p, o, d, S, cot, ray_only=True)
    assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["opacity"], b["opacity"])
    assert float(a["g_o"].abs().max()) > 0 and float(a["g_d"].abs().max()) > 0
    for k in ("g_o", "g_d"):
        assert float((a[k] - b[k]).abs().max()) <= 1e-13 * float(b[k].abs().max()), k
    assert torch.allclose(a["sqerr"], ((a["rgb"] - target) ** 2).sum(-1), rtol=0, atol=1e-15)
    assert abs(float(a["loss"]) - scale * float(a["sqerr"].sum())) <= 1e-15


def test_fused_scratch_decoder_returns_what_was_put_in():
    """a workspace filled by hand from the layout query's numbers: 9 rays of a blender scene at S = 70 (Sp = 128: two
    workgroups, ray 8 alone in the second), among them a ray with 0 shaded samples and one with 33 (a second tile block)"""
    from tests.test_host_logic import _fused_scene
    S, R, hid = 70, 9, 64
    lay = P.fused_layout(_fused_scene("blender", S), R)
    assert lay["Sp"] == 128 and lay["blocks"] == 2
    g = torch.Generator().manual_seed(0)
    counts = [0, 33, 1, 32, 31, 5, 0, 64, 3]
    ws = torch.randint(-2 ** 31, 2 ** 31 - 1, (lay["head"] + 16 * lay["slot"],), generator=g, dtype=torch.int64).to(torch.int32)
    mask = torch.zeros(R, S, dtype=torch.bool)
    signs = [[], []]
    for r, n in enumerate(counts):
        b, w = r % lay["blocks"], r // lay["blocks"]          # ray = w * blocks + b in a launch of one round
        base = lay["head"] + (b * lay["waves"] + w) * lay["slot"]
        pick = torch.randperm(S, generator=g)[:n].sort().values
        mask[r, pick] = True
        rank = torch.full((lay["Sp"],), -1, dtype=torch.int32)
        rank[pick] = torch.arange(n, dtype=torch.int32)
        ws[base + 5 * lay["Sp"]:base + 6 * lay["Sp"]] = rank
        for layer in range(2):
            m = torch.rand(n, hid, generator=g) < 0.5
            signs[layer].append(m)
            for e in range(n):
                for h in range(2):
                    word = 0
                    for mt in range(hid // 32):
                        for rr in range(16):
                            if bool(m[e, mt * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * h]):
                                word |= 1 << (mt * 16 + rr)
                    word = word - (1 << 32) if word >= 1 << 31 else word
                    ws[base + 6 * lay["Sp"] + (e // 32) * lay["tile_rows"] * 32 + (lay["row_sign"] + 2 * layer + h) * 32 + e % 32] = word
    got_mask, got_relu, count = P.decode_fused_scratch(ws, lay, R, S, hid)
    assert torch.equal(got_mask, mask) and count.tolist() == counts
    for layer in range(2):
        assert torch.equal(got_relu[layer], torch.cat(signs[layer])), layer
    # the slots of a second round are those of the first
    lay2 = dict(lay, blocks=256)
    assert torch.equal(P.fused_slot_of(lay2, 2057)[2048:], P.fused_slot_of(lay2, 2057)[:9])
    assert P.fused_slot_of(lay2, 2057)[:9].tolist() == [8 * b for b in range(9)] and int(P.fused_slot_of(lay2, 2057)[256]) == 1
