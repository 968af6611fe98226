"""tests/reg_ref.py and tests/adam_ref.py checked without a GPU: the closed forms against autograd through the oracle in
float64, the launch mirror against the constants in the sources, the exactness limits of every lattice input the GPU rows
use, and -- once, here, instead of breaking a kernel on the device -- that the judges of tests/test_gpu_reg_paths.py and
tests/test_gpu_adam_edges.py reject what a plausible kernel bug would produce."""
import os
import re

import pytest
import torch

from oracle import tensorf_oracle as O
from tests import adam_ref as A
from tests import reg_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "joint_tensorf_amd", "csrc")
# (H, W, C): single rows and columns, one texel, non-square, on both sides of the row walk's threshold
SHAPES = [(1, 1, 4), (1, 9, 16), (9, 1, 16), (5, 3, 48), (31, 7, 20), (33, 2, 4), (7, 12, 8)]
RTOL = 1e-12   # both sides are float64: the one tolerance here that is not derived


def _logical(x):
    """channel-last [H][W][C] -> the oracle's [1][C][H][W]"""
    return x.permute(2, 0, 1)[None]


def _draw(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _close(a, b, scale=None):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    scale = float(b.abs().max()) if scale is None else scale
    return bool(((a - b).abs() <= RTOL * max(scale, 1e-300)).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_raw_sums_and_gradient_vs_autograd(shape):
    x = _draw(shape, 1)
    x[0, 0, 0] = 0.0                                  # sign(0) = 0
    a = _logical(x).clone().requires_grad_(True)
    ref = torch.stack([a.abs().sum(), ((a[:, :, 1:] - a[:, :, :-1]) ** 2).sum(), ((a[..., 1:] - a[..., :-1]) ** 2).sum()])
    coef = (0.3, 1.7, -0.4)
    (ref * torch.tensor(coef, dtype=torch.float64)).sum().backward()
    assert _close(R.raw_sums(x), ref.detach())
    T, M = R.reg_grad(x, coef)
    want = a.grad[0].permute(1, 2, 0)
    assert _close(T, want) and float(T[0, 0, 0]) == float(want[0, 0, 0])
    assert bool((M >= T.abs() * (1 - 1e-12)).all())
    M2 = R.reg_grad(x, coef, exact_differences=False)[1]
    assert bool((M2 >= M * (1 - 1e-12)).all())
    assert _close(R.tv_value(x), O.tv_loss(_logical(x)) * 1e-2, scale=1.0)


@pytest.mark.parametrize("tv", [(True, True), (False, False), (True, False), (False, True)])
def test_scene_values_and_gradients_vs_oracle(tv):
    """three planes that need not come from one grid (as the batched entry points take them): a general one, a degenerate
    one, a 1 x 1 one; lines of 1, 5 and 12 entries"""
    hw, lines, Cd, Ca = [(31, 7), (1, 9), (1, 1)], [1, 5, 12], 16, 20
    dp = [_draw((h, w, Cd), 10 + i) for i, (h, w) in enumerate(hw)]
    dl = [_draw((n, 1, Cd), 20 + i) for i, n in enumerate(lines)]
    ap = [_draw((h, w, Ca), 30 + i) for i, (h, w) in enumerate(hw)]
    leaves = [_logical(t).clone().requires_grad_(True) for t in dp + dl + ap]
    pp = dict(density_plane=leaves[0:3], density_line=leaves[3:6])
    zero = torch.zeros((), dtype=torch.float64)
    ref = [O.density_L1(pp), O.tv_planes(leaves[0:3]) if tv[0] else zero, O.tv_planes(leaves[6:9]) if tv[1] else zero]
    w3 = (0.37, 1.9, 0.6)
    sum(r * w for r, w in zip(ref, w3)).backward()
    got = R.scene_values(dp, dl, ap, *tv)
    assert _close(got, [float(r.detach()) for r in ref])
    for slot, x in enumerate(dp + dl + ap):
        T, _ = R.reg_grad(x, R.scene_coefs(slot, *x.shape, w3, *tv))
        want = leaves[slot].grad
        want = torch.zeros_like(x) if want is None else want[0].permute(1, 2, 0)
        assert _close(T, want, scale=float(want.abs().max()) or 1.0), slot


# ---- the mirror --------------------------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _entry(src, name):
    """the body of extern "C" int `name`(...) up to the next extern "C\""""
    at = src.index('extern "C" int %s(' % name)
    end = src.find('extern "C"', at + 10)
    return src[at:end if end > 0 else len(src)]


def test_mirror_constants_are_the_sources():
    src = _source("jt_reg.hip")
    assert int(re.search(r"constexpr int kRegSeg = (\d+);", src).group(1)) == R.REG_SEG
    assert int(re.search(r"constexpr int kRegShards = (\d+);", src).group(1)) == R.REG_SHARDS
    assert len(re.findall(r"H >= 2 \* kRegSeg", src)) == 1            # the one loop pair's walk condition
    # the five launches, one per entry point, all of 256 threads; the quad-to-workgroup helper divides by the same number
    launches = re.findall(r"hipLaunchKernelGGL\((\w+)(?:<true>)?, dim3\((?:blocks|nblk)\), dim3\((\d+)\)", src)
    assert len(launches) == src.count("hipLaunchKernelGGL(") == 5 and {t for _, t in launches} == {str(R.THREADS)}
    assert sorted(k for k, _ in launches) == ["k_factor_reg_bwd", "k_factor_reg_fwd", "k_reg_batch_bwd", "k_reg_batch_fused",
                                              "k_reg_batch_fwd"]
    helper = src[src.index("static int reg_blocks("):src.index('extern "C" int jt_factor_reg_forward(')]
    assert "(quads + %d) / %d, kRegCaps[entry][tv ? 0 : 1]" % (R.THREADS - 1, R.THREADS) in helper
    assert src.count("+ 255) / 256") == 1 and "getenv" not in src      # no second cap arithmetic, no override
    # the caps table: one row per entry point, in the enum's order; a cap of 0 stands for "never launched that way"
    rows = re.findall(r"/\* (kReg\w+) \*/ \{(\d+), (\d+)\}", src[src.index("kRegCaps[][2] = {"):src.index("static int reg_blocks(")])
    assert [r[0] for r in rows] == re.search(r"enum RegEntry \{ ([\w, ]+) \};", src).group(1).split(", ")
    caps = {name: (int(tv), int(no) or None) for name, tv, no in rows}
    # the row each entry point asks for its workgroups under
    asks = {"factor_fwd": "jt_factor_reg_forward", "factor_bwd": "jt_factor_reg_backward", "batch_fwd": "jt_reg_losses_forward",
            "batch_bwd": "jt_reg_losses_backward", "fused": "jt_reg_losses_fused"}
    row = {e: re.findall(r"reg_(?:blocks|batch)\((kReg\w+), ", _entry(src, fn)) for e, fn in asks.items()}
    assert all(len(r) == 1 for r in row.values()) and len({r[0] for r in row.values()}) == 5
    assert {e: caps[r[0]] for e, r in row.items()} == R.CAPS
    builder = src[src.index("static int reg_batch("):src.index('extern "C" int jt_reg_losses_forward(')]
    assert "int blocks = reg_blocks(entry, tv, t.H, t.W, t.C);" in builder
    assert "if (entry == kRegBatchFwd && jt_deterministic()) blocks = 1;" in builder
    assert "jt_deterministic()" not in _entry(src, "jt_reg_losses_forward") + _entry(src, "jt_reg_losses_backward")
    fused = _entry(src, "jt_reg_losses_fused")
    assert fused.index("if (jt_deterministic()) return JT_ERR_UNSUPPORTED;") < fused.index("reg_batch(")   # before any write
    opt = _source("jt_optim.hip")
    assert int(re.search(r"constexpr int kAdamMaxItems = (\d+);", opt).group(1)) == A.MAX_ITEMS
    assert re.search(r"constexpr int kAdamElemsPerBlock = 256 \* 4 \* 4;", opt) and A.ELEMS_PER_BLOCK == 4096


def test_launch_shape_by_hand():
    L = R.launch_shape
    assert L("factor_fwd", 31, 7, 20, True) == ("general", 5, 1085, 1)
    assert L("factor_fwd", 32, 1, 4, True) == ("walk", 1, 2, 1)
    assert L("factor_fwd", 49, 2, 16, True) == ("walk", 2, 32, 1)            # segments of 16, 16, 16 and 1 rows
    assert L("factor_bwd", 64, 5, 16, False) == ("general", 5, 1280, 1)      # TV coefficients zero: no walk
    assert L("batch_fwd", 8200, 1, 16, False) == ("general", 128, 32800, 2)  # 32 threads past 128 x 256
    assert L("batch_fwd", 8200, 1, 16, False, deterministic=True) == ("general", 1, 32800, 129)
    assert L("fused", 8200, 1, 16, False) == ("general", 129, 32800, 1)
    with pytest.raises(ValueError):
        L("fused", 4, 4, 4, True, deterministic=True)
    with pytest.raises(ValueError):
        L("factor_fwd", 4, 4, 4, False)
    for entry, H, C in (("factor_fwd", 31, 48), ("factor_bwd", 31, 48), ("factor_fwd", 33, 48), ("factor_bwd", 33, 48),
                        ("batch_fwd", 33, 16), ("fused", 33, 16)):
        W = R.smallest_second_trip(entry, H, C)
        form, wgs, items, trips = L(entry, H, W, C, True)
        assert form == ("walk" if H >= 32 else "general") and trips == 2 and wgs == R.CAPS[entry][0], (entry, H, W)
        assert items - wgs * 256 >= 8 > L(entry, H, W - 1, C, True)[2] - wgs * 256, (entry, H, W)


# ---- the lattice inputs of the GPU rows ----------------------------------------------------------------------------------------
def test_lattice_inputs_are_exact():
    """every lattice tensor of tests/test_gpu_reg_paths.py: its float64 sums are inside the limits under which every fp32
    partial sum is exact, and its values are on the lattice with both zeros present"""
    from tests import test_gpu_reg_paths as G
    seen = 0
    for key in G.lattice_keys():
        x = G.tensor(key)
        assert bool(((x * 4) == (x * 4).round()).all()) and float(x.abs().max()) <= 0.5, key
        if x.numel() >= 256:
            z = x[x == 0]
            assert bool(torch.signbit(z).any()) and not bool(torch.signbit(z).all()), key
        R.assert_exact(G.sums(key))
        seen += 1
    assert seen >= 30


# ---- sensitivity: what the judges must reject ------------------------------------------------------------------------------
def test_judge_rejects_a_dropped_seam_term():
    """the row walk at a segment seam (row 16) forgetting the row above: the vertical term of that row loses x - up"""
    H, W, C = 33, 5, 16
    x = R.lattice(H, W, C, 3)
    coef = R.scene_coefs(0, H, W, C, (1.0, 2.0, 4.0))
    T, M = R.reg_grad(x, coef)
    assert R.judge_grad(T.float(), T, M, R.KAPPA_LATTICE, "clean") <= 1.0      # fp32 rounding of T itself is inside
    d = x[16].double() - x[15].double()
    assert int((d != 0).sum()) > W * C // 2
    one = torch.zeros_like(T)
    k = int((d != 0).flatten().nonzero()[0])
    one[16].view(-1)[k] = d.flatten()[k]
    row = torch.zeros_like(T)
    row[16] = d
    for wrong in (one, row):
        G = (T - 2 * coef[1] * wrong).float()
        with pytest.raises(AssertionError, match="gradient element"):
            R.judge_grad(G, T, M, R.KAPPA_LATTICE, "seam")
    # an element whose terms are all zero must be exactly zero
    zero = int((M == 0).flatten().nonzero()[0]) if bool((M == 0).any()) else None
    if zero is not None:
        G = T.float()
        G.view(-1)[zero] = 1e-30
        with pytest.raises(AssertionError):
            R.judge_grad(G, T, M, R.KAPPA_LATTICE, "stray")
    # a NaN (an element the kernel never wrote, under the tests' fill) fails as well
    G = T.float()
    G.view(-1)[7] = float("nan")
    with pytest.raises(AssertionError):
        R.judge_grad(G, T, M, R.KAPPA_LATTICE, "unwritten")
    # onto a prior gradient: the clean sum passes, the prior dropped at one element does not
    prior = R.lattice(H, W, C, 4)
    R.judge_grad((prior.double() + T).float(), T, M, R.KAPPA_LATTICE, "accumulate", prior=prior)
    G = (prior.double() + T).float()
    k = int((prior != 0).flatten().nonzero()[0])
    G.view(-1)[k] -= prior.view(-1)[k]
    with pytest.raises(AssertionError):
        R.judge_grad(G, T, M, R.KAPPA_LATTICE, "accumulate", prior=prior)


def test_judge_rejects_a_doubled_texel():
    """one texel of the mixed batch's walk plane counted twice: the exact raw sums differ, and the combined values move by
    far more than their eight roundings"""
    from tests import test_gpu_reg_paths as G
    keys = G.batch_keys("mixed20")
    ts = [G.tensor(k) for k in keys[:9]]
    sums = [G.sums(k) for k in keys[:9]]
    ref = R.scene_values(ts[0:3], ts[3:6], ts[6:9], sums=sums)
    R.judge_values(torch.tensor(ref).float(), ref, "clean")
    R.judge_sums(torch.tensor(sums[1]).float(), sums[1], "clean")
    x = ts[1]
    k = int((x != 0).flatten().nonzero()[0])
    more = (sums[1][0] + abs(float(x.flatten()[k])), sums[1][1], sums[1][2])
    with pytest.raises(AssertionError, match="raw sums"):
        R.judge_sums(torch.tensor(more).float(), sums[1], "doubled")
    wrong = R.scene_values(ts[0:3], ts[3:6], ts[6:9], sums=sums[:1] + [more] + sums[2:])
    with pytest.raises(AssertionError, match="value 0"):
        R.judge_values(torch.tensor(wrong).float(), ref, "doubled")
    # a squared difference of 1/16 doubled in the appearance plane's horizontal sum
    sq = (sums[7][0], sums[7][1], sums[7][2] + 1.0 / 16)
    wrong = R.scene_values(ts[0:3], ts[3:6], ts[6:9], sums=sums[:7] + [sq] + sums[8:])
    with pytest.raises(AssertionError, match="value 2"):
        R.judge_values(torch.tensor(wrong).float(), ref, "doubled")


def test_item_schedule_separates_the_launches():
    b1, b2 = 0.9, 0.99
    c = [A.item_coefficients(*A.item_schedule(k), b1, b2) for k in range(65)]
    assert len(set(c)) == 65
    for far in (32, 64):
        for near in (0, 1):
            for j in range(2):
                r = c[far][j] / c[near][j]
                assert r >= 2.0 or r <= 0.5, (far, near, j, r)


def test_judge_rejects_item_0s_step_size_on_item_32():
    """adam_launch offsetting the coefficients of its second launch by `first` instead of 2 * first -- or not at all -- hands
    item 32 another item's step size: every moving element of p leaves its bound; the moments, which do not see it, stay"""
    sc = A.scalars(0.9, 0.99, 1e-8)
    p, g, m, v, idle = A.inputs(A.SIZES[32 % len(A.SIZES)], 32)
    ss0, _ = A.item_coefficients(*A.item_schedule(0), 0.9, 0.99)
    ss, ibc = A.item_coefficients(*A.item_schedule(32), 0.9, 0.99)
    ref, bounds = A.step(p, g, m, v, sc, ss, ibc)
    as32 = tuple(t.float() for t in ref)
    assert max(A.judge(as32, ref, bounds, "clean")) <= 1.0
    wrong, _ = A.step(p, g, m, v, sc, ss0, ibc)
    with pytest.raises(AssertionError, match=r"p\["):
        A.judge(tuple(t.float() for t in wrong), ref, bounds, "item 32")
    off = (wrong[0].float().double() - ref[0]).abs() > bounds[0]
    assert float(off[~idle].float().mean()) > 0.99 and not bool(off[idle].any())
    assert bool((ref[0][idle] == p[idle].double()).all())           # m = g = v = 0: no update at all
    assert bool((bounds[1][idle] == 0).all()) and bool((bounds[2][idle] == 0).all())
