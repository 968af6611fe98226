"""Float64 closed forms of the regularisers (csrc/jt_reg.hip) on channel-last [H][W][C] arrays, a pure mirror of the
kernels' launch arithmetic, and the element-wise judges of tests/test_gpu_reg_paths.py.  Checked without a GPU by
tests/test_reg_ref.py: the closed forms against autograd through the oracle, the mirror's constants against the source.

Everything is written with slices and no autograd: a 25 M-element tensor costs about a second on the CPU.

The gradient of  c0 sum|x| + c1 sum (x[y+1] - x[y])^2 + c2 sum (x[., x+1] - x[., x])^2  at an element is
    c0 sign(x) + 2 c1 A + 2 c2 B,   A = [y > 0] (x - up) - [y + 1 < H] (down - x),   B likewise along W,
with sign(0) = 0 (torch's abs backward, and reg_texel's (v > 0) - (v < 0))."""
import functools

import torch

EPS32 = 2.0 ** -24

# ---- the launch arithmetic of jt_reg.hip (tests/test_reg_ref.py reads the same numbers out of the source) -----------------------
REG_SEG = 16          # kRegSeg: rows a thread of the row walk takes
REG_SHARDS = 16       # kRegShards: copies of the 36 sums the batched kernels add into
THREADS = 256
# entry -> (workgroup cap with TV, without); the backward's grid does not depend on TV, the per-tensor forward is always TV
CAPS = {"factor_fwd": (1024, None), "factor_bwd": (2048, 2048), "batch_fwd": (512, 128), "batch_bwd": (2048, 2048),
        "fused": (1024, 256)}


def launch_shape(entry, H, W, C, tv, deterministic=False):
    """(form, workgroups, items, max_trips) of one tensor in `entry`'s launch.  tv: the kernel's TV switch -- the template
    argument of reg_body -- the item's flag in the forward and fused kernels, "a TV coefficient is non-zero" in the
    backward.  form "walk": a thread takes (segment of REG_SEG rows, column, quad) items, "general": one quad per item.
    max_trips: the most iterations any thread's grid-stride loop makes.  Deterministic mode changes the batched forward alone
    (one workgroup per tensor); the fused entry point refuses it."""
    assert C % 4 == 0 and H >= 1 and W >= 1
    cap = CAPS[entry][0 if tv else 1]
    if cap is None:
        raise ValueError("%s has no launch without TV" % entry)
    if deterministic and entry == "fused":
        raise ValueError("jt_reg_losses_fused is unsupported in deterministic mode")
    quads = H * W * (C // 4)
    wgs = min((quads + THREADS - 1) // THREADS, cap)
    if deterministic and entry == "batch_fwd":
        wgs = 1
    walk = bool(tv) and H >= 2 * REG_SEG
    items = ((H + REG_SEG - 1) // REG_SEG) * W * (C // 4) if walk else quads
    return ("walk" if walk else "general"), wgs, items, (items + wgs * THREADS - 1) // (wgs * THREADS)


@functools.lru_cache(maxsize=None)
def smallest_second_trip(entry, H, C, tv=True, extra_threads=8):
    """the smallest W at which `entry`'s launch of an [H][W][C] tensor sends at least `extra_threads` threads round their
    loop a second time (and no thread a third time)"""
    cap = CAPS[entry][0 if tv else 1]
    W = 1
    while True:
        _, wgs, items, _ = launch_shape(entry, H, W, C, tv)
        if wgs == cap and items >= cap * THREADS + extra_threads:
            assert items <= 2 * cap * THREADS
            return W
        W += 1


# ---- values ----------------------------------------------------------------------------------------------------------------------
def raw_sums(x):
    """(sum|x|, sum of squared vertical differences, of squared horizontal ones) of x [H][W][C], float64"""
    x = x.double()
    s0 = float(x.abs().sum())
    s1 = float(((x[1:] - x[:-1]) ** 2).sum()) if x.shape[0] > 1 else 0.0
    s2 = float(((x[:, 1:] - x[:, :-1]) ** 2).sum()) if x.shape[1] > 1 else 0.0
    return s0, s1, s2


def tv_value(x, sums=None):
    """the oracle's tv_loss(plane) * 1e-2 of a channel-last plane: 2 (s1 / (C (H - 1) W) + s2 / (C H (W - 1))) 1e-2, a
    direction with a single row / column left out"""
    H, W, C = x.shape
    _, s1, s2 = raw_sums(x) if sums is None else sums
    t = 0.0
    if H > 1:
        t += s1 / (C * (H - 1) * W)
    if W > 1:
        t += s2 / (C * H * (W - 1))
    return 2 * t * 1e-2


def scene_values(density_plane, density_line, app_plane, tv_density=True, tv_app=True, sums=None):
    """(L1, TV_density, TV_color) as oracle.density_L1 / tv_planes give them (a term that is switched off is 0).  Every
    addend is non-negative, so each value is also the sum of its positive terms.  sums: raw_sums of the nine tensors, if the
    caller has them."""
    ts = list(density_plane) + list(density_line) + list(app_plane)
    sums = [raw_sums(t) for t in ts] if sums is None else sums
    l1 = sum(sums[i][0] / ts[i].numel() for i in range(6))
    tvd = sum(tv_value(ts[i], sums[i]) for i in range(3)) if tv_density else 0.0
    tva = sum(tv_value(ts[i], sums[i]) for i in range(6, 9)) if tv_app else 0.0
    return [l1, tvd, tva]


def scene_coefs(slot, H, W, C, w3, tv_density=True, tv_app=True):
    """(c0, c1, c2) of tensor `slot` (0-2 density planes, 3-5 density lines, 6-8 appearance planes) under the upstream
    gradients w3 = dL/d(L1, TV_density, TV_color), in float64"""
    c0 = w3[0] / (H * W * C) if slot < 6 else 0.0
    c1 = c2 = 0.0
    if (slot < 3 and tv_density) or (slot >= 6 and tv_app):
        wt = w3[1] if slot < 3 else w3[2]
        if H > 1:
            c1 = wt * 2 * 1e-2 / (C * (H - 1) * W)
        if W > 1:
            c2 = wt * 2 * 1e-2 / (C * H * (W - 1))
    return c0, c1, c2


# ---- gradients -------------------------------------------------------------------------------------------------------------------
def _axis_terms(x, dim, absolute):
    """A (dim 0) or B (dim 1) of the module docstring; absolute: |x - up| + |down - x| instead"""
    out = torch.zeros_like(x)
    if x.shape[dim] > 1:
        n = x.shape[dim]
        d = x.narrow(dim, 1, n - 1) - x.narrow(dim, 0, n - 1)
        if absolute:
            d = d.abs()
            out.narrow(dim, 1, n - 1).add_(d)
            out.narrow(dim, 0, n - 1).add_(d)
        else:
            out.narrow(dim, 1, n - 1).add_(d)
            out.narrow(dim, 0, n - 1).sub_(d)
    return out


def reg_grad(x, coef, exact_differences=True):
    """(T, M) of x [H][W][C] under coef = (c0, c1, c2), float64: T the gradient, M = |c0| |sign x| + 2 |c1| |A| + 2 |c2| |B|
    the magnitude of its terms.  exact_differences=False (inputs off the lattice, whose fp32 differences round): |A| and |B|
    are replaced by |x - up| + |down - x| and |x - left| + |right - x|."""
    x = x.double()
    c0, c1, c2 = (float(c) for c in coef)
    s = torch.sign(x)
    T, M = c0 * s, abs(c0) * s.abs()
    del s
    for dim, c in ((0, c1), (1, c2)):
        if c != 0.0:
            t = _axis_terms(x, dim, False)
            T.add_(t, alpha=2 * c)
            M.add_(t.abs_() if exact_differences else _axis_terms(x, dim, True), alpha=2 * abs(c))
    return T, M


# ---- judges ----------------------------------------------------------------------------------------------------------------------
# Gradient element, lattice inputs (A and B exact in fp32).  With u = 2^-24: the coefficient of the L1 term carries one rounded
# division (u); a TV coefficient carries 2e-2f against 2 * 1e-2 (u), a product with the upstream gradient (u, none for a power of
# two) and a division (u): 3 u.  c1 A and c2 B are a rounded product each (4 u of the term), their sum one more (5 u), the factor
# 2 is exact, and the sum with c0 sign(x) rounds once more, relative to a result that is at most |c0| + 2 |c1 A| + 2 |c2 B|:
#   |G - T| <= 2 u |c0| + 6 u (2 |c1 A| + 2 |c2 B|) <= 6 u M      (first order; a fused multiply-add only removes roundings)
# KAPPA_LATTICE = 8 leaves the second-order terms their room.  Off the lattice the two differences of A round (u each, of
# |x - up| and |down - x|) and so does their difference: 2 u more of the absolute-difference magnitude: KAPPA_RANDOM = 10.
KAPPA_LATTICE, KAPPA_RANDOM = 8.0, 10.0
# reg_combine, given exact sums (the integer products of the denominators are exact): a term of L1 goes through its division
# and at most six additions; a TV term through its division, the sum of the two directions, the product with 1e-2f, that
# constant's own rounding and at most two additions: at most 7 roundings each, 8 u of the (non-negative) terms' sum
VALUE_ROUNDINGS = 8


def judge_grad(G, T, M, kappa, what, prior=None):
    """|G - T| <= kappa 2^-24 M element by element, and G == T exactly where M == 0 (T is 0 there).  prior: a gradient the
    kernel added onto (accumulate = 1): G is compared with prior + T, the final addition may round by 2^-24 of the sum where
    M > 0, and an element with M == 0 keeps its prior value exactly.  Runs on G's device; NaN fails.  Returns the worst
    error as a fraction of its bound; raises AssertionError naming the first offending element."""
    dev = G.device
    G, T, M = G.double().reshape(-1), T.to(dev).reshape(-1), M.to(dev).reshape(-1)
    assert G.numel() == T.numel() == M.numel(), (what, G.numel(), T.numel())
    tol = kappa * EPS32 * M
    if prior is not None:
        T = T + prior.to(dev).double().reshape(-1)
        tol = torch.where(M > 0, tol + EPS32 * T.abs(), tol)
    err = (G - T).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        k = int(bad.nonzero()[0])
        raise AssertionError("%s: gradient element %d of %d: %r vs %r, bound %.3g (%d elements off)" % (
            what, k, G.numel(), float(G[k]), float(T[k]), float(tol[k]), int(bad.sum())))
    live = tol > 0
    return float((err[live] / tol[live]).max()) if bool(live.any()) else 0.0


def judge_values(out3, ref3, what, n_addends=None):
    """the batched entry points' (L1, TV_density, TV_color) against scene_values: VALUE_ROUNDINGS x 2^-24 of each value on
    lattice inputs; with n_addends = (n0, n1, n2), the largest number of addends of a tensor's sum in each value, the
    standard worst case of an fp32 sum in any order on top: (n + 3 + VALUE_ROUNDINGS) 2^-24 (3: the difference, the square
    and the quad's own additions).  A value of 0 must be exactly 0."""
    worst = 0.0
    for k in range(3):
        got, ref = float(out3[k]), float(ref3[k])
        n = VALUE_ROUNDINGS + (0 if n_addends is None else n_addends[k] + 3)
        if not abs(got - ref) <= n * EPS32 * ref:
            raise AssertionError("%s: value %d: %r vs %r (off by %.3g of it, bound %.3g)" % (
                what, k, got, ref, abs(got - ref) / max(ref, 1e-300), n * EPS32))
        worst = max(worst, abs(got - ref) / (EPS32 * ref) if ref else 0.0)
    return worst


def judge_sums(out3, sums, what):
    """the per-tensor forward's three raw sums on lattice inputs: exact"""
    got = [float(v) for v in out3]
    if got != [float(s) for s in sums]:
        raise AssertionError("%s: raw sums %r vs %r" % (what, got, list(sums)))


# ---- lattice inputs ----------------------------------------------------------------------------------------------------------------
SUM_LIMIT_ABS, SUM_LIMIT_SQ = 2.0 ** 22, 2.0 ** 20


def lattice(H, W, C, seed):
    """[H][W][C] float32 with values k / 4, k in -2 .. 2, some of the zeros written as -0.0.  Every |x| and every difference
    is a multiple of 1/4, every squared difference a multiple of 1/16 and at most 1.  A tensor too large for its expected
    sums to stay at half the exactness limits (assert_exact) is thinned out with zeros; its last row's last four texels stay
    dense and non-zero (they belong to the last items of the row walk: the threads of a partial last trip)."""
    g = torch.Generator().manual_seed(seed)
    n = H * W * C
    x = torch.randint(-2, 3, (H, W, C), generator=g).float() / 4.0
    # expected sums of the dense draw: 0.3 n of |x|, 0.25 n per direction of squares (2 var = 2 x 0.125)
    keep = min(1.0, (SUM_LIMIT_SQ / 2) / (0.25 * n))
    if keep < 1.0:
        x = x * (torch.rand(H, W, C, generator=g) < keep)
        tail = torch.randint(1, 3, (min(W, 4), C), generator=g).float() / 4.0
        x[H - 1, W - tail.shape[0]:] = tail * (1 - 2 * torch.randint(0, 2, tail.shape, generator=g).float())
    flip = (x == 0) & (torch.rand(H, W, C, generator=g) < 0.25)
    x[flip] = -0.0
    return x


def assert_exact(sums):
    """the exactness limits of a lattice tensor's raw sums: multiples of 1/4 below 2^22 and of 1/16 below 2^20 have at most
    24 significant bits, and so has every partial sum of their non-negative addends, in any order"""
    s0, s1, s2 = sums
    assert s0 < SUM_LIMIT_ABS and s1 < SUM_LIMIT_SQ and s2 < SUM_LIMIT_SQ, sums
    assert s0 * 4 == int(s0 * 4) and s1 * 16 == int(s1 * 16) and s2 * 16 == int(s2 * 16), sums
