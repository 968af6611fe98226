"""The loss-head kernels (jt_loss.hip) on every launch path, held to the float64 oracle with bounds that are derived, not
measured: the photometric loss and its gradient, its per-view form, the weighted sum and the finiteness guard.

Launch arithmetic the rows rest on (n = 3 B r colours).  The three forward kernels share ONE walk (walk_sums<U> in
jt_loss.hip): a thread takes first, first + stride, ... in that order, fetched U at a time with 32-bit indices, so a trip of
the walk covers U x stride colours; a fetch past n is clamped to n - 1 and must not be summed.  U = 8 where one workgroup
walks a whole batch (k_render_loss_fwd_one, k_render_loss_fwd<8> in deterministic mode), U = 1 where a thread owns a few
colours (k_render_loss_fwd<1> under the full grid, the per-view kernel); the sums do not depend on U.
  n <= 32 768   k_render_loss_fwd_one: ONE workgroup of 1 024 threads, first = thread, stride = 1 024, a trip covers 8 192
                colours: n = 3 (one live thread), 1 023 | 1 026 (the second element of thread 0 and 1), 8 190 | 8 193 (a
                second eight-deep trip for thread 0 alone: seven of its eight fetches are clamped), 32 766 (four trips, the
                last single-workgroup n).
  n > 32 768    k_loss_zero, k_render_loss_fwd<1> (min(ceil(n / 256), 512) workgroups of 256, first = global thread, stride
                = the grid, one colour per trip, atomic adds of the four sums), k_render_loss_final: n = 32 769 is 129
                workgroups and every live thread makes one trip; the grid is full at 512 x 256 = 131 072 threads, where
                n = 131 076 sends four threads on a grid-stride second trip -- in k_render_loss_bwd as well, which has the
                same grid at every n.  In deterministic mode k_render_loss_fwd<8> runs as ONE workgroup: stride = 256, an
                eight-deep trip covers 2 048 colours, 17 trips at n = 32 769 (thread 0 sums 129 elements, one in its
                last trip, whose other seven fetches are clamped) and 65 at n = 131 076.
  per view      k_render_loss_views_fwd: one 1 024-thread workgroup per view running k_render_loss_fwd_one's body, one
                colour per trip, on that view's colours (a view of 10 923 rays: 33 trips, the last for thread 0 alone; an
                empty view: none);
                k_render_loss_views_bwd finds a colour's view by bisection over the offsets (ragged_view) and forms the
                gradient with k_render_loss_bwd's function.
  guard         k_finite_check: min(ceil(max n / 256), 256) workgroups of 256: 65 536 elements fill the grid, 65 537 sends
                thread 0 on a second trip.

Exact inputs.  Colours and image values lie on the lattice k / 8 (k = 0 .. 8), masks in {0, 1}: every difference is a
multiple of 1/8, every squared term a multiple of 1/64 and at most 1, so every partial sum is an integer multiple of 1/64
below 2^18 for n <= 262 144 -- EXACT in fp32 in any summation order.  A lost, doubled or misplaced element moves a sum by at
least 1/64 and cannot hide in rounding.  What remains is rounded: one division for the unmasked loss
(|L - L64| <= 2^-23 |L64|); two divisions, two products and an add for the masked one (2^-21); a division, the products
with the weight, the mask, the difference and the upstream gradient for a gradient element (2^-20 |t|, and exactly 0 where
the reference is 0).  These bounds are derived; a failing element is reported, the bound is not widened."""
import re

import pytest
import torch

from oracle import tensorf_oracle as O
from tests import camera_ref as C
from tests import pinned_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
IH, IW = 96, 128                      # 12 288 pixels: room for 10 923 rays per view
FE, FNE, UP = 1.5, 0.5, 0.7           # edge / non-edge weights, upstream gradient
TOL_L, TOL_LM, TOL_G = 2.0 ** -23, 2.0 ** -21, 2.0 ** -20

# (B, r): n = 3 B r
SHAPES = [(1, 1), (1, 341), (1, 342), (2, 1365), (1, 2731), (2, 5461), (3, 3641), (4, 10923)]
_MEMO = {}


def _base_names(names):
    """device kernel names without namespace, template and argument lists: {"k_render_loss_fwd", ...}"""
    return {(re.split(r"[(<]", n)[0].split() or [""])[-1].split("::")[-1] for n in names}


def _lattice(shape, g):
    return torch.randint(0, 9, shape, generator=g).float() / 8.0


def _inputs(B, r, lattice=True, seed=0):
    """(rgb [B,r,3], image [B,3,IH,IW], ray_idx [r] with repeats, mask [B, IH IW] u8) on the CPU"""
    g = torch.Generator().manual_seed(7 + 100 * B + r + seed)
    draw = (lambda s: _lattice(s, g)) if lattice else (lambda s: torch.rand(s, generator=g))
    rgb, image = draw((B, r, 3)), draw((B, 3, IH, IW))
    ray_idx = torch.randint(0, IH * IW, (r,), generator=g)
    mask = (torch.rand(B, IH * IW, generator=g) < 0.4).to(torch.uint8)
    return rgb, image, ray_idx, mask


def _reference(rgb, image, ray_idx, mask, masked, up=UP):
    """the oracle in float64: (loss, g_rgb)"""
    B = rgb.shape[0]
    a = rgb.double().requires_grad_(True)
    img_at = image.double().view(B, 3, -1).permute(0, 2, 1)[:, ray_idx]
    ref = O.render_loss(a, img_at, mask[:, ray_idx] if masked else None, FE, FNE)
    (ref * up).backward()
    return ref.detach(), a.grad.detach()


def _case(B, r, masked):
    """inputs and the fp64 reference of a lattice shape, computed once and shared (never modified)"""
    key = (B, r, masked)
    if key not in _MEMO:
        rgb, image, ray_idx, mask = _inputs(B, r)
        assert float((rgb - image.view(B, 3, -1).permute(0, 2, 1)[:, ray_idx]).abs().max()) > 0   # not all zero
        _MEMO[key] = (rgb, image, ray_idx, mask) + _reference(rgb, image, ray_idx, mask, masked)
    return _MEMO[key]


def _run(ops, rgb, image, ray_idx, mask, masked, up=UP, profile=False):
    """ops.render_loss forward + backward under the guard band: (loss, g_rgb, device kernel names or None)"""
    a = rgb.to(DEV).requires_grad_(True)
    img, idx, m = image.to(DEV), ray_idx.to(DEV), (mask.to(DEV) if masked else None)

    def step():
        a.grad = None
        with P.guard_band() as guard:
            out = ops.render_loss(a, img, idx, m, FE, FNE)
            (out * up).backward()
            torch.cuda.synchronize()
        assert guard.violations() == []
        return out.detach()
    names = None
    if profile:
        from torch.profiler import ProfilerActivity, profile as tprofile
        for _ in range(2):                        # (the profiler has been seen to hand back a trace without this library's
            with tprofile(activities=[ProfilerActivity.CUDA]) as prof:      # kernels: the same step is then recorded once more)
                out = step()
            names = _base_names(P._device_kernel_names(prof))
            if "k_render_loss_bwd" in names:
                break
    else:
        out = step()
    return out, a.grad.detach().clone(), names


def _judge(loss, g, L64, T, masked, what):
    """the derived bounds of the module docstring, element by element; the offending element is reported"""
    tol = TOL_LM if masked else TOL_L
    err = abs(float(loss.double()) - float(L64))
    assert err <= tol * abs(float(L64)), "%s: loss %r vs %r (rel %.3g, bound %.3g)" % (what, float(loss), float(L64),
                                                                                        err / abs(float(L64)), tol)
    g = g.double().cpu()
    bad = ((g - T).abs() > TOL_G * T.abs()).flatten()     # (where T == 0 this asks for exactly 0)
    if bool(bad.any()):
        k = int(bad.nonzero()[0])
        raise AssertionError("%s: g_rgb element %d of %d: %r vs %r (%d elements off)" % (
            what, k, g.numel(), float(g.flatten()[k]), float(T.flatten()[k]), int(bad.sum())))
    rel = ((g - T).abs() / T.abs().clamp_min(1e-300))[T != 0]
    return err / abs(float(L64)), float(rel.max()) if rel.numel() else 0.0


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("B,r", SHAPES)
def test_render_loss_shapes(B, r, masked):
    from joint_tensorf_amd import ops
    rgb, image, ray_idx, mask, L64, T = _case(B, r, masked)
    n = 3 * B * r
    out, g, names = _run(ops, rgb, image, ray_idx, mask, masked, profile=n >= 32766)
    el, eg = _judge(out, g, L64, T, masked, "n=%d" % n)
    print("render_loss n=%d masked=%d: loss rel %.3g  worst g_rgb rel %.3g" % (n, masked, el, eg))
    if names is not None:
        multi = {"k_loss_zero", "k_render_loss_fwd", "k_render_loss_final"}
        assert "k_render_loss_bwd" in names, sorted(names)
        if n > 32768:
            assert multi <= names and "k_render_loss_fwd_one" not in names, sorted(names)
        else:
            assert "k_render_loss_fwd_one" in names and not (multi & names), sorted(names)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("B,r", [(3, 3641), (4, 10923)])
def test_render_loss_deterministic(B, r, masked):
    """Deterministic mode runs k_render_loss_fwd as one workgroup: same bounds, two runs bit-identical.  On the lattice the
    non-deterministic run equals them bit for bit as well: every partial sum of the four accumulators is exact in fp32
    (module docstring), so the order of the atomic adds cannot change acc, and k_render_loss_final / k_render_loss_bwd
    compute from the same acc with the same instructions."""
    from joint_tensorf_amd import ops
    from joint_tensorf_amd._lib import lib
    rgb, image, ray_idx, mask, L64, T = _case(B, r, masked)
    free, g_free, _ = _run(ops, rgb, image, ray_idx, mask, masked)
    prev = lib.jt_set_deterministic(1)
    try:
        d1, g1, _ = _run(ops, rgb, image, ray_idx, mask, masked)
        d2, g2, _ = _run(ops, rgb, image, ray_idx, mask, masked)
    finally:
        lib.jt_set_deterministic(prev)
    _judge(d1, g1, L64, T, masked, "deterministic n=%d" % (3 * B * r))
    assert torch.equal(d1, d2) and torch.equal(g1, g2)
    assert torch.equal(d1, free) and torch.equal(g1, g_free)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("B,r", [(2, 5461), (3, 3641)])
def test_render_loss_indirect_entry_points(B, r, masked):
    """jt_render_loss_*_ind read the image / mask addresses from device memory (as under graph capture): bit for bit the
    direct entry points, on both sides of the 32 768 edge"""
    from joint_tensorf_amd import ops
    rgb, image, ray_idx, mask, L64, T = _case(B, r, masked)
    direct, g_direct, _ = _run(ops, rgb, image, ray_idx, mask, masked)
    img, m = image.to(DEV).contiguous(), mask.to(DEV).contiguous()      # the kernel's layout: fp32 [B,3,HW], u8 [B,HW]
    slots = torch.tensor([img.data_ptr(), m.data_ptr()], dtype=torch.int64, device=DEV)
    a = rgb.to(DEV).requires_grad_(True)
    assert ops.SUPERVISION_SLOTS_STATIC is None
    ops.SUPERVISION_SLOTS_STATIC = slots
    try:
        with P.guard_band() as guard:
            out = ops.render_loss(a, img, ray_idx.to(DEV), m if masked else None, FE, FNE)
            (out * UP).backward()
            torch.cuda.synchronize()
    finally:
        ops.SUPERVISION_SLOTS_STATIC = None
    assert guard.violations() == []
    _judge(out.detach(), a.grad, L64, T, masked, "indirect n=%d" % (3 * B * r))
    assert torch.equal(out.detach(), direct) and torch.equal(a.grad, g_direct)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("B,r", [(2, 5461), (3, 3641)])
def test_render_loss_nan_colours(B, r, masked):
    """The nanmean rule on a general random input with three NaN colours: one under mask 1, one under mask 0, one the last
    element.  The loss is the oracle's nanmean; every gradient element of a finite colour is the oracle's.  AT a NaN colour
    the two differ on purpose: torch's nanmean backward gives NaN there (0 x 2 NaN), k_render_loss_bwd writes g x 0 = 0 --
    the element is excluded from the mean, so it gets no gradient, and a NaN colour (which the finiteness guard reports,
    FINITE_RENDER) does not poison every parameter before the host reads the status word."""
    from joint_tensorf_amd import ops
    rgb, image, ray_idx, mask = _inputs(B, r, lattice=False, seed=1)
    pix = ray_idx.clone()
    mask[0, pix[5]], mask[B - 1, pix[7]], mask[B - 1, pix[r - 1]] = 1, 0, 1
    assert int(pix[7]) != int(pix[r - 1])                  # (view B - 1 holds one NaN under mask 0 and one under mask 1)
    spots = [(0, 5, 1), (B - 1, 7, 0), (B - 1, r - 1, 2)]
    for b, k, ch in spots:
        rgb[b, k, ch] = float("nan")
    assert bool(torch.isnan(rgb.flatten()[-1]))
    L64, T = _reference(rgb, image, ray_idx, mask, masked)
    out, g, _ = _run(ops, rgb, image, ray_idx, mask, masked)
    assert abs(float(out) - float(L64)) <= 1e-6 * abs(float(L64)), (float(out), float(L64))
    g = g.double().cpu()
    nan = torch.isnan(rgb)
    assert int(nan.sum()) == 3 and bool(torch.isnan(T[nan]).all()) and not bool(torch.isnan(T[~nan]).any())
    assert bool((g[nan] == 0).all())                       # what the kernel writes: g x 0
    bad = (g - T).abs()[~nan] > TOL_G * T.abs()[~nan]      # (seven roundings, each relative to the element: < 2^-21)
    assert not bool(bad.any()), (int(bad.sum()), float(((g - T).abs()[~nan] / T.abs()[~nan].clamp_min(1e-300)).max()))


@pytest.mark.parametrize("B,r", [(1, 342), (3, 3641)])
def test_render_loss_counts_of_the_two_means_differ(B, r):
    """The edge and the non-edge mean each divide by their OWN count of non-NaN terms (acc[1], acc[3]).  A NaN colour leaves
    both (m NaN and (1 - m) NaN are NaN); an infinite colour under mask 0 leaves only the edge mean (0 x Inf = NaN, 1 x Inf =
    Inf), so here acc[1] = n - 1 and acc[3] = n: the loss is +Inf as the oracle's, and every other gradient element must
    carry its own mean's count -- they differ by 1 / n, against a bound of 2^-20."""
    from joint_tensorf_amd import ops
    rgb, image, ray_idx, mask = _inputs(B, r)
    mask[0, ray_idx[3]] = 0
    rgb[0, 3, 1] = float("inf")
    L64, T = _reference(rgb, image, ray_idx, mask, True)
    out, g, _ = _run(ops, rgb, image, ray_idx, mask, True)
    assert float(L64) == float("inf") and float(out) == float("inf")
    g = g.double().cpu()
    rest = torch.isfinite(rgb)
    assert bool(torch.isfinite(T[rest]).all()) and not bool(torch.isfinite(g[~rest]).any())
    bad = (g - T).abs()[rest] > TOL_G * T.abs()[rest]
    assert not bool(bad.any()), (int(bad.sum()), float(((g - T).abs()[rest] / T.abs()[rest].clamp_min(1e-300)).max()))
    assert int((mask[:, ray_idx] == 1).sum()) > 0 and int((mask[:, ray_idx] == 0).sum()) > 1


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("B,r", [(1, 342), (3, 3641)])
def test_render_loss_all_nan_is_nan(B, r, masked):
    """nanmean of an all-NaN tensor is NaN (0 / 0), as in torch, on both forward paths"""
    from joint_tensorf_amd import ops
    rgb, image, ray_idx, mask = _inputs(B, r)
    rgb = torch.full_like(rgb, float("nan"))
    out, g, _ = _run(ops, rgb, image, ray_idx, mask, masked)
    assert bool(torch.isnan(out))
    assert bool(torch.isnan(_reference(rgb, image, ray_idx, mask, masked)[0]))


# ---- per-view loss ---------------------------------------------------------------------------------------------------
def _views_inputs(sizes, lattice, seed=0):
    V, n = len(sizes), sum(sizes)
    g = torch.Generator().manual_seed(99 + seed + n)
    draw = (lambda s: _lattice(s, g)) if lattice else (lambda s: torch.rand(s, generator=g))
    rgb, image = draw((n, 3)), draw((V, 3, IH, IW))
    ray_idx = torch.randint(0, IH * IW, (n,), generator=g)
    up = 0.3 + torch.arange(V).float() * 0.17           # a distinct upstream gradient per view
    return rgb, image, ray_idx, C.ragged_offsets(sizes), up


def _run_views(ops, rgb, image, ray_idx, voff, up):
    a = rgb.to(DEV).requires_grad_(True)
    with P.guard_band() as guard:
        loss = ops.render_loss_views(a, image.to(DEV), ray_idx.to(DEV), voff.to(DEV))
        loss.backward(up.to(DEV))
        torch.cuda.synchronize()
    assert guard.violations() == []
    return loss.detach(), a.grad.detach()


@pytest.mark.parametrize("lattice", [True, False], ids=["lattice", "random"])
def test_render_loss_views_ragged(lattice):
    """Empty first, middle and last views, one ray, 256, 257 and 1 025 rays.  Each view's loss and every gradient element by
    the derived bounds (lattice inputs; on the random input the loss to 1e-6, as summation order now matters); an empty
    view's loss is NaN (0 / 0) and touches nothing else; and the written claim: ops.render_loss on a view alone (3 r <=
    32 768: k_render_loss_fwd_one, the same summation structure) gives a bit-identical loss and gradient -- on the random
    input too, where a different order would show."""
    from joint_tensorf_amd import ops
    rgb, image, ray_idx, voff, up = _views_inputs(C.RAGGED_SIZES, lattice)
    loss, g = _run_views(ops, rgb, image, ray_idx, voff, up)
    for b, a, e in C.ragged_views(voff):
        if a == e:
            assert bool(torch.isnan(loss[b])), b
            continue
        L64, T = _reference(rgb[None, a:e], image[b:b + 1], ray_idx[a:e], None, False, up=float(up[b]))
        if lattice:
            _judge(loss[b], g[a:e][None], L64, T, False, "view %d" % b)
        else:
            assert abs(float(loss[b]) - float(L64)) <= 1e-6 * float(L64), b
            assert bool(((g[a:e][None].double().cpu() - T).abs() <= TOL_G * T.abs()).all()), b
        one, g_one, _ = _run(ops, rgb[None, a:e], image[b:b + 1], ray_idx[a:e], None, False, up=float(up[b]))
        assert torch.equal(one, loss[b]), (b, float(one), float(loss[b]))
        assert torch.equal(g_one[0], g[a:e]), b
    assert not bool(torch.isnan(g).any())


def test_render_loss_views_past_the_single_workgroup_size():
    """A view of 10 923 rays (3 r = 32 769 > 32 768) between two small ones, and an all-NaN view: judged by the bounds only --
    the bit-for-bit claim ends at 3 r = 32 768, where the single-view op switches to k_render_loss_fwd."""
    from joint_tensorf_amd import ops
    sizes = (5, 10923, 3, 2)
    rgb, image, ray_idx, voff, up = _views_inputs(sizes, True)
    rgb[voff[2]:voff[3]] = float("nan")            # view 2: every colour NaN
    loss, g = _run_views(ops, rgb, image, ray_idx, voff, up)
    for b, a, e in C.ragged_views(voff):
        if b == 2:
            assert bool(torch.isnan(loss[b])) and bool((g[a:e] == 0).all())
            continue
        L64, T = _reference(rgb[None, a:e], image[b:b + 1], ray_idx[a:e], None, False, up=float(up[b]))
        _judge(loss[b], g[a:e][None], L64, T, False, "view %d" % b)


# ---- weighted sum ----------------------------------------------------------------------------------------------------
NANF = float("nan")
# (render, reg3, (w_render, w_l1, w_tv_density, w_tv_color), total is NaN)
SUM_CASES = {
    "all-nonzero": (0.0371, (2.25, 0.0119, 0.683), (1.0, 8e-5, 0.1, 0.01), False),
    "zero-tv-color-nan": (0.0371, (2.25, 0.0119, NANF), (1.0, 8e-5, 0.1, 0.0), False),
    "zero-render-nan": (NANF, (2.25, 0.0119, 0.683), (0.0, 8e-5, 0.1, 0.01), False),
    "zero-l1-nan": (0.0371, (NANF, 0.0119, 0.683), (1.0, 0.0, 0.1, 0.01), True),   # the L1 term is always added
}


def _loss_sum(ops, render, reg3, w, form, up=UP):
    r = torch.tensor(render, device=DEV).requires_grad_(True)
    q = torch.tensor(reg3, device=DEV).requires_grad_(True)
    finite = torch.ones(5, device=DEV)
    kw = dict(check_items=[(finite, ops.FINITE_POSE)], loss_bit=ops.FINITE_LOSS) if form == "check" else {}
    assert ops.LOSS_WEIGHTS_STATIC is None
    if form == "dyn":
        ops.LOSS_WEIGHTS_STATIC = torch.tensor(w, device=DEV, dtype=torch.float32)
    try:
        with P.guard_band() as guard:
            total = ops.loss_sum(r, q, *w, **kw)
            (total * up).backward()
            torch.cuda.synchronize()
    finally:
        ops.LOSS_WEIGHTS_STATIC = None
    assert guard.violations() == []
    return total.detach(), r.grad.detach(), q.grad.detach()


@pytest.mark.parametrize("case", list(SUM_CASES))
def test_loss_sum_forms(case):
    """by value, weights in device memory, and with the finiteness guard in the same launch: bit-identical totals, the
    fp64 sum to 4 x 2^-24 of the sum of absolute terms (four products, three adds), gradients exactly g w; a zero-weight
    term does not enter the sum (a NaN there does not spread), except the L1 term, which is always added."""
    from joint_tensorf_amd import ops
    render, reg3, w, is_nan = SUM_CASES[case]
    ops.read_status(DEV)                                  # start from a clear status word
    got = {}
    for form in ("value", "dyn", "check"):
        got[form] = _loss_sum(ops, render, reg3, w, form)
        status = ops.read_status(DEV)
        assert status == (ops.FINITE_LOSS if (is_nan and form == "check") else 0), (form, status)
    w32 = torch.tensor(w, dtype=torch.float32)
    x32 = torch.tensor((render,) + tuple(reg3), dtype=torch.float32)
    terms = [w32[k].double() * x32[k].double() for k in range(4) if (k == 1 or float(w32[k]) != 0.0)]
    ref, mag = sum(terms), sum(t.abs() for t in terms)
    g_ref = torch.tensor(UP, dtype=torch.float32) * w32              # one fp32 product per element: exact to compare
    for form, (total, g_r, g_q) in got.items():
        assert torch.equal(total.cpu().view(1).view(torch.int32), got["value"][0].cpu().view(1).view(torch.int32)), form
        if is_nan:
            assert bool(torch.isnan(total)), form
        else:
            assert abs(float(total.double()) - float(ref)) <= 4 * C.EPS32 * float(mag), (form, float(total), float(ref))
        assert torch.equal(g_r.cpu().view(1), g_ref[:1]) and torch.equal(g_q.cpu(), g_ref[1:]), form


def test_loss_sum_reuses_the_unit_seed_products():
    """LossSum._last: behind a registered unit seed the backward's products are the weights; a second backward with the same
    weights returns the remembered tensors, a third with other weights must not"""
    from joint_tensorf_amd import ops
    seed = ops.register_unit_seed(torch.ones((), device=DEV))
    keep = ops.LossSum._last
    ops.LossSum._last = None

    def step(w):
        r = torch.tensor(0.04, device=DEV).requires_grad_(True)
        q = torch.tensor([2.0, 0.01, 0.5], device=DEV).requires_grad_(True)
        ops.backward(ops.loss_sum(r, q, *w), gradient=seed)
        return torch.cat([r.grad.view(1), q.grad]).cpu()
    try:
        w1, w2 = (1.0, 8e-5, 0.1, 0.01), (0.5, 8e-5, 0.05, 0.01)
        a = step(w1)
        assert ops.LossSum._last is not None and ops.LossSum._last[0][0] == w1
        held = ops.LossSum._last[1]
        b = step(w1)
        assert ops.LossSum._last[1] is held               # the second pass launched nothing
        c = step(w2)
        assert torch.equal(a, torch.tensor(w1)) and torch.equal(b, a)
        assert torch.equal(c, torch.tensor(w2)) and ops.LossSum._last[0][0] == w2
    finally:
        ops.LossSum._last = keep
        ops.UNIT_SEEDS.pop(id(seed), None)


# ---- finiteness guard ------------------------------------------------------------------------------------------------
def test_finite_check_bits():
    """Three tensors of 1, 65 536 and 65 537 elements (the last: a grid-stride second trip at 256 x 256 threads), the middle
    one non-contiguous, each with its own bit.  Clean: the word stays 0, also with the largest finite float.  One +Inf, -Inf
    or NaN at the first, the last or element 65 536: exactly the owning tensor's bit, and the read clears the word."""
    from joint_tensorf_amd import ops
    big = torch.finfo(torch.float32).max
    g = torch.Generator().manual_seed(2)
    t0 = torch.randn(1, generator=g).to(DEV)
    wide = torch.randn(65536, 2, generator=g).to(DEV)
    t1 = wide[:, 0]                                        # stride 2: finite_check checks a contiguous copy
    t2 = torch.randn(65537, generator=g).to(DEV)
    assert not t1.is_contiguous()
    wide[:, 1] = float("nan")                              # the elements between t1's must not be looked at
    tensors, bits = [t0, t1, t2], [ops.FINITE_POSE, ops.FINITE_RENDER, ops.FINITE_GRAD]
    items = list(zip(tensors, bits))
    ops.read_status(DEV)
    ops.finite_check(items)
    assert ops.read_status(DEV) == 0
    t0[0], t1[65535], t2[65536] = big, -big, big
    ops.finite_check(items)
    assert ops.read_status(DEV) == 0
    spots = [(0, 0), (1, 0), (1, 65535), (2, 0), (2, 65535), (2, 65536)]
    for k, (which, at) in enumerate(spots):
        for bad in (float("inf"), float("-inf"), float("nan")):
            t = tensors[which]
            old = t[at].clone()
            t[at] = bad
            ops.finite_check(items)
            t[at] = old
            assert ops.read_status(DEV) == bits[which], (which, at, bad)
            assert ops.read_status(DEV) == 0               # cleared by the read
    ops.finite_check(items)
    assert ops.read_status(DEV) == 0
