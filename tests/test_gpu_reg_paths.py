"""The five regulariser kernels (csrc/jt_reg.hip) -- every instantiation of the one loop pair reg_body<TV, OUT>, on the row walk
and on the general loop -- held to the float64 closed forms of tests/reg_ref.py element by element, with bounds that are
derived, not measured.

Launch arithmetic (mirrored by reg_ref.launch_shape, whose constants tests/test_reg_ref.py reads out of the source).  A tensor
[H][W][C] has H W C/4 quads and gets min(ceil(quads / 256), cap) workgroups of 256 threads; cap (TV | no TV) is 1 024 for the
per-tensor forward, 2 048 | 2 048 for both backwards, 512 | 128 for the batched forward, 1 024 | 256 for the fused launch.
With TV and H >= 32 the loop pair WALKS: an item is (segment of 16 rows, column, quad), ceil(H / 16) W C/4 of them, and a thread
carries the vertical neighbours through registers from row to row; otherwise the GENERAL loop takes one quad per item.  The
backward walks when a TV coefficient is non-zero.  Both loops are grid-stride: a thread makes ceil(items / (256 workgroups))
trips at most.  In deterministic mode the batched forward runs ONE workgroup per tensor and the fused entry point refuses.
Every row asserts through the mirror the form and the trip count it is there for (the row's id or docstring names them).

Exact inputs.  Factor values lie on the lattice k / 4, k = -2 .. 2, with -0.0 among the zeros: every |x| and every difference
is a multiple of 1/4, every squared difference a multiple of 1/16 and at most 1.  Each tensor's own float64 sums stay below
2^22 (|x|) and 2^20 (squares) -- asserted on the reference, tests/test_reg_ref.py -- so that EVERY fp32 partial sum is exact in
any order (large tensors are thinned out with zeros for that).  The per-tensor forward's raw sums must therefore equal the
reference's exactly: a lost, doubled or misplaced texel moves one by at least 1/16.  Upstream weights are powers of two.

What stays rounded (u = 2^-24; the counts are spelled out beside reg_ref.KAPPA_LATTICE / VALUE_ROUNDINGS):
  * reg_combine: per term a division, the sum of the two directions, the product with 1e-2f, that constant's own rounding and
    the additions over the tensors -- at most 7 roundings on any term's way, all terms non-negative: 8 u of each value, 2^-21.
  * a gradient element  c0 sign(x) + 2 (c1 A + c2 B):  the coefficients are rounded (c0: a division, u; c1, c2: 2e-2f against
    2 * 1e-2, the product with the weight, a division, 3 u), two products, their sum, the final sum:
        |G - T| <= 2 u |c0| + 6 u (2 |c1 A| + 2 |c2 B|) <= 8 u M,   M = |c0| |sign x| + 2 |c1| |A| + 2 |c2| |B|
    with A and B the exact difference terms; fused multiply-adds only remove roundings.  Where M = 0 the element must be
    exactly 0.  Added onto a lattice-valued prior gradient (accumulate = 1): u of the sum more, and the prior itself where M = 0.
  * off the lattice (one leg, the mixed batch): the two differences inside A round as well, so M takes |x - up| + |down - x| for
    |A| and the factor is 10; a value is an fp32 sum of n addends in any order: (n + 3 + 8) u of it.
A failing element is reported with its index; the bound is not widened.

Every gradient and output buffer has a tail of NaN-patterned words behind it that must be unchanged; a buffer the kernel is to
write in full starts out with that pattern too, so an element nobody wrote fails.  After every batched call the persistent
scratch (ops._reg_scratch) is all zero."""
import ctypes

import pytest
import torch

from tests import reg_ref as R
from tests.pinned_ref import deterministic

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, FILL_BITS = 128, 0x7FA5A5A5          # floats behind every buffer; a NaN
W_LATTICE = (1.0, 2.0, 4.0)                 # dL/d(L1, TV_density, TV_color): powers of two
W_RANDOM = (0.37, 1.9, 0.6)
COEF = (0.5, 2.0, 0.25)                     # per-tensor backward: the coefficients themselves, powers of two
JT_ERR_ARG, JT_ERR_UNSUPPORTED = 1, 2

# (C, H, W) of the per-tensor rows
GENERAL = [(4, 1, 1), (16, 1, 9), (16, 9, 1), (20, 31, 7), (48, 5, 3)]
WALK = [(4, 32, 1), (16, 33, 2), (48, 47, 5), (16, 48, 1), (4, 49, 2), (48, 33, 1), (16, 49, 5), (16, 64, 5)]
# second trips: (entry, H, C); W is the smallest that sends eight threads round again (reg_ref.smallest_second_trip)
SECOND = {"general-forward": ("factor_fwd", 31, 48), "general-backward": ("factor_bwd", 31, 48),
          "walk-forward": ("factor_fwd", 33, 48), "walk-backward": ("factor_bwd", 33, 48)}
# batches: plane (H, W) per index, line lengths, (Cd, Ca).  "trip": the density plane of index 0 walks past 512 x 256 items
# (batched forward, three trips) and 1 024 x 256 (fused, two), beside tensors of a single workgroup; its appearance tensors
# are zeros that no call evaluates (TV on the colours is off in that batch)
BATCHES = {"mixed20": ([(31, 7), (33, 5), (1, 9)], [1, 5, 8200], 16, 20),
           "mixed48": ([(31, 7), (49, 2), (9, 1)], [1, 5, 8200], 16, 48),
           "trip": ([(33, None), (32, 2), (5, 3)], [1, 5, 7], 16, 20)}
TV = [(1, 1), (0, 0), (1, 0), (0, 1)]

_TENSORS, _SUMS, _GRADS, _DEVICE = {}, {}, {}, {}


# ---- inputs and references, computed once and shared (never modified); importable without a GPU ----------------------------------
def _seed(H, W, C):
    return 1000003 * H + 1009 * W + C


def _key(H, W, C, kind="lattice"):
    return (H, W, C, kind)


def second_trip_key(row):
    entry, H, C = SECOND[row]
    return _key(H, R.smallest_second_trip(entry, H, C), C)


def batch_keys(name, kind="lattice"):
    """the twelve tensors of a batch: density planes, density lines, appearance planes, appearance lines"""
    hw, lines, Cd, Ca = BATCHES[name]
    hw = [(h, w if w is not None else R.smallest_second_trip("fused", h, Cd)) for h, w in hw]
    app = "zeros" if name == "trip" else kind
    return ([_key(h, w, Cd, kind) for h, w in hw] + [_key(n, 1, Cd, kind) for n in lines] +
            [_key(h, w, Ca, app) for h, w in hw] + [_key(n, 1, Ca, app) for n in lines])


def lattice_keys():
    keys = [_key(H, W, C) for C, H, W in GENERAL + WALK] + [second_trip_key(r) for r in SECOND]
    for name in BATCHES:
        keys += [k for k in batch_keys(name) if k[3] == "lattice"]
    return sorted(set(keys))


def tensor(key):
    if key not in _TENSORS:
        H, W, C, kind = key
        if kind == "lattice":
            x = R.lattice(H, W, C, _seed(H, W, C))
        elif kind == "zeros":
            x = torch.zeros(H, W, C)
        else:
            x = torch.randn(H, W, C, generator=torch.Generator().manual_seed(_seed(H, W, C)))
        _TENSORS[key] = x
    return _TENSORS[key]


def sums(key):
    if key not in _SUMS:
        _SUMS[key] = R.raw_sums(tensor(key))
    return _SUMS[key]


def _grad(key, coef):
    """(T, M) of a tensor under a coefficient triple; the large tensors' are not kept"""
    k = (key, tuple(coef))
    if k in _GRADS:
        return _GRADS[k]
    TM = R.reg_grad(tensor(key), coef, exact_differences=key[3] == "lattice")
    if tensor(key).numel() < (1 << 20):
        _GRADS[k] = TM
    return TM


# ---- device side -----------------------------------------------------------------------------------------------------------------
def _dev(key):
    if key not in _DEVICE:
        _DEVICE[key] = tensor(key).to(DEV).contiguous()
    return _DEVICE[key]


def _guarded(n, fill=None):
    """n floats with GUARD pattern words behind them (and in them, unless `fill` gives their values)"""
    base = torch.empty(n + GUARD, device=DEV, dtype=torch.float32)
    base.view(torch.int32).fill_(FILL_BITS)
    if fill is not None:
        base[:n].copy_(fill.reshape(-1))
    return base


def _untouched(base, lo):
    return bool((base[lo:].view(torch.int32) == FILL_BITS).all())


def _shape_is(entry, key, tv, form, trips, deterministic=False):
    H, W, C, _ = key
    got = R.launch_shape(entry, H, W, C, tv, deterministic)
    assert (got[0], got[3]) == (form, trips), (entry, key, got)
    return got


def _api():
    from joint_tensorf_amd import ops
    from joint_tensorf_amd._lib import lib, ptr
    return ops, lib, ptr


def _factor_forward(key, what):
    ops, lib, ptr = _api()
    H, W, C, _ = key
    out = _guarded(3, torch.zeros(3))
    assert lib.jt_factor_reg_forward(ptr(_dev(key)), H, W, C, ptr(out), ops._stream()) == 0
    torch.cuda.synchronize()
    assert _untouched(out, 3), what
    R.judge_sums(out[:3].cpu(), sums(key), what)


def _factor_backward(key, coef, accumulate, what):
    ops, lib, ptr = _api()
    H, W, C, _ = key
    n = H * W * C
    prior = R.lattice(H, W, C, _seed(H, W, C) + 1) if accumulate else None
    g = _guarded(n, prior)
    c = torch.tensor(coef, device=DEV, dtype=torch.float32)
    assert lib.jt_factor_reg_backward(ptr(_dev(key)), H, W, C, ptr(c), ptr(g), accumulate, ops._stream()) == 0
    torch.cuda.synchronize()
    assert _untouched(g, n), what
    T, M = _grad(key, coef)
    return R.judge_grad(g[:n], T, M, R.KAPPA_LATTICE, what, prior=prior)


# ---- per-tensor entry points -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GENERAL + WALK, ids=lambda s: "%s-C%d-H%d-W%d" % (("walk" if s[1] >= 32 else "general",) + s))
def test_factor_reg_one_trip(shape):
    """jt_factor_reg_forward / _backward directly (accumulate 0 and 1) and through ops.factor_reg: the general loop (H < 32) or
    the row walk (H >= 32: segments of 16 rows, a last one of 1, 15 or 16), one trip.  A walk shape whose TV coefficients are
    zero takes the backward's general loop."""
    ops, lib, ptr = _api()
    C, H, W = shape
    key = _key(H, W, C)
    form = "walk" if H >= 32 else "general"
    _shape_is("factor_fwd", key, True, form, 1)
    _shape_is("factor_bwd", key, True, form, 1)
    _shape_is("factor_bwd", key, False, "general", 1)
    what = "%s C=%d H=%d W=%d" % (form, C, H, W)
    _factor_forward(key, what + " forward")
    worst = [_factor_backward(key, COEF, acc, what + " backward accumulate=%d" % acc) for acc in (0, 1)]
    worst.append(_factor_backward(key, (COEF[0], 0.0, 0.0), 0, what + " backward, TV coefficients zero"))
    # the autograd op: the upstream gradient of the three sums is the coefficient triple
    b = ops.factor_logical(_dev(key)).requires_grad_(True)
    out = ops.factor_reg(b)
    (out * torch.tensor(COEF, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    R.judge_sums(out.detach().cpu(), sums(key), what + " ops.factor_reg")
    T, M = _grad(key, COEF)
    worst.append(R.judge_grad(ops.factor_storage(b.grad), T, M, R.KAPPA_LATTICE, what + " ops.factor_reg"))
    print("%s: worst error / bound = %.3g" % (what, max(worst)))


@pytest.mark.parametrize("row", list(SECOND))
def test_factor_reg_second_trip(row):
    """the smallest tensor whose items exceed cap x 256 by eight threads: H = 31 (general loop) and H = 33 (row walk, the last
    segment a single row), C = 48, against the forward's cap of 1 024 and the backward's of 2 048 -- two trips"""
    entry, H, C = SECOND[row]
    key = second_trip_key(row)
    form = "walk" if H >= 32 else "general"
    _, wgs, items, _ = _shape_is(entry, key, True, form, 2)
    assert wgs == R.CAPS[entry][0] and items - wgs * 256 >= 8
    what = "%s, W=%d (%d items on %d workgroups)" % (row, key[1], items, wgs)
    if entry == "factor_fwd":
        _factor_forward(key, what)
    else:
        print("%s: worst error / bound = %.3g" % (what, _factor_backward(key, COEF, 0, what)))


# ---- batched entry points ----------------------------------------------------------------------------------------------------------
class _Batch:
    def __init__(self, name, kind="lattice"):
        ops, lib, ptr = _api()
        self.name, self.keys = name, batch_keys(name, kind)
        _, _, self.Cd, self.Ca = BATCHES[name]
        self.x = [_dev(k) for k in self.keys]
        self.fac = ops._factors_struct(self.x[0:3], self.x[3:6], self.x[6:9], self.x[9:12])
        hw = []
        for i in range(3):
            hw += [self.keys[i][0], self.keys[i][1], self.keys[3 + i][0]]
        self.hw = (ctypes.c_int32 * 9)(*hw)
        self.scratch = ops._reg_scratch(self.x[0].device)
        self.kappa = R.KAPPA_LATTICE if kind == "lattice" else R.KAPPA_RANDOM

    def weights(self, w3, tv):
        """a term that is switched off has weight zero in the run (the backward reads its switch from the weight)"""
        return (w3[0], w3[1] if tv[0] else 0.0, w3[2] if tv[1] else 0.0)

    def values(self, tv):
        ts = [tensor(k) for k in self.keys[:9]]
        return R.scene_values(ts[0:3], ts[3:6], ts[6:9], bool(tv[0]), bool(tv[1]), sums=[sums(k) for k in self.keys[:9]])

    def n_addends(self):
        """per value, the most addends of one tensor's sum (the leg off the lattice)"""
        tvn = lambda ks: max(max(C * (H - 1) * W, C * H * (W - 1)) for H, W, C, _ in ks)
        return max(H * W * C for H, W, C, _ in self.keys[:6]), tvn(self.keys[0:3]), tvn(self.keys[6:9])

    def buffers(self, prior):
        """twelve guarded gradient buffers: pattern-filled, or holding a lattice-valued prior gradient"""
        ops, lib, ptr = _api()
        self.prior = [R.lattice(H, W, C, _seed(H, W, C) + 2) if prior else None for H, W, C, _ in self.keys]
        self.g = [_guarded(k[0] * k[1] * k[2], p) for k, p in zip(self.keys, self.prior)]
        return ops._factors_struct(self.g[0:3], self.g[3:6], self.g[6:9], self.g[9:12])

    def check_scratch(self, what):
        assert int((self.scratch.view(torch.int32) != 0).sum()) == 0, what + ": residue in the scratch"

    def check_grads(self, w3, tv, what):
        """every element of the nine gradients; an appearance plane outside TV and the appearance lines keep their fill (or
        their prior) bit for bit; every guard tail"""
        worst = 0.0
        for slot, (key, g, prior) in enumerate(zip(self.keys, self.g, self.prior)):
            H, W, C, _ = key
            n = H * W * C
            assert _untouched(g, n), (what, slot)
            if slot < 6 or (slot < 9 and tv[1]):
                coef = R.scene_coefs(slot, H, W, C, w3, bool(tv[0]), bool(tv[1]))
                T, M = _grad(key, coef)
                worst = max(worst, R.judge_grad(g[:n], T, M, self.kappa, "%s tensor %d" % (what, slot), prior=prior))
            elif prior is None:
                assert _untouched(g, 0), (what, slot)
            else:
                assert torch.equal(g[:n].cpu().view(torch.int32), prior.reshape(-1).view(torch.int32)), (what, slot)
        return worst

    # the five calls
    def forward(self, tv, what, n_addends=None):
        ops, lib, ptr = _api()
        out = _guarded(3)
        rc = lib.jt_reg_losses_forward(self.fac, self.hw, self.Cd, self.Ca, tv[0], tv[1], ptr(self.scratch), ptr(out),
                                       ops._stream())
        torch.cuda.synchronize()
        assert rc == 0 and _untouched(out, 3), what
        self.check_scratch(what)
        R.judge_values(out[:3].cpu(), self.values(tv), what, n_addends)
        return out[:3].clone()

    def backward(self, w3, tv, accumulate, what):
        ops, lib, ptr = _api()
        w = self.weights(w3, tv)
        gfac = self.buffers(prior=bool(accumulate))
        g3 = torch.tensor(w, device=DEV, dtype=torch.float32)
        rc = lib.jt_reg_losses_backward(self.fac, self.hw, self.Cd, self.Ca, ptr(g3), tv[0], tv[1], gfac, accumulate,
                                        ptr(self.scratch), ops._stream())
        torch.cuda.synchronize()
        assert rc == 0, what
        self.check_scratch(what)
        return self.check_grads(w, tv, what)

    def fused(self, w3, tv, dev_weights, what, n_addends=None):
        ops, lib, ptr = _api()
        w = self.weights(w3, tv)
        gfac, out = self.buffers(prior=False), _guarded(3)
        g3 = torch.tensor(w, device=DEV, dtype=torch.float32)
        rc = lib.jt_reg_losses_fused(self.fac, self.hw, self.Cd, self.Ca, tv[0], tv[1],
                                     None if dev_weights else (ctypes.c_float * 3)(*w), ptr(g3) if dev_weights else None,
                                     gfac, ptr(self.scratch), ptr(out), ops._stream())
        torch.cuda.synchronize()
        assert rc == 0 and _untouched(out, 3), what
        self.check_scratch(what)
        R.judge_values(out[:3].cpu(), self.values(tv), what, n_addends)
        return self.check_grads(w, tv, what)


def _mixed_shapes(B, tv):
    """what the mixed batch is there for, through the mirror"""
    k = B.keys
    for entry in ("batch_fwd", "fused"):
        _shape_is(entry, k[0], tv[0], "general", 1)                                 # H = 31
        _shape_is(entry, k[1], tv[0], "walk" if tv[0] else "general", 1)            # H = 33 | 49: a last segment of one row
        _shape_is(entry, k[2], tv[0], "general", 1)                                 # H = 1 | W = 1
        _shape_is(entry, k[7], tv[1], "walk" if tv[1] else "general", 1)
    _shape_is("batch_fwd", k[5], False, "general", 2)                               # the 8 200-entry line: 32 threads go again
    _shape_is("fused", k[5], False, "general", 1)
    _shape_is("batch_bwd", k[1], tv[0], "walk" if tv[0] else "general", 1)
    assert (k[3][0], k[4][0], k[5][0]) == (1, 5, 8200) and (k[2][0] == 1 or k[2][1] == 1)
    assert k[1][0] % 16 == 1 and k[0][0] < 32 <= k[1][0]


@pytest.mark.parametrize("tv", TV, ids=lambda t: "tv%d%d" % t)
@pytest.mark.parametrize("name", ["mixed20", "mixed48"])
def test_reg_losses_mixed_batch(name, tv):
    """jt_reg_losses_forward, _backward (accumulate 0 and 1) and _fused (host and device weights), each against the reference,
    on three planes that come from no common grid -- general loop (H = 31), row walk with a one-row last segment (H = 33 | 49),
    degenerate (H = 1 | W = 1) -- and lines of 1, 5 and 8 200 entries: tensors from one workgroup of four live threads to 129
    (the no-TV forward: 128 and a second trip).  A TV term that is switched off gives 0 and leaves the appearance planes'
    buffers alone."""
    B = _Batch(name)
    _mixed_shapes(B, tv)
    what = "%s tv=%s " % (name, tv)
    out = B.forward(tv, what + "forward")
    assert (tv[0] or float(out[1]) == 0.0) and (tv[1] or float(out[2]) == 0.0)
    worst = [B.backward(W_LATTICE, tv, acc, what + "backward accumulate=%d" % acc) for acc in (0, 1)]
    worst += [B.fused(W_LATTICE, tv, dw, what + "fused, %s weights" % ("device" if dw else "host")) for dw in (False, True)]
    print("%sworst error / bound = %.3g" % (what, max(worst)))


@pytest.mark.parametrize("entry", ["forward", "fused", "backward"])
def test_reg_losses_second_trip(entry):
    """one density plane of 33 rows whose walk items exceed 1 024 x 256 by eight threads -- three trips of the batched forward
    (cap 512), two of the fused launch (cap 1 024), one of the backward (2 048 workgroups) -- beside tensors of a single
    workgroup; TV on the density only"""
    B = _Batch("trip")
    tv, k = (1, 0), B.keys
    _shape_is("batch_fwd", k[0], True, "walk", 3)
    _shape_is("fused", k[0], True, "walk", 2)
    _shape_is("batch_bwd", k[0], True, "walk", 1)
    for j in (1, 2, 3, 4, 5):
        assert R.launch_shape("batch_fwd", *k[j][:3], j < 3)[1] == 1
    if entry == "forward":
        B.forward(tv, "trip forward")
    elif entry == "fused":
        print("trip fused: worst error / bound = %.3g" % B.fused(W_LATTICE, tv, False, "trip fused"))
    else:
        print("trip backward: worst error / bound = %.3g" % B.backward(W_LATTICE, tv, 0, "trip backward"))


def test_reg_losses_deterministic():
    """Deterministic mode: jt_reg_losses_forward runs one workgroup per tensor (the 8 200-entry line: 129 trips of its general
    loop; the walk plane: one), meets the same bound, and two calls agree bit for bit.  jt_reg_losses_fused refuses: its
    gradient buffers, its output and the scratch keep every bit."""
    ops, lib, ptr = _api()
    B = _Batch("mixed20")
    tv = (1, 1)
    assert _shape_is("batch_fwd", B.keys[5], False, "general", 129, deterministic=True)[1] == 1
    assert _shape_is("batch_fwd", B.keys[1], True, "walk", 1, deterministic=True)[1] == 1
    assert _shape_is("batch_fwd", B.keys[0], True, "general", 4, deterministic=True)[1] == 1
    with deterministic(True):
        a = B.forward(tv, "deterministic forward")
        b = B.forward(tv, "deterministic forward, again")
        gfac, out = B.buffers(prior=False), _guarded(3)
        rc = lib.jt_reg_losses_fused(B.fac, B.hw, B.Cd, B.Ca, 1, 1, (ctypes.c_float * 3)(*W_LATTICE), None, gfac,
                                     ptr(B.scratch), ptr(out), ops._stream())
        torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert rc == JT_ERR_UNSUPPORTED
    assert _untouched(out, 0) and all(_untouched(g, 0) for g in B.g)
    B.check_scratch("fused, refused")


def test_reg_losses_off_the_lattice():
    """normal-distributed values on the mixed batch, weights that are no powers of two: a kernel that is right on exact inputs
    only.  Values to (n + 11) 2^-24, gradients to 10 x 2^-24 of the absolute-difference magnitude."""
    B = _Batch("mixed20", kind="random")
    tv, n = (1, 1), B.n_addends()
    B.forward(tv, "random forward", n)
    worst = [B.backward(W_RANDOM, tv, 0, "random backward"), B.fused(W_RANDOM, tv, False, "random fused", n)]
    with deterministic(True):
        B.forward(tv, "random forward, deterministic", n)
    print("off the lattice: worst error / bound = %.3g" % max(worst))
