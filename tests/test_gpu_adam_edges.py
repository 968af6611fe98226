"""k_adam_batch (csrc/jt_optim.hip) at its launch edges, element by element against the float64 reference of
tests/adam_ref.py, whose docstring derives the bounds (u = 2^-24, first order, counted, never tuned on the device):
    m': 3 u (|b1 m| + |omb1 g|)        v': 3 u v'        p': <= 9.5 u ss (|b1 m| + |omb1 g|) / d  +  2 u |p'|
from the fp32 inputs and the same fp32 scalars the kernel sees (b1, 1.f - b1, b2, 1.f - b2, eps, step size, 1 / sqrt(bc2),
formed the way adam_launch forms them).  An element with g = m = v = 0 must not move at all.

Launch arithmetic: a workgroup of 256 threads takes 4 096 elements, thread t the quads at t, t + 256, t + 512, t + 768 (a seam
every 1 024 elements); a quad that does not lie wholly inside n is stepped element by element.  adam_launch puts 32 items
into one launch and offsets the coefficients of a later launch by 2 x first item -- in the launch arguments, in `dyn` (device
memory) and in `coefs_host` alike.

Every item's p, g, m and v live in four arenas of NaN-patterned words, 16-byte aligned, 64 words apart: after a call every word
outside the items -- the gap up to the next aligned start included -- must hold the pattern."""
import ctypes

import pytest
import torch

from tests import adam_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
B1, B2, EPS = 0.9, 0.99, 1e-8
ENTRIES = ["value", "dyn", "coefs"]
FILL_BITS, GAP = 0x7FA5A5A5, 64
JT_ERR_ARG, JT_ERR_UNSUPPORTED = 1, 2


class _Arena:
    """items of the given sizes laid out in four pattern-filled arenas (p, g, m, v), with the schedule adam_ref.item_schedule
    gives item k (or `first_item`'s onwards)"""

    def __init__(self, sizes, first_item=0):
        from joint_tensorf_amd._lib import JtAdamItem
        self.sizes, self.off, at = list(sizes), [], GAP
        for n in self.sizes:
            self.off.append(at)
            at = (at + n + 3) // 4 * 4 + GAP
        self.total = at
        self.host = [A.inputs(n, 100 + first_item + k) for k, n in enumerate(self.sizes)]
        self.owned = torch.zeros(self.total, dtype=torch.bool)
        self.bufs = []
        for role in range(4):
            flat = torch.full((self.total,), FILL_BITS, dtype=torch.int32).view(torch.float32).clone()
            for o, n, h in zip(self.off, self.sizes, self.host):
                flat[o:o + n] = h[role]
                self.owned[o:o + n] = True
            self.bufs.append(flat.to(DEV))
        self.before = [b.clone() for b in self.bufs]
        self.sched = [A.item_schedule(first_item + k) for k in range(len(self.sizes))]
        self.coefs = [A.item_coefficients(lr, t, B1, B2) for lr, t in self.sched]
        self.arr = (JtAdamItem * len(self.sizes))()
        for k, (o, n) in enumerate(zip(self.off, self.sizes)):
            it = self.arr[k]
            it.p, it.g, it.m, it.v = (b.data_ptr() + 4 * o for b in self.bufs)
            it.n, it.lr = n, self.sched[k][0]
            it.bias_correction1, it.bias_correction2 = 1.0 - B1 ** self.sched[k][1], 1.0 - B2 ** self.sched[k][1]

    def call(self, entry):
        from joint_tensorf_amd import ops
        from joint_tensorf_amd._lib import lib, ptr
        flat = [c for pair in self.coefs for c in pair]
        n, st = len(self.sizes), ops._stream()
        if entry == "value":
            rc = lib.jt_adam_step(self.arr, n, B1, B2, EPS, st)
        elif entry == "dyn":
            self.dyn = torch.zeros(len(flat), device=DEV)
            ops.poke_floats(self.dyn, flat)
            rc = lib.jt_adam_step_dyn(self.arr, n, B1, B2, EPS, ptr(self.dyn), st)
        else:
            rc = lib.jt_adam_step_coefs(self.arr, n, B1, B2, EPS, (ctypes.c_float * len(flat))(*flat), st)
        torch.cuda.synchronize()
        return rc

    def outside_untouched(self):
        return all(bool((b.cpu().view(torch.int32)[~self.owned] == FILL_BITS).all()) for b in self.bufs)

    def unchanged(self):
        return all(torch.equal(b.view(torch.int32), c.view(torch.int32)) for b, c in zip(self.bufs, self.before))

    def judge(self, what):
        sc = A.scalars(B1, B2, EPS)
        worst = [0.0, 0.0, 0.0]
        got = [b.cpu() for b in self.bufs]
        assert torch.equal(got[1].view(torch.int32), self.before[1].cpu().view(torch.int32)), what + ": the gradient was written"
        for k, (o, n, h) in enumerate(zip(self.off, self.sizes, self.host)):
            p, g, m, v, idle = h
            ref, bounds = A.step(p, g, m, v, sc, *self.coefs[k])
            mine = (got[0][o:o + n], got[2][o:o + n], got[3][o:o + n])
            w = A.judge(mine, ref, bounds, "%s item %d (n=%d, lr=%.3g, t=%d)" % ((what, k, n) + self.sched[k]))
            worst = [max(a, b) for a, b in zip(worst, w)]
            # g = m = v = 0: no update at all
            assert torch.equal(mine[0][idle].view(torch.int32), p[idle].view(torch.int32)), (what, k)
            assert bool((mine[1][idle] == 0).all()) and bool((mine[2][idle] == 0).all()), (what, k)
        assert self.outside_untouched(), what + ": a word outside the items changed"
        return worst


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n", A.SIZES)
def test_adam_one_item(n, entry):
    """one tensor of n elements: the scalar tail (n = 1, 3, 5, 1 027, ...), a thread's quad seam at 1 024, the workgroup seam
    at 4 096, two and three workgroups"""
    a = _Arena([n], first_item=n % 7)
    assert a.call(entry) == 0
    print("n=%d %s: worst error / bound (p, m, v) = %.3g %.3g %.3g" % ((n, entry) + tuple(a.judge("n=%d %s" % (n, entry)))))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("items", [32, 33, 65])
def test_adam_many_items(items, entry):
    """32, 33 and 65 items in one call: one, two and three launches.  Every item has its own learning rate and step count, and
    items 32 and 64 (the first of a later launch) are a factor of two or more from items 0 and 1 in both coefficients, so a
    coefficient taken from the wrong item moves every element out of its bound (tests/test_reg_ref.py shows it)."""
    assert (items + A.MAX_ITEMS - 1) // A.MAX_ITEMS == {32: 1, 33: 2, 65: 3}[items]
    a = _Arena([A.SIZES[(5 * k) % len(A.SIZES)] for k in range(items)])
    assert a.call(entry) == 0
    print("%d items %s: worst error / bound (p, m, v) = %.3g %.3g %.3g" % (
        (items, entry) + tuple(a.judge("%d items %s" % (items, entry)))))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("at", [0, 40], ids=["item0", "item40"])
def test_adam_argument_checks_write_nothing(at, entry):
    """a misaligned pointer is unsupported, n = 0 or a null pointer a bad argument -- in the first item or in one of a later
    launch (item 40 of 42), and in either case nothing at all is written: no earlier launch of the call has run"""
    for fault, want in (("misaligned", JT_ERR_UNSUPPORTED), ("empty", JT_ERR_ARG), ("null", JT_ERR_ARG)):
        a = _Arena([A.SIZES[k % 5] for k in range(at + 2)])
        it = a.arr[at]
        if fault == "misaligned":
            it.m = it.m + 4
        elif fault == "empty":
            it.n = 0
        else:
            it.v = None
        assert a.call(entry) == want, fault
        assert a.unchanged(), fault


def test_vmadam_forty_tensors_vs_float64_adam():
    """optim.VMAdam over 40 small tensors -- more than 32 items, so two launches, through the general step and then the planned
    step -- against torch.optim.Adam in float64 on the CPU over three steps.  Both take betas and eps that are fp32 values and
    the same learning rates, so they differ by rounding alone: the kernel's operations, and the two coefficients VMAdam rounds
    from doubles (coef_roundings = 1 in adam_ref.step).  The bounds compound: step k's (E_p, E_m, E_v) enter step k + 1 as
    what its inputs carry (E_m' = b1 E_m + ..., E_v' = b2 E_v + ..., E_p' = E_p + ...), evaluated on the reference's values.
    After the last step every tensor's exp_avg / exp_avg_sq is held to its bound, not tensor 0's alone."""
    import math
    from joint_tensorf_amd import optim as jopt
    b1, b2, eps = A.f32(B1), A.f32(B2), A.f32(EPS)
    sc = A.scalars(b1, b2, eps)
    assert sc[0] == b1 and sc[2] == b2 and sc[4] == eps
    sizes = [A.SIZES[(2 * k) % 9] for k in range(40)]                     # 1 .. 4 095 elements
    base = [A.inputs(n, 500 + k)[0] for k, n in enumerate(sizes)]
    ref_p = [torch.nn.Parameter(b.double()) for b in base]
    hip_p = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    lrs = [0.02, 1e-3]
    groups = lambda ps: [dict(params=ps[:7], lr=lrs[0]), dict(params=ps[7:], lr=lrs[1])]
    ref = torch.optim.Adam(groups(ref_p), betas=(b1, b2), eps=eps)
    hip = jopt.VMAdam(groups(hip_p), betas=(b1, b2), eps=eps)
    assert jopt.PLAN_STEPS
    errs = [None] * 40
    for x in hip_p:                      # gradients rewritten in place from step to step: the plan made by step 1 holds
        x.grad = torch.empty_like(x)
    for t in (1, 2, 3):
        grads = [A.inputs(n, 900 + 40 * t + k)[1] for k, n in enumerate(sizes)]
        state = [(r.detach().clone(), ref.state[r]["exp_avg"].clone() if t > 1 else torch.zeros_like(r),
                  ref.state[r]["exp_avg_sq"].clone() if t > 1 else torch.zeros_like(r)) for r in ref_p]
        for r, x, g in zip(ref_p, hip_p, grads):
            r.grad = g.double()
            x.grad.copy_(g.to(DEV))
        ref.step()
        hip.step()
        torch.cuda.synchronize()
        for k in range(40):
            lr = lrs[0] if k < 7 else lrs[1]
            p0, m0, v0 = state[k]
            out, errs[k] = A.step(p0, grads[k], m0, v0, sc, lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), errs[k],
                                  coef_roundings=1)
            st = ref.state[ref_p[k]]
            theirs = (ref_p[k].detach(), st["exp_avg"], st["exp_avg_sq"])
            for mine, torchs, e in zip(out, theirs, errs[k]):        # adam_ref.step IS torch's Adam, far inside the bounds
                assert bool(((mine - torchs).abs() <= 1e-3 * e).all()), (t, k)
            hs = hip.state[hip_p[k]]
            A.judge((hip_p[k].detach(), hs["exp_avg"], hs["exp_avg_sq"]), theirs, errs[k],
                    "step %d tensor %d (n=%d)" % (t, k, sizes[k]))
            assert hs["step"] == float(t)
    assert getattr(hip, "planned_steps", 0) == 2
