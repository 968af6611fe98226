"""Float64 reference of k_adam_batch (csrc/jt_optim.hip) from the fp32 inputs and the fp32 scalars the kernel sees, with an
element-wise error bound that is derived, not measured, and carried from step to step.  No GPU needed.

The kernel, per element, in fp32 (u = 2^-24, every operation rounds once; a fused multiply-add only removes roundings):
    m' = b1 m + omb1 g                      omb1 = fl(1 - b1), omb2 = fl(1 - b2): the reference uses these fp32 VALUES
    v' = b2 v + (omb2 g) g
    p' = p - ss (m' / (sqrt(v') ibc + eps))  ss = step size lr / (1 - b1^t), ibc = 1 / sqrt(1 - b2^t), both fp32 values
Bounds, with e_m, e_v, e_p what the inputs m, v, p already carry (0 for a single step on given inputs):
    m': product, product, sum: three roundings, each at most u (|b1 m| + |omb1 g|) =: u Mm          E_m = b1 e_m + 3 u Mm
    v': the g term passes two products and the sum, the v term one product and the sum; all addends are non-negative,
        so each rounding is at most u v':                                                          E_v = b2 e_v + 3 u v'
    denominator d = sqrt(v') ibc + eps: sqrt halves the relative error of v', then the square root, the product and the
        sum round (sqrtf and the division are correctly rounded: the build uses no fast-math), and a coefficient that was
        rounded to fp32 from a double (`coef_roundings` = 1: optim.VMAdam) adds one u to ibc and one to ss;
        sqrt(v') ibc <= d, so relative to d:                                                        r_d = E_v / (2 v') + (3 + c) u
    update q = ss m' / d: the error of m', and relative to |m'| the denominator's, the division, the product, ss's own:
                                                                                                   E_q = ss / d (E_m + |m'| (r_d + (2 + c) u))
    p': one more rounding, allowed a whole ulp of p' (2 u |p'|):                                    E_p = e_p + E_q + 2 u |p'|
For one step with c = 0 this is  E_q <= ss / d (3 u Mm + 6.5 u |m'|) <= 9.5 u ss Mm / d.  The expressions are first order in u;
SECOND_ORDER multiplies every bound by 1 + 2^-16 for the products of two roundings (each below 2^-20 of a bound here).
An element with m = g = v = 0 has Mm = v' = 0: its m', v' and update are exactly 0 and p' is p bit for bit."""
import ctypes
import math

import torch

EPS32 = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -16
# n: the scalar tail, a thread's quad seam (256 threads x 4 floats = 1 024), the workgroup seam (4 096), two and three workgroups
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 1027, 4095, 4096, 4097, 4099, 8193]
MAX_ITEMS = 32        # kAdamMaxItems: items of one launch (tests/test_reg_ref.py reads it out of the source)
ELEMS_PER_BLOCK = 4096


def f32(x):
    return ctypes.c_float(x).value


def scalars(b1, b2, eps):
    """the fp32 values of (b1, 1.f - b1, b2, 1.f - b2, eps) as Python doubles"""
    b1, b2 = f32(b1), f32(b2)
    return b1, f32(1.0 - b1), b2, f32(1.0 - b2), f32(eps)


def item_coefficients(lr, t, b1, b2):
    """(step_size, inv_bc2_sqrt) as adam_launch forms them from a JtAdamItem's float fields"""
    bc1, bc2 = f32(1.0 - b1 ** t), f32(1.0 - b2 ** t)
    return f32(f32(lr) / bc1), f32(1.0 / f32(math.sqrt(bc2)))


def item_schedule(k):
    """(lr, step count) of item k of a multi-item call: every item its own, and items 32 and 64 (the first of the second and
    third launch) at least a factor of two from items 0 and 1 in both coefficients (asserted in tests/test_reg_ref.py)"""
    return 1e-3 * (1.0, 0.25, 4.0)[k % 3] * (1.0 + k / 256.0), k + 1


def step(p, g, m, v, sc, ss, ibc, errs=None, coef_roundings=0):
    """one reference step in float64: (p', m', v'), (E_p, E_m, E_v).  sc = scalars(...); ss, ibc: the fp32 coefficient values
    (or the doubles they were rounded from, with coef_roundings = 1); errs: the bounds the inputs carry."""
    b1, omb1, b2, omb2, eps = sc
    p, g, m, v = (t.double() for t in (p, g, m, v))
    e_p, e_m, e_v = errs if errs is not None else (0.0, 0.0, 0.0)
    c, u = float(coef_roundings), EPS32
    m2 = b1 * m + omb1 * g
    Mm = (b1 * m).abs() + (omb1 * g).abs()
    v2 = b2 * v + omb2 * g * g
    d = v2.sqrt() * ibc + eps
    p2 = p - ss * (m2 / d)
    E_m = b1 * e_m + 3 * u * Mm
    E_v = b2 * e_v + 3 * u * v2
    r_d = torch.where(v2 > 0, E_v / (2 * v2).clamp_min(1e-300), torch.zeros_like(v2)) + (3 + c) * u
    E_q = ss / d * (E_m + m2.abs() * (r_d + (2 + c) * u))
    E_p = e_p + E_q + 2 * u * p2.abs()
    return (p2, m2, v2), tuple(SECOND_ORDER * e for e in (E_p, E_m, E_v))


def judge(got, ref, bounds, what):
    """(p, m, v) of the kernel against the reference's, element by element at their bounds; NaN fails.  Raises AssertionError
    naming the tensor and the first offending element; returns the worst |got - ref| / bound per tensor."""
    worst = []
    for name, a, r, e in zip("pmv", got, ref, bounds):
        a, r, e = a.double().cpu().reshape(-1), r.reshape(-1), e.reshape(-1)
        err = (a - r).abs()
        bad = ~(err <= e)
        if bool(bad.any()):
            k = int(bad.nonzero()[0])
            raise AssertionError("%s: %s[%d] of %d: %r vs %r, bound %.3g (%d elements off)" % (
                what, name, k, a.numel(), float(a[k]), float(r[k]), float(e[k]), int(bad.sum())))
        live = e > 0
        worst.append(float((err[live] / e[live]).max()) if bool(live.any()) else 0.0)
    return worst


def inputs(n, seed):
    """(p, g, m, v) fp32 on the CPU: gradients spanning 1e-6 .. 1e3 in both signs with exact zeros, moments of a run in
    progress, and every seventh element (from element 0: the scalar tail of a short tensor has one) with g = m = v = 0"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.sign(torch.randn(n, generator=gen)) * 10.0 ** (9.0 * torch.rand(n, generator=gen) - 6.0)
    g[torch.rand(n, generator=gen) < 0.1] = 0.0
    m = torch.randn(n, generator=gen) * g.abs().clamp_min(1e-3)
    v = torch.rand(n, generator=gen) * (g * g).clamp_min(1e-6)
    idle = torch.arange(n) % 7 == 0
    g[idle], m[idle], v[idle] = 0.0, 0.0, 0.0
    return p, g, m, v, idle
