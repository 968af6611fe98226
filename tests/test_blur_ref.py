"""The blur reference of tests/blur_ref.py, held to account on the CPU: it reproduces the golden known answers, it is
self-adjoint-consistent in fp64, a correct fp32 implementation (the fp32 oracle) meets its criterion with room, and the
criterion catches each of seven plausible kernel faults that the earlier recipe -- Gaussian taps with sigma <= 6.4,
atol = 2e-5 on values, max-error ratio 1e-5 on gradients (tests/test_gpu_units.py) -- lets through in part.

Faults the earlier recipe does NOT catch (test_sensitivity asserts exactly this list):
    outer_tap_dropped                        the outermost Gaussian tap is 2.3e-7: below atol
    taps_reversed                            symmetric taps: correlation == convolution, forward index == adjoint index
    right_fold_one_tap_late                  the lost term is R_{n-r} = k[2 r], 2.3e-7 again
    last_quad_of_partial_chunk_not_written   no unit test has a channel count with a partial chunk behind a full one
The other three (left fold missing, zero padding, last position not written) move its outputs by far more than its
tolerances on the shapes it has; here they are caught too, on every tap kind."""
import os

import numpy as np
import pytest
import torch

from tests import blur_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _storage(x):      # logical [1, C, H, W] -> [H, W, C]
    return x[0].permute(1, 2, 0).contiguous()


def _logical(x):
    return x.permute(2, 0, 1)[None]


def test_reference_reproduces_golden_known_answers():
    d = np.load(os.path.join(GOLDEN, "known_answers.npz"))
    k = torch.tensor(d["blur.kernel"])
    cub = R.forward_ref(_storage(torch.tensor(d["blur.cubic.in"])), k)
    np.testing.assert_allclose(_logical(cub).numpy(), d["blur.cubic.out"], atol=1e-5)
    ln = R.forward_ref(_storage(torch.tensor(d["blur.line.in"])), k)
    np.testing.assert_allclose(_logical(ln).numpy(), d["blur.line.out"], atol=1e-5)
    # the reference's reshape quirk: the [13][9][C] storage of a [1, C, 13, 9] plane is blurred as [9][13][C]
    xs = _storage(torch.tensor(d["blur.noncubic.in"]))
    assert tuple(xs.shape) == (13, 9, 4)
    non = R.forward_ref(xs.reshape(9, 13, 4), k)
    assert tuple(_logical(non).shape) == d["blur.noncubic.out"].shape == (1, 4, 9, 13)
    np.testing.assert_allclose(_logical(non).numpy(), d["blur.noncubic.out"], atol=1e-5)


SHAPES = [(70, 70, 16), (9, 9, 4), (300, 40, 20), (33, 1, 8), (1, 21, 4), (13, 9, 4)]


@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint_identity_and_pass_composition_fp64(shape):
    """<A x, y> = <x, A^T y>, and blur_plane == the two blur_line passes the magnitude is built from"""
    H, W, C = shape
    for ntaps in (9, 65):
        k = R.make_taps("signed", ntaps)
        x, y = R.make_data(shape, "randn", 1).double(), R.make_data(shape, "randn", 2).double()
        Ax, ATy = R.forward_ref(x, k), R.adjoint_ref(y, k)
        lhs, rhs = float((Ax * y).sum()), float((x * ATy).sum())
        scale = float((R.magnitude_forward(x, k) * y.abs()).sum())
        assert abs(lhs - rhs) <= 1e-13 * scale, (shape, ntaps, lhs, rhs)
        z = x
        for axis, _n in R.passes(H, W):
            z = R.one_pass(z, k.double(), axis)
        assert float((z - Ax).abs().max()) <= 1e-13 * float(R.magnitude_forward(x, k).max())


def _fp32_oracle_ratios(shape, k, data_kind):
    H, W, C = shape
    x, g = R.make_data(shape, data_kind, 3), R.make_data(shape, data_kind, 4)
    fam = [R.LINE] * len(R.passes(H, W))
    out = R.forward_ref(x, k, torch.float32)
    gin = R.adjoint_ref(g, k, torch.float32)
    assert out.dtype == gin.dtype == torch.float32
    Mf, Ma = R.magnitude_forward(x, k), R.magnitude_adjoint(g, k)
    rf, ra = R.forward_ref(x, k), R.adjoint_ref(g, k)
    f = R.judge(out, rf, Mf, R.kappa_forward(fam, k.numel()))
    a = R.judge(gin, ra, Ma, R.kappa_adjoint(fam, k.numel(), H, W))
    return f, a, (out, rf, Mf), (gin, ra, Ma)


@pytest.mark.parametrize("shape", [(70, 70, 16), (9, 9, 4), (300, 40, 20)])
def test_fp32_oracle_meets_the_criterion(shape):
    """the bar is reachable: torch.float32 conv1d sits at kappa <= 8.4 against M (printed), the derived bounds are
    18 - 808"""
    worst = 0.0
    for kind, ntaps in (("signed", 9), ("signed", 65), ("signed", 201), ("gauss:0.3", 65), ("gauss:2.3", 65), ("gauss:6.4", 65),
                        ("ramp", 9), ("flat", 65)):
        f, a, _, _ = _fp32_oracle_ratios(shape, R.make_taps(kind, ntaps), "randn")
        assert f[0] == 0 and a[0] == 0, (shape, kind, ntaps, f, a)
        worst = max(worst, f[1], a[1])
    print("fp32 oracle, shape %s: worst kappa %.2f" % (shape, worst))


@pytest.mark.parametrize("shape", [(1, 1, 4), (3, 70, 4), (130, 33, 20)])
@pytest.mark.parametrize("ntaps", [1, 9, 65, 201])
def test_fp32_oracle_is_exact_on_integer_rows(shape, ntaps):
    if ntaps == 201 and shape == (130, 33, 20):
        shape = (130, 1, 20)     # (a plane's corner texel would collect 100 x 33 gradients x 201^2 taps: above 2^24)
    tap_kind, data_kind = R.exact_kinds(ntaps)
    for kind in [tap_kind, "flat", "onehot:0", "onehot:%d" % (ntaps // 2), "onehot:%d" % (ntaps - 1)]:
        k = R.make_taps(kind, ntaps)
        _, _, (out, rf, Mf), (gin, ra, _Ma) = _fp32_oracle_ratios(shape, k, data_kind)
        Ma = R.magnitude_adjoint(R.make_data(shape, data_kind, 4), k, cancellation=False)
        assert R.exact_magnitude_ok(Mf, k) and R.exact_magnitude_ok(Ma, k), (shape, ntaps, kind, float(Mf.max()), float(Ma.max()))
        assert R.exact_mismatches(out, rf) == 0 and R.exact_mismatches(gin, ra) == 0, (shape, ntaps, kind)


def test_onehot_is_the_clamped_shift():
    """the simplest known answer, without any reference: a one-hot tap at t shifts by t - r with the ends repeated"""
    x = R.make_data((11, 1, 4), "int", 5)
    for t in (0, 4, 8):
        out = R.forward_ref(x, R.make_taps("onehot:%d" % t, 9))
        idx = (torch.arange(11) + t - 4).clamp(0, 10)
        assert torch.equal(out, x.double()[idx])


# ---- sensitivity ------------------------------------------------------------------------------------------------
NEW_ROWS = [   # (H, W, C), ntaps, tap kind, data kind
    ((12, 17, 20), 9, "signed", "randn"), ((12, 17, 20), 9, "int", "int"), ((33, 1, 8), 65, "signed", "randn"),
    ((40, 1, 4), 65, "ramp", "randn"), ((9, 14, 4), 9, "flat", "int"), ((40, 1, 4), 65, "gauss:6.4", "randn"),
    ((12, 1, 4), 9, "onehot:8", "int"),
]
OLD_ROWS = [((14, 14, 16), s) for s in (0.7, 2.3, 6.4)] + [((21, 21, 48), s) for s in (0.7, 2.3, 6.4)] + \
           [((9, 9, 4), s) for s in (0.7, 2.3, 6.4)] + [((70, 70, 16), s) for s in (0.7, 2.3, 6.4)] + [((33, 1, 16), 3.1)]


def _new_catches(fault):
    rows = []
    for shape, ntaps, kind, data in NEW_ROWS:
        H, W, C = shape
        k = R.make_taps(kind, ntaps)
        x, g = R.make_data(shape, data, 6), R.make_data(shape, data, 7)
        fam = [R.LINE] * len(R.passes(H, W))
        out = torch.tensor(R.model_apply(x.numpy(), k.numpy(), fault, adjoint=False))
        gin = torch.tensor(R.model_apply(g.numpy(), k.numpy(), fault, adjoint=True))
        if data == "int":
            bad = R.exact_mismatches(out, R.forward_ref(x, k)) + R.exact_mismatches(gin, R.adjoint_ref(g, k))
        else:
            bad = R.judge(out, R.forward_ref(x, k), R.magnitude_forward(x, k), R.kappa_forward(fam, ntaps))[0] + \
                R.judge(gin, R.adjoint_ref(g, k), R.magnitude_adjoint(g, k), R.kappa_adjoint(fam, ntaps, H, W))[0]
        if bad:
            rows.append((shape, ntaps, kind))
    return rows


def _old_catches(fault):
    """the recipe of test_blur_plane_vs_oracle / test_blur_line_vs_oracle on their shapes and sigmas"""
    for shape, sigma in OLD_ROWS:
        k = R.make_taps("gauss:%g" % sigma, 65)
        x, g = R.make_data(shape, "randn", 8), R.make_data(shape, "randn", 9)
        out = R.model_apply(x.numpy(), k.numpy(), fault, adjoint=False)
        gin = R.model_apply(g.numpy(), k.numpy(), fault, adjoint=True)
        ref, gref = R.forward_ref(x, k).numpy(), R.adjoint_ref(g, k).numpy()
        if not np.allclose(out, ref, atol=2e-5, rtol=1e-5):
            return True
        if not np.abs(gin - gref).max() / max(np.abs(gref).max(), 1e-30) < 1e-5:
            return True
    return False


OLD_RECIPE_MISSES = ["outer_tap_dropped", "taps_reversed", "right_fold_one_tap_late",
                     "last_quad_of_partial_chunk_not_written"]


def test_sensitivity_to_faults():
    # no fault: the model is the operator, and both recipes accept it
    assert _new_catches(None) == [] and not _old_catches(None)
    missed = []
    for fault in R.FAULTS:
        rows = _new_catches(fault)
        old = _old_catches(fault)
        print("%-42s new criterion fails %d of %d rows %s; old recipe %s" % (
            fault, len(rows), len(NEW_ROWS), [r[2] for r in rows], "catches it" if old else "LETS IT THROUGH"))
        assert rows, fault
        if not old:
            missed.append(fault)
    assert missed == OLD_RECIPE_MISSES
