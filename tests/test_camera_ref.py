"""tests/camera_ref.py checked without a GPU: the helpers against plain autograd, and the float32 oracle against the float64
one on every input set tests/test_gpu_camera_paths.py uses -- the measurement the kernels' kappa bounds are 4x of.

Each family's worst fp32-oracle value must stay within HALF of the bound the kernels get (camera_ref.KAPPA = 4 x
camera_ref.ORACLE32), so a change to the inputs cannot quietly eat the kernels' margin."""
import math

import pytest
import torch

from oracle import tensorf_oracle as O
from tests import camera_ref as C


def test_kappa_rule():
    T = torch.tensor([1.0, 2.0, 0.0])
    M = torch.tensor([2.0, 2.0, 0.0])
    assert C.kappa(T.clone(), T, M) == 0.0
    G = T.clone()
    G[0] += 3 * C.EPS32 * 2.0
    assert abs(C.kappa(G, T, M) - 3.0) < 1e-6
    G = T.clone()
    G[2] = 1e-30                                   # where M == 0 the value must be exactly 0
    assert C.kappa(G, T, M) == float("inf")


def test_pose_inputs_hold_the_edge_rows():
    se3, noise, gt, _ = C.pose_inputs(130, "noise")
    th = se3[:, :3].double().norm(dim=-1)
    assert float(th[1]) == 0.0 and bool((se3[1, :3] == 0).all())
    assert abs(float(th[2]) - 1e-4) < 1e-10 and abs(float(th[3]) - 1.0) < 1e-6 and abs(float(th[0]) - 2.5) < 1e-6
    assert math.pi - 1e-5 < float(th[4]) <= math.pi and float(th.max()) <= math.pi
    assert float(se3[:, 3:].abs().max()) > 3.5
    assert C.pose_inputs(5, "no-noise")[1] is None and C.pose_inputs(5, "shared-gt")[2].shape == (3, 4)


@pytest.mark.parametrize("form", C.POSE_FORMS)
def test_pose_terms_vs_autograd(form):
    se3, noise, gt, cot = C.pose_inputs(65, form)
    T, M = C.pose_terms(se3, noise, gt, cot)
    a = se3.double().requires_grad_(True)
    (O.train_pose(a, None if noise is None else noise.double(), gt.double()) * cot.double()).sum().backward()
    assert float((T - a.grad).abs().max()) <= 1e-13 * float(M.max())
    assert bool((M >= T.abs() * (1 - 1e-12)).all()) and bool((M > 0).all())
    # M of one entry by hand: a one-hot cotangent gives |J| itself
    one = torch.zeros_like(cot)
    one[:, 1, 3] = 2.0
    T1, M1 = C.pose_terms(se3, noise, gt, one)
    assert torch.equal(M1, T1.abs())


@pytest.mark.parametrize("ndc", [False, True])
def test_raygen_terms_vs_autograd(ndc):
    pose, intr, intr_inv, ray_idx, co, cd = C.raygen_inputs(3, 257, ndc)
    assert int(ray_idx.min()) == 0 and int(ray_idx.max()) == C.H * C.W - 1 and ray_idx.unique().numel() < 257
    assert not intr_inv.is_contiguous()           # torch's batched inverse: column-major (ops._contig_cached's case)
    T, M = C.raygen_terms(pose, intr, ray_idx, C.W, co, cd, ndc, intr_inv=intr_inv)
    p = pose.double().requires_grad_(True)
    o, d = O.rays_for_pixels(p, intr_inv.double(), ray_idx, C.W)
    if ndc:
        o, d = O.convert_ndc(o, d, intr.double(), near=C.NEAR)
    ((o * co.double()).sum() + (d * cd.double()).sum()).backward()
    assert float(((T - p.grad).abs() / M).max()) <= 3e-14       # the per-ray contributions sum to the plain gradient
    assert bool((M >= T.abs() * (1 - 1e-12)).all())
    # the forward helper is the oracle, and its scales are positive
    o2, d2, so, sd = C.raygen_forward(pose, intr, intr_inv, ray_idx, ndc)
    assert torch.equal(o2, o.detach()) and torch.equal(d2, d.detach())
    assert float(so.min()) > 0 and float(sd.min()) > 0


def test_ragged_terms_are_the_views_own():
    pose, intr, intr_inv, ray_idx, voff, co, cd = C.ragged_inputs(False)
    assert voff.tolist() == [0, 0, 1, 257, 257, 514, 1539, 1539]
    o, d, so, sd, T, M = C.ragged_terms(pose, intr, intr_inv, ray_idx, voff, co, cd, False)
    assert o.shape == (1539, 3) and T.shape == (7, 3, 4)
    for b, a, e in C.ragged_views(voff):
        if a == e:
            assert bool((T[b] == 0).all()) and bool((M[b] == 0).all())
    b, a, e = C.ragged_views(voff)[4]
    T4, _ = C.raygen_terms(pose[4:5], intr[4:5], ray_idx[a:e], C.W, co[None, a:e], cd[None, a:e], False,
                           intr_inv=intr_inv[4:5])
    assert torch.equal(T4[0], T[4])


def _measure():
    """worst kappa / kappa_f of the float32 oracle per family, over every input set of the GPU tests"""
    worst = {k: (0.0, None) for k in C.ORACLE32}

    def note(k, v, where):
        if v > worst[k][0]:
            worst[k] = (v, where)
    for B in C.POSE_B:
        for form in C.POSE_FORMS:
            se3, noise, gt, cot = C.pose_inputs(B, form)
            p32, g32 = C.oracle32_pose(se3, noise, gt, cot)
            p64, s = C.pose_forward(se3, noise, gt)
            T, M = C.pose_terms(se3, noise, gt, cot)
            note("pose_fwd", C.forward_error(p32, p64, s), (B, form))
            note("pose_grad", C.kappa(g32, T, M), (B, form))
    for ndc in (False, True):
        sfx = "_ndc" if ndc else ""
        for B, r in C.RAYGEN_CASES:
            pose, intr, intr_inv, ray_idx, co, cd = C.raygen_inputs(B, r, ndc)
            o32, d32, g32 = C.oracle32_raygen(pose, intr, intr_inv, ray_idx, co, cd, ndc)
            o, d, so, sd = C.raygen_forward(pose, intr, intr_inv, ray_idx, ndc)
            T, M = C.raygen_terms(pose, intr, ray_idx, C.W, co, cd, ndc, intr_inv=intr_inv)
            note("rays_o" + sfx, C.forward_error(o32, o, so), (B, r))
            note("rays_d" + sfx, C.forward_error(d32, d, sd), (B, r))
            note("raygen_grad" + sfx, C.kappa(g32, T, M), (B, r))
        pose, intr, intr_inv, ray_idx, voff, co, cd = C.ragged_inputs(ndc)
        o, d, so, sd, T, M = C.ragged_terms(pose, intr, intr_inv, ray_idx, voff, co, cd, ndc)
        for b, a, e in C.ragged_views(voff):
            if a == e:
                continue
            o32, d32, g32 = C.oracle32_raygen(pose[b:b + 1], intr[b:b + 1], intr_inv[b:b + 1], ray_idx[a:e], co[None, a:e],
                                              cd[None, a:e], ndc)
            note("rays_o" + sfx, C.forward_error(o32[0], o[a:e], so[a:e]), ("ragged", b))
            note("rays_d" + sfx, C.forward_error(d32[0], d[a:e], sd[a:e]), ("ragged", b))
            note("raygen_grad" + sfx, C.kappa(g32[0], T[b], M[b]), ("ragged", b))
    return worst


def test_oracle32_kappa_table():
    worst = _measure()
    for k, (v, where) in worst.items():
        print("oracle32 %-16s %8.3f at %s   recorded %.3g, kernels' bound %.3g" % (k, v, where, C.ORACLE32[k], C.KAPPA[k]))
    for k, (v, where) in worst.items():
        assert C.KAPPA[k] == 4.0 * C.ORACLE32[k]
        assert v <= 0.5 * C.KAPPA[k], (k, v, where)          # the fp32 oracle keeps half of the kernels' margin free
