"""The camera kernels (jt_camera.hip) at their launch edges, held element by element to the float64 oracle
(tests/camera_ref.py): pose composition, ray generation, and the ragged ray generation of batched test-time pose
optimisation with its written claim "a view's rays are bit-identical whether it is rendered alone or in a batch".

Launch arithmetic the rows rest on:
  k_pose_fwd / k_pose_bwd   one thread per view, 64 threads per block: B = 1, 63 | 64 (a full block) | 65 (a second block
                            with one live thread), 130 (three blocks).  gt_stride 12 (a pose per view) or 0 (one shared
                            [3,4] pose); noise present or nullptr.
  k_raygen_fwd              one thread per ray, 256 per block, B r threads: (5, 77) = 385 rays crosses a block edge inside
                            view 3; (3, 1025) = 3 075 rays is 13 blocks.
  k_raygen_bwd              one 256-thread workgroup per view; thread t sums rays t, t + 256, ...: r = 255 | 256 (every
                            thread one ray) | 257 (thread 0 takes a second trip), 1 025 (five trips for thread 0, four for
                            the rest); 63 | 64 | 65 is the edge of the first 64-lane wave (r = 1, 63: no full wave), and the
                            12 sums cross four waves through LDS.
  ragged                    view offsets [0, 0, 1, 257, 257, 514, 1539, 1539]: an empty first, middle and last view (the
                            bisection ragged_view must return the LAST view whose offset is <= t), one ray, 256, 257 and
                            1 025 rays; 1 539 rays are 7 forward blocks, and views 2, 4 and 5 straddle block edges.
Every row runs through ops.* (the autograd glue is covered) inside pinned_ref.guard_band(), with a cotangent that arrives
non-contiguous (applied through a transposed view) and intr_inv as torch.linalg.inv returns it (column-major: the
ops._contig_cached path).

Criteria (tests/camera_ref.py): gradients by kappa = max |G - T| / (2^-24 M), forward outputs by
|g - t| <= kappa_f 2^-24 (|t| + s).  The bounds are 4x what the float32 oracle on the CPU shows on the same inputs
(camera_ref.ORACLE32, asserted by tests/test_camera_ref.py), not fitted to the kernels; the kernels' measured worst values
are recorded in profiles/camera_loss_paths.txt."""
import pytest
import torch

from tests import camera_ref as C
from tests import pinned_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(t):
    return None if t is None else t.to(DEV)


def _transposed_dot(x, cot):
    """sum(x cot) with the product taken on a transposed view: the gradient that reaches x's producer is non-contiguous"""
    perm = tuple(reversed(range(x.dim())))
    return (x.permute(*perm) * cot.to(x.device).permute(*perm).contiguous()).sum()


@pytest.mark.parametrize("form", C.POSE_FORMS)
@pytest.mark.parametrize("B", C.POSE_B)
def test_pose_paths(B, form):
    from joint_tensorf_amd import ops
    se3, noise, gt, cot = C.pose_inputs(B, form)
    p64, s = C.pose_forward(se3, noise, gt)
    T, M = C.pose_terms(se3, noise, gt, cot)
    a = se3.to(DEV).requires_grad_(True)
    with P.guard_band() as guard:
        pose = ops.train_pose(a, _dev(noise), _dev(gt))
        _transposed_dot(pose, cot).backward()
        torch.cuda.synchronize()
    assert guard.violations() == []
    kf, kg = C.forward_error(pose, p64, s), C.kappa(a.grad, T, M)
    print("pose B=%d %s: kappa_f %.3f (bound %.3g)  kappa %.3f (bound %.3g)" % (B, form, kf, C.KAPPA["pose_fwd"], kg,
                                                                             C.KAPPA["pose_grad"]))
    assert kf <= C.KAPPA["pose_fwd"]
    assert kg <= C.KAPPA["pose_grad"]


def _run_raygen(ops, pose, intr, intr_inv, ray_idx, co, cd, ndc):
    p = pose.to(DEV).requires_grad_(True)
    ki = intr_inv.to(DEV)
    assert not ki.is_contiguous()
    with P.guard_band() as guard:
        o, d = ops.ray_gen(p, ki, intr.to(DEV), ray_idx.to(DEV), C.W, ndc=ndc, ndc_near=C.NEAR)
        (_transposed_dot(o, co) + _transposed_dot(d, cd)).backward()
        torch.cuda.synchronize()
    assert guard.violations() == []
    return o.detach(), d.detach(), p.grad.detach()


@pytest.mark.parametrize("ndc", [False, True], ids=["plain", "ndc"])
@pytest.mark.parametrize("B,r", C.RAYGEN_CASES)
def test_raygen_paths(B, r, ndc):
    from joint_tensorf_amd import ops
    pose, intr, intr_inv, ray_idx, co, cd = C.raygen_inputs(B, r, ndc)
    t_o, t_d, s_o, s_d = C.raygen_forward(pose, intr, intr_inv, ray_idx, ndc)
    T, M = C.raygen_terms(pose, intr, ray_idx, C.W, co, cd, ndc, intr_inv=intr_inv)
    o, d, g = _run_raygen(ops, pose, intr, intr_inv, ray_idx, co, cd, ndc)
    sfx = "_ndc" if ndc else ""
    ko, kd, kg = C.forward_error(o, t_o, s_o), C.forward_error(d, t_d, s_d), C.kappa(g, T, M)
    print("raygen B=%d r=%d ndc=%d: o %.3f (%.3g)  d %.3f (%.3g)  g_pose %.3f (%.3g)" % (
        B, r, ndc, ko, C.KAPPA["rays_o" + sfx], kd, C.KAPPA["rays_d" + sfx], kg, C.KAPPA["raygen_grad" + sfx]))
    assert ko <= C.KAPPA["rays_o" + sfx]
    assert kd <= C.KAPPA["rays_d" + sfx]
    assert kg <= C.KAPPA["raygen_grad" + sfx]


def test_raygen_follows_an_in_place_change_of_the_intrinsics():
    """ops._contig_cached remembers the contiguous copy of a column-major intr_inv per (tensor, version): a second call after
    an in-place change must compute with the new values, not the remembered copy"""
    from joint_tensorf_amd import ops
    pose, intr, intr_inv, ray_idx, co, cd = C.raygen_inputs(3, 65, False)
    p, ki, k, idx = pose.to(DEV), intr_inv.to(DEV), intr.to(DEV), ray_idx.to(DEV)
    assert not ki.is_contiguous()
    o1, d1 = ops.ray_gen(p, ki, k, idx, C.W)
    intr2 = intr.clone()
    intr2[:, 0, 0] *= 1.25
    intr2[:, 1, 2] += 3.0
    inv2 = torch.linalg.inv(intr2)
    ki.copy_(inv2.to(DEV))                        # in place: same tensor, same address, same strides, a new version
    assert not ki.is_contiguous()
    o2, d2 = ops.ray_gen(p, ki, k, idx, C.W)
    _, t1, _, s1 = C.raygen_forward(pose, intr, intr_inv, ray_idx, False)
    _, t2, _, s2 = C.raygen_forward(pose, intr2, inv2, ray_idx, False)
    assert float((t1 - t2).abs().max()) > 1e-2
    assert C.forward_error(d1, t1, s1) <= C.KAPPA["rays_d"]
    assert C.forward_error(d2, t2, s2) <= C.KAPPA["rays_d"]
    assert torch.equal(o1, o2)                    # the centres do not depend on the intrinsics


@pytest.mark.parametrize("ndc", [False, True], ids=["plain", "ndc"])
def test_raygen_ragged(ndc):
    """o, d and g_pose of the ragged launch view by view against the reference; an empty view's g_pose row exactly zero; and
    the kernels' written claim: ops.ray_gen on a view alone returns bit-identical o, d and g_pose."""
    from joint_tensorf_amd import ops
    pose, intr, intr_inv, ray_idx, voff, co, cd = C.ragged_inputs(ndc)
    t_o, t_d, s_o, s_d, T, M = C.ragged_terms(pose, intr, intr_inv, ray_idx, voff, co, cd, ndc)
    p = pose.to(DEV).requires_grad_(True)
    ki, k, idx = intr_inv.to(DEV), intr.to(DEV), ray_idx.to(DEV)
    with P.guard_band() as guard:
        o, d = ops.ray_gen_ragged(p, ki, k, idx, voff.to(DEV), C.W, ndc=ndc, ndc_near=C.NEAR)
        (_transposed_dot(o, co) + _transposed_dot(d, cd)).backward()
        torch.cuda.synchronize()
    assert guard.violations() == []
    g = p.grad.detach()
    sfx = "_ndc" if ndc else ""
    for b, a, e in C.ragged_views(voff):
        if a == e:
            assert bool((g[b] == 0).all()), b
            continue
        ko, kd = C.forward_error(o[a:e], t_o[a:e], s_o[a:e]), C.forward_error(d[a:e], t_d[a:e], s_d[a:e])
        kg = C.kappa(g[b], T[b], M[b])
        print("ragged ndc=%d view %d (%d rays): o %.3f  d %.3f  g_pose %.3f" % (ndc, b, e - a, ko, kd, kg))
        assert ko <= C.KAPPA["rays_o" + sfx], b
        assert kd <= C.KAPPA["rays_d" + sfx], b
        assert kg <= C.KAPPA["raygen_grad" + sfx], b
        # bit for bit the single-view launch
        o1, d1, g1 = _run_raygen(ops, pose[b:b + 1], intr[b:b + 1], intr_inv[b:b + 1], ray_idx[a:e], co[None, a:e],
                                 cd[None, a:e], ndc)
        assert torch.equal(o1[0], o[a:e].detach()), b
        assert torch.equal(d1[0], d[a:e].detach()), b
        assert torch.equal(g1[0], g[b]), b
