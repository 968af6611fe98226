"""The render node (ops.RenderRays) as a sequence of library calls: which entry points one forward + backward goes through,
in which order, in every mode the node decides between -- and that each mode's gradients are the CPU oracle's.

  1. the four ways the regularisers' gradient reaches the factor gradients (trusted from the forward's fused launch, rewritten,
     written first, added last), each with TV on the colours on and off;
  2. a backward whose tape another forward has taken since: it records again, and the gradients are the same bits;
  3. the pose-only order;
  4. what the step timers record.

The ray batch is tests/test_gpu_edge.py's hand-made one (10 rays through the scene, 3 through a corner of the box)."""
import pytest
import torch

from oracle import tensorf_oracle as O
from tests.golden_util import Fixture
from tests.pinned_ref import deterministic
from tests.test_gpu_edge import _batch, _check_grads
from tests.test_gpu_parity import build_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPEC = [("hit", 10), ("graze", 3)]
# the render node's entry points (the spy also sees the loss head, the planners, ...)
NODE = {"jt_march_forward", "jt_march_forward_pose", "jt_shade_list", "jt_shade_forward", "jt_composite_forward",
        "jt_reg_losses_forward", "jt_reg_losses_fused", "jt_composite_backward", "jt_reg_losses_backward", "jt_shade_backward",
        "jt_march_backward", "jt_march_backward_pose"}
FORWARD = ["jt_march_forward", "jt_shade_list", "jt_shade_forward", "jt_composite_forward"]
# (L1, TV_density, TV_color): powers of two, large enough that on this 14^3 scene the regularisers' part of every density
# gradient (and of every appearance plane's, with TV on the colours) is a fifth or more of the whole: test_regulariser_legs
# asserts >= 0.1 from the oracle's two parts
WEIGHTS = (64.0, 32.0, 32.0)


class spy_calls:
    """with spy_calls() as seen: the names ops.check is handed, in order"""

    def __enter__(self):
        from joint_tensorf_amd import ops
        self.ops, self.orig, seen = ops, ops.check, []

        def spy(rc, what):
            seen.append(what)
            return self.orig(rc, what)
        ops.check = spy
        return seen

    def __exit__(self, *exc):
        self.ops.check = self.orig
        return False


def _node(seen):
    return [w for w in seen if w in NODE]


def _cotangents(shapes):
    g = torch.Generator().manual_seed(99)
    return [torch.randn(s, generator=g) for s in shapes]


_SEED = {}


def _unit_seed():
    from joint_tensorf_amd import ops
    if "t" not in _SEED:
        _SEED["t"] = ops.register_unit_seed(torch.ones((), device=DEV))
    return _SEED["t"]


_ORACLE = {}


def _oracle(fx, tv_app):
    """the oracle's parameters with .grad = d(render term + weighted regularisers), and the two parts by tensor name; computed
    once per weight set and left alone"""
    if tv_app not in _ORACLE:
        m = fx.meta
        o, d = _batch(SPEC, seed=3)
        params = fx.params()
        ref = O.render(fx.cfg(), params, o, d, m["N_samples"], white_bg=True)
        cot = _cotangents([ref[0].shape, ref[2].shape])
        render = (ref[0] * cot[0]).sum() + (ref[2] * cot[1]).sum()
        w_l1, w_tvd, w_tvc = WEIGHTS[0], WEIGHTS[1], WEIGHTS[2] if tv_app else 0.0
        reg = w_l1 * O.density_L1(params) + w_tvd * O.tv_planes(params["density_plane"]) \
            + w_tvc * O.tv_planes(params["app_plane"])
        names, leaves = zip(*O.flat_params(params))
        parts = []
        for term in (render, reg):
            gs = torch.autograd.grad(term, leaves, allow_unused=True)
            parts.append({n: torch.zeros_like(v) if g is None else g for n, v, g in zip(names, leaves, gs)})
        for n, v in zip(names, leaves):
            v.grad = parts[0][n] + parts[1][n]
        _ORACLE[tv_app] = (params, parts[0], parts[1])
    return _ORACLE[tv_app]


def _train_step(tf, fx, o, d, weights=None, hint=None):
    """one forward + loss + backward on the GPU; weights: the regularisers ride on the render node, and the loss is
    ops.loss_sum behind the registered unit seed (as Model.forward_backward forms it)"""
    from joint_tensorf_amd import ops
    m = fx.meta
    og, dg = o.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
    opt = None
    if weights is not None:
        opt = {"loss_weight": {"TV_density": weights[1], "TV_color": weights[2]}}
        if hint is not None:
            tf.reg_weights_hint = tuple(hint)
    out = tf(opt, og, dg, white_bg=True, is_train=False, ndc_ray=False, N_samples=m["N_samples"])
    cot = _cotangents([out[0].shape, out[2].shape])
    render = (out[0] * cot[0].to(DEV)).sum() + (out[2] * cot[1].to(DEV)).sum()
    if weights is None:
        return render, (og, dg)
    total = ops.loss_sum(render, tf._reg(), 1.0, *weights)
    ops.backward(total, _unit_seed())
    return total, (og, dg)


def _all_grads(tf, rays):
    """the twelve factor gradients, the basis', the MLP's six and the rays' two"""
    leaves = [p for grp in (tf.density_plane, tf.density_line, tf.app_plane, tf.app_line) for p in grp]
    leaves += [tf.basis_mat.weight] + list(tf.renderModule.weights()) + list(rays)
    return [p.grad.clone() for p in leaves]


# leg -> (reg_weights hint as a multiple of the weights or None, deterministic, statistics that move, forward's reg call,
#         the backward's calls)
LEGS = {
    "trusted": (1.0, False, "trusted", "jt_reg_losses_fused",
                ["jt_composite_backward", "jt_shade_backward", "jt_march_backward"]),
    "rewritten": (2.0, False, "rewritten", "jt_reg_losses_fused",
                  ["jt_composite_backward", "jt_reg_losses_backward", "jt_shade_backward", "jt_march_backward"]),
    "written-first": (None, False, None, "jt_reg_losses_forward",
                      ["jt_composite_backward", "jt_reg_losses_backward", "jt_shade_backward", "jt_march_backward"]),
    "added-last": (None, True, None, "jt_reg_losses_forward",
                   ["jt_composite_backward", "jt_shade_backward", "jt_march_backward", "jt_reg_losses_backward"]),
}


@pytest.mark.parametrize("tv_app", [True, False], ids=["tv-colours", "no-tv-colours"])
@pytest.mark.parametrize("leg", list(LEGS))
def test_regulariser_legs(leg, tv_app):
    from joint_tensorf_amd import ops
    hint_scale, det, stat, reg_fwd, bwd_calls = LEGS[leg]
    fx = Fixture("blender_train_mid")
    params, g_render, g_reg = _oracle(fx, tv_app)
    # the regularisers' gradient is a visible part of every gradient it reaches: dropped or doubled, it cannot pass 2e-3
    reached = ["density_plane.%d" % i for i in range(3)] + ["density_line.%d" % i for i in range(3)] \
        + (["app_plane.%d" % i for i in range(3)] if tv_app else [])
    for n in reached:
        whole = float((g_render[n] + g_reg[n]).abs().max())
        assert float(g_reg[n].abs().max()) >= 0.1 * whole > 0.0, (n, float(g_reg[n].abs().max()), whole)
    weights = (WEIGHTS[0], WEIGHTS[1], WEIGHTS[2] if tv_app else 0.0)
    hint = None if hint_scale is None else (weights[0] * hint_scale, weights[1], weights[2])
    tf = build_scene(fx, DEV, "mfma")
    o, d = _batch(SPEC, seed=3)
    before = dict(ops.REG_FUSION_STATS)
    with deterministic(det), spy_calls() as seen:
        _train_step(tf, fx, o, d, weights, hint)
    moved = {k: ops.REG_FUSION_STATS[k] - before[k] for k in before}
    assert moved == {k: int(k == stat) for k in before}, moved
    assert _node(seen) == FORWARD + [reg_fwd] + bwd_calls, _node(seen)
    _check_grads(tf, params)


def test_backward_records_again_when_another_forward_took_the_tape():
    """Forward A, forward B, backward of A: B's records lie in the shade workspace, so A's backward puts its own back
    (jt_shade_forward inside the backward) -- in deterministic mode to the same bits as without B."""
    from joint_tensorf_amd import ops
    fx = Fixture("blender_train_mid")
    o, d = _batch(SPEC, seed=3)
    o2, d2 = _batch(SPEC, seed=21)
    grads = {}
    with deterministic(True):
        for between in (False, True):
            tf = build_scene(fx, DEV, "mfma")
            loss, rays = _train_step(tf, fx, o, d)
            if between:
                _train_step(tf, fx, o2, d2)
            with spy_calls() as seen:
                ops.backward(loss)
            assert ("jt_shade_forward" in _node(seen)) == between, _node(seen)
            assert _node(seen)[0] == "jt_composite_backward" and _node(seen)[-1] == "jt_march_backward", _node(seen)
            grads[between] = _all_grads(tf, rays)
    assert len(grads[True]) == len(grads[False]) == 21
    for a, b in zip(grads[True], grads[False]):
        assert float(b.abs().max()) > 0.0 and torch.equal(a, b)


def test_pose_only_call_order():
    """only the rays want a gradient: the march's pose entry points both ways, no regulariser call, no jt_march_backward
    (the values: tests/test_gpu_edge.py)"""
    from joint_tensorf_amd import ops
    fx = Fixture("blender_train_mid")
    o, d = _batch(SPEC, seed=3)
    tf = build_scene(fx, DEV, "mfma")
    for p in tf.parameters():
        p.requires_grad_(False)
    with spy_calls() as seen:
        loss, rays = _train_step(tf, fx, o, d)
        ops.backward(loss)
    assert _node(seen) == ["jt_march_forward_pose", "jt_shade_list", "jt_shade_forward", "jt_composite_forward",
                           "jt_composite_backward", "jt_shade_backward", "jt_march_backward_pose"], _node(seen)
    assert all(torch.isfinite(r.grad).all() and float(r.grad.abs().max()) > 0.0 for r in rays)


@pytest.mark.parametrize("walk", [False, True], ids=["plain", "walk"])
def test_step_timers(walk):
    from joint_tensorf_amd import ops
    fx = Fixture("blender_train_mid")
    o, d = _batch(SPEC, seed=3)
    tf = build_scene(fx, DEV, "mfma")
    keep = ops.STEP_TIMERS, ops.STEP_TIMERS_WALK
    ops.STEP_TIMERS, ops.STEP_TIMERS_WALK = [], walk
    try:
        _train_step(tf, fx, o, d, (WEIGHTS[0], WEIGHTS[1], 0.0))
        torch.cuda.synchronize()
        timers = ops.STEP_TIMERS
    finally:
        ops.STEP_TIMERS, ops.STEP_TIMERS_WALK = keep
    forked = ops._use_aux(tf.last_render_cfg.scene())
    want = ["fwd"] + (["bwd_chain", "bwd_scatter", "bwd"] if forked else ["bwd"]) + (["march_bwd"] if walk else [])
    assert [t[0] for t in timers] == want, [t[0] for t in timers]
    for kind, start, end, tensor in timers:
        assert start.elapsed_time(end) >= 0.0, kind
        if kind == "march_bwd":
            assert tensor.numel() == 1 and 0 <= int(tensor.item()) <= o.shape[0] * fx.meta["N_samples"]
        else:
            assert tensor is tf.last_render_cfg.shade_lists[0]
