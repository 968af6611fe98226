"""What the render node (ops.RenderRays) decides, checked without a GPU.

RenderRays.forward / .backward execute a plan that a pure function forms from plain flags (ops.plan_render_forward,
ops.plan_render_backward).  Here:

  1. the backward plan over the full cross product of its inputs against a frozen restatement of the branch logic that
     RenderRays.backward had while it still decided as it launched -- written from that source, branch for branch, in its
     order: every case gives an equal plan or the same error;
  2. the same for the forward plan;
  3. the Python restatement of the march backward's workspace layout (ops.march_bwd_counts_offset: where the per-ray counts
     sit), extended by the two blocks behind the counts, against jt_march_backward_workspace_bytes."""
import itertools

import pytest

from joint_tensorf_amd import ops
from joint_tensorf_amd._lib import lib
from tests.test_launch_plan import thin_scene

BOOLS = (False, True)
DET_ERROR = "JT_DETERMINISTIC is a single-process debugging mode"
DP_ERROR = "data-parallel render backward needs the fused path with all scene gradients wanted"
REG_ERROR = "regulariser gradient wanted without factor gradients"


# ---- the restatement: RenderRays.backward before the plan, with every launch replaced by a note of it --------------------------
def old_backward(want_fac, want_mlp, det, dp_on, has_reg, tv_app, has_g_reg, hint_holds, pre, use_aux, adam_early, capturing,
                 kept_dfeat, timers_on, timers_walk):
    """ctx.reg is not None = has_reg (ctx.reg[4] = tv_app), g_reg is not None = has_g_reg, _reg_hint_holds(..) = hint_holds,
    ctx.pre = None or (.., pre), ctx.dfeat_dn is not None = kept_dfeat; ctx.pose_only = nothing but the rays wants a gradient"""
    did = dict(buffers=None, groups=0, unzeroed=(), reg_before=None, reg_after=False, mlp=None, early=False, timers=[],
               walk_timed=False)
    pose_only = not (want_fac or want_mlp)
    fused_mlp_zero = want_fac and want_mlp
    reg_first = False
    if det and want_fac:
        if dp_on:
            raise RuntimeError(DET_ERROR)
        did.update(buffers="shadow", groups=4)          # _zeros_flat([sdp, sdl, sap, sal]) + the int64 shadow
        fused_mlp_zero = False
    elif want_fac and pre is not None and pre == fused_mlp_zero:
        did.update(buffers="forward")
        reg_first = True
        if not hint_holds:
            did.update(reg_before="overwrite")          # accumulate 0, REG_FUSION_STATS["rewritten"]
        else:
            did.update(reg_before="trusted")
    elif want_fac:
        reg_first = has_reg and has_g_reg and not dp_on
        skip = ((0, 1, 2) if tv_app else (0, 1)) if reg_first else ()
        did.update(buffers="fresh", groups=5 if fused_mlp_zero else 4, unzeroed=skip)
        if reg_first:
            did.update(reg_before="write")              # accumulate 0
    gfac_is_none = not want_fac
    dp = dp_on and fused_mlp_zero
    if dp_on and not dp and (want_fac or want_mlp):
        raise RuntimeError(DP_ERROR)
    if want_mlp:
        did.update(mlp="carved" if fused_mlp_zero else "zeros")
    forked = use_aux and want_mlp                       # h_aux[0] is not None
    if timers_on and not pose_only:
        if forked:
            did["timers"] += ["bwd_chain", "bwd_scatter"]
        did["timers"].append("bwd")
    # jt_shade_backward
    if dp:
        pass                                            # reducer.reduce(2, 3)
    elif (adam_early and want_fac and not det and use_aux and (reg_first or not has_reg or not has_g_reg) and not capturing):
        did.update(early=True)
    did.update(walk_timed=timers_on and timers_walk and not pose_only)
    march_pose = kept_dfeat and gfac_is_none
    # jt_march_backward(_pose), the collectives, the join, the fixed-point conversion
    if reg_first:
        pass
    elif has_reg and has_g_reg and want_fac:
        did.update(reg_after=True)                      # accumulate 1
    elif has_reg and has_g_reg:
        raise RuntimeError(REG_ERROR)
    return ops.BackwardPlan(dp=dp, fork=forked, march_pose=march_pose, **dict(did, timers=tuple(did["timers"])))


def old_forward(grad_enabled, wants_any, wants_scene, wants_reg_factors, want_mlp, pose_march, det, oversize, capturing,
                timers_on, has_reg, has_hint, tv_app, dp_on):
    recording = grad_enabled and wants_any
    pose_only = recording and not wants_scene
    keep = False
    if pose_only and pose_march and not det:
        keep = True                                     # jt_march_forward_pose
    sync = False
    if oversize and not capturing:
        sync = True
    timed = timers_on and recording                     # (ws_args[0] is not None)
    reg, reg_mlp, unzeroed = None, False, ()
    if has_reg:
        if has_hint and wants_reg_factors and not dp_on and not det:
            reg, reg_mlp, unzeroed = "fused", want_mlp, (0, 1, 2) if tv_app else (0, 1)
        else:
            reg = "value"
    return ops.ForwardPlan(recording, pose_only, keep, sync, timed, reg, reg_mlp, unzeroed)


def _outcome(fn, *args):
    try:
        return fn(*args)
    except RuntimeError as e:
        return str(e)


def test_backward_plan_is_the_old_branch_logic_in_every_case():
    plans, raising, cases, plain = set(), 0, 0, [0, 0, set()]
    for flags in itertools.product(BOOLS, repeat=14):
        (want_fac, want_mlp, det, dp_on, has_reg, tv_app, has_g_reg, hint_holds, use_aux, adam_early, capturing, kept_dfeat,
         timers_on, timers_walk) = flags
        for pre in (None, False, True):
            if pre is not None and not has_reg:
                continue                                # (buffers of the fused regulariser launch without regularisers)
            args = (want_fac, want_mlp, det, dp_on, has_reg, tv_app, has_g_reg, hint_holds, pre, use_aux, adam_early,
                    capturing, kept_dfeat, timers_on, timers_walk)
            want, got = _outcome(old_backward, *args), _outcome(ops.plan_render_backward, *args)
            assert type(got) is type(want) and got == want, (args, want, got)
            cases += 1
            raising += isinstance(got, str)
            plans.add(got)
            if not timers_on and not timers_walk:       # the twelve flags + pre alone
                plain[0] += 1
                plain[1] += isinstance(got, str)
                plain[2].add(got)
    errors = {p for p in plans if isinstance(p, str)}
    assert errors == {DET_ERROR, DP_ERROR, REG_ERROR}
    print("\n[render plan] backward: %d cases, %d raise, %d distinct plans; timers off: %d cases, %d raise, %d distinct plans"
          % (cases, raising, len(plans - errors), plain[0], plain[1], len(plain[2] - errors)))
    assert cases == 4 * 8192 and plain[0] == 8192
    # every leg is there
    legs = {(p.buffers, p.reg_before, p.reg_after) for p in plans - errors}
    assert legs >= {("forward", "trusted", False), ("forward", "overwrite", False), ("fresh", "write", False),
                    ("fresh", None, True), ("fresh", None, False), ("shadow", None, True), ("shadow", None, False),
                    (None, None, False)}


def test_backward_plan_oddities_kept():
    base = dict(want_fac=True, want_mlp=True, det=False, dp_on=False, has_reg=True, tv_app=True, has_g_reg=True,
                hint_holds=True, pre=True, use_aux=True, adam_early=True, capturing=False, kept_dfeat=False)
    p = ops.plan_render_backward(**base)
    assert (p.buffers, p.reg_before, p.mlp, p.early, p.fork) == ("forward", "trusted", "carved", True, True)
    # a forward whose buffers were made for another set of gradients: fresh ones, the regularisers written first
    p = ops.plan_render_backward(**dict(base, pre=False))
    assert (p.buffers, p.groups, p.unzeroed, p.reg_before) == ("fresh", 5, (0, 1, 2), "write")
    # a deterministic backward ignores the forward's buffers and adds the regularisers last
    p = ops.plan_render_backward(**dict(base, det=True))
    assert (p.buffers, p.groups, p.reg_before, p.reg_after, p.mlp, p.early) == ("shadow", 4, None, True, "zeros", False)
    # the early offer looks at use_aux, not at the fork
    p = ops.plan_render_backward(**dict(base, want_mlp=False, pre=False))
    assert p.early and not p.fork
    with pytest.raises(RuntimeError, match="single-process"):
        ops.plan_render_backward(**dict(base, det=True, dp_on=True))
    with pytest.raises(RuntimeError, match="data-parallel"):
        ops.plan_render_backward(**dict(base, dp_on=True, want_mlp=False, pre=None))
    with pytest.raises(RuntimeError, match="without factor gradients"):
        ops.plan_render_backward(**dict(base, want_fac=False, pre=None))


def test_forward_plan_is_the_old_branch_logic_in_every_case():
    plans = set()
    for flags in itertools.product(BOOLS, repeat=14):
        want, got = old_forward(*flags), ops.plan_render_forward(*flags)
        assert got == want, (flags, want, got)
        plans.add(got)
    assert {p.reg for p in plans} == {None, "value", "fused"}
    print("\n[render plan] forward: %d cases, %d distinct plans" % (2 ** 14, len(plans)))


def test_plans_are_pure():
    """no module global, no torch, no library: the only names the two functions resolve outside their arguments"""
    assert set(ops.plan_render_forward.__code__.co_names) <= {"ForwardPlan", "_reg_covered"}
    assert set(ops.plan_render_backward.__code__.co_names) <= {"BackwardPlan", "_reg_covered", "RuntimeError"}
    assert set(ops._reg_covered.__code__.co_names) == set()
    assert not hasattr(ops, "FUSE_REG_GRADIENT")


@pytest.mark.parametrize("S", [1, 7, 64, 221, 443, 1000, 1024])
def test_march_backward_workspace_restatement(S):
    def align256(v):
        return (v + 255) // 256 * 256
    scene = thin_scene("blender", 33, S=S)
    for R in (1, 2, 13, 63, 64, 65, 1995, 62500):
        o = ops.march_bwd_counts_offset(R, S)
        assert o == align256(align256(4 * R * S) + 2 * R * S)
        assert align256(align256(o + 4 * R) + 48 * R) == lib.jt_march_backward_workspace_bytes(scene, R), (R, S)
