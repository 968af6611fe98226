"""JT_SCATTER_CLAIM: how the twelve-wave k_shade_scatter hands its batches of 32 shaded samples to its waves -- 0 every
twelfth batch of the workgroup's share per wave, 1 drawn from a counter per workgroup.
Whatever the split, every batch is scattered exactly once: factor gradients, dBasis and the ray gradients against the
float64 reference of tests/pinned_ref.py, at the tolerances of tests/test_gpu_scatter_shapes.py (its _check_row, which
also holds the profiled kernel names to the plan's).

The knob is read once per process, so each mode runs in a fresh child (this file as a script).  The scene is the thin
VM-48 box of test_gpu_scatter_shapes.py at L = 441, the longest line beside which the twelve-wave shape's LDS fits.  The
rays run along the long axis with S = 40 samples each -- 39 shaded: a ray's last sample has no length -- plus one ray that
leaves the box early: the shaded-sample counts are
  5                 one partial batch: eleven waves of the one workgroup claim nothing
  32 * 12 - 1, + 1  one round of a workgroup, and one batch into the second
  32 * 12 * 9 + 5   more than eight workgroups: every XCD label has work, and the labels' shares differ by one batch
  7 * 99            seven rays of 100 samples: batches that span a ray boundary (as do all the S = 40 counts above)
The rays of a count are picked from a pool by the shaded counts a forward pass over the pool reports.

Deterministic mode keeps the fixed split whatever the knob says (its dBasis sum has a fixed order): two launches are
bit-identical, and bit-identical to tests/golden/scatter_claim_det.pt, recorded with the library as it was before the
knob existed (`python tests/test_gpu_scatter_claim.py record FILE`)."""
import hashlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scatter_claim_det.pt")
pytestmark = pytest.mark.gpu

L, S = 441, 40
GRID = [12, 9, L]
COUNTS = [5, 32 * 12 - 1, 32 * 12 + 1, 32 * 12 * 9 + 5]
SPAN = (7, 100)        # rays x samples of the ray-boundary case
N_FULL, DET_COUNT = 90, 32 * 12 + 1


def _pool(P, aabb):
    """N_FULL rays along +z from in front of the end face (S samples in the box each), and S - 1 rays along +z from
    inside the box that leave it after nominally 1 .. S - 1 samples (near = 0.5, half-texel steps)"""
    import torch
    o, d = P.ray_set(aabb, N_FULL, 0, 0, seed=L)
    step = P.UNIT * 0.5
    os_ = o[:S - 1].clone()
    for k in range(1, S):
        os_[k - 1, 2] = aabb[5] - 0.5 - (k - 0.5) * step
    return torch.cat([o, os_]).contiguous(), torch.cat([d, d[:S - 1]]).contiguous()


def _shaded_counts(tf, o, d, n_samples):
    import torch
    with torch.no_grad():
        tf(None, o.cuda(), d.cuda(), white_bg=True, is_train=False, ndc_ray=False, N_samples=n_samples)
    offset = tf.last_render_cfg.shade_lists[0]
    return (offset[1:] - offset[:-1]).long().cpu()


def _pick(o, d, cnt, n):
    """rays of the pool with n shaded samples in all: full rays, then one ray with the remainder"""
    import torch
    per = int(cnt[:N_FULL].max())
    assert 32 < per <= S, cnt[:N_FULL].tolist()
    full = (cnt[:N_FULL] == per).nonzero()[:, 0]
    q, r = divmod(n, per)
    assert q <= len(full), (n, per, len(full))
    idx = full[:q].tolist()
    if r:
        short = ((cnt == r) & (torch.arange(len(cnt)) >= N_FULL)).nonzero()[:, 0]
        assert len(short), ("no ray of the pool has %d shaded samples" % r, cnt[N_FULL:].tolist())
        idx.append(int(short[0]))
    return o[idx].contiguous(), d[idx].contiguous()


def _hash(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _det_run(P, aabb, o, d):
    """deterministic mode, two launches: {name: sha256} of every gradient, and the dBasis gradient itself"""
    import torch
    tf = P.build_scene("blender", GRID, aabb, "cuda")
    with P.deterministic(True):
        a = P.run_hip(tf, o, d, S, profile=True)
        b = P.run_hip(tf, o, d, S)
    assert int(a["shade_mask"].sum()) == DET_COUNT
    assert any("k_shade_scatter<jt::ShadeCfg<48, 27, 64, 0>, true" in n for n in a["kernels"]), sorted(a["kernels"])
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), n
    for n in ("g_o", "g_d"):
        assert torch.equal(a[n], b[n]), n
    h = {n: _hash(g) for n, g in a["grads"].items()}
    h["g_o"], h["g_d"] = _hash(a["g_o"]), _hash(a["g_d"])
    return h, a["grads"]["basis_mat.weight"].cpu()


def child(mode):
    sys.path.insert(0, ROOT)
    import torch
    from tests import pinned_ref as P
    aabb = P.thin_box(GRID)
    o, d = _pool(P, aabb)
    tf = P.build_scene("blender", GRID, aabb, "cuda")
    cnt = _shaded_counts(tf, o, d, S)
    if mode == "record":
        h, db = _det_run(P, aabb, *_pick(o, d, cnt, DET_COUNT))
        torch.save({"sha256": h, "dbasis": db}, sys.argv[2])
        return
    if mode == "det":
        h, db = _det_run(P, aabb, *_pick(o, d, cnt, DET_COUNT))
        gold = torch.load(GOLDEN)
        assert torch.equal(db, gold["dbasis"]), float((db - gold["dbasis"]).abs().max())
        assert h == gold["sha256"], sorted(n for n in h if h[n] != gold["sha256"][n])
        return
    from tests.test_gpu_scatter_shapes import SC48, _check_row
    expect = [SC48 + "false, 8, 12, 3>"]
    for n in COUNTS:
        oo, dd = _pick(o, d, cnt, n)
        hip, _ = _check_row("claim%s-n%d" % (mode, n), "blender", GRID, aabb, oo, dd, S, expect=expect, long_line=False)
        assert int(hip["shade_mask"].sum()) == n, (n, int(hip["shade_mask"].sum()))
    cnt2 = _shaded_counts(tf, o[:SPAN[0]], d[:SPAN[0]], SPAN[1])
    assert cnt2.tolist() == [SPAN[1] - 1] * SPAN[0], cnt2.tolist()
    _check_row("claim%s-span" % mode, "blender", GRID, aabb, o[:SPAN[0]].contiguous(), d[:SPAN[0]].contiguous(), SPAN[1],
               expect=expect, long_line=False)


def _run_child(mode, claim):
    env = dict(os.environ, JT_SCATTER_CLAIM=str(claim))
    for k in ("JT_SCATTER_WAVES", "JT_SCATTER_WGS", "JT_SCATTER_FLAGS", "JT_BWD_SPLIT", "JT_LEAN_TAPE", "JT_DETERMINISTIC",
              "JT_BF16X3", "JT_ABLATE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("claim", [0, 1])
def test_claim_mode(claim):
    _run_child(str(claim), claim)


@pytest.mark.parametrize("claim", [0, 1])
def test_deterministic_keeps_the_fixed_split(claim):
    _run_child("det", claim)


if __name__ == "__main__":
    child(sys.argv[1])
