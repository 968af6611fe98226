"""The appearance forward k_shade_fwd<C, REC, B16> (jt_shade.hip) at the edges of its work split, for every record set on
both matrix-core paths, held to the pinned fp64 reference (tests/pinned_ref.py).

A forward launch cuts the n shaded samples into 32-sample tiles and gives each wave of a workgroup one tile at a time: four
waves per workgroup on the fp32 matrix cores, eight on the bf16 ones; ceil(tiles / waves) workgroups share the tiles
(xcd_share), the rest of the grid returns at once.  The scenes, rays and classes of n are those of
tests/test_gpu_wgrad_edges.py (without its two-chunk class: the forward is not chunked):
  half0       1..15           one tile, only lane half 0 holds live samples; every other wave of the workgroup has no tile
  partial     17..31          one partial tile across both lane halves
  onewave     33..128, odd    2..4 tiles, one workgroup with at most one tile per wave: on the bf16 path its upper waves are empty
  emptywaves  129..384        more tiles than one workgroup has waves and no multiple of them: a second, partly empty one
  blocks      513..4 096, odd many workgroups through xcd_share, a partial last tile
The class is asserted, with the tile conditions for the row's own number of waves.

Rows, for both scene kinds -- together all sixteen instantiations:
  mfma              REC 3 (lean tape), bf16        mfma-split8-fp32  REC 3, fp32
  mfma-fulltape     REC 1 (full tape), bf16        mfma-fp32         REC 1, fp32
  pose-mfma         REC 2 (pose-only), bf16        pose-mfma-fp32    REC 2, fp32
  infer-mfma        REC 0 (no records), bf16       infer-mfma-fp32   REC 0, fp32
infer-mfma on the 48-channel kind is the ping-pong loop (the waves of a SIMD take the gather and the compute step of their
tiles in opposite order, a workgroup barrier after every step): in onewave, emptywaves and blocks wave 0 has one tile more
than the upper waves of its workgroup, which go on meeting its barriers without one.

Every case asserts (1) the class, (2) that the profiler saw exactly one k_shade_fwd instantiation, with the row's REC and
B16, (3) rgb and opacity within TOL_VAL and depth within TOL_DEPTH (tests/test_gpu_scatter_shapes.py) of the reference
pinned to the run's own shading mask and ReLU sign words, no sign farther than 2e-5 from a tie -- an inference row leaves
no sign words: it is held, within the same bounds, to the training row of its matrix mode, scene kind and class (mfma,
mfma-fp32), which is held to the reference here -- and (4) for the pose-only rows that no kernel wrote past a buffer.
The tape itself (every record row) is what the backward of the training and pose-only rows reads: their gradients are
held to the same reference by test_gpu_wgrad_edges.py, test_gpu_scatter_shapes.py and test_gpu_pose_paths.py.
Measured on MI355X (n = 8, 24, 99, 282 and 2 045 in both scene kinds; profiles/shade_fwd_one_kernel.txt): rgb 1.7e-7, opacity
2.5e-7, depth 5.9e-7 at worst for every recording row, no ReLU sign decided differently by the reference, and the inference
rows equal to their training rows to the bit."""
import re

import pytest
import torch

from tests import pinned_ref as P
from tests.test_gpu_parity import kernel_variant
from tests.test_gpu_scatter_shapes import TOL_DEPTH, TOL_VAL
from tests.test_gpu_wgrad_edges import CLASSES, GRID

pytestmark = pytest.mark.gpu
DEV = "cuda"

# row: (kernel variant of tests/test_gpu_parity.py, what runs, REC, bf16 matrix cores)
ROWS = {
    "mfma": ("mfma", "train", 3, True),
    "mfma-fulltape": ("mfma-fulltape", "train", 1, True),
    "mfma-split8-fp32": ("mfma-split8-fp32", "train", 3, False),
    "mfma-fp32": ("mfma-fp32", "train", 1, False),
    "pose-mfma": ("mfma", "pose", 2, True),
    "pose-mfma-fp32": ("mfma-fp32", "pose", 2, False),
    "infer-mfma": ("mfma", "infer", 0, True),
    "infer-mfma-fp32": ("mfma-fp32", "infer", 0, False),
}
FWD_CLASSES = [c for c in CLASSES if c != "chunks"]
CASES = [(c, k, r) for c in FWD_CLASSES for k in ("blender", "llff") for r in ROWS]
CFG = {"blender": "jt::ShadeCfg<48, 27, 64, 0>", "llff": "jt::ShadeCfg<20, 20, 32, 1>"}


def forward_kernels(kernels):
    """the k_shade_fwd instantiations among the profiled device kernels, as `k_shade_fwd<config, REC, B16>`"""
    seen = set()
    for name in kernels:
        m = re.search(r"k_shade_fwd\w*<.*?>(?=\()", name + "(")   # up to the argument list, if the name carries one
        if m:
            seen.add(m.group(0))
    return seen


def check_class(cls, n, b16):
    lo, hi, odd = CLASSES[cls][:3]
    tiles, waves = (n + 31) // 32, 8 if b16 else 4
    assert lo <= n <= hi and (not odd or n % 32 != 0), (cls, n)
    if cls == "onewave":
        assert 2 <= tiles <= 4, (cls, n, tiles)
    if cls == "emptywaves":
        assert tiles > waves and tiles % waves != 0, (cls, n, tiles, waves)
    if cls == "blocks":
        assert tiles > 2 * waves, (cls, n, tiles, waves)


def run_infer(tf, o, d, S):
    """the forward alone under torch.no_grad() (P.run_hip's rays and sampling): outputs, shading mask, device kernels"""
    from torch.profiler import ProfilerActivity, profile as tprofile
    with torch.no_grad(), tprofile(activities=[ProfilerActivity.CUDA]) as prof:
        out = tf(None, o.to(DEV), d.to(DEV), white_bg=True, is_train=False, ndc_ray=False, N_samples=S)
        torch.cuda.synchronize()
    offset, _ = tf.last_render_cfg.shade_lists
    return dict(rgb=out[0].detach(), depth=out[1].detach(), opacity=out[2].detach(), n=int(offset[-1]),
                kernels=P._device_kernel_names(prof))


_REFS = {}    # (class, kind, what) -> (shading mask, ReLU signs, reference): shared by the rows that took the same decisions
_TRAIN = {}   # (class, kind, variant) -> outputs of a training row that passed its own check (the inference rows' yardstick)


def _scene(cls, kind):
    n_axial, n_oblique, S, seed = CLASSES[cls][3:]
    aabb = P.thin_box(GRID)
    o, d = P.ray_set(aabb, n_axial, n_oblique, 0, seed=seed)
    return P.build_scene(kind, GRID, aabb, DEV), o, d, S


def _reference(cls, kind, what, tf, hip, o, d, S):
    relu = [m.cpu() for m in hip["relu"]]
    mask = hip["shade_mask"].cpu()
    held = _REFS.get((cls, kind, what))
    if held is not None and torch.equal(held[0], mask) and all(torch.equal(a, b) for a, b in zip(held[1], relu)):
        return held[2]
    ref = P.run_reference(tf, kind, hip, o, d, S, ray_only=(what == "pose"))
    _REFS[(cls, kind, what)] = (mask, relu, ref)
    return ref


def _recorded_row(cls, kind, row):
    """a training or pose-only row against the pinned reference; returns (its outputs, n)"""
    variant, what, rec, b16 = ROWS[row]
    tf, o, d, S = _scene(cls, kind)
    with kernel_variant(variant):
        hip = P.run_hip(tf, o, d, S, profile=True, pose_only=(what == "pose"))
    n = int(hip["shade_mask"].sum())
    seen = forward_kernels(hip["kernels"])
    ref = _reference(cls, kind, what, tf, hip, o, d, S)
    vals = {k: float((hip[k].double().cpu() - ref[k]).abs().max()) for k in ("rgb", "opacity", "depth")}
    print("\n[shade-fwd] %s %s %s: n = %d (%d tiles); %s; relu %s; %s" % (
        cls, kind, row, n, (n + 31) // 32, " ".join("%s %.1e" % kv for kv in vals.items()), ref["relu"],
        " ".join(sorted(seen))))
    check_class(cls, n, b16)
    assert seen == {"k_shade_fwd<%s, %d, %s>" % (CFG[kind], rec, "true" if b16 else "false")}, sorted(seen)
    assert ref["relu"].get("max_abs", 0.0) <= 2e-5, ref["relu"]   # ReLU signs the reference decides differently: near-ties only
    for key, tol in (("rgb", TOL_VAL), ("opacity", TOL_VAL), ("depth", TOL_DEPTH)):
        assert vals[key] <= tol, (row, key, vals[key])
    if what == "pose":
        assert hip["overruns"] == [], hip["overruns"]
    return {k: hip[k].cpu() for k in ("rgb", "opacity", "depth")}, n


@pytest.mark.parametrize("cls,kind,row", CASES, ids=["-".join(c) for c in CASES])
def test_shade_fwd_edge(cls, kind, row):
    variant, what, rec, b16 = ROWS[row]
    if what != "infer":
        checked = _recorded_row(cls, kind, row)
        if what == "train":
            _TRAIN[(cls, kind, variant)] = checked
        return
    if (cls, kind, variant) not in _TRAIN:   # (a case that runs alone, or first: its yardstick is checked here)
        _TRAIN[(cls, kind, variant)] = _recorded_row(cls, kind, variant)
    train, n_train = _TRAIN[(cls, kind, variant)]
    tf, o, d, S = _scene(cls, kind)
    with kernel_variant(variant):
        got = run_infer(tf, o, d, S)
    seen = forward_kernels(got["kernels"])
    vals = {k: float((got[k].double().cpu() - train[k].double()).abs().max()) for k in ("rgb", "opacity", "depth")}
    print("\n[shade-fwd] %s %s %s: n = %d (%d tiles); against the training row: %s; %s" % (
        cls, kind, row, got["n"], (got["n"] + 31) // 32, " ".join("%s %.1e" % kv for kv in vals.items()),
        " ".join(sorted(seen))))
    check_class(cls, got["n"], b16)
    assert got["n"] == n_train, (got["n"], n_train)
    assert seen == {"k_shade_fwd<%s, 0, %s>" % (CFG[kind], "true" if b16 else "false")}, sorted(seen)
    for key, tol in (("rgb", TOL_VAL), ("opacity", TOL_VAL), ("depth", TOL_DEPTH)):
        assert vals[key] <= tol, (row, key, vals[key])
