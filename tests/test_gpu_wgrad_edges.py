"""The weight-gradient GEMM k_wgrad<MT, NT, XF, XA, B16> (jt_shade.hip) at the edges of its work split, on both matrix-core
paths, held to the pinned fp64 reference (tests/pinned_ref.py).

A GEMM launch splits the n shaded samples of a backward chunk into 32-sample tiles, gives every wave of a four-wave workgroup
max(ceil(tiles / 2 048), 4) consecutive tiles, and only the workgroups that get a tile write a slab.  Each case is one forward
plus backward on a thin scene whose rays and sample count S put n into one class of that split:
  half0       1..15           one tile, only lane half 0 holds live samples; three of the four waves have no tile and still
                              take part in the epilogue's barriers
  partial     17..31          one partial tile across both lane halves
  onewave     33..128, odd    one wave, several tiles: the look-ahead load and a partial last tile ("odd": n % 32 != 0)
  emptywaves  129..384        some waves of the one active workgroup have no tile
  blocks      513..4 096, odd several active workgroups, the others return at once; the slab sum runs over the active ones only
  chunks      2^16 < n < 2^17 two backward chunks of 2^16 entries: a non-zero chunk_start, and the slab sum across chunks
(n = 0 is tests/test_gpu_edge.py's, more than four tiles per wave the full-size and parity suites'.)  The rays are a bundle
along the long axis -- each ray contributes exactly min(S, 143) shaded samples -- plus oblique rays, which contribute 0..S
each and give the view-direction columns of dW1 something to sum: the class bounds hold for any outcome of the oblique
rays except the two "odd" conditions, which the seeds were chosen for.  The class is asserted.

Variants, for both scene kinds: mfma (bf16 matrix cores, G2 derived, three GEMMs), mfma-fulltape (bf16, G2 recorded, four
GEMMs), mfma-split8-fp32 (fp32, G2 derived) and mfma-fp32 (fp32, G2 recorded, four GEMMs) -- together all sixteen
instantiations.  Every case asserts that the profiler saw exactly the GEMM instantiations of its variant, and that the
basis and the six MLP gradients are within DENSE_TOL (tests/test_gpu_scatter_shapes.py: 5e-5, measured 7.9e-6) of the
reference (measured here on MI355X: 1.5e-6 at worst, n = 8, 24, 99, 282, 2 045 and 90 049; profiles/wgrad_one_kernel.txt)."""
import re

import pytest
import torch

from tests import pinned_ref as P
from tests.test_gpu_parity import kernel_variant
from tests.test_gpu_scatter_shapes import DENSE_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRID = [11, 9, 72]   # 143 in-box samples on a ray along z

# class: (smallest n, largest n, n % 32 != 0 required, rays along z, oblique rays, S, seed)
CLASSES = {
    "half0": (1, 15, False, 2, 2, 3, 1),                  # 6 + 0..6
    "partial": (17, 31, False, 4, 2, 5, 2),               # 20 + 0..10
    "onewave": (33, 128, True, 6, 5, 10, 3),              # 60 + 0..50
    "emptywaves": (129, 384, False, 8, 8, 20, 4),         # 160 + 0..160
    "blocks": (513, 4096, True, 30, 40, 40, 5),           # 1 200 + 0..1 600
    "chunks": (65537, 131071, False, 600, 200, 143, 6),   # 85 800 + 0..28 600
}
# variant: (bf16 matrix cores, G2 derived and dBasis out of the scatter: three GEMMs)
VARIANTS = {"mfma": (True, True), "mfma-fulltape": (True, False), "mfma-split8-fp32": (False, True), "mfma-fp32": (False, False)}
CASES = [(c, k, v) for c in CLASSES for k in ("blender", "llff") for v in VARIANTS
         if c != "chunks" or v in ("mfma", "mfma-fp32")]


def gemm_name(mt, nt, xf, xa, b16):
    return "k_wgrad<%d, %d, %d, %d, %s>" % (mt, nt, xf, xa, "true" if b16 else "false")


def expected_gemms(kind, variant):
    """dW3, dW2, dW1 and (full tape) dBasis of launch_wgrad for the scene kind: hidden-layer tiles, layer-1 input form, basis tiles"""
    b16, lean = VARIANTS[variant]
    mt, xf1, ntb = (2, 1, 5) if kind == "blender" else (1, 2, 2)
    names = {gemm_name(1, 2, 0, 0, b16), gemm_name(mt, mt, 0, 1 if lean else 0, b16), gemm_name(mt, 5, xf1, 0, b16)}
    if not lean:
        names.add(gemm_name(1, ntb, 0, 0, b16))
    return names


_REFS = {}   # (class, kind) -> (shading mask, ReLU signs, reference): shared by the variants that took the same decisions
#              (kept only to save time: a case that runs alone, or first, computes its own reference)


def _reference(cls, kind, tf, hip, o, d, S):
    relu = [m.cpu() for m in hip["relu"]]
    mask = hip["shade_mask"].cpu()
    held = _REFS.get((cls, kind))
    if held is not None and torch.equal(held[0], mask) and all(torch.equal(a, b) for a, b in zip(held[1], relu)):
        return held[2]
    ref = P.run_reference(tf, kind, hip, o, d, S)
    _REFS[(cls, kind)] = (mask, relu, ref)
    return ref


@pytest.mark.parametrize("cls,kind,variant", CASES, ids=["-".join(c) for c in CASES])
def test_wgrad_edge(cls, kind, variant):
    from joint_tensorf_amd._lib import lib
    lo, hi, odd, n_axial, n_oblique, S, seed = CLASSES[cls]
    aabb = P.thin_box(GRID)
    o, d = P.ray_set(aabb, n_axial, n_oblique, 0, seed=seed)
    tf = P.build_scene(kind, GRID, aabb, DEV)
    prev = lib.jt_shade_set_chunk_log2(16) if cls == "chunks" else None
    try:
        with kernel_variant(variant):
            hip = P.run_hip(tf, o, d, S, profile=True)
    finally:
        if prev is not None:
            lib.jt_shade_set_chunk_log2(prev)
    n = int(hip["shade_mask"].sum())
    seen = set()
    for name in hip["kernels"]:
        m = re.search(r"k_wgrad\w*<[^>]*>", name)
        if m and not m.group(0).startswith("k_wgrad_reduce"):
            seen.add(m.group(0))
    ref = _reference(cls, kind, tf, hip, o, d, S)
    dense = {k: P.max_rel(hip["grads"][k].cpu(), ref["T"][k]) for k in P.DENSE}
    print("\n[wgrad] %s %s %s: n = %d (%d tiles), worst %.1e; %s; GEMMs: %s" % (
        cls, kind, variant, n, (n + 31) // 32, max(dense.values()), " ".join("%s %.1e" % kv for kv in dense.items()),
        " ".join(sorted(seen))))
    assert lo <= n <= hi and (not odd or n % 32 != 0), (cls, n)
    assert seen == expected_gemms(kind, variant), (sorted(seen), sorted(expected_gemms(kind, variant)))
    assert ref["relu"].get("max_abs", 0.0) <= 2e-5, ref["relu"]   # ReLU signs the reference decides differently: near-ties only
    assert all(v <= DENSE_TOL for v in dense.values()), dense
