"""Which kernels the two shape-dependent backward launchers pick, checked without a GPU.

jt_shade_backward and jt_march_backward execute a plan that a pure function forms from the library's switches, the chip
geometry and the scene (plan_shade_bwd<C> in jt_shade.hip, plan_march_bwd in jt_march.hip); jt_shade_backward_plan and
jt_march_backward_plan report that plan and need no device.  Here:

  1. every row of tests/test_gpu_scatter_shapes.py ROWS and the pose-only expectations of tests/test_gpu_pose_paths.py:
     the kernel names formed from the plan are the names those rows saw run on a GPU;
  2. a sweep of both scene kinds over L = 2 .. 1300 against a restatement, written here from the budget arithmetic in the
     docstring of tests/test_gpu_scatter_shapes.py (and jt_tile.h's tile_lds_bytes for the tile-owned variant), which first
     has to reproduce every ROWS name itself;
  3. the tape: plan, jt_shade_record_layout and jt_shade_workspace_layout agree under every mode;
  4. the environment-only switches bench.py --full depends on, each in a fresh process (they are read once);
  5. ops._use_aux against the rule it used to restate.

Without a device the chip geometry is MI355X's (256 compute units, 8 XCDs), which the workgroup counts below assume."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from joint_tensorf_amd import _lib
from joint_tensorf_amd._lib import JtScene, lib
from tests.test_gpu_parity import VARIANTS, kernel_variant
from tests.test_gpu_pose_paths import C20, C48, GATHER
from tests.test_gpu_scatter_shapes import ROWS, SC20, SC48, SHORT, WALK

LDS_BUDGET = 163840
KINDS = {"blender": (48, 27, 64, _lib.JT_MLP_FEA), "llff": (20, 20, 32, _lib.JT_MLP_WEAKVIEW)}
CHAINS = {0: "k_shade_bwd<%s, false>", 1: "k_shade_bwd<%s, true>", 2: "k_shade_bwd<%s, false, true>",
          3: "k_shade_bwd<%s, false, true, true>"}
TRAIN, POSE = (1, 1), (0, 0)    # (factor gradients, MLP gradients) wanted


def thin_scene(kind, L, cd=16, S=None, short=SHORT):
    """the JtScene of tests/pinned_ref.py's thin scenes: grid (short[0], short[1], L), the long axis is line 0"""
    ca, app_dim, hid, mlp = KINDS[kind]
    grid = (short[0], short[1], L)
    s = JtScene()
    for a in range(3):
        s.aabb_lo[a], s.aabb_hi[a] = -1.0, 1.0
        s.plane_h[a], s.plane_w[a] = grid[(1, 2, 2)[a]], grid[(0, 0, 1)[a]]
        s.line_len[a] = grid[2 - a]
    s.n_comp_density, s.n_comp_app, s.app_dim, s.mlp_hidden, s.mlp_kind = cd, ca, app_dim, hid, mlp
    s.view_pe = s.fea_pe = 2
    s.n_samples = S if S is not None else 2 * (L - 1) + 9
    return s


def shade_plan(scene, want=TRAIN, have_aux=1, flags=0):
    out = (ctypes.c_int32 * 16)()
    rc = lib.jt_shade_backward_plan(scene, want[0], want[1], flags, have_aux, out)
    assert rc == 0, rc
    return list(out)


def march_plan(scene, n_rays, want_fac=1, have_dfeat=0):
    out = (ctypes.c_int32 * 8)()
    rc = lib.jt_march_backward_plan(scene, n_rays, want_fac, have_dfeat, out)
    assert rc == 0, rc
    return list(out)


def _b(v):
    return "true" if v else "false"


def scatter_name(kind, p):
    """k_shade_scatter<C, DET, RUN, WAVES, FLAGS> of a shade plan, or None when the second kernel is another one"""
    return None if p[3] != 1 else (SC48 if kind == "blender" else SC20) + "%s, %d, %d, %d>" % (_b(p[4]), p[5], p[6], p[7])


def walk_name(cd, det, m):
    return None if not m[1] else WALK + "%d, %s, %d, %d>" % (cd, _b(det), m[3], m[4])


class deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = lib.jt_set_deterministic(1 if self.on else 0)

    def __exit__(self, *exc):
        lib.jt_set_deterministic(self.prev)
        return False


# ---- the restatement: tests/test_gpu_scatter_shapes.py's budget arithmetic, as Python -----------------------------------------
# ScatCfg<C>: channels, floats of the basis^T image, floats of the dBasis sum; tile-owned scatter: 8 L Ca + 8 x 896 bytes
SCAT = {"blender": (48, 1344, 1536), "llff": (20, 640, 640)}


def scatter_lds(kind, L, run, fl, sw, dbs):
    ca, bt, red = SCAT[kind]
    return 4 * (bt + (fl & 1) * L * ca + (red if dbs else 0) + sw * (4 * run * (4 + 4 + 20) + (512 if dbs else 0)))


def restate_shade(kind, L, det, variant, want):
    """(chain id, second id, scatter name or None, lean, GEMMs per chunk) under the default environment"""
    mode, split_knob, lean_knob = VARIANTS[variant]
    ca = SCAT[kind][0]
    default = 16 if (ca < 48 or mode & 4) else 0
    req = split_knob if split_knob >= 0 else default
    lean = bool(lean_knob) and req in (8, 16)
    want_fac, want_mlp = want
    split = req
    if split == 1 and (det or not want_fac or 8 * L * ca + 8 * 896 > LDS_BUDGET):
        split = default
    pose_only = not det and not want_fac and not want_mlp
    if pose_only:
        split = 16
    dbs = lean and not pose_only and bool(want_mlp)
    gemms = 0 if not want_mlp else (3 if dbs else 4)
    chain = (3 if mode & 4 else 2) if split else (1 if det else 0)
    if split == 0:
        return chain, 0, None, lean, gemms
    if pose_only:
        return chain, (4 if (mode & 4 and ca >= 48) else 3), None, lean, gemms
    if split == 1:
        return chain, 2, None, lean, gemms
    fl = 0 if det else 1
    waves = 8
    if ca < 48 and scatter_lds(kind, L, split, fl, 16, dbs) <= LDS_BUDGET:
        waves = 16
    if (ca >= 48 and not det and dbs and split_knob == -1 and split == 16
            and scatter_lds(kind, L, 8, 1, 12, dbs) <= LDS_BUDGET):
        split, waves = 8, 12
    if scatter_lds(kind, L, split, fl, waves, dbs) > LDS_BUDGET:
        fl = 0
    name = (SC48 if kind == "blender" else SC20) + "%s, %d, %d, %d>" % (_b(det), split, waves, fl | (2 if dbs else 0))
    return chain, 1, name, lean, gemms


def restate_walk(L, cd, n, det, want_fac, have_dfeat=0):
    """(scan id, walk name or None, prefix table) under the default environment"""
    if not want_fac and not det:
        return (2 if have_dfeat else 1), None, 0
    for need_prefix in ((True, False) if n <= 16384 else (False,)):
        for lm in (() if det else (2, 1)):     # doubles before floats; deterministic mode keeps no LDS line
            for w in (8, 16):
                got = _walk_fits(L, cd, n, lm, w)
                if got is not None and (got or not need_prefix):
                    return 0, WALK + "%d, %s, %d, %d>" % (cd, _b(det), lm, w), int(got)
    for w in (8, 16):
        got = _walk_fits(L, cd, n, 0, w)
        if got is not None:
            return 0, WALK + "%d, %s, 0, %d>" % (cd, _b(det), w), int(got)
    raise AssertionError("no walk shape")


def _walk_fits(L, cd, n, lm, w):
    """None when the shape does not fit; otherwise whether it keeps the prefix table"""
    b = w * 5376 + L * cd * 4 * lm
    if b > 161792:
        return None
    prefix = n <= 16384 and b + 4 * n <= 161792
    if prefix:
        b += 4 * n
    if w == 8 and 2 * (b + 256) > LDS_BUDGET:
        return None
    return prefix


# ---- 1. every GPU row -------------------------------------------------------------------------------------------------------------
def planned_kernels(kind, grid, S, n_rays, cd=16, variant="mfma", det=False, pose=False, stored=True):
    """The kernel names the two plan queries give for one backward as joint_tensorf_amd.ops issues it -- a training step, or
    (pose) a render in which only the rays want a gradient, with the march derivatives stored or not: (names of the
    appearance backward, names of the density backward, shade plan, march plan).  The GPU rows of
    tests/test_gpu_scatter_shapes.py and tests/test_gpu_pose_paths.py tie these names to what the profiler saw."""
    from joint_tensorf_amd import ops
    scene = thin_scene(kind, grid[2], cd=cd, S=S, short=(grid[0], grid[1]))
    cfg = C48 if kind == "blender" else C20
    with deterministic(det), kernel_variant(variant):
        p = shade_plan(scene, POSE if pose else TRAIN, have_aux=0 if pose else int(ops._use_aux(scene)))
        m = march_plan(scene, n_rays, want_fac=0 if pose else 1, have_dfeat=int(pose and stored))
    second = {1: scatter_name(kind, p), 3: "k_pose_gather<%s, false>" % cfg, 4: "k_pose_gather<%s, true>" % cfg}.get(p[3])
    shade = [k for k in (CHAINS[p[2]] % cfg, second) if k]
    march = [k for k in ("k_march_bwd_scan<%d>" % m[0], walk_name(cd, det, m)) if k]
    return shade, march, p, m


def _canonical(name):
    """a kernel name without its argument list, k_shade_bwd's defaulted trailing template arguments written out (some
    demanglers print them, some do not)"""
    import re
    name = name.split("(")[0]
    m = re.search(r"(k_shade_bwd<jt::ShadeCfg<[^>]*>)((?:, (?:true|false))*)>", name)
    if m:
        flags = m.group(2).split(", ")[1:]
        name = name[:m.start()] + m.group(1) + "".join(", " + f for f in flags + ["false"] * (3 - len(flags))) + ">"
    return name


def missing_from(planned, profiled):
    """the planned kernel names that are not among the profiler's device kernel names"""
    seen = [_canonical(n) for n in profiled]
    return [k for k in planned if not any(_canonical(k) in n for n in seen)]


def test_canonical_names():
    c = "void jt::k_shade_bwd<jt::ShadeCfg<48, 27, 64, 0>, false, true, false>(jt::Dev, int)"
    assert missing_from([CHAINS[2] % C48], [c]) == [] and missing_from([CHAINS[3] % C48, CHAINS[0] % C48], [c]) == [
        CHAINS[3] % C48, CHAINS[0] % C48]
    assert missing_from([WALK + "16, false, 2, 8>"], ["void jt::k_march_bwd_walk<16, false, 2, 8>(jt::Dev)"]) == []


def row_kernels(row):
    kind, L, cd, rays, variant, det, ndc, expect = ROWS[row]
    S = 2 * (L - 1) + 1 if ndc else 2 * (L - 1) + 9
    shade, march, p, m = planned_kernels(kind, [SHORT[0], SHORT[1], L], S, sum(rays), cd=cd, variant=variant, det=det)
    return shade + march, p, m


@pytest.mark.parametrize("row", list(ROWS))
def test_gpu_row_on_cpu(row):
    kind, L, cd, rays, variant, det, ndc, expect = ROWS[row]
    names, p, m = row_kernels(row)
    for k in expect:
        assert k in names, (row, k, names)
    if row.startswith("walk-"):
        want_prefix = 0 if "noprefix" in row else 1
        assert m[5] == want_prefix, (row, m)
    # the restatement reproduces the row as well (where the two disagree the row is right: it ran on a GPU)
    rs = restate_shade(kind, L, det, variant, TRAIN)
    rw = restate_walk(L, cd, sum(rays), det, 1)
    for k in expect:
        assert k in (rs[2], rw[1]), (row, k, rs, rw)
    if row.startswith("walk-"):
        assert rw[2] == want_prefix, (row, rw)


def pose_kernels(kind, variant, det=False, stored=True):
    shade, march, _, _ = planned_kernels(kind, [12, 9, 72], 151, 100, variant=variant, det=det, pose=True, stored=stored)
    return shade + march


@pytest.mark.parametrize("row", list(GATHER) + ["vm48-fp32-mode0"])
def test_pose_rows_on_cpu(row):
    kind, variant, gather, chain = GATHER["vm48-fp32"] if row == "vm48-fp32-mode0" else GATHER[row]
    if row == "vm48-fp32-mode0":
        variant = "mfma-fp32"
    for stored in (True, False):
        names = pose_kernels(kind, variant, stored=stored)
        assert names == [chain, gather, "k_march_bwd_scan<%d>" % (2 if stored else 1)], (row, names)
    assert (gather == "k_pose_gather<%s, true>" % C48) == (kind == "blender" and bool(VARIANTS[variant][0] & 4))
    if row not in ("vm48-b16", "c20"):     # (the rows of test_gpu_pose_paths.test_deterministic)
        return
    # deterministic mode: the training-form kernels with their targets switched off
    names = pose_kernels(kind, variant, det=True)
    cfg = C48 if kind == "blender" else C20
    assert names[0] == chain and names[1].startswith("k_shade_scatter<%s, true, " % cfg), names
    assert names[2] == "k_march_bwd_scan<0>" and names[3].startswith("k_march_bwd_walk<16, true, "), names


# ---- 2. the sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_sweep_shade(kind):
    scene = thin_scene(kind, 2, short=(2, 2))    # (short axes of 2 texels: the long axis is the longest line from L = 2)
    checked = 0
    for variant in VARIANTS:
        for det in (False, True):
            with deterministic(det), kernel_variant(variant):
                for L in range(2, 1301):
                    scene.line_len[0] = scene.plane_h[1] = scene.plane_h[2] = L
                    for want in (TRAIN, POSE):
                        p = shade_plan(scene, want, have_aux=1)
                        got = (p[2], p[3], scatter_name(kind, p), bool(p[10]), p[14])
                        assert got == restate_shade(kind, L, det, variant, want), (kind, variant, det, L, want, p)
                        assert p[8] <= LDS_BUDGET and (p[3] != 1 or p[8] == scatter_lds(kind, L, p[5], p[7], p[6], bool(p[12])))
                        assert not p[10] or (p[0] in (8, 16) and p[1] in (8, 16)), p
                        checked += 1
    assert checked == 8 * 2 * 1299 * 2


@pytest.mark.parametrize("cd", [16, 8])
def test_sweep_walk(cd):
    scene = thin_scene("llff", 2, cd=cd, short=(2, 2))
    for det in (False, True):
        with deterministic(det):
            for L in range(2, 1301):
                scene.line_len[0] = scene.plane_h[1] = scene.plane_h[2] = L
                for n in (1000, 16384, 16385):
                    for want_fac, dfeat in ((1, 0), (0, 0), (0, 1)):
                        m = march_plan(scene, n, want_fac, dfeat)
                        got = (m[0], walk_name(cd, det, m), m[5] if m[1] else 0)
                        assert got == restate_walk(L, cd, n, det, want_fac, dfeat), (cd, det, L, n, want_fac, dfeat, m)
                        assert m[6] <= LDS_BUDGET


# ---- 3. the tape ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_tape_agrees(kind):
    scene = thin_scene(kind, 400, short=(400, 400))
    prev = (lib.jt_shade_matrix_mode(), lib.jt_shade_bwd_split(), lib.jt_shade_lean_tape())
    rows_seen = set()
    try:
        for mode in range(8):
            for split in (-1, 0, 1, 8, 16):
                for lean in (0, 1):
                    lib.jt_shade_set_matrix_mode(mode), lib.jt_shade_set_bwd_split(split), lib.jt_shade_set_lean_tape(lean)
                    for want in (TRAIN, POSE):
                        p = shade_plan(scene, want)
                        rec = (ctypes.c_int32 * 4)()
                        assert lib.jt_shade_record_layout(scene, rec) == 0
                        ws = (ctypes.c_int64 * 23)()
                        assert lib.jt_shade_workspace_layout(scene, 100000, ws) == 0
                        assert p[11] == rec[0] == ws[5], (mode, split, lean, p, list(rec), list(ws))
                        # lean: the backward is the split form with the walker scatter (or the pose gather in its place)
                        assert not p[10] or (p[0] in (8, 16) and p[1] in (8, 16) and p[3] in (1, 3, 4)), p
                        assert p[8] <= LDS_BUDGET
                        assert ws[7] <= ws[3] - ws[6], list(ws)   # the dBasis slabs fit the fourth GEMM's slab range
                        assert bool(ws[8]) == (split == 1)
                        rows_seen.add(p[11])
    finally:
        lib.jt_shade_set_matrix_mode(prev[0]), lib.jt_shade_set_bwd_split(prev[1]), lib.jt_shade_set_lean_tape(prev[2])
    assert len(rows_seen) == 2, rows_seen


# ---- 4. environment-only switches, each read once by a fresh process ---------------------------------------------------------------
_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
scene = ctypes.create_string_buffer(bytes.fromhex(sys.argv[2]))
out = (ctypes.c_int32 * 16)()
lib.jt_shade_backward_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
rc = lib.jt_shade_backward_plan(ctypes.addressof(scene), 1, 1, 0, int(sys.argv[3]), ctypes.addressof(out))
print(json.dumps([rc] + list(out)))
"""
ENV_POINTS = {
    "scatter-8-waves": ({"JT_SCATTER_WAVES": "8"}, 1),
    "default": ({}, 1),
    "scatter-wgs-256-no-aux": ({"JT_SCATTER_WGS": "256"}, 0),
    "tile-owned": ({"JT_BWD_SPLIT": "1"}, 1),
    "fused": ({"JT_BWD_SPLIT": "0"}, 0),
    "full-tape": ({"JT_LEAN_TAPE": "0"}, 1),
}


@pytest.mark.parametrize("point", list(ENV_POINTS))
def test_environment_knob(point):
    """VM-48 at 400^3 under the environment a bench.py --full extra sets"""
    extra, have_aux = ENV_POINTS[point]
    scene = thin_scene("blender", 400, short=(400, 400))
    env = {k: v for k, v in os.environ.items() if not k.startswith("JT_")}
    env.update(extra)
    out = subprocess.run([sys.executable, "-c", _CHILD, _lib.LIB_PATH, bytes(scene).hex(), str(have_aux)], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rc, *p = json.loads(out.stdout.strip().splitlines()[-1])
    assert rc == 0
    name = scatter_name("blender", p)
    if point == "scatter-8-waves":
        assert name == SC48 + "false, 16, 8, 3>" and p[9] == 224, p
    elif point == "default":
        assert name == SC48 + "false, 8, 12, 3>" and p[9] == 192, p
    elif point == "scatter-wgs-256-no-aux":
        assert p[9] == 256 and p[15] == 0, p
    elif point == "tile-owned":
        assert p[3] == 2 and p[0] == 1 and p[1] == 1, p
    elif point == "fused":
        assert p[2] == 0 and p[3] == 0 and p[1] == 0, p
    else:
        assert p[11] == 480 and p[14] == 4 and not p[10] and not p[12], p


# ---- 5. ops._use_aux ----------------------------------------------------------------------------------------------------------------
def test_use_aux_keeps_its_rule(monkeypatch):
    from joint_tensorf_amd import ops
    monkeypatch.setattr(ops, "USE_AUX_STREAM", True)
    monkeypatch.setattr(ops, "_AUX_ENV", None)

    def old_rule(n_comp_app):
        split = lib.jt_shade_bwd_split()
        if split < 0:
            return n_comp_app < 48 or bool(lib.jt_shade_matrix_mode() & 4)
        return split != 0

    prev = (lib.jt_shade_matrix_mode(), lib.jt_shade_bwd_split())
    try:
        for kind in KINDS:
            scene = thin_scene(kind, 400, short=(400, 400))
            for mode in range(8):
                for split in (-1, 0, 1, 8, 16):
                    lib.jt_shade_set_matrix_mode(mode), lib.jt_shade_set_bwd_split(split)
                    assert ops._use_aux(scene) is old_rule(KINDS[kind][0]), (kind, mode, split)
    finally:
        lib.jt_shade_set_matrix_mode(prev[0]), lib.jt_shade_set_bwd_split(prev[1])
    monkeypatch.setattr(ops, "_AUX_ENV", "0")
    assert ops._use_aux(scene) is True
    monkeypatch.setattr(ops, "USE_AUX_STREAM", False)
    assert ops._use_aux(scene) is False
