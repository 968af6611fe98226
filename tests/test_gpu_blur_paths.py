"""Every kernel family of csrc/jt_blur.hip, forward and adjoint, against the fp64 reference of tests/blur_ref.py, element
by element, with taps that all carry weight -- at the dispatch edges, the short axes, the channel counts and the batch
shapes where such kernels go wrong.  The criterion, its kappa and the exact integer rows are derived in blur_ref.py.

Dispatch (launch_line_batch; max_n / max_taps over all items of a pass, LDS limit 65 536 bytes per workgroup):
  k_blur_mfma   taps <= 65 and 4 ((ceil16(max_n) + 64) 16 + 66) <= 65 536   <=>  ceil16(max_n) <= 944: axes up to 944
  k_blur_line   npad = ceil8(max_n) + max_taps rounded up to 2 mod 16;  4 (16 npad + 8 (max_taps + 7) + max_taps + 1) <= 65 536
                65 taps:  npad <= 978, ceil8(n) <= 913: axes up to 912 -- but every such axis is taken by k_blur_mfma first,
                          so the line kernel is not reachable at 65 taps unless JT_BLUR_MFMA=0 (945 is past both)
                67 taps:  16 npad <= 15 724, npad <= 978, ceil8(n) <= 911: axes up to 904
                201 taps: 16 npad <= 14 518, npad <= 898, ceil8(n) <= 697: axes up to 696
  otherwise     k_blur_axis (single-factor entry points) / k_blur_batch (batch entry points); also with JT_BLUR_LDS=0
  workgroups    min(chunks, 256 w), w = min(5, 163 840 / (lds + 512)) for the matrix-core pass, min(8, ..) for the line
                kernel; chunks = lines x ceil(C / 16).  The row "persistent" (900 x 260 x 20, 65 taps) has 520 chunks for
                512 workgroups along H and 1 800 for 1 280 along W: every busy workgroup walks two chunks.
blur_ref.family restates this arithmetic; test_dispatch_arithmetic pins the edges above to it, and the run asserts, from
torch.profiler's device kernel names, that each family ran exactly as many passes as the arithmetic says -- per
direction, over the whole table.

The table runs three times: in this process with the default dispatch, and in one fresh child process each for
JT_BLUR_MFMA=0 (k_blur_line takes the 65-tap rows, its adjoint included) and JT_BLUR_LDS=0 (k_blur_axis / k_blur_batch take
everything); the switches are read once per process.  A child prints one JSON line; one that exits non-zero or times
out fails its test and is not started again.

Worst |out - ref| / (2^-24 M) measured on MI355X over the value rows (each run prints its own), against the smallest
derived kappa that family is held to at 65 taps (one forward pass; the adjoint's border texels and second passes get more):
                 forward  adjoint   derived, one pass at 65 taps
  k_blur_mfma      4.67     3.26      80
  k_blur_line      4.67     3.58      65     (4.27 / 3.58 on the default dispatch's 67- and 201-tap rows)
  k_blur_axis      4.27     3.58      65
  k_blur_batch     4.67     2.73      65
The vector kernels and the matrix-core pass give the same figure on the same rows: v_mfma_f32_16x16x4_f32 is an fp32
multiply-add chain in the same order.  No family comes near its bound, every exact row is bit-exact in all three
processes, no guard band is touched, and the launch counts equal the arithmetic: no finding in jt_blur.hip.  That the
bound still decides is shown in tests/test_blur_ref.py (fault model) and by faulty builds of the library, each run
once: a K loop one step short (62 rows of the default table fail), a right fold that starts one texel late (64) and an
adjoint band built with the forward's tap index (95), while the four earlier blur tests pass on all three.
"""
import json
import os
import re
import subprocess
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import tensorf_oracle as O   # noqa: E402
from tests import blur_ref as R          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = "value"    # signed random taps on randn data, judged by the criterion
X = "exact"    # integer taps on integer data, bit for bit

# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
def _single(rid, shape, ntaps, kinds=(V, X)):
    rows = []
    for kd in kinds:
        if kd == V:
            tap_kind, data_kind = "signed", "randn"
        elif kd == X:
            tap_kind, data_kind = R.exact_kinds(ntaps)
        else:
            tap_kind, data_kind = kd
        rows.append(dict(id="%s/%s" % (rid, tap_kind), items=[shape + (0,)], taps=[(tap_kind, ntaps)], data=data_kind,
                         batch=False))
    return rows


def _table():
    T = []
    # dispatch edges: the last axis a family takes and the first it does not
    T += _single("mfma-last-944", (944, 1, 8), 65)
    T += _single("mfma-past-945", (945, 1, 8), 65)
    T += _single("line67-last-904", (904, 1, 8), 67)
    T += _single("line67-past-905", (905, 1, 8), 67)
    T += _single("line201-last-696", (696, 1, 4), 201)
    T += _single("line201-past-697", (697, 1, 4), 201)
    T += _single("two-families-960x8", (960, 8, 4), 65)           # W pass on the matrix cores, H pass in k_blur_axis
    T += _single("two-families-700x8-201", (700, 8, 4), 201, (V,))  # W pass in k_blur_line, H pass in k_blur_axis
    # axis lengths around r = 32: 1, 2, r - 1, r, r + 1, 2 r, 2 r + 1; around the 16-position blocks and kLineP / kBlurP
    for n in (1, 2, 31, 32, 33, 64, 65, 15, 16, 17, 7, 8, 9):
        T += _single("line-n%d" % n, (n, 1, 8), 65)
    for hw in ((31, 33), (2, 64), (17, 15), (32, 65), (7, 9)):
        T += _single("plane-%dx%d" % hw, hw + (4,), 65)
    T += _single("row-1x40", (1, 40, 8), 65)                      # H == 1: the single pass runs along W
    for n in (1, 2, 3, 4, 5, 8, 9):                               # the same around r = 4
        T += _single("line-n%d-9" % n, (n, 1, 4), 9)
    T += _single("plane-3x5-9", (3, 5, 4), 9)
    T += _single("plane-4x9-9", (4, 9, 8), 9)
    # block counts: 9 (second trip of the b0 += 8 loop, odd: the last pair is half), 10 (even), 17 (third trip)
    T += _single("blocks-9", (130, 1, 16), 65)
    T += _single("blocks-10", (150, 1, 16), 65)
    T += _single("blocks-17", (260, 3, 4), 65)
    # tap counts
    for ntaps in (1, 3, 9, 63, 65, 67):
        T += _single("taps-%d" % ntaps, (20, 33, 8), ntaps)
    T += _single("taps-201", (12, 17, 8), 201)
    # tap kinds, 65 taps on a plane with an axis past 2 r
    for kd in (("flat", "int"), ("ramp", "randn"), ("onehot:0", "int"), ("onehot:32", "int"), ("onehot:64", "int"),
               ("gauss:6.4", "randn"), ("gauss:0.3", "randn")):
        T += _single("kinds-40x70", (40, 70, 4), 65, (kd,))
    T += _single("kinds-line-201", (230, 1, 4), 201, (("ramp", "randn"), ("onehot:0", "int"), ("onehot:200", "int")))
    # channel counts: one partial chunk (4, 8), one full (16), full + partial of one quad (20, 36), three full (48)
    for C in (4, 8, 16, 20, 36, 48):
        T += _single("channels-%d" % C, (12, 17, C), 65)
    for C in (8, 20, 36):
        T += _single("channels-%d-67" % C, (12, 17, C), 67, (X,))
    # more chunks than workgroups: every busy workgroup walks two chunks (arithmetic in the module docstring)
    T += _single("persistent", (900, 260, 20), 65, (X,))
    # ---- batch entry points ----
    g = (9, 13, 11)                                               # a render's twelve factors on a non-cubic grid
    mat, vec = ((0, 1), (0, 2), (1, 2)), (2, 1, 0)

    def render(cd, ca):   # planes are the [g[m1]][g[m0]][C] storage read as H = g[m0], W = g[m1] (the reshape quirk)
        return [(g[m0], g[m1], cd, 0) for m0, m1 in mat] + [(g[v], 1, cd, 0) for v in vec] + \
               [(g[m0], g[m1], ca, 1) for m0, m1 in mat] + [(g[v], 1, ca, 1) for v in vec]
    for kd in (V, X):
        tk, dk = ("signed", "randn") if kd == V else R.exact_kinds(65)
        T.append(dict(id="batch-render-16-48/" + tk, items=render(16, 48), taps=[(tk, 65), (tk, 65)], data=dk, batch=True))
        T.append(dict(id="batch-render-20-20-taps-65-9/" + tk, items=render(20, 20), taps=[(tk, 65), (tk, 9)], data=dk,
                      batch=True))
        # one long line moves the whole first pass to k_blur_batch; the second pass (planes only) stays on the matrix cores
        T.append(dict(id="batch-long-item/" + tk, items=[(12, 17, 20, 0), (945, 1, 8, 1), (33, 1, 16, 0), (21, 14, 4, 1)],
                      taps=[(tk, 65), (tk, 9)], data=dk, batch=True))
        T.append(dict(id="batch-five-items/" + tk, items=[(13, 9, 16, 0), (11, 1, 16, 0), (9, 11, 48, 1), (13, 1, 48, 1),
                                                          (1, 24, 4, 1)],
                      taps=[(tk, 65), (tk, 3)], data=dk, batch=True))
    # an item that holds Inf, and a workgroup that walks from its last chunk into the next item (H pass: 801 + 1 600 chunks
    # over 1 280 workgroups, two each: workgroup 400 takes chunk 800 of item 0 and chunk 0 of item 1); the other items exact
    T.append(dict(id="batch-inf-neighbour", items=[(24, 801, 16, 0), (24, 800, 20, 0), (40, 1, 16, 0)], taps=[("int", 9)],
                  data="int", batch=True, inf=True))
    return T


TABLE = _table()
ROW_IDS = [r["id"] for r in TABLE]
assert len(set(ROW_IDS)) == len(ROW_IDS)


def _row_families(row, mfma_on, lds_on):
    """-> {adjoint: (families per pass, [families of each item's passes])} from the dispatch arithmetic"""
    out = {}
    for adj in (False, True):
        per_item = [R.passes(H, W, adj) for H, W, _C, _t in row["items"]]
        fams = []
        for p in (0, 1):
            ns = [ps[p][1] for ps in per_item if len(ps) > p]
            tp = [row["taps"][it[3]][1] for it, ps in zip(row["items"], per_item) if len(ps) > p]
            if ns:
                fams.append(R.family(max(ns), max(tp), row["batch"], mfma_on, lds_on))
        out[adj] = (fams, [fams[:len(ps)] for ps in per_item])
    return out


def _kname(fam, adj):
    return "%s<%s>" % (fam, "true" if adj else "false")


# ---------------------------------------------------------------------------------------------------------------------
# running one row through the C entry points, buffers in a guard arena
# ---------------------------------------------------------------------------------------------------------------------
def _launch(row, taps, srcs, adjoint):
    from joint_tensorf_amd._lib import JtBlurItem, lib, ptr
    from joint_tensorf_amd.ops import _stream
    sizes = [t.numel() for t in taps]
    slots = []
    for H, W, C, _t in row["items"]:
        n, plane = H * W * C, H > 1 and W > 1
        i = len(sizes)
        slots.append((i, i + 1 if plane else None, i + 2 if plane else i + 1))
        sizes += [n] * (3 if plane else 2)
    A = R.Arena(sizes, DEV)
    for i, t in enumerate(taps):
        A.view(i).copy_(t)
    for (s, _tmp, _d), x in zip(slots, srcs):
        A.view(s).copy_(x.reshape(-1))

    def p(i):
        return None if i is None else ptr(A.view(i))
    if row["batch"]:
        arr = (JtBlurItem * len(slots))()
        for k, ((s, tmp, d), (H, W, C, ti)) in enumerate(zip(slots, row["items"])):
            arr[k].in_, arr[k].tmp, arr[k].out, arr[k].taps = p(s), p(tmp), p(d), p(ti)
            arr[k].H, arr[k].W, arr[k].C, arr[k].n_taps = H, W, C, taps[ti].numel()
        fn = lib.jt_blur_batch_backward if adjoint else lib.jt_blur_batch_forward
        rc = fn(arr, len(slots), _stream())
    else:
        (s, tmp, d), (H, W, C, ti) = slots[0], row["items"][0]
        fn = lib.jt_blur_backward if adjoint else lib.jt_blur_forward
        rc = fn(p(s), p(d), p(tmp), H, W, C, p(ti), taps[ti].numel(), _stream())
    torch.cuda.synchronize()
    outs = [A.view(d, (H, W, C)).cpu() for (_s, _t, d), (H, W, C, _ti) in zip(slots, row["items"])]
    return rc, outs, A.guards_intact()


def _judge_item(res, tag, out, ref, M, kappa, exact, taps, key):
    if torch.isnan(out).any():
        res["failures"].append("%s: %d NaN outputs (an element not written, or a read past the clamp)" % (
            tag, int(torch.isnan(out).sum())))
    if exact:
        if not R.exact_magnitude_ok(M, taps):
            res["failures"].append("%s: not an exact row, max M %.3g" % (tag, float(M.max())))
        bad = R.exact_mismatches(out, ref)
        if bad:
            res["failures"].append("%s: %d elements differ from the fp64 reference on an exact row" % (tag, bad))
    else:
        bad, worst, at = R.judge(out, ref, M, kappa)
        res["kappa"][key] = max(res["kappa"].get(key, 0.0), worst)
        if bad:
            res["failures"].append("%s: %d elements outside kappa 2^-24 M, worst ratio %.4g at flat index %d" % (
                tag, bad, worst, at))


def _fam_key(fams, adj):
    return _kname(fams[0], adj) if len(set(fams)) == 1 else "+".join(_kname(f, adj) for f in fams)


def run_row(row, mfma_on=True, lds_on=True):
    res = dict(failures=[], kappa={}, launches={})
    exact = row["data"].startswith("int")
    taps = [R.make_taps(k, n, i) for i, (k, n) in enumerate(row["taps"])]
    fam = _row_families(row, mfma_on, lds_on)
    for adj in (False, True):
        srcs = [R.make_data((H, W, C), row["data"], 11 + 2 * i + adj) for i, (H, W, C, _t) in enumerate(row["items"])]
        if row.get("inf"):
            srcs[0][5, 800, 3] = float("inf")
            srcs[0][17, 800, 9] = float("-inf")
            srcs[0][0, 0, 0] = float("inf")
        rc, outs, guards = _launch(row, taps, srcs, adj)
        tag0 = "%s %s" % (row["id"], "adjoint" if adj else "forward")
        if rc != 0:
            res["failures"].append("%s: rc %d" % (tag0, rc))
            continue
        for f in fam[adj][0]:
            res["launches"][_kname(f, adj)] = res["launches"].get(_kname(f, adj), 0) + 1
        if not guards:
            res["failures"].append("%s: a guard band was written" % tag0)
        for i, ((H, W, C, ti), x, out) in enumerate(zip(row["items"], srcs, outs)):
            if row.get("inf") and i == 0:
                continue                         # (Inf in, Inf / NaN out: only its neighbours are judged)
            tag = "%s item %d (%d x %d x %d, %d taps)" % (tag0, i, H, W, C, taps[ti].numel())
            fams, nt = fam[adj][1][i], taps[ti].numel()
            if adj:
                ref, M = R.adjoint_ref(x, taps[ti]), R.magnitude_adjoint(x, taps[ti], cancellation=not exact)
                kap = R.kappa_adjoint(fams, nt, H, W)
            else:
                ref = R.forward_ref(x, taps[ti])
                # (an exact row's forward M is at most max|x| (sum|k|)^passes: the big rows skip the fp64 pass when that decides)
                cheap = float(x.abs().max()) * float(taps[ti].abs().sum()) ** len(fams)
                M = torch.full_like(ref, cheap) if exact and cheap < 2.0 ** 24 else R.magnitude_forward(x, taps[ti])
                kap = R.kappa_forward(fams, nt)
            _judge_item(res, tag, out, ref, M, kap, exact, taps[ti], _fam_key(fams, adj))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the Python entry points: ops.blur_factor, ops.blur_factors, ops.blur_images
# ---------------------------------------------------------------------------------------------------------------------
def _storage(x):
    return x[0].permute(1, 2, 0).contiguous()


def _logical(x):
    return x.permute(2, 0, 1)[None]


def _count(res, fams, adj):
    for f in fams:
        res["launches"][_kname(f, adj)] = res["launches"].get(_kname(f, adj), 0) + 1


def _factor_case(x, k, reinterpret):
    """reference, magnitudes and blurred shape of one factor the way ops.blur_factor(.., reinterpret) treats it: the oracle
    on the LOGICAL tensor (the reshape quirk is the oracle's), the magnitudes on the storage the kernel is handed"""
    _, C, A, B = x.shape
    a = x.double().requires_grad_(True)
    k64 = k.double()
    if B == 1:
        ref, H, W = O.blur_line(k64, a), A, 1
    elif reinterpret:
        ref, H, W = O.blur_plane(k64, a, B, A), B, A            # x is [1, C, g[m1], g[m0]]: (gm0, gm1) = (B, A)
    else:
        ref, H, W = O.blur_plane(k64, a, A, B), A, B
    return a, ref, H, W


def run_ops_rows(mfma_on=True, lds_on=True):
    from joint_tensorf_amd import ops
    res = dict(failures=[], kappa={}, launches={})
    gen = torch.Generator().manual_seed(5)

    def fams_of(shapes_taps, adj, batch):
        row = dict(items=[s + (i,) for i, (s, _n) in enumerate(shapes_taps)], taps=[(None, n) for _s, n in shapes_taps],
                   batch=batch)
        return _row_families(row, mfma_on, lds_on)[adj]

    def judge_factor(tag, x, k, reinterpret, out, gin, cot, fam_f, fam_a):
        """x, cot logical CPU tensors; out, gin what the HIP path returned"""
        a, ref, H, W = _factor_case(x, k, reinterpret)
        C, nt = x.shape[1], k.numel()
        (ref * cot.double()).sum().backward()
        xs = _storage(x).reshape(H, W, C)
        Mf = _logical(R.magnitude_forward(xs, k))
        _judge_item(res, tag + " forward", out.detach().cpu(), ref.detach(), Mf, R.kappa_forward(fam_f, nt), False, k,
                    _fam_key(fam_f, False))
        if gin is not None:
            Ma = R.magnitude_adjoint(_storage(cot), k).reshape(x.shape[2], x.shape[3], C)
            kap = R.kappa_adjoint(fam_a, nt, H, W).expand(H, W, C).reshape(x.shape[2], x.shape[3], C)
            _judge_item(res, tag + " adjoint", gin.detach().cpu(), a.grad, _logical(Ma), _logical(kap), False, k,
                        _fam_key(fam_a, True))

    # ops.blur_factor: a non-square plane re-interpreted as the reference does, the same plane taken as it is, a line
    k65, k9 = R.make_taps("signed", 65), R.make_taps("signed", 9, 1)
    for tag, shape, k, reint in (("blur_factor reinterpret [1,20,13,9]", (1, 20, 13, 9), k65, True),
                                 ("blur_factor plain [1,8,13,9]", (1, 8, 13, 9), k9, False),
                                 ("blur_factor line [1,16,33,1]", (1, 16, 33, 1), k65, False)):
        x = torch.randn(*shape, generator=gen)
        b = ops.factor_logical(ops.factor_storage(x).to(DEV)).requires_grad_(True)
        out = ops.blur_factor(b, k.to(DEV), reint)
        cot = torch.randn(*out.shape, generator=gen)
        (out * cot.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        H, W = (out.shape[2], out.shape[3])
        ff, fa = fams_of([((H, W, shape[1]), k.numel())], False, False), fams_of([((H, W, shape[1]), k.numel())], True, False)
        _count(res, ff[0], False), _count(res, fa[0], True)
        judge_factor(tag, x, k, reint, out, b.grad, cot, ff[1][0], fa[1][0])

    # ops.blur_factors: the twelve factors of a render, two tap vectors of different lengths; the loss uses seven of the
    # twelve outputs, so five gradients are absent (autograd hands the node zeros for them, or None)
    g, mat, vec = (9, 13, 11), ((0, 1), (0, 2), (1, 2)), (2, 1, 0)
    for cd, ca in ((16, 48), (20, 20)):
        xs = [torch.randn(1, cd, g[m1], g[m0], generator=gen) for m0, m1 in mat] + \
             [torch.randn(1, cd, g[v], 1, generator=gen) for v in vec] + \
             [torch.randn(1, ca, g[m1], g[m0], generator=gen) for m0, m1 in mat] + \
             [torch.randn(1, ca, g[v], 1, generator=gen) for v in vec]
        ks = [k65] * 6 + [k9] * 6
        bs = [ops.factor_logical(ops.factor_storage(x).to(DEV)).requires_grad_(True) for x in xs]
        outs = ops.blur_factors(k65.to(DEV), k9.to(DEV), bs[0:3], bs[3:6], bs[6:9], bs[9:12])
        outs = outs[0] + outs[1] + outs[2] + outs[3]
        used = (0, 2, 3, 7, 8, 10, 11)
        cots = [torch.randn(*o.shape, generator=gen) for o in outs]
        sum((outs[i] * cots[i].to(DEV)).sum() for i in used).backward()
        torch.cuda.synchronize()
        shp = [((o.shape[2], o.shape[3], o.shape[1]), k.numel()) for o, k in zip(outs, ks)]
        ff = fams_of(shp, False, True)
        _count(res, ff[0], False)
        # the backward's batch holds the items autograd gave a gradient for: all twelve (zeros materialised)
        fa = fams_of(shp, True, True)
        _count(res, fa[0], True)
        for i, (x, k) in enumerate(zip(xs, ks)):
            tag = "blur_factors %d/%d item %d" % (cd, ca, i)
            if i in used:
                judge_factor(tag, x, k, True, outs[i], bs[i].grad, cots[i], ff[1][i], fa[1][i])
            else:
                judge_factor(tag, x, k, True, outs[i], None, cots[i], ff[1][i], None)
                if bs[i].grad is not None and float(bs[i].grad.abs().max()) != 0.0:
                    res["failures"].append(tag + ": an unused output produced a gradient")

    # ops.blur_images: n c not a multiple of 4; one size in k_blur_line, one whose H pass is past it (k_blur_axis)
    k201 = R.make_taps("signed", 201)
    for n, c, H, W in ((3, 3, 40, 36), (1, 3, 705, 24)):
        img = torch.randn(n, c, H, W, generator=gen)
        out = ops.blur_images(img.to(DEV), k201.to(DEV))
        torch.cuda.synchronize()
        C = (n * c + 3) // 4 * 4
        ff = fams_of([((H, W, C), 201)], False, False)
        _count(res, ff[0], False)
        xl = img.reshape(1, n * c, H, W)
        ref = O.blur_plane(k201.double(), xl.double(), H, W).reshape(n, c, H, W)
        Mf = _logical(R.magnitude_forward(_storage(xl), k201)).reshape(n, c, H, W)
        _judge_item(res, "blur_images %dx%dx%dx%d" % (n, c, H, W), out.cpu(), ref, Mf, R.kappa_forward(ff[1][0], 201), False,
                    k201, _fam_key(ff[1][0], False))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the whole table in one profiler session
# ---------------------------------------------------------------------------------------------------------------------
_KERNEL = re.compile(r"k_blur_(?:mfma|line|axis|batch)<(?:true|false)>")


def run_table(mfma_on=True, lds_on=True):
    from torch.profiler import ProfilerActivity, profile
    import joint_tensorf_amd  # noqa: F401
    t0 = time.time()
    rows, attempts = {}, 0
    for attempts in (1, 2):
        rows = {}
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for row in TABLE:
                try:
                    rows[row["id"]] = run_row(row, mfma_on, lds_on)
                except Exception as e:   # a row that cannot be judged is a failed row; a GPU fault ends the process anyway
                    rows[row["id"]] = dict(failures=["%s: %r" % (row["id"], e)], kappa={}, launches={})
            try:
                rows["ops"] = run_ops_rows(mfma_on, lds_on)
            except Exception as e:
                rows["ops"] = dict(failures=["ops rows: %r" % (e,)], kappa={}, launches={})
            torch.cuda.synchronize()
        seen = {}
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA:
                m = _KERNEL.search(e.name)
                if m:
                    seen[m.group(0)] = seen.get(m.group(0), 0) + 1
        expect, kappa = {}, {}
        for r in rows.values():
            for k, v in r["launches"].items():
                expect[k] = expect.get(k, 0) + v
            for k, v in r["kappa"].items():
                kappa[k] = max(kappa.get(k, 0.0), v)
        # (torch.profiler has returned traces that lack some of this library's kernels on MI355X, tests/pinned_ref.py: the
        #  table is deterministic, so it is recorded once more; a kernel that really is not the expected one stays so)
        if seen == expect:
            break
    return dict(rows=rows, seen=seen, expect=expect, kappa=kappa, attempts=attempts, seconds=time.time() - t0)


@pytest.fixture(scope="module")
def default_run():
    out = run_table()
    print("\n[blur paths] default dispatch: %d rows in %.1f s (profiler attempts: %d)" % (
        len(out["rows"]), out["seconds"], out["attempts"]))
    print("   launches seen %s" % sorted(out["seen"].items()))
    print("   worst kappa   %s" % sorted((k, round(v, 2)) for k, v in out["kappa"].items()))
    return out


@pytest.mark.parametrize("rid", ROW_IDS + ["ops"])
def test_row(default_run, rid):
    assert default_run["rows"][rid]["failures"] == []


def test_every_family_ran_as_the_dispatch_arithmetic_says(default_run):
    """kernel launches by name, over the whole table: what ran == what blur_ref.family expects, and all four families in
    both directions are among them"""
    assert default_run["seen"] == default_run["expect"], (default_run["seen"], default_run["expect"])
    for fam in (R.MFMA, R.LINE, R.AXIS, R.BATCH):
        for adj in (False, True):
            assert default_run["seen"].get(_kname(fam, adj), 0) > 0, (fam, adj)


def test_dispatch_arithmetic():
    """the edges of the module docstring, and the persistent row's chunk counts, from the restated launch arithmetic"""
    assert R.family(944, 65) == R.MFMA and R.family(945, 65) == R.AXIS and R.family(945, 65, batch=True) == R.BATCH
    assert R.family(904, 67) == R.LINE and R.family(905, 67) == R.AXIS
    assert R.family(696, 201) == R.LINE and R.family(697, 201) == R.AXIS
    assert R.family(912, 65, mfma_on=False) == R.LINE and R.family(913, 65, mfma_on=False) == R.AXIS
    assert R.family(8, 9, lds_on=False) == R.AXIS
    assert all(R.family(n, 65) != R.LINE for n in range(1, 1200))       # not reachable at 65 taps by default
    for mfma_on in (True, False):
        for axis, n in ((0, 900), (1, 260)):
            fam = R.family(n, 65, mfma_on=mfma_on)
            ch = R.chunks(900, 260, 20, axis)
            assert fam == (R.MFMA if mfma_on else R.LINE), (mfma_on, axis)
            assert R.workgroups(fam, n, 65, ch) < ch <= 2 * R.workgroups(fam, n, 65, ch), (mfma_on, axis)
    # the Inf row: 801 + 1 600 chunks over 1 280 workgroups, two chunks each, so workgroup 400 crosses the items
    assert R.chunks(24, 801, 16, 0) == 801 and R.chunks(24, 800, 20, 0) == 1600
    assert R.workgroups(R.MFMA, 24, 9, 801 + 1600) == 1280 and R.workgroups(R.MFMA, 40, 9, 801 + 1600 + 1) == 1280


def test_batch_argument_errors():
    """thirteen items, a channel count that is not a multiple of 4, an even tap count: refused before any launch"""
    from joint_tensorf_amd._lib import JtBlurItem, lib, ptr
    from joint_tensorf_amd.ops import _stream
    x = torch.zeros(3 * 8 * 8 * 8 + 16, device=DEV)

    def items(n, C=8, ntaps=9):
        arr = (JtBlurItem * n)()
        for k in range(n):
            arr[k].in_, arr[k].tmp, arr[k].out, arr[k].taps = ptr(x), ptr(x[512:]), ptr(x[1024:]), ptr(x[1536:])
            arr[k].H, arr[k].W, arr[k].C, arr[k].n_taps = 8, 8, C, ntaps
        return arr
    for fn in (lib.jt_blur_batch_forward, lib.jt_blur_batch_backward):
        assert fn(items(13), 13, _stream()) == 2        # JT_ERR_UNSUPPORTED
        assert fn(items(2, C=6), 2, _stream()) == 2
        assert fn(items(2, ntaps=8), 2, _stream()) == 2
        assert fn(items(1), 0, _stream()) == 1          # JT_ERR_ARG
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


_ABNORMAL = []   # a child that died or timed out: nothing more is started on the GPU from here


def _child(env_name):
    assert not _ABNORMAL, "not started: %s ended abnormally" % _ABNORMAL[0]
    env = dict(os.environ)
    env[env_name] = "0"
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                           timeout=600, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _ABNORMAL.append(env_name + "=0 (timeout)")
        raise
    if r.returncode != 0:
        _ABNORMAL.append("%s=0 (exit %d)" % (env_name, r.returncode))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print("\n[blur paths] %s=0: %.1f s; launches %s; worst kappa %s" % (
        env_name, out["seconds"], sorted(out["seen"].items()), sorted((k, round(v, 2)) for k, v in out["kappa"].items())))
    assert out["failures"] == {}, out["failures"]
    assert out["seen"] == out["expect"], (out["seen"], out["expect"])
    return out


def test_vector_line_kernel_takes_the_table_without_the_matrix_cores():
    """JT_BLUR_MFMA=0 in a fresh process: k_blur_line and its adjoint at 65 taps and below, under the same reference"""
    out = _child("JT_BLUR_MFMA")
    assert not any(R.MFMA in k for k in out["seen"])
    for adj in (False, True):
        assert out["seen"].get(_kname(R.LINE, adj), 0) > 100, out["seen"]


def test_general_kernels_take_the_table_without_the_lds_kernels():
    """JT_BLUR_LDS=0 in a fresh process: k_blur_axis and k_blur_batch, forward and adjoint, on every row"""
    out = _child("JT_BLUR_LDS")
    assert sorted(out["seen"]) == sorted(_kname(f, a) for f in (R.AXIS, R.BATCH) for a in (False, True)), out["seen"]


if __name__ == "__main__":   # the child: the table under the environment it was started with, one JSON line
    assert sys.argv[1:] == ["--child"]
    res = run_table(mfma_on=os.environ.get("JT_BLUR_MFMA", "1") != "0", lds_on=os.environ.get("JT_BLUR_LDS", "1") != "0")
    print(json.dumps(dict(failures={k: v["failures"] for k, v in res["rows"].items() if v["failures"]}, seen=res["seen"],
                          expect=res["expect"], kappa=res["kappa"], seconds=res["seconds"], attempts=res["attempts"])))
