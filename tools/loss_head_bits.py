"""Two builds of libjt_render.so in ONE process: every output word of the loss-head entry points (jt_render_loss_*, the per-view
pair, jt_loss_sum_*, jt_finite_check) on the inputs of tests/test_gpu_loss_paths.py, compared as int32.
usage: python tools/loss_head_bits.py OTHER/libjt_render.so     (the other build, e.g. the parent commit's, built from a scratch
checkout with joint_tensorf_amd/build.py; "new" is the library the package loads: the tree's, or JT_LIB_PATH)
Prints every differing word and a count.  acc4 of general inputs above one workgroup in free mode is listed but not counted:
the atomic adds arrive in any order, and the other build is compared with itself there as a control."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from joint_tensorf_amd import _lib, ops  # noqa: E402
from joint_tensorf_amd._lib import ptr  # noqa: E402
from tests import camera_ref as C  # noqa: E402
from tests import test_gpu_loss_paths as T  # noqa: E402

DEV = "cuda"
NEW = _lib.lib
PAR = ctypes.CDLL(os.path.abspath(sys.argv[1]))
for name, (res, args) in _lib.SIGNATURES.items():
    fn = getattr(PAR, name)
    fn.restype, fn.argtypes = res, args
assert PAR.jt_version() == NEW.jt_version()
LIBS = {"parent": PAR, "new": NEW}
ST = ops._stream
n_cmp = n_diff = 0


def ok(rc):
    assert rc == 0, rc


def words(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.int32)


def compare(what, a, b, order_dependent=False):
    """a, b: dicts name -> tensor"""
    global n_cmp, n_diff
    for k in a:
        wa, wb = words(a[k]), words(b[k])
        d = int((wa != wb).sum())
        n_cmp += wa.numel()
        if d:
            if not order_dependent:
                n_diff += d
            i = int((wa != wb).nonzero()[0])
            print("DIFF%s %s %s: %d of %d words; first at %d: parent %r (0x%08x) new %r (0x%08x)" % (
                " (atomic order: not a defined value)" if order_dependent else "", what, k, d, wa.numel(), i,
                float(a[k].flatten()[i]), int(wa[i]) & 0xffffffff, float(b[k].flatten()[i]), int(wb[i]) & 0xffffffff))


def render(L, rgb, image, idx, mask, masked, ind, det):
    B, r = rgb.shape[0], rgb.shape[1]
    HW = image.shape[1] * image.shape[2] // 3 if image.dim() == 3 else image[0].numel() // 3
    acc = torch.full((4,), -7.0, device=DEV)
    loss = torch.full((1,), -7.0, device=DEV)
    g = torch.tensor([T.UP], device=DEV)
    g_rgb = torch.full_like(rgb, -7.0)
    m = mask if masked else None
    prev = L.jt_set_deterministic(1 if det else 0)
    try:
        if ind:
            slots = torch.tensor([image.data_ptr(), mask.data_ptr()], dtype=torch.int64, device=DEV)
            ok(L.jt_render_loss_forward_ind(ptr(rgb), ptr(slots), ptr(idx), int(masked), B, r, HW, T.FE, T.FNE, ptr(acc), ptr(loss), ST()))
            ok(L.jt_render_loss_backward_ind(ptr(rgb), ptr(slots), ptr(idx), int(masked), B, r, HW, T.FE, T.FNE, ptr(acc), ptr(g),
                                             ptr(g_rgb), ST()))
        else:
            ok(L.jt_render_loss_forward(ptr(rgb), ptr(image), ptr(idx), ptr(m), B, r, HW, T.FE, T.FNE, ptr(acc), ptr(loss), ST()))
            ok(L.jt_render_loss_backward(ptr(rgb), ptr(image), ptr(idx), ptr(m), B, r, HW, T.FE, T.FNE, ptr(acc), ptr(g), ptr(g_rgb),
                                         ST()))
        torch.cuda.synchronize()
    finally:
        L.jt_set_deterministic(prev)
    return dict(loss=loss, acc4=acc, g_rgb=g_rgb)


def render_rows():
    for lattice in (True, False):
        for B, r in T.SHAPES:
            rgb, image, idx, mask = T._inputs(B, r, lattice=lattice, seed=0 if lattice else 1)
            if not lattice:     # the NaN / Inf rows of the tests ride on the random rows
                rgb[0, min(5, r - 1), 1] = float("nan")
                rgb[B - 1, r - 1, 2] = float("inf")
            rgb, image, idx, mask = (rgb.to(DEV).contiguous(), image.to(DEV).view(B, 3, -1).contiguous(), idx.to(DEV),
                                     mask.to(DEV).contiguous())
            n = 3 * B * r
            for masked in (False, True):
                for ind in (False, True):
                    for det in (False, True):
                        what = "render %s n=%d masked=%d ind=%d det=%d" % ("lattice" if lattice else "random", n, masked, ind, det)
                        # free mode above one workgroup on general inputs: the atomic adds arrive in any order
                        loose = (not lattice) and (not det) and n > 32768
                        out = {k: render(L, rgb, image, idx, mask, masked, ind, det) for k, L in LIBS.items()}
                        compare(what, out["parent"], out["new"], order_dependent=loose)
                        if loose:   # control: the parent against itself
                            compare(what + " [parent twice]", out["parent"], render(PAR, rgb, image, idx, mask, masked, ind, det), True)


def views(L, rgb, image, idx, voff, up):
    V, n, HW = voff.numel() - 1, rgb.shape[0], image[0].numel() // 3
    acc2 = torch.full((V, 2), -7.0, device=DEV)
    loss = torch.full((V,), -7.0, device=DEV)
    g_rgb = torch.full_like(rgb, -7.0)
    ok(L.jt_render_loss_views_forward(ptr(rgb), ptr(image), ptr(idx), ptr(voff), V, HW, ptr(acc2), ptr(loss), ST()))
    ok(L.jt_render_loss_views_backward(ptr(rgb), ptr(image), ptr(idx), ptr(voff), V, n, HW, ptr(acc2), ptr(up), ptr(g_rgb), ST()))
    torch.cuda.synchronize()
    return dict(loss=loss, acc2=acc2, g_rgb=g_rgb)


def views_rows():
    for sizes, nan_view in ((C.RAGGED_SIZES, None), ((5, 10923, 3, 2), 2)):
        for lattice in (True, False):
            rgb, image, idx, voff, up = T._views_inputs(sizes, lattice)
            if nan_view is not None:
                rgb[voff[nan_view]:voff[nan_view + 1]] = float("nan")
            args = (rgb.to(DEV).contiguous(), image.to(DEV).contiguous(), idx.to(DEV), voff.to(DEV).to(torch.int32), up.to(DEV))
            out = {k: views(L, *args) for k, L in LIBS.items()}
            compare("views %s lattice=%d" % (sizes, lattice), out["parent"], out["new"])


def loss_sum(L, render_v, reg3, w, form, word):
    r = torch.tensor([render_v], device=DEV)
    q = torch.tensor(reg3, device=DEV)
    w4 = torch.tensor(w, device=DEV, dtype=torch.float32)
    total = torch.full((1,), -7.0, device=DEV)
    g = torch.tensor([T.UP], device=DEV)
    g_r, g_q = torch.full((1,), -7.0, device=DEV), torch.full((3,), -7.0, device=DEV)
    word.zero_()
    if form == "value":
        ok(L.jt_loss_sum_forward(ptr(r), ptr(q), *w, ptr(total), ST()))
        ok(L.jt_loss_sum_backward(ptr(g), *w, ptr(g_r), ptr(g_q), ST()))
    elif form == "dyn":
        ok(L.jt_loss_sum_forward_dyn(ptr(r), ptr(q), ptr(w4), ptr(total), ST()))
        ok(L.jt_loss_sum_backward_dyn(ptr(g), ptr(w4), ptr(g_r), ptr(g_q), ST()))
    else:
        fin = torch.ones(5, device=DEV)
        arr = (_lib.JtFiniteItem * 1)()
        arr[0].data, arr[0].n, arr[0].bit = ptr(fin), 5, ops.FINITE_POSE
        host = (ctypes.c_float * 4)(*w) if form == "check" else None
        ok(L.jt_loss_sum_check_forward(ptr(r), ptr(q), host, None if host else ptr(w4), ptr(total), arr, 1, ops.FINITE_LOSS, ptr(word),
                                       ST()))
        ok(L.jt_loss_sum_backward(ptr(g), *w, ptr(g_r), ptr(g_q), ST()))
    torch.cuda.synchronize()
    return dict(total=total, g_render=g_r, g_reg3=g_q, status=word.clone())


def sum_rows():
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    for case, (render_v, reg3, w, _) in T.SUM_CASES.items():
        for form in ("value", "dyn", "check", "check_dyn"):
            out = {k: loss_sum(L, render_v, reg3, w, form, word) for k, L in LIBS.items()}
            compare("loss_sum %s %s" % (case, form), out["parent"], out["new"])


def guard(L, tensors, bits, word):
    word.zero_()
    arr = (_lib.JtFiniteItem * len(tensors))()
    for k, t in enumerate(tensors):
        arr[k].data, arr[k].n, arr[k].bit = ptr(t), t.numel(), bits[k]
    ok(L.jt_finite_check(arr, len(tensors), ptr(word), ST()))
    torch.cuda.synchronize()
    return dict(status=word.clone())


def guard_rows():
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(2)
    tensors = [torch.randn(n, generator=g).to(DEV) for n in (1, 65536, 65537)]
    bits = [ops.FINITE_POSE, ops.FINITE_RENDER, ops.FINITE_GRAD]
    spots = [None, (0, 0), (1, 0), (1, 65535), (2, 0), (2, 65535), (2, 65536)]
    for spot in spots:
        for bad in (float("inf"), float("-inf"), float("nan")):
            if spot:
                old = tensors[spot[0]][spot[1]].clone()
                tensors[spot[0]][spot[1]] = bad
            out = {k: guard(L, tensors, bits, word) for k, L in LIBS.items()}
            if spot:
                tensors[spot[0]][spot[1]] = old
                assert int(out["new"]["status"]) == bits[spot[0]], (spot, bad, int(out["new"]["status"]))
            else:
                assert int(out["new"]["status"]) == 0
            compare("guard %s %r" % (spot, bad), out["parent"], out["new"])


render_rows()
views_rows()
sum_rows()
guard_rows()
print("compared %d words: %d differ (outside the order-dependent rows)" % (n_cmp, n_diff))
