"""Device-event time of the loss-head paths bench.py does not reach, for the library JT_LIB_PATH names (or the tree's).
usage: [TAG=name] [JT_LIB_PATH=OTHER/libjt_render.so] python tools/loss_head_micro.py      (one process per library and repeat;
alternate the two libraries)
Prints one line, us per CALL of the entry point (device events around 200 back-to-back calls after 20 warm-up calls; the
deterministic row 50 after 5):
  fwd187k_free / _det   jt_render_loss_forward, 62 500 rays of one 800 x 800 view, masked (k_loss_zero + k_render_loss_fwd + _final)
  views_fwd / views_bwd jt_render_loss_views_forward / _backward, 32 views of 4 071 rays, 400 x 400 pixels per view
  fwd_one6k / bwd6k     jt_render_loss_forward / _backward at the headline step's shape, 100 views x 20 rays, no mask"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from joint_tensorf_amd import _lib, ops  # noqa: E402
from joint_tensorf_amd._lib import ptr  # noqa: E402

L, ST, DEV = _lib.lib, ops._stream, "cuda"
g = torch.Generator().manual_seed(0)
HW = 800 * 800


def timed(fn, reps=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


# k_loss_zero + k_render_loss_fwd + k_render_loss_final at 62 500 rays of one view, masked
r = 62500
rgb = torch.rand(1, r, 3, generator=g).to(DEV)
image = torch.rand(1, 3, HW, generator=g).to(DEV)
idx = torch.randint(0, HW, (r,), generator=g).to(DEV)
mask = (torch.rand(1, HW, generator=g) < 0.4).to(torch.uint8).to(DEV)
acc, loss = torch.empty(4, device=DEV), torch.empty(1, device=DEV)


def fwd():
    rc = L.jt_render_loss_forward(ptr(rgb), ptr(image), ptr(idx), ptr(mask), 1, r, HW, 1.5, 0.5, ptr(acc), ptr(loss), ST())
    assert rc == 0


out = []
for det in (0, 1):
    prev = L.jt_set_deterministic(det)
    out.append(timed(fwd, reps=200 if not det else 50, warm=20 if not det else 5))
    L.jt_set_deterministic(prev)

# 32 views of 4 071 rays
V, rv = 32, 4071
n = V * rv
rgb2 = torch.rand(n, 3, generator=g).to(DEV)
image2 = torch.rand(V, 3, HW // 4, generator=g).to(DEV)
idx2 = torch.randint(0, HW // 4, (n,), generator=g).to(DEV)
voff = (torch.arange(V + 1) * rv).to(torch.int32).to(DEV)
acc2, loss2, up = torch.empty(V, 2, device=DEV), torch.empty(V, device=DEV), torch.rand(V, generator=g).to(DEV)
g_rgb = torch.empty_like(rgb2)


def vf():
    assert L.jt_render_loss_views_forward(ptr(rgb2), ptr(image2), ptr(idx2), ptr(voff), V, HW // 4, ptr(acc2), ptr(loss2), ST()) == 0


def vb():
    assert L.jt_render_loss_views_backward(ptr(rgb2), ptr(image2), ptr(idx2), ptr(voff), V, n, HW // 4, ptr(acc2), ptr(up),
                                           ptr(g_rgb), ST()) == 0


# k_render_loss_fwd_one / k_render_loss_bwd at the headline step's shape: 100 views x 20 rays, 400 x 400 pixels, no mask
B3, r3, HW3 = 100, 20, 160000
rgb3 = torch.rand(B3, r3, 3, generator=g).to(DEV)
image3 = torch.rand(B3, 3, HW3, generator=g).to(DEV)
idx3 = torch.randint(0, HW3, (r3,), generator=g).to(DEV)
g3, g_rgb3 = torch.ones(1, device=DEV), torch.empty_like(rgb3)


def one():
    assert L.jt_render_loss_forward(ptr(rgb3), ptr(image3), ptr(idx3), None, B3, r3, HW3, 1.0, 1.0, ptr(acc), ptr(loss), ST()) == 0


def one_bwd():
    assert L.jt_render_loss_backward(ptr(rgb3), ptr(image3), ptr(idx3), None, B3, r3, HW3, 1.0, 1.0, ptr(acc), ptr(g3), ptr(g_rgb3),
                                     ST()) == 0


t_one, t_bwd = timed(one), timed(one_bwd)
out.append(timed(vf))
out.append(timed(vb))
print("MICRO %s fwd187k_free %.2f fwd187k_det %.2f views_fwd %.2f views_bwd %.2f fwd_one6k %.2f bwd6k %.2f" % (
    os.environ.get("TAG", "?"), out[0], out[1], out[2], out[3], t_one, t_bwd))
