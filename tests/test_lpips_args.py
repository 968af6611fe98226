"""What the LPIPS entry points of the C ABI refuse, decided before any launch (no GPU), their place in the header, and
eval_io.write_quant with and without the fourth list."""
import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 256          # a non-NULL pointer that is never dereferenced on these paths
OK, ARG, UNSUPPORTED = 0, 1, 2


def _weights(fill=P):
    from joint_tensorf_amd import _lib
    w = _lib.JtLpipsWeights()
    for l in range(5):
        w.conv[l], w.bias[l], w.lin[l] = fill, fill, fill
    return w


def test_lpips_forward_refusals():
    from joint_tensorf_amd import _lib
    L = _lib.lib
    w = ctypes.byref(_weights())
    big = 1 << 40

    def run(V, H, W, pred=P, target=P, weights=w, out=P, ws=P, ws_bytes=big):
        return L.jt_lpips_forward(pred, target, V, H, W, weights, out, None, ws, ws_bytes, None)
    # the second pool needs 3 rows: 31 is the smallest side
    assert run(1, 30, 64) == UNSUPPORTED and run(1, 64, 30) == UNSUPPORTED
    assert L.jt_lpips_workspace_bytes(1, 30, 64) == 0 and L.jt_lpips_workspace_bytes(1, 64, 30) == 0
    assert L.jt_lpips_workspace_bytes(1, 31, 31) > 0 and L.jt_lpips_workspace_bytes(1, 64, 31) > 0
    table = (ctypes.c_int64 * 20)()
    assert L.jt_lpips_feature_layout(1, 30, 64, table) == UNSUPPORTED and L.jt_lpips_feature_layout(1, 31, 31, None) == ARG
    # an activation of 2^31 elements: the scaled batch 2 V x 3 x H x W, then the first feature stack 2 V x 64 x h x w
    assert 2 * 3 * 18919 * 18919 >= 1 << 31 > 2 * 3 * 18918 * 18918
    assert run(1, 18919, 18919) == UNSUPPORTED and L.jt_lpips_workspace_bytes(1, 18919, 18919) == 0
    h = (16387 - 7) // 4 + 1
    assert 2 * 64 * h * h >= 1 << 31 > 2 * 3 * 16387 * 16387
    assert run(1, 16387, 16387) == UNSUPPORTED
    assert run(1 << 20, 64, 64) == UNSUPPORTED
    # NULL pointers and sizes below 1, also where the shape would be refused: argument errors come first
    for kw in (dict(pred=None), dict(target=None), dict(weights=None), dict(out=None), dict(ws=None)):
        assert run(1, 64, 64, **kw) == ARG, kw
        assert run(1, 30, 64, **kw) == ARG, kw
    for slot in ("conv", "bias", "lin"):
        bad = _weights()
        getattr(bad, slot)[3] = None
        assert run(1, 64, 64, weights=ctypes.byref(bad)) == ARG, slot
    assert run(0, 64, 64) == ARG and run(1, 0, 64) == ARG
    # a short workspace
    need = L.jt_lpips_workspace_bytes(2, 64, 64)
    assert need % 8 == 0 and run(2, 64, 64, ws_bytes=need - 1) == ARG


def test_layer_entry_points_refuse_before_a_launch():
    from joint_tensorf_amd import _lib
    L = _lib.lib

    def conv(batch=1, c_in=3, h=31, w=31, c_out=64, k=11, stride=4, pad=2, variant=0, x=P, packed=P, bias=P, out=P):
        return L.jt_conv2d_relu_forward(x, packed, bias, batch, c_in, h, w, c_out, k, k, stride, pad, variant, out, None)
    for kw in (dict(x=None), dict(packed=None), dict(bias=None), dict(out=None), dict(batch=0), dict(variant=3), dict(variant=-1)):
        assert conv(**kw) == ARG, kw
    assert conv(k=7, stride=2, pad=3) == UNSUPPORTED              # a geometry the kernel is not instantiated for
    assert conv(k=3, stride=2, pad=1) == UNSUPPORTED
    assert conv(c_out=48) == UNSUPPORTED                          # not a multiple of 32
    assert conv(c_out=96, variant=_lib.JT_CONV_TILE_64X64) == UNSUPPORTED
    assert conv(h=6, w=31) == UNSUPPORTED                         # the picture with its padding is smaller than the window
    assert conv(batch=1 << 16, c_in=64, h=256, w=256, c_out=64, k=3, stride=1, pad=1) == UNSUPPORTED      # 2^38 inputs
    assert L.jt_conv_pack_weights(None, 64, 3, 11, 11, P, None) == ARG
    assert L.jt_conv_pack_weights(P, 64, 3, 11, 11, None, None) == ARG
    assert L.jt_conv_pack_weights(P, 0, 3, 11, 11, P, None) == ARG
    # Kpad = K rounded up to the k step of the kernel: 363 -> 384, 1600 -> 1600, 3456 -> 3456
    assert L.jt_conv_packed_floats(64, 3, 11, 11) == 384 * 64
    assert L.jt_conv_packed_floats(192, 64, 5, 5) == 1600 * 192
    assert L.jt_conv_packed_floats(256, 384, 3, 3) == 3456 * 256
    assert L.jt_conv_packed_floats(0, 3, 11, 11) == 0
    assert L.jt_maxpool_3x3s2_forward(None, 1, 3, 3, P, None) == ARG
    assert L.jt_maxpool_3x3s2_forward(P, 1, 3, 3, None, None) == ARG
    assert L.jt_maxpool_3x3s2_forward(P, 1, 2, 3, P, None) == ARG
    assert L.jt_maxpool_3x3s2_forward(P, 1 << 15, 256, 256, P, None) == UNSUPPORTED


def test_header_cites_the_reference_lines():
    src = open(os.path.join(ROOT, "include", "jt_render.h")).read()
    block = src[src.index("LPIPS with the AlexNet backbone"):src.index("int jt_lpips_forward")]
    assert "model/nerf.py:33" in block and "model/nerf.py:551" in block
    for name in ("jt_conv_pack_weights", "jt_conv2d_relu_forward", "jt_maxpool_3x3s2_forward", "jt_lpips_forward"):
        m = re.search(r"\*\s+%s: \(([^)]*)\)" % name, block)
        assert m, name                                           # every entry names what it replaces
    assert "model/nerf.py:33" in re.search(r"jt_conv_pack_weights: \(([^)]*)\)", block).group(1)
    assert "model/nerf.py:551" in re.search(r"jt_lpips_forward: \(([^)]*)\)", block).group(1)


def test_write_quant_with_and_without_lpips(tmp_path):
    from joint_tensorf_amd import eval_io
    psnr, ssim, lp = [31.25, 28.5, 0.1 + 0.2], [0.9, 0.75, 1.0], [0.0625, 1e-5, 0.1 + 0.7]
    eval_io.write_quant(str(tmp_path), psnr, ssim)
    three = open(os.path.join(str(tmp_path), "quant.txt")).read()
    assert three == "".join("{} {} {} {}\n".format(i, psnr[i], ssim[i], float("nan")) for i in range(3))
    eval_io.write_quant(str(tmp_path), psnr, ssim, None)
    assert open(os.path.join(str(tmp_path), "quant.txt")).read() == three
    eval_io.write_quant(str(tmp_path), psnr, ssim, lpips_per_view=lp)
    lines = open(os.path.join(str(tmp_path), "quant.txt")).read().splitlines()
    assert lines == ["{} {} {} {}".format(i, psnr[i], ssim[i], lp[i]) for i in range(3)]     # the reference's formatting of floats
    for i, ln in enumerate(lines):
        f = ln.split(" ")
        assert len(f) == 4 and f[3] == repr(lp[i]) and float(f[3]) == lp[i] and not math.isnan(float(f[3]))
    with pytest.raises(ValueError, match="2 LPIPS values for 3 views"):
        eval_io.write_quant(str(tmp_path), psnr, ssim, lp[:2])
