"""LPIPS on the GPU (csrc/jt_lpips.hip): every convolution layer against a bound derived from its arithmetic, its bitwise
independence of tile, batch and run, the max-pool and the fp64 head against stock ops, ops.lpips against the fp64 evaluation of
the definition (tests/lpips_ref.py), and the evaluation stage with and without the two weight files (model/nerf.py:33,551,561,572).
All weights are seeded random ones (tests/lpips_ref.py: random_weights): no trained file exists in this repository."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.lpips_ref import head, lpips_ref, noisy_pairs, random_weights, state_dicts

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Cin, Cout, kernel, stride, pad, H, W): the smallest shapes that reach each hazard of the implicit GEMM
LAYER_CASES = [
    (3, 64, 11, 4, 2, 31, 31),      # K = 363 (odd, not a multiple of the k step), 49 pixels (not a multiple of the pixel tile)
    (3, 64, 11, 4, 2, 35, 43),
    (64, 192, 5, 1, 2, 3, 3),       # most taps outside the picture
    (64, 192, 5, 1, 2, 7, 11),
    (192, 384, 3, 1, 1, 1, 1),      # one pixel: the centre tap only
    (192, 384, 3, 1, 1, 3, 5),
    (384, 256, 3, 1, 1, 3, 5),      # K = 3456
]
_LAYER = {}


def _layer(case, batch):
    """inputs, the fp64 result and the bound of one case, computed once on the host and left unchanged"""
    key = case + (batch,)
    if key not in _LAYER:
        cin, cout, k, stride, pad, H, W = case
        gen = torch.Generator().manual_seed(1000 + 7 * LAYER_CASES.index(case) + batch)
        K = cin * k * k
        w = (torch.randn(cout, cin, k, k, generator=gen) * (2.0 / K) ** 0.5).float()
        b = (0.1 * torch.randn(cout, generator=gen)).float()
        x = torch.randn(batch, cin, H, W, generator=gen).float()
        ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad))
        mag = F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=pad) + b.double().abs().view(1, -1, 1, 1)
        # any fp32 fma chain of K products plus the bias add is within gamma_(K+1) <= (K + 2) 2^-24 of the exact value, relative
        # to the sum of the magnitudes; ReLU is 1-Lipschitz
        _LAYER[key] = (x, w, b, ref, (K + 2) * 2.0 ** -24 * mag)
    return _LAYER[key]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "%dto%d_k%d_%dx%d" % (c[0], c[1], c[2], c[5], c[6]))
def test_conv_layer_within_the_derived_bound(case, batch):
    from joint_tensorf_amd import ops
    cin, cout, k, stride, pad, H, W = case
    x, w, b, ref, bound = _layer(case, batch)
    packed = ops.conv_pack_weights(w.to(DEV))
    got = ops.conv2d_relu(x.to(DEV), packed, b.to(DEV), k, stride, pad)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = (got.cpu().double() - ref).abs()
    stock = (F.relu(F.conv2d(x, w, b, stride=stride, padding=pad)).double() - ref).abs()
    print("%s batch %d: kernel / bound %.3e, stock fp32 / bound %.3e, %.1f %% of the outputs positive"
          % (case, batch, float((err / bound).max()), float((stock / bound).max()), 100 * float((ref > 0).double().mean())))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert 0.2 < float((ref > 0).double().mean()) < 0.8           # ReLU cuts some and keeps some


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "%dto%d_k%d_%dx%d" % (c[0], c[1], c[2], c[5], c[6]))
def test_conv_layer_is_the_same_bits_for_every_tile_batch_and_run(case):
    from joint_tensorf_amd import _lib, ops
    cin, cout, k, stride, pad, H, W = case
    x, w, b, _, _ = _layer(case, 3)
    x, b = x.to(DEV), b.to(DEV)
    packed = ops.conv_pack_weights(w.to(DEV))
    first = ops.conv2d_relu(x, packed, b, k, stride, pad)
    assert torch.equal(first, ops.conv2d_relu(x, packed, b, k, stride, pad))                       # two runs
    for tile in ops.CONV_TILES:
        full = ops.conv2d_relu(x, packed, b, k, stride, pad, tile=tile)
        assert torch.equal(full, first), tile                                                      # every tile variant
        for i in range(3):
            alone = ops.conv2d_relu(x[i:i + 1], packed, b, k, stride, pad, tile=tile)
            assert torch.equal(alone[0], first[i]), (tile, i)                                      # alone and as a member of a batch
    assert set(ops.CONV_TILES) == {_lib.JT_CONV_TILE_64X64, _lib.JT_CONV_TILE_32X32}
    assert float(first.abs().max()) > 0


def test_packed_weights_are_k_major_with_zero_rows_behind_k():
    from joint_tensorf_amd import ops
    w = torch.arange(64 * 3 * 11 * 11, dtype=torch.float32).view(64, 3, 11, 11) + 1      # asymmetric: a transpose shows
    packed = ops.conv_pack_weights(w.to(DEV)).cpu().view(384, 64)
    assert torch.equal(packed[:363], w.view(64, 363).t()) and not bool(packed[363:].any())


@pytest.mark.parametrize("shape", [(2, 5, 16, 23), (1, 3, 7, 11), (2, 2, 3, 3), (3, 1, 15, 15)])
def test_max_pool_equals_the_stock_op(shape):
    from joint_tensorf_amd import ops
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(shape[2]))
    got = ops.max_pool_3x3s2(x.to(DEV))
    assert torch.equal(got.cpu(), F.max_pool2d(x, 3, 2))


_WEIGHTS = {}


def _weights():
    from joint_tensorf_amd import lpips
    if not _WEIGHTS:
        host = random_weights(0)
        _WEIGHTS["host"], _WEIGHTS["dev"] = host, lpips.pack(*host, device=DEV)
    return _WEIGHTS["host"], _WEIGHTS["dev"]


def test_head_matches_the_fp64_evaluation_of_the_same_features():
    from joint_tensorf_amd import ops
    host, dev = _weights()
    for V, H, W, noise in ((1, 31, 31, 0.1), (3, 67, 95, 0.3)):
        pred, target = noisy_pairs(V, H, W, noise, seed=40 + V)
        out, layers, feats = ops.lpips_features(pred.to(DEV), target.to(DEV), dev)
        feats = [f.cpu() for f in feats]
        want = head([f[:V] for f in feats], [f[V:] for f in feats], host[2])
        # a term is lin_c (a - b)^2 with |a|, |b| <= 1: a layer is at most 4 sum(lin); every term carries at most (C + 10) fp64
        # roundings, about 4e-14 relative
        tol = torch.tensor([1e-12 * 4 * float(l.double().sum()) for l in host[2]], dtype=torch.float64)
        err = (layers.cpu() - want).abs()
        print("V=%d %dx%d: head - fp64 per layer %s (allowed %s)" % (V, H, W, err.amax(dim=0).tolist(), tol.tolist()))
        assert bool((err <= tol).all())
        assert bool(((out.cpu() - want.sum(dim=1)).abs() <= tol.sum()).all())
        assert bool((want > 0).all())


# (H, W, V, noise): every size with V = 1 and V = 3, the noise levels from 0.02 to 0.3
E2E_CASES = [(31, 31, 1, 0.02), (31, 31, 3, 0.3), (64, 64, 1, 0.1), (64, 64, 3, 0.02), (67, 95, 1, 0.3), (67, 95, 3, 0.1),
             (128, 160, 1, 0.05), (128, 160, 3, 0.3)]


def test_lpips_end_to_end():
    """Relative error against the fp64 evaluation of the definition on the CPU.  Measured on MI355X with these cases (random
    weights; profiles/lpips.txt): kernel 6e-9 .. 2.5e-7, stock fp32 CPU ops 1.3e-8 .. 1.9e-7; allowed min(8 x the largest stock
    figure, 1e-5) = 1.5e-6.  The factor 8 covers a sequential k-ordered chain against torch's blocked sums; a broken layer is off
    by 1e-3 or more."""
    from joint_tensorf_amd import ops
    host, dev = _weights()
    rows = []
    for k, (H, W, V, noise) in enumerate(E2E_CASES):
        pred, target = noisy_pairs(V, H, W, noise, seed=200 + k)
        ref, ref_layers = lpips_ref(pred, target, host)
        f32, _ = lpips_ref(pred, target, host, dtype=torch.float32)
        got, layers = ops.lpips(pred.to(DEV), target.to(DEV), dev, return_layers=True)
        alone = ops.lpips(pred.to(DEV), target.to(DEV), dev)
        assert got.dtype == torch.float64 and got.shape == (V,) and got.is_cuda and layers.shape == (V, 5)
        assert torch.equal(alone, got)                                                   # the layers are an extra output
        lc = layers.cpu()
        assert torch.equal(got.cpu(), (((lc[:, 0] + lc[:, 1]) + lc[:, 2]) + lc[:, 3]) + lc[:, 4])       # ascending, exactly
        for v in range(V):                                                               # a view does not see its batch
            assert torch.equal(ops.lpips(pred[v:v + 1].to(DEV), target[v:v + 1].to(DEV), dev)[0], got[v])
        rel = float(((got.cpu() - ref).abs() / ref).max())
        rel32 = float(((f32.double() - ref).abs() / ref).max())
        rows.append((H, W, V, noise, float(ref.min()), float(ref.max()), rel, rel32))
        print("%3dx%-3d V=%d noise=%.2f lpips %.6f..%.6f | kernel - fp64: rel %.2e | stock fp32 - fp64: rel %.2e" % rows[-1])
    stock = max(r[7] for r in rows)
    worst = max(r[6] for r in rows)
    print("largest relative error: kernel %.2e, stock fp32 %.2e, allowed min(8 x stock, 1e-5) = %.2e"
          % (worst, stock, min(8 * stock, 1e-5)))
    for r in rows:
        assert r[6] <= 8 * stock and r[6] <= 1e-5, r
    assert min(r[4] for r in rows) < 0.5 * max(r[5] for r in rows)                       # the cases span close and far pairs
    # identical pictures and all-zero pictures: exactly 0
    pred, target = noisy_pairs(2, 67, 95, 0.3, seed=9)
    same, same_layers = ops.lpips(target.to(DEV), target.clone().to(DEV), dev, return_layers=True)
    assert torch.equal(same.cpu(), torch.zeros(2, dtype=torch.float64)) and not bool(same_layers.any())
    zero = ops.lpips(torch.zeros(1, 3, 31, 31, device=DEV), torch.zeros(1, 3, 31, 31, device=DEV), dev)
    assert torch.equal(zero.cpu(), torch.zeros(1, dtype=torch.float64))
    # nothing is clamped: a prediction outside [0, 1] is not the clamped one
    a = ops.lpips(pred.to(DEV), target.to(DEV), dev)
    assert float(pred.min()) < 0 and not torch.equal(a, ops.lpips(pred.clamp(0, 1).to(DEV), target.to(DEV), dev))
    assert torch.equal(a, ops.lpips(pred.to(DEV), target.to(DEV), dev))                  # run to run


def test_lpips_refuses_what_it_cannot_run():
    from joint_tensorf_amd import ops
    from joint_tensorf_amd._lib import JtError
    _, dev = _weights()
    with pytest.raises(JtError, match="unsupported shape"):
        ops.lpips(torch.zeros(1, 3, 30, 64, device=DEV), torch.zeros(1, 3, 30, 64, device=DEV), dev)
    with pytest.raises(ValueError, match=r"\[V, 3, H, W\]"):
        ops.lpips(torch.zeros(1, 1, 64, 64, device=DEV), torch.zeros(1, 1, 64, 64, device=DEV), dev)


def _weight_files(directory):
    a, b = state_dicts(random_weights(0))
    pa, pb = os.path.join(str(directory), "alexnet.pth"), os.path.join(str(directory), "alex.pth")
    torch.save(a, pa)
    torch.save(b, pb)
    return pa, pb


def _build(output_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import eval_dist_worker as W
    return W.build(output_path)


def test_evaluate_full_fills_the_lpips_column(tmp_path, capsys):
    """the model and the three views of tests/eval_dist_worker.py (40 x 40)"""
    from joint_tensorf_amd import ops
    from joint_tensorf_amd.options import Opt
    opt, model, views, pose_gt = _build(os.path.join(str(tmp_path), "plain"))
    assert opt.H >= 31 and opt.W >= 31
    # without the options: today's output
    np.random.seed(0)
    plain = model.evaluate_full(opt, views, pose_gt)
    text = capsys.readouterr().out
    assert "LPIPS" not in text and text.count("SSIM:") == 1
    assert "lpips" not in plain and "lpips_per_view" not in plain and all("lpips" not in r for r in plain.views)
    plain_lines = open(os.path.join(opt.output_path, "quant.txt")).read().splitlines()
    assert len(plain_lines) == 3 and all(ln.split(" ")[3] == "nan" for ln in plain_lines)
    # only one of the two: an error
    pa, pb = _weight_files(tmp_path)
    opt.eval = Opt(lpips=Opt(alexnet=pa))
    with pytest.raises(ValueError, match="both weight files"):
        model.evaluate_full(opt, views, pose_gt)
    # both
    opt.eval = Opt(lpips=Opt(alexnet=pa, linear=pb))
    opt.output_path = os.path.join(str(tmp_path), "with")
    capsys.readouterr()
    np.random.seed(0)
    res = model.evaluate_full(opt, views, pose_gt)
    text = capsys.readouterr().out
    assert text.count("LPIPS:") == 1 and text.index("SSIM:") < text.index("LPIPS:")
    assert "LPIPS: {:8.2f}".format(res.lpips) in text
    weights = model.lpips_weights(opt)
    assert weights is model.lpips_weights(opt)                                           # loaded and packed once
    lines = open(os.path.join(opt.output_path, "quant.txt")).read().splitlines()
    assert len(lines) == 3 and len(res.lpips_per_view) == 3
    for i, (ln, r) in enumerate(zip(lines, res.views)):
        want = float(ops.lpips(r.rgb_map, views[i].image, weights))
        f = ln.split(" ")
        print("view %d: lpips %r" % (i, want))
        assert len(f) == 4 and f[3] == repr(want) and math.isfinite(want) and want > 0
        assert r.lpips == want == res.lpips_per_view[i]
        assert f[:3] == plain_lines[i].split(" ")[:3]                                    # PSNR and SSIM as without it
    assert res.lpips == float(np.mean(res.lpips_per_view)) or abs(res.lpips - np.mean(res.lpips_per_view)) < 1e-15
    assert res.psnr_per_view == plain.psnr_per_view and res.ssim_per_view == plain.ssim_per_view


def test_two_rank_evaluation_gathers_lpips(tmp_path):
    """gloo on one device, as tests/test_gpu_metrics.py: every rank renders every second view; both return the complete LPIPS
    list, equal to the single process's, and rank 0 alone prints the line and writes quant.txt."""
    pa, pb = _weight_files(tmp_path)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "lpips_dist_worker.py"), str(tmp_path), pa, pb],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    from joint_tensorf_amd.options import Opt
    opt, model, views, pose_gt = _build(os.path.join(str(tmp_path), "one_process"))
    opt.eval = Opt(lpips=Opt(alexnet=pa, linear=pb))
    np.random.seed(0)
    one = model.evaluate_full(opt, views, pose_gt)
    assert len(one.lpips_per_view) == 3 and all(math.isfinite(v) and v > 0 for v in one.lpips_per_view)
    for rank in range(2):
        r = torch.load(os.path.join(str(tmp_path), "eval_rank%d.pt" % rank))
        assert r["lpips_per_view"] == one.lpips_per_view and r["lpips"] == one.lpips
        assert r["n_own_views"] == (2, 1)[rank]
    assert outs[0].count("LPIPS:") == 1 and outs[1].count("LPIPS:") == 0
    lines = open(os.path.join(str(tmp_path), "two_ranks", "quant.txt")).read().splitlines()
    assert [ln.split(" ")[3] for ln in lines] == [repr(v) for v in one.lpips_per_view]
    assert lines == open(os.path.join(str(tmp_path), "one_process", "quant.txt")).read().splitlines()
