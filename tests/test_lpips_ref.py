"""The host side of LPIPS (no GPU): the weight-file reader of joint_tensorf_amd/lpips.py, the layer geometry of the definition
(tests/lpips_ref.py), of the host mirror and of the C ABI, the options that switch the column on, and sanity of the reference
the device kernels are held to (tests/test_gpu_lpips.py)."""
import ctypes

import pytest
import torch

from tests.lpips_ref import features, lpips_ref, noisy_pairs, random_weights, scale_layer, state_dicts

# the five feature sizes of the issue's table
GEOMETRY = {(31, 31): [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)],
            (64, 64): [(15, 15), (7, 7), (3, 3), (3, 3), (3, 3)],
            (67, 95): [(16, 23), (7, 11), (3, 5), (3, 5), (3, 5)]}
CHANNELS = [64, 192, 384, 256, 256]


def _files(tmp_path, a, b):
    pa, pb = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth")
    torch.save(a, pa)
    torch.save(b, pb)
    return pa, pb


def test_loader_reads_the_two_files_and_names_what_is_wrong(tmp_path):
    from joint_tensorf_amd import lpips
    weights = random_weights(3)
    a, b = state_dicts(weights)
    a["classifier.1.weight"] = torch.zeros(4, 4)             # torchvision's file holds more than the convolutions
    conv, bias, lin = lpips.load_state_dicts(*_files(tmp_path, a, b))
    for l in range(5):
        assert torch.equal(conv[l], weights[0][l]) and torch.equal(bias[l], weights[1][l])
        assert lin[l].shape == (CHANNELS[l],) and torch.equal(lin[l], weights[2][l])
    # a missing key, a wrong shape and a wrong dtype, each by name
    bad = dict(a)
    del bad["features.6.bias"]
    with pytest.raises(ValueError, match=r"features\.6\.bias.*missing"):
        lpips.load_state_dicts(*_files(tmp_path, bad, b))
    bad = dict(a)
    bad["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.3\.weight.*\(192, 64, 5, 5\)"):
        lpips.load_state_dicts(*_files(tmp_path, bad, b))
    bad = dict(b)
    bad["lin2.model.1.weight"] = torch.zeros(1, 384, 1, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight.*float32"):
        lpips.load_state_dicts(*_files(tmp_path, a, bad))
    bad = dict(b)
    del bad["lin4.model.1.weight"]
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight.*missing"):
        lpips.load_state_dicts(*_files(tmp_path, a, bad))
    # weights_only=True: a file that needs arbitrary unpickling is refused by torch, not executed
    pa, pb = _files(tmp_path, a, b)
    torch.save({"features.0.weight": ValueError}, pa)
    with pytest.raises(Exception):
        lpips.load_state_dicts(pa, pb)


def test_layer_geometry():
    from joint_tensorf_amd import _lib, lpips
    weights = random_weights(0)
    for (H, W), want in GEOMETRY.items():
        feats = features(scale_layer(torch.zeros(1, 3, H, W), torch.float32), weights, torch.float32)
        assert [tuple(f.shape) for f in feats] == [(1, c, h, w) for c, (h, w) in zip(CHANNELS, want)], (H, W)
        assert lpips.feature_sizes(H, W) == want
        # the C ABI's plan of the same picture, for a batch of 2 x 3 pictures: sizes, and stacks that do not overlap
        table = (ctypes.c_int64 * 20)()
        assert _lib.lib.jt_lpips_feature_layout(3, H, W, table) == 0
        rows = [tuple(table[4 * l:4 * l + 4]) for l in range(5)]
        assert [r[1:] for r in rows] == [(c, h, w) for c, (h, w) in zip(CHANNELS, want)]
        spans = sorted((r[0], r[0] + 6 * r[1] * r[2] * r[3]) for r in rows)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[0][0] >= 6 * 3 * H * W
        assert spans[-1][1] * 4 <= _lib.lib.jt_lpips_workspace_bytes(3, H, W)


def test_reference_sanity():
    """identical pictures give exactly 0 in both precisions, more noise gives more, and the stock fp32 formulation sits within
    a few 1e-7 of the fp64 one: the figure the GPU test scales its bound by"""
    weights = random_weights(0)
    pred, target = noisy_pairs(2, 31, 40, 0.1, seed=1)
    z, zl = lpips_ref(target, target.clone(), weights)
    assert torch.equal(z, torch.zeros(2, dtype=torch.float64)) and torch.equal(zl, torch.zeros(2, 5, dtype=torch.float64))
    a, al = lpips_ref(pred, target, weights)
    b, _ = lpips_ref(noisy_pairs(2, 31, 40, 0.3, seed=1)[0], target, weights)
    assert a.dtype == torch.float64 and al.shape == (2, 5) and bool((al > 0).all()) and bool((b > a).all())
    assert torch.equal(al.sum(dim=1), a)
    f32, _ = lpips_ref(pred, target, weights, dtype=torch.float32)
    rel = ((f32.double() - a).abs() / a).max().item()
    print("stock fp32 against fp64: relative %.2e" % rel)
    assert f32.dtype == torch.float32 and rel < 1e-5


def test_options_switch_the_column_on():
    from joint_tensorf_amd import lpips
    from joint_tensorf_amd.options import Opt, apply_overrides, load_options, parse_overrides
    opt = load_options("bat_blender_VM")
    assert lpips.paths_from_options(opt) is None
    both = apply_overrides(load_options("bat_blender_VM"),
                           parse_overrides(["--eval.lpips.alexnet=/w/alexnet.pth", "--eval.lpips.linear=/w/alex.pth"]))
    assert lpips.paths_from_options(both) == ("/w/alexnet.pth", "/w/alex.pth")
    for one in ("--eval.lpips.alexnet=/w/alexnet.pth", "--eval.lpips.linear=/w/alex.pth"):
        half = apply_overrides(load_options("bat_blender_VM"), parse_overrides([one]))
        with pytest.raises(ValueError, match="both weight files"):
            lpips.paths_from_options(half)
    assert lpips.paths_from_options(Opt(eval=Opt(lpips=Opt(alexnet=None, linear=None)))) is None
