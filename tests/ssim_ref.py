"""SSIM with stock torch ops on the CPU: what ops.ssim (csrc/jt_metrics.hip) is held to.

The definition is that of the `pytorch_ssim.ssim(img1, img2)` call of the reference's evaluation loop (model/nerf.py:550),
restated from the package's published formulation: an 11-tap Gaussian window (sigma 1.5) built as a FLOAT tensor and divided by
its float sum, the 2-D window its outer product, grouped conv2d with ZERO padding of 5 for the five moments, C1 = 0.01^2,
C2 = 0.03^2, the mean over channels and pixels.

  ssim_ref(pred, target)                       fp64 evaluation (the fp32 taps promoted; the 2-D window their exact product)
  ssim_ref(pred, target, dtype=torch.float32)  the stock-op fp32 formulation the reference would run (fp32 window, fp32 conv2d)
  ssim_ref(pred, target, padding="replicate")  a variant with another border rule (tests show that the border rule is pinned)
Each returns (per-view mean [V] and the map [V, C, H, W]) in `dtype`.
"""
import math

import torch
import torch.nn.functional as F

WINDOW, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps_fp32():
    """the package's 1-D window: python-double exponentials stored as floats, divided by their float sum"""
    g = torch.Tensor([math.exp(-(x - WINDOW // 2) ** 2 / float(2 * SIGMA ** 2)) for x in range(WINDOW)])
    return g / g.sum()


_WINDOWS = {}


def window_2d(channels, dtype, device="cpu"):
    """built once per (channels, dtype, device): a timed stock-op call must not pay for an upload"""
    key = (channels, dtype, str(device))
    if key not in _WINDOWS:
        _WINDOWS[key] = _window_2d(channels, dtype).to(device)
    return _WINDOWS[key]


def _window_2d(channels, dtype):
    g = taps_fp32()
    if dtype == torch.float32:
        w = g[:, None].mm(g[None, :])                   # the package: an fp32 matrix product
    else:
        w = g.to(dtype)[:, None] * g.to(dtype)[None, :]   # exact: two 24-bit significands
    return w.expand(channels, 1, WINDOW, WINDOW).contiguous()


def ssim_ref(pred, target, dtype=torch.float64, padding="zeros", device="cpu"):
    x, y = pred.detach().to(device, dtype), target.detach().to(device, dtype)
    C = x.shape[1]
    w = window_2d(C, dtype, device)
    pad = WINDOW // 2

    def filt(t):
        if padding == "zeros":
            return F.conv2d(t, w, padding=pad, groups=C)
        return F.conv2d(F.pad(t, (pad, pad, pad, pad), mode=padding), w, groups=C)
    mu1, mu2 = filt(x), filt(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = filt(x * x) - mu1_sq
    s2 = filt(y * y) - mu2_sq
    s12 = filt(x * y) - mu1_mu2
    smap = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return smap.mean(dim=(1, 2, 3)), smap


def smooth_pairs(V, H, W, noise, seed, device="cpu"):
    """Test pictures of the kind a Blender evaluation sees: a smooth random picture (a few low-frequency waves per channel) on
    the left half, constant white on the right; the prediction is the target + uniform noise of amplitude `noise`, clamped to
    [0, 1].  Returns (pred, target) [V, 3, H, W] fp32."""
    gen = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, H)[None, None, :, None]
    xx = torch.linspace(0, 1, W)[None, None, None, :]
    img = torch.full((V, 3, H, W), 0.5)
    for _ in range(4):
        fy, fx = torch.rand(V, 3, 1, 1, generator=gen) * 6 + 0.5, torch.rand(V, 3, 1, 1, generator=gen) * 6 + 0.5
        ph, amp = torch.rand(V, 3, 1, 1, generator=gen) * 6.2832, torch.rand(V, 3, 1, 1, generator=gen) * 0.2
        img = img + amp * torch.sin(6.2832 * (fy * yy + fx * xx) + ph)
    img = img.clamp(0, 1)
    img[..., W // 2:] = 1.0
    pred = (img + (torch.rand(V, 3, H, W, generator=gen) * 2 - 1) * noise).clamp(0, 1)
    return pred.float().to(device), img.float().to(device)


# the input set of the SSIM parity test (tests/test_gpu_metrics.py) and of the border-rule check (tests/test_eval_outputs.py):
# (name, V, H, W, noise amplitude).  Sizes below, at and above the 11-tap window, not multiples of the 32 x 16 tile, up to the
# full Blender frame; V = 32 (opt.optim.test_batch's ceiling) at 200 x 200 only, to keep memory small; three noise levels.
NOISE = (0.005, 0.05, 0.3)
PARITY_CASES = [
    ("7x9", 1, 7, 9, NOISE[1]), ("7x9", 3, 7, 9, NOISE[2]),
    ("11x11", 1, 11, 11, NOISE[0]), ("11x11", 3, 11, 11, NOISE[1]),
    ("37x53", 1, 37, 53, NOISE[2]), ("37x53", 3, 37, 53, NOISE[0]),
    ("200x200", 1, 200, 200, NOISE[0]), ("200x200", 3, 200, 200, NOISE[2]), ("200x200", 32, 200, 200, NOISE[1]),
    ("400x400", 1, 400, 400, NOISE[1]), ("400x400", 3, 400, 400, NOISE[0]),
    ("800x800", 1, 800, 800, NOISE[2]), ("800x800", 3, 800, 800, NOISE[0]),
]


def parity_inputs():
    """yields (label, pred, target) over PARITY_CASES plus the three degenerate pairs: identical, all-zero, two constants"""
    for k, (name, V, H, W, noise) in enumerate(PARITY_CASES):
        pred, target = smooth_pairs(V, H, W, noise, seed=100 + k)
        yield "%s V=%d noise=%g" % (name, V, noise), pred, target
    pred, target = smooth_pairs(2, 37, 53, 0.1, seed=7)
    yield "identical", target, target.clone()
    yield "all-zero", torch.zeros(1, 3, 37, 53), torch.zeros(1, 3, 37, 53)
    yield "constants", torch.full((1, 3, 37, 53), 0.25), torch.full((1, 3, 37, 53), 0.75)
