"""LPIPS(alex) with stock torch ops on the CPU: what ops.lpips (csrc/jt_lpips.hip) is held to.

The definition is that of the `lpips.LPIPS(net="alex")(rgb_map * 2 - 1, image * 2 - 1)` call of the reference's evaluation loop
(model/nerf.py:33,551), restated from the package's published formulation: the scaling layer (x - shift) / scale, torchvision's
AlexNet feature stack with a tap after each of the five ReLUs, every tap divided by its channel norm + 1e-10, the squared
difference weighted by a 1x1 convolution, the spatial mean, the sum over the five layers.

  lpips_ref(pred, target, weights)                       fp64 evaluation (the reference)
  lpips_ref(pred, target, weights, dtype=torch.float32)  the stock-op fp32 formulation, for comparison
Each returns (per-view value [V], per-layer terms [V, 5]) in `dtype`.  `weights` = (conv [5], bias [5], lin [5]) fp32 tensors,
as random_weights builds them and joint_tensorf_amd.lpips.check_state_dicts returns them.
"""
import torch
import torch.nn.functional as F

from joint_tensorf_amd.lpips import LAYERS, LIN_KEYS

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def random_weights(seed=0):
    """conv weights randn * sqrt(2 / K), bias 0.1 * randn, lin = rand / C (non-negative, as the trained ones are)"""
    gen = torch.Generator().manual_seed(seed)
    conv, bias, lin = [], [], []
    for _, cout, cin, k, _, _ in LAYERS:
        K = cin * k * k
        conv.append((torch.randn(cout, cin, k, k, generator=gen) * (2.0 / K) ** 0.5).float())
        bias.append((0.1 * torch.randn(cout, generator=gen)).float())
        lin.append((torch.rand(cout, generator=gen) / cout).float())
    return conv, bias, lin


def state_dicts(weights):
    """the two state dicts of the weight files, with the key names of torchvision's AlexNet and of the lpips package"""
    conv, bias, lin = weights
    a, b = {}, {}
    for l, (key, cout, _, _, _, _) in enumerate(LAYERS):
        a[key + ".weight"], a[key + ".bias"] = conv[l].clone(), bias[l].clone()
        b[LIN_KEYS[l]] = lin[l].reshape(1, cout, 1, 1).clone()
    return a, b


def noisy_pairs(V, H, W, noise, seed):
    """Pictures of the test set: box-blurred uniform noise (a smooth picture) as the target, plus Gaussian noise of standard
    deviation `noise` as the prediction, NOT clamped; both rounded to fp32 first, so every evaluation sees the same inputs."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(V, 3, H + 8, W + 8, generator=gen, dtype=torch.float64)
    target = F.avg_pool2d(base, 9, stride=1)
    pred = target + noise * torch.randn(V, 3, H, W, generator=gen, dtype=torch.float64)
    return pred.float(), target.float()


def scale_layer(x, dtype):
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return ((x.to(dtype) * 2 - 1) - shift) / scale


def features(x, weights, dtype=torch.float64):
    """the five taps of a batch [B, 3, H, W] that has been through scale_layer"""
    conv, bias, _ = weights
    out = []
    for l, (_, _, _, _, stride, pad) in enumerate(LAYERS):
        if l in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, conv[l].to(dtype), bias[l].to(dtype), stride=stride, padding=pad))
        out.append(x)
    return out


def head(feats0, feats1, lin, dtype=torch.float64):
    """per-layer terms [V, 5] of two lists of five feature stacks"""
    terms = []
    for f0, f1, w in zip(feats0, feats1, lin):
        f0, f1 = f0.to(dtype), f1.to(dtype)
        n0 = f0.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10
        n1 = f1.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10
        d = (f0 / n0 - f1 / n1).pow(2)
        terms.append((d * w.to(dtype).view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2)))
    return torch.stack(terms, dim=1)


def lpips_ref(pred, target, weights, dtype=torch.float64):
    f0 = features(scale_layer(pred.detach().cpu(), dtype), weights, dtype)
    f1 = features(scale_layer(target.detach().cpu(), dtype), weights, dtype)
    layers = head(f0, f1, weights[2], dtype)
    return layers.sum(dim=1), layers
