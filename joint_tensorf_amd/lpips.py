"""The weights of LPIPS(alex), the `lpips.LPIPS(net="alex")` of model/nerf.py:33, read from the two files the user names:
torchvision's AlexNet state dict (its five convolutions) and the lpips package's `alex.pth` (the five 1x1 linear layers).
Neither file is part of this repository; ops.lpips runs on whatever weights of the right shapes it is handed."""
import torch

from . import _lib

# (key of the convolution in torchvision's AlexNet, Cout, Cin, kernel, stride, padding); a MaxPool2d(3, 2) precedes layers 1 and 2
LAYERS = (("features.0", 64, 3, 11, 4, 2), ("features.3", 192, 64, 5, 1, 2), ("features.6", 384, 192, 3, 1, 1),
          ("features.8", 256, 384, 3, 1, 1), ("features.10", 256, 256, 3, 1, 1))
LIN_KEYS = tuple("lin%d.model.1.weight" % l for l in range(5))


def feature_sizes(H, W):
    """[(h, w)] of the five feature stacks of an H x W picture"""
    out = []
    for l, (_, _, _, k, s, p) in enumerate(LAYERS):
        if l in (1, 2):
            H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        H, W = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        out.append((H, W))
    return out


class LpipsWeights:
    """conv [5] (packed for the kernel), bias [5], lin [5] on one device, and the struct of pointers jt_lpips_forward takes"""

    def __init__(self, conv, bias, lin):
        self.conv, self.bias, self.lin = list(conv), list(bias), list(lin)
        self._struct = _lib.JtLpipsWeights()
        for l in range(5):
            self._struct.conv[l] = _lib.ptr(self.conv[l])
            self._struct.bias[l] = _lib.ptr(self.bias[l])
            self._struct.lin[l] = _lib.ptr(self.lin[l])

    @property
    def device(self):
        return self.conv[0].device

    def struct(self, device):
        if torch.device(device) != self.device:
            raise ValueError("lpips: the weights live on %s, the pictures on %s" % (self.device, device))
        return self._struct


def _take(sd, key, shape, path):
    if key not in sd:
        raise ValueError("%s: key %r is missing" % (path, key))
    t = sd[key]
    if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError("%s: key %r must be float32 %s, got %s %s" % (
            path, key, tuple(shape), getattr(t, "dtype", type(t).__name__), tuple(getattr(t, "shape", ()))))
    return t


def check_state_dicts(alexnet_sd, linear_sd, alexnet_path="alexnet", linear_path="linear"):
    """every key, shape and dtype LPIPS(alex) reads; a ValueError names the first key that is missing or wrong.  Returns
    (conv weights [5], biases [5], lin [5] as [C]) on the host."""
    conv, bias, lin = [], [], []
    for l, (key, cout, cin, k, _, _) in enumerate(LAYERS):
        conv.append(_take(alexnet_sd, key + ".weight", (cout, cin, k, k), alexnet_path))
        bias.append(_take(alexnet_sd, key + ".bias", (cout,), alexnet_path))
        lin.append(_take(linear_sd, LIN_KEYS[l], (1, cout, 1, 1), linear_path).reshape(cout))
    return conv, bias, lin


def pack(conv, bias, lin, device="cuda"):
    """host or device tensors of the shapes check_state_dicts returns -> LpipsWeights on `device` (one pack launch per layer)"""
    from . import ops
    dev = torch.device(device)
    return LpipsWeights([ops.conv_pack_weights(w.to(dev)) for w in conv], [b.to(dev, torch.float32).contiguous() for b in bias],
                        [v.to(dev, torch.float32).reshape(-1).contiguous() for v in lin])


def load_state_dicts(alexnet_path, linear_path):
    """the two files, read with weights_only=True and checked (host tensors)"""
    a = torch.load(alexnet_path, map_location="cpu", weights_only=True)
    b = torch.load(linear_path, map_location="cpu", weights_only=True)
    if not isinstance(a, dict) or not isinstance(b, dict):
        raise ValueError("lpips.load_weights: %s and %s must each hold a state dict" % (alexnet_path, linear_path))
    return check_state_dicts(a, b, str(alexnet_path), str(linear_path))


def load_weights(alexnet_path, linear_path, device="cuda"):
    """torchvision's AlexNet state dict (keys features.{0,3,6,8,10}.{weight,bias}) and the lpips package's alex.pth (keys
    lin{0..4}.model.1.weight, [1, C, 1, 1]) -> LpipsWeights on `device`, the convolution weights packed once"""
    return pack(*load_state_dicts(alexnet_path, linear_path), device=device)


def paths_from_options(opt):
    """(alexnet, linear) of opt.eval.lpips, or None when neither is set; exactly one set is a ValueError"""
    node = opt.get("eval", None) if hasattr(opt, "get") else None
    node = node.get("lpips", None) if isinstance(node, dict) else None
    a = node.get("alexnet", None) if isinstance(node, dict) else None
    b = node.get("linear", None) if isinstance(node, dict) else None
    if not a and not b:
        return None
    if not a or not b:
        raise ValueError("LPIPS needs both weight files: eval.lpips.alexnet=%r, eval.lpips.linear=%r" % (a, b))
    return str(a), str(b)
