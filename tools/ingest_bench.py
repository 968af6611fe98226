#!/usr/bin/env python3
"""How long the dataset loaders' picture preprocessing takes, host against device, on the two set shapes the BAT yamls read:
100 views of 800 x 800 RGBA -> 400 x 400 over white (Blender) and 20 views of 3024 x 4032 RGB -> 480 x 640 (LLFF).  From one
process and the same decoded arrays:
  (a) host:   Pillow's LANCZOS resize + to_tensor + composite (datasets.preprocess_image_host) on the loader's thread count;
  (b) device: pinned buffer -> device copy + ops.image_ingest, HIP events around both, after a warm-up of the same shape;
  (c) decode: reading and decoding the files alone on the same threads -- it bounds what (b) can save of a load.
Needs the GPU; prints one JSON line per set.  usage: python tools/ingest_bench.py [--repeats 5] [--llff-views 20]"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dataset_scenes  # noqa: E402


def write_set(directory, n, h, w, c):
    """n files of the closed-form picture, shifted per view; PNG for RGBA (Blender), JPEG for RGB (the LLFF sets are photographs)"""
    from PIL import Image
    base = dataset_scenes.picture(h, w, c)
    files = []
    for k in range(n):
        a = np.roll(base, (37 * k, 101 * k), axis=(0, 1))
        path = os.path.join(directory, "view%03d.%s" % (k, "png" if c == 4 else "jpg"))
        Image.fromarray(a).save(path, **(dict(compress_level=1) if c == 4 else dict(quality=92)))
        files.append(path)
    return files


def measure(name, files, H, W, bg, threads, repeats):
    from joint_tensorf_amd import datasets, ops
    from joint_tensorf_amd.options import Opt
    opt = Opt(data=dict(bgcolor=bg))
    n = len(files)
    with ThreadPoolExecutor(max_workers=threads) as pool:
        t_decode = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            arrays = list(pool.map(datasets.decode, files))
            t_decode.append(time.perf_counter() - t0)
        t_host = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            host = list(pool.map(lambda a: datasets.preprocess_image_host(opt, a, H, W), arrays))
            t_host.append(time.perf_counter() - t0)
    h, w, c = arrays[0].shape
    pinned = torch.empty(n, h, w, c, dtype=torch.uint8).pin_memory()
    for i, a in enumerate(arrays):
        pinned[i] = torch.from_numpy(a)
    staged = torch.empty(n, h, w, c, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, 3, H, W, device="cuda")
    t_dev, t_kernel = [], []
    for r in range(repeats + 1):                       # (the first round is the warm-up: code object, tables, allocator)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        staged.copy_(pinned, non_blocking=True)
        e[1].record()
        ops.image_ingest(staged, out, H, W, bg)
        e[2].record()
        torch.cuda.synchronize()
        if r:
            t_dev.append(e[0].elapsed_time(e[2]) * 1e-3)
            t_kernel.append(e[1].elapsed_time(e[2]) * 1e-3)
    equal = all(torch.equal(out[i].cpu(), host[i]) for i in range(n))
    med = lambda v: round(float(np.median(v)) * 1e3, 2)
    return dict(set=name, views=n, source=[h, w, c], target=[H, W], threads=threads, repeats=repeats,
                host_pillow_torch_ms=med(t_host), device_upload_ingest_ms=med(t_dev), device_ingest_only_ms=med(t_kernel),
                decode_ms=med(t_decode), host_spread_ms=[med([min(t_host)]), med([max(t_host)])],
                device_spread_ms=[med([min(t_dev)]), med([max(t_dev)])], device_equals_host=equal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--blender-views", type=int, default=100)
    ap.add_argument("--llff-views", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ingest_bench.py measures the device path: it needs the GPU")
    from joint_tensorf_amd import datasets
    from joint_tensorf_amd.options import Opt
    threads = datasets.n_decode_threads(Opt(data=dict(num_workers=4)))
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, (h, w, c), (H, W), bg in (("blender", args.blender_views, (800, 800, 4), (400, 400), 1),
                                               ("llff", args.llff_views, (3024, 4032, 3), (480, 640), None)):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            files = write_set(d, n, h, w, c)
            print(json.dumps(measure(name, files, H, W, bg, threads, args.repeats)), flush=True)


if __name__ == "__main__":
    main()
