"""`python -m joint_tensorf_amd.train --yaml=bat_blender_VM --data.root=DIR --data.scene=lego --output_path=OUT
[--key.sub=value ...] [--compress=F]`: the reference's entry point (train_3d.py:61-107) on this package's engine -- train
on an image set read by the native loaders (datasets.py), write the checkpoint, then evaluate the held-out split
(quant.txt, quant_pose.txt, test_view/) and render the novel views.

Every `--key.sub=value` is one of the reference's dotted overrides (options.parse_overrides); `--compress=F` shortens the
schedule by F without changing its shape (options.compress_schedule).  No other flags."""
import os
import shutil
import sys

import numpy as np
import torch


def build_options(argv):
    from .options import apply_overrides, compress_schedule, load_options, parse_overrides
    over = parse_overrides(argv)
    name = over.pop("yaml", None)
    if not isinstance(name, str):
        raise SystemExit("usage: python -m joint_tensorf_amd.train --yaml=NAME --data.root=DIR --output_path=OUT [--key.sub=value ...]")
    factor = over.pop("compress", 1)
    opt = apply_overrides(load_options(name), over)
    compress_schedule(opt, factor)
    if "device" not in opt:
        opt.device = "cuda:0"
    opt.H, opt.W = (int(v) for v in opt.data.image_size)
    return opt


def main(argv=None):
    """Returns the trained Model (its .eval_result holds what evaluate_full returned)."""
    from .model import bat_hip
    from .options import Opt
    opt = build_options(sys.argv[1:] if argv is None else list(argv))
    if not opt.get("output_path", None):
        raise SystemExit("--output_path=OUT is required: the checkpoint and the result files go there")
    torch.manual_seed(int(opt.get("seed", 0)))
    np.random.seed(int(opt.get("seed", 0)))
    dev = torch.device(opt.device)
    # ---- train_3d.py:61-80 ----
    if os.path.exists(opt.output_path) and not opt.get("resume", False):
        shutil.rmtree(opt.output_path)
    os.makedirs(opt.output_path, exist_ok=True)
    with torch.cuda.device(dev):
        m = bat_hip.Model(opt)
        m.load_dataset(opt, train_split="train")
        print("joint_tensorf_amd.train: opt.data.dataset_class = %s, %d training views at %d x %d"
              % (opt.data.get("dataset_class", None), len(m.train_data), opt.H, opt.W), flush=True)
        m.build_networks(opt)
        m.setup_optimizer(opt)
        m.restore_checkpoint(opt)
        m.setup_visualizer(opt)
        m.train(opt)
        # ---- train_3d.py:88-107 ----
        opt2 = Opt({k: v for k, v in opt.items() if k != "resume"})
        opt2.load = "{0}/model.ckpt".format(opt.output_path)
        e = bat_hip.Model(opt2)
        e.load_dataset(opt2, eval_split="test", train_split="train")
        e.build_networks(opt2)
        e.restore_checkpoint(opt2)
        e.freeze_scene(opt2)
        e.freeze_poses(opt2)
        m.eval_result = e.evaluate_full(opt2)
        e.generate_videos_synthesis(opt2)
        print("joint_tensorf_amd.train: PSNR %.3f over %d held-out views; results in %s"
              % (float(m.eval_result.psnr), len(m.eval_result.psnr_per_view), opt.output_path), flush=True)
    return m


if __name__ == "__main__":
    main()
