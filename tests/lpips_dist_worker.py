#!/usr/bin/env python3
"""One rank of the two-process LPIPS evaluation test (tests/test_gpu_lpips.py): tests/eval_dist_worker.py's model and views with
the two weight files named; writes what Model.evaluate_full returned to <out>/eval_rank<r>.pt.
usage: lpips_dist_worker.py OUT ALEXNET_PTH LINEAR_PTH"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    out, alexnet, linear = sys.argv[1:4]
    import torch.distributed as dist
    from eval_dist_worker import build
    from joint_tensorf_amd.options import Opt
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    opt, model, views, pose_gt = build(os.path.join(out, "two_ranks"))
    opt.eval = Opt(lpips=Opt(alexnet=alexnet, linear=linear))
    np.random.seed(0)
    res = model.evaluate_full(opt, views, pose_gt)
    torch.save(dict(lpips_per_view=res.lpips_per_view, lpips=res.lpips, n_own_views=len(res.views)),
               os.path.join(out, "eval_rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
