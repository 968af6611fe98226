#!/usr/bin/env python3
"""One rank of the two-process evaluation test (tests/test_gpu_metrics.py): a FRESH process, gloo rendezvous, every rank on
GPU 0.  Model.evaluate_full over three held-out views with an output path; writes what it returned to <out>/eval_rank<r>.pt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def build(output_path):
    """the fixture model of tests/test_gpu_eval.py and three held-out views.  Without the test-time pose optimisation: its host
    draws follow the order in which a process meets its views, which a rank that takes every second view does not share with
    the single process; the render and the metrics that this test is about draw nothing."""
    from joint_tensorf_amd.options import Opt
    from joint_tensorf_amd.synthetic import make_views
    from tests.golden_util import Fixture
    from tests.test_gpu_eval import _model
    fx = Fixture("blender_test_optim")
    opt, model = _model(fx)
    opt.optim.test_photo = False
    opt.output_path = output_path
    tv = make_views(opt, 3, seed=21, device="cuda")
    views = [Opt(idx=torch.arange(1, device="cuda"), pose=tv.pose[i:i + 1], intr=tv.intr[i:i + 1], intr_inv=tv.intr_inv[i:i + 1],
                 image=tv.image[i:i + 1]) for i in range(3)]
    return opt, model, views, fx.t("in.pose_gt", "cuda")


def main():
    out = sys.argv[1]
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    opt, model, views, pose_gt = build(os.path.join(out, "two_ranks"))
    np.random.seed(0)
    res = model.evaluate_full(opt, views, pose_gt)
    torch.save(dict(ssim_per_view=res.ssim_per_view, psnr_per_view=res.psnr_per_view, ssim=res.ssim, psnr=res.psnr,
                    n_own_views=len(res.views)), os.path.join(out, "eval_rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
