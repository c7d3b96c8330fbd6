#!/usr/bin/env python3
"""Wall time of ContSurv_Evaluator.compute with the full metric list (recorded in docs/DESIGN_HISTORY.md, not gated).

usage: evaluator_time.py                 the HIP path on the MI355X at n = 1000 and n = 60000 (collector on the host, as test_model
                                         returns it; median of 5 calls after one warm-up)
       evaluator_time.py --reference DIR the reference's evaluator (DIR = a checkout of it) on the CPU at n = 1000; its python pair
                                         loops make n = 60000 impractical"""
import functools
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def collector(n):
    g = torch.Generator().manual_seed(5)
    t = torch.rand(n, generator=g)
    e = (torch.rand(n, generator=g) < 0.5).float()
    return {"y": torch.stack([t, e], dim=1), "y_hat": torch.rand(n, 1, generator=g), "f_fake": 4 * torch.rand(n, 1, generator=g) - 2}


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--reference":
        sys.path.insert(0, sys.argv[2])
        from eval.evaluator import ContSurv_Evaluator
        from loss import utils as LU
        sizes, reps, sync = (1000,), 3, lambda: None
    else:
        from advmil_amd.eval import ContSurv_Evaluator
        from advmil_amd.loss import utils as LU
        sizes, reps, sync = (1000, 60000), 5, torch.cuda.synchronize
    ev = ContSurv_Evaluator(end_time=1.0, recon_loss=functools.partial(LU.recon_loss, alpha=0.3, gamma=0.137),
                            rank_loss=functools.partial(LU.rank_loss, gamma=0.137, add_weight=True),
                            disc_loss=functools.partial(LU.real_fake_loss, which="bce"))
    for n in sizes:
        data = collector(n)

        def once():
            r = ev.compute(data, ev.valid_metrics)
            sync()
            return r
        print(f"n = {n}: ContSurv_Evaluator.compute, {len(ev.valid_metrics)} metrics: {timed(once, reps) * 1e3:.2f} ms")


if __name__ == "__main__":
    main()
