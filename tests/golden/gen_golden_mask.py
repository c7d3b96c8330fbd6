#!/usr/bin/env python3
"""Golden kept-region sets of the occlusion-robustness test's instance mask, drawn by the REAL reference function
(utils/func.py:14-40 random_mask_square_instance, way mask_zero), for advmil_amd.utils.func.square_instance_keep.

Runs only in the build container (the reference never travels); the fixture holds results only: tests/golden/mask_v1.npz.
Usage:  python tests/golden/gen_golden_mask.py

Under np.random.seed(7), as ONE stream of the global np.random, the reference masks bags of the (rows, ratio) pairs of CASES in
order. A bag is the column of its own row numbers, so the rows that survive name the kept regions. Recorded: the kept region
indices of every bag and the next np.random.randint draw behind the sequence, which pins how much of the stream was consumed
(ratio 1.0 still draws; 48 rows at 0.999 keep one region; 160 rows at 0.8 keep ONE region, not two: 10 * (1 - 0.8) is
1.9999999999999996).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SEED = 7
CASES = ((16, .8), (32, .5), (160, .8), (4096, .8), (48, 1.0), (48, .999), (8192, .1), (8192, .5))
NEXT_DRAW_BOUND = 1 << 30


def main():
    sys.path.insert(0, REF)
    from utils.func import random_mask_square_instance          # the reference's own
    out = {"seed": np.int64(SEED), "rows": np.array([n for n, _ in CASES], dtype=np.int64),
           "ratio": np.array([r for _, r in CASES], dtype=np.float64)}
    np.random.seed(SEED)
    for i, (n, ratio) in enumerate(CASES):
        bag = torch.arange(1, n + 1, dtype=torch.float32).reshape(n, 1)          # row j holds j + 1: a zero row is a masked row
        got = random_mask_square_instance(bag, ratio, scale=4, mask_way="mask_zero")
        kept_rows = torch.nonzero(got[:, 0]).reshape(-1).numpy()
        assert len(kept_rows) % 16 == 0 and np.array_equal(kept_rows.reshape(-1, 16) % 16, np.tile(np.arange(16), (len(kept_rows) // 16, 1)))
        out[f"keep_{i}"] = (kept_rows.reshape(-1, 16)[:, 0] // 16).astype(np.int64)
    out["next_draw"] = np.int64(np.random.randint(NEXT_DRAW_BOUND))
    np.savez(os.path.join(HERE, "mask_v1.npz"), **out)
    print({k: (v.tolist() if v.size <= 8 else v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
