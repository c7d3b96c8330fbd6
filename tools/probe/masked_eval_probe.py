#!/usr/bin/env python3
"""The occlusion-robustness evaluation pass (MyHandler.test_model with a mask ratio) by three routes, one per process:

  resident_masked   clean dataset, test_model(mask_ratio=r): bags out of the device-resident cache, masked by the staging launch
  resident_clean    the same pass without a mask (what masking on the way into the slab may cost at most)
  host_masked       the only route there was before: the dataset zeroes the square instances on the host at every visit (as the
                    reference's __getitem__, dataset/PatchWSI.py:80-81) and is never cached -- every bag crosses PCIe in every pass.
                    `host_mask_s` is the part of each pass the host spent masking.

usage: masked_eval_probe.py ROUTE [--bags 64] [--rows 8192] [--ratio 0.8] [--passes 5] [--out FILE.jsonl]
Prints one JSON line (and appends it to --out): seconds and bags/s of every pass; the first pass fills the cache and is not part of
`bags_per_s` (second and later passes, median)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from advmil_amd import ingest  # noqa: E402
from advmil_amd.config import default_cfg  # noqa: E402
from advmil_amd.model import MyHandler  # noqa: E402
from advmil_amd.utils.func import random_mask_square_instance  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("route", choices=["resident_masked", "resident_clean", "host_masked"])
ap.add_argument("--bags", type=int, default=64)
ap.add_argument("--rows", type=int, default=8192)
ap.add_argument("--ratio", type=float, default=0.8)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--batch-bags", type=int, default=16)
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
hh = MyHandler(default_cfg(bcb_mode="abmil", bp_every_batch=16, cuda_id=0, gemm_mode="bf16x3"), device=dev)
g = torch.Generator().manual_seed(7)
items = [(torch.tensor([[i]], dtype=torch.int), [torch.randn(1, a.rows, 1024, generator=g), torch.zeros(1, 1)], torch.tensor([[0.3, 1.0]]))
         for i in range(a.bags)]
mask_s = [0.0]


class DS:
    ratio_mask = a.ratio if a.route == "host_masked" else None


class DL:
    def __init__(self, ds):
        self.dataset = ds

    def __iter__(self):
        for idx, (x, ext), y in items:
            if a.route == "host_masked":
                t0 = time.perf_counter()
                x = random_mask_square_instance(x[0], a.ratio).unsqueeze(0)
                mask_s[0] += time.perf_counter() - t0
            yield idx, [x, ext], y


dl = DL(DS())
np.random.seed(0)
secs, host = [], []
for p in range(a.passes):
    mask_s[0] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    MyHandler.test_model(hh.netG, hh.netD, "abmil", dl, batch_bags=a.batch_bags, mask_ratio=a.ratio if a.route == "resident_masked" else None)
    torch.cuda.synchronize()
    secs.append(time.perf_counter() - t0)
    host.append(mask_s[0])
later = sorted(secs[1:])
line = {"probe": "masked_eval", "route": a.route, "bags": a.bags, "rows": a.rows, "ratio": a.ratio, "batch_bags": a.batch_bags,
        "pass_s": [round(s, 5) for s in secs], "host_mask_s": [round(s, 5) for s in host],
        "bags_per_s": round(a.bags / later[len(later) // 2], 1), "bags_per_s_best": round(a.bags / later[0], 1),
        "bags_per_s_without_host_mask": round(a.bags / sorted(s - h for s, h in zip(secs[1:], host[1:]))[len(later) // 2], 1),
        "cache": ingest.device_bag_cache(dev).stats(), "device": torch.cuda.get_device_name(0)}
print(json.dumps(line), flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
