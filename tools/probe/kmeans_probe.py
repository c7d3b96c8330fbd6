#!/usr/bin/env python3
"""Dev probe: device time of the batched k-means (ops.kmeans_assign, ops.kmeans_update, wsicluster.kmeans; csrc/kmeans.hip) at C = 1024,
K = 8 for one bag of 8192 rows, one bag of 32768 rows and a slab of 16 patients of 8192 rows, beside two yardsticks taken in the same run:

  * the bytes each pass MUST move (assign: the two bf16 planes of X, 4 N C bytes; update: the fp32 rows, 4 N C bytes; labels, norms and
    centres are below 1 % of that) against the HBM roof DESIGN.md section 4 uses (8 TB/s nominal, 6.3 TB/s achievable: shares are of 6.3);
  * sklearn's KMeans(init=<the same K rows>, n_init=1, algorithm="lloyd") on the host's granted CPUs at N = 8192 (the numpy oracle
    tests/kmeans_ref.py where sklearn is not installed).

Timing: device events around each single call, REPEATS calls after a warm-up of every shape; median, min and max are recorded. The assign
figure is the steady-state call of the loop (planes split and row norms in place, labels and dist2 updated in place, `changed` counted);
the update figure writes the centres in place. The whole-run figure is wsicluster.kmeans from K stated rows (a host clock around a call
that ends in a readback), with its iteration count; the features are |N(0, 1)| (one overlapping cloud: many iterations).
usage: kmeans_probe.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from advmil_amd import ops, wsicluster  # noqa: E402

HBM_ROOF = 6.3e12
C, K, REPEATS = 1024, 8, 20
dev = "cuda:0"


def timed(fn, reps=REPEATS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    ts = np.array(ts)
    return dict(median_us=float(np.median(ts)) * 1e6, min_us=float(ts.min()) * 1e6, max_us=float(ts.max()) * 1e6, repeats=reps)


rows = []
for name, lens in (("1x8192", [8192]), ("1x32768", [32768]), ("16x8192", [8192] * 16)):
    N, nseg = sum(lens), len(lens)
    g = torch.Generator(device="cpu").manual_seed(N + nseg)
    x = torch.randn(N, C, generator=g).abs_().to(dev)
    seg = ops.Segments(lens, dev) if nseg > 1 else None
    offs = np.concatenate([[0], np.cumsum(lens)])
    pick = torch.as_tensor(np.concatenate([o + np.arange(K) * (n // K) for o, n in zip(offs[:-1], lens)])).to(dev)
    init = x.index_select(0, pick).reshape(nseg, K, C).contiguous()
    pl = x._advmil_planes = ops.split_planes(x)
    cent = init.clone()
    labels, d2, chg, ws = ops.kmeans_assign(x, cent, seg, None, None, return_dist=True, return_changed=True, planes=pl)
    t_as = timed(lambda: ops.kmeans_assign(x, cent, seg, None, labels, return_dist=d2, return_changed=True, planes=pl, norms=ws))
    count = torch.zeros(nseg, K, dtype=torch.int32, device=dev)
    scratch = cent.clone()
    t_up = timed(lambda: ops.kmeans_update(x, labels, scratch, seg, None, out=scratch, count=count))
    must = 4.0 * N * C
    runs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lab, info = wsicluster.kmeans(x, K, init=init if nseg > 1 else init[0], seg=seg, return_info=True)
        it = info["n_iter"].tolist()
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    row = dict(case=name, N=N, C=C, K=K, nseg=nseg, assign=t_as, update=t_up, bytes_per_pass=must,
               roof_us_per_pass=must / HBM_ROOF * 1e6, assign_share_of_hbm_roof=must / HBM_ROOF / (t_as["median_us"] * 1e-6),
               update_share_of_hbm_roof=must / HBM_ROOF / (t_up["median_us"] * 1e-6), kmeans_run_s=sorted(runs)[1], kmeans_run_s_all=runs,
               n_iter=it, ms_per_iteration=sorted(runs)[1] * 1e3 / max(it))
    if name == "1x8192":
        xn, c0 = x.cpu().numpy(), init[0].cpu().numpy()
        try:
            from sklearn.cluster import KMeans
            t0 = time.perf_counter()
            km = KMeans(n_clusters=K, init=c0, n_init=1, algorithm="lloyd", tol=1e-4, max_iter=300).fit(xn)
            row.update(host_yardstick="sklearn KMeans lloyd fp32", host_s=time.perf_counter() - t0, host_n_iter=int(km.n_iter_),
                       labels_differing_from_host=int((km.labels_ != lab.cpu().numpy()).sum()))
        except ImportError:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
            import kmeans_ref
            t0 = time.perf_counter()
            r = kmeans_ref.lloyd(xn, c0)
            row.update(host_yardstick="numpy float64 oracle", host_s=time.perf_counter() - t0, host_n_iter=int(r["n_iter"]),
                       labels_differing_from_host=int((r["labels"] != lab.cpu().numpy()).sum()))
        row["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0"))
    rows.append(row)
    print(json.dumps(row), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rows, f, indent=1)
