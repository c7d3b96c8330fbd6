#!/usr/bin/env python3
"""Dev probe: device time of the two k-NN graph kernels (ops.knn_spatial, ops.knn_latent; csrc/knn.hip) at N in {4096, 8192, 32768},
C = 1024, k = 8, beside two yardsticks taken in the same run:

  * ops.gemm forming a [N, 4096] panel of X . X^T in bf16x3 (the contraction engine fed the same operand planes, no selection), scaled to N columns: the MFMA work
    of the latent search without its epilogue;
  * the numpy float64 brute force (Gram matrix + argpartition + sort of k + 1) at N = 8192 on the host's granted CPUs.

Timing: device events around REPS back-to-back calls after a warm-up of every shape; the latent figure includes its norm launch and
excludes the plane split (done once, outside the window, as a slab that carries its planes would). Achieved rate = 2 N^2 C / time,
against the nominal 833 TFLOP/s bf16x3 roof (2.5 PFLOP/s dense bf16 over three MFMAs per product).
usage: knn_probe.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from advmil_amd import ops  # noqa: E402

ROOF = 2.5e15 / 3.0
C, K, PANEL = 1024, 8, 4096
dev = "cuda:0"
ops.set_gemm_mode("bf16x3")


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


rows = []
for N in (4096, 8192, 32768):
    g = torch.Generator(device="cpu").manual_seed(N)
    x = torch.randn(N, C, generator=g).to(dev)
    side = int(np.ceil(np.sqrt(N)))
    cells = torch.randperm(side * side, generator=g)[:N]
    xy = (torch.stack([cells % side, cells // side], dim=1) * 256).to(torch.int32).to(dev)
    pl = x._advmil_planes = ops.split_planes(x)
    reps = 20 if N <= 8192 else 5
    t_sp = timed(lambda: ops.knn_spatial(xy, K), reps)
    t_lt = timed(lambda: ops.knn_latent(x, K), reps)
    out = torch.empty(N, PANEL, device=dev)
    t_gemm = timed(lambda: ops.gemm(x, x[:PANEL], True, True, N, PANEL, C, out=out, a_planes=pl, b_planes=pl.view_rows(0, PANEL)), reps) * (N / PANEL)
    flop = 2.0 * N * N * C
    row = dict(N=N, C=C, k=K, knn_spatial_ms=t_sp * 1e3, knn_latent_ms=t_lt * 1e3, gemm_panel_scaled_ms=t_gemm * 1e3,
               latent_tflops=flop / t_lt / 1e12, latent_share_of_bf16x3_roof=flop / t_lt / ROOF,
               gemm_tflops=flop / t_gemm / 1e12, latent_over_gemm=t_lt / t_gemm)
    if N == 8192:
        xn = x.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        n2 = (xn * xn).sum(axis=1)
        D = n2[:, None] + n2[None, :] - 2.0 * (xn @ xn.T)
        part = np.argpartition(D, K + 1, axis=1)[:, :K + 1]
        np.take_along_axis(part, np.argsort(np.take_along_axis(D, part, axis=1), axis=1, kind="stable"), axis=1)
        row["numpy_f64_bruteforce_s"] = time.perf_counter() - t0
        row["numpy_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0"))
    rows.append(row)
    print(json.dumps(row), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rows, f, indent=1)
