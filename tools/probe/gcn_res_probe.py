"""The residual block between the GENConv layers of a deep PatchGCN, out = dropout_p(x + relu(LayerNorm(h))), forward + backward, two
ways on the same tensors (N = 65536 rows = 16 graphs of 4096 nodes, d = 128 by default, p = 0.1):

  composed   ops.ln_relu + add + ops.dropout and their backwards      (needs nothing of csrc/gcnres.hip: runs on any earlier build too,
                                                                        ADVMIL_HIP_LIB names the library)
  fused      ops.gcn_res: advmil_gcn_res_fwd / advmil_gcn_res_bwd     one launch each way

    python tools/probe/gcn_res_probe.py --variant composed|fused [--rows 65536] [--d 128] [--iters 50]

One variant per process; alternate them on one box. One JSON line: device time per forward + backward pair and per forward alone
(events around `iters` repetitions, host-issued back to back), the backward as their difference, the host wall time per pair and, for
the fused form, the achieved bytes per second of each launch (forward: h, x read, out written, + the row statistics; backward: dout,
h read, dh, dx written, + the statistics)."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="fused", choices=("composed", "fused"))
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import torch
    from advmil_amd import _lib, ops
    _lib.lib()
    dev = torch.device("cuda", 0)
    N, d, p = args.rows, args.d, args.p
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *sh, k=1.0: (torch.randn(*sh, device=dev, generator=g) * k)   # noqa: E731
    h, x = rnd(N, d).requires_grad_(True), rnd(N, d).requires_grad_(True)
    gamma, beta = (1 + rnd(d, k=0.1)).requires_grad_(True), rnd(d, k=0.1).requires_grad_(True)
    dout = rnd(N, d)
    rng = ops.DeviceRng(dev, seed=11)

    def forward():
        if args.variant == "fused":
            return ops.gcn_res(h, x, gamma, beta, 1e-5, p, rng, "gcn_res1")
        return ops.dropout(x + ops.ln_relu(h, gamma, beta, 1e-5), p, rng, "gcn_res1")

    def pair():
        for t in (h, x, gamma, beta):
            t.grad = None
        forward().backward(dout)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters, (time.perf_counter() - t0) * 1e6 / args.iters

    pair_us, wall_us = timed(pair)
    fwd_us, _ = timed(forward)
    bwd_us = pair_us - fwd_us
    out = {"probe": "gcn_res", "tag": args.tag, "variant": args.variant, "rows": N, "d": d, "p": p, "iters": args.iters,
           "pair_us_device": round(pair_us, 2), "fwd_us_device": round(fwd_us, 2), "bwd_us_device": round(bwd_us, 2),
           "pair_us_wall": round(wall_us, 2)}
    if args.variant == "fused":
        out["fwd_TBps"] = round((3 * N * d + 2 * N) * 4 / fwd_us * 1e-6, 3)
        out["bwd_TBps"] = round((4 * N * d + 2 * N) * 4 / bwd_us * 1e-6, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
