"""The tail of the gapool region embedding behind its FC -- LayerNorm + ReLU, the gate scorer, the 16-row attention pooling -- forward +
backward, two ways on the same tensors (N = 131072 rows, d = 128 by default):

  dedicated    ops.ln_relu -> ops.gate_scores -> ops.gapool16            csrc/gapool16.hip: the pooling as one launch each way
  composition  ops.ln_relu -> ops.gated_attn_pool(seg=Segments([16] * R))  the bag-level segmented kernels with 16-row segments; the
                                                                           offsets and row ids are built per call, as a step would

    python tools/probe/gapool16_probe.py --variant dedicated|composition|composition_cached [--rows 131072] [--d 128] [--iters 50]

composition_cached builds the segment arrays once, outside the timed loop. One variant per process; alternate them on one box. One JSON
line: device time per forward + backward pair (events around `iters` pairs, host-issued back to back) and the host wall time per pair."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="dedicated", choices=("dedicated", "composition", "composition_cached"))
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import torch
    from advmil_amd import _lib, ops
    _lib.lib()
    dev = torch.device("cuda", 0)
    N, d = args.rows, args.d
    R = N // 16
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *sh, k=1.0: (torch.randn(*sh, device=dev, generator=g) * k)   # noqa: E731
    y = rnd(N, d).requires_grad_(True)
    gamma, beta = (1 + rnd(d, k=0.1)).requires_grad_(True), rnd(d, k=0.1).requires_grad_(True)
    Wa, Wb = rnd(d, d, k=d ** -0.5).requires_grad_(True), rnd(d, d, k=d ** -0.5).requires_grad_(True)
    ba, bb = rnd(d, k=0.1).requires_grad_(True), rnd(d, k=0.1).requires_grad_(True)
    wc, bc = rnd(1, d, k=d ** -0.5).requires_grad_(True), rnd(1, k=0.1).requires_grad_(True)
    params = (y, gamma, beta, Wa, ba, Wb, bb, wc, bc)
    demb = rnd(R, d)
    seg0 = ops.Segments([16] * R, dev)

    def pair(variant):
        for p in params:
            p.grad = None
        z = ops.ln_relu(y, gamma, beta, 1e-5)
        if variant == "dedicated":
            emb, _ = ops.gapool16(ops.gate_scores(z, Wa, ba, Wb, bb, wc, bc, 0.0), z)
        else:
            seg = seg0 if variant == "composition_cached" else ops.Segments([16] * R, dev)
            emb, _, _ = ops.gated_attn_pool(z, Wa, ba, Wb, bb, wc, bc, 0.0, seg=seg)
        emb.backward(demb)
        return emb

    for _ in range(args.warmup):
        pair(args.variant)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.iters):
        pair(args.variant)
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e6 / args.iters
    print(json.dumps({"probe": "gapool16", "tag": args.tag, "variant": args.variant, "rows": N, "d": d, "iters": args.iters,
                      "gemm_mode": ops.get_gemm_mode(), "pair_us_device": round(e0.elapsed_time(e1) * 1e3 / args.iters, 2),
                      "pair_us_wall": round(wall, 2)}), flush=True)


if __name__ == "__main__":
    main()
