"""Launch count and eager step time of ONE single-process optimizer step (16 bags of 8192 patches, abmil, the shipped dropout) with the
discriminator's region embedding set by --backbone avgpool | gapool: the figures of DESIGN.md section 7b. bench.py runs avgpool only.

    python tools/probe/gapool_step_probe.py --backbone gapool [--warmup 3] [--steps 50] [--runs 1] [--tag NAME]

One JSON line per run: C-ABI calls per step (counted on the host through _lib.check, as tools/probe/disc_step_probe.py counts them)
and the step time (device events around `steps` eager steps, host-issued back to back, divided by `steps`). Run once per process and
alternate the two backbones on one box."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--backbone", default="gapool", choices=("avgpool", "gapool"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--bags", type=int, default=16)
    ap.add_argument("--patches", type=int, default=8192)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from advmil_amd import _lib
    from advmil_amd.config import default_cfg
    from advmil_amd.model import MyHandler

    dev = torch.device("cuda", 0)
    nb, N = args.bags, args.patches
    h = MyHandler(default_cfg(bcb_mode="abmil", bp_every_batch=nb, disc_netx_backbone=args.backbone), device=dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    slab = torch.randn(nb, N, 1024, device=dev, generator=g)            # the bags back to back: the step slab is a zero-copy view
    xs = [[slab[i:i + 1], torch.zeros(1, 1, device=dev)] for i in range(nb)]
    ys_host = [torch.tensor([[0.05 + 0.055 * i, float(i % 2)]]) for i in range(nb)]
    ys = [y.to(dev) for y in ys_host]
    base = h.rng.counter

    def step():
        h.rng.counter = base
        plan = h._plan(xs, ys, "wlabel", None, ys_host)
        h._update_disc(0, xs, ys, "wlabel", None, ys_host=ys_host, plan=plan)
        h._update_gen(0, xs, ys, "wlabel", None, ys_host=ys_host, plan=plan)
        h.rng.advance(1)
        h.history.clear()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    names, real = [], _lib.check
    _lib.check = lambda code, what: (names.append(what), real(code, what))[1]
    try:
        step()
    finally:
        _lib.check = real
    torch.cuda.synchronize()
    for run in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / args.steps
        print(json.dumps({"probe": "gapool_step", "tag": args.tag, "backbone": args.backbone, "run": run, "bags": nb, "patches": N,
                          "warmup": args.warmup, "steps": args.steps, "abi_calls_per_step": len(names),
                          "gapool16_calls": sum(n.startswith("gapool16") for n in names),
                          "step_ms_device": round(e0.elapsed_time(e1) / args.steps, 4), "step_ms_wall": round(wall, 4)}), flush=True)


if __name__ == "__main__":
    main()
