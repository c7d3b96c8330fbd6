"""Launch count and eager step time of ONE single-process disc_gansurv optimizer step (16 bags of 8192 patches, abmil, time_bins = 4, the
shipped dropout): the figures of DESIGN.md section 7. bench.py does not run this task.

    python tools/probe/disc_step_probe.py [--root TREE] [--warmup 3] [--steps 100] [--runs 1] [--tag NAME]

--root: import advmil_amd from another checkout (its own built library), so that two commits can be timed alternately on one box. One
JSON line per run: C-ABI calls per step (counted on the host through _lib.check: every entry point that launches goes through it -- an
entry may enqueue more than one kernel, e.g. the fused head's two), which of them are head calls, and the step time (device events around
`steps` eager steps, host-issued back to back, divided by `steps`)."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--bags", type=int, default=16)
    ap.add_argument("--patches", type=int, default=8192)
    ap.add_argument("--bins", type=int, default=4)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from advmil_amd import _lib
    from advmil_amd.config import default_cfg
    from advmil_amd.model import MyHandler

    dev = torch.device("cuda", 0)
    nb, N, K = args.bags, args.patches, args.bins
    cfg = default_cfg(task="disc_gansurv", time_format="quantile", time_bins=K, gen_dims=f"384-{K}", disc_nety_in_dim=K, bcb_mode="abmil",
                      bp_every_batch=nb)
    h = MyHandler(cfg, device=dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    slab = torch.randn(nb, N, 1024, device=dev, generator=g)            # the bags back to back: the step slab is a zero-copy view
    xs = [[slab[i:i + 1], torch.zeros(1, 1, device=dev)] for i in range(nb)]
    ys_host = [torch.tensor([[float(i % K), float(i % 2)]]) for i in range(nb)]
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
    # ---- C-ABI calls of one step, by name
    names, real = [], _lib.check
    _lib.check = lambda code, what: (names.append(what), real(code, what))[1]
    try:
        step()
    finally:
        _lib.check = real
    torch.cuda.synchronize()
    heads = [n for n in names if n.startswith("ghead")]
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
        print(json.dumps({"probe": "disc_step", "tag": args.tag, "run": run, "bags": nb, "patches": N, "bins": K, "warmup": args.warmup,
                          "steps": args.steps, "abi_calls_per_step": len(names), "head_calls": heads,
                          "step_ms_device": round(e0.elapsed_time(e1) / args.steps, 4), "step_ms_wall": round(wall, 4)}), flush=True)


if __name__ == "__main__":
    main()
