"""Eager G+D step of MyHandler in graph mode (PatchGCN, dims 1024-128-128) over 16 bags of 4096 nodes (8-NN grid graphs), at a given
depth:

    python tools/probe/gcn_step_probe.py [--layers 1] [--bags 16] [--nodes 4096] [--steps 10]

--layers 1 sets no cfg key at all, so the same file runs on a checkout from before the depth keys existed (copy it there). One JSON
line: device time per step (events around `steps` steps after `warmup` steps) and the host wall time per step."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--bags", type=int, default=16)
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import torch
    from advmil_amd import synth
    from advmil_amd.config import default_cfg
    from advmil_amd.model import MyHandler
    dev = torch.device("cuda", 0)
    over = dict(bcb_mode="graph", bcb_dims="1024-128-128", gen_dims="128-1", bp_every_batch=args.bags)
    if args.layers != 1:
        over["bcb_gcn_layers"] = args.layers
    h = MyHandler(default_cfg(**over), device=dev)
    ei = torch.as_tensor(synth.grid_knn_graph(args.nodes, 8)).to(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    xs, ys_host = [], []
    for i in range(args.bags):
        x = torch.randn(1, args.nodes, 1024, device=dev, generator=g)
        xs.append([x, SimpleNamespace(x=x[0], edge_index=ei)])
        ys_host.append(torch.tensor([[0.2 + 0.04 * i, float(i % 2)]]))
    ys = [y.to(dev) for y in ys_host]

    def step():
        h._update_disc(0, xs, ys, ys_host=ys_host)
        h._update_gen(0, xs, ys, ys_host=ys_host)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    h.pop_logs()
    print(json.dumps({"probe": "gcn_step", "tag": args.tag, "layers": args.layers, "bags": args.bags, "nodes": args.nodes,
                      "steps": args.steps, "step_ms_device": round(e0.elapsed_time(e1) / args.steps, 3), "step_ms_wall": round(wall, 3)}),
          flush=True)


if __name__ == "__main__":
    main()
