#!/usr/bin/env python3
"""Randomised check of the GENConv softmax-aggregation gather kernels (ops.genconv_aggregate -> advmil_genconv_fwd / _bwd over the two
CSR images of the graph) against float64 on RANDOM graphs -- not only the 8-NN grids of the WSI pipeline: random in-degrees 0 .. 40
(isolated nodes, hubs by target and by source, self loops, multi-edges), 1 .. 20000 nodes, channel widths 64 / 128 / 256, temperatures
0.3 .. 3 of either sign (t is a learnable Parameter), feature scales up to 2, forward and both gradients (x, t). The aggregation
restated in float64 is the published GENConv message passing (oracle header: PARITY UNPINNED against torch_geometric itself).

The C == 128 kernels pick their walk from the graph (csrc/graph.hip): a workgroup owns 8 S consecutive nodes, S = clamp(N // 4096, 1, 16),
and reads the tile's edge indices from LDS when the tile holds <= 2048 of them, from global memory otherwise; t < 0 takes the running
minimum. Every case's S, largest tile in each CSR image and sign of t are worked out on the host; `--plan` prints them without a GPU
(the same draws as the run), and a run of >= 40 cases that never reached S > 1, an unstaged forward tile, an unstaged backward tile
or t < 0 among its C == 128 cases does not report `all ok`.
usage: graph_fuzz.py [cases] [seed] [--plan]"""
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# csrc/graph.hip: GT_EDGES, GT_MAXS and the 8 * 512 of tile_nodes_for() (pinned to the source text by tests/test_genconv_plan_cpu.py)
GT_EDGES, GT_MAXS, TILE_DIV = 2048, 16, 8 * 512
FACTS = ("S > 1", "forward unstaged", "backward unstaged", "t < 0")


def tile_facts(key, N):
    """(S, edges of the largest tile) of the CSR image sorted by `key` (targets: the forward's, sources: the backward's)."""
    S = min(max(N // TILE_DIV, 1), GT_MAXS)
    counts = torch.bincount(key, minlength=N) if key.numel() else torch.zeros(N, dtype=torch.long)
    pad = (-N) % (8 * S)
    tiles = torch.cat([counts, counts.new_zeros(pad)]).view(-1, 8 * S).sum(1)
    return S, int(tiles.max())


def ref(x, t, ei, go, eps=1e-7):
    """-> out, and the uncancelled magnitude of dt (see below); call .backward on (out * go).sum() for the gradients."""
    src, dst = ei[0], ei[1]
    n, d = x.shape
    msg = torch.relu(x[src]) + eps
    z = msg * t
    zmax = torch.full((n, d), -float("inf"), dtype=x.dtype).scatter_reduce(0, dst[:, None].expand(-1, d), z, reduce="amax", include_self=True)
    e = torch.exp(z - zmax[dst])
    den = torch.zeros(n, d, dtype=x.dtype).index_add_(0, dst, e)
    w = e / den[dst]
    agg = torch.zeros(n, d, dtype=x.dtype).index_add_(0, dst, w * msg)
    # dt = sum over (edge, channel) of dout w msg (msg - sum w msg): signed terms that largely cancel -> measure the error against the
    # sum of their magnitudes (what an fp32 accumulation can resolve), not against the cancelled total
    # (the uncancelled products w msg^2 and w msg agg: the kernel forms the difference of two fp32 sums)
    with torch.no_grad():
        mag = float((go[dst].abs() * w * msg * (msg + agg[dst])).sum()) if ei.shape[1] else 0.0
    return agg + x, mag


def draw(rnd, g):
    """One case: every draw of the run, so that --plan sees the cases the run sees."""
    N = rnd.choice((1, 7, 64, 500, 4096, rnd.randint(2, 9000), rnd.randint(8192, 20000), rnd.randint(8192, 20000)))
    C = rnd.choice((64, 128, 128, 128, 256))
    kind = rnd.choice(("sparse", "dense", "hub", "dense_hub", "fanout", "none"))
    deg = {"sparse": 3, "dense": 24, "hub": 8, "dense_hub": 12, "fanout": 12, "none": 0}[kind]
    E = N * deg
    if E * C > 1 << 26:                                   # (the float64 restatement holds about ten E x C arrays at once)
        C = 128
    if E:
        src = torch.randint(0, N, (E,), generator=g)
        dst = torch.randint(0, N, (E,), generator=g)
        if kind == "hub":                                 # a few targets collect a third of all edges
            dst[: E // 3] = torch.randint(0, max(1, N // 50), (E // 3,), generator=g)
        if kind == "dense_hub":                           # ... half of them: ~300 in-edges each, 8 neighbouring hubs pass 2048 per tile
            dst[: E // 2] = torch.randint(0, max(1, N // 50), (E // 2,), generator=g)
        if kind == "fanout":                              # the same by source: the backward's tiles
            src[: E // 2] = torch.randint(0, max(1, N // 50), (E // 2,), generator=g)
        ei = torch.stack([src, dst])
    else:
        ei = torch.zeros(2, 0, dtype=torch.long)
    x = torch.randn(N, C, generator=g) * rnd.choice((0.5, 1.0, 2.0))       # (scale 4 x t 3 puts z = t msg at 40: the hubs' dx then reaches 1e-5)
    t = torch.tensor([rnd.uniform(0.3, 3.0) * rnd.choice((1.0, 1.0, -1.0))])
    go = torch.randn(N, C, generator=g)
    S, ftile = tile_facts(ei[1], N)
    _, btile = tile_facts(ei[0], N)
    wide = C == 128                                       # the tiled kernels; the other widths walk a wave per node
    hits = (wide and S > 1, wide and ftile > GT_EDGES, wide and btile > GT_EDGES, wide and float(t) < 0)
    return dict(N=N, C=C, kind=kind, E=E, ei=ei, x=x, t=t, go=go, S=S, ftile=ftile, btile=btile, hits=hits)


def main(argv):
    plan = "--plan" in argv
    args = [a for a in argv if a != "--plan"]
    ncase = int(args[0]) if len(args) > 0 else 60
    rnd = random.Random(int(args[1]) if len(args) > 1 else 1)
    g = torch.Generator().manual_seed(rnd.randrange(1 << 30))
    if not plan:
        sys.path.insert(0, ROOT)
        from advmil_amd import ops
        dev = "cuda:0"
    count = [0, 0, 0, 0]
    worst = [0.0, 0.0, 0.0]
    for case in range(ncase):
        c = draw(rnd, g)
        N, C, kind, E, ei, x, t, go = (c[k] for k in ("N", "C", "kind", "E", "ei", "x", "t", "go"))
        count = [n + bool(h) for n, h in zip(count, c["hits"])]
        if plan:
            print(f"case {case}: {kind} graph N {N} E {E} C {C} t {float(t):.2f}: S {c['S']} forward tile {c['ftile']} backward tile "
                  f"{c['btile']} sign {'-' if float(t) < 0 else '+'}", flush=True)
            continue
        xd, td = x.clone().to(dev).requires_grad_(True), t.clone().to(dev).requires_grad_(True)
        csr = ops.GraphCSR(ei.to(dev), N)
        out = ops.genconv_aggregate(xd, td, csr)
        (out * go.to(dev)).sum().backward()
        xr, tr = x.clone().double().requires_grad_(True), t.clone().double().requires_grad_(True)
        orf, mag = ref(xr, tr, ei, go.double())
        (orf * go.double()).sum().backward()
        rel = lambda a, b: float((a.detach().cpu().double() - b).abs().max() / (b.abs().max() + 1e-30))
        e_o, e_x = rel(out, orf.detach()), rel(xd.grad, xr.grad)
        e_t = abs(float(td.grad) - float(tr.grad)) / (mag + 1e-30) if mag > 0 else abs(float(td.grad) - float(tr.grad))
        worst = [max(worst[0], e_o), max(worst[1], e_x), max(worst[2], e_t)]
        ok = e_o < 4e-6 and e_x < 2e-5 and e_t < 2e-6       # (fp32 sums over 100-400 in-edges at the hubs: dx 1e-5 there, 4e-7 on grids)
        if not ok or case % 10 == 0:
            print(f"case {case}: {kind} graph N {N} E {E} C {C} t {float(t):.2f}: out {e_o:.1e} dx {e_x:.1e} dt {e_t:.1e} {'ok' if ok else 'FAIL'}", flush=True)
        if not ok:
            return 1
    reached = "; ".join(f"{name}: {n}" for name, n in zip(FACTS, count))
    if plan:
        print(f"plan; {ncase} cases; C == 128 cases with {reached}")
        return 0
    if ncase >= 40 and not all(count):
        print(f"cases passed, but a walk was never reached; {ncase} cases; {reached}")
        return 1
    print("all ok;", ncase, "cases; worst out / dx / dt:", worst, ";", reached)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
