"""GPU: every walk of the GENConv gather kernels (csrc/graph.hip) against the float64 restatement of the aggregation.

The C == 128 kernels pick their path from the graph: a workgroup owns a tile of 8 S consecutive nodes, S = clamp(N // 4096, 1, 16);
half-wave h walks nodes h, h + 8, ... of the tile as one software-pipelined run of edge chunks (8 edges forward, 4 backward); the
tile's edge indices come from LDS when the tile holds <= 2048 edges and from global memory otherwise; t < 0 takes the running minimum
of the messages; any other width, or one pointer off 16-byte alignment, takes the generic wave-per-node kernels. Each case below
names the path it is aimed at and ASSERTS ON THE HOST, before it launches, that its graph is there (`walk_facts`, which mirrors
tile_nodes_for() and sums the edges per tile from the CSR row pointers; its three constants are pinned to the source text by
tests/test_genconv_plan_cpu.py).

Bounds: the project's own (test_genconv_on_random_graph_and_without_edges, tools/probe/graph_fuzz.py): out 4e-6 and dx 2e-5 of the
reference maximum, dt 2e-6 of the uncancelled magnitude sum |dout| w m (m + agg). They were measured for |t| <= 3, x scale <= 2,
degree <= 400, N <= 9000. Two regimes here lie outside that: dt at 65549 nodes, and the score gaps of the five-chunk rescale cases
(|t| m log2 e up to 130). There the bound is max(project bound, 4 e32), e32 = the error of the SAME restatement evaluated in float32 on
the host against its float64 self (the reference's own fp32 sensitivity; 4 for the different summation order) -- never a figure
taken from the kernels. Measured on an MI355X when this file was written: see `test_degree_ladders_across_the_walk` and
`test_online_rescale_under_large_score_gaps`.

`float64_body` is the one body every case runs (tests/test_poison_kernels_gpu.py runs it under poisoned allocations)."""
import collections
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GT_EDGES, GT_MAXS, TILE_DIV = 2048, 16, 8 * 512          # csrc/graph.hip (tests/test_genconv_plan_cpu.py pins them)
FWD_CH, BWD_CH = 8, 4                                     # edges per chunk: forward, GENCONV_BWD_CH
BOUND = dict(out=4e-6, dx=2e-5, dt=2e-6)
LADDER_IN = (0, 1, 7, 8, 9, 15, 16, 17, 0, 24, 8)         # in-degrees: empty / on, one short of and one past the 8-edge chunk
LADDER_OUT = (0, 1, 3, 4, 5, 7, 8, 9, 0, 13, 4)           # out-degrees: the same around the backward's 4-edge chunk

Facts = collections.namedtuple("Facts", "S tile_max deg_max tiles")


# ------------------------------------------------------------------------------------------------------------------------------
# host side: where a graph puts the kernels
# ------------------------------------------------------------------------------------------------------------------------------
def tile_nodes_for(N):
    return 8 * min(max(N // TILE_DIV, 1), GT_MAXS)


def rowptr_of(key, N):
    """Row pointers of the CSR image sorted by `key` (ops.GraphCSR._csr)."""
    rp = torch.zeros(N + 1, dtype=torch.long)
    if key.numel():
        rp[1:] = torch.cumsum(torch.bincount(key, minlength=N), 0)
    return rp


def walk_facts(rowptr, N):
    """S, the edges of the largest tile, the largest degree and every tile's edge count, from a CSR rowptr (plain Python)."""
    rp = [int(v) for v in rowptr]
    tn = tile_nodes_for(N)
    tiles = [rp[min(i + tn, N)] - rp[i] for i in range(0, N, tn)]
    return Facts(tn // 8, max(tiles), max(rp[i + 1] - rp[i] for i in range(N)), tiles)


def facts_of(ei, N):
    """(forward facts: by target, backward facts: by source)."""
    return walk_facts(rowptr_of(ei[1], N), N), walk_facts(rowptr_of(ei[0], N), N)


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 restatement (scatter_reduce amax / index_add_: any sign of t), evaluated in `dtype`
# ------------------------------------------------------------------------------------------------------------------------------
def restate(x, t, ei, go, dtype=torch.float64, eps=1e-7):
    """-> dict(out, dx, dt, mag): out_i = sum_j softmax_j(t m_j) m_j + x_i, m = relu(x) + eps, the gradients of (out * go).sum(), and
    the uncancelled magnitude of dt, sum |dout| w m (m + agg)."""
    src, dst = ei[0], ei[1]
    N, C = x.shape
    xr, tr = x.detach().clone().to(dtype).requires_grad_(True), t.detach().clone().to(dtype).requires_grad_(True)
    gr = go.to(dtype)
    if ei.shape[1] == 0:
        return dict(out=xr.detach().double(), dx=gr.double(), dt=0.0, mag=0.0)
    msg = torch.relu(xr[src]) + eps
    z = msg * tr
    zmax = torch.full((N, C), -float("inf"), dtype=dtype).scatter_reduce(0, dst[:, None].expand(-1, C), z.detach(), reduce="amax", include_self=True)
    e = torch.exp(z - zmax[dst])
    w = e / torch.zeros(N, C, dtype=dtype).index_add_(0, dst, e)[dst]
    agg = torch.zeros(N, C, dtype=dtype).index_add_(0, dst, w * msg)
    out = agg + xr
    (out * gr).sum().backward()
    with torch.no_grad():
        mag = float((gr[dst].abs() * w * msg * (msg + agg[dst])).double().sum())
    return dict(out=out.detach().double(), dx=xr.grad.double(), dt=float(tr.grad), mag=mag)


def errors(got, ref):
    """The three figures the project's bounds are stated in."""
    rel = lambda a, b: float((a.detach().cpu().double() - b).abs().max() / (b.abs().max() + 1e-30))
    return dict(out=rel(got["out"], ref["out"]), dx=rel(got["dx"], ref["dx"]), dt=abs(float(got["dt"]) - ref["dt"]) / (ref["mag"] + 1e-30))


# ------------------------------------------------------------------------------------------------------------------------------
# graphs (all deterministic; GraphCSR sorts stably, so the order of edge_index is the order inside every node's list)
# ------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _by_degree(deg, other, g, shuffle=True):
    """Edges with node i repeated deg[i] times on one side and random nodes on the other; some self loops and repeated edges."""
    N = deg.numel()
    own = torch.repeat_interleave(torch.arange(N), deg)
    oth = torch.randint(0, N, (own.numel(),), generator=g) if other is None else other
    first = torch.zeros(N + 1, dtype=torch.long); first[1:] = torch.cumsum(deg, 0)
    loops = torch.arange(0, N, 5)[deg[0::5] > 0]                  # self loop: the first edge of every fifth node
    oth[first[loops]] = loops
    twice = torch.arange(3, N, 7)[deg[3::7] > 1]                  # repeated edge: the first two edges of every seventh
    oth[first[twice] + 1] = oth[first[twice]]
    if shuffle:
        p = torch.randperm(own.numel(), generator=g)
        own, oth = own[p], oth[p]
    return own, oth


def ladder_degrees(N, ladder, thin):
    i = torch.arange(N)
    deg = torch.tensor(ladder)[i % len(ladder)]
    if thin:                                                      # every third node keeps its rung (period 33, coprime to the tile)
        deg = torch.where(i % 3 == 0, deg, torch.zeros_like(deg))
    return deg


@functools.lru_cache(maxsize=None)
def ladder_in(N, thin=False):
    dst, src = _by_degree(ladder_degrees(N, LADDER_IN, thin), None, _gen(N))
    return torch.stack([src, dst])


@functools.lru_cache(maxsize=None)
def ladder_out(N, thin=False):
    src, dst = _by_degree(ladder_degrees(N, LADDER_OUT, thin), None, _gen(N + 1))
    return torch.stack([src, dst])


@functools.lru_cache(maxsize=None)
def heavy_tiles(N):
    """In-degrees that put three tiles of the forward walk on either side of the staging limit: one of 2080 edges, one of exactly 2048
    and one of 2049 (N = 300, tiles of 8 nodes: 260 / 256 / 256 each, one extra edge into the third); one of 2048 and one of 2049
    (N = 8213, tiles of 16 nodes: 128 each). Every other node has 8 in-edges (N = 300) or its rung of the ladder (N = 8213)."""
    tn = tile_nodes_for(N)
    if N == 300:
        deg = torch.full((N,), 8)
        deg[5 * tn:6 * tn] = 260; deg[10 * tn:11 * tn] = 256; deg[15 * tn:16 * tn] = 256; deg[15 * tn + 3] += 1
    else:
        deg = ladder_degrees(N, LADDER_IN, False)
        deg[10 * tn:11 * tn] = 128; deg[20 * tn:21 * tn] = 128; deg[20 * tn + 9] += 1
    dst, src = _by_degree(deg, None, _gen(N + 2))
    return torch.stack([src, dst])


def mirror(ei):
    """Rows swapped: the by-target image of `ei` is the by-source image of its mirror."""
    return torch.stack([ei[1], ei[0]])


HUB_TILE, HUB_NODE, HUB_EDGES = 5, 43, 60


@functools.lru_cache(maxsize=None)
def hub_pair():
    """(A, B), N = 300: tile 5 (nodes 40 .. 47) holds 8 x 250 = 2000 in-edges in A, all from sources below 200; B is A followed by 60
    more edges into node 43 from sources 200 .. 259, which have no edge into that tile in A. Every node but 43 keeps its in-list."""
    N = 300
    g = _gen(77)
    deg = torch.full((N,), 8); deg[8 * HUB_TILE:8 * HUB_TILE + 8] = 250
    dst, src = _by_degree(deg, None, g)
    into = (dst >= 8 * HUB_TILE) & (dst < 8 * HUB_TILE + 8)
    src[into] = torch.randint(0, 200, (int(into.sum()),), generator=g)
    a = torch.stack([src, dst])
    extra = torch.stack([torch.arange(200, 200 + HUB_EDGES), torch.full((HUB_EDGES,), HUB_NODE)])
    return a, torch.cat([a, extra], 1)


RESCALE_NODE, RESCALE_EDGES = 5, 40


@functools.lru_cache(maxsize=None)
def rescale_graph(order, unstaged):
    """N = 64: node 5 has 40 in-edges (five forward chunks) from sources 10 .. 49, whose messages ascend with the source id, listed
    ascending, descending, or with the largest in the middle chunk. The other nodes of its tile have 8 in-edges each (staged) or 290
    (7 x 290 + 40 = 2070 edges: unstaged); the rest have 8."""
    N = 64
    g = _gen(5)
    deg = torch.full((N,), 8)
    if unstaged:
        deg[:8] = 290
    deg[RESCALE_NODE] = RESCALE_EDGES
    dst, src = _by_degree(deg, None, g, shuffle=False)
    ids = torch.arange(10, 10 + RESCALE_EDGES)
    if order == "descending":
        ids = ids.flip(0)
    elif order == "middle":                                       # the largest message sits in the third of the five chunks
        ids = torch.cat([ids[:16], ids[32:], ids[16:32]])
    src[dst == RESCALE_NODE] = ids
    return torch.stack([src, dst])


def rescale_x(N, C, top):
    """Rows 10 .. 49 rise from 0 to `top` (per channel: times 0.5 .. 1, a few channels negative -> message eps); the rest randn."""
    g = _gen(9)
    x = torch.randn(N, C, generator=g)
    ramp = torch.linspace(0, top, RESCALE_EDGES)[:, None] * (0.5 + 0.5 * torch.rand(C, generator=g))[None, :]
    ramp[:, ::17] = -ramp[:, ::17]
    x[10:10 + RESCALE_EDGES] = ramp
    return x


def block_union(parts):
    """Block-diagonal union, node ids offset (PatchGCN.features_multi)."""
    off, eis = 0, []
    for ei, n in parts:
        eis.append(ei + off); off += n
    return torch.cat(eis, 1), off


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, launches, the body
# ------------------------------------------------------------------------------------------------------------------------------
def inputs(N, C, seed, content="randn", scale=1.0):
    g = _gen(1000 + seed)
    x = torch.randn(N, C, generator=g) * scale
    go = torch.randn(N, C, generator=g)
    if content == "production":          # what FC + ReLU + dropout in front of the op produce: exact zeros; and a block of negative rows
        x = torch.relu(x) * (torch.rand(N, C, generator=g) > 0.25)
        x[N // 3:N // 3 + 64] = -torch.rand(64, C, generator=g) - 0.1
    return x, go


def launch(x, t, ei, go, misalign=False):
    """Forward (grad mode and no-grad mode: the same bits), backward -> dict(out, dx, dt) on the host."""
    from advmil_amd import ops
    N, C = x.shape
    if misalign:                                                  # a contiguous view one float into a larger buffer
        buf = torch.zeros(N * C + 4, device=DEV)
        xd = buf[1:1 + N * C].view(N, C)
        xd.copy_(x)
        assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
        xd.requires_grad_(True)
    else:
        xd = x.clone().to(DEV).requires_grad_(True)
        assert xd.data_ptr() % 16 == 0
    td = t.clone().to(DEV).requires_grad_(True)
    csr = ops.GraphCSR(ei.to(DEV), N)
    out = ops.genconv_aggregate(xd, td, csr)
    with torch.no_grad():
        out_n = ops.genconv_aggregate(xd, td, csr)
    assert torch.equal(out, out_n), "the no-grad forward differs from the grad-mode forward"
    (out * go.to(DEV)).sum().backward()
    return dict(out=out.detach().cpu(), dx=xd.grad.cpu(), dt=td.grad.cpu())


_REFS = {}


def reference(key, x, t, ei, go, e32=False):
    """The float64 restatement of a case, computed once per `key` and left unchanged; with e32, its float32 self's errors too."""
    if key not in _REFS:
        ref = restate(x, t, ei, go)
        ref["e32"] = errors(restate(x, t, ei, go, torch.float32), ref) if e32 else None
        _REFS[key] = ref
    return _REFS[key]


def float64_body(key, x, t, ei, go, unmeasured=(), misalign=False):
    """Launch, compare with float64 at the project's bounds (for the figures in `unmeasured`: max(bound, 4 e32)); -> (got, ref)."""
    key = f"{key}/t{float(t):g}"
    ref = reference(key, x, t, ei, go, e32=bool(unmeasured))
    got = launch(x, t, ei, go, misalign)
    err = errors(got, ref)
    bound = {k: max(BOUND[k], 4 * ref["e32"][k]) if k in unmeasured else BOUND[k] for k in BOUND}
    print(f"{key}: t {float(t):g}: " + " ".join(f"{k} {err[k]:.2e} (bound {bound[k]:.1e})" for k in BOUND)
          + (" e32 " + " ".join(f"{k} {ref['e32'][k]:.2e}" for k in BOUND) if unmeasured else ""))
    for k in BOUND:
        assert err[k] < bound[k], (key, k, err, bound)
    for k in ("out", "dx", "dt"):
        assert bool(torch.isfinite(got[k]).all()), (key, k)
    return got, ref


def named_graph(name):
    """The graphs tests/test_poison_kernels_gpu.py shares with this file: (edge_index, N, host-side precondition)."""
    if name == "ladder_s2":
        N = 8213
        ei = ladder_in(N)
        f, b = facts_of(ei, N)
        assert f.S == 2 and N % 16 == 5 and f.tile_max <= GT_EDGES and b.tile_max <= GT_EDGES
    elif name == "unstaged_forward":
        N = 300
        ei = heavy_tiles(N)
        f, b = facts_of(ei, N)
        assert f.S == 1 and sorted(f.tiles)[-3:] == [2048, 2049, 2080] and b.tile_max <= GT_EDGES and f.deg_max <= 400
    elif name == "unstaged_backward":
        N = 300
        ei = mirror(heavy_tiles(N))
        f, b = facts_of(ei, N)
        assert b.S == 1 and sorted(b.tiles)[-3:] == [2048, 2049, 2080] and f.tile_max <= GT_EDGES and b.deg_max <= 400
    else:
        raise KeyError(name)
    return ei, N


def named_case(name, C=128, t=1.7):
    """float64_body on a named graph at width C (C != 128: the generic kernels, where the graph is just a graph)."""
    ei, N = named_graph(name)
    x, go = inputs(N, C, seed=C)
    return float64_body(f"{name}/C{C}/t{t}", x, torch.tensor([t]), ei, go)


# ------------------------------------------------------------------------------------------------------------------------------
# (a) degree ladders across the pipelined walk
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["in", "out"])
@pytest.mark.parametrize("N,S,last", [(8213, 2, 5), (12301, 3, 13), (65549, 16, 13)])
def test_degree_ladders_across_the_walk(N, S, last, side):
    """Node i takes the in-degree (side = in: the forward's walk) or the out-degree (out: the backward's) LADDER[i % 11]: the period is
    coprime to the tile, so every half-wave slot hands over from, to and across an empty node, and lists end on, one short of and one
    past the chunk; self loops and repeated edges included; the last tile is ragged. At 65549 nodes every third node keeps its rung
    (E <= 4 N). dt at 65549 nodes is outside the regime the 2e-6 bound was measured in: max(2e-6, 4 e32).
    Measured on an MI355X (N = 65549, in / out ladder): dt 4.4e-11 / 4.7e-12 of the uncancelled magnitude (e32: 9e-11 / 3e-11), so the bound in
    force is the project's 2e-6; out 4.0e-7 / 1.3e-7, dx 9.4e-7 / 3.5e-7."""
    thin = N > 60000
    ei = (ladder_in if side == "in" else ladder_out)(N, thin)
    f, b = facts_of(ei, N)
    assert f.S == S == b.S and tile_nodes_for(N) == 8 * S and N % (8 * S) == last
    assert f.tile_max <= GT_EDGES and b.tile_max <= GT_EDGES and max(f.deg_max, b.deg_max) <= 400
    walked = f if side == "in" else b
    ladder, ch = (LADDER_IN, FWD_CH) if side == "in" else (LADDER_OUT, BWD_CH)
    assert walked.deg_max == max(ladder) and {0, ch - 1, ch, ch + 1, 2 * ch} <= set(ladder)
    assert ei.shape[1] <= 4 * N or not thin
    assert int((ei[0] == ei[1]).sum()) > 0                                             # self loops
    x, go = inputs(N, 128, seed=N)
    float64_body(f"ladder_{side}/{N}", x, torch.tensor([1.7]), ei, go, unmeasured=("dt",) if thin else ())


# ------------------------------------------------------------------------------------------------------------------------------
# (b) unstaged tiles and the 2048 / 2049 boundary, forward and backward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unstaged_forward", "unstaged_backward"])
def test_unstaged_tiles_and_the_staging_boundary(name):
    """Tiles of 2080 (indices from global memory), exactly 2048 (the last staged size) and 2049 edges, S = 1; see heavy_tiles()."""
    named_case(name)


@pytest.mark.parametrize("mirrored", [False, True])
def test_staging_boundary_at_sixteen_node_tiles(mirrored):
    """N = 8213 (S = 2): a 16-node tile of exactly 2048 edges and one of 2049, the ladder everywhere else."""
    N = 8213
    ei = mirror(heavy_tiles(N)) if mirrored else heavy_tiles(N)
    f, b = facts_of(ei, N)
    heavy, light = (b, f) if mirrored else (f, b)
    assert heavy.S == 2 and sorted(heavy.tiles)[-2:] == [2048, 2049] and light.tile_max <= GT_EDGES and heavy.deg_max <= 400
    x, go = inputs(N, 128, seed=N + 1)
    float64_body(f"heavy_tiles/{N}/{mirrored}", x, torch.tensor([1.7]), ei, go)


# ------------------------------------------------------------------------------------------------------------------------------
# (c) where the indices come from must not move a bit
# ------------------------------------------------------------------------------------------------------------------------------
def test_index_source_does_not_move_a_bit():
    """hub_pair(): B = A + 60 edges into node 43, which push its tile from 2000 (staged) to 2060 (unstaged) edges. Every other node
    keeps its in-list and its chunk sequence, so its `out` row is the same bits; on the mirrored graphs the same holds for the dx rows
    of the seven bystander sources of the tile (none of their targets gained an in-edge)."""
    a, b = hub_pair()
    N = 300
    fa, _ = facts_of(a, N)
    fb, _ = facts_of(b, N)
    assert fa.S == 1 and fa.tiles[HUB_TILE] == 2000 == fa.tile_max and fb.tiles[HUB_TILE] == 2060 == fb.tile_max and fb.deg_max <= 400
    new_src = set(range(200, 200 + HUB_EDGES))
    into_tile = a[0][(a[1] >= 8 * HUB_TILE) & (a[1] < 8 * HUB_TILE + 8)]
    assert not new_src & set(into_tile.tolist())
    x, go = inputs(N, 128, seed=43)
    t = torch.tensor([1.7])
    ga, _ = float64_body("hub_pair/A", x, t, a, go)
    gb, _ = float64_body("hub_pair/B", x, t, b, go)
    rows = torch.arange(N) != HUB_NODE
    assert torch.equal(ga["out"][rows], gb["out"][rows])
    assert not torch.equal(ga["out"][HUB_NODE], gb["out"][HUB_NODE])
    _, ba = facts_of(mirror(a), N)
    _, bb = facts_of(mirror(b), N)
    assert ba.tiles[HUB_TILE] == 2000 == ba.tile_max and bb.tiles[HUB_TILE] == 2060 == bb.tile_max
    ma, _ = float64_body("hub_pair/mirror A", x, t, mirror(a), go)
    mb, _ = float64_body("hub_pair/mirror B", x, t, mirror(b), go)
    bystanders = [j for j in range(8 * HUB_TILE, 8 * HUB_TILE + 8) if j != HUB_NODE]
    assert torch.equal(ma["dx"][bystanders], mb["dx"][bystanders])
    assert not torch.equal(ma["dx"][HUB_NODE], mb["dx"][HUB_NODE])


# ------------------------------------------------------------------------------------------------------------------------------
# (d) temperature: both signs, zero, nearly zero
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [-1.3, -3.0, 0.0, 1e-3, 3.0])
@pytest.mark.parametrize("name", ["ladder_s2", "unstaged_forward", "unstaged_backward"])
def test_temperature_of_either_sign(name, t):
    """t is a learnable Parameter: t < 0 takes the running minimum (never the unpredicated full-chunk form), t = 0 weighs uniformly.
    The ladder holds lists of 8, 16 and 24 edges, the heavy tiles lists of 256: exact multiples of the chunk.
    Closest to a bound: `out` of the 260-edge lists at t = 3, 3.84e-6 of 4e-6 on an MI355X -- the float32 restatement of the same case is
    3.8e-6 from float64 too (sequential fp32 sums over 260 weights that t = 3 concentrates on a few edges), so that is what fp32 gives."""
    ei, N = named_graph(name)
    deg = torch.bincount(ei[1], minlength=N)
    assert int(((deg > 0) & (deg % FWD_CH == 0)).sum()) > 0 and abs(t) <= 3
    named_case(name, 128, t)


# ------------------------------------------------------------------------------------------------------------------------------
# (e) the online rescale between the chunks of one list
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unstaged", [False, True])
@pytest.mark.parametrize("t", [3.0, -3.0])
@pytest.mark.parametrize("order", ["ascending", "descending", "middle"])
def test_online_rescale_under_large_score_gaps(order, t, unstaged):
    """One node with 40 in-edges = five forward chunks whose messages run from 0 to 30, so |t| m log2 e spans 0 .. 130 inside the list
    and the weights of whole chunks underflow after the rescale. Ascending: the running extreme of t > 0 moves at every chunk (of
    t < 0: never); descending: the reverse; middle: the extreme arrives in the third chunk. Outside the measured regime (score gaps
    beyond 40): every bound is max(project bound, 4 e32).
    Measured on an MI355X, worst over the twelve cases: out 6.2e-7, dx 1.8e-5, dt 2.1e-9 (e32: 5.3e-7 / 1.4e-5 / 2.3e-9; the dx figures are those of
    the unstaged variant at t = 3, whose 290-edge neighbours see the same score gaps: bound 4 e32 = 4.2e-5 .. 5.7e-5 there, 2e-5 elsewhere)."""
    N, C, top = 64, 128, 30.0
    ei = rescale_graph(order, unstaged)
    f, b = facts_of(ei, N)
    assert f.S == 1 and (f.tiles[0] == 2070 if unstaged else f.tile_max <= GT_EDGES) and f.deg_max <= 400
    x = rescale_x(N, C, top)
    lst = ei[0][ei[1] == RESCALE_NODE]
    assert lst.numel() == 5 * FWD_CH
    m = x[lst, 1]                                                                      # channel 1: positive ramp
    chunk_max = m.view(5, FWD_CH).max(1).values
    assert {"ascending": bool((chunk_max[1:] > chunk_max[:-1]).all()), "descending": bool((chunk_max[1:] < chunk_max[:-1]).all()),
            "middle": int(chunk_max.argmax()) == 2}[order]
    assert 120 < abs(t) * float(x[lst].max()) * 1.4427 < 135
    _, go = inputs(N, C, seed=7)
    float64_body(f"rescale/{order}/{unstaged}", x, torch.tensor([t]), ei, go, unmeasured=("out", "dx", "dt"))


# ------------------------------------------------------------------------------------------------------------------------------
# (f) the generic kernels: other widths, and C = 128 off 16-byte alignment
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 64, 96, 130, 256])
def test_generic_widths(C):
    N = 1003
    ei = ladder_in(N)
    f, b = facts_of(ei, N)
    assert C != 128 and f.deg_max == max(LADDER_IN)
    x, go = inputs(N, C, seed=C)
    float64_body(f"generic/{C}", x, torch.tensor([1.7]), ei, go)


def test_misaligned_rows_fall_back_to_the_generic_kernels():
    """C = 128 with x a contiguous view one float into a larger buffer: 4 bytes off 16-byte alignment, so the float4 kernels must not
    take it (launch() asserts the address). Against float64, and within the same bounds of the aligned run."""
    N = 1003
    ei = ladder_in(N)
    x, go = inputs(N, 128, seed=128)
    t = torch.tensor([1.7])
    mis, ref = float64_body("misaligned", x, t, ei, go, misalign=True)
    ali, _ = float64_body("misaligned", x, t, ei, go)
    mis["dt"], ali["dt"] = float(mis["dt"]), float(ali["dt"])
    err = errors(mis, dict(out=ali["out"].double(), dx=ali["dx"].double(), dt=ali["dt"], mag=ref["mag"]))
    print("misaligned against aligned:", err)
    for k in BOUND:
        assert err[k] < BOUND[k], (k, err)


# ------------------------------------------------------------------------------------------------------------------------------
# (g) production-like content
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 96])
def test_production_like_content(C):
    """x = relu(randn) * keep-mask (exact zeros) with a block of 64 all-negative rows, on the S = 2 ladder; targets 5000 .. 5049 draw
    every source from that block: every message is eps, the weights are uniform, agg = eps. Where x <= 0, dx is dout bit for bit."""
    ei, N = named_graph("ladder_s2")
    ei = ei.clone()
    blk = N // 3
    sel = (ei[1] >= 5000) & (ei[1] < 5050)
    ei[0][sel] = blk + torch.arange(int(sel.sum())) % 64
    x, go = inputs(N, C, seed=C, content="production")
    assert int((x == 0).sum()) > N * C // 4 and bool((x[blk:blk + 64] < 0).all()) and int(sel.sum()) > 100
    got, ref = float64_body(f"production/{C}", x, torch.tensor([1.7]), ei, go)
    off = x <= 0
    assert torch.equal(got["dx"][off], go[off])
    fed = torch.bincount(ei[1][sel], minlength=N) > 0
    assert float((got["out"][fed] - x[fed] - 1e-7).abs().max()) <= 2.0 ** -23 * float(x[fed].abs().max())     # agg = eps to the rounding of out


# ------------------------------------------------------------------------------------------------------------------------------
# (h) invariances
# ------------------------------------------------------------------------------------------------------------------------------
def test_block_diagonal_union_equals_its_parts():
    """Three graphs (4001-node in-ladder, the 300-node heavy tiles, 3907-node out-ladder) and their block-diagonal union of 8208 nodes:
    the parts walk at S = 1, the union at S = 2 with every tile boundary moved; out and dx rows are the same bits, dt of the union is
    within the dt bound of the sum of the parts, and two identical backward calls give the same dt bits."""
    from advmil_amd import ops
    parts = [(ladder_in(4001), 4001), (heavy_tiles(300), 300), (ladder_out(3907), 3907)]
    ei, N = block_union(parts)
    f, b = facts_of(ei, N)
    assert N >= 2 * TILE_DIV and f.S == 2 and f.tile_max > GT_EDGES
    for e, n in parts:
        assert facts_of(e, n)[0].S == 1
    x, go = inputs(N, 128, seed=N)
    t = torch.tensor([1.7])
    whole, _ = float64_body("union", x, t, ei, go)
    off, dt, mag = 0, 0.0, 0.0
    for k, (e, n) in enumerate(parts):
        got, ref = float64_body(f"union/part{k}", x[off:off + n], t, e, go[off:off + n])
        assert torch.equal(got["out"], whole["out"][off:off + n]) and torch.equal(got["dx"], whole["dx"][off:off + n]), k
        dt += float(got["dt"]); mag += ref["mag"]
        off += n
    print(f"union dt {float(whole['dt'])!r}, parts {dt!r}, magnitude {mag:.3e}")
    assert abs(float(whole["dt"]) - dt) < BOUND["dt"] * mag
    again = launch(x, t, ei, go)
    assert torch.equal(again["dt"], whole["dt"]) and torch.equal(again["dx"], whole["dx"])
