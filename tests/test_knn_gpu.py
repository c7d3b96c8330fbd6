"""GPU: the exact k-NN graph construction (csrc/knn.hip, advmil_amd/wsigraph.py) against the int64 / float64 oracle tests/knn_ref.py.

Walks (the constants below mirror csrc/knn.hip). `walks(lens, C)` restates on the host where a slab puts the
kernels, and every case ASSERTS before it launches that it lands on the walks it is aimed at:

  spatial  one thread per query, workgroups of SP_T = 256 consecutive slab rows, the keys of [first query's bag start, last query's
           bag end) streamed through LDS in chunks of SP_CH = 1024 coordinates:
             sp_q_short   the last query group is short of 256 rows           sp_chunks    a workgroup streams more than one chunk
             sp_k_short   a workgroup's last chunk is short                   sp_bag_mid   a bag starts in the middle of a query group
             sp_bag_small a bag lies inside one query group with others       (every lane walks only its own bag's part of a chunk)
  latent   workgroups of TQ = 128 query rows (32 per wave), key tiles of TK = 128 rows aligned to the slab, feature chunks of BK = 32:
             lt_q_short   the last query tile is short                        lt_k_short   the last key tile reaches past the slab
             lt_bag_mid   a bag starts in the middle of a tile                lt_bag_small a bag smaller than one tile
             lt_k_tiles   a bag spans several key tiles                       lt_c_min / lt_c_1024: the K loop at 1 and at 32 chunks

Exact cases (ids AND dist2 EQUAL the oracle): spatial is int64 on any input. Latent features are small integers: drawn from [-7, 7]
every product and partial sum is an integer below 2^24 (n <= 50 176 at C = 1024, d2 <= 200 704), so fp32 is exact in any order and the
bf16 hi plane holds the value (lo = 0) -- the argument of tests/gemm_ref.py. Every exact case runs four times through tests/poison.py
(plain, plain again, outputs / planes / workspace pre-filled with 0xFF and with 0x7F) and must give the same bits each time.

Real-valued cases: per pair delta_ij = 2e-5 (n_i + n_j), the project's contraction parity contract (README, bf16x3 row), not a figure
of this kernel. (a) every row and rank: |dist2 - d64(i, nbr)| <= delta, |d64(i, nbr) - d64(i, oracle)| <= the two pairs' deltas
summed (2 delta), distances non-decreasing, no duplicate, no self, no -1; (b) on rows whose oracle gaps between consecutive ranks
1 .. k+1 all exceed the two deltas summed the ids EQUAL the oracle's; the rows (b) leaves out are asserted <= 20 %. Measured on an
MI355X when this file was written: see `test_latent_real_valued`."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import knn_ref as R
from tests import poison as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SP_T, SP_CH = 256, 1024                  # KNN_THREADS, KNN_SP_CHUNK
TQ, TK, BK = 128, 128, 32                # KNN_TQ, KNN_TK, KNN_BK
SLAB = [17, 200, 9, 1031]                # k = 8: a bag of exactly k + 1, bags inside one tile, a bag over nine key tiles / two chunks


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import ops as _ops
    from advmil_amd import _lib
    _lib.lib()
    return _ops


def walks(lens, C=None):
    N, offs = sum(lens), np.concatenate([[0], np.cumsum(lens)])
    bag_of = lambda i: int(np.searchsorted(offs, i, side="right") - 1)     # noqa: E731
    w = set()
    for T, pre in ((SP_T, "sp"), (TQ, "lt")):
        if N % T:
            w.add(pre + "_q_short")
        if any(o % T for o in offs[1:-1]):
            w.add(pre + "_bag_mid")
        if any(n < T for n in lens):
            w.add(pre + "_bag_small")
        for q0 in range(0, N, T):
            kb, ke = offs[bag_of(q0)], offs[bag_of(min(q0 + T, N) - 1) + 1]
            if pre == "sp":
                if ke - kb > SP_CH:
                    w.add("sp_chunks")
                if (ke - kb) % SP_CH:
                    w.add("sp_k_short")
            else:
                kt0 = kb // TK * TK
                if -(-(ke - kt0) // TK) > 1:
                    w.add("lt_k_tiles")
                if kt0 + -(-(ke - kt0) // TK) * TK > N:
                    w.add("lt_k_short")
    if C is not None:
        Cp = -(-C // BK) * BK
        if Cp // BK == 1:
            w.add("lt_c_min")
        if Cp // BK == 32:
            w.add("lt_c_1024")
    return w


def seg_of(ops, lens):
    return None if lens is None else ops.Segments(lens, DEV)


def four_runs(fn):
    """plain, plain again, poisoned 0xFF, poisoned 0x7F: the same bits (determinism and independence of what the buffers held)."""
    trees = P.three_runs(fn)
    P.assert_same_bits(trees)
    return [t.cpu().numpy() for t in trees[0]]


def check_spatial(ops, xy, k, lens=None):
    o = R.knn(xy, k, lens)
    t = torch.from_numpy(np.ascontiguousarray(xy)).to(DEV)
    nbr, d2 = four_runs(lambda: ops.knn_spatial(t, k, seg_of(ops, lens), return_dist=True))
    assert nbr.dtype == np.int32 and d2.dtype == np.int64
    assert np.array_equal(nbr, o["nbr"]) and np.array_equal(d2, o["dist2"])
    return nbr


def check_latent_exact(ops, x, k, lens=None):
    o = R.knn(x, k, lens, latent=True)
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    nbr, d2 = four_runs(lambda: ops.knn_latent(t, k, seg_of(ops, lens), return_dist=True))
    assert nbr.dtype == np.int32 and d2.dtype == np.float32
    assert np.array_equal(nbr, o["nbr"]), int((nbr != o["nbr"]).sum())
    assert np.array_equal(d2.astype(np.float64), o["dist2"])
    return nbr


def assert_bag_local(nbr, lens, k):
    offs = np.concatenate([[0], np.cumsum(lens)])
    for b, n in enumerate(lens):
        rows = nbr[offs[b]:offs[b + 1]]
        assert rows.min() >= 0 and rows.max() < n, (b, int(rows.min()), int(rows.max()))
        assert (rows != np.arange(n)[:, None]).all()
        if n == k + 1:                                   # a bag of exactly k + 1: every row lists all the others
            assert (np.sort(rows, axis=1) == np.array([[j for j in range(n) if j != i] for i in range(n)])).all()


# ------------------------------------------------------------------------------------------------------------------------------
# spatial: exact on any input
# ------------------------------------------------------------------------------------------------------------------------------
def grid_xy(rows, cols, step, seed):
    xy = np.array([[c * step, r * step] for r in range(rows) for c in range(cols)], dtype=np.int64)
    return xy[np.random.default_rng(seed).permutation(len(xy))]


@pytest.mark.parametrize("k", [1, 8, 16])
def test_spatial_exact(ops, k):
    rng = np.random.default_rng(100 + k)
    assert "sp_q_short" in walks([35]) and "sp_chunks" not in walks([35])
    check_spatial(ops, grid_xy(5, 7, 256, 3), k)                                         # full of ties
    lim = (1 << 30) - 1
    far = rng.integers(-lim, lim + 1, size=(300, 2), dtype=np.int64)                     # the int64 range: d2 up to 2^63 - 2^33
    far[:4] = [[lim, lim], [-lim, -lim], [lim, -lim], [-lim, lim]]
    assert {"sp_q_short"} <= walks([300])
    assert int(R.dist2_spatial(far).max()) > 1 << 62                                      # candidates near 2^63 pass through the compare
    check_spatial(ops, far, k)
    assert k < 16 or int(R.knn(far[:18], k)["dist2"].max()) >= 1 << 62                    # ... and, with 17 candidates for 16 slots, are returned
    check_spatial(ops, far[:18], k)
    dup = rng.integers(0, 6, size=(90, 2), dtype=np.int64) * 512                         # 36 sites for 90 points: duplicates at distance 0
    assert (R.knn(dup, 1)["dist2"] == 0).mean() > 0.5
    check_spatial(ops, dup, k)
    check_spatial(ops, dup.astype(np.float32), k)                                        # integer-valued float coordinates (`centroid`)


def test_spatial_slab(ops):
    k = 8
    assert {"sp_q_short", "sp_chunks", "sp_k_short", "sp_bag_mid", "sp_bag_small"} <= walks(SLAB)
    rng = np.random.default_rng(7)
    xy = rng.integers(0, 40, size=(sum(SLAB), 2), dtype=np.int64) * 224                   # 1600 sites: ties and duplicates in the long bag
    nbr = check_spatial(ops, xy.astype(np.int32), k, SLAB)
    assert_bag_local(nbr, SLAB, k)
    full = [1024, 1024]                                                                   # whole groups and whole chunks: the unmasked walk
    assert not {"sp_q_short", "sp_k_short", "sp_bag_mid"} & walks(full)
    check_spatial(ops, rng.integers(-5000, 5000, size=(sum(full), 2), dtype=np.int64), k, full)


# ------------------------------------------------------------------------------------------------------------------------------
# latent: exact on small integers
# ------------------------------------------------------------------------------------------------------------------------------
def int_feats(N, C, seed, lim=7):
    return np.random.default_rng(seed).integers(-lim, lim + 1, size=(N, C)).astype(np.float32)


@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("N,C,want", [(9, 32, {"lt_q_short", "lt_k_short", "lt_bag_small", "lt_c_min"}),
                                      (200, 1024, {"lt_q_short", "lt_k_short", "lt_k_tiles", "lt_c_1024"}),
                                      (1031, 64, {"lt_q_short", "lt_k_short", "lt_k_tiles"})])
def test_latent_exact_on_small_integers(ops, N, C, want, k):
    if N <= k:
        with pytest.raises(ValueError, match="bag 0 has 9 rows"):                       # (9, 32) at k = 16: refused before any launch
            ops.knn_latent(torch.zeros(N, C, device=DEV), k)
        return
    assert want <= walks([N], C)
    check_latent_exact(ops, int_feats(N, C, 11 * N + k), k)


def test_latent_exact_slab_and_whole_tiles(ops):
    k = 8
    assert {"lt_q_short", "lt_k_short", "lt_bag_mid", "lt_bag_small", "lt_k_tiles"} <= walks(SLAB, 64)
    nbr = check_latent_exact(ops, int_feats(sum(SLAB), 64, 5), k, SLAB)
    assert_bag_local(nbr, SLAB, k)
    full = [256, 128]
    assert not {"lt_q_short", "lt_k_short", "lt_bag_mid"} & walks(full, 32)
    check_latent_exact(ops, int_feats(sum(full), 32, 6), k, full)
    check_latent_exact(ops, int_feats(150, 40, 8), 4)                                    # C = 40: zero-padded to 64 by the wrapper


def test_latent_tie_rule_inside_the_mfma_kernel(ops):
    """Features from [-2, 2] at C = 32: distances are small integers, nearly every row has ties inside its first k + 1 -- the (distance,
    id) order is decided by the tie rule alone, across register slots, lane halves and key tiles."""
    x = int_feats(700, 32, 9, lim=2)
    for k in (1, 8, 16):
        o = R.knn(x, k, latent=True, extra=1)
        tied = (np.diff(o["more_dist2"], axis=1) == 0).any(axis=1).mean()
        assert k == 1 or tied > 0.9, tied
        check_latent_exact(ops, x, k)
    x[300:340] = x[17]                                                                   # 41 copies of one row: duplicates at distance 0, self by index
    check_latent_exact(ops, x, 8)


# ------------------------------------------------------------------------------------------------------------------------------
# latent: real-valued features
# ------------------------------------------------------------------------------------------------------------------------------
REAL = {"520x1024": (520, 1024, None, 1, None), "333x64": (333, 64, None, 2, None), "slab_x30": (520, 64, [150, 200, 170], 3, 1)}
MEASURED = {}


@pytest.mark.parametrize("name", list(REAL))
def test_latent_real_valued(ops, name):
    """fp32 N(0, 1) features (one bag of the slab scaled by 30). Rows (b) leaves out, from the oracle alone (numpy, these seeds):
    520x1024 12.3 %, 333x64 1.2 %, slab_x30 3.1 % (cap 20 %). Largest |dist2 - d64| / (n_i + n_j) over every returned pair, measured
    on an MI355X when this file was written: 520x1024 9.0e-7, 333x64 3.8e-6, slab_x30 4.0e-6 (bound 2e-5)."""
    N, C, lens, seed, scaled = REAL[name]
    k = 8
    x = np.random.default_rng(seed).standard_normal((N, C)).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(lens or [N])])
    if scaled is not None:
        x[offs[scaled]:offs[scaled + 1]] *= 30.0
    o = R.knn(x, k, lens, latent=True, extra=1)
    t = torch.from_numpy(x).to(DEV)
    nbr, d2 = [v.cpu().numpy() for v in ops.knn_latent(t, k, seg_of(ops, lens), return_dist=True)]
    again = ops.knn_latent(t, k, seg_of(ops, lens), return_dist=True)
    assert np.array_equal(again[0].cpu().numpy(), nbr) and np.array_equal(again[1].cpu().numpy().view(np.int32), d2.view(np.int32))
    worst, left_out = 0.0, 0
    for b in range(len(offs) - 1):
        lo, hi = offs[b], offs[b + 1]
        D = o["D"][b]
        n = (x[lo:hi].astype(np.float64) ** 2).sum(axis=1)
        got, gd = nbr[lo:hi].astype(np.int64), d2[lo:hi].astype(np.float64)
        want, more_d = o["more_nbr"][lo:hi, :k], o["more_dist2"][lo:hi]
        rows = np.arange(hi - lo)[:, None]
        assert got.min() >= 0 and got.max() < hi - lo and (got != rows).all()                         # no -1, no self, bag-local
        assert (np.sort(got, axis=1)[:, 1:] != np.sort(got, axis=1)[:, :-1]).all()                    # no duplicate
        assert (np.diff(d2[lo:hi], axis=1) >= 0).all()                                               # non-decreasing as returned
        d_got, d_want = D[rows, got], D[rows, want]
        del_got, del_want = 2e-5 * (n[:, None] + n[got]), 2e-5 * (n[:, None] + n[want])
        err = np.abs(gd - d_got)
        worst = max(worst, float((err / (n[:, None] + n[got])).max()))
        assert (err <= del_got).all(), float((err / del_got).max())
        assert (np.abs(d_got - d_want) <= del_got + del_want).all()
        more_n = o["more_nbr"][lo:hi]
        del_more = 2e-5 * (n[:, None] + n[more_n])
        clear = (np.diff(more_d, axis=1) > del_more[:, 1:] + del_more[:, :-1]).all(axis=1)            # gaps of ranks 1 .. k+1
        assert np.array_equal(got[clear], want[clear]), int((got[clear] != want[clear]).any(axis=1).sum())
        left_out += int((~clear).sum())
    MEASURED[name] = (worst, left_out / N)
    print(f"knn_latent real-valued {name}: max |dist2 - d64| / (n_i + n_j) = {worst:.3e}, rows left out of (b) = {100.0 * left_out / N:.1f} %")
    assert left_out <= 0.20 * N, left_out / N


# ------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------
def slide(N, C, seed):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(N)))
    cells = rng.permutation(side * side)[:N]
    coords = np.stack([cells % side, cells // side], axis=1).astype(np.float32) * 256.0          # the reference stores `centroid` as float
    return int_feats(N, C, seed + 1), coords


def oracle_graph(x, coords, k):
    from advmil_amd.wsigraph import edges_from_neighbours
    E = lambda o: edges_from_neighbours(torch.from_numpy(o["nbr"])).to(DEV)      # noqa: E731
    return SimpleNamespace(x=torch.from_numpy(x).to(DEV), edge_index=E(R.knn(coords.astype(np.int64), k)), edge_latent=E(R.knn(x, k, latent=True)))


@pytest.mark.parametrize("edge_agg", ["spatial", "latent"])
def test_patchgcn_on_built_graph_equals_oracle_graph(ops, edge_agg):
    from advmil_amd import synth, wsigraph
    from advmil_amd.model.backbone import PatchGCN
    x, coords = slide(300, 64, 21)
    built = wsigraph.build_graph(torch.from_numpy(x).to(DEV), torch.from_numpy(coords).to(DEV), k=8)
    ref = oracle_graph(x, coords, 8)
    assert torch.equal(built.edge_index, ref.edge_index) and torch.equal(built.edge_latent, ref.edge_latent)
    assert built.edge_index.dtype == torch.int64 and tuple(built.edge_index.shape) == (2, 8 * 300) and built.centroid.shape == (300, 2)
    outs = []
    for g in (built, ref):
        bb = PatchGCN([64, 32, 32], num_layers=2, edge_agg=edge_agg)
        bb.load_state_dict({k_: H.T(synth.param(H.PARAM_SEED, "knn-gcn:" + k_, tuple(v.shape))) for k_, v in bb.state_dict().items()})
        bb = bb.to(DEV).eval()
        out = bb(g)
        out.sum().backward()
        outs.append({"H": out.detach(), **{n: p.grad for n, p in bb.named_parameters() if p.grad is not None}})
    assert set(outs[0]) == set(outs[1]) and len(outs[0]) >= 20, sorted(outs[0])           # (layers.0.norm is never used: no gradient)
    P.assert_finite(outs[0])
    P.assert_same_bits(outs, names=("built graph", "oracle graph"))


def test_build_graphs_and_merge_equal_per_slide_builds(ops):
    from advmil_amd import wsigraph
    slides = [slide(n, 64, 30 + i) for i, n in enumerate((100, 257, 40))]
    feats = [torch.from_numpy(s[0]).to(DEV) for s in slides]
    coords = [torch.from_numpy(s[1]).to(DEV) for s in slides]
    assert {"lt_bag_mid", "lt_bag_small", "lt_k_tiles"} <= walks([100, 257, 40], 64)
    one = [wsigraph.build_graph(f, c) for f, c in zip(feats, coords)]
    many = wsigraph.build_graphs(feats, coords)
    for a, b, s in zip(one, many, slides):
        assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_latent, b.edge_latent) and torch.equal(a.x, b.x)
        assert torch.equal(a.edge_index, oracle_graph(s[0], s[1], 8).edge_index)
    m1, m2 = wsigraph.merge_graphs(one), wsigraph.merge_graphs(many)
    for name in ("x", "edge_index", "edge_latent", "centroid"):
        assert torch.equal(getattr(m1, name), getattr(m2, name)), name
    assert m2.x.shape == (397, 64) and m2.edge_latent.shape == (2, 8 * 397)
    assert int(m2.edge_index[1, 8 * 100:8 * 357].min()) >= 100 and int(m2.edge_index[1, 8 * 100:8 * 357].max()) < 357
    no_lat = wsigraph.build_graphs(feats, coords, latent=False)
    assert no_lat[0].edge_latent is None and wsigraph.merge_graphs(no_lat).edge_latent is None


def test_handler_step_on_built_graphs(ops):
    """One MyHandler step with bcb_mode graph, fed by build_graphs (two bags of 256 nodes): finite losses."""
    from advmil_amd import wsigraph
    from advmil_amd.config import default_cfg
    from advmil_amd.model import MyHandler
    prev = ops.get_gemm_mode()
    try:
        h = MyHandler(default_cfg(bcb_mode="graph", bcb_dims="1024-128-128", gen_dims="128-1", bp_every_batch=2), device=DEV)
        feats = [H.bag(500 + i, 256, DEV)[0].contiguous() for i in range(2)]
        coords = [torch.from_numpy(grid_xy(16, 16, 256, 40 + i)).to(DEV) for i in range(2)]
        graphs = wsigraph.build_graphs(feats, coords)
        loader = [(torch.tensor([[i]], dtype=torch.int), [g.x.unsqueeze(0), g], H.label(500 + i)) for i, g in enumerate(graphs)]
        h._train_each_epoch(loader, "train")
        logs = h.pop_logs()
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(prev)
    vals = [float(v) for d in logs for k_, v in d.items() if k_.split("/")[-1].startswith(("Loss", "D_"))]
    assert len(vals) >= 4 and all(np.isfinite(v) for v in vals), logs
