"""GPU: the batched k-means (csrc/kmeans.hip, advmil_amd/ops.py kmeans_*, advmil_amd/wsicluster.py) against the float64 oracle
tests/kmeans_ref.py and the recorded sklearn runs tests/golden/kmeans_v1.npz.

Walks (the constants below mirror csrc/kmeans.hip). `walks(lens, C, K)` restates on the host where a slab puts the
kernels, and every case ASSERTS before it launches that it lands on the walks it is aimed at:

  assign   workgroups of TR = 32 consecutive slab rows (the 32 columns of one MFMA tile), four waves that share the chunks of CH = 64
           feature columns round-robin; the centre slot of accumulator register e in lane half h is (e & 3) + 8 (e >> 2) + 4 h:
             as_q_short    the last row tile is short                 as_bag_mid   a bag starts inside a tile (the tile walks two bags)
             as_bag_small  a bag smaller than a tile                   as_bag_k     a bag of exactly K rows
             as_c_min      one 32-column unit (C = 32): one wave works  as_c_1024    32 units, four chunks per wave
             as_c_pad      C zero-padded by the wrapper                 as_c_half    C % 64 == 32: the last chunk holds 32 columns
             as_k_1        one centre (lane half 0, register 0)         as_k_half    K > 4: both lane halves hold live slots
             as_k_groups   K % 8 == 0: whole register groups            as_k_edge    K % 8 == 1, K > 1: one slot past a group edge
             as_k_32       every slot live
  update   grid (chunk of UR = 128 rows counted from the BAG's first row, column tile of UC = 256, bag), rows in load groups of UG = 8:
             up_chunk_short  a bag's last chunk is short               up_chunks    several chunks per bag
             up_row_tail     a chunk's row count is no multiple of UG   up_col_short a column tile reaches past C
             up_col_tiles    several column tiles
           (an empty cluster and a bag with every row in one cluster are properties of the labels: asserted where they are made)
  both     an inactive bag between two active ones (`active`): asserted where the mask is made.

Exact cases: features and centres are integers in [-7, 7], so every product and partial sum is an integer below 2^24 (dist2 <= 200 704
at C = 1024) and the bf16 hi plane holds the value (lo = 0) -- the argument of tests/gemm_ref.py: labels, dist2 and count EQUAL the
oracle, cent_new EQUALS np.float32(np.float64(sum) / count). Every exact case runs four times through tests/poison.py (plain, plain
again, every fresh allocation pre-filled with 0xFF and with 0x7F) and must give the same bits each time.

Real-valued cases: per (row, centre) delta_ij = 2e-5 (n_i + c_j), the project's contraction parity contract (README, bf16x3 row), not a
figure of this kernel. Measured figures: in the docstrings of the tests and in DESIGN.md section 7f."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import kmeans_cases as CASES
from tests import kmeans_ref as R
from tests import poison as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TR, CH = 32, 64                          # KM_TR, KM_CH
UR, UC, UG = 128, 256, 8                 # KM_UR, KM_UC, KM_UG
SLAB = [8, 200, 33, 1031]                # K = 8: a bag of exactly K rows, bags inside / across tiles, a bag over nine update chunks
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import ops as _ops
    from advmil_amd import _lib
    _lib.lib()
    return _ops


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "kmeans_v1.npz"))


def walks(lens, C, K):
    N, offs = sum(lens), np.concatenate([[0], np.cumsum(lens)])
    Cp = -(-C // 32) * 32
    w = set()
    if N % TR:
        w.add("as_q_short")
    if any(o % TR for o in offs[1:-1]):
        w.add("as_bag_mid")
    if any(n < TR for n in lens):
        w.add("as_bag_small")
    if any(n == K for n in lens):
        w.add("as_bag_k")
    if Cp // 32 == 1:
        w.add("as_c_min")
    if Cp // 32 == 32:
        w.add("as_c_1024")
    if C != Cp:
        w.add("as_c_pad")
    if Cp % CH:
        w.add("as_c_half")
    if K == 1:
        w.add("as_k_1")
    if K > 4:
        w.add("as_k_half")
    if K % 8 == 0:
        w.add("as_k_groups")
    if K % 8 == 1 and K > 1:
        w.add("as_k_edge")
    if K == 32:
        w.add("as_k_32")
    if any(n % UR for n in lens):
        w.add("up_chunk_short")
    if any(n > UR for n in lens):
        w.add("up_chunks")
    if any((n % UR) % UG for n in lens):
        w.add("up_row_tail")
    if Cp % UC:
        w.add("up_col_short")
    if Cp > UC:
        w.add("up_col_tiles")
    return w


def seg_of(ops, lens):
    return None if lens is None or len(lens) == 1 else ops.Segments(lens, DEV)


def bounds(lens):
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [(int(offs[b]), int(offs[b + 1])) for b in range(len(lens))]


def four_runs(fn):
    trees = P.three_runs(fn)
    P.assert_same_bits(trees)
    return [t.cpu().numpy() for t in trees[0]]


def fill_byte():
    """What an `empty` block handed to a launch holds in this run: the poison byte, or a sentinel in the plain runs."""
    return P.active() if P.active() is not None else SENTINEL


def filled(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(fill_byte())
    return t


def is_fill(t):
    return bool((t.contiguous().view(torch.uint8) == fill_byte()).all())


def int_feats(N, C, seed, lim=7):
    return np.random.default_rng(seed).integers(-lim, lim + 1, size=(N, C)).astype(np.float32)


def oracle_assign(x, cent, lens):
    lab, d2 = [], []
    for b, (lo, hi) in enumerate(bounds(lens)):
        l, d, _ = R.assign(x[lo:hi], cent[b])
        lab.append(l), d2.append(d)
    return np.concatenate(lab), np.concatenate(d2)


# ------------------------------------------------------------------------------------------------------------------------------
# assign: exact on small integers
# ------------------------------------------------------------------------------------------------------------------------------
def check_assign_exact(ops, x, cent, lens, active=None):
    """cent [nseg, K, C]. Labels and dist2 start as a fill pattern, so rows of an inactive bag must still hold it afterwards."""
    N = x.shape[0]
    want_l, want_d = oracle_assign(x, cent, lens)
    tx, tc = H.T(x, DEV), H.T(cent, DEV)
    act = None if active is None else torch.tensor(active, dtype=torch.int32, device=DEV)
    on = np.ones(N, dtype=bool)
    for b, (lo, hi) in enumerate(bounds(lens)):
        on[lo:hi] = active is None or bool(active[b])
    on_t = torch.from_numpy(on).to(DEV)

    def run():
        lab, d2 = filled((N,), torch.int32), filled((N,), torch.float32)
        got = ops.kmeans_assign(tx, tc if len(lens) > 1 else tc[0], seg_of(ops, lens), act, lab, return_dist=d2, return_changed=True)
        assert got[0] is lab and got[1] is d2
        assert is_fill(lab[~on_t]) and is_fill(d2[~on_t])                  # an inactive bag's rows keep their bits (the poison, under poison)
        return lab[on_t], d2[on_t], got[2]

    lab, d2, chg = four_runs(run)
    assert lab.dtype == np.int32 and d2.dtype == np.float32 and chg.dtype == np.int32
    assert np.array_equal(lab, want_l[on]), int((lab != want_l[on]).sum())
    assert np.array_equal(d2.astype(np.float64), want_d[on])
    assert chg.tolist() == [n if (active is None or active[b]) else 0 for b, n in enumerate(lens)]     # the fill pattern is no label
    return want_l


@pytest.mark.parametrize("K", [1, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("N,C,want", [(9, 32, {"as_q_short", "as_bag_small", "as_c_min", "as_c_half"}),
                                      (200, 1024, {"as_q_short", "as_c_1024"}),
                                      (1031, 64, {"as_q_short"}),
                                      (300, 50, {"as_q_short", "as_c_pad"})])
def test_assign_exact_on_small_integers(ops, N, C, want, K):
    got = walks([N], C, K)
    assert want <= got
    assert {1: "as_k_1", 8: "as_k_groups", 9: "as_k_edge", 16: "as_k_groups", 17: "as_k_edge", 32: "as_k_32"}[K] in got
    assert ("as_k_half" in got) == (K > 4) and ("as_bag_k" in got) == (N == K)
    lab = check_assign_exact(ops, int_feats(N, C, 11 * N + K), int_feats(K, C, 13 * N + K)[None], [N])
    assert N != 1031 or len(np.unique(lab)) == K                              # at 1031 rows every slot wins somewhere: no live slot is dead


def test_assign_exact_k32_at_300x32(ops):
    assert {"as_k_32", "as_c_min", "as_q_short"} <= walks([300], 32, 32)
    lab = check_assign_exact(ops, int_feats(300, 32, 5), int_feats(32, 32, 6)[None], [300])
    assert len(np.unique(lab)) == 32


def test_assign_tie_rule_inside_the_mfma_kernel(ops):
    """Features from [-2, 2] at C = 32 and K = 16 centres that repeat with period 4: every row's best distance is shared by the slots
    j, j + 4, j + 8, j + 12 -- the other lane half and the other register groups --, so the label is decided by the tie rule alone and
    must be below 4. K = 9 with centre 8 = centre 0: the tie crosses the register-group edge."""
    x = int_feats(700, 32, 9, lim=2)
    base = int_feats(4, 32, 10, lim=2)
    cent = np.concatenate([base] * 4)[None]
    D = R.dist2(x, cent[0])
    assert ((D == D.min(axis=1, keepdims=True)).sum(axis=1) >= 4).all()
    lab = check_assign_exact(ops, x, cent, [700])
    assert lab.max() < 4 and len(np.unique(lab)) == 4
    c9 = int_feats(9, 32, 12, lim=2)
    c9[8] = c9[0]
    lab = check_assign_exact(ops, x, c9[None], [700])
    assert (lab != 8).all() and (lab == 0).any()
    rows = x[:16].copy()                                                       # centres that ARE rows: distance 0, and duplicates of a row
    x[300:340] = x[3]
    lab = check_assign_exact(ops, x, rows[None], [700])
    assert (lab[300:340] == 3).all()


def test_assign_exact_slab_and_inactive_bag(ops):
    K, C = 8, 64
    assert {"as_q_short", "as_bag_mid", "as_bag_small", "as_bag_k", "as_k_groups", "up_chunks"} <= walks(SLAB, C, K)
    x = int_feats(sum(SLAB), C, 5)
    cent = int_feats(len(SLAB) * K, C, 6).reshape(len(SLAB), K, C)
    check_assign_exact(ops, x, cent, SLAB)
    check_assign_exact(ops, x, cent, SLAB, active=[1, 0, 1, 1])               # an inactive bag between two active ones
    check_assign_exact(ops, x, cent, SLAB, active=[0, 1, 0, 0])
    full = [64, 32]                                                            # whole tiles, bags on tile edges: the unmasked walk
    assert not {"as_q_short", "as_bag_mid", "as_bag_small"} & walks(full, 32, K)
    check_assign_exact(ops, int_feats(96, 32, 7), int_feats(2 * K, 32, 8).reshape(2, K, 32), full)


def test_changed_counts_the_rows_whose_label_moved(ops):
    K, C = 8, 64
    x, cent = int_feats(sum(SLAB), C, 5), int_feats(len(SLAB) * K, C, 6).reshape(len(SLAB), K, C)
    tx, tc, seg = H.T(x, DEV), H.T(cent, DEV), seg_of(ops, SLAB)
    lab, chg, ws = ops.kmeans_assign(tx, tc, seg, return_changed=True)         # no labels given: they start as -1, every row moves
    assert chg.tolist() == SLAB
    lab2, chg2, ws2 = ops.kmeans_assign(tx, tc, seg, None, lab, return_changed=True, norms=ws)
    assert lab2 is lab and ws2 is ws and chg2.tolist() == [0, 0, 0, 0]
    keep = lab.clone()
    lo = bounds(SLAB)[3][0]
    lab[lo + 5:lo + 10] = (lab[lo + 5:lo + 10] + 1) % K
    lab[3] = 31
    act = torch.tensor([1, 1, 1, 0], dtype=torch.int32, device=DEV)
    _, chg3, _ = ops.kmeans_assign(tx, tc, seg, act, lab, return_changed=True, norms=ws)
    assert chg3.tolist() == [1, 0, 0, 0] and not torch.equal(lab, keep)        # the inactive bag's moved labels stay moved
    _, chg4, _ = ops.kmeans_assign(tx, tc, seg, None, lab, return_changed=True, norms=ws)
    assert chg4.tolist() == [0, 0, 0, 5] and torch.equal(lab, keep)


# ------------------------------------------------------------------------------------------------------------------------------
# update: exact on small integers
# ------------------------------------------------------------------------------------------------------------------------------
def oracle_update32(x, labels, cent, lens, active=None):
    """cent_new as fp32 [nseg, K, C] = np.float32(np.float64(sum) / count), count, shift2 (float64 of the fp32 centres)."""
    new, cnt, sh = cent.astype(np.float32).copy(), np.zeros(cent.shape[:2], dtype=np.int32), np.zeros(cent.shape[0])
    for b, (lo, hi) in enumerate(bounds(lens)):
        if active is not None and not active[b]:
            continue
        _, count, _, sums = R.update(x[lo:hi], labels[lo:hi], cent[b])
        cnt[b] = count
        for j in range(cent.shape[1]):
            if count[j]:
                new[b, j] = np.float32(np.float64(sums[j]) / count[j])
        sh[b] = ((new[b].astype(np.float64) - cent[b].astype(np.float64)) ** 2).sum()
    return new, cnt, sh


def check_update_exact(ops, x, labels, cent, lens, active=None):
    K, C = cent.shape[1], cent.shape[2]
    want_c, want_n, want_s = oracle_update32(x, labels, cent, lens, active)
    tx, tl, tc = H.T(x, DEV), H.T(labels.astype(np.int32), DEV), H.T(cent, DEV)
    act = None if active is None else torch.tensor(active, dtype=torch.int32, device=DEV)
    on = [active is None or bool(a) for a in (active if active is not None else [1] * len(lens))]

    def run():
        cnt = filled((len(lens), K), torch.int32)
        new, cnt2, sh = ops.kmeans_update(tx, tl, tc, seg_of(ops, lens), act, count=cnt)
        assert cnt2 is cnt and all(is_fill(cnt[b]) for b in range(len(lens)) if not on[b])      # an inactive bag's counts are not written
        inplace = ops.kmeans_pad(tc).contiguous().clone()                                       # (C = 50: the padded image)
        _, _, sh2 = ops.kmeans_update(tx, tl, inplace, seg_of(ops, lens), act, out=inplace)     # cent_new may be cent itself
        assert torch.equal(inplace[..., :C], new) and torch.equal(sh2, sh)
        return new, cnt[torch.tensor(on, device=DEV)], sh

    new, cnt, sh = four_runs(run)
    assert new.dtype == np.float32 and cnt.dtype == np.int32 and sh.dtype == np.float32
    assert np.array_equal(new.view(np.int32), want_c.view(np.int32))           # bits: an empty cluster and an inactive bag keep cent
    assert np.array_equal(cnt, want_n[np.array(on)])
    # shift2: each of the K C terms (a - b)^2 carries three fp32 roundings and each of at most K C additions of non-negative terms one more
    assert (np.abs(sh - want_s) <= (K * C + 3) * 2.0 ** -24 * want_s).all(), (sh, want_s)
    assert all(s == 0.0 for s, o in zip(sh, on) if not o)
    return want_n


def test_update_exact_slab_empty_cluster_one_cluster_and_inactive_bag(ops):
    K, C = 8, 64
    assert {"up_chunk_short", "up_chunks", "up_row_tail", "up_col_short", "as_bag_k"} <= walks(SLAB, C, K)
    x = int_feats(sum(SLAB), C, 5)
    cent = int_feats(len(SLAB) * K, C, 6).reshape(len(SLAB), K, C)
    labels, _ = oracle_assign(x, cent, SLAB)
    b = bounds(SLAB)
    labels[b[1][0]:b[1][1]][labels[b[1][0]:b[1][1]] == 3] = 4                  # bag 1: cluster 3 is empty
    labels[b[2][0]:b[2][1]] = 5                                                # bag 2: every row in one cluster
    cnt = check_update_exact(ops, x, labels, cent, SLAB)
    assert cnt[1, 3] == 0 and cnt[1].sum() == 200 and cnt[2].tolist() == [0, 0, 0, 0, 0, 33, 0, 0] and (cnt[3] > 0).all()
    check_update_exact(ops, x, labels, cent, SLAB, active=[1, 0, 1, 1])
    check_update_exact(ops, x, labels, cent, SLAB, active=[0, 1, 0, 0])


@pytest.mark.parametrize("N,C,K,want", [(9, 32, 8, {"up_chunk_short", "up_row_tail", "up_col_short"}),
                                        (200, 1024, 8, {"up_chunk_short", "up_chunks", "up_col_tiles"}),
                                        (1031, 64, 17, {"up_chunk_short", "up_chunks", "up_row_tail"}),
                                        (300, 50, 9, {"up_chunks", "as_c_pad", "up_col_short"}),
                                        (300, 32, 32, {"up_chunks", "as_k_32"}),
                                        (256, 256, 1, set())])
def test_update_exact_on_small_integers(ops, N, C, K, want):
    got = walks([N], C, K)
    assert want <= got and (N != 256 or not {"up_chunk_short", "up_row_tail", "up_col_short", "up_col_tiles"} & got)
    x, cent = int_feats(N, C, 3 * N + K), int_feats(K, C, 5 * N + K)[None]
    labels, _ = oracle_assign(x, cent, [N])
    check_update_exact(ops, x, labels, cent, [N])


# ------------------------------------------------------------------------------------------------------------------------------
# batched equals solo; seeding
# ------------------------------------------------------------------------------------------------------------------------------
def test_batched_equals_solo_single_calls(ops):
    """Real-valued rows: the sums round, so equal bits mean equal ORDER -- chunks counted from the bag's first row, not from the slab's."""
    K, C = 8, 96
    x = CASES.normal("solo", sum(SLAB), C)
    cent = np.stack([x[lo:lo + K] for lo, _ in bounds(SLAB)]) + np.float32(0.25)
    tx, tc, seg = H.T(x, DEV), H.T(cent, DEV), seg_of(ops, SLAB)
    lab, d2, _ = ops.kmeans_assign(tx, tc, seg, return_dist=True)
    new, cnt, sh = ops.kmeans_update(tx, lab, tc, seg)
    for b, (lo, hi) in enumerate(bounds(SLAB)):
        l1, d1, _ = ops.kmeans_assign(tx[lo:hi], tc[b], return_dist=True)
        n1, c1, s1 = ops.kmeans_update(tx[lo:hi], l1, tc[b])
        P.assert_same_bits([[lab[lo:hi], d2[lo:hi], new[b], cnt[b], sh[b]], [l1, d1, n1, c1[0], s1[0]]], names=("slab", f"bag {b} alone"))


def test_batched_equals_solo_whole_run_and_seeding(ops):
    from advmil_amd import wsicluster
    K, C = 8, 64
    xi = int_feats(sum(SLAB), C, 21)
    ti, seg = H.T(xi, DEV), seg_of(ops, SLAB)
    rows = wsicluster.seed_rows(ti, K, 42, seg).cpu().numpy()
    for b, (lo, hi) in enumerate(bounds(SLAB)):                               # integer data: every distance exact, the picks EQUAL the oracle's
        want = R.seed_rows(xi[lo:hi], K, wsicluster.seeding_uniforms(42, hi - lo, C, K))
        assert rows[b].tolist() == want, (b, rows[b].tolist(), want)
        assert wsicluster.seed_rows(ti[lo:hi], K, 42).cpu().numpy()[0].tolist() == want
    assert sorted(rows[0].tolist()) == list(range(8))                         # the bag of exactly K rows: every row is picked once
    for t in (ti, H.T(CASES.halfnormal(sum(SLAB), C, tag="solo-run"), DEV)):
        lab, info = wsicluster.kmeans(t, K, seed=42, seg=seg, return_info=True)
        assert int(info["n_iter"].max()) > int(info["n_iter"].min())          # the bags stop in different iterations: the mask is at work
        for b, (lo, hi) in enumerate(bounds(SLAB)):
            l1, i1 = wsicluster.kmeans(t[lo:hi], K, seed=42, return_info=True)
            P.assert_same_bits([[lab[lo:hi], info["centers"][b], info["count"][b], info["inertia"][b], info["n_iter"][b]],
                                [l1, i1["centers"][0], i1["count"][0], i1["inertia"][0], i1["n_iter"][0]]], names=("slab", f"bag {b} alone"))


# ------------------------------------------------------------------------------------------------------------------------------
# real-valued features
# ------------------------------------------------------------------------------------------------------------------------------
REAL = {"blobs_1031x64": lambda: (CASES.blobs(1031, 64, 8, tag="real64", spread=1.0)[0], 8),
        "blobs_1031x1024": lambda: (CASES.blobs(1031, 1024, 8, tag="real1024", spread=1.0)[0], 8),
        "half_1500x96": lambda: (CASES.halfnormal(1500, 96, tag="h96"), 8),
        "half_700x1024": lambda: (CASES.halfnormal(700, 1024, tag="h1024"), 8),
        "half_300x32_k32": lambda: (CASES.halfnormal(300, 32, tag="k32"), 32)}


def deltas(x, cent):
    x, cent = x.astype(np.float64), cent.astype(np.float64)
    return 2e-5 * ((x * x).sum(axis=1)[:, None] + (cent * cent).sum(axis=1)[None, :])


def update_bound(x, labels, count):
    """(count_j + 1) 2^-24 mean_{i in j} |x_ic| per element [K, C]: recursive fp32 summation of count_j terms, then the division."""
    K = len(count)
    out = np.zeros((K, x.shape[1]))
    for j in range(K):
        if count[j]:
            out[j] = (count[j] + 1) * 2.0 ** -24 * np.abs(x[labels == j].astype(np.float64)).mean(axis=0)
    return out


@pytest.mark.parametrize("name", list(REAL))
def test_assign_and_update_real_valued(ops, name):
    """One assign from K random rows as centres, one update from the oracle's labels. Rows left out of the label comparison (oracle gap
    between best and second best <= the two deltas summed), from the oracle alone: blobs_1031x64 0 %, blobs_1031x1024 0.10 %,
    half_1500x96 0 %, half_700x1024 0.57 %, half_300x32_k32 0 % (cap 5 %). Largest |dist2 - d64| / (n_i + c_j) measured on an MI355X when
    this file was written: 3.8e-6, 3.1e-6, 3.7e-6, 3.0e-6, 4.7e-6 in that order (bound 2e-5)."""
    x, K = REAL[name]()
    N = x.shape[0]
    cent = x[np.random.default_rng(len(name)).permutation(N)[:K]].copy()
    want_l, _, D = R.assign(x, cent)
    dl = deltas(x, cent)
    tx, tc = H.T(x, DEV), H.T(cent, DEV)
    lab, d2, _ = [v.cpu().numpy() for v in ops.kmeans_assign(tx, tc, return_dist=True)]
    i = np.arange(N)
    assert lab.min() >= 0 and lab.max() < K
    err = np.abs(d2.astype(np.float64) - D[i, lab])
    print(f"kmeans_assign real-valued {name}: max |dist2 - d64| / (n_i + c_j) = {(err / (dl[i, lab] / 2e-5)).max():.3e}")
    assert (err <= dl[i, lab]).all(), float((err / dl[i, lab]).max())
    assert (D[i, lab] <= D.min(axis=1) + 2 * dl[i, lab]).all()
    order = np.argsort(D, axis=1, kind="stable")[:, :2]
    clear = D[i, order[:, 1]] - D[i, order[:, 0]] > dl[i, order[:, 0]] + dl[i, order[:, 1]]
    assert np.array_equal(lab[clear], want_l[clear]), int((lab[clear] != want_l[clear]).sum())
    print(f"kmeans_assign real-valued {name}: rows left out = {100.0 * (1 - clear.mean()):.2f} %")
    assert (~clear).sum() <= 0.05 * N
    c64, count, _, _ = R.update(x, want_l, cent)
    new, cnt, _ = [v.cpu().numpy() for v in ops.kmeans_update(tx, H.T(want_l, DEV), tc)]
    assert np.array_equal(cnt[0], count)
    assert (np.abs(new.astype(np.float64) - c64) <= update_bound(x, want_l, count)).all()


def run_golden(ops, name):
    from advmil_amd import wsicluster
    x, init, K = CASES.golden_cases()[name]
    lab, info = wsicluster.kmeans(H.T(x, DEV), K, init=H.T(init, DEV), return_info=True)
    return x, K, lab.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}


def test_separated_blobs_equal_the_recorded_sklearn_run(ops, fixture):
    x, K, lab, info = run_golden(ops, "separated")
    want = fixture["separated_labels"].astype(np.int32)
    assert lab.dtype == np.int32 and np.array_equal(lab, want)                 # sklearn's labels, which are also the true partition
    assert int(info["n_iter"][0]) == int(fixture["separated_n_iter"])
    count = np.bincount(want, minlength=K)
    assert np.array_equal(info["count"][0], count)
    assert (np.abs(info["centers"][0].astype(np.float64) - fixture["separated_centers"]) <= update_bound(x, want, count)).all()
    slack = deltas(x, info["centers"][0])[np.arange(len(lab)), lab].sum()
    assert abs(float(info["inertia"][0]) - float(fixture["separated_inertia"])) <= slack


def test_overlapping_data_reaches_a_fixed_point(ops, fixture):
    """A trajectory may leave sklearn's at a near-tie, so the fixed point is asserted, not the path. On the MI355X run this file was
    written with the path did not leave it: 35 iterations (sklearn 35) and the labels EQUALLED the fixture's, 0 of 1500 differed."""
    x, K, lab, info = run_golden(ops, "overlap")
    cent = info["centers"][0]
    D, dl, i = R.dist2(x, cent), deltas(x, cent), np.arange(len(lab))
    assert (D[i, lab] <= D.min(axis=1) + 2 * dl[i, lab]).all()                 # every label within 2 delta of the float64 best
    count = np.bincount(lab, minlength=K)
    assert np.array_equal(info["count"][0], count)
    c64 = R.update(x, lab, cent)[0]
    assert (np.abs(cent.astype(np.float64) - c64) <= update_bound(x, lab, count))[count > 0].all()
    assert 1 <= int(info["n_iter"][0]) <= 300
    diff = int((lab != fixture["overlap_labels"]).sum())
    print(f"kmeans overlap: n_iter {int(info['n_iter'][0])} (sklearn {int(fixture['overlap_n_iter'])}), labels differing from sklearn's: {diff}")


def test_max_iter_bounds_the_loop(ops, fixture):
    from advmil_amd import wsicluster
    x, init, K = CASES.golden_cases()["overlap"]
    lab, info = wsicluster.kmeans(H.T(x, DEV), K, init=H.T(init, DEV), max_iter=3, return_info=True)
    want = R.lloyd(x, init, max_iter=3)
    assert int(info["n_iter"][0]) == 3 == want["n_iter"]
    cent = info["centers"][0].cpu().numpy()
    D, dl, i = R.dist2(x, cent), deltas(x, cent), np.arange(len(x))
    got = lab.cpu().numpy()
    assert (D[i, got] <= D.min(axis=1) + 2 * dl[i, got]).all()                     # the extra assign: labels belong to the RETURNED centres
    assert np.array_equal(info["count"][0].cpu().numpy(), np.bincount(got, minlength=K))


# ------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------
def test_cluster_patient_feeds_deepattmisl(ops):
    from advmil_amd import synth, wsicluster
    from advmil_amd.model.backbone import DeepAttMISL
    K = 8
    x, truth = CASES.blobs(1031, 64, K)
    tx = H.T(x, DEV)
    slides = [tx[:400], tx[400:700], tx[700:]]
    ids = wsicluster.cluster_patient(slides, K, seed=42)
    assert ids.dtype == torch.float32 and tuple(ids.shape) == (1031,) and float(ids.min()) >= 0 and float(ids.max()) < K
    assert torch.equal(ids, wsicluster.kmeans(tx, K, seed=42).to(torch.float32))
    many = wsicluster.cluster_patients([slides, [tx[:300]], [tx[300:650], tx[650:]]], K, seed=42)
    assert torch.equal(many[0], ids) and [int(m.shape[0]) for m in many] == [1031, 300, 731]
    assert torch.equal(many[1], wsicluster.cluster_patient([tx[:300]], K, seed=42))
    want = R.kmeans(x, K, u=[wsicluster.seeding_uniforms(42, 1031, 64, K)])[0]
    assert len(set(truth[want["rows"]].tolist())) == K                         # the seeding found every blob: the partition is the true one
    oracle_ids = torch.from_numpy(want["labels"].astype(np.float32)).to(DEV)
    assert torch.equal(ids, oracle_ids)
    outs = []
    for e in (ids, oracle_ids):
        bb = DeepAttMISL([64, 32, 32], num_clusters=K)
        bb.load_state_dict({k_: H.T(synth.param(H.PARAM_SEED, "kmeans-misl:" + k_, tuple(v.shape))) for k_, v in bb.state_dict().items()})
        bb = bb.to(DEV).eval()
        out = bb(tx.unsqueeze(0), e)
        out.sum().backward()
        outs.append({"H": out.detach(), **{n: p.grad for n, p in bb.named_parameters() if p.grad is not None}})
    assert set(outs[0]) == set(outs[1]) and len(outs[0]) >= 8, sorted(outs[0])
    P.assert_finite(outs[0])
    P.assert_same_bits(outs, names=("cluster_patient ids", "oracle ids"))
