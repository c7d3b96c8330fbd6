"""CPU: the greedy k-means++ seeding without a GPU -- the oracle (tests/kmeans_greedy_ref.py) against the recorded sklearn runs
(tests/golden/kmeans_greedy_v1.npz, tests/golden/gen_golden_kmeans_greedy.py) and against live sklearn where it is installed, its rules
on cases written out by hand, the host side of the feature (wsicluster.sklearn_draws), the three new entry points in header / binding
table / library with every validation rule of the two launching ones (fake aligned addresses, as tests/test_kmeans_cpu.py: EVERY call
below is an invalid one), and the Python layer's refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import kmeans_greedy_cases as G
from tests import kmeans_greedy_ref as GR
from tests.test_abi_cpu import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -2
A16 = 0x7F0000001000
NEW = ("advmil_kmeans_seed_workspace_bytes", "advmil_kmeans_seed_cand", "advmil_kmeans_seed_pick")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kmeans_greedy_v1.npz")


def p(k, off=0):
    return ctypes.c_void_p(A16 + (k << 24) + off)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def cases():
    return G.golden_cases()


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def test_trial_counts_and_the_stream_by_hand():
    assert [GR.trials(K) for K in (1, 2, 3, 7, 8, 20, 21, 32)] == [2, 2, 3, 3, 4, 4, 5, 5]
    rs = np.random.RandomState(42)
    want = []
    for _ in range(2):                                                     # two inits continue ONE stream
        first = rs.choice(50, p=np.full(50, 1.0 / 50))
        want.append((first, [rs.uniform(size=4) for _ in range(7)]))
    got = GR.draws(42, 50, 8, n_init=2)
    for (f, u), (wf, wu) in zip(got, want):
        assert f == wf and u.shape == (7, 4) and np.array_equal(u, np.array(wu))
    assert got[0][0] == GR.draws(42, 50, 8)[0][0] and np.array_equal(got[0][1], GR.draws(42, 50, 8)[0][1])
    assert GR.draws(42, 50, 1)[0][1].shape == (0, 2)
    from advmil_amd import ops, wsicluster
    assert [ops.kmeans_seed_trials(K) for K in range(1, 33)] == [GR.trials(K) for K in range(1, 33)]
    f, u = wsicluster.sklearn_draws(42, 50, 8, n_init=2)                   # the product's host function draws the same numbers
    assert f.dtype == np.int64 and u.dtype == np.float64 and u.shape == (2, 7, 4)
    assert f.tolist() == [g[0] for g in got] and np.array_equal(u, np.stack([g[1] for g in got]))


def test_seeding_rule_by_hand():
    """Rows 0, 1, 3, 7, 8 on a line, K = 3 (L = 3), first centre row 2 (x = 3): closest = (9, 4, 0, 16, 25), cum (9, 13, 13, 29, 54).
    u = (0.1, 13 / 54, 0.99) -> targets (5.4, 13, 53.46): rows 0, 1 (searchsorted left: the FIRST prefix >= 13, not row 2), 4.
    Potentials: row 0 -> min(closest, (0, 1, 9, 49, 64)) = (0, 1, 0, 16, 25) = 42; row 1 -> (1, 0, 0, 16, 25) = 42; row 4 ->
    (9, 4, 0, 1, 0) = 14: the pick is row 4. Then closest = (9, 4, 0, 1, 0), cum (9, 13, 13, 14, 14); u = (0, 0.5, 0.95) -> targets
    (0, 7, 13.3): rows 0, 0, 3; potentials: row 0 -> min(closest, (0, 1, 9, 49, 64)) = (0, 1, 0, 1, 0) = 2, twice, and row 3 ->
    min(closest, (49, 36, 16, 0, 1)) = (9, 4, 0, 0, 0) = 13: the tie of trials 0 and 1 goes to the lowest, the pick is row 0."""
    x = np.array([[0.0], [1.0], [3.0], [7.0], [8.0]])
    u = np.array([[0.1, 13.0 / 54.0, 0.99], [0.0, 0.5, 0.95]])
    s = GR.seed(x, 3, 2, u)
    assert s["pot0"] == 54.0
    assert s["cand"].tolist() == [[0, 1, 4], [0, 0, 3]] and s["pot"].tolist() == [[42.0, 42.0, 14.0], [2.0, 2.0, 13.0]]
    assert s["best"].tolist() == [2, 0] and s["rows"] == [2, 4, 0] and s["closest"].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]
    same = np.ones((6, 2))                                                  # potential 0: every draw gives row 0, as sklearn does
    s = GR.seed(same, 3, 4, np.array([[0.3, 0.6, 0.9], [0.1, 0.5, 0.7]]))
    assert s["rows"] == [4, 0, 0] and s["cand"].tolist() == [[0, 0, 0], [0, 0, 0]] and s["pot"].tolist() == [[0.0] * 3] * 2
    assert GR.seed(x, 1, 3, np.zeros((0, 2)))["rows"] == [3]


def test_selection_rule_by_hand():
    a = np.array([0, 0, 1, 1, 2])
    assert GR.same_clustering(a, np.array([2, 2, 0, 0, 1]), 3) and not GR.same_clustering(a, np.array([0, 1, 1, 1, 2]), 3)
    assert GR.same_clustering(a, np.array([1, 1, 1, 1, 1]), 3)            # sklearn's rule is one-sided: a refines b
    runs = [dict(labels=a, inertia=5.0), dict(labels=np.array([1, 1, 2, 2, 0]), inertia=4.0),       # lower, but the same clustering: not kept
            dict(labels=np.array([0, 1, 1, 1, 2]), inertia=4.5), dict(labels=np.array([0, 1, 1, 2, 2]), inertia=4.5)]
    assert GR.select(runs[:2], 3) == 0 and GR.select(runs[:3], 3) == 2 and GR.select(runs, 3) == 2   # equal inertia never replaces


def test_oracle_picks_equal_the_recorded_sklearn_indices(fixture, cases):
    assert str(fixture["sklearn_version"]) >= "1.7"
    for name, (x, K, _) in cases.items():
        first, u = GR.draws(G.RANDOM_STATE, x.shape[0], K)[0]
        s = GR.seed(x, K, first, u)
        assert s["rows"] == fixture[name + "_idx"].tolist(), name
    assert os.path.getsize(FIXTURE) < 64 * 1024
    n8 = cases["slab_bag0"][0].shape[0]
    assert n8 == 8 and sorted(fixture["slab_bag0_idx"].tolist()) == list(range(8))      # a bag of exactly K distinct rows: each picked once


@pytest.mark.parametrize("n_init", [1, 3])
def test_oracle_labels_equal_the_recorded_sklearn_runs(fixture, cases, n_init):
    tag = "" if n_init == 1 else "3"
    changed = 0
    for name, (x, K, run) in cases.items():
        if not run:
            continue
        r = GR.kmeans(x, K, G.RANDOM_STATE, n_init=n_init)
        assert np.array_equal(r["labels"], fixture[name + "_labels" + tag].astype(np.int32)), name
        assert r["n_iter"] == int(fixture[name + "_n_iter" + tag]), name
        want = float(fixture[name + "_inertia" + tag])
        assert abs(r["inertia"] - want) <= 1e-9 * max(want, 1.0), name
        assert np.abs(r["centers"] - fixture[name + "_centers" + tag]).max() <= 1e-10 * max(np.abs(r["centers"]).max(), 1.0), name
        changed += r["init_index"] != 0
    assert n_init == 1 or changed >= 1                                      # the selection is at work: a later init wins in more_blobs


@pytest.mark.parametrize("name", ["slab_bag1", "blobs_k8_c32_n129", "more_blobs"])
def test_oracle_equals_live_sklearn(cases, name):
    cluster = pytest.importorskip("sklearn.cluster")
    x, K, _ = cases[name]
    for state in (G.RANDOM_STATE, 7):
        _, idx = cluster.kmeans_plusplus(x.astype(np.float64), K, random_state=state)
        first, u = GR.draws(state, x.shape[0], K)[0]
        assert GR.seed(x, K, first, u)["rows"] == idx.tolist()
        km = cluster.KMeans(n_clusters=K, random_state=state, n_init=2).fit(x.astype(np.float64))
        assert np.array_equal(GR.kmeans(x, K, state, n_init=2)["labels"], km.labels_)


def test_every_draw_of_the_real_valued_cases_is_decidable():
    """The cases of the GPU test's pick comparison: no draw and no argmin may be left out, so all of them are decidable by choice of
    the random_state (gen_golden_kmeans_greedy.py --scan). An integer case is decidable with any bound that is zero."""
    for name, (x, K, state) in G.real_cases().items():
        first, u = GR.draws(state, x.shape[0], K)[0]
        s = GR.seed(x, K, first, u, delta=G.deltas)
        assert s["draw_ok"].all() and s["pick_ok"].all(), (name, int((~s["draw_ok"]).sum()), int((~s["pick_ok"]).sum()))
        assert s["draw_ok"].shape == (K - 1, GR.trials(K)) and len(set(s["rows"])) == K
    x, K, _ = G.golden_cases()["k8_c32_n129"]
    first, u = GR.draws(42, 129, K)[0]
    s = GR.seed(x, K, first, u, delta=lambda a, c: np.zeros((len(a), len(c))))
    assert s["draw_ok"].all() and s["pick_ok"].all()
    u2 = u.copy()                                                           # a target moved ONTO a prefix value is undecidable under any bound > 0
    cum = np.cumsum(GR.R.dist2(x, x[[first]])[:, 0])
    u2[0, 0] = cum[40] / cum[-1]
    assert not GR.seed(x, K, first, u2, delta=G.deltas)["draw_ok"][0, 0]


# ------------------------------------------------------------------------------------------------------------------------------
# the ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_and_library(L):
    syms = header_symbols()
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in syms and name in L.SIGNATURES and hasattr(handle, name), name
    f = L.lib().advmil_kmeans_seed_workspace_bytes
    assert f(1000, 1000, 4, 1) == 4000 + 8 * 4 * 8                          # norms | chunk potentials [1][8][4] float64
    assert f(1001, 300, 5, 3) == 4016 + 368                                 # 3 bags x 3 chunks x 5 x 8 = 360, rounded up to 16
    assert f(1001, 300, 1, 3) == 4016 + 80                                  # 72 rounded up to 16
    assert f(0, 1, 4, 1) == 0 and f(10, 0, 4, 1) == 0 and f(10, 10, 0, 1) == 0 and f(10, 10, 9, 1) == 0 and f(10, 10, 4, 0) == 0


def test_cand_entry_validates_before_it_launches(L):
    lib = L.lib()
    N, C, Lt = 300, 64, 4
    need = lib.advmil_kmeans_seed_workspace_bytes(N, N, Lt, 1)
    f = lambda hi=p(0), lo=p(1), ldx=C, N=N, C=C, Lt=Lt, nseg=1, seg=None, mlen=N, cand=p(2), closest=p(3), ready=0, out=p(4), ws=p(5), wsb=need: (   # noqa: E731
        lib.advmil_kmeans_seed_cand(hi, lo, ldx, N, C, Lt, nseg, seg, mlen, cand, closest, ready, out, ws, wsb, None))
    for name in ("hi", "lo", "cand", "out", "ws"):
        assert f(**{name: None}) == EINVAL, name
    assert f(N=0, mlen=0) == EINVAL and f(N=1 << 31) == EINVAL
    assert f(Lt=0) == EINVAL and f(Lt=9) == EINVAL
    assert f(C=48, ldx=48) == EINVAL and f(C=0, ldx=0) == EINVAL
    assert f(hi=p(0, 8)) == EINVAL and f(lo=p(1, 2)) == EINVAL and f(cand=p(2, 2)) == EINVAL and f(closest=p(3, 1)) == EINVAL
    assert f(out=p(4, 2)) == EINVAL and f(ws=p(5, 8)) == EINVAL
    assert f(ldx=60) == EINVAL and f(ldx=68) == EINVAL
    assert f(nseg=0) == EINVAL and f(nseg=3) == EINVAL and f(nseg=65536, seg=p(6)) == EINVAL
    assert f(mlen=0) == EINVAL and f(mlen=N + 1) == EINVAL
    assert f(Lt=8, C=8192, ldx=8192) == EINVAL                              # 2 L (C + 8) halfwords do not fit in LDS
    assert f(wsb=need - 8) == EWORKSPACE and f(wsb=0) == EWORKSPACE


def test_pick_entry_validates_before_it_launches(L):
    lib = L.lib()
    N, Lt = 300, 4
    need = lib.advmil_kmeans_seed_workspace_bytes(N, N, Lt, 1)
    f = lambda N=N, Lt=Lt, nseg=1, seg=None, mlen=N, cand=p(0), cm=p(1), u=p(2), us=Lt, Ln=Lt, row=p(3), rs=1, pot=p(4), closest=p(5), nxt=p(6), ws=p(7), wsb=need: (   # noqa: E731
        lib.advmil_kmeans_seed_pick(N, Lt, nseg, seg, mlen, cand, cm, u, us, Ln, row, rs, pot, closest, nxt, ws, wsb, None))
    for name in ("cand", "cm", "u", "row", "pot", "closest", "nxt", "ws"):
        assert f(**{name: None}) == EINVAL, name
    assert f(N=0, mlen=0) == EINVAL and f(N=1 << 31) == EINVAL
    assert f(Lt=0) == EINVAL and f(Lt=9) == EINVAL and f(Ln=-1) == EINVAL and f(Ln=9, us=9) == EINVAL
    assert f(us=3) == EINVAL and f(rs=0) == EINVAL
    assert f(nxt=p(0)) == EINVAL                                            # the next trials must not overwrite the ones being read
    assert f(cand=p(0, 2)) == EINVAL and f(cm=p(1, 2)) == EINVAL and f(u=p(2, 4)) == EINVAL and f(row=p(3, 4)) == EINVAL
    assert f(pot=p(4, 4)) == EINVAL and f(closest=p(5, 2)) == EINVAL and f(nxt=p(6, 1)) == EINVAL and f(ws=p(7, 8)) == EINVAL
    assert f(nseg=0) == EINVAL and f(nseg=2) == EINVAL and f(mlen=0) == EINVAL and f(mlen=N + 1) == EINVAL
    assert f(wsb=need - 8) == EWORKSPACE and f(wsb=0) == EWORKSPACE


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_have_no_fallback(L):
    from advmil_amd import ops, wsicluster
    x = torch.zeros(40, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wsicluster.kmeans(x, 8, init="greedy-k-means++")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wsicluster.seed_rows_greedy(x, 8, 42)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wsicluster.cluster_patients([[x], [x, x]], init="greedy-k-means++", n_init=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_seed_greedy(x, 8, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 7, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_seed_cand(x, torch.zeros(1, 4, dtype=torch.int32))


def test_bad_arguments_are_refused_by_name():
    from advmil_amd import ops, wsicluster
    x = torch.zeros(58, 32)
    with pytest.raises(ValueError, match="n_init = 2 needs init = 'greedy-k-means\\+\\+'"):
        wsicluster.kmeans(x, 8, init=torch.zeros(8, 32), n_init=2)
    with pytest.raises(ValueError, match="n_init = 3 needs"):
        wsicluster.kmeans(x, 8, n_init=3)
    with pytest.raises(ValueError, match="n_init = 2 needs"):
        wsicluster.cluster_patient([x], n_init=2)
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError, match="n_init = "):
            wsicluster.kmeans(x, 8, init="greedy-k-means++", n_init=bad)
    with pytest.raises(ValueError, match="init = 'random'"):
        wsicluster.kmeans(x, 8, init="random", n_init=1)
    with pytest.raises(ValueError, match="bag 0 has 5 rows"):
        wsicluster.seed_rows_greedy(torch.zeros(5, 32), 8, 42)
    with pytest.raises(ValueError, match="init_index"):
        wsicluster.seed_rows_greedy(x, 8, 42, init_index=-1)
    with pytest.raises(ValueError, match="`u` must be"):
        ops.kmeans_seed_greedy(x, 8, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 7, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="`first` must be"):
        ops.kmeans_seed_greedy(x, 8, torch.zeros(1, dtype=torch.int64), torch.zeros(1, 7, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="`cand` must be"):
        ops.kmeans_seed_cand(x, torch.zeros(1, 9, dtype=torch.int32))
    with pytest.raises(ValueError, match="cover 58 rows"):
        ops.kmeans_seed_cand(torch.zeros(60, 32), torch.zeros(3, 4, dtype=torch.int32), seg=ops.Segments([20, 7, 31], "cpu"))
