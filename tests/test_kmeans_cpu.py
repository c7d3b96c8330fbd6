"""CPU: the batched k-means without a GPU -- the oracle (tests/kmeans_ref.py) against the recorded sklearn runs
(tests/golden/kmeans_v1.npz, tests/golden/gen_golden_kmeans.py) and against live sklearn where it is installed, its seeding rule on a case
written out by hand, the four new entry points in header / binding table / library, every validation rule of the two launching ones
(argument checks run before anything is enqueued: fake aligned addresses, as tests/test_abi_negative_cpu.py; EVERY call below is an
invalid one), and the Python layer's refusals (advmil_amd/ops.py kmeans_*, advmil_amd/wsicluster.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import kmeans_cases as CASES
from tests import kmeans_ref as R
from tests.test_abi_cpu import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -2
A16 = 0x7F0000001000
NEW = ("advmil_kmeans_assign_workspace_bytes", "advmil_kmeans_assign", "advmil_kmeans_update_workspace_bytes", "advmil_kmeans_update")


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
    return np.load(os.path.join(ROOT, "tests", "golden", "kmeans_v1.npz"))


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def assert_same_run(r, labels, centers, n_iter, inertia):
    assert np.array_equal(r["labels"], labels.astype(np.int32)), int((r["labels"] != labels).sum())
    assert r["n_iter"] == int(n_iter)
    assert np.abs(r["centers"] - centers).max() <= 1e-12 * np.abs(centers).max()
    assert abs(r["inertia"] - float(inertia)) <= 1e-9 * float(inertia)
    assert np.array_equal(r["count"], np.bincount(labels, minlength=centers.shape[0]))


@pytest.mark.parametrize("name", ["separated", "overlap"])
def test_oracle_equals_the_recorded_sklearn_run(fixture, name):
    x, init, K = CASES.golden_cases()[name]
    r = R.lloyd(x, init)
    assert_same_run(r, fixture[name + "_labels"], fixture[name + "_centers"], fixture[name + "_n_iter"], fixture[name + "_inertia"])
    assert fixture[name + "_labels"].shape == (x.shape[0],) and fixture[name + "_centers"].shape == (K, x.shape[1])
    if name == "separated":                                 # the recorded labels are also the true partition
        assert np.array_equal(fixture[name + "_labels"], CASES.blobs(1031, 64, K)[1])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kmeans_v1.npz")) < 64 * 1024


@pytest.mark.parametrize("name", ["separated", "overlap", "small"])
def test_oracle_equals_live_sklearn(name):
    cluster = pytest.importorskip("sklearn.cluster")
    if name == "small":
        x = CASES.halfnormal(300, 32, tag="small")
        init, K = x[::20][:15].copy(), 15
    else:
        x, init, K = CASES.golden_cases()[name]
    km = cluster.KMeans(n_clusters=K, init=init.astype(np.float64), n_init=1, algorithm="lloyd", tol=1e-4, max_iter=300).fit(x.astype(np.float64))
    assert_same_run(R.lloyd(x, init), km.labels_, km.cluster_centers_, km.n_iter_, km.inertia_)


def test_oracle_ties_empty_clusters_and_the_stop_rule_by_hand():
    x = np.array([[0.0], [1.0], [2.0], [10.0], [11.0]])
    lab, d2, _ = R.assign(x, np.array([[1.0], [1.0], [10.5], [50.0]]))
    assert lab.tolist() == [0, 0, 0, 2, 2] and d2.tolist() == [1.0, 0.0, 1.0, 0.25, 0.25]            # duplicate centres 0 / 1: lowest j
    assert R.assign(x, np.array([[0.5], [1.5]]))[0].tolist() == [0, 0, 1, 1, 1]                          # row 1 at 0.25 from both
    new, count, shift2, _ = R.update(x, lab, np.array([[1.0], [1.0], [10.5], [50.0]]))
    assert new[:, 0].tolist() == [1.0, 1.0, 10.5, 50.0] and count.tolist() == [3, 0, 2, 0] and shift2 == 0.0     # empty clusters keep their centre
    r = R.lloyd(x, np.array([[0.0], [1.0]]))
    # it 1: {0} | {1, 2, 10, 11} -> (0, 6); it 2: {0, 1, 2} | {10, 11} -> (1, 10.5); it 3: same labels -> stop, no label changed
    assert r["labels"].tolist() == [0, 0, 0, 1, 1] and r["n_iter"] == 3 and r["centers"][:, 0].tolist() == [1.0, 10.5] and r["inertia"] == 2.5
    # a loose tolerance stops after iteration 1 on the centre shift (25 <= 1e3 var): the labels are then re-assigned against (0, 6)
    r = R.lloyd(x, np.array([[0.0], [1.0]]), tol=1e3)
    assert r["n_iter"] == 1 and r["centers"][:, 0].tolist() == [0.0, 6.0] and r["labels"].tolist() == [0, 0, 0, 1, 1]
    assert R.lloyd(x, np.array([[0.0], [1.0]]), max_iter=1)["n_iter"] == 1


def test_oracle_seeding_rule_by_hand():
    """Rows 0, 1, 3, 7 on a line. u_0 = 0.5 -> row floor(0.5 * 4) = 2 (x = 3). min d2 = (9, 4, 0, 16), prefix (9, 13, 13, 29), total 29:
    u_1 = 0.4 -> 11.6: the first prefix above it is row 1 (13). Then min d2 = (1, 0, 0, 16), prefix (1, 1, 1, 17), total 17:
    u_2 = 0.05 -> 0.85 -> row 0; u_2 = 0.5 -> 8.5 -> row 3; a picked row (distance 0) is never the first to exceed."""
    x = np.array([[0.0], [1.0], [3.0], [7.0]])
    assert R.seed_rows(x, 3, [0.5, 0.4, 0.05]) == [2, 1, 0]
    assert R.seed_rows(x, 3, [0.5, 0.4, 0.5]) == [2, 1, 3]
    assert R.seed_rows(x, 2, [0.999, 0.0]) == [3, 0]                       # u = 0: the first row with a positive prefix
    same = np.ones((5, 2))
    assert R.seed_rows(same, 3, [0.3, 0.5, 0.99]) == [1, 2, 4]            # total == 0: row floor(u n)
    from advmil_amd import wsicluster
    u = wsicluster.seeding_uniforms(42, 200, 64, 8)
    assert u.shape == (8,) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u, wsicluster.seeding_uniforms(42, 200, 64, 8)) and not np.array_equal(u, wsicluster.seeding_uniforms(43, 200, 64, 8))


# ------------------------------------------------------------------------------------------------------------------------------
# the ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_and_library(L):
    syms = header_symbols()
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in syms and name in L.SIGNATURES and hasattr(handle, name), name
    lib = L.lib()
    assert lib.advmil_kmeans_assign_workspace_bytes(1000, 64, 8) == 8000                # norms | moved flags
    assert lib.advmil_kmeans_assign_workspace_bytes(1001, 1024, 32) == 2 * 4016
    assert lib.advmil_kmeans_assign_workspace_bytes(1000, 64, 33) == 0 and lib.advmil_kmeans_assign_workspace_bytes(0, 64, 8) == 0
    # update: chunk partials of 128 rows [nseg, chunks, K, C] fp32 | their counts | the shift shares [nseg, K, column tiles of 256]
    assert lib.advmil_kmeans_update_workspace_bytes(1031, 64, 8, 3) == 3 * 9 * 8 * 64 * 4 + 3 * 9 * 8 * 4 + 3 * 8 * 1 * 4
    assert lib.advmil_kmeans_update_workspace_bytes(128, 1024, 8, 1) == 8 * 1024 * 4 + 32 + 8 * 4 * 4
    assert lib.advmil_kmeans_update_workspace_bytes(0, 64, 8, 1) == 0 and lib.advmil_kmeans_update_workspace_bytes(10, 64, 0, 1) == 0


def test_assign_entry_validates_before_it_launches(L):
    lib = L.lib()
    N, C, K = 100, 64, 8
    need = lib.advmil_kmeans_assign_workspace_bytes(N, C, K)
    f = lambda hi=p(0), lo=p(1), ldx=C, N=N, C=C, K=K, nseg=1, seg=None, act=None, cent=p(2), ready=0, lab=p(3), d2=p(4), chg=p(5), ws=p(6), wsb=need: (   # noqa: E731
        lib.advmil_kmeans_assign(hi, lo, ldx, N, C, K, nseg, seg, act, cent, ready, lab, d2, chg, ws, wsb, None))
    assert f(hi=None) == EINVAL and f(lo=None) == EINVAL and f(cent=None) == EINVAL and f(lab=None) == EINVAL and f(ws=None) == EINVAL
    assert f(N=0) == EINVAL and f(N=-5) == EINVAL and f(N=1 << 31) == EINVAL           # labels are int32
    assert f(K=0) == EINVAL and f(K=33) == EINVAL
    assert f(C=48, ldx=48) == EINVAL and f(C=0, ldx=0) == EINVAL                       # C % 32
    assert f(hi=p(0, 8)) == EINVAL and f(lo=p(1, 2)) == EINVAL and f(cent=p(2, 4)) == EINVAL     # 16-byte units
    assert f(ldx=60) == EINVAL and f(ldx=68) == EINVAL                                 # pitch >= C, pitch % 8
    assert f(nseg=0) == EINVAL and f(nseg=3) == EINVAL                                 # three bags, no offsets
    assert f(K=32, C=1248, ldx=1248) == EINVAL                                         # K (C + 8) > 37 856: the centres do not fit in LDS
    assert f(wsb=need - 4) == EWORKSPACE and f(wsb=0) == EWORKSPACE
    assert f(ws=p(6, 2)) == EINVAL


def test_update_entry_validates_before_it_launches(L):
    lib = L.lib()
    N, C, K = 300, 64, 8
    need = lib.advmil_kmeans_update_workspace_bytes(N, C, K, 1)
    f = lambda x=p(0), ldx=C, N=N, C=C, K=K, nseg=1, seg=None, mlen=N, act=None, lab=p(1), cent=p(2), cnew=p(3), cnt=p(4), sh=p(5), ws=p(6), wsb=need: (   # noqa: E731
        lib.advmil_kmeans_update(x, ldx, N, C, K, nseg, seg, mlen, act, lab, cent, cnew, cnt, sh, ws, wsb, None))
    for name in ("x", "lab", "cent", "cnew", "cnt", "sh", "ws"):
        assert f(**{name: None}) == EINVAL, name
    assert f(N=0, mlen=0) == EINVAL and f(N=1 << 31) == EINVAL
    assert f(K=0) == EINVAL and f(K=33) == EINVAL
    assert f(C=40, ldx=40) == EINVAL and f(C=0, ldx=0) == EINVAL
    assert f(x=p(0, 4)) == EINVAL and f(cent=p(2, 8)) == EINVAL and f(cnew=p(3, 4)) == EINVAL and f(ws=p(6, 8)) == EINVAL
    assert f(ldx=60) == EINVAL and f(ldx=66) == EINVAL                                 # pitch >= C, pitch % 4
    assert f(nseg=0) == EINVAL and f(nseg=2, mlen=150) == EINVAL                       # two bags, no offsets
    assert f(mlen=0) == EINVAL and f(mlen=N + 1) == EINVAL
    assert f(wsb=need - 4) == EWORKSPACE and f(wsb=0) == EWORKSPACE


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_have_no_fallback(L):
    from advmil_amd import ops, wsicluster
    x, c = torch.zeros(40, 32), torch.zeros(8, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_assign(x, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_update(x, torch.zeros(40, dtype=torch.int32), c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wsicluster.kmeans(x, 8, init=c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wsicluster.cluster_patient([x, x])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wsicluster.cluster_patients([[x], [x, x]])


def test_bad_arguments_are_refused_by_name():
    from advmil_amd import ops, wsicluster
    x = torch.zeros(58, 32)
    seg = ops.Segments([20, 7, 31], "cpu")
    for K in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="n_clusters = "):
            wsicluster.kmeans(x, K)
    with pytest.raises(ValueError, match="n_clusters = 33"):
        ops.kmeans_assign(x, torch.zeros(33, 32))
    with pytest.raises(ValueError, match="n_clusters = 33"):
        ops.kmeans_update(x, torch.zeros(58, dtype=torch.int32), torch.zeros(33, 32))
    with pytest.raises(ValueError, match="bag 1 has 7 rows, fewer than n_clusters = 8"):
        wsicluster.kmeans(x, 8, seg=seg)
    with pytest.raises(ValueError, match="bag 0 has 5 rows"):
        wsicluster.kmeans(torch.zeros(5, 32), 8)
    with pytest.raises(ValueError, match="bag 1 has 3 rows"):
        wsicluster.cluster_patients([[torch.zeros(9, 32)], [torch.zeros(1, 32), torch.zeros(2, 32)]])
    with pytest.raises(ValueError, match="cover 58 rows"):
        wsicluster.kmeans(torch.zeros(60, 32), 4, seg=seg)
    with pytest.raises(ValueError, match="cover 58 rows"):
        ops.kmeans_assign(torch.zeros(60, 32), torch.zeros(3, 4, 32), seg)
    for bad in (torch.zeros(8, 31), torch.zeros(7, 32), torch.zeros(2, 8, 32), torch.zeros(8)):
        with pytest.raises(ValueError, match="init must be"):
            wsicluster.kmeans(x, 8, init=bad)
    with pytest.raises(ValueError, match=r"init must be \[3, 4, 32\]"):
        wsicluster.kmeans(x, 4, init=torch.zeros(4, 32), seg=seg)                    # one set of centres for three bags
    with pytest.raises(ValueError, match="init = 'random'"):
        wsicluster.kmeans(x, 8, init="random")
    with pytest.raises(ValueError, match="max_iter"):
        wsicluster.kmeans(x, 8, max_iter=0)
    with pytest.raises(ValueError, match="centres must be"):
        ops.kmeans_assign(x, torch.zeros(8, 64))
    with pytest.raises(ValueError, match="centres must be"):
        ops.kmeans_update(x, torch.zeros(58, dtype=torch.int32), torch.zeros(2, 8, 32), seg)
    with pytest.raises(ValueError, match="features must be"):
        wsicluster.kmeans(torch.zeros(58), 8)
    with pytest.raises(ValueError, match="without slides"):
        wsicluster.cluster_patient([])
    with pytest.raises(ValueError, match="no patient"):
        wsicluster.cluster_patients([])
