"""GPU: the greedy k-means++ seeding (csrc/kmeans.hip kmeans_seed_*, advmil_amd/ops.py kmeans_seed_*, advmil_amd/wsicluster.py) against
the float64 oracle tests/kmeans_greedy_ref.py and the recorded sklearn runs tests/golden/kmeans_greedy_v1.npz.

Walks (the constants mirror csrc/kmeans.hip): both passes run on a grid (chunk of UR = 128 rows counted from the BAG's first row, bag).
In the candidate pass wave w of a workgroup owns rows [32 w, 32 w + 32) of the chunk, trial slot l sits in register l & 3 of lane half
l >> 2; the pick pass folds the chunk potentials and carries the scan from chunk to chunk. The cases:
  L = 2 (K = 1, 2), 4 (K = 8), 5 (K = 32: a slot in the second lane half); C = 32 (one half chunk) and 1024 (16 chunks, four per
  accumulator); a row pitch larger than C; bags of exactly K rows, of 127 / 128 / 129 rows (the chunk edge: a short chunk, a whole one,
  a second chunk of one row) and of 2^16 + 3 rows (513 workgroups carry the scan); a four-bag slab of unequal lengths, each bag also
  alone; a bag of identical rows (potential 0).

Exact cases: integer features in [-7, 7] make every bf16x3 distance, every float64 potential and every prefix sum exact (the argument
of tests/test_kmeans_gpu.py), so rows, closest, potentials and trial rows EQUAL the oracle, and rows equal sklearn's recorded indices.
Every exact case runs four times through tests/poison.py and must give the same bits each time.
Real-valued cases: candmin / closest within tests/test_kmeans_gpu.py::deltas of the oracle; the picks are compared in full, after the
assertion that every one of them is decidable under that bound (tests/kmeans_greedy_ref.py; the share of draws left out is zero)."""
import gc
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import kmeans_cases as CASES
from tests import kmeans_greedy_cases as G
from tests import kmeans_greedy_ref as GR
from tests import kmeans_ref as R
from tests import poison as P
from tests.test_kmeans_gpu import deltas, update_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UR = 128
GREEDY = "greedy-k-means++"


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import ops as _ops
    from advmil_amd import _lib
    _lib.lib()
    return _ops


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "kmeans_greedy_v1.npz"))


@pytest.fixture(scope="module")
def cases():
    return G.golden_cases()


def bounds(lens):
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [(int(offs[b]), int(offs[b + 1])) for b in range(len(lens))]


def seg_of(ops, lens):
    return None if len(lens) == 1 else ops.Segments(lens, DEV)


def device_draws(lens, K, state, init_index=0):
    """The oracle's draws of every bag on the device -> (first int32 [nseg], u float64 [nseg, K - 1, L], the host pairs)."""
    host = [GR.draws(state, n, K, init_index + 1)[init_index] for n in lens]
    first = torch.tensor([f for f, _ in host], dtype=torch.int32, device=DEV)
    return first, H.T(np.stack([u for _, u in host]), DEV), host


def run_seeding(ops, x, K, lens, state, planes=None, tx=None):
    first, u, host = device_draws(lens, K, state)
    tx = H.T(x, DEV) if tx is None else tx
    seg = seg_of(ops, lens)

    def run():
        rows, tr = ops.kmeans_seed_greedy(tx, K, first, u, seg, planes, return_trace=True)
        return [rows, tr["closest"], tr["pot0"], tr["pot"], tr["cand"]]

    return run, host


def check_exact(ops, x, K, lens, state=G.RANDOM_STATE, planes=None, tx=None):
    """Four runs with equal bits, every output EQUAL to the oracle's, bag by bag -> rows [nseg, K]."""
    run, host = run_seeding(ops, x, K, lens, state, planes, tx)
    trees = P.three_runs(run)
    P.assert_same_bits(trees)
    rows, closest, pot0, pot, cand = [t.cpu().numpy() for t in trees[0]]
    assert rows.dtype == np.int64 and closest.dtype == np.float32 and pot.dtype == np.float64 and cand.dtype == np.int32
    assert rows.shape == (len(lens), K) and pot.shape == (K - 1, len(lens), GR.trials(K)) and cand.shape == pot.shape
    for b, (lo, hi) in enumerate(bounds(lens)):
        s = GR.seed(x[lo:hi], K, *host[b])
        assert rows[b].tolist() == s["rows"], (b, rows[b].tolist(), s["rows"])
        assert np.array_equal(cand[:, b], s["cand"]), b
        assert pot0[b, 0] == s["pot0"] and np.array_equal(pot[:, b], s["pot"]), b
        assert np.array_equal(closest[lo:hi].astype(np.float64), s["closest"]), b
    return rows


# ------------------------------------------------------------------------------------------------------------------------------
# exact on small integers
# ------------------------------------------------------------------------------------------------------------------------------
SINGLE = ["k1_c32_n127", "k2_c32_n128", "k8_c32_n129", "blobs_k8_c32_n129", "k32_c32_n32", "k32_c32_n300", "k8_c1024_n200",
          "k32_c1024_n129", "k8_c32_big"]


@pytest.mark.parametrize("name", SINGLE)
def test_seeding_exact_on_small_integers_equals_oracle_and_sklearn(ops, fixture, cases, name):
    x, K, _ = cases[name]
    n = x.shape[0]
    assert {"k1_c32_n127": n % UR == UR - 1 and K == 1, "k2_c32_n128": n == UR and K == 2, "k8_c32_n129": n == UR + 1,
            "k32_c32_n32": n == K == 32, "k8_c32_big": n == (1 << 16) + 3 and n > 512 * UR}.get(name, True)
    assert GR.trials(K) == {1: 2, 2: 2, 8: 4, 32: 5}[K]
    rows = check_exact(ops, x, K, [n])
    assert rows[0].tolist() == fixture[name + "_idx"].tolist()               # sklearn.cluster.kmeans_plusplus(x, K, random_state=42)
    assert len(set(rows[0].tolist())) == K


def test_other_random_states_and_later_inits_follow_the_stream(ops, cases):
    from advmil_amd import wsicluster
    x, K, _ = cases["k8_c32_n129"]
    tx = H.T(x, DEV)
    for state, index in ((7, 0), (42, 2), (123456, 1)):
        first, u = GR.draws(state, 129, K, index + 1)[index]
        got = wsicluster.seed_rows_greedy(tx, K, state, init_index=index).cpu().numpy()
        assert got.dtype == np.int64 and got[0].tolist() == GR.seed(x, K, first, u)["rows"], (state, index)


def test_row_pitch_larger_than_c(ops, cases):
    x, K, _ = cases["k8_c32_n129"]
    wide = np.concatenate([x, G.ints("pitch", 129, 32)], axis=1)             # 32 more columns that must not be read
    tw = H.T(wide, DEV)
    full = ops.split_planes(tw)
    planes = ops.Planes(full.hi[:, :32], full.lo[:, :32])
    assert planes.hi.stride(0) == 64 and planes.hi.shape[1] == 32
    rows = check_exact(ops, x, K, [129], planes=planes, tx=tw[:, :32])
    assert torch.equal(ops.kmeans_seed_greedy(H.T(x, DEV), K, *device_draws([129], K, 42)[:2]), torch.from_numpy(rows).to(DEV))


def test_slab_of_four_bags_exact_and_each_bag_alone(ops, fixture):
    x, K = G.slab()
    rows = check_exact(ops, x, K, G.SLAB)
    assert sorted(rows[0].tolist()) == list(range(8))                        # the bag of exactly K rows: every row picked once
    for b, (lo, hi) in enumerate(bounds(G.SLAB)):
        assert rows[b].tolist() == fixture[f"slab_bag{b}_idx"].tolist(), b
    check_exact(ops, G.ints("slab-unstructured", sum(G.SLAB), 64), K, G.SLAB, state=7)
    check_exact(ops, x[:8 + 200], K, [8, 200])                               # a slab that ends inside the first chunk of its last bag


def test_slab_equals_solo_bit_for_bit_on_real_valued_rows(ops):
    """Real-valued rows: the potentials and prefix sums round, so equal bits mean equal ORDER -- chunks counted from the bag's first
    row, not from the slab's."""
    K, C = 8, 96
    x = CASES.normal("greedy-solo", sum(G.SLAB), C)
    tx = H.T(x, DEV)
    first, u, _ = device_draws(G.SLAB, K, 3)
    rows, tr = ops.kmeans_seed_greedy(tx, K, first, u, seg_of(ops, G.SLAB), return_trace=True)
    for b, (lo, hi) in enumerate(bounds(G.SLAB)):
        r1, t1 = ops.kmeans_seed_greedy(tx[lo:hi], K, first[b:b + 1], u[b:b + 1], return_trace=True)
        P.assert_same_bits([[rows[b], tr["closest"][lo:hi], tr["pot0"][b], tr["pot"][:, b], tr["cand"][:, b]],
                            [r1[0], t1["closest"], t1["pot0"][0], t1["pot"][:, 0], t1["cand"][:, 0]]], names=("slab", f"bag {b} alone"))


def test_a_bag_of_identical_rows_yields_row_zero(ops):
    """Potential 0: every target is 0 and the first prefix >= 0 is row 0's, as sklearn's searchsorted gives. Between two ordinary
    bags, so that a neighbour's potential cannot leak in."""
    K = 8
    lens = [150, 200, 129]
    x = G.ints("ident", sum(lens), 32)
    x[150:350] = x[150]
    rows = check_exact(ops, x, K, lens)
    first = GR.draws(G.RANDOM_STATE, 200, K)[0][0]
    assert rows[1].tolist() == [first] + [0] * (K - 1) and len(set(rows[0].tolist())) == K and len(set(rows[2].tolist())) == K


# ------------------------------------------------------------------------------------------------------------------------------
# real-valued features
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.REAL_STATES))
def test_real_valued_picks_are_all_decidable_and_equal_the_oracle(ops, name):
    """Largest |closest - c64| as a share of the row's bound, measured on an MI355X when this file was written: 0.12, 0.16, 0.20."""
    x, K, state = G.real_cases()[name]
    n = x.shape[0]
    first, u = GR.draws(state, n, K)[0]
    s = GR.seed(x, K, first, u, delta=deltas)
    assert s["draw_ok"].all() and s["pick_ok"].all()                         # first: nothing is left out of the comparison
    run, _ = run_seeding(ops, x, K, [n], state)
    rows, closest, pot0, pot, cand = [t.cpu().numpy() for t in run()]
    assert np.array_equal(cand[:, 0], s["cand"]), int((cand[:, 0] != s["cand"]).sum())
    assert rows[0].tolist() == s["rows"]
    err = np.abs(closest.astype(np.float64) - s["closest"])
    print(f"kmeans_seed real-valued {name}: max |closest - c64| / bound = {(err / s['err']).max():.3e}")
    assert (err <= s["err"]).all()
    assert np.array_equal(np.argmin(pot[:, 0], axis=1), s["best"])


@pytest.mark.parametrize("name", list(G.REAL_STATES))
def test_candidate_pass_real_valued(ops, name):
    """One candidate pass against L stated rows and a stated closest: candmin within the dist2 bound of min(closest, d64), and the
    distance bits are those kmeans_assign gives for the trial row as a centre. Largest |candmin - m64| / (n_i + n_cand) measured on an
    MI355X when this file was written: 3.2e-6, 3.0e-6, 3.9e-6 in the order of the cases (bound 2e-5)."""
    x, K, _ = G.real_cases()[name]
    n, L = x.shape[0], GR.trials(K)
    cand = np.random.default_rng(len(name)).permutation(n)[:L].astype(np.int32)
    D, dl = R.dist2(x, x[cand]), deltas(x, x[cand])
    closest = np.float32(0.9) * np.median(D, axis=1).astype(np.float32)      # about half of the trials lie below it
    tx = H.T(x, DEV)
    cm, ws = ops.kmeans_seed_cand(tx, H.T(cand[None], DEV), H.T(closest, DEV))
    got = cm.cpu().numpy().astype(np.float64)
    want = np.minimum(closest[:, None].astype(np.float64), D)
    print(f"kmeans_seed_cand real-valued {name}: max |candmin - m64| / (n_i + n_cand) = {(np.abs(got - want) / (dl / 2e-5)).max():.3e}")
    assert (np.abs(got - want) <= dl).all()
    assert (got <= closest[:, None]).all() and (got < closest[:, None]).any() and (got == closest[:, None]).any()
    plain, _ = ops.kmeans_seed_cand(tx, H.T(cand[None], DEV), None, ws=ws)   # closest None: +inf, the distances themselves
    for l in range(L):
        _, d2, _ = ops.kmeans_assign(tx, tx[int(cand[l])][None], return_dist=True)
        assert torch.equal(plain[:, l], d2), l


# ------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------
E2E = ["separated", "slab_bag1", "slab_bag2", "slab_bag3", "blobs_k8_c32_n129", "k1_c32_n127", "more_blobs"]


@pytest.mark.parametrize("n_init", [1, 3])
@pytest.mark.parametrize("name", E2E)
def test_kmeans_equals_the_recorded_sklearn_run(ops, fixture, cases, name, n_init):
    from advmil_amd import wsicluster
    x, K, _ = cases[name]
    tag = "" if n_init == 1 else "3"
    lab, info = wsicluster.kmeans(H.T(x, DEV), K, init=GREEDY, seed=42, n_init=n_init, return_info=True)
    lab = lab.cpu().numpy()
    want = fixture[name + "_labels" + tag].astype(np.int32)
    assert lab.dtype == np.int32 and np.array_equal(lab, want), int((lab != want).sum())
    count = np.bincount(want, minlength=K)
    assert np.array_equal(info["count"][0].cpu().numpy(), count)
    assert (np.abs(info["centers"][0].cpu().numpy().astype(np.float64) - fixture[name + "_centers" + tag]) <= update_bound(x, want, count)).all()
    print(f"kmeans greedy {name} n_init={n_init}: n_iter {int(info['n_iter'][0])} (sklearn {int(fixture[name + '_n_iter' + tag])})")
    if name == "more_blobs":                                                  # the case in which a later init wins
        assert not np.array_equal(fixture[name + "_labels"], fixture[name + "_labels3"])


def test_kmeans_slab_equals_the_recorded_runs_and_solo(ops, fixture):
    from advmil_amd import wsicluster
    x, K = G.slab()
    tx, seg = H.T(x, DEV), seg_of(ops, G.SLAB)
    for n_init, tag in ((1, ""), (3, "3")):
        lab, info = wsicluster.kmeans(tx, K, init=GREEDY, seed=42, seg=seg, n_init=n_init, return_info=True)
        for b, (lo, hi) in enumerate(bounds(G.SLAB)):
            assert np.array_equal(lab[lo:hi].cpu().numpy(), fixture[f"slab_bag{b}_labels{tag}"].astype(np.int32)), (n_init, b)
            l1, i1 = wsicluster.kmeans(tx[lo:hi], K, init=GREEDY, seed=42, n_init=n_init, return_info=True)
            P.assert_same_bits([[lab[lo:hi], info["centers"][b], info["count"][b], info["inertia"][b], info["n_iter"][b]],
                                [l1, i1["centers"][0], i1["count"][0], i1["inertia"][0], i1["n_iter"][0]]], names=("slab", f"bag {b} alone"))


def test_cluster_patients_equals_cluster_patient_bit_for_bit(ops, fixture):
    from advmil_amd import wsicluster
    x, K, _ = G.more_blobs()
    tx = H.T(x, DEV)
    pats = [[tx[:250], tx[250:]], [tx[:300]], [tx[300:450], tx[450:]]]
    for n_init in (1, 2):
        many = wsicluster.cluster_patients(pats, K, seed=42, init=GREEDY, n_init=n_init)
        assert [int(m.shape[0]) for m in many] == [600, 300, 300]
        for slides, ids in zip(pats, many):
            one = wsicluster.cluster_patient(slides, K, seed=42, init=GREEDY, n_init=n_init)
            assert ids.dtype == torch.float32 and torch.equal(ids, one)
    assert np.array_equal(wsicluster.cluster_patient(pats[0], K, init=GREEDY).cpu().numpy(), fixture["more_blobs_labels"].astype(np.float32))
    default = wsicluster.cluster_patient(pats[0], K, seed=42)               # the default init is still the plain D^2 seeding
    assert torch.equal(default, wsicluster.kmeans(tx, K, seed=42).to(torch.float32))
    with pytest.raises(ValueError, match="n_init = 2 needs"):
        wsicluster.kmeans(tx, K, init=tx[:K].clone(), n_init=2)


def test_whole_seeding_is_captured_on_one_stream_and_replays(ops):
    """Nothing between the first pick and the last reads the device: the 1 + 2 K launches of a four-bag slab are captured into one
    graph on one stream, and the replay returns the eager rows."""
    x, K = G.slab()
    tx, seg = H.T(x, DEV), seg_of(ops, G.SLAB)
    first, u, _ = device_draws(G.SLAB, K, G.RANDOM_STATE)
    planes = ops.kmeans_planes(tx)
    eager = ops.kmeans_seed_greedy(tx, K, first, u, seg, planes).clone()      # (every kernel has run once before the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    gc.collect()                                                              # dead cycles (with graphs of earlier tests in them) go now,
    gc.disable()                                                              # not in the middle of the capture
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                rows = ops.kmeans_seed_greedy(tx, K, first, u, seg, planes)
    finally:
        gc.enable()
    for _ in range(2):
        rows.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rows, eager)
