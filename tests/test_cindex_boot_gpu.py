"""GPU: advmil_cindex_counts_weighted against its numpy restatement (tests/cindex_boot_ref.py, pinned to the oracle on the CPU), exactly,
on all eight counters; against advmil_cindex_counts itself on the expanded arrays; and the statistics built on it against the same
numpy expressions over the oracle's per-resample values. Every exact case runs plain twice and under both allocation poisons."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cindex_oracle as CO
from tests import cindex_boot_ref as R
from tests.poison import assert_same_bits, three_runs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _consts():
    from advmil_amd import _lib
    return _lib.CINDEX_BOOT_ROW_TILE, _lib.CINDEX_BOOT_RESAMPLE_CHUNK, _lib.CINDEX_BOOT_MAX_CHUNK_BLOCKS


T, RC, MAXC = _consts()          # imported, not copied: the sizes below sit around the kernel's own constants
NS = [2, 3, T - 1, T, T + 1, 2 * T + 1]
BS = [1, RC - 1, RC, RC + 1, 2 * RC + 1]
MS = [1, 2, 31, 64]


def _pitched(a, pad, fill):
    """a [rows, n] -> a device view of it inside a block with `pad` more columns holding `fill` (a row pitch > n)."""
    a = np.ascontiguousarray(a)
    wide = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=a.dtype)
    wide[:, :a.shape[1]] = a
    return torch.from_numpy(wide).to(DEV)[:, :a.shape[1]]


def _launch(ev, tm, est, W, pad=0, tied_tol=1e-8):
    from advmil_amd.eval import concordance_counts_weighted
    e = _pitched(est, pad, np.nan) if pad else torch.from_numpy(np.ascontiguousarray(est)).to(DEV)
    w = _pitched(W, pad + 3 if pad else 0, 7777) if pad else torch.from_numpy(np.ascontiguousarray(W)).to(DEV)
    assert not pad or (e.stride(0) > e.shape[1] and w.stride(0) > w.shape[1])
    return concordance_counts_weighted(torch.from_numpy(ev), torch.from_numpy(tm), e, w, tied_tol=tied_tol)


def _exact(ev, tm, est, W, pad=0, tied_tol=1e-8):
    """Four runs with equal bits, equal to the restatement on all eight counters -> the counts (numpy)."""
    runs = three_runs(lambda: _launch(ev, tm, est, W, pad, tied_tol))
    assert_same_bits(runs)
    got = runs[0].cpu().numpy()
    want = R.counts_weighted(ev, tm, est, W, tied_tol)
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def _weights(rs, n, B):
    W = R.multiplicities(rs.randint(0, n, size=(B, n)), n)
    W[rs.randint(B), :] += rs.randint(0, 3, size=n).astype(np.int32)         # one row that is no bootstrap draw
    return W


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
def test_kernel_equals_restatement_around_the_tile_and_the_chunk(n, B):
    M = MS[(NS.index(n) + BS.index(B)) % len(MS)]
    p_event = 0.15 if n > 3 and (NS.index(n) + BS.index(B)) % 2 else 0.5
    ev, tm, est = R.boot_case(NS.index(n) * 8 + BS.index(B), n, p_event, time_levels=7, est_levels=5, M=M)
    W = _weights(np.random.RandomState(n * 31 + B), n, B)
    got = _exact(ev, tm, est, W, pad=5)
    assert got[:, :, 7].min() >= 1


@pytest.mark.parametrize("M", MS)
def test_every_estimate_row_count_with_and_without_a_pitch(M):
    n, B = T + 1, RC + 1
    ev, tm, est = R.boot_case(300 + M, n, 0.5, time_levels=11, est_levels=6, M=M)
    W = _weights(np.random.RandomState(M), n, B)
    a = _exact(ev, tm, est, W, pad=0)
    b = _exact(ev, tm, est, W, pad=1)
    assert np.array_equal(a, b)


def test_more_chunks_than_workgroups_take_the_stride_loop():
    n, B = 3, MAXC * RC + RC + 1
    ev, tm, est = R.boot_case(400, n, 0.5, M=2)
    ev[0] = 1.0
    W = np.random.RandomState(4).randint(0, 3, size=(B, n)).astype(np.int32)
    _exact(ev, tm, est, W, pad=0)


def _plain_counts(ev, tm, est):
    """advmil_cindex_counts on plain arrays -> its six counters."""
    from advmil_amd import _lib
    d = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in (tm, ev, est)]
    out = torch.empty(6, dtype=torch.int64, device=DEV)
    rc = _lib.lib().advmil_cindex_counts(*(ctypes.c_void_p(t.data_ptr()) for t in d), d[0].numel(), 1e-8, ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, rc
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [2, 65, 2 * T + 1])
def test_unit_weights_give_the_bits_of_the_existing_entry(n):
    ev, tm, est = R.boot_case(500 + n, n, 0.5, time_levels=9, est_levels=5, M=2)
    got = _exact(ev, tm, est, np.ones((2, n), dtype=np.int32), pad=2)
    for m in range(2):
        want = _plain_counts(ev, tm, est[m])
        assert got[m, 0, :6].tolist() == want.tolist() and got[m, 1, :6].tolist() == want.tolist()
    assert got[0, 0, 6] == int((ev != 0).sum()) and got[0, 0, 7] == n


def test_counts_are_those_of_the_existing_entry_on_the_expanded_arrays():
    """The contract itself, slot 5 included: sample i repeated w_i times through advmil_cindex_counts."""
    n = 65
    ev, tm, est = R.boot_case(600, n, 0.15, M=1)
    W = _weights(np.random.RandomState(6), n, RC + 1)
    got = _exact(ev, tm, est, W, pad=1)
    for b in range(W.shape[0]):
        xe, xt, xs = R.expand(W[b], ev, tm, est[0])
        assert got[0, b, :6].tolist() == _plain_counts(xe, xt, xs).tolist(), b


def test_edge_rows_of_the_weights():
    f = np.float32
    tol = f(0.25)
    above = np.nextafter(f(1.25), f(2.0))
    #              0     1     2     3      4     5     6     7     8
    tm = np.array([1.0,  1.0,  1.0,  2.0,   2.0,  3.0,  3.0,  0.5,  4.0], dtype=f)     # time ties with mixed events
    ev = np.array([1.0,  0.0,  1.0,  1.0,   0.0,  0.0,  1.0,  0.0,  1.0], dtype=f)     # sample 8: the only sample at the largest time
    est = np.array([[1.0, 1.25, above, 1.0, 1.25, above, 0.5, 1.0,  0.75],              # exactly tol apart, and one float above it
                    [above, 1.0, 1.0, 1.25, 1.0,  1.0,  1.25, above, 1.0]], dtype=f)
    n = tm.size
    assert f(1.25) - f(1.0) == tol and above - f(1.0) > tol
    rows = {
        "event_n_times": np.eye(n, dtype=np.int32)[0] * n,
        "censored_n_times": np.eye(n, dtype=np.int32)[1] * n,
        "all_zero": np.zeros(n, dtype=np.int32),
        "size_one": np.eye(n, dtype=np.int32)[3],
        "no_event_copy": (ev == 0).astype(np.int32) * 2,
        "event_alone_at_the_end": np.array([0, 2, 0, 0, 1, 3, 0, 1, 1], dtype=np.int32),
        "two_copies_alone_at_the_end": np.array([0, 2, 0, 0, 1, 3, 0, 1, 2], dtype=np.int32),
        "largest_multiplicity": np.array([n, 1, 1, 1, 1, 1, 1, 1, 1], dtype=np.int32),
        "tied_group_only": np.array([2, 3, 1, 0, 0, 0, 0, 0, 0], dtype=np.int32),
        "around_the_tolerance": np.array([1, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.int32),
        "ones": np.ones(n, dtype=np.int32),
    }
    W = np.stack(list(rows.values()))
    got = _exact(ev, tm, est, W, pad=3, tied_tol=float(tol))
    code = R.classify(got)
    names = list(rows)
    want_code = {"event_n_times": R.NO_PAIR, "censored_n_times": R.ALL_CENSORED, "all_zero": R.TOO_SMALL, "size_one": R.TOO_SMALL,
                 "no_event_copy": R.ALL_CENSORED, "event_alone_at_the_end": R.NO_COMPARABLE, "two_copies_alone_at_the_end": R.NO_PAIR,
                 "largest_multiplicity": R.OK, "tied_group_only": R.OK, "around_the_tolerance": R.OK, "ones": R.OK}
    for b, name in enumerate(names):
        for m in range(2):
            assert code[m, b] == want_code[name], (name, m, got[m, b].tolist())
            wcode, wc, wcounts = R.oracle_resample(CO, ev, tm, est[m], W[b], tied_tol=float(tol))
            assert wcode == code[m, b], name
            if wcounts is not None:
                assert got[m, b, :4].tolist() == list(wcounts), (name, m)
    # by hand, estimate row 0. Anchor 0 (w 2) and anchor 2 (w 1) share their time with the censored sample 1 (w 3) and are no pair of
    # each other; |1.25 - 1.0| == tol and |1.25 - above| is one ulp: both tied
    assert got[0, names.index("tied_group_only")].tolist() == [0, 0, 9, 9, 9, 3, 3, 6]
    # anchor 0 against sample 1 (exactly tol apart: tied) and the later sample 5 (one float further: e_j > e_i, discordant)
    assert got[0, names.index("around_the_tolerance")].tolist() == [0, 1, 1, 1, 2, 1, 1, 3]
    assert got[0, names.index("event_n_times"), 5] == n and got[0, names.index("event_alone_at_the_end"), 5] == 0


# ---- statistics level -------------------------------------------------------------------------------------------------------------
N_STAT, B_STAT, SEED = 64, 200, 11


@pytest.fixture(scope="module")
def stat():
    """n = 64, half the samples events, two models; the oracle's C-index of every resample through the documented indices."""
    rs = np.random.RandomState(8)
    tm = (np.floor(rs.rand(N_STAT) * 20) / 20).astype(np.float32)
    ev = np.zeros(N_STAT, dtype=np.float32)
    ev[rs.permutation(N_STAT)[:N_STAT // 2]] = 1.0
    pa = (tm + 0.3 * rs.randn(N_STAT)).astype(np.float32)                    # predictions of a time: the reference negates them
    pb = (tm + 0.6 * rs.randn(N_STAT)).astype(np.float32)
    pb[:8] = pa[:8]
    idx = np.random.RandomState(SEED).randint(0, N_STAT, size=(B_STAT, N_STAT))
    orc = np.array([[CO.cindex_counts(ev[i] != 0, tm[i], -p[i])[0] for i in idx] for p in (pa, pb)])
    return dict(y=np.stack([tm, ev], axis=1), pa=pa.reshape(-1, 1), pb=pb.reshape(-1, 1), idx=idx, orc=orc)


def test_bootstrap_interval_equals_numpy_over_the_oracle(stat):
    from advmil_amd.eval import bootstrap_concordance_index, concordance_index
    r = bootstrap_concordance_index(stat["y"], stat["pa"], n_boot=B_STAT, seed=SEED, level=0.9)
    s = stat["orc"][0]
    assert r.n_undefined == 0 and r.samples.dtype == np.float64 and np.array_equal(r.samples, s)
    lo, hi = np.nanpercentile(s, [50 * (1 - 0.9), 50 * (1 + 0.9)])
    assert (r.lo, r.hi, r.se) == (lo, hi, np.nanstd(s, ddof=1))
    assert r.cindex == concordance_index(torch.from_numpy(stat["y"]), torch.from_numpy(stat["pa"]))
    assert r.counts.shape == (B_STAT, 8) and (r.counts[:, 7] == N_STAT).all()
    again = bootstrap_concordance_index(stat["y"], stat["pa"], indices=stat["idx"], level=0.9)
    assert np.array_equal(again.samples, s) and (again.lo, again.hi) == (r.lo, r.hi)


def test_paired_comparison_equals_numpy_over_the_oracle(stat):
    from advmil_amd.eval import paired_bootstrap_concordance
    r = paired_bootstrap_concordance(stat["y"], stat["pa"], stat["pb"], n_boot=B_STAT, seed=SEED)
    d = stat["orc"][0] - stat["orc"][1]
    assert np.array_equal(r.delta_samples, d) and r.delta == r.cindex_a - r.cindex_b
    lo, hi = np.nanpercentile(d, [50 * (1 - 0.95), 50 * (1 + 0.95)])
    assert (r.lo, r.hi) == (lo, hi)
    want_p = min(1.0, 2.0 * min(int((d <= 0).sum()) + 1, int((d >= 0).sum()) + 1) / (d.size + 1))
    assert r.p_value == want_p and 0 < r.p_value <= 1
    same = paired_bootstrap_concordance(stat["y"], stat["pa"], stat["pa"], n_boot=B_STAT, seed=SEED)
    assert same.delta == 0 and same.p_value == 1.0 and not same.delta_samples.any()


def test_sampled_predictions_column_by_column(stat):
    from advmil_amd.eval import bootstrap_concordance_index, bootstrap_concordance_samples
    dist = np.concatenate([stat["pa"], stat["pb"], 0.5 * (stat["pa"] + stat["pb"])], axis=1)
    r = bootstrap_concordance_samples(stat["y"], dist, n_boot=B_STAT, seed=SEED)
    assert r.samples.shape == (3, B_STAT) and np.array_equal(r.samples[:2], stat["orc"])
    for s in range(3):
        one = bootstrap_concordance_index(stat["y"], dist[:, s:s + 1], n_boot=B_STAT, seed=SEED)
        assert np.array_equal(r.samples[s], one.samples) and np.array_equal(r.counts[s], one.counts)
        assert (r.cindex[s], r.lo[s], r.hi[s], r.se[s]) == (one.cindex, one.lo, one.hi, one.se)


def test_evaluators_bootstrap_the_estimate_their_c_index_ranks_by(stat):
    from advmil_amd.eval import ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator
    y = torch.from_numpy(stat["y"])
    rs = np.random.RandomState(9)
    hz = torch.from_numpy((0.05 + 0.9 * rs.rand(N_STAT, 4)).astype(np.float32))
    yd = y.clone()
    yd[:, 0] = torch.from_numpy(rs.randint(0, 4, size=N_STAT).astype(np.float32))
    y1 = y.clone()
    y1[:, 0] = 0.0                                                           # one bin: every sample carries bin index 0
    for evl, data in ((ContSurv_Evaluator(end_time=1.0), {"y": y, "y_hat": torch.from_numpy(stat["pa"])}),
                      (CoxSurv_Evaluator(), {"y": y, "y_hat": torch.from_numpy(stat["pb"]), "avg_y_hat": torch.from_numpy(stat["pa"])}),
                      (DiscSurv_Evaluator(), {"y": yd, "y_hat": hz}), (DiscSurv_Evaluator(), {"y": y1, "y_hat": hz[:, :1]})):
        b = evl.bootstrap(data, n_boot=50, seed=SEED)
        assert set(b) == {"c_index", "c_index_lo", "c_index_hi", "c_index_se", "n_undefined"}
        assert b["c_index"] == evl.compute(data, ["c_index"])["c_index"], type(evl).__name__
        assert b["c_index_lo"] <= b["c_index_hi"] and b["c_index_se"] > 0 and b["n_undefined"] == 0
    cont = ContSurv_Evaluator(end_time=1.0).bootstrap({"y": y, "y_hat": torch.from_numpy(stat["pa"])}, n_boot=B_STAT, seed=SEED, level=0.9)
    lo, hi = np.nanpercentile(stat["orc"][0], [50 * (1 - 0.9), 50 * (1 + 0.9)])
    assert (cont["c_index_lo"], cont["c_index_hi"], cont["c_index_se"]) == (lo, hi, np.nanstd(stat["orc"][0], ddof=1))


def test_cap_on_undefined_resamples():
    """n = 17 at 15 % events (two of them): 19 of these 200 resamples draw no event, none with an entry, or no comparable pair."""
    from advmil_amd.eval import bootstrap_concordance_index
    ev, tm, est = R.boot_case(77, 17, 0.15)
    assert ev.sum() == 2
    y, pred = np.stack([tm, ev], axis=1), -est[0].reshape(-1, 1)
    B = 200
    idx = np.random.RandomState(SEED).randint(0, 17, size=(B, 17))
    refused = np.array([R.oracle_resample(CO, ev[i], tm[i], est[0][i], np.ones(17, dtype=np.int64))[0] != R.OK for i in idx])
    assert 0.05 * B < refused.sum() < B
    with pytest.raises(ValueError, match="resamples"):
        bootstrap_concordance_index(y, pred, n_boot=B, seed=SEED)
    r = bootstrap_concordance_index(y, pred, n_boot=B, seed=SEED, max_undefined=1.0)
    assert r.n_undefined == int(refused.sum()) and np.array_equal(np.isnan(r.samples), refused)
    want = np.array([R.oracle_resample(CO, ev[i], tm[i], est[0][i], np.ones(17, dtype=np.int64))[1] for i in idx])
    assert np.array_equal(r.samples[~refused], want[~refused])
    assert (r.lo, r.hi) == tuple(np.nanpercentile(want, [50 * (1 - 0.95), 50 * (1 + 0.95)]))
