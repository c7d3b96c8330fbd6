"""GPU: advmil_logrank_rows (csrc/strat.hip) against its float64 restatement (tests/logrank_ref.py, pinned to scipy on the CPU): the six
counts bit for bit, E1, V, the curves and z inside the restatement's derived rounding bounds, the medians equal; and what
advmil_amd/eval/stratify.py builds on it against the same numpy expressions over the restatement's rows. Every kernel case runs plain
twice and under both allocation poisons (tests/poison.py) with equal bits.

Sizes: a wavefront takes 64 sorted samples per trip (n = 63, 64, 65, 129, 200: under, at and over one trip, three and four trips) and a
workgroup four rows (R = 1, 3, 5, 65: under one workgroup, over one, seventeen of them with a ragged last)."""
import importlib

import numpy as np
import pytest
import torch

from tests import logrank_ref as R
from tests.poison import assert_same_bits, three_runs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NS = [1, 2, 63, 64, 65, 129, 200]
RS = [1, 3, 5, 65]


def S():
    return importlib.import_module("advmil_amd.eval.stratify")       # (the package exports a function of the same name)


def _pitched(a, pad, fill):
    """a [rows, n] -> a device view of it inside a block with `pad` more columns holding `fill` (a row pitch > n)."""
    a = np.ascontiguousarray(a)
    wide = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=a.dtype)
    wide[:, :a.shape[1]] = a
    return torch.from_numpy(wide).to(DEV)[:, :a.shape[1]]


def _launch(ev, tm, G, W, at, pad=0):
    """-> the result tree of one logrank_rows call; `pad` > 0 gives every 2-D operand a row pitch and garbage behind each row."""
    from advmil_amd.eval import logrank_rows
    G = np.asarray(G, dtype=np.uint8)
    if G.ndim == 2:
        g = _pitched(G, pad + 3, 1) if pad else torch.from_numpy(np.ascontiguousarray(G)).to(DEV)
    else:
        g = torch.from_numpy(G).to(DEV)
    w = None
    if W is not None:
        w = _pitched(np.asarray(W, dtype=np.int32), pad, 7777) if pad else torch.from_numpy(np.ascontiguousarray(W, dtype=np.int32)).to(DEV)
    r = logrank_rows(torch.from_numpy(ev), torch.from_numpy(tm), g, w, None if at is None else torch.from_numpy(at))
    # what reached the C entry: the pitched views themselves, not dense copies (the pitch of a single row is arbitrary: n is handed over)
    n, many = tm.size, max(G.shape[0] if G.ndim == 2 else 0, 0 if W is None else len(W)) > 1
    assert r.ldg == (0 if G.ndim == 1 else (g.stride(0) if many else n)) and r.ldw == (0 if W is None else (w.stride(0) if many else n))
    if pad and many:
        assert (G.ndim == 1 or r.ldg == n + pad + 3 > n) and (W is None or r.ldw == n + pad > n)
    return dict(counts=r.counts, sums=r.sums, km=r.km, median=r.median)


def _compare(got, want, what=""):
    """got: numpy counts, sums, km, median of the kernel; want: Cohort.rows(...). Counts and medians equal, the rest inside the bounds."""
    from advmil_amd.eval import logrank_from_rows
    bad = np.argwhere(got["counts"] != want["counts"])
    assert bad.size == 0, (what, bad[:5].tolist(), got["counts"][bad[0][0]].tolist(), want["counts"][bad[0][0]].tolist())
    dE, dV = np.abs(got["sums"][:, 0] - want["E1"]), np.abs(got["sums"][:, 1] - want["V"])
    assert (dE <= want["bE1"]).all(), (what, "E1", int(np.argmax(dE - want["bE1"])), dE.max())
    assert (dV <= want["bV"]).all(), (what, "V", int(np.argmax(dV - want["bV"])), dV.max())
    assert np.array_equal(got["median"], want["median"]), (what, np.argwhere(got["median"] != want["median"])[:5].tolist())
    if want["km"].shape[-1]:
        assert got["km"].shape == want["km"].shape
        assert np.array_equal(got["km"] == 0, want["km"] == 0) and np.array_equal(got["km"] == 1, want["km"] == 1), what
        dk = np.abs(got["km"] - want["km"])
        assert (dk <= want["bkm"][:, None, None] * want["km"]).all(), (what, "km", dk.max())
    s = logrank_from_rows(got["counts"], got["sums"])
    assert np.array_equal(s.undefined, want["undefined"]), what
    ok = ~s.undefined
    assert (np.abs(s.z[ok] - want["z"][ok]) <= want["bz"][ok]).all(), (what, "z")
    assert np.isnan(s.z[~ok]).all()
    return s


def _exact(ev, tm, G, W, at, pad=0, what=""):
    """Four runs with equal bits, compared with the restatement -> (numpy results, the restatement's)."""
    runs = three_runs(lambda: _launch(ev, tm, G, W, at, pad))
    assert_same_bits(runs)
    got = {k: v.cpu().numpy() for k, v in runs[0].items()}
    assert got["counts"].dtype == np.int64 and got["sums"].dtype == np.float64 and got["km"].dtype == np.float64
    want = R.Cohort(ev, tm).rows(G, W, at)
    _compare(got, want, what)
    return got, want


def _queries(tm):
    """Before every time, at every time, between them and after the last."""
    return np.unique(np.concatenate([tm, tm + np.float32(0.01), [np.float32(-1.0), np.float32(1e3)]]).astype(np.float32))


def _weights(rs, n, rows):
    W = R.multiplicities(rs.randint(0, n, size=(rows, n)), n)
    W[rs.randint(rows)] += rs.randint(0, 3, size=n).astype(np.int32)          # one row that is no bootstrap draw
    return W


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("rows", RS)
def test_kernel_equals_restatement_around_the_trip_and_the_workgroup(n, rows):
    rs = np.random.RandomState(1000 * n + rows)
    ev, tm, g, _ = R.cohort(n * 7 + rows, n, 0.5, time_levels=(0 if (n + rows) % 2 else max(2, n // 3)))
    G = (rs.rand(rows, n) < 0.5).astype(np.uint8)
    G[0] = g
    W = _weights(rs, n, rows)
    at = _queries(tm)
    a, _ = _exact(ev, tm, G, None, at, pad=0, what="per-row groups")
    b, _ = _exact(ev, tm, G, None, at, pad=5, what="per-row groups, pitched")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    c, _ = _exact(ev, tm, G, W, at, pad=0, what="groups and weights")
    d, _ = _exact(ev, tm, G, W, at, pad=2, what="groups and weights, pitched")
    for k in c:
        assert np.array_equal(c[k], d[k]), k
    any_value = (G * rs.randint(1, 256, size=G.shape)).astype(np.uint8)        # "not 0" is group 1, whatever the byte
    v, _ = _exact(ev, tm, any_value, W, at, pad=1, what="group bytes other than 1, pitched")
    for k in c:
        assert np.array_equal(c[k], v[k]), k
    _exact(ev, tm, g, W, at, pad=0, what="shared groups, weights")
    _exact(ev, tm, g, W, None, pad=3, what="shared groups, weights pitched, no queries")
    one, _ = _exact(ev, tm, g, None, at, what="one shared row")
    for k in one:                                                              # row 0 of the batch carries the same groups, unit weights
        assert np.array_equal(one[k][0], a[k][0]), k


TIES = ["all_equal", "straddles_a_trip", "longer_than_a_trip", "no_ties", "block_of_weight_zero"]


@pytest.mark.parametrize("kind", TIES)
def test_tie_structures(kind):
    rs = np.random.RandomState(TIES.index(kind))
    n, rows = 200, 5
    tm = np.arange(n, dtype=np.float64)
    ev = (rs.rand(n) < 0.6)
    lo, hi = 0, 0
    if kind == "all_equal":
        n = 130
        tm, ev = np.full(n, 0.5), ev[:n]
    elif kind == "straddles_a_trip":
        lo, hi = 60, 71
    elif kind == "longer_than_a_trip":
        lo, hi = 30, 140
    elif kind == "block_of_weight_zero":
        lo, hi = 100, 110
    tm[lo:hi] = lo
    if hi:
        ev[lo], ev[hi - 1] = True, True
    W = _weights(rs, n, rows)
    if kind == "block_of_weight_zero":
        W[2, lo:hi] = 0
        W[3, lo:hi] = 0
        W[3, hi:] = 0                                                          # ... and nothing after it either
    G = (rs.rand(rows, n) < 0.5).astype(np.uint8)
    p = rs.permutation(n)                                                      # the caller's sample order is not the time order
    ev, tm, G, W = ev[p].astype(np.float32), tm[p].astype(np.float32), np.ascontiguousarray(G[:, p]), np.ascontiguousarray(W[:, p])
    got, want = _exact(ev, tm, G, W, _queries(tm), pad=1, what=kind)
    if kind == "all_equal":
        assert (got["counts"][:, 4] <= 1).all() and got["counts"][:, 4].max() == 1
    if kind == "no_ties":
        assert (got["counts"][:, 4] == [int(((ev != 0) & (W[r] > 0)).sum()) for r in range(rows)]).all()
    _exact(ev, tm, G, None, _queries(tm), what=kind + ", unit weights")


@pytest.mark.parametrize("n", [5, 70])
def test_dense_query_grid_over_a_small_cohort(n):
    """The grid a curve is plotted on: far more query times than samples, so a lane owns long runs of queries (the whole wave stores a
    run longer than four), next to short runs and runs that end exactly on a sample's time."""
    rs = np.random.RandomState(n)
    ev, tm, g, _ = R.cohort(900 + n, n, 0.6, time_levels=(0 if n == 5 else 12))
    at = np.unique(np.concatenate([np.linspace(-0.5, 1.5, 3001).astype(np.float32), tm, tm[:3] + np.float32(1e-3)]))
    G, W = (rs.rand(6, n) < 0.5).astype(np.uint8), _weights(rs, n, 6)
    got, want = _exact(ev, tm, G, W, at, pad=2, what="dense grid")
    assert got["km"].shape == (6, 3, at.size) and at.size > 3000
    one, _ = _exact(ev, tm, g, None, at, what="dense grid, one row")
    assert (one["km"][0][:, at < tm.min()] == 1).all()


def test_edge_rows_in_one_launch():
    f = np.float32
    #              0    1    2    3    4    5    6    7    8
    tm = np.array([2.0, 1.0, 2.0, 3.0, 1.0, 3.0, 2.0, 0.5, 4.0], dtype=f)      # sample 8: alone at the largest time, an event
    ev = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0], dtype=f)      # time 2.0: samples 0, 2, 6, all events
    g0 = np.array([1, 0, 0, 1, 1, 0, 0, 1, 0], dtype=np.uint8)
    n = tm.size
    one = np.ones(n, dtype=np.int32)
    rows = {
        "all_weights_zero": (g0, 0 * one),
        "one_sample_n_times": (g0, np.eye(n, dtype=np.int32)[0] * n),
        "no_event": (g0, (ev == 0).astype(np.int32) * 2),
        "all_events": (g0, (ev != 0).astype(np.int32)),
        "group_1_empty": (0 * g0, one),
        "group_0_empty": (0 * g0 + 1, one),
        "last_at_risk_an_event": (g0, one),
        "all_at_risk_die_at_once": (g0, np.array([2, 0, 1, 0, 0, 0, 3, 0, 0], dtype=np.int32)),
        "dies_out_then_nobody": (g0, np.array([1, 1, 1, 0, 1, 0, 1, 0, 0], dtype=np.int32)),
    }
    names = list(rows)
    G, W = np.stack([rows[k][0] for k in names]), np.stack([rows[k][1] for k in names])
    at = _queries(tm)
    got, want = _exact(ev, tm, G, W, at, pad=4, what="edge rows")
    s = _compare(got, want)
    i = names.index
    assert got["counts"][i("all_weights_zero")].tolist() == [0] * 6 and not got["sums"][i("all_weights_zero")].any()
    assert (got["km"][i("all_weights_zero")] == 1).all() and np.isinf(got["median"][i("all_weights_zero")]).all()
    assert got["counts"][i("one_sample_n_times")].tolist() == [n, n, n, n, 1, 1] and got["sums"][i("one_sample_n_times")].tolist() == [n, 0.0]
    assert got["counts"][i("no_event"), 1] == 0 and got["counts"][i("no_event"), 4] == 0 and (got["km"][i("no_event")] == 1).all()
    assert got["counts"][i("all_events"), 1] == got["counts"][i("all_events"), 3]
    for k in ("all_weights_zero", "one_sample_n_times", "no_event", "group_1_empty", "group_0_empty", "all_at_risk_die_at_once"):
        assert s.undefined[i(k)], k
    for k in ("all_events", "last_at_risk_an_event", "dies_out_then_nobody"):
        assert not s.undefined[i(k)], k
    last = got["counts"][i("last_at_risk_an_event")]
    assert last[4] == 4 and last[5] == 3                                       # four event times, the last with one at risk: no V term
    q_end = at >= f(4.0)
    assert (got["km"][i("last_at_risk_an_event"), 2][q_end] == 0).all() and (got["km"][i("last_at_risk_an_event"), 0][q_end] == 0).all()
    assert (got["km"][i("last_at_risk_an_event"), 1][q_end] > 0).all()         # group 1 ends on a censored sample
    die = i("all_at_risk_die_at_once")
    assert got["counts"][die].tolist() == [2, 6, 2, 6, 1, 1] and got["sums"][die].tolist() == [2.0, 0.0]
    assert (got["km"][die][:, at >= f(2.0)] == 0).all() and (got["km"][die][:, at < f(2.0)] == 1).all()
    assert got["median"][die].tolist() == [2.0, 2.0, 2.0]
    gone = got["km"][i("dies_out_then_nobody"), 2]
    assert (gone[at >= f(2.0)] == 0).all()                                     # nobody at risk after 2.0: the curve keeps its last value


def test_a_row_of_a_batch_has_the_bits_of_the_one_row_call():
    n, rows = 200, 65
    rs = np.random.RandomState(65)
    ev, tm, _, _ = R.cohort(65, n, 0.5, time_levels=40)
    G, W, at = (rs.rand(rows, n) < 0.4).astype(np.uint8), _weights(rs, n, rows), _queries(tm)
    batch = _launch(ev, tm, G, W, at, pad=3)
    again = _launch(ev, tm, G, W, at, pad=0)
    assert_same_bits([batch, again], names=("pitched", "dense"))
    for r in (0, 1, 3, 4, 31, 63, 64):
        single = _launch(ev, tm, G[r:r + 1], W[r:r + 1], at)
        assert_same_bits([{k: v[r:r + 1] for k, v in batch.items()}, single], names=(f"row {r} of {rows}", "alone"))
    head = _launch(ev, tm, G[:5], W[:5], at)                                   # ... nor do they move with R
    assert_same_bits([{k: v[:5] for k, v in batch.items()}, head], names=("first five of 65", "five"))


# ---- API level --------------------------------------------------------------------------------------------------------------------------
N_API, SEED = 200, 0


@pytest.fixture(scope="module")
def api():
    """n = 200, half the samples events, times rounded to 0.05, the median split of the risk randn - t; the restatement of the observed
    split, of 300 resamples and of 500 permutations, computed once."""
    y, pred = R.api_cohort(N_API)
    tm, ev = y[:, 0].copy(), y[:, 1].copy()
    g, thr = R.risk_groups(-pred[:, 0])
    co = R.Cohort(ev, tm)
    at = np.unique(tm[ev != 0])
    B, P = 300, 500
    idx = np.random.RandomState(SEED).randint(0, N_API, size=(B, N_API))
    W = R.multiplicities(idx, N_API)
    rs = np.random.RandomState(SEED)
    perms = np.stack([rs.permutation(g) for _ in range(P)])
    return dict(y=y, pred=pred, tm=tm, ev=ev, g=g, thr=thr, co=co, at=at, B=B, P=P, W=W, perms=perms, obs=co.row(g, None, at),
                boot=co.rows(g, W, at), perm=co.rows(perms))


def test_api_cohort_leaves_no_resample_undefined():
    for n in (N_API, 65):
        y, pred = R.api_cohort(n)
        g, _ = R.risk_groups(-pred[:, 0])
        co = R.Cohort(y[:, 1], y[:, 0])
        for seed in (0, 1):
            W = R.multiplicities(np.random.RandomState(seed).randint(0, n, size=(1000, n)), n)
            assert not co.rows(g, W)["undefined"].any(), (n, seed)


def test_logrank_test_is_the_restatements(api):
    from advmil_amd.eval import logrank_test
    r = logrank_test(api["ev"], api["tm"], api["g"])
    o = api["obs"]
    assert r.counts.tolist() == o["counts"].tolist() and not r.undefined
    assert abs(r.E1 - o["E1"]) <= o["bE1"] and abs(r.V - o["V"]) <= o["bV"] and abs(r.z - o["z"]) <= o["bz"]
    assert r.chi2 == r.z ** 2 and abs(r.p - R.p_of(o["z"])) <= 1e-9 * r.p


def test_kaplan_meier_bands_and_median_intervals(api):
    from advmil_amd.eval import kaplan_meier
    level = 0.9
    r = kaplan_meier(api["ev"], api["tm"], api["g"], n_boot=api["B"], seed=SEED, level=level)
    o, b = api["obs"], api["boot"]
    assert np.array_equal(r.at, api["at"])                                     # the default queries: the distinct event times
    assert (np.abs(r.surv - o["km"]) <= o["bkm"] * o["km"]).all() and np.array_equal(r.median, o["median"])
    assert r.n_undefined == 0 and r.samples.shape == (api["B"], 3, api["at"].size)
    tol = b["bkm"][:, None, None] * b["km"]
    assert (np.abs(r.samples - b["km"]) <= tol).all()
    assert np.array_equal(r.median_samples, b["median"])
    pct = [50 * (1 - level), 50 * (1 + level)]
    lo, hi = np.nanpercentile(r.samples, pct, axis=0)
    assert np.array_equal(r.lo, lo) and np.array_equal(r.hi, hi)               # numpy over the rows ...
    wlo, whi = np.nanpercentile(b["km"], pct, axis=0)                          # ... which lie within the bound of the restatement's
    assert (np.abs(r.lo - wlo) <= tol.max(axis=0)).all() and (np.abs(r.hi - whi) <= tol.max(axis=0)).all()
    assert np.array_equal(r.median_lo, np.nanpercentile(b["median"], pct[0], axis=0, method="lower"))
    assert np.array_equal(r.median_hi, np.nanpercentile(b["median"], pct[1], axis=0, method="higher"))
    assert (r.lo <= r.hi).all() and (r.median_lo <= r.median_hi).all()
    idx = np.random.RandomState(SEED).randint(0, N_API, size=(api["B"], N_API))
    again = kaplan_meier(api["ev"], api["tm"], api["g"], indices=idx, level=level, at=api["at"])
    assert np.array_equal(again.samples, r.samples) and np.array_equal(again.lo, r.lo)
    plain = kaplan_meier(api["ev"], api["tm"])                                 # no groups, no resamples: the pooled curve
    assert np.array_equal(plain.surv[2], r.surv[2]) and np.array_equal(plain.surv[0], r.surv[2]) and (plain.surv[1] == 1).all()
    assert not hasattr(plain, "lo")


def _p_perm(z_perm, z_obs):
    ok = ~np.isnan(z_perm)
    return (1 + int((np.abs(z_perm[ok]) >= abs(z_obs)).sum())) / (1 + int(ok.sum()))


def test_permutation_test(api):
    from advmil_amd.eval import logrank_permutation_test
    r = logrank_permutation_test(api["ev"], api["tm"], api["g"], n_perm=api["P"], seed=SEED)
    o, p = api["obs"], api["perm"]
    assert r.n_undefined == 0 and not p["undefined"].any()
    assert abs(r.z - o["z"]) <= o["bz"] and (np.abs(r.z_perm - p["z"]) <= p["bz"]).all()
    assert r.p_perm == _p_perm(r.z_perm, r.z)
    # no permutation's |z| lies within the rounding bounds of the observed one, so the count is the restatement's
    assert not (np.abs(np.abs(p["z"]) - abs(o["z"])) <= p["bz"] + o["bz"]).any()
    assert r.p_perm == _p_perm(p["z"], o["z"]) and 0 < r.p_perm <= 1


def _hazards(n):
    rs = np.random.RandomState(9)
    return (0.05 + 0.9 * rs.rand(n, 4)).astype(np.float32)


@pytest.mark.parametrize("kind", ["continuous", "hazards"])
def test_stratify(api, kind):
    from advmil_amd.eval import bootstrap as BS
    from advmil_amd.eval import stratify
    y = api["y"]
    pred = api["pred"] if kind == "continuous" else _hazards(N_API)
    B, P, level = 200, 100, 0.9
    r = stratify(y, pred, n_perm=P, n_boot=B, seed=SEED, level=level)
    risk = BS._risks(torch.from_numpy(y), torch.from_numpy(pred))[2].cpu().numpy()
    g, thr = R.risk_groups(risk)
    if kind == "continuous":
        assert np.array_equal(g, api["g"]) and thr == api["thr"]
    co = api["co"]
    o = co.row(g)
    rs = np.random.RandomState(SEED)
    perm = co.rows(np.stack([rs.permutation(g) for _ in range(P)]))
    boot = co.rows(g, R.multiplicities(np.random.RandomState(SEED).randint(0, N_API, size=(B, N_API)), N_API))
    c = o["counts"]
    assert (r.threshold, r.n_low, r.n_high, r.events_low, r.events_high) == (thr, c[3] - c[2], c[2], c[1] - c[0], c[0])
    assert (r.median_low, r.median_high) == (o["median"][0], o["median"][1])
    assert abs(r.z - o["z"]) <= o["bz"] and r.chi2 == r.z ** 2 and abs(r.p - R.p_of(o["z"])) <= 1e-9 * r.p
    assert not (np.abs(np.abs(perm["z"]) - abs(o["z"])) <= perm["bz"] + o["bz"]).any()
    assert r.p_perm == _p_perm(perm["z"], o["z"]) and r.n_undefined_perm == 0
    assert r.n_undefined == 0 and (np.abs(r.z_samples - boot["z"]) <= boot["bz"]).all()
    pct = [50 * (1 - level), 50 * (1 + level)]
    assert (r.z_lo, r.z_hi) == tuple(np.nanpercentile(r.z_samples, pct))
    wlo, whi = np.nanpercentile(boot["z"], pct)
    assert abs(r.z_lo - wlo) <= boot["bz"].max() and abs(r.z_hi - whi) <= boot["bz"].max()
    bare = stratify(y, pred)
    assert (bare.z, bare.p, bare.n_high) == (r.z, r.p, r.n_high) and bare.p_perm is None and bare.z_lo is None


def test_logrank_scan(api):
    from advmil_amd.eval import logrank_scan
    n_cuts, P = 8, 50
    r = logrank_scan(api["y"], api["pred"], n_cuts=n_cuts, min_frac=0.15, n_perm=P, seed=SEED)
    risk = -api["pred"][:, 0]
    qs, G = [], []
    for c in range(n_cuts):
        g, _ = R.risk_groups(risk, (c + 1) / (n_cuts + 1))
        k = int(g.sum())
        if min(k, N_API - k) >= 0.15 * N_API and not (G and np.array_equal(G[-1], g)):
            qs.append((c + 1) / (n_cuts + 1)), G.append(g)
    G = np.stack(G)
    assert 2 <= len(qs) < n_cuts and np.array_equal(r.quantiles, qs) and np.array_equal(r.n_high, G.sum(axis=1))   # min_frac drops the ends
    co = api["co"]
    obs = co.rows(G)
    assert (np.abs(r.z - obs["z"]) <= obs["bz"]).all()
    best = int(np.argmax(np.abs(obs["z"])))
    gap = np.sort(np.abs(obs["z"]))[-1] - np.sort(np.abs(obs["z"]))[-2]
    assert gap > 2 * obs["bz"].max() and r.best == best and r.best_quantile == qs[best] and r.z_best == r.z[best]
    rs = np.random.RandomState(SEED)
    zmax = np.empty(P)
    for p in range(P):
        rows = co.rows(G[:, rs.permutation(N_API)])
        assert not rows["undefined"].any()
        zmax[p] = np.abs(rows["z"]).max()
        assert abs(r.max_abs_z_perm[p] - zmax[p]) <= rows["bz"].max()
    assert not (np.abs(zmax - abs(obs["z"][best])) <= 4 * obs["bz"].max()).any()
    assert r.p_adjusted == (1 + int((zmax >= abs(obs["z"][best])).sum())) / (1 + P)
    assert 0 < r.p_adjusted <= 1


def test_logrank_scan_chunks_its_launches(api, monkeypatch):
    """The same scan with the cap on a launch's [rows, n] array lowered so that the 20 permutations take several launches."""
    from advmil_amd.eval import logrank_scan
    whole = logrank_scan(api["y"], api["pred"], n_cuts=4, n_perm=20, seed=3)
    C = whole.z.size
    monkeypatch.setattr(S(), "MAX_ROW_BYTES", 3 * C * N_API)                   # three permutations per launch: seven launches
    parts = logrank_scan(api["y"], api["pred"], n_cuts=4, n_perm=20, seed=3)
    assert np.array_equal(parts.max_abs_z_perm, whole.max_abs_z_perm) and parts.p_adjusted == whole.p_adjusted


def test_evaluators_stratify_by_the_estimate_their_c_index_ranks_by(api):
    from advmil_amd.eval import ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator, stratify
    from advmil_amd.eval import bootstrap as BS
    y = torch.from_numpy(api["y"])
    pa = torch.from_numpy(api["pred"])
    pb = torch.from_numpy(api["pred"][::-1].copy())
    hz = torch.from_numpy(_hazards(N_API))
    yd = y.clone()
    yd[:, 0] = torch.from_numpy(np.random.RandomState(9).randint(0, 4, size=N_API).astype(np.float32))
    y1 = y.clone()
    y1[:, 0] = 0.0                                                             # one bin: every sample carries bin index 0
    keys = {"n_low", "n_high", "events_low", "events_high", "median_low", "median_high", "z", "chi2", "p", "p_perm", "z_lo", "z_hi", "n_undefined"}
    for evl, data, yy, pred in ((ContSurv_Evaluator(end_time=1.0), {"y": y, "y_hat": pa}, y, pa),
                                (CoxSurv_Evaluator(), {"y": y, "y_hat": pb, "avg_y_hat": pa}, y, pa),
                                (DiscSurv_Evaluator(), {"y": yd, "y_hat": hz}, yd, hz), (DiscSurv_Evaluator(), {"y": y1, "y_hat": hz[:, :1]}, y1, hz[:, :1])):
        d = evl.stratify(data, n_perm=40, n_boot=40, seed=SEED)
        assert set(d) == keys
        # numpy over the restatement on the same rows: the split of the risk concordance_index forms from this prediction
        risk = BS._risks(yy, pred)[2].cpu().numpy()
        g, _ = R.risk_groups(risk)
        co = R.Cohort(yy[:, 1].numpy(), yy[:, 0].numpy())
        o = co.row(g)
        rs = np.random.RandomState(SEED)
        perm = co.rows(np.stack([rs.permutation(g) for _ in range(40)]))
        boot = co.rows(g, R.multiplicities(np.random.RandomState(SEED).randint(0, N_API, size=(40, N_API)), N_API))
        c = o["counts"]
        name = type(evl).__name__
        assert (d["n_low"], d["n_high"], d["events_low"], d["events_high"]) == (c[3] - c[2], c[2], c[1] - c[0], c[0]), name
        assert (d["median_low"], d["median_high"]) == (o["median"][0], o["median"][1]), name
        if o["undefined"]:
            assert np.isnan(d["z"]), name
            continue
        assert abs(d["z"] - o["z"]) <= o["bz"] and abs(d["p"] - R.p_of(o["z"])) <= 1e-9 * d["p"], name
        assert d["p_perm"] == _p_perm(perm["z"], o["z"]), name
        wlo, whi = np.nanpercentile(boot["z"], [2.5, 97.5])
        assert abs(d["z_lo"] - wlo) <= boot["bz"].max() and abs(d["z_hi"] - whi) <= boot["bz"].max() and d["n_undefined"] == 0, name
        s = stratify(yy, pred, n_perm=40, n_boot=40, seed=SEED)
        assert (s.z, s.p, s.p_perm, s.z_lo, s.z_hi) == (d["z"], d["p"], d["p_perm"], d["z_lo"], d["z_hi"]), name


def test_cap_on_undefined_resamples():
    """t = [1, 2, 3, 4], e = [1, 0, 0, 0], g = [1, 1, 0, 0]: 401 of the 1000 resamples of seed 0 draw no event, one group only, or V == 0."""
    from advmil_amd.eval import stratify
    t, e = np.array([1, 2, 3, 4], dtype=np.float32), np.array([1, 0, 0, 0], dtype=np.float32)
    y, pred = np.stack([t, e], axis=1), t.reshape(-1, 1).copy()               # a predicted time: risk = -t, the high half is [1, 1, 0, 0]
    g = np.array([1, 1, 0, 0], dtype=np.uint8)
    B = 1000
    W = R.multiplicities(np.random.RandomState(0).randint(0, 4, size=(B, 4)), 4)
    want = R.Cohort(e, t).rows(g, W)
    assert int(want["undefined"].sum()) == 401
    with pytest.raises(ValueError, match="resamples"):
        stratify(y, pred, n_boot=B, seed=0)
    r = stratify(y, pred, n_boot=B, seed=0, max_undefined=1)
    assert (r.n_high, r.n_low, r.events_high) == (2, 2, 1)
    assert r.n_undefined == 401 and np.array_equal(np.isnan(r.z_samples), want["undefined"])
    ok = ~want["undefined"]
    assert (np.abs(r.z_samples[ok] - want["z"][ok]) <= want["bz"][ok]).all()
    assert (r.z_lo, r.z_hi) == tuple(np.nanpercentile(r.z_samples, [2.5, 97.5]))
