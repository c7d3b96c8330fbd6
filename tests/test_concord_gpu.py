"""GPU: advmil_concord_rows (csrc/concord.hip) against its float64 restatement (tests/concord_ref.py, pinned on the CPU to exact rationals
and to cohorts worked by hand): the pair counts and the G = 0 counts bit for bit, the Uno sums inside the header's derived bound plus the
restatement's own (3 n 2^-52 each); and what advmil_amd/eval/concordance.py and the evaluators build on it. Every kernel case runs plain
twice and under both allocation poisons (tests/poison.py) with equal bits: no output slot keeps what its buffer held; the API-level tests
run under the `poison` fixture.

Sizes (advmil_concord_rows_plan): the pair pass takes P = 256 cases per tile (one per thread) and 256 controls per LDS tile, and a
workgroup carries W = 8 rows; the per-row walk takes 64 sorted samples per trip. n = 1, 2, P - 1, P, P + 1, 2 P + 3; R = 1, W - 1, W,
W + 1 and one call chunked over several launches."""
import gc
import importlib

import numpy as np
import pytest
import torch

from tests import concord_ref as R
from tests import timedep_ref as TR
from tests.poison import assert_same_bits, poison, three_runs  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
P, W8 = 256, 8
NS = [1, 2, P - 1, P, P + 1, 2 * P + 3]
RS = [1, W8 - 1, W8, W8 + 1]


def _pitched(a, pad, fill):
    """a [rows, c] -> a device view of it inside a block with `pad` more columns holding `fill` (a row pitch > c)."""
    a = np.ascontiguousarray(a)
    wide = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=a.dtype)
    wide[:, :a.shape[1]] = a
    return torch.from_numpy(wide).to(DEV)[:, :a.shape[1]]


def _launch(ev, tm, risk, surv, col, tau, W, pad=0):
    """-> the result tree of one concord_rows call; `pad` > 0 gives every 2-D operand a row pitch and garbage behind each row."""
    from advmil_amd.eval import concord_rows
    n = tm.size
    w = None if W is None else (_pitched(np.asarray(W, dtype=np.int32), pad, 7777) if pad else torch.from_numpy(np.asarray(W, dtype=np.int32)).to(DEV))
    s = None if surv is None else (_pitched(surv, pad + 1, np.float32(np.nan)) if pad else torch.from_numpy(surv).to(DEV))
    r = concord_rows(torch.from_numpy(ev), torch.from_numpy(tm), None if risk is None else torch.from_numpy(risk), s,
                     None if col is None else torch.from_numpy(col), tau, w)
    if pad:                     # what reached the C entry: the pitched views themselves (the pitch of a single row is arbitrary)
        assert W is None or len(W) == 1 or r.ldw == n + pad
        assert n == 1 or surv is None or r.lds == surv.shape[1] + pad + 1
    return dict(counts=r.counts, rowcnt=r.rowcnt, sums=r.sums)


def _compare(got, want, what="", bound=None):
    """got: numpy counts, rowcnt, sums of the kernel; want: concord_ref.rows(...). Integers equal, doubles inside the two bounds."""
    for k in ("counts", "rowcnt"):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (what, k, bad[:5].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    b = 2 * (want["bound"] if bound is None else bound)                        # the kernel's bound and the restatement's
    g, w = got["sums"], want["sums"]
    assert g.dtype == np.float64 and g.shape == w.shape, what
    d = np.abs(g - w)
    print(what, "largest relative deviation of a sum", float((d / np.where(w > 0, w, 1)).max()), "allowed", b)
    assert (d <= b * w).all(), (what, np.argwhere(d > b * w)[:5].tolist(), d.max())


def _exact(ev, tm, risk, surv, col, tau, W, pad=0, what=""):
    """Four runs with equal bits, compared with the restatement -> (numpy results, the restatement's)."""
    runs = three_runs(lambda: _launch(ev, tm, risk, surv, col, tau, W, pad))
    assert_same_bits(runs)
    got = {k: v.cpu().numpy() for k, v in runs[0].items()}
    want = R.rows(ev, tm, risk, surv, col, tau, W, literal=tm.size <= 2)
    _compare(got, want, what)
    return got, want


def _weights(rs, n, rows):
    Wt = R.multiplicities(rs.randint(0, n, size=(rows, n)), n)
    Wt[rs.randint(rows)] += rs.randint(0, 3, size=n).astype(np.int32)         # one row that is no bootstrap draw
    return Wt


@pytest.mark.parametrize("n", NS)
def test_kernel_equals_restatement_around_every_tile_count(n):
    """Per n: a rotating R of 1, W - 1, W, W + 1, Q of 1, 3, T of 1, 8 and an alphabet of 1, 4 or n distinct times; both sources, then
    each alone (its slots keep their bits, the other's are 0), dense and with a row pitch, with weights and without."""
    i = NS.index(n)
    rows, Q, T = RS[i % 4], (1, 3)[i % 2], (8, 1)[i % 2]
    for levels in ((1, 4, 0)[i % 3], (4, 0, 1)[i % 3]):
        rs = np.random.RandomState(1000 * n + levels)
        ev, tm, risk, surv, col = R.cohort(7 * n + levels, n, 0.5, levels, Q=Q)
        tau = R.taus_for(tm, T)
        Wt = _weights(rs, n, rows)
        a, want = _exact(ev, tm, risk, surv, col, tau, Wt, what=f"n {n} levels {levels} both")
        b, _ = _exact(ev, tm, risk, surv, col, tau, Wt, pad=3, what=f"n {n} levels {levels} both, pitched")
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        r_only, _ = _exact(ev, tm, risk, None, None, tau, Wt, pad=(1 if i % 2 else 0), what="risk alone")
        s_only, _ = _exact(ev, tm, None, surv, col, tau, Wt, what="surv alone")
        for one, src in ((r_only, R.RISK), (s_only, R.SURV)):
            assert np.array_equal(one["counts"][:, src], a["counts"][:, src]) and np.array_equal(one["sums"][:, src], a["sums"][:, src])
            assert not one["counts"][:, 1 - src].any() and not one["sums"][:, 1 - src].any()
            assert np.array_equal(one["rowcnt"], a["rowcnt"])
        one, _ = _exact(ev, tm, risk, surv, col, tau, None, what="no weights: one row of ones")
        unit, _ = _exact(ev, tm, risk, surv, col, tau, np.ones((1, n), dtype=np.int32), what="a row of ones")
        for k in one:
            assert np.array_equal(one[k], unit[k]), k
        if n >= P - 1 and levels != 1:                                         # the comparison is not vacuous
            assert (want["counts"][:, :, R.COMP] > n).all() and (want["counts"][:, :, R.CONC] > 0).all()


@pytest.mark.parametrize("rows", RS)
def test_every_row_count_around_a_workgroup(rows):
    n = 70
    ev, tm, risk, surv, col = R.cohort(rows, n, 0.6, 9, Q=3)
    _exact(ev, tm, risk, surv, col, R.taus_for(tm, 8), _weights(np.random.RandomState(rows), n, rows), pad=2, what=f"{rows} rows")


EDGES = ["all_tied", "all_events", "all_censored", "events_only_in_the_last_block", "largest_time_censored",
         "event_tied_with_the_censorings_at_the_end", "zero_weight_on_whole_tie_blocks", "one_sample_left", "tau_on_a_tie_block"]


@pytest.mark.parametrize("kind", EDGES)
def test_tie_and_edge_structures(kind):
    from advmil_amd.eval.concordance import statistics_from_rows
    i = EDGES.index(kind)
    n, rows, Q = 300, 5, 3
    rs = np.random.RandomState(i)
    tied = i % 2 == 1 or kind in ("zero_weight_on_whole_tie_blocks", "tau_on_a_tie_block")
    ev, tm, risk, surv, col = R.cohort(50 + i, n, 0.5, (12 if tied else 0), Q=Q)
    Wt = _weights(rs, n, rows)
    tau = R.taus_for(tm, 8)
    if kind == "all_tied":
        tm[:] = np.float32(2.0)
        tau = np.array([1.0, 2.0, 3.0, np.inf], dtype=np.float32)
    elif kind == "all_events":
        ev[:] = 1
    elif kind == "all_censored":
        ev[:] = 0
    elif kind == "events_only_in_the_last_block":
        ev[:] = 0
        last = np.argsort(tm, kind="stable")[-6:]
        tm[last] = tm.max()
        ev[last] = [1, 0, 1, 0, 0, 1]
    elif kind == "largest_time_censored":
        ev[np.argmax(tm)] = 0
    elif kind == "event_tied_with_the_censorings_at_the_end":
        last = np.argsort(tm, kind="stable")[-4:]
        tm[last] = tm.max()
        ev[last] = [1, 0, 0, 1]
        Wt[:, last] = np.maximum(Wt[:, last], 1)
    elif kind == "zero_weight_on_whole_tie_blocks":
        levels = np.unique(tm)
        Wt[:, np.isin(tm, levels[::3])] = 0
        Wt[1, np.argsort(tm)[:70]] = 0                                         # whole trips of weight zero at the start ...
        Wt[2, np.argsort(tm)[-70:]] = 0                                        # ... and at the end
    elif kind == "one_sample_left":
        Wt[:] = 0
        Wt[0, np.argmax(tm)], Wt[1, np.argmin(tm)], Wt[2, np.argsort(tm)[n // 2]] = 1, 3, 1 << 20
        Wt[3, 5], Wt[4, 6] = 2, 1
    elif kind == "tau_on_a_tie_block":
        u = np.unique(tm)
        assert u.size <= 12
        tau = np.array([u[3], np.nextafter(u[3], np.float32(9)), u[-1], np.inf], dtype=np.float32)
    got, want = _exact(ev, tm, risk, surv, col, tau, Wt, pad=2, what=kind)
    _exact(ev, tm, risk, surv, col, tau, None, what=kind + ", unit weights")
    st = statistics_from_rows(got["counts"], got["rowcnt"], got["sums"])
    ref = R.statistics(want)
    for k in ("c_harrell", "c_td", "c_td_adj", "c_uno", "c_uno_td"):
        assert np.array_equal(np.isnan(getattr(st, k)), np.isnan(ref[k])), (kind, k)
        ok = ~np.isnan(ref[k])
        assert (np.abs(getattr(st, k)[ok] - ref[k][ok]) <= ref["b_" + k][ok]).all(), (kind, k)
    if kind == "all_tied":
        # one block of events and censorings: the censorings are every event's partners, and G = 0 at the only time there is
        assert (got["counts"][..., R.COMP] > 0).all() and not got["sums"].any()
        assert (got["rowcnt"][:, 4:] > 0).all() and not got["rowcnt"][:, 2:4].any() and np.isnan(st.c_uno).all()
    if kind == "all_events":
        assert np.array_equal(got["sums"][:, :, -1, :], got["counts"].astype(np.float64))      # G = 1: tau = +inf gives the counts
    if kind == "all_censored":
        assert not got["counts"].any() and not got["sums"].any() and np.isnan(st.c_uno).all() and np.isnan(st.c_td).all()
    if kind == "events_only_in_the_last_block":
        assert (got["counts"][..., R.COMP] > 0).any()                          # the tied censorings are their only partners
    if kind == "event_tied_with_the_censorings_at_the_end":
        assert (got["rowcnt"][:, -1] > 0).all() and np.isnan(st.c_uno[:, -1]).all() and not np.isnan(st.c_uno[:, 2]).any()
        assert not (got["rowcnt"][:, 2:5] > 0).any()                           # ... and only beyond the last time
    if kind == "one_sample_left":
        assert got["rowcnt"][:, 0].tolist() == [1, 3, 1 << 20, 2, 1] and not got["counts"].any() and np.isnan(st.c_harrell).all()


def test_a_row_of_a_batch_has_the_bits_of_the_one_row_call():
    n, rows = 300, 33
    rs = np.random.RandomState(33)
    ev, tm, risk, surv, col = R.cohort(33, n, 0.5, 40, Q=3)
    tau = R.taus_for(tm, 8)
    Wt = _weights(rs, n, rows)
    batch = _launch(ev, tm, risk, surv, col, tau, Wt, pad=3)
    again = _launch(ev, tm, risk, surv, col, tau, Wt, pad=0)
    assert_same_bits([batch, again], names=("pitched", "dense"))
    for r in (0, 1, 7, 8, 31, 32):
        single = _launch(ev, tm, risk, surv, col, tau, Wt[r:r + 1])
        assert_same_bits([{k: v[r:r + 1] for k, v in batch.items()}, single], names=(f"row {r} of {rows}", "alone"))
    head = _launch(ev, tm, risk, surv, col, tau, Wt[:9])                       # ... nor do they move with R
    assert_same_bits([{k: v[:9] for k, v in batch.items()}, head], names=("first nine of 33", "nine"))
    shuffled = _launch(ev, tm, risk, surv, col, tau, Wt[::-1].copy())          # ... or with the row's place
    assert_same_bits([{k: v.flip(0) for k, v in shuffled.items()}, batch], names=("reversed batch", "batch"))


def test_more_rows_than_one_workspace_go_through_several_launches(monkeypatch):
    from advmil_amd.eval import concord_rows
    n, rows = 100, 21
    ev, tm, risk, surv, col = R.cohort(21, n, 0.5, 10, Q=3)
    Wt = torch.from_numpy(_weights(np.random.RandomState(21), n, rows)).to(DEV)
    args = (torch.from_numpy(ev), torch.from_numpy(tm), torch.from_numpy(risk), torch.from_numpy(surv).to(DEV), torch.from_numpy(col), [0.5, np.inf])
    whole = concord_rows(*args, Wt)
    assert whole.launches == 1
    monkeypatch.setattr(importlib.import_module("advmil_amd.eval.stratify"), "MAX_ROW_BYTES", 8 * (8 * n + 8 * 17))      # 8 rows per launch
    parts = concord_rows(*args, Wt)
    assert parts.launches == 3
    assert_same_bits([dict(c=whole.counts, r=whole.rowcnt, s=whole.sums), dict(c=parts.counts, r=parts.rowcnt, s=parts.sums)], names=("one", "three"))
    _compare({k: getattr(parts, k).cpu().numpy() for k in ("counts", "rowcnt", "sums")},
             R.rows(ev, tm, risk, surv, col, [0.5, np.inf], Wt.cpu().numpy(), literal=False), "chunked")


@pytest.mark.parametrize("n", [40, 200])
def test_a_weighted_row_is_the_unweighted_call_on_the_expanded_cohort(n):
    rs = np.random.RandomState(n)
    ev, tm, risk, surv, col = R.cohort(n, n, 0.5, n // 4, Q=3)
    tau = R.taus_for(tm, 8)
    Wt = _weights(rs, n, 3)
    got = {k: v.cpu().numpy() for k, v in _launch(ev, tm, risk, surv, col, tau, Wt).items()}
    for r in range(3):
        xe, xt, xr, xs, xc = R.expand(Wt[r], ev, tm, risk, surv, col)
        x = {k: v.cpu().numpy() for k, v in _launch(xe, xt, xr, xs, xc, tau, None).items()}
        # either side is within 3 n 2^-52 of the exact value, n its own number of samples
        _compare({k: v[r:r + 1] for k, v in got.items()}, dict(x, bound=None), f"row {r}", bound=R.bound(max(n, xt.size)))


def test_one_captured_graph_replay_equals_the_eager_call():
    """The C entry itself on prepared device arrays: four launches on the capturing stream, no host synchronisation."""
    import ctypes
    from advmil_amd import _lib
    n, rows, Q, T = 300, 9, 3, 8
    ev, tm, risk, surv, col = R.cohort(9, n, 0.5, 30, Q=Q)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)            # noqa: E731
    stime, order = torch.sort(d(tm), stable=True)
    sevent, order = d(ev)[order].contiguous(), order.to(torch.int32)
    Wt, rk, sv, cl, tau = d(_weights(np.random.RandomState(9), n, rows)), d(risk), d(surv), d(col), d(R.taus_for(tm, T))
    L = _lib.lib()
    wsb = L.advmil_concord_rows_workspace_bytes(n, rows, T)
    ws = torch.empty(wsb // 8 + 1, dtype=torch.float64, device=DEV)
    out = [torch.empty((rows, 2, 3), dtype=torch.int64, device=DEV), torch.empty((rows, 2 + T), dtype=torch.int64, device=DEV),
           torch.empty((rows, 2, T, 3), dtype=torch.float64, device=DEV)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                # noqa: E731

    def call():
        stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        _lib.check(L.advmil_concord_rows(p(stime), p(sevent), p(order), n, p(Wt), n, rows, p(rk), p(sv), Q, Q, p(cl), p(tau), T, p(out[0]),
                                         p(out[1]), p(out[2]), p(ws), wsb, stream), "concord_rows")
    call()
    torch.cuda.synchronize()
    eager = [o.clone() for o in out]
    _compare(dict(counts=eager[0].cpu().numpy(), rowcnt=eager[1].cpu().numpy(), sums=eager[2].cpu().numpy()),
             R.rows(ev, tm, risk, surv, col, R.taus_for(tm, T), Wt.cpu().numpy(), literal=False), "the C entry")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                call()
    finally:
        gc.enable()
    for o in out:
        o.view(torch.uint8).fill_(0x7F)
    ws.view(torch.uint8).fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits([eager, [o.clone() for o in out]], names=("eager", "replay"))


# ---- API level --------------------------------------------------------------------------------------------------------------------------
N_API, B_API = 200, 60


@pytest.fixture(scope="module")
def api():
    """n = 200, about half censored, times rounded to 1 / 64 (ties); the restatement's rows of the cohort and of 60 resamples, once."""
    a = TR.api_cohort(N_API, 0)
    tm, ev = a["y"][:, 0].copy(), a["y"][:, 1].copy()
    at = np.unique(tm[ev != 0])
    col = R.own_columns(tm, at).astype(np.int32)
    surv = TR.survival_from_samples(a["dist"], at)
    risk = -a["dist"].mean(axis=1).astype(np.float32)
    tau = np.array([np.quantile(tm, 0.7), np.inf], dtype=np.float32)
    idx = np.random.RandomState(3).randint(0, N_API, size=(B_API, N_API))
    Wt = np.concatenate([np.ones((1, N_API), dtype=np.int32), R.multiplicities(idx, N_API)])
    want = R.rows(ev, tm, risk, surv, col, tau, Wt, literal=False)
    return dict(a, tm=tm, ev=ev, at=at, col=col, surv=surv, risk=risk, tau=tau, idx=idx, W=Wt, want=want, st=R.statistics(want))


def test_functions_are_the_restatements(api, poison):
    from advmil_amd.eval import concordance_ipcw, concordance_td, surv_at_own_times
    ev, tm, st, want = api["ev"], api["tm"], api["st"], api["want"]
    at, col, surv = surv_at_own_times(ev, tm, dist_y_hat=torch.from_numpy(api["dist"]), chunk=7)
    assert np.array_equal(at, api["at"]) and np.array_equal(col, api["col"]) and surv.is_cuda and np.array_equal(surv.cpu().numpy(), api["surv"])
    # (16 samples per patient: many survival ties, which Antolini's plain form counts as not concordant)
    assert 20 < at.size < N_API and 0.5 < st["c_uno"][0, 1] < 1 and 0 < st["c_td"][0] < st["c_td_adj"][0] < 1 and st["c_td_adj"][0] > 0.5
    u = concordance_ipcw(ev, tm, api["risk"], api["tau"])
    assert np.array_equal(u.counts, want["counts"][0, R.RISK]) and not u.n_zero_g.any()
    assert (np.abs(u.c_uno - st["c_uno"][0]) <= st["b_c_uno"][0]).all() and abs(u.c_harrell - st["c_harrell"][0]) <= st["b_c_harrell"][0]
    assert concordance_ipcw(ev, tm, api["risk"]).c_uno[0] == u.c_uno[1]                     # tau None: no truncation
    td = concordance_td(ev, tm, surv, at)
    adj = concordance_td(ev, tm, surv, at, method="adj_antolini")
    assert np.array_equal(td.counts, want["counts"][0, R.SURV]) and want["counts"][0, R.SURV, R.TIED] > 0
    assert abs(td.c_td - st["c_td"][0]) <= st["b_c_td"][0] and abs(adj.c_td - st["c_td_adj"][0]) <= st["b_c_td_adj"][0]
    hz = torch.from_numpy(api["hazards"])
    lab, evd = api["yd"][:, 0], api["yd"][:, 1]
    at_d, col_d, surv_d = surv_at_own_times(evd, lab, hazards=hz)
    want_s = np.cumprod(1 - api["hazards"].astype(np.float32), axis=1)[:, at_d.astype(np.int64)]
    assert at_d.tolist() == sorted(set(lab[evd != 0].tolist())) and np.allclose(surv_d.cpu().numpy(), want_s, rtol=1e-6)
    assert np.array_equal(col_d, R.own_columns(lab, at_d))


def test_bootstrap_from_given_indices(api, poison):
    from advmil_amd.eval import bootstrap_concordance, concord_rows
    from advmil_amd.eval.concordance import statistics_from_rows
    ev, tm, st, level = api["ev"], api["tm"], api["st"], 0.9
    names = ("c_uno", "c_harrell", "c_td", "c_td_adj", "c_uno_td")
    assert not any(np.isnan(st[k]).any() for k in names)                       # the ORACLE's undefined share is 0
    b = bootstrap_concordance(ev, tm, api["risk"], api["surv"], api["col"], api["tau"], indices=api["idx"], level=level)
    assert b.launches == 1 and b.c_uno_samples.shape == (B_API, 2) and b.c_td_samples.shape == (B_API,)
    assert np.array_equal(b.counts, api["want"]["counts"][0]) and b.n_undefined == {k: 0 for k in names}
    point = concord_rows(ev, tm, api["risk"], api["surv"], api["col"], api["tau"])          # the point row is the unweighted call
    ps = statistics_from_rows(point.counts, point.rowcnt, point.sums)
    pct = [50 * (1 - level), 50 * (1 + level)]
    for k in names:
        assert np.array_equal(np.asarray(getattr(b, k)), getattr(ps, k)[0]), k
        tol = st["b_" + k]
        assert (np.abs(getattr(b, k) - st[k][0]) <= tol[0]).all(), k
        samples = getattr(b, k + "_samples")
        assert (np.abs(samples - st[k][1:]) <= tol[1:]).all(), k
        lo, hi = np.nanpercentile(samples, pct, axis=0)
        assert np.array_equal(getattr(b, k + "_lo"), lo) and np.array_equal(getattr(b, k + "_hi"), hi) and (lo <= hi).all(), k
    seeded = bootstrap_concordance(ev, tm, api["risk"], api["surv"], api["col"], api["tau"], n_boot=B_API, seed=3, level=level)
    assert np.array_equal(seeded.c_uno_samples, b.c_uno_samples) and seeded.c_td_lo == b.c_td_lo


@pytest.mark.parametrize("kind", ["continuous", "hazards", "cox"])
def test_evaluators(api, kind, poison):
    from advmil_amd.eval import (ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator, bootstrap_concordance, concordance_ipcw,
                                 concordance_td, surv_at_own_times)
    y = torch.from_numpy(api["y"])
    names = ("c_uno", "c_harrell", "c_td", "c_td_adj", "c_uno_td")
    if kind == "continuous":
        dist = torch.from_numpy(api["dist"]).reshape(N_API, -1, 1)
        evl, data = ContSurv_Evaluator(end_time=1.0), {"y": y, "y_hat": dist.median(dim=1).values, "dist_y_hat": dist}
        ev, tm = api["ev"], api["tm"]
        at, col, surv = surv_at_own_times(ev, tm, dist_y_hat=torch.from_numpy(api["dist"]))
    elif kind == "hazards":
        yd, hz = torch.from_numpy(api["yd"]), torch.from_numpy(api["hazards"])
        evl, data = DiscSurv_Evaluator(), {"y": yd, "y_hat": hz[torch.randperm(N_API)], "avg_y_hat": hz}      # avg_y_hat is preferred
        ev, tm = api["yd"][:, 1], api["yd"][:, 0]
        at, col, surv = surv_at_own_times(ev, tm, hazards=hz)
    else:
        pred = torch.from_numpy(api["dist"]).mean(dim=1, keepdim=True)
        evl, data = CoxSurv_Evaluator(), {"y": y, "y_hat": pred}
        ev, tm = api["ev"], api["tm"]
        at = col = surv = None
        names = names[:2]
    risk = evl._risk_estimate(data)[2]                                         # the risk the c_index metric ranks by
    # (bins: the last one holds events and censorings, so G = 0 there and only a truncated Uno's C is defined)
    tau = [2.0, 3.0] if kind == "hazards" else [float(np.quantile(tm, 0.7)), float("inf")]
    d = evl.concordance(data, tau=tau)
    assert set(d) == {"tau", *names}
    u = concordance_ipcw(ev, tm, risk, tau)
    assert np.array_equal(d["c_uno"], u.c_uno) and d["c_harrell"] == u.c_harrell and not np.isnan(u.c_uno).any()
    if surv is not None:
        assert d["c_td"] == concordance_td(ev, tm, surv, at).c_td and d["c_td_adj"] == concordance_td(ev, tm, surv, at, "adj_antolini").c_td
        assert 0 < d["c_td"] <= d["c_td_adj"] < 1
    # ... and the restatement on the same arrays
    st = R.statistics(R.rows(ev, tm, risk.cpu().numpy(), None if surv is None else surv.cpu().numpy(), col, tau, literal=False),
                      has_surv=surv is not None)
    for k in names:
        assert (np.abs(d[k] - st[k][0]) <= st["b_" + k][0]).all(), (kind, k)
    db = evl.concordance(data, tau=tau, n_boot=40, seed=5)
    assert set(db) == {"tau", "n_undefined", *names, *(k + s for k in names for s in ("_lo", "_hi"))}
    b = bootstrap_concordance(ev, tm, risk, surv, col, tau, n_boot=40, seed=5)
    for k in names:
        assert np.array_equal(db[k], d[k]) and np.array_equal(db[k + "_lo"], getattr(b, k + "_lo")), (kind, k)
        assert np.array_equal(db[k + "_hi"], getattr(b, k + "_hi")) and db["n_undefined"][k] == b.n_undefined[k] == 0, (kind, k)


def test_cap_on_undefined_resamples(poison):
    """tests/test_concord_cpu.py shows by the restatement alone that the undefined share of this cohort lies between 5 % and 60 %."""
    from advmil_amd.eval import bootstrap_concordance
    c = R.cap_cohort()
    st = R.statistics(R.rows(c["ev"], c["tm"], c["risk"], W=R.multiplicities(c["idx"], 5)), has_surv=False)
    n_uno, n_har = int(np.isnan(st["c_uno"][:, 0]).sum()), int(np.isnan(st["c_harrell"]).sum())
    assert n_uno >= n_har > 0.05 * len(c["idx"])
    with pytest.raises(ValueError, match="resamples"):
        bootstrap_concordance(c["ev"], c["tm"], c["risk"], indices=c["idx"])
    r = bootstrap_concordance(c["ev"], c["tm"], c["risk"], indices=c["idx"], max_undefined=0.6)
    assert r.n_undefined == {"c_uno": n_uno, "c_harrell": n_har}
    assert np.array_equal(np.isnan(r.c_uno_samples[:, 0]), np.isnan(st["c_uno"][:, 0])) and r.c_harrell == 1.0
    ok = ~np.isnan(st["c_uno"][:, 0])
    assert (np.abs(r.c_uno_samples[ok, 0] - st["c_uno"][ok, 0]) <= st["b_c_uno"][ok, 0]).all()
