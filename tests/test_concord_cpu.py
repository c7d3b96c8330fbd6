"""CPU: Uno's C and Antolini's concordance without a device. The two restatements of tests/concord_ref.py (naive float64 over the expanded
row; exact rationals over the weighted row) against each other on an enumerated family and against cohorts worked by hand; the
invariants both must keep; the host side of the product (advmil_amd/eval/concordance.py); and the negative paths of advmil_concord_rows
(include/advmil_hip.h), which answer before anything is enqueued and so need no device."""
import ctypes
import itertools
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest
import torch

from tests import concord_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -2
A16 = 0x7F0000001000          # a fake, 16-byte aligned "device address": never dereferenced when validation does its job
INF = float("inf")


def _agree(a, x, what):
    """a: concord_ref.row(...), x: concord_ref.row_exact(...) of the same row: integers equal, doubles within the bound of the rational."""
    assert a["counts"].tolist() == x["counts"] and a["rowcnt"].tolist() == x["rowcnt"], what
    for s in (R.RISK, R.SURV):
        for t in range(len(x["sums"][s])):
            for k in range(3):
                want = float(x["sums"][s][t][k])
                assert abs(a["sums"][s, t, k] - want) <= a["bound"] * want, (what, s, t, k)
    st = R.statistics({k: np.asarray(a[k])[None] for k in ("counts", "rowcnt", "sums")} | {"bound": a["bound"]})
    for k in ("c_harrell", "c_td", "c_td_adj"):
        assert np.isnan(st[k][0]) == (x[k] is None), (what, k)
        if x[k] is not None:
            assert abs(st[k][0] - float(x[k])) <= 2 * R.U52, (what, k)
    for k in ("c_uno", "c_uno_td"):
        for t, v in enumerate(x[k]):
            assert np.isnan(st[k][0, t]) == (v is None), (what, k, t)
            if v is not None:
                assert abs(st[k][0, t] - float(v)) <= 3 * a["bound"] * float(v) + 2 * R.U52, (what, k, t)


# ---- the two restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_float64_restatement_equals_the_rational_one_on_every_small_cohort(n):
    """Times from the alphabet {1, 2, 3} (ascending: the order of the samples is the subject of another test), every event pattern;
    risks and survival columns from a four-value alphabet so that they tie, weights 0 ... 2, tau below, between, at and beyond."""
    tau = [0.5, 1.5, 2.0, 3.0, INF]
    seen = 0
    for times in itertools.combinations_with_replacement([1.0, 2.0, 3.0], n):
        for ev in itertools.product([0.0, 1.0], repeat=n):
            rs = np.random.RandomState(seen)
            risk = (rs.randint(0, 4, size=n) / 4).astype(np.float32)
            surv = (rs.randint(0, 4, size=(n, 3)) / 4).astype(np.float32)
            col = R.own_columns(times, [1.0, 2.0, 3.0])
            w = rs.randint(0, 3, size=n) if seen % 2 else None
            a = R.row(ev, times, risk, surv, col, tau, w)
            x = R.row_exact(ev, times, risk, surv, col, tau, w)
            _agree(a, x, (times, ev, seen))
            seen += 1
    assert seen == len(list(itertools.combinations_with_replacement(range(3), n))) * 2 ** n


def test_five_samples_with_an_event_tied_with_a_censoring():
    """y = 1 2 2 3 4, e = 1 1 0 0 1. G (events before censorings): 1 at 1, (4 - 1 - 1) / (4 - 1) = 2/3 at 2, 1/3 at 3 and 4.
    Cases: 0 (comparable with 1 2 3 4), 1 (with 2: tied and censored, 3, 4), 4 (with nobody): comp = 4 + 3 + 0 = 7.
    risk = 3 1 2 1 0: case 0 is worse than all four; case 1 is not worse than 2, ties 3, is worse than 4: conc 5, tied 1.
      Harrell (5 + 1/2) / 7 = 11/14. Uno without truncation, weights 1, 9/4, 9: conc 4 + 9/4 = 25/4, tied 9/4, comp 4 + 27/4 = 43/4:
      (25/4 + 9/8) / (43/4) = 59/86. tau = 2: case 0 alone, 4 of 4: 1. tau = 1: no case: undefined.
    surv on the grid 1 2 4, columns 0 1 1 1 2: case 0 reads column 0 = .25 | .875 .25 .5 .125: conc 2 (1, 3), tied 1 (2); case 1 reads
      column 1 = .5 | .5 .75 .5: conc 1 (3), tied 2 (2, 4): conc 3, tied 3, comp 7: C_td 3/7, adjusted 9/14; with Uno's weights
      conc 2 + 9/4 = 17/4, tied 1 + 9/2 = 11/2: (17/4 + 11/4) / (43/4) = 28/43."""
    y, e = [1, 2, 2, 3, 4], [1, 1, 0, 0, 1]
    risk = [3, 1, 2, 1, 0]
    surv = np.full((5, 3), 0.5, dtype=np.float32)
    surv[:, 0] = [.25, .875, .25, .5, .125]
    surv[3, 1] = .75
    col = R.own_columns(y, [1, 2, 4])
    assert col.tolist() == [0, 1, 1, 1, 2]
    tau = [INF, 2.0, 1.0]
    x = R.row_exact(e, y, risk, surv, col, tau)
    assert x["G"] == [F(1), F(2, 3), F(2, 3), F(1, 3), F(1, 3)]
    assert x["counts"] == [[5, 1, 7], [3, 3, 7]] and x["rowcnt"] == [5, 3, 0, 0, 0]
    assert x["sums"][R.RISK][0] == [F(25, 4), F(9, 4), F(43, 4)] and x["sums"][R.SURV][0] == [F(17, 4), F(11, 2), F(43, 4)]
    assert x["sums"][R.RISK][1] == [F(4), F(0), F(4)] and x["sums"][R.RISK][2] == [F(0)] * 3
    assert (x["c_harrell"], x["c_td"], x["c_td_adj"]) == (F(11, 14), F(3, 7), F(9, 14))
    assert x["c_uno"] == [F(59, 86), F(1), None] and x["c_uno_td"][0] == F(28, 43)
    _agree(R.row(e, y, risk, surv, col, tau), x, "by hand")


def test_an_event_tied_with_the_censoring_that_ends_the_row_is_flagged():
    """y = 1 2 2, e = 1 1 0: at 2 one of two at risk has the event, the other is censored: G(2) = (2 - 1 - 1) / (2 - 1) = 0. Case 1
    (comparable with 2) cannot be weighted: Uno's C is undefined for every tau beyond 2, and 0/2 for tau = 2 (case 0, risk 1 < 2, 3)."""
    y, e, risk = [1, 2, 2], [1, 1, 0], [1, 2, 3]
    x = R.row_exact(e, y, risk, tau=[2.0, 2.5, INF])
    assert x["G"] == [F(1), F(0), F(0)] and x["rowcnt"] == [3, 2, 0, 1, 1] and x["counts"][R.RISK] == [0, 0, 3]
    assert x["c_uno"] == [F(0), None, None] and x["c_harrell"] == F(0) and x["sums"][R.RISK][2] == [F(0), F(0), F(2)]
    _agree(R.row(e, y, risk, tau=[2.0, 2.5, INF]), x, "G = 0")


def test_two_weighted_samples():
    """y = 1 2, e = 1 0, w = 2 3, risk = 1 0: each of the two copies of the case is worse than three controls: 6 of 6; G(1) = 1."""
    x = R.row_exact([1, 0], [1, 2], [1, 0], w=[2, 3])
    assert x["counts"][R.RISK] == [6, 0, 6] and x["sums"][R.RISK][0] == [F(6), F(0), F(6)] and x["c_uno"] == [F(1)] and x["rowcnt"] == [5, 2, 0]
    _agree(R.row([1, 0], [1, 2], [1, 0], w=[2, 3]), x, "weighted")


@pytest.mark.parametrize("seed,n,levels", [(1, 30, 0), (2, 41, 5), (3, 64, 1)])
def test_the_vectorised_inner_loop_is_the_literal_one(seed, n, levels):
    ev, tm, risk, surv, col = R.cohort(seed, n, 0.6, levels, Q=4)
    w = np.random.RandomState(seed).randint(0, 3, size=n)
    a, b = R.row(ev, tm, risk, surv, col, R.taus_for(tm, 8), w, literal=True), R.row(ev, tm, risk, surv, col, R.taus_for(tm, 8), w, literal=False)
    for k in ("counts", "rowcnt", "sums"):
        assert np.array_equal(a[k], b[k]), k


# ---- invariants -------------------------------------------------------------------------------------------------------------------------
def test_without_censoring_unos_c_is_the_ratio_of_the_counts():
    ev, tm, risk, surv, col = R.cohort(7, 40, 1.0, 9, Q=3)
    a = R.row(ev, tm, risk, surv, col)
    assert (a["G"] == 1.0).all() and a["rowcnt"].tolist() == [40, 40, 0]
    assert np.array_equal(a["sums"][:, 0, :], a["counts"].astype(np.float64))
    st = R.statistics({k: a[k][None] for k in ("counts", "rowcnt", "sums")} | {"bound": a["bound"]})
    c = a["counts"][R.RISK]
    assert st["c_uno"][0, 0] == (c[0] + 0.5 * c[1]) / c[2] == st["c_harrell"][0]


def test_a_survival_matrix_that_decreases_in_one_risk_gives_the_risks_counts():
    ev, tm, risk, _, col = R.cohort(8, 50, 0.5, 7, Q=5)
    scale = np.array([1, 2, 4, 8, 16], dtype=np.float32)                          # exact products: ties of the risk stay ties in every column
    surv = (-risk[:, None] * scale[None, :]).astype(np.float32)
    a = R.row(ev, tm, risk, surv, col, R.taus_for(tm, 8))
    assert a["counts"][R.RISK].tolist() == a["counts"][R.SURV].tolist() and a["counts"][R.RISK, R.TIED] > 0
    assert np.array_equal(a["sums"][R.RISK], a["sums"][R.SURV])


@pytest.mark.parametrize("n,levels", [(12, 0), (30, 4)])
def test_a_weighted_row_is_the_expanded_cohort(n, levels):
    ev, tm, risk, surv, col = R.cohort(n, n, 0.5, levels, Q=3)
    w = R.multiplicities(np.random.RandomState(n).randint(0, n, size=(1, n)), n)[0]
    tau = R.taus_for(tm, 8)
    a = R.row(ev, tm, risk, surv, col, tau, w)
    xe, xt, xr, xs, xc = R.expand(w, ev, tm, risk, surv, col)
    b = R.row(xe, xt, xr, xs, xc, tau)
    for k in ("counts", "rowcnt", "sums"):
        assert np.array_equal(a[k], b[k]), k


def test_the_order_of_the_samples_changes_nothing():
    ev, tm, risk, surv, col = R.cohort(5, 35, 0.5, 6, Q=3)
    tau = R.taus_for(tm, 8)
    a = R.row(ev, tm, risk, surv, col, tau)
    p = np.random.RandomState(5).permutation(35)
    b = R.row(ev[p], tm[p], risk[p], surv[p], col[p], tau)
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["rowcnt"], b["rowcnt"])
    assert (np.abs(a["sums"] - b["sums"]) <= 2 * R.U52 * a["sums"]).all()          # (fsum: the order of the terms cannot show)


def test_cap_cohort_has_an_undefined_share_between_the_two_caps():
    """The cohort of the GPU test of `max_undefined`: by the float64 restatement alone, more than 5 % and less than 60 % of its
    resamples have no defined Uno's C (a resample without a comparable pair, or with an event tied with the censoring that ends it)."""
    c = R.cap_cohort()
    st = R.statistics(R.rows(c["ev"], c["tm"], c["risk"], W=R.multiplicities(c["idx"], c["tm"].size)), has_surv=False)
    share = np.isnan(st["c_uno"][:, 0]).mean()
    assert 0.05 < share < 0.6, share
    assert 0.05 < np.isnan(st["c_harrell"]).mean() <= share


# ---- the host side of the product -------------------------------------------------------------------------------------------------------
def test_statistics_from_rows_is_the_restatements():
    from advmil_amd.eval.concordance import statistics_from_rows
    ev, tm, risk, surv, col = R.cohort(4, 40, 0.5, 6, Q=4)
    ev[np.argsort(tm, kind="stable")[-3:]] = [1, 0, 0]                            # ... whose last tie block may give G = 0
    tm[np.argsort(tm, kind="stable")[-3:]] = tm.max()
    W = R.multiplicities(np.random.RandomState(4).randint(0, 40, size=(12, 40)), 40)
    res = R.rows(ev, tm, risk, surv, col, R.taus_for(tm, 8), W, literal=False)
    want = R.statistics(res)
    got = statistics_from_rows(res["counts"], res["rowcnt"], res["sums"])
    for k in ("c_harrell", "c_td", "c_td_adj", "c_uno", "c_uno_td"):
        assert np.array_equal(np.isnan(getattr(got, k)), np.isnan(want[k])), k
        assert np.allclose(getattr(got, k), want[k], rtol=1e-15, atol=0, equal_nan=True), k
    assert np.isnan(want["c_uno"]).any() and not np.isnan(want["c_uno"]).all()
    only = statistics_from_rows(res["counts"], res["rowcnt"], res["sums"], has_risk=True, has_surv=False)
    assert np.isnan(only.c_td).all() and np.isnan(only.c_uno_td).all() and np.array_equal(only.c_harrell, got.c_harrell)


def test_columns_at_own_times_is_the_post_step_lookup():
    from advmil_amd.eval import columns_at_own_times
    assert columns_at_own_times([0.5, 1, 1.5, 2, 9], [1, 2, 4]).tolist() == [0, 0, 0, 1, 2]
    with pytest.raises(ValueError, match="ascend"):
        columns_at_own_times([1.0], [2, 1])


def test_wrappers_validate_and_refuse_without_a_device(monkeypatch):
    from advmil_amd.eval import (ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator, bootstrap_concordance, concord_rows,
                                 concordance_ipcw, concordance_td, surv_at_own_times)
    ev, tm, risk, surv, col = (torch.from_numpy(a) for a in R.cohort(1, 17, 0.5, 6, Q=3))
    ev[0] = 1
    W = torch.ones(4, 17, dtype=torch.int32)
    with pytest.raises(ValueError, match="neither"):
        concord_rows(ev, tm)
    with pytest.raises(ValueError, match="inconsistent"):
        concord_rows(ev[:5], tm, risk)
    with pytest.raises(ValueError, match="inconsistent"):
        concord_rows(ev, tm, risk[:16])
    with pytest.raises(ValueError, match="inconsistent"):
        concord_rows(ev, tm, surv=surv[:16], col=col)
    with pytest.raises(ValueError, match="inconsistent"):
        concord_rows(ev, tm, surv=surv, col=col[:16])
    with pytest.raises(ValueError, match="inconsistent"):
        concord_rows(ev, tm, risk, weights=W[:, :9])
    with pytest.raises(ValueError, match="needs col"):
        concord_rows(ev, tm, surv=surv)
    with pytest.raises(ValueError, match="integer column"):
        concord_rows(ev, tm, surv=surv, col=col.to(torch.float32))
    for bad_value in (-1, 3):
        bad = col.clone()
        bad[0] = bad_value                                                             # sample 0 has an observed event
        with pytest.raises(ValueError, match="col: sample 0"):
            concord_rows(ev, tm, surv=surv, col=bad)
    with pytest.raises(ValueError, match="int32"):
        concord_rows(ev, tm, risk, weights=W.to(torch.int64))
    neg = W.clone()
    neg[2, 3] = -1
    with pytest.raises(ValueError, match="negative"):
        concord_rows(ev, tm, risk, weights=neg)
    big = W.clone()
    big[1, :] = (1 << 31) // 17 + 1
    with pytest.raises(ValueError, match="2\\^31"):
        concord_rows(ev, tm, risk, weights=big)
    for name, bad in (("time", tm), ("surv", surv), ("risk", risk)):
        bad = bad.clone()
        bad.reshape(-1)[3] = float("nan")
        with pytest.raises(ValueError, match=name + ": NaN"):
            concord_rows(ev, bad if name == "time" else tm, risk=bad if name == "risk" else risk, surv=bad if name == "surv" else surv, col=col)
    with pytest.raises(ValueError, match="tau: NaN"):
        concord_rows(ev, tm, risk, tau=[1.0, float("nan")])
    with pytest.raises(ValueError, match="truncation times"):
        concord_rows(ev, tm, risk, tau=np.arange(9.0))
    with pytest.raises(ValueError, match="truncation times"):
        concord_rows(ev, tm, risk, tau=[])
    with pytest.raises(ValueError, match="surv: 4097 columns"):
        concord_rows(ev, tm, surv=torch.zeros(17, 4097), col=col)
    with pytest.raises(ValueError, match="2\\^16"):
        concord_rows(torch.zeros((1 << 16) + 1), torch.zeros((1 << 16) + 1), torch.zeros((1 << 16) + 1))
    with pytest.raises(ValueError, match="method"):
        concordance_td(ev, tm, surv, [0.1, 0.2, 0.3], method="harrell")
    with pytest.raises(ValueError, match="one column per grid time"):
        concordance_td(ev, tm, surv, [0.1, 0.2])
    many = torch.arange(4097, dtype=torch.float32)
    with pytest.raises(ValueError, match="4097 distinct event times"):
        surv_at_own_times(torch.ones(4097), many, dist_y_hat=torch.zeros(4097, 2))
    with pytest.raises(ValueError, match="no observed event"):
        surv_at_own_times(0 * ev, tm, dist_y_hat=surv)
    with pytest.raises(ValueError, match="exactly one"):
        surv_at_own_times(ev, tm)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    y = torch.stack([tm, ev], dim=1)
    for fn in (lambda: concord_rows(ev, tm, risk), lambda: concord_rows(ev, tm, risk, surv, col, [0.5], W),
               lambda: concordance_ipcw(ev, tm, risk), lambda: concordance_td(ev, tm, surv, [0.1, 0.2, 0.3]),
               lambda: bootstrap_concordance(ev, tm, risk, n_boot=5), lambda: surv_at_own_times(ev, tm, dist_y_hat=surv)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    for evl, data in ((ContSurv_Evaluator(end_time=1.0), {"y": y, "y_hat": tm.reshape(-1, 1), "dist_y_hat": surv.reshape(17, 3, 1)}),
                      (DiscSurv_Evaluator(), {"y": y, "y_hat": surv}), (CoxSurv_Evaluator(), {"y": y, "y_hat": tm.reshape(-1, 1)})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evl.concordance(data)


# ---- the C entry without a device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib


def _p(k, off=0):
    return ctypes.c_void_p(A16 + (k << 28) + off)


GOOD = dict(stime=_p(0), sevent=_p(1), order=_p(2), n=64, weights=_p(3), ldw=64, R=8, risk=_p(4), surv=_p(5), lds=16, Q=16, col=_p(6),
            tau=_p(7), T=2, counts=_p(8), rowcnt=_p(9), sums=_p(10), ws=_p(11), ws_bytes=8 * 64 * 8 + 8 * 1 * 17 * 8 + 64 * 4)
NAMES = list(GOOD)


def _call(L, **kw):
    a = dict(GOOD, **kw)
    return L.lib().advmil_concord_rows(*(a[k] for k in NAMES), None)


def test_symbols_are_declared_bound_and_exported(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "advmil_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(advmil_[a-z0-9_]+)\s*\(", hdr))
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in ("advmil_concord_rows", "advmil_concord_rows_workspace_bytes", "advmil_concord_rows_plan"):
        assert name in declared and name in L.SIGNATURES and hasattr(handle, name), name
    assert len(L.SIGNATURES["advmil_concord_rows"][1]) == len(NAMES) + 1


def test_workspace_query_and_plan_are_pure_host_functions(L):
    f = L.lib().advmil_concord_rows_workspace_bytes
    assert f(64, 8, 2) == GOOD["ws_bytes"] and f(1, 1, 1) == 8 + 11 * 8 + 8
    assert f(257, 3, 8) == 3 * 257 * 8 + 3 * 2 * 53 * 8 + 258 * 4                      # two tiles; n odd: rounded up to 8 bytes
    assert f(1 << 16, 1 << 20, 8) == (1 << 39) + (1 << 28) * 53 * 8 + (1 << 18)
    assert f(0, 1, 1) == 0 and f((1 << 16) + 1, 1, 1) == 0 and f(5, 0, 1) == 0 and f(5, (1 << 20) + 1, 1) == 0
    assert f(5, 1, 0) == 0 and f(5, 1, 9) == 0
    v = [ctypes.c_int(0) for _ in range(4)]
    assert L.lib().advmil_concord_rows_plan(*(ctypes.byref(x) for x in v)) == 0
    assert [x.value for x in v] == [4, 64, 256, 8]                                     # the sizes tests/test_concord_gpu.py straddles
    from advmil_amd.eval import concordance as C
    assert v[2].value == C.PAIR_TILE
    assert L.lib().advmil_concord_rows_plan(ctypes.byref(v[0]), None, ctypes.byref(v[2]), ctypes.byref(v[3])) == EINVAL


def test_every_null_pointer_is_refused(L):
    for name in ("stime", "sevent", "order", "tau", "counts", "rowcnt", "sums", "ws"):
        assert _call(L, **{name: None}) == EINVAL, name
    assert _call(L, col=None) == EINVAL                                                # surv without its columns
    assert _call(L, risk=None, surv=None) == EINVAL                                    # no source at all


def test_what_may_be_absent_is_refused_for_the_next_reason_only(L):
    """weights NULL means all ones; one of risk and surv may be NULL (without surv neither col, lds nor Q is looked at): such a call
    passes validation -- shown by making it fail on the workspace, the last check, since a valid call would launch."""
    assert _call(L, weights=None, ldw=0, ws_bytes=GOOD["ws_bytes"] - 1) == EWORKSPACE
    assert _call(L, surv=None, col=None, lds=0, Q=0, ws_bytes=0) == EWORKSPACE
    assert _call(L, risk=None, ws_bytes=0) == EWORKSPACE
    assert _call(L, weights=None, risk=None, n=0) == EINVAL


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=-1), dict(n=(1 << 16) + 1, ldw=1 << 17, ws_bytes=1 << 40), dict(R=0), dict(R=-3),
                                dict(R=(1 << 20) + 1, ws_bytes=1 << 40), dict(T=0), dict(T=-1), dict(T=9, ws_bytes=1 << 40), dict(Q=0),
                                dict(Q=-1), dict(Q=4097, lds=4097), dict(ldw=63), dict(ldw=0), dict(ldw=-64), dict(lds=15), dict(lds=0)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_out_of_range_shapes(L, kw):
    assert _call(L, **kw) == EINVAL


@pytest.mark.parametrize("kw", [dict(n=1 << 16, ldw=1 << 16), dict(R=1 << 20), dict(T=8), dict(T=1), dict(Q=4096, lds=4096), dict(Q=1),
                                dict(n=1, R=1)], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_the_limits_themselves_pass_validation(L, kw):
    assert _call(L, ws_bytes=0, **kw) == EWORKSPACE


@pytest.mark.parametrize("name,off", [("stime", 2), ("sevent", 1), ("order", 2), ("weights", 2), ("risk", 1), ("surv", 2), ("col", 2),
                                      ("tau", 1), ("counts", 4), ("rowcnt", 4), ("sums", 4), ("ws", 4)])
def test_misaligned_pointers(L, name, off):
    k = [n for n in NAMES if isinstance(GOOD[n], ctypes.c_void_p)].index(name)
    assert _call(L, **{name: _p(k, off)}) == EINVAL
    assert _call(L, **{name: _p(k, 16), "ws_bytes": 0}) == EWORKSPACE                 # (aligned elsewhere: validation goes on to the workspace)


def test_workspace_too_small(L):
    need = L.lib().advmil_concord_rows_workspace_bytes(64, 8, 2)
    assert _call(L, ws_bytes=need - 1) == EWORKSPACE and _call(L, ws_bytes=0) == EWORKSPACE
    assert _call(L, ws_bytes=need - 1, n=0) == EINVAL                                 # the argument checks come first
