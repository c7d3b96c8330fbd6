"""CPU: the two restatements of advmil_calib_rows (tests/calib_ref.py) against each other and against cohorts worked by hand, the host
side of advmil_amd/eval/calibration.py (statistics, the chi-square tail, validation), and the C entry's argument checks, which return
before anything is enqueued and so need no device."""
import ctypes
import itertools
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import calib_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -2
A16 = 0x7F0000001000          # a fake, 16-byte aligned "device address": never dereferenced when validation does its job
U52 = R.U52


def _close(a, x, b, what):
    """a: the float64 restatement's number, x: the exact one, b: the former's absolute bound (plus one rounding of float(x))."""
    xf = float(x)
    assert abs(a - xf) <= b + U52 * abs(xf), (what, a, xf, abs(a - xf), b)


def _agree(ev, tm, pred, p, bins, gamma, w, what):
    a = R.row(ev, tm, pred, p, bins, gamma, w)
    x = R.row_exact(ev, tm, pred, p, bins, gamma, w, literal=True)        # (asserts block form == deletion, in exact rationals)
    assert a["rowcnt"].tolist() == x["rowcnt"], (what, a["rowcnt"], x["rowcnt"])
    for j in range(3):
        _close(a["km"][j], x["km"][j], a["b_km"][j], (what, "km", j))
    for c in range(a["err"].shape[0]):
        for j in range(3):
            for k in range(2):
                _close(a["err"][c, j, k], x["err"][c][j][k], a["b_err"][c, j, k], (what, "err", c, j, k))
    for j in range(bins):
        _close(a["dcal"][j], x["dcal"][j], a["b_dcal"], (what, "dcal", j))
    assert sum(x["dcal"], Fraction(0)) == x["rowcnt"][0], what                 # the masses sum to N, exactly
    return a, x


# ---- the two restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7])
def test_float64_restatement_equals_the_rational_one_on_every_event_pattern(n):
    """Times from {1, 2, 3, 4} (ties abound), EVERY event pattern (all-censored and all-events among them), weights 0 ... 2 (zeros
    remove whole times, the largest included), predictions below and beyond the times, p_own with 0, 1 and bin edges; once per n with
    everything tied."""
    rs = np.random.RandomState(n)
    for i, ev in enumerate(itertools.product([0.0, 1.0], repeat=n)):
        tm = rs.randint(1, 5, size=n).astype(np.float32)
        if i == 1:
            tm[:] = 3.0
        w = rs.randint(0, 3, size=n) if i % 3 else None
        if w is not None and not w.any():
            w[rs.randint(n)] = 1
        pred = (rs.randint(0, 12, size=(n, 2)) / 2).astype(np.float32)
        bins = (2, 10, 32, 3)[i % 4]
        p = np.array([(0.0, 1.0, 0.5, 1.0 / bins, 0.3, 0.77, 2.0 / bins)[rs.randint(7)] for _ in range(n)], dtype=np.float32)
        _agree(np.array(ev, dtype=np.float32), tm, pred, p, bins, (0.0, 1.0, 0.5)[i % 3], w, (n, i))


def test_three_samples_by_hand():
    """y = 1 2 3, e = 1 0 1: S = 2/3, 2/3, 0; theta = 1 + 2/3 + 2/3 = 7/3. The censored sample (block 2): A = S(2) (3 - 2) = 2/3, the
    margin time 2 + (2/3) / (2/3) = 3, omega = 1/3. Deleting it leaves y = 1 3, e = 1 1: S = 1/2 at 1 and at 2 (nobody dies), 0 at 3:
    theta^- = 1 + 1/2 + 1/2 = 2, so the pseudo-observation is 3 * 7/3 - 2 * 2 = 3 (here the margin time)."""
    x = R.row_exact([1, 0, 1], [1, 2, 3], pred=[[1], [1], [1]], literal=True)
    assert x["km"] == [Fraction(7, 3), Fraction(0), Fraction(3)] and x["rowcnt"] == [3, 2, 3, 0]
    assert x["m"][1] == 3 and x["s"][1] == 3
    # hinge (gamma 0): 0 + 1 + 2 over 3; margin and pseudo-observation: 0 + (1/3) 2 + 2 over 1 + 1/3 + 1
    assert x["err"][0] == [[Fraction(3), Fraction(3)], [Fraction(8, 3), Fraction(7, 3)], [Fraction(8, 3), Fraction(7, 3)]]
    a = R.row([1, 0, 1], [1, 2, 3], pred=[[1], [1], [1]])
    assert np.allclose(a["err"][0], [[3, 3], [8 / 3, 7 / 3], [8 / 3, 7 / 3]], rtol=1e-14, atol=0)
    # a weighted case: y = 1 2 4, e = 1 0 1, w = 1 2 1. S = 3/4, 3/4, 0; theta = 1 + 3/4 + 3/2 = 13/4;
    # margin 2 + (3/2) / (3/4) = 4; one copy deleted: S = 2/3, 2/3, 0, theta^- = 1 + 2/3 + 4/3 = 3, pseudo-observation 4 * 13/4 - 3 * 3 = 4
    x = R.row_exact([1, 0, 1], [1, 2, 4], pred=[[1], [1], [1]], w=[1, 2, 1], literal=True)
    assert x["km"][0] == Fraction(13, 4) and x["m"][1] == 4 and x["s"][1] == 4


def test_a_censored_block_tied_with_an_event_block_and_a_censored_tail():
    """y = 1 1 2, e = 1 0 0: the event leaves first, S(1) = 2/3 for the censoring tied with it; the curve never reaches 0 and the
    restricted mean stops at 2. The last sample's tail integral is empty: its margin time is its own time."""
    x = R.row_exact([1, 0, 0], [1, 1, 2], pred=[[0], [0], [0]], literal=True)
    assert x["km"] == [Fraction(1) + Fraction(2, 3), Fraction(2, 3), Fraction(2)]
    assert x["m"] == [1, 1 + Fraction(1), 2] and x["rowcnt"] == [3, 1, 2, 0]


def test_the_curve_is_never_zero_at_a_censored_samples_time():
    """A censored sample is at risk at every time up to its own and the events of a tied time leave before it, so d_v < n_v there:
    rowcnt[3] is 0 under these tie conventions (the slot is the guard of the `m = t where S = 0` clause). The closest case: an event
    tied with the censoring that ends the row, y = 2 2, e = 1 0, w = 5 1: S(2) = 1/6."""
    x = R.row_exact([1, 0], [2, 2], pred=[[0], [0]], w=[5, 1], literal=True)
    assert x["km"][1] == Fraction(1, 6) and x["rowcnt"] == [6, 5, 1, 0] and x["m"][1] == 2
    x = R.row_exact([1, 1], [1, 1], pred=[[0], [0]])
    assert x["km"][1] == 0 and x["rowcnt"][3] == 0


def test_weighted_row_is_the_expanded_cohort():
    ev, tm, pred, p = R.cohort(3, 7, 0.5, 3)
    w = np.array([2, 0, 1, 3, 1, 0, 2])
    xe, xt, xp, xq = R.expand(w, ev, tm, pred, p)
    a, b = R.row(ev, tm, pred, p, 10, 1.0, w), R.row(xe, xt, xp, xq, 10, 1.0)
    assert np.array_equal(a["rowcnt"], b["rowcnt"])
    for k in ("km", "err", "dcal"):
        assert np.allclose(a[k], b[k], rtol=1e-13, atol=1e-13), k


def test_hinge_at_gamma_one_is_the_references_mae():
    """tests/golden/calib_v1.json: the reference's recon_loss(pred, t, e, cur_alpha=0) (its `mae`) on a vector on a grid of 1 / 8, where
    every fp32 step but the final mean is exact: one float32 rounding apart at the most."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "calib_v1.json")))
    for gamma, key in ((1.0, "mae"), (0.0, "hinge0")):
        a = R.row(g["event"], g["time"], np.asarray(g["pred"]).reshape(-1, 1), gamma=gamma, po=False)
        got = a["err"][0, R.HINGE, R.NUM] / a["err"][0, R.HINGE, R.DEN]
        assert abs(got - g[key]) <= 2.0 ** -23 * g[key], (key, got, g[key])


# ---- the host side of the product -------------------------------------------------------------------------------------------------------
def test_statistics_from_rows_is_the_restatements():
    from advmil_amd.eval.calibration import statistics_from_rows
    ev, tm, pred, p = R.cohort(4, 40, 0.5, 6)
    W = np.concatenate([np.ones((1, 40), dtype=np.int32), R.multiplicities(np.random.RandomState(4).randint(0, 40, size=(5, 40)), 40)])
    W[3, ev != 0] = 0                                                              # a row without an event: margin and po undefined
    res = R.rows(ev, tm, pred, p, 10, 1.0, W)
    st = R.statistics(res)
    s = statistics_from_rows(res["rowcnt"], res["km"], res["err"], res["dcal"])
    for k in ("mae_hinge", "mae_margin", "mae_po", "d_cal_chi2", "d_cal_bins"):
        assert np.array_equal(np.isnan(getattr(s, k)), np.isnan(st[k])), k
        assert np.allclose(getattr(s, k), st[k], rtol=1e-15, atol=0, equal_nan=True), k
    assert np.isnan(s.mae_margin[3]).all() and np.isnan(s.mae_po[3]).all() and not np.isnan(s.mae_hinge).any()
    assert np.allclose(s.d_cal_bins.sum(axis=1), 1.0, rtol=1e-13)
    for r in range(6):
        assert abs(s.d_cal_p[r] - R.chi2_sf(st["d_cal_chi2"][r], 9)) <= 1e-13
    absent = statistics_from_rows(res["rowcnt"], res["km"], res["err"], res["dcal"], has_pred=False, has_p=False)
    assert np.isnan(absent.mae_hinge).all() and np.isnan(absent.d_cal_chi2).all() and np.isnan(absent.d_cal_p).all()
    off = statistics_from_rows(res["rowcnt"], res["km"], res["err"], res["dcal"], with_po=False)
    assert np.isnan(off.mae_po).all() and not np.isnan(off.mae_margin[0]).any()


GRID = [(B, x) for B in (2, 3, 10, 32) for x in (0.0, 1e-3, 0.5, 1.0, float(B - 1), 2.0 * B, 5.0 * B, 10.0 * B)]


def test_chi_square_tail():
    """chi2_sf (torch.special.gammaincc in float64) against the series / continued fraction of tests/calib_ref.py, and against
    scipy.stats.chi2.sf where scipy imports."""
    from advmil_amd.eval.calibration import chi2_sf
    assert chi2_sf(np.array(0.0), 3) == 1.0 and np.isnan(chi2_sf(np.array([np.nan]), 3)).all()
    assert abs(chi2_sf(np.array(2.0), 2) - math.exp(-1.0)) <= 4 * U52                 # two degrees: exp(-x / 2)
    for B, x in GRID:
        got, want = float(chi2_sf(np.array(x), B - 1)), R.chi2_sf(x, B - 1)
        assert abs(got - want) <= 1e-13 * want + 1e-300, (B, x, got, want)
    sp = pytest.importorskip("scipy.stats")
    # the largest relative disagreement measured over GRID is 9.3e-15; with the 16 x margin: 1.5e-13
    worst = 0.0
    for B, x in GRID:
        got, want = float(chi2_sf(np.array(x), B - 1)), float(sp.chi2.sf(x, B - 1))
        worst = max(worst, abs(got - want) / want)
        assert abs(got - want) <= 1.5e-13 * want, (B, x, got, want)
    print("largest relative disagreement with scipy", worst)


def test_survival_at_own_time_and_wrappers_validate_and_refuse_without_a_device(monkeypatch):
    from advmil_amd.eval import (ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator, bootstrap_calibration, calib_rows,
                                 d_calibration, survival_at_own_time, time_error)
    ev, tm, pred, p = (torch.from_numpy(a) for a in R.cohort(1, 17, 0.5, 6))
    W = torch.ones(4, 17, dtype=torch.int32)
    with pytest.raises(ValueError, match="neither pred"):
        calib_rows(ev, tm)
    with pytest.raises(ValueError, match="inconsistent"):
        calib_rows(ev[:5], tm, pred)
    with pytest.raises(ValueError, match="inconsistent"):
        calib_rows(ev, tm, pred[:16])
    with pytest.raises(ValueError, match="inconsistent"):
        calib_rows(ev, tm, p_own=p[:16])
    with pytest.raises(ValueError, match="inconsistent"):
        calib_rows(ev, tm, pred, weights=W[:, :9])
    with pytest.raises(ValueError, match="pred: 9 columns"):
        calib_rows(ev, tm, torch.zeros(17, 9))
    with pytest.raises(ValueError, match="pred: expected predicted times"):
        calib_rows(ev, tm, torch.zeros(17, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="p_own: expected probabilities"):
        calib_rows(ev, tm, p_own=torch.zeros(17, dtype=torch.int64))
    for bad_bins in (1, 33, 2.5, True):
        with pytest.raises(ValueError, match="bins:"):
            calib_rows(ev, tm, p_own=p, bins=bad_bins)
    with pytest.raises(ValueError, match="gamma:"):
        calib_rows(ev, tm, pred, gamma=float("nan"))
    with pytest.raises(ValueError, match="int32"):
        calib_rows(ev, tm, pred, weights=W.to(torch.int64))
    with pytest.raises(ValueError, match="expected \\[rows, n\\]"):
        calib_rows(ev, tm, pred, weights=W[0])
    neg = W.clone()
    neg[2, 3] = -1
    with pytest.raises(ValueError, match="negative multiplicities"):
        calib_rows(ev, tm, pred, weights=neg)
    big = W.clone()
    big[1, :] = (1 << 31) // 17 + 1
    with pytest.raises(ValueError, match="2\\^31"):
        calib_rows(ev, tm, pred, weights=big)
    for name, bad in (("time", tm), ("pred", pred), ("p_own", p), ("event", ev)):
        bad = bad.clone()
        bad.reshape(-1)[3] = float("nan")
        with pytest.raises(ValueError, match=name + ": NaN"):
            calib_rows(bad if name == "event" else ev, bad if name == "time" else tm, pred=bad if name == "pred" else pred,
                       p_own=bad if name == "p_own" else p)
    low = tm.clone()
    low[2] = -0.5
    with pytest.raises(ValueError, match="time: negative"):
        calib_rows(ev, low, pred)
    for v in (-0.01, 1.01):
        bad = p.clone()
        bad[5] = v
        with pytest.raises(ValueError, match="p_own: probabilities outside"):
            calib_rows(ev, tm, p_own=bad)
    with pytest.raises(ValueError, match="2\\^16"):
        calib_rows(torch.zeros((1 << 16) + 1), torch.zeros((1 << 16) + 1), torch.zeros((1 << 16) + 1))
    with pytest.raises(ValueError, match="exactly one"):
        survival_at_own_time(tm)
    with pytest.raises(ValueError, match="exactly one"):
        survival_at_own_time(tm, dist_y_hat=pred, hazards=pred)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    y = torch.stack([tm, ev], dim=1)
    for fn in (lambda: calib_rows(ev, tm, pred), lambda: calib_rows(ev, tm, pred, p, 10, 1.0, True, W), lambda: time_error(ev, tm, pred),
               lambda: d_calibration(ev, tm, p), lambda: bootstrap_calibration(ev, tm, pred, n_boot=5),
               lambda: survival_at_own_time(tm, dist_y_hat=pred)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    cont, disc = ContSurv_Evaluator(end_time=1.0), DiscSurv_Evaluator()
    for call in (lambda: cont.time_error({"y": y, "y_hat": tm.reshape(-1, 1)}),
                 lambda: cont.d_calibration({"y": y, "y_hat": tm.reshape(-1, 1), "dist_y_hat": pred.reshape(17, 2, 1)}),
                 lambda: disc.d_calibration({"y": y, "y_hat": pred})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert not hasattr(CoxSurv_Evaluator, "time_error") and not hasattr(CoxSurv_Evaluator, "d_calibration")
    assert not hasattr(DiscSurv_Evaluator, "time_error")


def test_compute_and_its_metric_lists_do_not_change():
    from advmil_amd.eval import ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator
    assert ContSurv_Evaluator(end_time=1.0).valid_metrics == ["c_index", "loss_rank", "loss_recon", "loss_recon_org", "loss_fake_netD",
                                                              "loss_fake_netG", "avg_fake", "event_t_rae", "nonevent_t_rae", "event_t_nre",
                                                              "nonevent_t_nre", "mae"]
    assert DiscSurv_Evaluator().valid_metrics == ["c_index", "loss_mle", "loss_mle_org", "loss_fake_netD", "loss_fake_netG", "avg_fake"]
    assert CoxSurv_Evaluator().valid_metrics == ["c_index", "loss_ple"]


# ---- the C entry without a device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib


def _p(k, off=0):
    return ctypes.c_void_p(A16 + (k << 28) + off)


GOOD = dict(stime=_p(0), sevent=_p(1), order=_p(2), n=64, weights=_p(3), ldw=64, R=8, pred=_p(4), ldp=2, P=2, p_own=_p(5), bins=10,
            gamma=1.0, with_po=1, rowcnt=_p(6), km=_p(7), err=_p(8), dcal=_p(9), ws=_p(10), ws_bytes=8 * 64 * 5 * 8)
NAMES = list(GOOD)


def _call(L, **kw):
    a = dict(GOOD, **kw)
    return L.lib().advmil_calib_rows(*(a[k] for k in NAMES), None)


def test_symbols_are_declared_bound_and_exported(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "advmil_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(advmil_[a-z0-9_]+)\s*\(", hdr))
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in ("advmil_calib_rows", "advmil_calib_rows_workspace_bytes", "advmil_calib_rows_plan"):
        assert name in declared and name in L.SIGNATURES and hasattr(handle, name), name
    assert len(L.SIGNATURES["advmil_calib_rows"][1]) == len(NAMES) + 1


def test_workspace_query_and_plan_are_pure_host_functions(L):
    f = L.lib().advmil_calib_rows_workspace_bytes
    assert f(64, 8, 1) == GOOD["ws_bytes"] and f(64, 8, 0) == 8 * 64 * 3 * 8 and f(1, 1, 0) == 24
    assert f(1 << 16, 1 << 20, 1) == (1 << 36) * 40
    for bad in ((0, 1, 1), ((1 << 16) + 1, 1, 1), (5, 0, 1), (5, (1 << 20) + 1, 1), (5, 1, 2), (5, 1, -1)):
        assert f(*bad) == 0, bad
    v = [ctypes.c_int(-1) for _ in range(3)]
    assert L.lib().advmil_calib_rows_plan(*(ctypes.byref(x) for x in v)) == 0
    assert [x.value for x in v] == [4, 64, 1]
    assert L.lib().advmil_calib_rows_plan(ctypes.byref(v[0]), None, ctypes.byref(v[2])) == EINVAL


def test_every_null_pointer_is_refused(L):
    for name in ("stime", "sevent", "order", "rowcnt", "km", "err", "dcal", "ws"):
        assert _call(L, **{name: None}) == EINVAL, name
    assert _call(L, pred=None, p_own=None) == EINVAL                                   # no source at all


def test_what_may_be_absent_is_refused_for_the_next_reason_only(L):
    """weights NULL means all ones; one of pred and p_own may be NULL: such a call passes validation -- shown by making it fail on the
    workspace, the last check, since a valid call would launch."""
    assert _call(L, weights=None, ldw=0, ws_bytes=GOOD["ws_bytes"] - 1) == EWORKSPACE
    assert _call(L, pred=None, ldp=0, ws_bytes=0) == EWORKSPACE
    assert _call(L, p_own=None, ws_bytes=0) == EWORKSPACE
    assert _call(L, with_po=0, ws_bytes=8 * 64 * 3 * 8 - 1) == EWORKSPACE
    assert _call(L, weights=None, p_own=None, n=0) == EINVAL


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=-1), dict(n=(1 << 16) + 1, ldw=1 << 17), dict(R=0), dict(R=-3), dict(R=(1 << 20) + 1),
                                dict(P=0), dict(P=9, ldp=9), dict(bins=1), dict(bins=33), dict(bins=-1), dict(ldw=63), dict(ldw=0),
                                dict(ldp=1), dict(ldp=0), dict(with_po=2), dict(with_po=-1), dict(gamma=float("nan"))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_out_of_range_arguments(L, kw):
    assert _call(L, **kw) == EINVAL


@pytest.mark.parametrize("kw", [dict(n=1 << 16, ldw=1 << 16), dict(R=1 << 20), dict(P=8, ldp=8), dict(P=1), dict(bins=2), dict(bins=32),
                                dict(n=1, R=1), dict(gamma=-1.0)], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_the_limits_themselves_pass_validation(L, kw):
    assert _call(L, ws_bytes=0, **kw) == EWORKSPACE


@pytest.mark.parametrize("name,off", [("stime", 2), ("sevent", 1), ("order", 2), ("weights", 2), ("pred", 1), ("p_own", 2), ("rowcnt", 4),
                                      ("km", 4), ("err", 4), ("dcal", 4), ("ws", 4)])
def test_misaligned_pointers(L, name, off):
    k = [n for n in NAMES if isinstance(GOOD[n], ctypes.c_void_p)].index(name)
    assert _call(L, **{name: _p(k, off)}) == EINVAL
    assert _call(L, **{name: _p(k, 16), "ws_bytes": 0}) == EWORKSPACE                 # (aligned elsewhere: validation goes on to the workspace)


def test_workspace_too_small(L):
    need = L.lib().advmil_calib_rows_workspace_bytes(64, 8, 1)
    assert _call(L, ws_bytes=need - 1) == EWORKSPACE and _call(L, ws_bytes=0) == EWORKSPACE
    assert _call(L, ws_bytes=need - 1, n=0) == EINVAL                                 # the argument checks come first
