"""CPU: the time-dependent evaluation without a device. The float64 restatement (tests/timedep_ref.py) is pinned against what scipy and
scikit-learn answered (tests/golden/timedep_v1.npz), against the closed forms that hold without censoring, against a cohort of five
computed by hand and against itself on an expanded row; the host side of the product (advmil_amd/eval/timedep.py) against the restatement;
and the negative paths of advmil_ipcw_rows (include/advmil_hip.h), which answer before anything is enqueued and so need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import timedep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "timedep_v1.npz"))
EINVAL, EWORKSPACE = -1, -2
A16 = 0x7F0000001000          # a fake, 16-byte aligned "device address": never dereferenced when validation does its job


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(R.GOLDEN_KM)))
def test_restatement_equals_scipys_kaplan_meier(k):
    ev, tm = R.golden_km_inputs(k)
    assert GOLD["km_len"].shape == (len(R.GOLDEN_KM), 2)
    lens = GOLD["km_len"].reshape(-1)
    at = np.unique(np.concatenate([tm, tm + np.float32(0.125), [np.float32(-1.0), np.float32(1e3)]]).astype(np.float32))
    row = R.row(ev, tm, at)
    for which in (0, 1):                                                               # G, S_KM
        o = int(lens[:2 * k + which].sum())
        t, p = GOLD["km_t"][o:o + lens[2 * k + which]], GOLD["km_p"][o:o + lens[2 * k + which]]
        want = R.step(t, p, at.astype(np.float64))
        got = row["sums"][:, 2 + which]
        assert np.array_equal(got == 0, want == 0) and got[0] == 1.0, which
        assert (np.abs(got - want) <= row["bound"] * want).all(), (which, np.abs(got - want).max())


@pytest.mark.parametrize("k", range(len(R.GOLDEN_AUC)))
def test_restatement_equals_the_roc_auc_without_censoring(k):
    tm, at, risk = R.golden_auc_inputs(k)
    o = int(GOLD["auc_len"][:k].sum())
    want = GOLD["auc"][o:o + GOLD["auc_len"][k]]
    assert want.size == at.size >= 2
    res = R.rows(np.ones_like(tm), tm, at, risk=risk)
    st = R.statistics(res, at)
    assert (res["sums"][0, :, 2] == 1.0).all()                                         # nobody censored: G is the empty product
    assert (np.abs(st["auc"][0] - want) <= st["b_auc"][0] + 4 * R.U52).all(), (st["auc"][0], want)


def test_without_censoring_the_brier_score_is_the_mean_squared_error():
    ev, tm, at, surv, risk = R.cohort(5, 40, p_event=1.0, time_levels=7, Q=4, risk_cols=4)
    st = R.statistics(R.rows(ev, tm, at, surv, risk), at)
    t64, s64 = tm.astype(np.float64), surv.astype(np.float64)
    for q in range(at.size):
        want = np.mean(((t64 > at[q]).astype(np.float64) - s64[:, q]) ** 2)
        assert abs(st["brier"][0, q] - want) <= st["b_brier"][0, q] + 4 * R.U52 * want, q


def test_five_samples_with_an_event_tied_with_a_censoring():
    """y = 1 2 2 3 4, e = 1 1 0 0 1. Distinct times: u = 1: n 5 d 1 c 0; u = 2: n 4 d 1 c 1; u = 3: n 2 d 0 c 1; u = 4: n 1 d 1 c 0.
    G: 1 at 1, (4 - 1 - 1) / (4 - 1) = 2/3 at 2 (the event leaves before the censoring), 2/3 * (2 - 0 - 1) / 2 = 1/3 at 3 and at 4.
    S_KM: 4/5 at 1, 4/5 * 3/4 = 3/5 at 2 and 3, 0 at 4.
    At t = 2.5: cases {0, 1} with 1 / G = 1 and 3/2, controls {3, 4}. S = .9 .6 .5 .4 .2, risk = 1 - S.
      A = .81 + .36 * 1.5 = 1.35, B = .36 + .64 = 1, BS = (1.35 + 1 / (2/3)) / 5 = 0.57
      K_0 = 0 (risk .1 against .6 and .8), K_1 = 0 (.4 against .6, .8): C = 0, AUC = 0.
    At t = 1: case {0}, controls {1, 2, 3, 4}; at t = 4 nobody is beyond: undefined."""
    y = np.array([1, 2, 2, 3, 4], dtype=np.float32)
    e = np.array([1, 1, 0, 0, 1], dtype=np.float32)
    S = np.array([.9, .6, .5, .4, .2], dtype=np.float32)
    at = np.array([0.5, 1.0, 2.5, 4.0], dtype=np.float32)
    surv = np.repeat(S[:, None], 4, axis=1)
    r = R.row(e, y, at, surv, 1.0 - S)
    assert r["counts"].tolist() == [[0, 5], [1, 4], [2, 2], [3, 0]] and r["rowcnt"].tolist() == [5, 3]
    assert np.allclose(r["sums"][:, 2], [1, 1, 2 / 3, 1 / 3], rtol=1e-15) and np.allclose(r["sums"][:, 3], [1, .8, .6, 0], rtol=1e-15)
    s64 = S.astype(np.float64)
    A, B, G, _, Wc, C = r["sums"][2]
    assert abs(A - (s64[0] ** 2 + 1.5 * s64[1] ** 2)) < 1e-15 and abs(B - ((1 - s64[3]) ** 2 + (1 - s64[4]) ** 2)) < 1e-15
    assert abs(Wc - 2.5) < 1e-15 and C == 0.0
    st = R.statistics(dict(counts=r["counts"][None], rowcnt=r["rowcnt"][None], sums=r["sums"][None], bound=r["bound"]), at)
    assert abs(st["brier"][0, 2] - 0.57) < 1e-7 and st["auc"][0, 2] == 0.0             # (the fp32 inputs are not the decimals)
    assert abs(st["brier"][0, 0] - np.mean((1 - s64) ** 2)) < 1e-15 and np.isnan(st["auc"][0, 0])      # before every time: G = 1
    assert np.isnan(st["brier"][0, 3]) and np.isnan(st["auc"][0, 3]) and r["sums"][3, [0, 4, 5]].tolist() == [0, 0, 0]
    flipped = R.row(e, y, at, surv, S)                                                 # the risks reversed: every pair concordant
    assert R.statistics(dict(counts=flipped["counts"][None], rowcnt=flipped["rowcnt"][None], sums=flipped["sums"][None],
                             bound=r["bound"]), at)["auc"][0, 1:3].tolist() == [1.0, 1.0]


@pytest.mark.parametrize("n,levels", [(12, 0), (40, 6)])
def test_a_weighted_row_is_the_expanded_cohort(n, levels):
    ev, tm, at, surv, risk = R.cohort(n, n, 0.5, levels, Q=3, risk_cols=3)
    w = R.multiplicities(np.random.RandomState(n).randint(0, n, size=(1, n)), n)[0]
    a = R.row(ev, tm, at, surv, risk, w)
    xe, xt, xs, xr = R.expand(w, ev, tm, surv, risk)
    b = R.row(xe, xt, at, xs, xr)
    for k in ("counts", "rowcnt", "sums"):
        assert np.array_equal(a[k], b[k]), k


def test_all_risks_equal_is_one_half():
    ev, tm, at, surv, _ = R.cohort(9, 30, 0.5, 0, Q=3)
    st = R.statistics(R.rows(ev, tm, at, risk=np.zeros(30, dtype=np.float32)), at)
    # K_i = N_ctrl for every case, so C = (N_ctrl / 2) Wc up to the rounding of the two sums
    assert np.isnan(st["auc"][0, 0]) and (np.abs(st["auc"][0, 1:] - 0.5) <= st["b_auc"][0, 1:]).all()


# ---- the host side of the product -------------------------------------------------------------------------------------------------------
def test_statistics_from_rows_is_the_restatements():
    from advmil_amd.eval import statistics_from_rows
    ev, tm, at, surv, risk = R.cohort(4, 60, 0.5, 9, Q=5, risk_cols=5)
    at = np.concatenate([at, [np.float32(2.0)]]).astype(np.float32)                    # ... and one beyond everyone
    surv = np.concatenate([surv, surv[:, -1:] * np.float32(0.5)], axis=1)
    risk = np.concatenate([risk, risk[:, -1:]], axis=1)
    W = R.multiplicities(np.random.RandomState(4).randint(0, 60, size=(6, 60)), 60)
    res = R.rows(ev, tm, at, surv, risk, W)
    want = R.statistics(res, at)
    got = statistics_from_rows(res["counts"], res["rowcnt"], res["sums"], at)
    for k in ("brier", "auc", "ibs", "mean_auc"):
        assert np.array_equal(np.isnan(getattr(got, k)), np.isnan(want[k])), k
        assert np.allclose(getattr(got, k), want[k], rtol=1e-14, atol=0, equal_nan=True), k
    assert np.isnan(got.brier[:, -1]).all() and np.isnan(got.ibs).all() and not np.isnan(got.brier[:, :-1]).any()
    inner = statistics_from_rows(res["counts"][:, 1:-1], res["rowcnt"], res["sums"][:, 1:-1], at[1:-1])
    want_inner = R.statistics(dict(res, counts=res["counts"][:, 1:-1], sums=res["sums"][:, 1:-1]), at[1:-1])
    assert not np.isnan(inner.ibs).any() and np.allclose(inner.ibs, want_inner["ibs"], rtol=1e-14, atol=0)
    assert not np.isnan(inner.mean_auc).any() and np.allclose(inner.mean_auc, want_inner["mean_auc"], rtol=1e-13, atol=0)


def test_default_times_are_deciles_of_the_event_times_below_the_largest_time():
    from advmil_amd.eval import default_times
    a = R.api_cohort()
    tm, ev = a["y"][:, 0], a["y"][:, 1]
    got = default_times(torch.from_numpy(ev), torch.from_numpy(tm))
    assert got.dtype == np.float32 and np.array_equal(got, R.default_times(ev, tm)) and 2 <= got.size <= 9
    assert (np.diff(got) > 0).all() and got.max() < tm.max() and np.isin(got, tm[ev != 0]).all()
    t2, e2 = np.array([1, 1, 1, 2], dtype=np.float32), np.array([1, 1, 1, 1], dtype=np.float32)
    assert default_times(e2, t2).tolist() == [1.0]                                     # de-duplicated; 2.0 is the largest time: dropped
    with pytest.raises(ValueError, match="no observed event"):
        default_times(0 * e2, t2)


def test_wrappers_validate_and_refuse_without_a_device(monkeypatch):
    from advmil_amd.eval import (ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator, bootstrap_timedep, brier_score,
                                 cumulative_dynamic_auc, integrated_brier_score, ipcw_rows, survival_from_hazards, survival_from_samples)
    ev, tm, at, surv, risk = (torch.from_numpy(a) for a in R.cohort(1, 17, 0.5, 6, Q=3, risk_cols=3))
    W = torch.ones(4, 17, dtype=torch.int32)
    with pytest.raises(ValueError, match="inconsistent"):
        ipcw_rows(ev[:5], tm, at)
    with pytest.raises(ValueError, match="inconsistent"):
        ipcw_rows(ev, tm, at, weights=W[:, :9])
    with pytest.raises(ValueError, match="inconsistent"):
        ipcw_rows(ev, tm, at, surv=surv[:16])
    with pytest.raises(ValueError, match="inconsistent"):
        ipcw_rows(ev, tm, at, risk=risk[:16, 0])
    with pytest.raises(ValueError, match="surv: 2 columns"):
        ipcw_rows(ev, tm, at, surv=surv[:, :2])
    with pytest.raises(ValueError, match="risk: 2 columns"):
        ipcw_rows(ev, tm, at, risk=risk[:, :2])
    with pytest.raises(ValueError, match="int32"):
        ipcw_rows(ev, tm, at, weights=W.to(torch.int64))
    neg = W.clone()
    neg[2, 3] = -1
    with pytest.raises(ValueError, match="negative"):
        ipcw_rows(ev, tm, at, weights=neg)
    big = W.clone()
    big[1, :] = (1 << 31) // 17 + 1
    with pytest.raises(ValueError, match="2\\^31"):
        ipcw_rows(ev, tm, at, weights=big)
    for name, bad in (("time", tm), ("surv", surv), ("risk", risk)):
        bad = bad.clone()
        bad.reshape(-1)[3] = float("nan")
        with pytest.raises(ValueError, match=name + ": NaN"):
            ipcw_rows(ev, bad if name == "time" else tm, at, surv=bad if name == "surv" else None, risk=bad if name == "risk" else None)
    with pytest.raises(ValueError, match="ascend"):
        ipcw_rows(ev, tm, torch.tensor([0.5, 0.25]))
    with pytest.raises(ValueError, match="query"):
        ipcw_rows(ev, tm, torch.zeros(4097))
    with pytest.raises(ValueError, match="query"):
        ipcw_rows(ev, tm, torch.zeros(0))
    with pytest.raises(ValueError, match="2\\^16"):
        ipcw_rows(torch.zeros((1 << 16) + 1), torch.zeros((1 << 16) + 1), at)
    with pytest.raises(ValueError, match="two query times"):
        integrated_brier_score(ev, tm, surv[:, :1], at[:1])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    y = torch.stack([tm, ev], dim=1)
    for fn in (lambda: ipcw_rows(ev, tm, at), lambda: ipcw_rows(ev, tm, at, surv, risk, W), lambda: brier_score(ev, tm, surv, at),
               lambda: integrated_brier_score(ev, tm, surv, at), lambda: cumulative_dynamic_auc(ev, tm, risk, at),
               lambda: bootstrap_timedep(ev, tm, at, surv, risk, n_boot=5), lambda: survival_from_samples(surv, at),
               lambda: survival_from_hazards(surv)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    for evl, data in ((ContSurv_Evaluator(end_time=1.0), {"y": y, "y_hat": tm.reshape(-1, 1), "dist_y_hat": surv.reshape(17, 3, 1)}),
                      (DiscSurv_Evaluator(), {"y": y, "y_hat": surv}), (CoxSurv_Evaluator(), {"y": y, "y_hat": tm.reshape(-1, 1)})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evl.time_dependent(data)


# ---- the C entry without a device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib


def _p(k, off=0):
    return ctypes.c_void_p(A16 + (k << 28) + off)


GOOD = dict(stime=_p(0), sevent=_p(1), order=_p(2), n=64, weights=_p(3), ldw=64, R=8, at=_p(4), Q=16, surv=_p(5), lds=16, risk=_p(6), ldr=16,
            risk_cols=16, counts=_p(7), rowcnt=_p(8), sums=_p(9), ws=_p(10), ws_bytes=8 * 64 * 8 + (64 + 16) * 4)
NAMES = list(GOOD)


def _call(L, **kw):
    a = dict(GOOD, **kw)
    return L.lib().advmil_ipcw_rows(*(a[k] for k in NAMES), None)


def test_symbols_are_declared_bound_and_exported(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "advmil_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(advmil_[a-z0-9_]+)\s*\(", hdr))
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in ("advmil_ipcw_rows", "advmil_ipcw_rows_workspace_bytes", "advmil_ipcw_rows_plan"):
        assert name in declared and name in L.SIGNATURES and hasattr(handle, name), name
    assert len(L.SIGNATURES["advmil_ipcw_rows"][1]) == len(NAMES) + 1


def test_workspace_query_and_plan_are_pure_host_functions(L):
    f = L.lib().advmil_ipcw_rows_workspace_bytes
    assert f(64, 8, 16) == GOOD["ws_bytes"] and f(1, 1, 1) == 8 + 8 and f(1000, 1001, 16) == 1000 * 1001 * 8 + 1016 * 4
    assert f(3, 2, 2) == 48 + 24                                                       # n + Q odd: rounded up to 8 bytes
    assert f(1 << 16, 1 << 20, 4096) == (1 << 39) + ((1 << 16) + 4096) * 4
    assert f(0, 1, 1) == 0 and f((1 << 16) + 1, 1, 1) == 0 and f(5, 0, 1) == 0 and f(5, 1, 0) == 0 and f(5, 1, 4097) == 0
    v = [ctypes.c_int(0) for _ in range(4)]
    assert L.lib().advmil_ipcw_rows_plan(*(ctypes.byref(x) for x in v)) == 0
    assert [x.value for x in v] == [4, 64, 256, 8]                                     # the sizes tests/test_timedep_gpu.py straddles
    assert L.lib().advmil_ipcw_rows_plan(None, ctypes.byref(v[1]), ctypes.byref(v[2]), ctypes.byref(v[3])) == EINVAL


def test_every_null_pointer_is_refused(L):
    for name in ("stime", "sevent", "order", "at", "counts", "rowcnt", "sums", "ws"):
        assert _call(L, **{name: None}) == EINVAL, name


def test_what_may_be_absent_is_refused_for_the_next_reason_only(L):
    """weights NULL means all ones, surv NULL and risk NULL leave their sums 0: such a call passes validation -- shown by making it fail
    on the workspace, the last check, since a valid call would launch."""
    assert _call(L, weights=None, ldw=0, ws_bytes=GOOD["ws_bytes"] - 1) == EWORKSPACE
    assert _call(L, surv=None, lds=0, ws_bytes=0) == EWORKSPACE
    assert _call(L, risk=None, ldr=0, risk_cols=0, ws_bytes=0) == EWORKSPACE
    assert _call(L, risk_cols=1, ldr=1, ws_bytes=0) == EWORKSPACE                      # one shared risk column
    assert _call(L, weights=None, surv=None, risk=None, n=0) == EINVAL


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=-1), dict(n=(1 << 16) + 1, ldw=1 << 17, ws_bytes=1 << 40), dict(R=0), dict(R=-3),
                                dict(R=(1 << 20) + 1, ws_bytes=1 << 40), dict(Q=0), dict(Q=-1),
                                dict(Q=4097, lds=4097, ldr=4097, risk_cols=4097, ws_bytes=1 << 40), dict(ldw=63), dict(ldw=0), dict(ldw=-64),
                                dict(lds=15), dict(lds=0), dict(ldr=15), dict(ldr=0), dict(risk_cols=2), dict(risk_cols=0), dict(risk_cols=15, ldr=15)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_out_of_range_shapes(L, kw):
    assert _call(L, **kw) == EINVAL


@pytest.mark.parametrize("name,off", [("stime", 2), ("sevent", 1), ("order", 2), ("weights", 2), ("at", 1), ("surv", 2), ("risk", 1),
                                      ("counts", 4), ("rowcnt", 4), ("sums", 4), ("ws", 4)])
def test_misaligned_pointers(L, name, off):
    k = [n for n in NAMES if isinstance(GOOD[n], ctypes.c_void_p)].index(name)
    assert _call(L, **{name: _p(k, off)}) == EINVAL
    assert _call(L, **{name: _p(k, 16), "ws_bytes": 0}) == EWORKSPACE                 # (aligned elsewhere: validation goes on to the workspace)


def test_workspace_too_small(L):
    need = L.lib().advmil_ipcw_rows_workspace_bytes(64, 8, 16)
    assert _call(L, ws_bytes=need - 1) == EWORKSPACE and _call(L, ws_bytes=0) == EWORKSPACE
    assert _call(L, ws_bytes=need - 1, n=0) == EINVAL                                 # the argument checks come first
