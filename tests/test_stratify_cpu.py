"""CPU: the risk-group stratification without a device. The float64 restatement (tests/logrank_ref.py) is pinned against what scipy
answered on the expanded cohorts (tests/golden/logrank_v1.npz) and against live scipy where it imports; its weighted formulas against
the unweighted ones on the expansion, bit for bit; and the host side of the product (advmil_amd/eval/stratify.py) against both."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import logrank_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "logrank_v1.npz"))
K = len(R.GOLDEN_CASES)


def S():
    return importlib.import_module("advmil_amd.eval.stratify")       # (the package exports a function of the same name)


def _golden_sf(k, c):
    lens = GOLD["sf_len"].reshape(-1)
    o = int(lens[:3 * k + c].sum())
    return GOLD["sf_t"][o:o + lens[3 * k + c]], GOLD["sf_p"][o:o + lens[3 * k + c]]


def _step(t, p, at):
    """A right-continuous step function (value 1 before its first time) at the times `at`."""
    i = np.searchsorted(t, at, side="right") - 1
    return np.where(i >= 0, p[np.maximum(i, 0)], 1.0)


def _check_against_sf(row, sf, at):
    """row: the restatement at the query times `at`; sf(c) -> scipy's (times, survival) of class c."""
    for c in range(3):
        t, p = sf(c)
        want = _step(t, p, at)
        got = row["km"][c]
        assert np.array_equal(got == 0, want == 0), c                                  # an exact zero is one on both sides
        assert (np.abs(got - want) <= row["bkm"] * want).all(), (c, np.abs(got - want).max())
        below = np.nonzero(p <= 0.5)[0]
        assert row["median"][c] == (t[below[0]] if below.size else np.inf), c


@pytest.mark.parametrize("k", range(K))
def test_restatement_equals_the_golden(k):
    ev, tm, g, w = R.golden_inputs(k)
    assert GOLD["z"].shape == (K,) and GOLD["sf_len"].shape == (K, 3)
    at = np.unique(np.concatenate([tm, tm + np.float32(0.01), [np.float32(-1.0), np.float32(99.0)]]).astype(np.float32))
    row = R.Cohort(ev, tm).row(g, w, at)
    assert not row["undefined"] and abs(row["z"] - GOLD["z"][k]) <= row["bz"], (row["z"], GOLD["z"][k], row["bz"])
    _check_against_sf(row, lambda c: _golden_sf(k, c), at.astype(np.float64))
    assert (row["km"][:, 0] == 1.0).all()                                              # before every time: the empty product


def test_five_sample_case_ends_on_an_event_with_one_at_risk():
    k = next(i for i, c in enumerate(R.GOLDEN_CASES) if c.get("five"))
    ev, tm, g, _ = R.golden_inputs(k)
    row = R.Cohort(ev, tm).row(g, None, tm)
    assert row["counts"].tolist() == [2, 3, 2, 5, 3, 2]                                # three event times, the last with n_j == 1
    assert row["km"][0, -1] == 0.0 and row["km"][2, -1] == 0.0 and row["km"][1, -1] == 0.0
    assert row["km"][2].tolist() == [0.8, 0.8, 0.8 * (2.0 / 3.0), 0.8 * (2.0 / 3.0), 0.0]
    assert row["median"].tolist() == [5.0, 1.0, 5.0]


@pytest.mark.parametrize("seed", range(4))
def test_restatement_equals_live_scipy(seed):
    stats = pytest.importorskip("scipy.stats")
    if not hasattr(stats, "logrank"):
        pytest.skip("scipy without stats.logrank")
    ev, tm, g, w = R.cohort(100 + seed, 30 + 7 * seed, p_event=0.4 + 0.1 * seed, time_levels=(0, 8, 0, 15)[seed], weighted=seed % 2 == 1)
    at = np.unique(tm)
    row = R.Cohort(ev, tm).row(g, w, at)
    xe, xt, xg = (ev, tm, g) if w is None else R.expand(w, ev, tm, g)
    e, t, g1 = xe != 0, xt.astype(np.float64), xg != 0
    cd = lambda sel: stats.CensoredData(uncensored=t[sel & e], right=t[sel & ~e])     # noqa: E731
    res = stats.logrank(cd(g1), cd(~g1))
    assert abs(res.statistic - row["z"]) <= row["bz"]
    assert abs(res.pvalue - R.p_of(row["z"])) <= 1e-9 * res.pvalue

    def sf(c):
        s = stats.ecdf(cd((~g1, g1, np.ones_like(g1))[c])).sf
        return np.asarray(s.quantiles), np.asarray(s.probabilities)
    _check_against_sf(row, sf, at.astype(np.float64))


@pytest.mark.parametrize("n,levels", [(1, 0), (2, 1), (17, 5), (64, 0), (65, 9)])
def test_weights_are_the_expansion_bit_for_bit(n, levels):
    rs = np.random.RandomState(n)
    ev, tm, g, _ = R.cohort(200 + n, n, 0.5, levels)
    at = np.unique(np.concatenate([tm, [np.float32(0.5)]]))
    W = np.concatenate([R.multiplicities(rs.randint(0, n, size=(6, n)), n), np.zeros((1, n), np.int32), 3 * np.eye(n, dtype=np.int32)[:1]])
    for w in W:
        a = R.Cohort(ev, tm).row(g, w, at)
        xe, xt, xg = R.expand(w, ev, tm, g)
        b = R.Cohort(xe, xt).row(xg, None, at) if w.sum() else None
        if b is None:                                                                  # nothing to expand: every sum empty, every product 1
            assert a["counts"].tolist() == [0] * 6 and a["E1"] == 0 and a["V"] == 0 and (a["km"] == 1).all() and np.isinf(a["median"]).all()
            assert a["undefined"]
            continue
        for key in ("counts", "km", "median"):
            assert np.array_equal(a[key], b[key]), key
        assert (a["E1"], a["V"], a["bE1"], a["bV"]) == (b["E1"], b["V"], b["bE1"], b["bV"])
        assert a["undefined"] == b["undefined"] and (a["undefined"] or (a["z"], a["bz"]) == (b["z"], b["bz"]))


def test_permutation_groups_is_the_documented_stream():
    from advmil_amd.eval import permutation_groups
    g = np.array([1, 0, 0, 1, 1, 0, 0, 0, 2], dtype=np.int64)                           # not 0 counts as 1
    got = permutation_groups(g, 7, seed=3)
    assert got.dtype == np.uint8 and got.shape == (7, 9) and (got.sum(axis=1) == 4).all()
    for p in (0, 4, 6):
        rs = np.random.RandomState(3)
        for _ in range(p + 1):
            row = rs.permutation((g != 0).astype(np.uint8))
        assert np.array_equal(got[p], row), p
    assert np.array_equal(permutation_groups(torch.from_numpy(g), 7, seed=3), got)


def test_logrank_from_rows_forms_z_and_p_as_scipy_does():
    from advmil_amd.eval import logrank_from_rows
    rows = [R.Cohort(*R.golden_inputs(k)[:2]).row(*R.golden_inputs(k)[2:]) for k in range(K)]
    counts = np.stack([r["counts"] for r in rows])
    sums = np.array([[r["E1"], r["V"]] for r in rows])
    s = logrank_from_rows(counts, sums)
    assert s.z.dtype == np.float64 and not s.undefined.any()
    for k in range(K):
        assert s.z[k] == rows[k]["z"] and s.chi2[k] == s.z[k] ** 2
        assert abs(GOLD["z"][k]) <= 6 and abs(s.p[k] - GOLD["p"][k]) <= 1e-9 * GOLD["p"][k], (k, s.p[k], GOLD["p"][k])
    # the tail, against the same double-precision erfc: |z| up to 6
    zs = np.linspace(-6, 6, 49)
    t = logrank_from_rows(np.tile(np.array([5, 10, 10, 20, 3, 3]), (49, 1)), np.stack([5 - zs, np.ones(49)], axis=1))
    assert np.array_equal(t.z, zs) and np.array_equal(t.p, [math.erfc(abs(z) / math.sqrt(2.0)) for z in zs])
    # what has no statistic: V == 0, no group 1, no group 0, no event
    bad = logrank_from_rows(np.array([[1, 2, 3, 6, 1, 0], [0, 2, 0, 6, 2, 2], [2, 2, 6, 6, 2, 2], [0, 0, 3, 6, 0, 0], [1, 2, 3, 6, 2, 2]]),
                            np.array([[1.0, 0.0], [0.0, 1.0], [2.0, 1.0], [0.0, 0.0], [1.0, 0.5]]))
    assert bad.undefined.tolist() == [True, True, True, True, False]
    assert np.isnan(bad.z[:4]).all() and np.isnan(bad.p[:4]).all() and bad.z[4] == 0.0 and bad.p[4] == 1.0
    both = logrank_from_rows(torch.from_numpy(counts), torch.from_numpy(sums))
    assert np.array_equal(both.z, s.z)


def test_risk_groups_split_above_the_quantile():
    from advmil_amd.eval import risk_groups
    r = np.array([0.1, 0.4, 0.4, 0.4, 0.9, 0.2], dtype=np.float32)
    g, thr = risk_groups(torch.from_numpy(r), 0.5)
    assert thr == 0.4000000059604645 and g.tolist() == [0, 0, 0, 0, 1, 0]                # ties with the quantile go to the low group
    g2, thr2 = R.risk_groups(r, 0.5)
    assert np.array_equal(g, g2) and thr == thr2
    with pytest.raises(ValueError, match="quantile"):
        risk_groups(r, 1.0)


def test_wrappers_validate_and_refuse_without_a_device(monkeypatch):
    from advmil_amd.eval import (ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator, kaplan_meier, logrank_permutation_test,
                                 logrank_rows, logrank_scan, logrank_test, stratify)
    ev, tm, g, _ = (torch.from_numpy(a) if a is not None else None for a in R.cohort(1, 17, 0.5, 6))
    W = torch.ones(4, 17, dtype=torch.int32)
    with pytest.raises(ValueError, match="inconsistent"):
        logrank_rows(ev, tm, g[:16])
    with pytest.raises(ValueError, match="inconsistent"):
        logrank_rows(ev[:5], tm, g)
    with pytest.raises(ValueError, match="inconsistent"):
        logrank_rows(ev, tm, g, W[:, :9])
    with pytest.raises(ValueError, match="int32"):
        logrank_rows(ev, tm, g, W.to(torch.int64))
    with pytest.raises(ValueError, match="rows"):
        logrank_rows(ev, tm, g.repeat(3, 1), W)
    with pytest.raises(ValueError, match="groups"):
        logrank_rows(ev, tm, g.to(torch.float32))
    neg = W.clone()
    neg[2, 3] = -1
    with pytest.raises(ValueError, match="negative"):
        logrank_rows(ev, tm, g, neg)
    big = W.clone()
    big[1, :] = (1 << 31) // 17 + 1
    with pytest.raises(ValueError, match="2\\^31"):
        logrank_rows(ev, tm, g, big)
    bad_t = tm.clone()
    bad_t[3] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        logrank_rows(ev, bad_t, g)
    with pytest.raises(ValueError, match="ascend"):
        logrank_rows(ev, tm, g, at=torch.tensor([0.5, 0.25]))
    with pytest.raises(ValueError, match="query"):
        logrank_rows(ev, tm, g, at=torch.zeros((1 << 16) + 1))
    with pytest.raises(ValueError, match="n_cuts"):
        logrank_scan(torch.stack([tm, ev], dim=1), tm.reshape(-1, 1), n_cuts=65)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    y, pred = torch.stack([tm, ev], dim=1), tm.reshape(-1, 1)
    for fn in (lambda: logrank_rows(ev, tm, g), lambda: logrank_rows(ev, tm, g, W, at=tm.sort().values), lambda: logrank_test(ev, tm, g),
               lambda: logrank_permutation_test(ev, tm, g, n_perm=5), lambda: kaplan_meier(ev, tm), lambda: kaplan_meier(ev, tm, g, n_boot=5),
               lambda: stratify(y, pred), lambda: stratify(y, pred, n_perm=3, n_boot=3), lambda: logrank_scan(y, pred, n_cuts=4, n_perm=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    for evl in (ContSurv_Evaluator(end_time=1.0), DiscSurv_Evaluator(), CoxSurv_Evaluator()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evl.stratify({"y": y, "y_hat": pred})
    from advmil_amd.eval import bootstrap as BS
    assert S()._NO_DEVICE is BS._NO_DEVICE                                             # the same text as the C-index bootstrap


def test_product_imports_neither_scipy_nor_the_tests():
    pat = re.compile(r"^\s*(from|import)\s+(scipy|tests)\b|__import__\(\s*[\"'](scipy|tests)|import_module\(\s*[\"'](scipy|tests)", re.M)
    seen = 0
    for d, _, files in os.walk(os.path.join(ROOT, "advmil_amd")):
        for f in files:
            if f.endswith(".py"):
                seen += 1
                assert not pat.search(open(os.path.join(d, f)).read()), os.path.join(d, f)
    assert seen > 10 and os.path.exists(os.path.join(ROOT, "advmil_amd", "eval", "stratify.py"))
