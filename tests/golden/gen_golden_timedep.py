#!/usr/bin/env python3
"""Golden vectors for the time-dependent evaluation (tests/golden/timedep_v1.npz): what scipy.stats.ecdf(CensoredData ...) and
sklearn.metrics.roc_auc_score answer on the seeded cohorts of tests/timedep_ref.py.

  GOLDEN_KM   cohorts without any tied time, so that the order of events and censorings at a tie plays no part: the event Kaplan-Meier
              estimate S_KM is ecdf(uncensored = event times, right = censoring times).sf, the censoring estimate G the same with the two
              roles swapped. Stored per case and estimate (0: G, 1: S_KM): km_len[K, 2] distinct times each, laid end to end in km_t
              (the times) and km_p (the survival there).
  GOLDEN_AUC  cohorts without censoring, where every IPCW weight is 1 and AUC(t) is the ROC AUC of the labels y <= t under the risk
              (ties count one half): auc_len[K] query times each, laid end to end in auc.
Only numbers. The generator asserts that the restatement reproduces them inside its own bounds before it writes anything.
Build container only (scipy >= 1.11, scikit-learn). Usage: python tests/golden/gen_golden_timedep.py"""
import os
import sys

import numpy as np
from scipy import stats
from sklearn.metrics import roc_auc_score

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import timedep_ref as R  # noqa: E402


def main():
    km_len, km_t, km_p, auc_len, auc = [], [], [], [], []
    for k in range(len(R.GOLDEN_KM)):
        ev, tm = R.golden_km_inputs(k)
        e, t = ev != 0, tm.astype(np.float64)
        assert np.unique(t).size == t.size
        ut, G, S = R.km_pair(e, t)
        for which, (unc, right) in enumerate(((t[~e], t[e]), (t[e], t[~e]))):
            sf = stats.ecdf(stats.CensoredData(uncensored=unc, right=right)).sf
            km_len.append(len(sf.quantiles)), km_t.append(sf.quantiles), km_p.append(sf.probabilities)
            mine = R.step(ut, (G, S)[which], sf.quantiles)
            assert (np.abs(mine - sf.probabilities) <= R.bound(t.size) * sf.probabilities).all(), (k, which)
    for k in range(len(R.GOLDEN_AUC)):
        tm, at, risk = R.golden_auc_inputs(k)
        vals = [roc_auc_score(tm <= t, risk[:, 0].astype(np.float64)) for t in at]
        auc_len.append(len(vals)), auc.append(vals)
        st = R.statistics(R.rows(np.ones_like(tm), tm, at, risk=risk), at)
        assert (np.abs(st["auc"][0] - vals) <= 1e-12).all(), (k, st["auc"][0], vals)
    out = dict(km_len=np.array(km_len, dtype=np.int64).reshape(-1, 2), km_t=np.concatenate(km_t).astype(np.float64),
               km_p=np.concatenate(km_p).astype(np.float64), auc_len=np.array(auc_len, dtype=np.int64),
               auc=np.concatenate(auc).astype(np.float64))
    path = os.path.join(HERE, "timedep_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
