#!/usr/bin/env python3
"""Golden vectors for the risk-group stratification (tests/golden/logrank_v1.npz): what scipy.stats.logrank and
scipy.stats.ecdf(CensoredData ...) answer on the seeded cohorts of tests/logrank_ref.py::GOLDEN_CASES -- tied times, bootstrap
resamples EXPANDED into plain arrays (scipy knows no weights), and the five-sample cohort whose last sample at risk is an event.

Stored: z[K], p[K] (scipy's statistic with x = group 1, y = group 0, and its two-sided p-value), and for the classes c = 0 (group 0),
1 (group 1), 2 (pooled) the Kaplan-Meier step function: sf_len[K, 3] distinct times each, laid end to end in sf_t (the times) and sf_p
(the survival there), case by case and class by class. Only numbers. The generator asserts that no cohort is an undefined row (V == 0, an
empty group, no event) and that the restatement reproduces scipy inside its own bounds before it writes anything.
Build container only (scipy >= 1.11). Usage: python tests/golden/gen_golden_logrank.py"""
import os
import sys

import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import logrank_ref as R  # noqa: E402


def censored(t, e):
    return stats.CensoredData(uncensored=t[e], right=t[~e])


def main():
    z, p, sf_len, sf_t, sf_p = [], [], [], [], []
    for k in range(len(R.GOLDEN_CASES)):
        ev, tm, g, w = R.golden_inputs(k)
        row = R.Cohort(ev, tm).row(g, w)
        assert not row["undefined"], f"case {k} is an undefined row"
        if w is not None:
            ev, tm, g = R.expand(w, ev, tm, g)
        e, t, g1 = ev != 0, tm.astype(np.float64), g != 0
        res = stats.logrank(censored(t[g1], e[g1]), censored(t[~g1], e[~g1]))
        z.append(res.statistic), p.append(res.pvalue)
        assert abs(res.statistic - row["z"]) <= row["bz"], (k, res.statistic, row["z"], row["bz"])
        for c, sel in enumerate((~g1, g1, np.ones_like(g1))):
            sf = stats.ecdf(censored(t[sel], e[sel])).sf
            sf_len.append(len(sf.quantiles)), sf_t.append(sf.quantiles), sf_p.append(sf.probabilities)
    out = dict(z=np.array(z, dtype=np.float64), p=np.array(p, dtype=np.float64), sf_len=np.array(sf_len, dtype=np.int64).reshape(-1, 3),
               sf_t=np.concatenate(sf_t).astype(np.float64), sf_p=np.concatenate(sf_p).astype(np.float64))
    path = os.path.join(HERE, "logrank_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
