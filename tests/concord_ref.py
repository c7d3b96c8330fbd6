"""Two independent restatements of advmil_concord_rows (include/advmil_hip.h, csrc/concord.hip) and of what
advmil_amd/eval/concordance.py builds on it.

(a) `row` / `rows`: float64 numpy, written naively. A weighted row is EXPANDED into repeated samples (`timedep_ref.expand`), the censoring
    Kaplan-Meier estimate is `timedep_ref.km_pair`'s loop over the distinct times of the expansion, and the pairs are a literal double
    loop over the expansion (`literal=True`; `literal=False` replaces the inner loop by one numpy comparison per case, for cohorts of
    hundreds -- tests/test_concord_cpu.py holds the two equal).
(b) `row_exact`: `fractions.Fraction` over the WEIGHTED row (no expansion, its own Kaplan-Meier product), for n <= 8: G, the Uno sums
    and the ratios as exact rationals.

Rounding bound of (a), u = 2^-53 (n = the cohort's size, before expansion; at most n distinct times): G is np.cumprod over at most n
correctly rounded quotients, relative (2n - 1) u; a term K / (G G) squares it and divides, (4n) u; math.fsum adds one rounding:
below 3 n 2^-52 (`bound`), which is also what the header derives for the kernel. A test allows the sum of the two.
Counts and every K_i are integers: equal or wrong."""
import math
from fractions import Fraction

import numpy as np

from tests.timedep_ref import U52, expand, km_pair, multiplicities, step  # noqa: F401

RISK, SURV = 0, 1
CONC, TIED, COMP = 0, 1, 2


def bound(n):
    return 3.0 * n * U52


def taus(tau):
    return np.asarray([np.inf] if tau is None else tau, dtype=np.float32).reshape(-1)


def own_columns(time, at):
    """pycox's idx_at_times, steps = "post": the last grid time at or before the sample's time (column 0 before the grid)."""
    return (np.searchsorted(np.asarray(at, dtype=np.float32), np.asarray(time, dtype=np.float32), side="right") - 1).clip(0, len(at) - 1)


def row(event, time, risk=None, surv=None, col=None, tau=None, w=None, literal=True):
    """One row. event [n], time [n]; risk [n] or None; surv [n, Q] with col int [n], or None; tau None, a number or [T]; w int [n] or None.
    -> dict: counts int64 [2, 3] (source risk | surv; conc, tied, comp), rowcnt int64 [2 + T], sums float64 [2, T, 3], bound (relative,
    of every sum), G (float64, of every expanded sample at its own time)."""
    n = len(time)
    w = np.ones(n, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64).reshape(-1)
    assert w.size == n and (w >= 0).all() and (risk is not None or surv is not None)
    tv = taus(tau).astype(np.float64)
    T = tv.size
    idx = np.repeat(np.arange(n), w)                                              # the expansion
    N = idx.size
    e = (np.asarray(event) != 0)[idx]
    y = np.asarray(time, dtype=np.float32).astype(np.float64)[idx]
    ut, G, _ = km_pair(e, y)
    Gy = step(ut, G, y) if N else np.zeros(0)
    K = np.zeros((2, N, 3), dtype=np.int64)
    for s in (RISK, SURV):
        if (risk if s == RISK else surv) is None:
            continue
        if s == RISK:
            r = np.asarray(risk, dtype=np.float32).reshape(n)[idx]
        else:
            S = np.asarray(surv, dtype=np.float32).reshape(n, -1)
            c = np.asarray(col).reshape(n)
        for i in range(N):
            if not e[i]:
                continue
            # the two numbers compared for the pair (i, j), such that "i worse than j" reads a[j] < mine
            mine, theirs = (-r[i], -r) if s == RISK else (S[idx[i], c[idx[i]]], S[idx, c[idx[i]]])
            if literal:
                for j in range(N):
                    if y[j] > y[i] or (y[j] == y[i] and not e[j]):
                        K[s, i, COMP] += 1
                        if mine < theirs[j]:
                            K[s, i, CONC] += 1
                        elif mine == theirs[j]:
                            K[s, i, TIED] += 1
            else:
                comp = (y > y[i]) | ((y == y[i]) & ~e)
                K[s, i] = ((mine < theirs) & comp).sum(), ((mine == theirs) & comp).sum(), comp.sum()
    counts = K.sum(axis=1)
    rowcnt = np.zeros(2 + T, dtype=np.int64)
    rowcnt[0], rowcnt[1] = int(w.sum()), int(w[np.asarray(event) != 0].sum())
    sums = np.zeros((2, T, 3), dtype=np.float64)
    for t in range(T):
        before = e & (y < tv[t])
        rowcnt[2 + t] = int((before & (Gy == 0)).sum())
        use = before & (Gy > 0)
        for s in (RISK, SURV):
            for k in range(3):
                sums[s, t, k] = math.fsum(K[s, use, k] / (Gy[use] * Gy[use]))
    return dict(counts=counts, rowcnt=rowcnt, sums=sums, bound=bound(n), G=Gy)


def rows(event, time, risk=None, surv=None, col=None, tau=None, W=None, literal=True):
    """W [R, n] or None (one row of ones) -> the rows' results stacked: counts [R, 2, 3], rowcnt [R, 2 + T], sums [R, 2, T, 3]."""
    res = [row(event, time, risk, surv, col, tau, None if W is None else W[r], literal) for r in range(1 if W is None else len(W))]
    return dict(counts=np.stack([x["counts"] for x in res]), rowcnt=np.stack([x["rowcnt"] for x in res]),
                sums=np.stack([x["sums"] for x in res]), bound=res[0]["bound"])


def statistics(res, has_risk=True, has_surv=True):
    """The statistics of rows (see `rows`): c_harrell, c_td, c_td_adj [R], c_uno, c_uno_td [R, T] (NaN where undefined or absent), and
    b_<name>: the absolute bound of each (a ratio of sums that are each within `bound`: 3 bound relative; 0 for the count ratios, which
    are one correctly rounded division apart at the most -- 2^-52 relative is allowed for them)."""
    c, rc, s, b = res["counts"], res["rowcnt"], res["sums"], res["bound"]
    R, T = c.shape[0], s.shape[2]
    out = {k: np.full(R, np.nan) for k in ("c_harrell", "c_td", "c_td_adj")}
    out.update({k: np.full((R, T), np.nan) for k in ("c_uno", "c_uno_td")})
    for r in range(R):
        if has_risk and c[r, RISK, COMP] > 0:
            out["c_harrell"][r] = (c[r, RISK, CONC] + 0.5 * c[r, RISK, TIED]) / c[r, RISK, COMP]
        if has_surv and c[r, SURV, COMP] > 0:
            out["c_td"][r] = c[r, SURV, CONC] / c[r, SURV, COMP]
            out["c_td_adj"][r] = (c[r, SURV, CONC] + 0.5 * c[r, SURV, TIED]) / c[r, SURV, COMP]
        for t in range(T):
            for name, src, has in (("c_uno", RISK, has_risk), ("c_uno_td", SURV, has_surv)):
                if has and rc[r, 2 + t] == 0 and s[r, src, t, COMP] > 0:
                    out[name][r, t] = (s[r, src, t, CONC] + 0.5 * s[r, src, t, TIED]) / s[r, src, t, COMP]
    for k in ("c_harrell", "c_td", "c_td_adj"):
        out["b_" + k] = 2 * U52 * out[k]
    for k in ("c_uno", "c_uno_td"):
        out["b_" + k] = 3 * 2 * b * out[k]                                        # the restatement's bound and the kernel's
    return out


# ---- (b) exact rationals --------------------------------------------------------------------------------------------------------------
def row_exact(event, time, risk=None, surv=None, col=None, tau=None, w=None):
    """The same row in exact arithmetic, on the weighted samples themselves (n <= 8). -> dict: counts [2][3] (int), rowcnt [2 + T] (int),
    sums [2][T][3] (Fraction), G [n] (Fraction, at every sample's own time), and the ratios c_harrell, c_td, c_td_adj, c_uno [T],
    c_uno_td [T] (Fraction, None where undefined or absent)."""
    n = len(time)
    assert n <= 8
    w = [1] * n if w is None else [int(x) for x in w]
    e = [bool(x != 0) for x in event]
    y = [float(np.float32(x)) for x in time]
    tv = [float(x) for x in taus(tau)]
    T = len(tv)
    # G at every sample's own time: the product over the distinct times u <= y_i that hold a censoring
    G = []
    for i in range(n):
        g = Fraction(1)
        for u in sorted(set(y[k] for k in range(n) if w[k] > 0)):
            if u > y[i]:
                break
            at_risk = sum(w[k] for k in range(n) if y[k] >= u)
            d = sum(w[k] for k in range(n) if y[k] == u and e[k])
            c = sum(w[k] for k in range(n) if y[k] == u and not e[k])
            if c > 0:
                g *= Fraction(at_risk - d - c, at_risk - d)                       # the events leave before the censorings
        G.append(g)
    K = [[[0, 0, 0] for _ in range(n)] for _ in (RISK, SURV)]
    have = [risk is not None, surv is not None]
    for i in range(n):
        if not e[i]:
            continue
        for j in range(n):
            if not (y[j] > y[i] or (y[j] == y[i] and not e[j])):
                continue
            if have[RISK]:
                a, b = np.float32(risk[i]), np.float32(risk[j])
                K[RISK][i][COMP] += w[j]
                K[RISK][i][CONC] += w[j] * int(a > b)
                K[RISK][i][TIED] += w[j] * int(a == b)
            if have[SURV]:
                a, b = np.float32(surv[i][col[i]]), np.float32(surv[j][col[i]])
                K[SURV][i][COMP] += w[j]
                K[SURV][i][CONC] += w[j] * int(a < b)
                K[SURV][i][TIED] += w[j] * int(a == b)
    counts = [[sum(w[i] * K[s][i][k] for i in range(n)) for k in range(3)] for s in (RISK, SURV)]
    rowcnt = [sum(w), sum(w[i] for i in range(n) if e[i])]
    sums = [[[Fraction(0)] * 3 for _ in range(T)] for _ in (RISK, SURV)]
    for t in range(T):
        rowcnt.append(sum(w[i] for i in range(n) if e[i] and y[i] < tv[t] and G[i] == 0))
        for s in (RISK, SURV):
            sums[s][t] = [sum((Fraction(w[i] * K[s][i][k]) / (G[i] * G[i]) for i in range(n)
                               if e[i] and w[i] > 0 and y[i] < tv[t] and G[i] > 0), Fraction(0)) for k in range(3)]

    def ratio(x, half, ok=True):
        return (Fraction(x[CONC]) + Fraction(half) * x[TIED]) / x[COMP] if ok and x[COMP] > 0 else None
    half = Fraction(1, 2)
    return dict(counts=counts, rowcnt=rowcnt, sums=sums, G=G,
                c_harrell=ratio(counts[RISK], half, have[RISK]), c_td=ratio(counts[SURV], 0, have[SURV]),
                c_td_adj=ratio(counts[SURV], half, have[SURV]),
                c_uno=[ratio(sums[RISK][t], half, have[RISK] and rowcnt[2 + t] == 0) for t in range(T)],
                c_uno_td=[ratio(sums[SURV][t], half, have[SURV] and rowcnt[2 + t] == 0) for t in range(T)])


# ---- seeded cohorts ---------------------------------------------------------------------------------------------------------------------
def cohort(seed, n, p_event=0.5, time_levels=0, Q=3):
    """event, time (float32; `time_levels` > 0: that many distinct values, so ties), risk [n] (rounded to 1 / 8 where there are time
    ties, so that risks tie too), surv [n, Q] and col [n] in [0, Q) (a synthetic matrix: each column is its own ranking, values rounded
    to 1 / 8 so that they tie -- the kernel does not care where a column comes from)."""
    rs = np.random.RandomState(seed)
    tm = rs.rand(n)
    if time_levels:
        tm = np.floor(tm * time_levels) / time_levels
    tm = tm.astype(np.float32)
    ev = (rs.rand(n) < p_event).astype(np.float32)
    risk = rs.randn(n)
    if time_levels:
        risk = np.round(risk * 8) / 8
    surv = (np.round(rs.rand(n, Q) * 8) / 8).astype(np.float32)
    col = rs.randint(0, Q, size=n).astype(np.int32)
    return ev, tm, risk.astype(np.float32), surv, col


def taus_for(tm, T):
    """T truncation times for the times `tm`: below the smallest time, (T = 8:) between two times, equal to a time that is there, some
    quantiles, and last +inf."""
    u = np.unique(tm)
    if T == 1:
        return np.array([u[len(u) // 2]], dtype=np.float32)
    mid = (u[0] + u[min(1, len(u) - 1)]) / 2 if len(u) > 1 else u[0] + 0.5
    base = [u[0] - 1.0, mid, u[len(u) // 2], u[-1], np.quantile(tm, 0.3), np.quantile(tm, 0.8), u[-1] + 1.0, np.inf]
    return np.asarray(base, dtype=np.float32)


def cap_cohort(B=200, seed=0):
    """Five samples, one event (tied with a censoring at the first time): a resample that draws no copy of the event has no comparable
    pair, and one that draws nothing beyond the first time has G = 0 at its only cases. -> dict ev, tm, risk, idx [B, 5]."""
    tm = np.array([1, 1, 2, 3, 4], dtype=np.float32)
    ev = np.array([1, 0, 0, 0, 0], dtype=np.float32)
    risk = np.array([5, 4, 3, 2, 1], dtype=np.float32)
    return dict(ev=ev, tm=tm, risk=risk, idx=np.random.RandomState(seed).randint(0, 5, size=(B, 5)))
