"""Float64 numpy restatement of advmil_logrank_rows (include/advmil_hip.h, csrc/strat.hip) and of what advmil_amd/eval/stratify.py
builds on it: the six exact counts, E1 and V of the log-rank test, z, the Kaplan-Meier products at query times and the medians, for a
row of group bits and integer weights. A weighted row is BY DEFINITION the unweighted computation on the expanded arrays (`expand`);
`row` evaluates the weighted formulas directly and tests/test_stratify_cpu.py pins the two against each other, bit for bit (the counts
are integers either way, so the floating-point operations are the same).

Rounding bounds, returned alongside each value (m = number of distinct event times of the row, u = 2^-53):
  E1, V   2 (m + 4) 2^-52 sum|terms|: a term is a few correctly rounded operations on exact integers (two for E1: d n1 rounded, / n; the
          quotient form of V has six, each relative u, together below 4 * 2u), a sum of m terms in ANY order adds at most (m - 1) u
          sum|terms|; all of it doubled because this restatement rounds too.
  km      relative 4 m 2^-53: a factor (n - d) / n is one rounding of exact integers, a product of at most m factors in any order has at
          most 2m - 1 roundings; doubled for the restatement's own.
  z       propagated to first order from the two above through z = (O1 - E1) / sqrt(V), with V taken at its lower end, plus 8u |z| for the
          subtraction, the square root and the division on either side.
Medians are times of the data: equal or wrong."""
import math

import numpy as np

U52, U53 = 2.0 ** -52, 2.0 ** -53
CLASSES = ("group0", "group1", "pooled")


def expand(w, *arrays):
    """Every array with sample i repeated w[i] times, in sample order."""
    idx = np.repeat(np.arange(len(w)), np.asarray(w, dtype=np.int64))
    return tuple(np.asarray(a)[idx] for a in arrays)


def multiplicities(indices, n):
    idx = np.asarray(indices, dtype=np.int64)
    return np.stack([np.bincount(r, minlength=n) for r in idx]).astype(np.int32)


class Cohort:
    """What every row shares: the distinct times and the block of each sample."""

    def __init__(self, event, time):
        self.event = np.asarray(event) != 0
        self.time = np.asarray(time, dtype=np.float32).astype(np.float64)
        self.ut, self.inv = np.unique(self.time, return_inverse=True)
        self.n = self.time.size

    def _block(self, x):
        return np.bincount(self.inv, weights=x.astype(np.float64), minlength=self.ut.size).astype(np.int64)      # exact below 2^53

    def row(self, group, weights=None, at=None):
        """-> dict: counts int64 [6], E1, V, bE1, bV (bounds), z, bz, km float64 [3, Q], bkm (relative), median float64 [3], m."""
        g = np.asarray(group).reshape(-1) != 0
        w = np.ones(self.n, dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64).reshape(-1)
        assert g.size == self.n == w.size and (w >= 0).all()
        e = self.event
        tot, tot1 = self._block(w), self._block(w * g)
        d, d1 = self._block(w * e), self._block(w * (e & g))
        nj = tot[::-1].cumsum()[::-1]                                         # at risk: everything at or after the block
        n1 = tot1[::-1].cumsum()[::-1]
        hit = d > 0
        dj, nn, nn1, dd1 = d[hit].astype(np.float64), nj[hit].astype(np.float64), n1[hit].astype(np.float64), d1[hit]
        t_e1 = dj * nn1 / nn
        big = nn > 1
        t_v = (nn1[big] / nn[big]) * ((nn[big] - nn1[big]) / nn[big]) * dj[big] * ((nn[big] - dj[big]) / (nn[big] - 1.0))
        m = int(hit.sum())
        E1, V = math.fsum(t_e1), math.fsum(t_v)
        bE1, bV = 2 * (m + 4) * U52 * math.fsum(np.abs(t_e1)), 2 * (m + 4) * U52 * math.fsum(np.abs(t_v))
        counts = np.array([int((w * (e & g)).sum()), int((w * e).sum()), int((w * g).sum()), int(w.sum()), m, int(big.sum())], dtype=np.int64)
        out = dict(counts=counts, E1=E1, V=V, bE1=bE1, bV=bV, m=m)
        out["z"], out["bz"], out["undefined"] = z_of(counts, E1, V, bE1, bV)
        # the curves: group 0, group 1, pooled
        dc = (d - d1, d1, d)
        nc = (nj - n1, n1, nj)
        q_at = np.zeros(0) if at is None else np.asarray(at, dtype=np.float32).astype(np.float64)
        last = np.searchsorted(self.ut, q_at, side="right") - 1                # the last block at or before each query
        km = np.ones((3, q_at.size), dtype=np.float64)
        med = np.full(3, np.inf)
        for c in range(3):
            f = np.ones(self.ut.size, dtype=np.float64)
            on = dc[c] > 0
            f[on] = (nc[c][on] - dc[c][on]).astype(np.float64) / nc[c][on].astype(np.float64)
            cp = np.cumprod(f)
            km[c] = np.where(last >= 0, cp[np.maximum(last, 0)], 1.0)
            below = np.nonzero(cp <= 0.5)[0]
            if below.size:
                med[c] = self.ut[below[0]]
        out.update(km=km, bkm=4 * max(m, 1) * U53, median=med, at=q_at)
        return out

    def rows(self, groups, weights=None, at=None):
        """groups [R, n] or [n] (shared), weights [R, n] or None -> the rows' results stacked: counts [R, 6], E1, V, z, ... [R], km [R, 3, Q]."""
        groups = np.asarray(groups)
        R = groups.shape[0] if groups.ndim == 2 else (1 if weights is None else np.asarray(weights).shape[0])
        res = [self.row(groups[r] if groups.ndim == 2 else groups, None if weights is None else weights[r], at) for r in range(R)]
        return {k: np.stack([np.asarray(x[k]) for x in res]) for k in res[0]}


def z_of(counts, E1, V, bE1=0.0, bV=0.0):
    """-> (z, its bound, undefined) of one row."""
    O1, ev, n1, n = (int(counts[i]) for i in range(4))
    if not V > 0 or n1 == 0 or n1 == n or ev == 0:
        return float("nan"), float("nan"), True
    z = (O1 - E1) / math.sqrt(V)
    v_lo = V - bV
    bz = bE1 / math.sqrt(v_lo) + (abs(O1 - E1) + bE1) * bV / (2.0 * v_lo ** 1.5) + 8 * U53 * abs(z)
    return z, bz, False


def p_of(z):
    return math.erfc(abs(z) / math.sqrt(2.0))


# ---- seeded cohorts ---------------------------------------------------------------------------------------------------------------------
def cohort(seed, n, p_event=0.5, time_levels=0, weighted=False):
    """event, time (float32; `time_levels` > 0: that many distinct values, so ties), group (uint8), weights (int32 bootstrap draw or None)."""
    rs = np.random.RandomState(seed)
    tm = rs.rand(n)
    if time_levels:
        tm = np.floor(tm * time_levels) / time_levels
    ev = (rs.rand(n) < p_event).astype(np.float32)
    g = (rs.rand(n) < 0.5).astype(np.uint8)
    w = multiplicities(rs.randint(0, n, size=(1, n)), n)[0] if weighted else None
    return ev, tm.astype(np.float32), g, w


# the cohorts of tests/golden/logrank_v1.npz (tests/golden/gen_golden_logrank.py records scipy's answers on their expansions)
GOLDEN_CASES = [dict(seed=1, n=17, p_event=0.6, time_levels=6), dict(seed=2, n=40, p_event=0.5), dict(seed=3, n=12, p_event=0.7, weighted=True),
                dict(five=True), dict(seed=5, n=64, p_event=0.3, time_levels=20, weighted=True), dict(seed=6, n=33, p_event=0.9, time_levels=4)]


def golden_inputs(k):
    c = GOLDEN_CASES[k]
    if c.get("five"):                        # the last sample at risk is an event (n_j == 1), and so is group 0's own last sample
        return (np.array([1, 0, 1, 0, 1], dtype=np.float32), np.array([1, 2, 3, 4, 5], dtype=np.float32), np.array([1, 0, 1, 0, 0], dtype=np.uint8),
                None)
    return cohort(**c)


# ---- the API cohort of tests/test_stratify_gpu.py ---------------------------------------------------------------------------------------
def api_cohort(n, seed=0):
    """n samples, 50 % events, times rounded to 0.05, a prediction of the time with noise: y [n, 2] (time | event), pred [n, 1]."""
    rs = np.random.RandomState(seed)
    tm = (np.round(rs.rand(n) * 20) / 20).astype(np.float32)
    ev = np.zeros(n, dtype=np.float32)
    ev[rs.permutation(n)[:n // 2]] = 1.0
    pred = (tm - rs.randn(n)).astype(np.float32)          # the risk the product ranks by is -pred = randn - t
    return np.stack([tm, ev], axis=1), pred.reshape(-1, 1)


def risk_groups(risk, q=0.5):
    r = np.asarray(risk, dtype=np.float32).astype(np.float64)
    thr = np.quantile(r, q)
    return (r > thr).astype(np.uint8), thr
