"""Two independent restatements of advmil_calib_rows (include/advmil_hip.h, csrc/calib.hip) and of what advmil_amd/eval/calibration.py
builds on it.

(a) `row` / `rows`: float64 numpy, written naively. A weighted row is EXPANDED into repeated samples (`timedep_ref.expand`); the
    Kaplan-Meier curve is re-counted at every grid time from the expansion (`curve`); the pseudo-observation of a censored sample is
    formed by literally DELETING that element from the expanded arrays and integrating the new curve over the full row's grid (one
    deletion per distinct censored time: which of two equal elements is deleted does not change the arrays that remain); a censored
    sample's D-calibration mass is handed to every bin below its own one bin at a time.
(b) `row_exact`: `fractions.Fraction` over the WEIGHTED row (no expansion, the block form of the header: n_v lowered by one for
    v <= k), for n <= 8; with `literal=True` the pseudo-observation is ALSO formed by deletion from the expansion, in exact rationals,
    and asserted equal to the block form. Only the D-calibration bin index is floating point: it is the fp32 product the header names.

Rounding bounds of (a), returned alongside the values as ABSOLUTE numbers (`b_km`, `b_err`, `b_dcal`); they are the header's bounds
for the kernel, which (a) meets as well: its sums are math.fsum (one rounding), its products np.cumprod over correctly rounded
quotients ((2n - 1) 2^-53 relative), so it is inside the header's derivation term by term. A test allows the sum of the two, i.e.
twice these; against (b), which has no error, once these plus one rounding of the conversion to float.
  theta, S                  2 n 2^-52 relative
  hinge, margin numerator   5 n 2^-52 sum w (m + |gamma| + |y|), m the surrogate (t for the hinge); denominator 2 n 2^-52 N (margin), 0 (hinge)
  pseudo-obs numerator      2^-52 n (8 N u_K sum_{e=0} w + 5 sum w (|s| + |y|)), s the surrogate
  D-calibration mass        (n + B + 4) 2^-52 N
Counts are integers: equal or wrong."""
import math
from fractions import Fraction

import numpy as np

from tests.timedep_ref import U52, expand, multiplicities  # noqa: F401

HINGE, MARGIN, PO = 0, 1, 2
NUM, DEN = 0, 1


def curve(e, y, grid):
    """e bool [N], y float64 [N], grid ascending [K] -> S on the grid: prod_{x <= v} (1 - d_x / n_x), n and d re-counted at every grid
    time from the arrays given (by binary search in their sorted copies: #{y >= u}, #{e, y == u}); a grid time at which nobody is at
    risk or nobody dies is a factor of 1."""
    grid = np.asarray(grid, dtype=np.float64)
    ys, es = np.sort(y), np.sort(y[e])
    n_u = len(ys) - np.searchsorted(ys, grid, side="left")
    d_u = np.searchsorted(es, grid, side="right") - np.searchsorted(es, grid, side="left")
    f = np.where((n_u > 0) & (d_u > 0), (n_u - d_u) / np.maximum(n_u, 1), 1.0)
    return np.cumprod(f)


def restricted_mean(S, grid):
    """sum_v S(u_{v-1}) (u_v - u_{v-1}), u_0 = 0, S(u_0) = 1."""
    prev_s = np.concatenate([[1.0], S[:-1]])
    prev_u = np.concatenate([[0.0], grid[:-1]])
    return math.fsum(prev_s * (grid - prev_u))


def bins_of(p, B):
    """min(B - 1, (int)(p * (float)B)), the product in fp32."""
    p = np.asarray(p, dtype=np.float32)
    return np.minimum(B - 1, (p * np.float32(B)).astype(np.int64))


def row(event, time, pred=None, p_own=None, bins=10, gamma=0.0, w=None, po=True):
    """One row. event [n], time [n]; pred [n, P] or None; p_own [n] or None; w int [n] or None.
    -> dict: rowcnt int64 [4], km float64 [3], err float64 [P, 3, 2], dcal float64 [bins], and the absolute bounds b_km [3],
    b_err [P, 3, 2], b_dcal (one number); m, s: the margin and pseudo-observation surrogates of the expanded samples, idx: the
    expansion."""
    n = len(time)
    w = np.ones(n, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64).reshape(-1)
    assert w.size == n and (w >= 0).all() and (pred is not None or p_own is not None)
    Y = None if pred is None else np.asarray(pred, dtype=np.float32).reshape(n, -1).astype(np.float64)
    P = 1 if Y is None else Y.shape[1]
    g = float(np.float32(gamma))
    idx = np.repeat(np.arange(n), w)                                              # the expansion
    N = idx.size
    e = (np.asarray(event) != 0)[idx]
    y = np.asarray(time, dtype=np.float32).astype(np.float64)[idx]
    rowcnt = np.array([N, int(e.sum()), 0, 0], dtype=np.int64)
    km, err, dcal = np.array([0.0, 1.0, 0.0]), np.zeros((P, 3, 2)), np.zeros(bins)
    b_err = np.zeros((P, 3, 2))
    m, s = y.copy(), y.copy()
    if N:
        ut = np.unique(y)
        S = curve(e, y, ut)
        theta = restricted_mean(S, ut)
        rowcnt[2] = ut.size
        km[:] = theta, S[-1], ut[-1]
        blk = np.searchsorted(ut, y)
        Sy = S[blk]
        omega = np.where(e, 1.0, 1.0 - Sy)
        rowcnt[3] = int((~e & (Sy == 0)).sum())
        prev_s, prev_u = np.concatenate([[1.0], S[:-1]]), np.concatenate([[0.0], ut[:-1]])
        terms = prev_s * (ut - prev_u)
        deleted = {}
        for i in np.flatnonzero(~e):
            k = blk[i]
            if Sy[i] > 0:
                m[i] = y[i] + math.fsum(terms[k + 1:]) / Sy[i]
            if po:
                if k not in deleted:                                              # delete element i, keep the full row's grid
                    e2, y2 = np.delete(e, i), np.delete(y, i)
                    deleted[k] = N * theta - (N - 1) * restricted_mean(curve(e2, y2, ut), ut)
                s[i] = deleted[k]
        if Y is not None:
            Ye = Y[idx]
            wc = float((~e).sum())
            for c in range(P):
                yc = Ye[:, c]
                hinge = np.where(e, np.abs(y - yc), np.maximum(0.0, y + g - yc))
                err[c, HINGE] = math.fsum(hinge), N
                err[c, MARGIN] = math.fsum(omega * np.abs(m - yc)), math.fsum(omega)
                b_err[c, HINGE] = 5 * n * U52 * math.fsum(y + abs(g) + np.abs(yc)), 0.0
                b_err[c, MARGIN] = 5 * n * U52 * math.fsum(m + abs(g) + np.abs(yc)), 2 * n * U52 * N
                if po:
                    err[c, PO] = math.fsum(omega * np.abs(s - yc)), err[c, MARGIN, DEN]
                    b_err[c, PO] = U52 * n * (8 * N * ut[-1] * wc + 5 * math.fsum(np.abs(s) + np.abs(yc))), 2 * n * U52 * N
        if p_own is not None:
            p32 = np.asarray(p_own, dtype=np.float32).reshape(n)[idx]
            p = p32.astype(np.float64)
            kb = bins_of(p32, bins)
            parts = [[] for _ in range(bins)]
            for i in range(N):
                if e[i]:
                    parts[kb[i]].append(1.0)
                elif p[i] > 0:
                    parts[kb[i]].append((p[i] - kb[i] / bins) / p[i])
                    for j in range(kb[i]):                                        # every bin below, one at a time
                        parts[j].append(1.0 / (bins * p[i]))
                else:
                    parts[0].append(1.0)
            dcal = np.array([math.fsum(x) for x in parts])
    b_km = np.array([2 * n * U52 * km[0], 2 * n * U52 * km[1], 0.0])
    return dict(rowcnt=rowcnt, km=km, err=err, dcal=dcal, b_km=b_km, b_err=b_err, b_dcal=(n + bins + 4) * U52 * N, m=m, s=s, idx=idx)


def rows(event, time, pred=None, p_own=None, bins=10, gamma=0.0, W=None, po=True):
    """W [R, n] or None (one row of ones) -> the rows' results stacked: rowcnt [R, 4], km [R, 3], err [R, P, 3, 2], dcal [R, bins] and
    b_km, b_err, b_dcal [R]."""
    res = [row(event, time, pred, p_own, bins, gamma, None if W is None else W[r], po) for r in range(1 if W is None else len(W))]
    return {k: np.stack([np.asarray(x[k]) for x in res]) for k in ("rowcnt", "km", "err", "dcal", "b_km", "b_err", "b_dcal")}


def chi2_sf(x, df):
    """The upper tail of chi-square with `df` degrees, by the series / continued fraction of the regularised incomplete gamma function
    (Numerical Recipes' gser / gcf): a third route, next to torch.special.gammaincc and scipy."""
    a, x = df / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1:
        term = total = 1.0 / a
        k = a
        for _ in range(10000):
            k += 1
            term *= x / k
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        return 1.0 - total * math.exp(-x + a * math.log(x) - lg)
    b = x + 1 - a
    c = 1e300
    d = 1 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = 1e-300 if abs(d) < 1e-300 else d
        c = b + an / c
        c = 1e-300 if abs(c) < 1e-300 else c
        d = 1 / d
        de = d * c
        h *= de
        if abs(de - 1) < 1e-17:
            break
    return math.exp(-x + a * math.log(x) - lg) * h


def statistics(res, has_pred=True, has_p=True):
    """The statistics of rows (see `rows`): mae_hinge, mae_margin, mae_po [R, P] (NaN where the denominator is 0 or the source absent),
    d_cal_chi2 [R], d_cal_bins [R, B], and b_<name>: the absolute bound of each for a comparison of the kernel's statistic with this
    one (both sides' bounds: a ratio num / den moves by (b_num + ratio b_den) / den on either side, plus the division's rounding)."""
    err, dc, N = res["err"], res["dcal"], res["rowcnt"][:, 0].astype(np.float64)
    out = {}
    with np.errstate(all="ignore"):
        for j, name in ((HINGE, "mae_hinge"), (MARGIN, "mae_margin"), (PO, "mae_po")):
            num, den = err[:, :, j, NUM], err[:, :, j, DEN]
            ok = (den > 0) & has_pred
            out[name] = np.where(ok, num / den, np.nan)
            out["b_" + name] = np.where(ok, 2 * (res["b_err"][:, :, j, NUM] + np.abs(num / den) * res["b_err"][:, :, j, DEN]) / den
                                        + 2 * U52 * np.abs(num / den), np.nan)
        B = dc.shape[1]
        exp = (N / B)[:, None]
        ok = (N > 0) & has_p
        out["d_cal_chi2"] = np.where(ok, ((dc - exp) ** 2 / exp).sum(axis=1), np.nan)
        out["b_d_cal_chi2"] = np.where(ok, 2 * (2 * np.abs(dc - exp) / exp).sum(axis=1) * res["b_dcal"] + (B + 4) * U52 * out["d_cal_chi2"], np.nan)
        out["d_cal_bins"] = np.where(ok[:, None], dc / N[:, None], np.nan)
        out["b_d_cal_bins"] = np.where(ok, 2 * res["b_dcal"] / N + 2 * U52, np.nan)
    return out


# ---- (b) exact rationals --------------------------------------------------------------------------------------------------------------
def _km_exact(items, grid, lowered_through=None):
    """items: [(time, event, weight)], grid ascending -> [S(u_v)] as Fractions; `lowered_through` = k: every n_v with v <= k is one less
    (a factor whose lowered n_v is 0 is 1)."""
    S, run = [], Fraction(1)
    for v, u in enumerate(grid):
        n_u = sum(wt for (t, _, wt) in items if t >= u)
        d_u = sum(wt for (t, ev, wt) in items if t == u and ev)
        if lowered_through is not None and v <= lowered_through:
            n_u -= 1
        if n_u > 0 and d_u > 0:
            run *= Fraction(n_u - d_u, n_u)
        S.append(run)
    return S


def _rmean_exact(S, grid):
    total, prev_s, prev_u = Fraction(0), Fraction(1), Fraction(0)
    for sv, u in zip(S, grid):
        total += prev_s * (Fraction(u) - prev_u)
        prev_s, prev_u = sv, Fraction(u)
    return total


def row_exact(event, time, pred=None, p_own=None, bins=10, gamma=0.0, w=None, po=True, literal=False):
    """The same row in exact arithmetic, on the weighted samples themselves (n <= 8). -> dict: rowcnt [4] (int), km [3], err [P][3][2],
    dcal [bins] (Fractions), m, s: the surrogates per sample (Fraction; None where the weight is 0)."""
    n = len(time)
    assert n <= 8
    w = [1] * n if w is None else [int(x) for x in w]
    e = [bool(x != 0) for x in event]
    y = [Fraction(float(np.float32(x))) for x in time]
    g = Fraction(float(np.float32(gamma)))
    Y = None if pred is None else [[Fraction(float(v)) for v in r] for r in np.asarray(pred, dtype=np.float32).reshape(n, -1)]
    P = 1 if Y is None else len(Y[0])
    N = sum(w)
    items = [(y[i], e[i], w[i]) for i in range(n)]
    grid = sorted(set(y[i] for i in range(n) if w[i] > 0))
    K = len(grid)
    S = _km_exact(items, grid)
    theta = _rmean_exact(S, grid)
    zero = Fraction(0)
    rowcnt = [N, sum(w[i] for i in range(n) if e[i]), K, 0]
    km = [theta, S[-1] if K else Fraction(1), grid[-1] if K else zero]
    m, s, omega = [None] * n, [None] * n, [None] * n
    for i in range(n):
        if w[i] == 0:
            continue
        if e[i]:
            m[i], s[i], omega[i] = y[i], y[i], Fraction(1)
            continue
        k = grid.index(y[i])
        prev = [Fraction(1)] + S[:-1]
        A = sum((prev[v] * (grid[v] - (grid[v - 1] if v else zero)) for v in range(k + 1, K)), zero)
        m[i] = y[i] + A / S[k] if S[k] > 0 else y[i]
        omega[i] = 1 - S[k]
        if S[k] == 0:
            rowcnt[3] += w[i]
        s[i] = y[i]
        if po:
            s[i] = N * theta - (N - 1) * _rmean_exact(_km_exact(items, grid, lowered_through=k), grid)
            if literal:                                                           # one copy of sample i leaves the expanded arrays
                less = [(y[j], e[j], w[j] - (1 if j == i else 0)) for j in range(n)]
                by_deletion = N * theta - (N - 1) * _rmean_exact(_km_exact(less, grid), grid)
                assert by_deletion == s[i], (i, by_deletion, s[i])
    err = [[[zero, zero] for _ in range(3)] for _ in range(P)]
    if Y is not None:
        live = [i for i in range(n) if w[i] > 0]
        for c in range(P):
            err[c][HINGE] = [sum((w[i] * (abs(y[i] - Y[i][c]) if e[i] else max(zero, y[i] + g - Y[i][c])) for i in live), zero), Fraction(N)]
            den = sum((w[i] * omega[i] for i in live), zero)
            err[c][MARGIN] = [sum((w[i] * omega[i] * abs(m[i] - Y[i][c]) for i in live), zero), den]
            if po:
                err[c][PO] = [sum((w[i] * omega[i] * abs(s[i] - Y[i][c]) for i in live), zero), den]
    dcal = [zero] * bins
    if p_own is not None:
        p32 = np.asarray(p_own, dtype=np.float32).reshape(n)
        kb = bins_of(p32, bins)
        for i in range(n):
            p, k = Fraction(float(p32[i])), int(kb[i])
            if e[i]:
                dcal[k] += w[i]
            elif p > 0:
                dcal[k] += w[i] * (p - Fraction(k, bins)) / p
                for j in range(k):
                    dcal[j] += Fraction(w[i]) / (bins * p)
            else:
                dcal[0] += w[i]
    return dict(rowcnt=rowcnt, km=km, err=err, dcal=dcal, m=m, s=s)


# ---- seeded cohorts ---------------------------------------------------------------------------------------------------------------------
def cohort(seed, n, p_event=0.5, time_levels=0, P=2, bins=10):
    """event, time (float32, > 0; `time_levels` > 0: that many distinct values, so ties), pred [n, P] (the time with noise, some below
    and some beyond it), p_own [n] in [0, 1] (a few exactly 0, exactly 1 and exactly on a bin edge)."""
    rs = np.random.RandomState(seed)
    tm = rs.rand(n) * 4 + 0.25
    if time_levels:
        tm = np.ceil(tm * time_levels / 4.25) * (4.25 / time_levels)
    tm = tm.astype(np.float32)
    ev = (rs.rand(n) < p_event).astype(np.float32)
    pred = (tm[:, None] * np.exp(0.5 * rs.randn(n, P))).astype(np.float32)
    p = rs.rand(n).astype(np.float32)
    edge = rs.rand(n) < 0.2
    p[edge] = (rs.randint(0, bins + 1, size=int(edge.sum())) / np.float32(bins)).astype(np.float32)
    return ev, tm, pred, p


def boot_cohort(n=60, seed=1):
    """The bootstrap test's cohort: n samples with ALTERNATING events, times on a grid of 16 values (ties), two prediction columns and a
    p_own."""
    rs = np.random.RandomState(seed)
    tm = (np.ceil(rs.rand(n) * 16) / 4).astype(np.float32)
    ev = (np.arange(n) % 2 == 0).astype(np.float32)
    pred = (tm[:, None] * np.exp(0.4 * rs.randn(n, 2))).astype(np.float32)
    p = rs.rand(n).astype(np.float32)
    return ev, tm, pred, p
