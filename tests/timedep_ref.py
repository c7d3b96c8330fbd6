"""Float64 numpy restatement of advmil_ipcw_rows (include/advmil_hip.h, csrc/timedep.hip) and of what advmil_amd/eval/timedep.py builds
on it, written naively: a weighted row is EXPANDED into repeated samples (`expand`), the two Kaplan-Meier estimates are loops over the
distinct times of the expansion, and every query time forms its cases x controls comparison table.

Rounding bounds, returned alongside the values (n = the cohort's size, before expansion):
  A, B, G, S_KM, Wc, C   relative 4 n 2^-52 (`bound`). Every sum has non-negative terms, at most n of them in the kernel (one per sample,
          weight folded in); every product has at most n factors (one per distinct time), each one correctly rounded quotient of exact
          integers. A term of A or C divides by a G (up to 2n roundings) and takes a handful of roundings of its own; adding at most n
          non-negative terms in ANY order costs another (n - 1) 2^-53 relative. Together below 2 n 2^-52 for the kernel, and as much
          again for this restatement (its sums are math.fsum, its products np.cumprod).
  brier    (A + B / G) / W, all terms non-negative: relative 4 `bound`.
  auc      C / (Wc N_ctrl): relative 3 `bound`.
  ibs      a non-negative combination of Brier scores: relative 4 `bound`.
  mean_auc sum_q auc_q (S_{q-1} - S_q) / (1 - S_{Q-1}) with auc <= 1: every difference of two S carries an ABSOLUTE 2 `bound`, so the
          numerator moves by at most (3 + 2 Q) `bound` and the denominator by `bound`: absolute (2 Q + 5) `bound` / (1 - S_{Q-1}).
Counts and every K_i are integers: equal or wrong."""
import math

import numpy as np

U52 = 2.0 ** -52


def bound(n):
    return 4.0 * n * U52


def expand(w, *arrays):
    """Every array with sample i repeated w[i] times, in sample order."""
    idx = np.repeat(np.arange(len(w)), np.asarray(w, dtype=np.int64))
    return tuple(np.asarray(a)[idx] for a in arrays)


def multiplicities(indices, n):
    idx = np.asarray(indices, dtype=np.int64)
    return np.stack([np.bincount(r, minlength=n) for r in idx]).astype(np.int32)


def km_pair(e, y):
    """e bool [N], y float64 [N] (an expanded row) -> (distinct times u, G(u), S_KM(u)): the censoring estimate with events before
    censorings at a tied time, and the event estimate, both right-continuous."""
    ut = np.unique(y)
    fg, fs = np.ones(ut.size), np.ones(ut.size)
    for b, u in enumerate(ut):
        n_u = int((y >= u).sum())
        d_u = int((e & (y == u)).sum())
        c_u = int((~e & (y == u)).sum())
        if c_u > 0:
            fg[b] = (n_u - d_u - c_u) / (n_u - d_u)
        if d_u > 0:
            fs[b] = (n_u - d_u) / n_u
    return ut, np.cumprod(fg), np.cumprod(fs)


def step(ut, p, t):
    """The right-continuous step function with value p[b] from ut[b] on (1 before ut[0]) at the times t."""
    i = np.searchsorted(ut, t, side="right") - 1
    return np.where(i >= 0, p[np.maximum(i, 0)] if p.size else 1.0, 1.0)


def row(event, time, at, surv=None, risk=None, w=None):
    """One row. event [n], time [n], at [Q]; surv [n, Q] or None; risk [n], [n, 1], [n, Q] or None; w int [n] or None.
    -> dict: counts int64 [Q, 2], rowcnt int64 [2], sums float64 [Q, 6] (A, B, G(at), S_KM(at), Wc, C), bound (relative, of every sum)."""
    n = len(time)
    w = np.ones(n, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64).reshape(-1)
    assert w.size == n and (w >= 0).all()
    at = np.asarray(at, dtype=np.float32).reshape(-1)
    Q = at.size
    S = None if surv is None else np.asarray(surv, dtype=np.float32).reshape(n, Q)
    rho = None if risk is None else np.asarray(risk, dtype=np.float32).reshape(n, -1)
    assert rho is None or rho.shape[1] in (1, Q)
    idx = np.repeat(np.arange(n), w)                                              # the expansion
    e = (np.asarray(event) != 0)[idx]
    y = np.asarray(time, dtype=np.float32).astype(np.float64)[idx]
    ut, G, Skm = km_pair(e, y)
    Gy = step(ut, G, y)
    counts, sums = np.zeros((Q, 2), dtype=np.int64), np.zeros((Q, 6), dtype=np.float64)
    for q in range(Q):
        t = float(at[q])
        case, ctrl = e & (y <= t), y > t
        counts[q] = int(case.sum()), int(ctrl.sum())
        sums[q, 2], sums[q, 3] = step(ut, G, t), step(ut, Skm, t)
        if S is not None:
            s = S[idx, q].astype(np.float64)
            sums[q, 1] = math.fsum((1.0 - s[ctrl]) ** 2)
        if counts[q, 1] == 0:
            continue                                                              # A, Wc, C are written as 0 there
        ig = 1.0 / Gy[case]
        sums[q, 4] = math.fsum(ig)
        if S is not None:
            sums[q, 0] = math.fsum(s[case] ** 2 * ig)
        if rho is not None:
            r = rho[idx, q if rho.shape[1] > 1 else 0]                            # float32: ties are fp32 equality
            ri, rj = r[case][:, None], r[ctrl][None, :]
            K = (2 * (ri > rj).astype(np.int64) + (ri == rj)).sum(axis=1)         # exact
            sums[q, 5] = math.fsum(ig * (K / 2.0))
    return dict(counts=counts, rowcnt=np.array([int(w.sum()), int(w[np.asarray(event) != 0].sum())], dtype=np.int64), sums=sums,
                bound=bound(n))


def rows(event, time, at, surv=None, risk=None, W=None):
    """W [R, n] or None (one row of ones) -> the rows' results stacked: counts [R, Q, 2], rowcnt [R, 2], sums [R, Q, 6]."""
    res = [row(event, time, at, surv, risk, None if W is None else W[r]) for r in range(1 if W is None else len(W))]
    return dict(counts=np.stack([x["counts"] for x in res]), rowcnt=np.stack([x["rowcnt"] for x in res]),
                sums=np.stack([x["sums"] for x in res]), bound=res[0]["bound"])


def statistics(res, at):
    """The statistics of rows (see `rows`) with their bounds: brier, auc [R, Q], ibs, mean_auc [R] (NaN where undefined), b_brier, b_auc,
    b_ibs, b_mean_auc (absolute)."""
    c, s, b = res["counts"], res["sums"], res["bound"]
    t = np.asarray(at, dtype=np.float32).astype(np.float64)
    R, Q = c.shape[0], c.shape[1]
    brier, auc = np.full((R, Q), np.nan), np.full((R, Q), np.nan)
    ibs, mean_auc, b_mean = np.full(R, np.nan), np.full(R, np.nan), np.full(R, np.nan)
    for r in range(R):
        for q in range(Q):
            A, B, G, _, Wc, C = s[r, q]
            if c[r, q, 1] > 0:
                brier[r, q] = (A + B / G) / res["rowcnt"][r, 0]
                if c[r, q, 0] > 0:
                    auc[r, q] = C / (Wc * c[r, q, 1])
        if Q >= 2 and not np.isnan(brier[r]).any():
            ibs[r] = sum(0.5 * (brier[r, q] + brier[r, q + 1]) * (t[q + 1] - t[q]) for q in range(Q - 1)) / (t[-1] - t[0])
        S = s[r, :, 3]
        if not np.isnan(auc[r]).any() and S[-1] < 1.0:
            prev = 1.0
            acc = 0.0
            for q in range(Q):
                acc += auc[r, q] * (prev - S[q])
                prev = S[q]
            mean_auc[r] = acc / (1.0 - S[-1])
            b_mean[r] = (2 * Q + 5) * b / (1.0 - S[-1])
    return dict(brier=brier, auc=auc, ibs=ibs, mean_auc=mean_auc, b_brier=4 * b * brier, b_auc=3 * b * auc, b_ibs=4 * b * ibs,
                b_mean_auc=b_mean)


def default_times(event, time):
    e = np.asarray(event) != 0
    t = np.asarray(time, dtype=np.float32)
    at = np.unique(np.quantile(t[e], np.arange(1, 10) / 10, method="lower").astype(np.float32))
    return at[at < t.max()]


# ---- seeded cohorts ---------------------------------------------------------------------------------------------------------------------
def cohort(seed, n, p_event=0.5, time_levels=0, Q=3, risk_cols=1):
    """event, time (float32; `time_levels` > 0: that many distinct values, so ties), at [Q] (quantiles of the times, so that cases and
    controls both exist at most of them; for Q > 1 the first lies below every time), surv [n, Q] (decreasing along q), risk
    [n, risk_cols] (rounded to 1 / 8 where there are time ties, so that risks tie too)."""
    rs = np.random.RandomState(seed)
    tm = rs.rand(n)
    if time_levels:
        tm = np.floor(tm * time_levels) / time_levels
    tm = tm.astype(np.float32)
    ev = (rs.rand(n) < p_event).astype(np.float32)
    lead = [np.float32(-0.5)] if Q > 1 else []                                    # (Q == 1: the median alone)
    at = np.unique(np.concatenate([lead, np.quantile(tm, np.linspace(0.15, 0.85, max(Q - 1, 1)) if Q > 2 else [0.5], method="lower")])
                   .astype(np.float32))[:Q]
    while at.size < Q:                                                            # (tiny cohorts: fill with times between the others)
        at = np.unique(np.concatenate([at, [at[-1] + np.float32(0.03125)]]).astype(np.float32))
    surv = np.sort(rs.rand(n, Q), axis=1)[:, ::-1].astype(np.float32).copy()
    risk = rs.randn(n, risk_cols)
    if time_levels:
        risk = np.round(risk * 8) / 8
    return ev, tm, at, surv, risk.astype(np.float32)


# the cohorts of tests/golden/timedep_v1.npz (tests/golden/gen_golden_timedep.py records scipy's and scikit-learn's answers on them)
GOLDEN_KM = [dict(seed=11, n=23, p_event=0.6), dict(seed=12, n=50, p_event=0.4), dict(seed=13, n=9, p_event=0.5)]       # no ties at all
GOLDEN_AUC = [dict(seed=21, n=30), dict(seed=22, n=41, levels=8)]                                                        # no censoring


def golden_km_inputs(k):
    """event, time of a cohort without any tie (so none between an event and a censoring)."""
    c = GOLDEN_KM[k]
    rs = np.random.RandomState(c["seed"])
    tm = (rs.permutation(4 * c["n"])[:c["n"]] / np.float32(4.0)).astype(np.float32)      # distinct quarter steps
    ev = (rs.rand(c["n"]) < c["p_event"]).astype(np.float32)
    ev[np.argmin(tm)] = 1.0
    return ev, tm


def golden_auc_inputs(k):
    """time, at, risk [n, 1] of a cohort in which every time is an event; `levels`: tied times and tied risks."""
    c = GOLDEN_AUC[k]
    rs = np.random.RandomState(c["seed"])
    tm = rs.rand(c["n"])
    risk = -tm + 0.5 * rs.randn(c["n"])
    if c.get("levels"):
        tm, risk = np.floor(tm * c["levels"]) / c["levels"], np.round(risk * 4) / 4
    tm = tm.astype(np.float32)
    at = np.unique(np.quantile(tm, [0.2, 0.4, 0.6, 0.8], method="lower").astype(np.float32))
    at = at[at < tm.max()]
    return tm, at, risk.astype(np.float32).reshape(-1, 1)


# ---- the API cohort of tests/test_timedep_gpu.py ----------------------------------------------------------------------------------------
def api_cohort(n=200, seed=0, S=16, bins=4):
    """n patients, about half censored (an exponential event time against an independent exponential censoring time, rounded to 1 / 64),
    a sampled prediction dist [n, S] around the true scale, and for the discrete task bin labels 0 ... bins - 1 of the same times with
    hazards [n, bins]. -> dict of float32 arrays: y [n, 2] (time | event), dist, yd [n, 2] (bin | event), hazards."""
    rs = np.random.RandomState(seed)
    scale = np.exp(0.5 * rs.randn(n))
    te, tc = rs.exponential(scale), rs.exponential(1.0, size=n)
    tm = (np.ceil(np.minimum(te, tc) * 64) / 64).astype(np.float32)
    ev = (te <= tc).astype(np.float32)
    dist = (rs.exponential(1.0, size=(n, S)) * scale[:, None]).astype(np.float32)
    edges = np.quantile(tm, np.arange(1, bins) / bins)
    lab = np.searchsorted(edges, tm, side="left").astype(np.float32)
    hz = (0.05 + 0.5 * rs.rand(n, bins) / scale[:, None].clip(0.5, 2.0)).clip(0.02, 0.95).astype(np.float32)
    return dict(y=np.stack([tm, ev], axis=1), dist=dist, yd=np.stack([lab, ev], axis=1), hazards=hz)


def survival_from_samples(dist, at):
    d, at = np.asarray(dist, dtype=np.float32), np.asarray(at, dtype=np.float32)
    return ((d[:, None, :] > at[None, :, None]).sum(axis=2).astype(np.float32) / np.float32(d.shape[1])).astype(np.float32)
