"""Risk-group stratification: Kaplan-Meier curves with bootstrap bands, the log-rank test with its permutation p-value, and a scan over
cut points with a multiplicity-adjusted p-value -- what is read right after the C-index, on the device.

The structure is that of eval/bootstrap.py. A bootstrap resample is a row of integer multiplicities; a label permutation and a candidate
cut point are each a row of group bits; the event times, their order and their tie blocks are the same for every row. So the cohort is
sorted ONCE (a stable torch.sort on the device) and all rows go through ONE launch (advmil_logrank_rows, csrc/strat.hip), which leaves per
row six exact integer counts, the log-rank sums E1 and V in double, the three curves (group 0, group 1, pooled) at the query times and
their medians. The rows stay in the caller's sample order; the kernel reads them through the sort permutation.

Everything random is documented so that anyone can redo a row with numpy: resamples are `bootstrap.resample_indices(n, n_boot, seed)`,
permutations are `permutation_groups(group, n_perm, seed)`, the scan's are `np.random.RandomState(seed).permutation(n)` in succession.

A row is UNDEFINED where the log-rank statistic does not exist: V == 0, an empty group, or no event. Its z is NaN; when the share of such
rows exceeds `max_undefined` the functions raise, because a distribution conditional on "defined" is not the one that was asked for
(eval/bootstrap.py gives the same reason). There is no CPU fallback."""
import ctypes
import math
import types

import numpy as np
import torch

from .. import _lib
from .bootstrap import _NO_DEVICE, _interval, _risks, _rows, multiplicities, resample_indices

MAX_CUTS = 64
MAX_ROW_BYTES = 256 << 20               # logrank_scan: no [rows, n] array of one launch is larger
_SQRT2 = math.sqrt(2.0)


def _device(*tensors):
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_DEVICE)
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def logrank_rows(event, time, groups, weights=None, at=None):
    """The launch. event [n] (!= 0: observed), time [n]; groups [n] (one row shared by all) or [R, n], 0 / not 0, any integer or bool type;
    weights None (all ones) or int32 [R, n], >= 0, every row sum below 2^31; at None or [Q] ascending query times.
    -> namespace of device tensors: counts int64 [R, 6] (events of group 1, events, size of group 1, size, distinct event times, those
    with more than one at risk), sums float64 [R, 2] (E1, V), km float64 [R, 3, Q] (group 0, group 1, pooled), median float64 [R, 3],
    at float32 [Q], and ldg, ldw: the row pitches (elements) the kernel was handed -- a uint8 `groups` and `weights` with unit stride along n
    are read where they lie, whatever their row pitch; ldg == 0: the shared row."""
    event, time = torch.as_tensor(event).reshape(-1), torch.as_tensor(time).reshape(-1)
    groups = torch.as_tensor(groups)
    n = time.numel()
    if weights is not None:
        weights = torch.as_tensor(weights)
        if weights.dtype != torch.int32:
            raise ValueError(f"weights: expected int32 multiplicities, got {weights.dtype}")
        if weights.dim() != 2:
            raise ValueError(f"weights: expected [rows, n], got shape {tuple(weights.shape)}")
    if groups.dim() not in (1, 2) or groups.is_floating_point() or groups.is_complex():
        raise ValueError(f"groups: expected 0 / 1 in an integer or bool [n] or [rows, n], got {groups.dtype} {tuple(groups.shape)}")
    if not (event.numel() == n == groups.shape[-1]) or (weights is not None and weights.shape[1] != n):
        raise ValueError("Found input variables with inconsistent numbers of samples")
    shared = groups.dim() == 1
    R = weights.shape[0] if (shared and weights is not None) else (1 if shared else groups.shape[0])
    if weights is not None and weights.shape[0] != R:
        raise ValueError(f"groups has {R} rows, weights {weights.shape[0]}")
    if not 1 <= n <= 1 << 20 or not 1 <= R <= 1 << 20:
        raise ValueError(f"logrank_rows: n = {n}, {R} rows (1 to 2^20 each)")
    if weights is not None:
        if bool((weights < 0).any()):
            raise ValueError("weights: negative multiplicities")
        if int(weights.sum(dim=1, dtype=torch.int64).max()) >= 1 << 31:
            raise ValueError("weights: a row sums to 2^31 or more")
    if bool(torch.isnan(time.to(torch.float32)).any()):
        raise ValueError("time: NaN")
    Q = 0
    if at is not None:
        at = torch.as_tensor(at).reshape(-1).to(torch.float32)
        Q = at.numel()
        if Q > 1 << 16:
            raise ValueError(f"at: {Q} query times (0 to 2^16)")
        if Q and (bool(torch.isnan(at).any()) or bool((at[1:] < at[:-1]).any())):
            raise ValueError("at: the query times must ascend")
    dev = _device(weights, groups, time)
    if event.dtype == torch.bool:
        event = event.to(torch.float32)
    tm = time.to(device=dev, dtype=torch.float32)
    stime, order = torch.sort(tm, stable=True)                       # the replicate-independent preparation
    sevent = event.to(device=dev, dtype=torch.float32)[order].contiguous()
    order = order.to(torch.int32)
    # uint8 groups go to the kernel as they are (it reads 0 / not 0), a row pitch included; other types are reduced to 0 / 1 first
    g = groups if groups.dtype == torch.uint8 else (groups != 0).to(torch.uint8)
    g = g.to(dev).contiguous() if shared else _rows(g, torch.uint8, dev)
    w = _rows(weights, torch.int32, dev) if weights is not None else None
    pitch = lambda t: t.stride(0) if t.shape[0] > 1 else n           # noqa: E731  (the stride of a single row is arbitrary)
    counts = torch.empty((R, 6), dtype=torch.int64, device=dev)
    sums = torch.empty((R, 2), dtype=torch.float64, device=dev)
    median = torch.empty((R, 3), dtype=torch.float64, device=dev)
    km = torch.empty((R, 3, Q), dtype=torch.float64, device=dev)
    atd = at.to(dev).contiguous() if Q else None
    L = _lib.lib()
    wsb = L.advmil_logrank_rows_workspace_bytes(n, Q)
    ws = torch.empty((wsb + 3) // 4, dtype=torch.int32, device=dev) if wsb else None
    ldg, ldw = 0 if shared else pitch(g), pitch(w) if w is not None else 0
    _lib.check(L.advmil_logrank_rows(_p(stime), _p(sevent), _p(order), n, _p(g), ldg, _p(w), ldw,
                                     R, _p(atd), Q, _p(counts), _p(sums), _p(km) if Q else None, _p(median), _p(ws), wsb,
                                     ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "logrank_rows")
    return types.SimpleNamespace(counts=counts, sums=sums, km=km, median=median, ldg=ldg, ldw=ldw,
                                 at=atd if Q else torch.empty(0, dtype=torch.float32, device=dev))


def logrank_from_rows(counts, sums):
    """counts int64 [..., 6], sums float64 [..., 2] (numpy or tensors) -> namespace of numpy arrays: z = (O1 - E1) / sqrt(V), chi2 = z^2,
    p = erfc(|z| / sqrt 2) (the two-sided normal p-value = the chi-square one with one degree of freedom), NaN where `undefined`:
    V == 0, an empty group, or no event."""
    c = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    s = sums.cpu().numpy() if torch.is_tensor(sums) else np.asarray(sums, dtype=np.float64)
    O1, ev, n1, n = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    E1, V = s[..., 0], s[..., 1]
    undefined = ~(V > 0) | (n1 == 0) | (n1 == n) | (ev == 0)
    ok = ~undefined
    z = np.full(c.shape[:-1], np.nan, dtype=np.float64)
    z[ok] = (O1[ok] - E1[ok]) / np.sqrt(V[ok])
    p = np.full(z.shape, np.nan, dtype=np.float64)
    p[ok] = [math.erfc(abs(v) / _SQRT2) for v in z[ok].tolist()]
    return types.SimpleNamespace(z=z, chi2=z * z, p=p, undefined=undefined)


def _check_share(n_undefined, total, max_undefined, what):
    share = n_undefined / total if total else 0.0
    if share > max_undefined:
        raise ValueError(f"{n_undefined} of {total} {what} ({share:.1%}) have no defined log-rank statistic "
                         f"(max_undefined = {max_undefined:g})")


def logrank_test(event, time, group):
    """The two-sample log-rank test of group 1 against group 0 (scipy.stats.logrank's statistic with x = group 1).
    -> namespace: z, chi2, p (NaN when `undefined`), counts int64 [6], E1, V."""
    r = logrank_rows(event, time, torch.as_tensor(group).reshape(-1))
    counts, sums = r.counts.cpu().numpy(), r.sums.cpu().numpy()
    s = logrank_from_rows(counts, sums)
    return types.SimpleNamespace(z=float(s.z[0]), chi2=float(s.chi2[0]), p=float(s.p[0]), undefined=bool(s.undefined[0]), counts=counts[0],
                                 E1=float(sums[0, 0]), V=float(sums[0, 1]))


def permutation_groups(group, n_perm, seed):
    """uint8 numpy [n_perm, n]: row p is the p-th successive `rs.permutation(g)` of `rs = np.random.RandomState(seed)`, with
    g = (group != 0) as uint8 in sample order. To redo row p: draw p + 1 permutations from a fresh RandomState(seed), keep the last."""
    g = torch.as_tensor(group).reshape(-1).cpu().numpy() if torch.is_tensor(group) else np.asarray(group).reshape(-1)
    g = (g != 0).astype(np.uint8)
    rs = np.random.RandomState(seed)
    out = np.empty((n_perm, g.size), dtype=np.uint8)
    for p in range(n_perm):
        out[p] = rs.permutation(g)
    return out


def logrank_permutation_test(event, time, group, n_perm=10000, seed=0, max_undefined=0.05):
    """The permutation p-value of the log-rank statistic: the group labels of `permutation_groups(group, n_perm, seed)` and the observed
    ones as one more row, one launch. -> namespace: z, chi2, p (the observed row's, asymptotic), p_perm = (1 + #{|z_p| >= |z|}) /
    (1 + defined permutations), z_perm float64 [n_perm] (NaN where undefined), n_undefined."""
    dev = _device(torch.as_tensor(time))
    g = torch.as_tensor(group).reshape(-1)
    rows = np.concatenate([permutation_groups(g, n_perm, seed), _bits(g)[None]])
    r = logrank_rows(event, time, torch.from_numpy(rows).to(dev))
    s = logrank_from_rows(r.counts, r.sums)
    z_perm, z = s.z[:n_perm], float(s.z[n_perm])
    n_undefined = int(s.undefined[:n_perm].sum())
    _check_share(n_undefined, n_perm, max_undefined, "permutations")
    defined = n_perm - n_undefined
    p_perm = (1 + int((np.abs(z_perm[~s.undefined[:n_perm]]) >= abs(z)).sum())) / (1 + defined) if not s.undefined[n_perm] else float("nan")
    return types.SimpleNamespace(z=z, chi2=float(s.chi2[n_perm]), p=float(s.p[n_perm]), p_perm=p_perm, z_perm=z_perm, n_undefined=n_undefined)


def _bits(group):
    g = group.cpu().numpy() if torch.is_tensor(group) else np.asarray(group)
    return (g.reshape(-1) != 0).astype(np.uint8)


def _order_interval(samples, level):
    """Order statistics (no interpolation: a median may be +inf) at 50(1 -+ level) along the first axis, NaN rows ignored."""
    lo = np.nanpercentile(samples, 50.0 * (1.0 - level), axis=0, method="lower")
    hi = np.nanpercentile(samples, 50.0 * (1.0 + level), axis=0, method="higher")
    return lo, hi


def kaplan_meier(event, time, group=None, at=None, n_boot=0, seed=0, level=0.95, indices=None, max_undefined=0.05):
    """Kaplan-Meier curves of group 0, group 1 and the pooled cohort (`group` None: everyone is group 0) at the times `at` (default: the
    distinct event times), with percentile bootstrap bands: the point estimate and the `n_boot` resamples (`indices` [B, n], default
    bootstrap.resample_indices(n, n_boot, seed): the resamples of the C-index bootstrap) are rows of one launch.
    -> namespace: at float32 [Q], surv float64 [3, Q], median float64 [3] (+inf: never at or below 0.5), counts int64 [6]; with resamples
    also samples [B, 3, Q], lo, hi [3, Q] (np.nanpercentile at 50(1 -+ level)), median_samples [B, 3], median_lo, median_hi [3] (the order
    statistics `method="lower"` / `"higher"` at the same percentiles: no interpolation between a time and +inf), n_undefined. A resample
    that leaves a group of the cohort empty has no curve for it: NaN there, counted in n_undefined and capped by `max_undefined`."""
    event_t, time_t = torch.as_tensor(event).reshape(-1), torch.as_tensor(time).reshape(-1)
    n = time_t.numel()
    dev = _device(time_t, event_t)
    g = torch.zeros(n, dtype=torch.uint8) if group is None else torch.from_numpy(_bits(torch.as_tensor(group)))
    if g.numel() != n or event_t.numel() != n:
        raise ValueError("Found input variables with inconsistent numbers of samples")
    tm = time_t.to(device=dev, dtype=torch.float32)
    if at is None:
        at = torch.unique(tm[event_t.to(dev) != 0])
    if indices is None and n_boot > 0:
        indices = resample_indices(n, n_boot, seed)
    weights = None
    if indices is not None:
        W = multiplicities(indices, n, device=dev)
        weights = torch.cat([torch.ones((1, n), dtype=torch.int32, device=dev), W])
    r = logrank_rows(event_t, tm, g.to(dev), weights, at)
    counts, km, med = r.counts.cpu().numpy(), r.km.cpu().numpy(), r.median.cpu().numpy()
    out = types.SimpleNamespace(at=r.at.cpu().numpy(), surv=km[0], median=med[0], counts=counts[0])
    if weights is None:
        return out
    B = counts.shape[0] - 1
    size = np.stack([counts[:, 3] - counts[:, 2], counts[:, 2], counts[:, 3]], axis=1)       # [1 + B, 3]
    empty = (size[1:] == 0) & (size[:1] > 0)                                                  # a class the cohort has and the resample lacks
    n_undefined = int(empty.any(axis=1).sum())
    _check_share(n_undefined, B, max_undefined, "bootstrap resamples")
    samples, msamples = km[1:].copy(), med[1:].copy()
    samples[empty] = np.nan
    msamples[empty] = np.nan
    absent = size[0] == 0                                                                     # (a class nobody is in: its curve is the constant 1)
    with np.errstate(all="ignore"):
        lo, hi = np.nanpercentile(samples, [50.0 * (1.0 - level), 50.0 * (1.0 + level)], axis=0) if B else (km[0] * np.nan, km[0] * np.nan)
        mlo, mhi = _order_interval(np.where(absent, np.inf, msamples), level) if B else (med[0] * np.nan, med[0] * np.nan)
    out.__dict__.update(samples=samples, lo=lo, hi=hi, median_samples=msamples, median_lo=mlo, median_hi=mhi, n_undefined=n_undefined)
    return out


def risk_groups(risk, q=0.5):
    """High risk (1) is risk > np.quantile(risk, q) (float64 of the fp32 risks, numpy's default linear interpolation); ties with the
    quantile go to the low group. -> (uint8 numpy [n], the threshold)."""
    r = risk.detach().cpu().numpy() if torch.is_tensor(risk) else np.asarray(risk)
    r = r.reshape(-1).astype(np.float32).astype(np.float64)
    if not 0.0 < q < 1.0:
        raise ValueError(f"risk_groups: q = {q} (a quantile strictly between 0 and 1)")
    thr = float(np.quantile(r, q))
    return (r > thr).astype(np.uint8), thr


def stratify_risk(event, time, risk, q=0.5, n_perm=0, n_boot=0, seed=0, level=0.95, max_undefined=0.05):
    """`stratify` for a risk vector that is already formed (what concordance_index_censored takes as its estimate)."""
    risk = torch.as_tensor(risk).reshape(-1)
    dev = _device(risk, torch.as_tensor(time))
    n = risk.numel()
    g, thr = risk_groups(risk, q)
    rows = [g[None]]
    if n_perm > 0:
        rows.append(permutation_groups(g, n_perm, seed))
    weights = None
    if n_boot > 0:
        rows.append(np.broadcast_to(g, (n_boot, n)))
        W = multiplicities(resample_indices(n, n_boot, seed), n, device=dev)
        weights = torch.cat([torch.ones((1 + n_perm, n), dtype=torch.int32, device=dev), W])
    groups = torch.from_numpy(np.concatenate(rows) if len(rows) > 1 else g).to(dev)      # the observed split alone: one shared row
    r = logrank_rows(event, time, groups, weights)
    counts, med = r.counts.cpu().numpy(), r.median.cpu().numpy()
    s = logrank_from_rows(counts, r.sums)
    c = counts[0]
    out = types.SimpleNamespace(threshold=thr, n_low=int(c[3] - c[2]), n_high=int(c[2]), events_low=int(c[1] - c[0]), events_high=int(c[0]),
                                median_low=float(med[0, 0]), median_high=float(med[0, 1]), z=float(s.z[0]), chi2=float(s.chi2[0]),
                                p=float(s.p[0]), p_perm=None, z_lo=None, z_hi=None, z_samples=None, n_undefined=0, n_undefined_perm=0)
    if n_perm > 0:
        zp, up = s.z[1:1 + n_perm], s.undefined[1:1 + n_perm]
        out.n_undefined_perm = int(up.sum())
        _check_share(out.n_undefined_perm, n_perm, max_undefined, "permutations")
        out.p_perm = (1 + int((np.abs(zp[~up]) >= abs(out.z)).sum())) / (1 + n_perm - out.n_undefined_perm) if not s.undefined[0] else float("nan")
    if n_boot > 0:
        zb = s.z[1 + n_perm:]
        out.n_undefined = int(s.undefined[1 + n_perm:].sum())
        _check_share(out.n_undefined, n_boot, max_undefined, "bootstrap resamples")
        with np.errstate(all="ignore"):
            lo, hi = _interval(zb, level)
        out.z_lo, out.z_hi, out.z_samples = float(lo), float(hi), zb
    return out


def stratify(y_true, y_pred, q=0.5, n_perm=0, n_boot=0, seed=0, level=0.95, max_undefined=0.05):
    """Split the cohort at the `q`-quantile of the predicted risk (formed as concordance_index forms it: -prediction of a time, or minus
    the summed survival of discrete hazards) and compare the halves; the observed split, `n_perm` label permutations and `n_boot`
    resamples of the patients (the split kept) are rows of one launch.
    -> namespace: threshold, n_low, n_high, events_low, events_high, median_low, median_high (Kaplan-Meier medians, +inf: not reached),
    z, chi2, p (log-rank, high against low), p_perm, z_lo, z_hi (percentile interval of z over the resamples), z_samples, n_undefined
    (resamples without a statistic), n_undefined_perm."""
    e, t, risk, _ = _risks(y_true, y_pred)
    return stratify_risk(e, t, risk, q, n_perm, n_boot, seed, level, max_undefined)


def logrank_scan(y_true, y_pred, n_cuts=32, min_frac=0.1, n_perm=1000, seed=0):
    """The log-rank z at the quantile cut points q_c = (c + 1) / (n_cuts + 1) of the predicted risk (n_cuts <= 64), those kept whose
    smaller group holds at least `min_frac` of the cohort and whose split differs from the previous one; the cut with the largest |z|;
    and p_adjusted = (1 + #{p: max_c |z_{p,c}| >= max_c |z_c|}) / (1 + n_perm), which answers for having looked at every cut: row (p, c)
    is split c under the p-th successive `np.random.RandomState(seed).permutation(n)` of the samples (G[c][perm]). The permutation x cut
    rows are launched in chunks of at most 256 MB. -> namespace: quantiles, thresholds, n_high [C], z, p [C], best (index into them),
    best_quantile, best_threshold, z_best, p_adjusted, max_abs_z_perm [n_perm]."""
    if not 1 <= n_cuts <= MAX_CUTS:
        raise ValueError(f"logrank_scan: n_cuts = {n_cuts} (1 to {MAX_CUTS})")
    e, t, risk, dev = _risks(y_true, y_pred)
    r64 = risk.cpu().numpy().astype(np.float64)
    n = r64.size
    qs, thrs, G = [], [], []
    for c in range(n_cuts):
        qc = (c + 1) / (n_cuts + 1)
        g, thr = risk_groups(r64, qc)
        k = int(g.sum())
        if min(k, n - k) < min_frac * n or min(k, n - k) == 0 or (G and np.array_equal(G[-1], g)):
            continue
        qs.append(qc), thrs.append(thr), G.append(g)
    if not G:
        raise ValueError(f"logrank_scan: no cut point leaves {min_frac:g} of the cohort in the smaller group")
    G = np.stack(G)
    C = G.shape[0]
    obs = logrank_rows(e, t, torch.from_numpy(G).to(dev))
    s = logrank_from_rows(obs.counts, obs.sums)
    absz = np.abs(s.z)
    if np.isnan(absz).all():
        raise ValueError("logrank_scan: the log-rank statistic is undefined at every cut point")
    best = int(np.nanargmax(absz))
    rs = np.random.RandomState(seed)
    per_chunk = max(1, min(n_perm, MAX_ROW_BYTES // (C * n), (1 << 20) // C)) if n_perm else 0
    zmax = np.full(n_perm, -np.inf)
    for p0 in range(0, n_perm, per_chunk or 1):
        k = min(per_chunk, n_perm - p0)
        rows = np.empty((k, C, n), dtype=np.uint8)
        for p in range(k):
            rows[p] = G[:, rs.permutation(n)]
        r = logrank_rows(e, t, torch.from_numpy(rows.reshape(k * C, n)).to(dev))
        zp = np.abs(logrank_from_rows(r.counts, r.sums).z).reshape(k, C)
        zmax[p0:p0 + k] = np.where(np.isnan(zp).all(axis=1), -np.inf, np.nanmax(np.where(np.isnan(zp), -np.inf, zp), axis=1))
    p_adjusted = (1 + int((zmax >= absz[best]).sum())) / (1 + n_perm)
    return types.SimpleNamespace(quantiles=np.array(qs), thresholds=np.array(thrs), n_high=G.sum(axis=1), z=s.z, p=s.p, best=best,
                                 best_quantile=qs[best], best_threshold=thrs[best], z_best=float(s.z[best]), p_adjusted=p_adjusted,
                                 max_abs_z_perm=zmax)
