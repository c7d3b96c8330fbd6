"""Global discrimination beyond the reference's C-index: Uno's C (inverse probability of censoring weighted, truncated at tau; what
scikit-survival's `concordance_index_ipcw` answers) and Antolini's time-dependent concordance of a predicted survival FUNCTION (pycox's
`EvalSurv.concordance_td`), on the device and with bootstrap intervals. Their conventions are restated in include/advmil_hip.h, so that
neither package is needed.

Harrell-type concordance converges to a quantity that depends on how the cohort was censored; Uno's C weights every case by
1 / G(y_i)^2, G the Kaplan-Meier estimate of the censoring distribution OF THE ROW, and removes that dependence. Antolini's concordance
compares S_i(y_i) with S_j(y_i): it ranks by the survival curves, which may cross, not by one number per patient.

The structure is that of eval/timedep.py: a bootstrap resample is a row of integer multiplicities; the sort of the cohort, its tie
blocks, which pairs are comparable and every comparison of two predictions are the same for every row. So the cohort is sorted ONCE and
all rows go through ONE call (advmil_concord_rows, csrc/concord.hip), which leaves per row and source three exact pair counts and per
truncation time three double sums; the statistics are a few numpy operations on them (`statistics_from_rows`).

Uno's C at tau is UNDEFINED where a case before tau has G(y_i) = 0 (an event tied with the censorings that end the row; sksurv raises
there) or where no pair is comparable; the count-based measures where no pair is comparable. Undefined entries are NaN; when the share of
resamples with an undefined statistic exceeds `max_undefined` the bootstrap raises, because an interval conditional on "defined" is not
the interval that was asked for (eval/bootstrap.py gives the same reason). There is no CPU fallback."""
import ctypes
import importlib
import types

import numpy as np
import torch

from .. import _lib
from .bootstrap import _interval, _rows, multiplicities, resample_indices
from .stratify import _device, _p
from .timedep import _pitched

_strat = importlib.import_module(__package__ + ".stratify")      # (the package exports a function of the same name)

MAX_N, MAX_ROWS, MAX_COLUMNS, MAX_TAUS = 1 << 16, 1 << 20, 4096, 8
PAIR_TILE = 256                                                  # advmil_concord_rows_plan's pair tile: the workspace's partial sums
RISK, SURV = 0, 1                                                # the source axis of counts and sums
CONC, TIED, COMP = 0, 1, 2                                       # the last axis


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _taus(tau):
    """tau None (no truncation), a number or up to 8 numbers -> float32 [T]; +inf = no truncation."""
    t = torch.as_tensor([float("inf")] if tau is None else tau, dtype=torch.float32).reshape(-1)
    if not 1 <= t.numel() <= MAX_TAUS:
        raise ValueError(f"tau: {t.numel()} truncation times (1 to {MAX_TAUS})")
    if bool(torch.isnan(t).any()):
        raise ValueError("tau: NaN")
    return t


def concord_rows(event, time, risk=None, surv=None, col=None, tau=None, weights=None):
    """The launch. event [n] (!= 0: observed), time [n]; risk None or [n] (higher = earlier event); surv None or [n, Q] with col int [n]:
    surv[:, col[i]] holds everybody's predicted probability of surviving time[i] (read where event[i] != 0 only, and checked there);
    tau None (no truncation), a number or up to 8 of them; weights None (all ones) or int32 [R, n], >= 0, every row sum below 2^31.
    -> namespace of device tensors: counts int64 [R, 2, 3] (source risk | surv; conc, tied, comp), rowcnt int64 [R, 2 + T] (sum w,
    sum w e, per tau the weight of the cases before it with G = 0), sums float64 [R, 2, T, 3] (include/advmil_hip.h), tau float32 [T],
    has_risk, has_surv, and ldw, lds: the row pitches (elements) the kernel was handed. The slots of an absent source are 0. More rows
    than fit a workspace of `stratify.MAX_ROW_BYTES` go through several launches."""
    event, time = torch.as_tensor(event).reshape(-1), torch.as_tensor(time).reshape(-1)
    n = time.numel()
    if risk is None and surv is None:
        raise ValueError("concord_rows: neither a risk nor a survival matrix to compare by")
    if weights is not None:
        weights = torch.as_tensor(weights)
        if weights.dtype != torch.int32:
            raise ValueError(f"weights: expected int32 multiplicities, got {weights.dtype}")
        if weights.dim() != 2:
            raise ValueError(f"weights: expected [rows, n], got shape {tuple(weights.shape)}")
    if event.numel() != n or (weights is not None and weights.shape[1] != n):
        raise ValueError("Found input variables with inconsistent numbers of samples")
    R = weights.shape[0] if weights is not None else 1
    if not 1 <= n <= MAX_N or not 1 <= R <= MAX_ROWS:
        raise ValueError(f"concord_rows: n = {n} (1 to 2^16), {R} rows (1 to 2^20)")
    tau = _taus(tau)
    T = tau.numel()
    if weights is not None:
        if bool((weights < 0).any()):
            raise ValueError("weights: negative multiplicities")
        if int(weights.sum(dim=1, dtype=torch.int64).max()) >= 1 << 31:
            raise ValueError("weights: a row sums to 2^31 or more")
    if bool(torch.isnan(time.to(torch.float32)).any()):
        raise ValueError("time: NaN")
    rk = s = c = None
    Q = 1
    if risk is not None:
        rk = torch.as_tensor(risk).reshape(-1).to(torch.float32)
        if rk.numel() != n:
            raise ValueError("Found input variables with inconsistent numbers of samples")
        if bool(torch.isnan(rk).any()):
            raise ValueError("risk: NaN")
    if surv is not None:
        s = torch.as_tensor(surv)
        if s.dim() != 2 or s.shape[0] != n:
            raise ValueError("Found input variables with inconsistent numbers of samples")
        Q = s.shape[1]
        if not 1 <= Q <= MAX_COLUMNS:
            raise ValueError(f"surv: {Q} columns (1 to {MAX_COLUMNS})")
        s = s.to(torch.float32)
        if bool(torch.isnan(s).any()):
            raise ValueError("surv: NaN")
        if col is None:
            raise ValueError("surv needs col: the column that holds everybody's survival probability at a sample's own time")
        c = torch.as_tensor(col).reshape(-1)
        if c.numel() != n:
            raise ValueError("Found input variables with inconsistent numbers of samples")
        if c.is_floating_point() or c.dtype == torch.bool:
            raise ValueError(f"col: expected integer column indices, got {c.dtype}")
        observed = (event != 0).to(c.device)
        bad = observed & ((c < 0) | (c >= Q))
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise ValueError(f"col: sample {i} has an observed event and column {int(c[i])}, outside [0, {Q})")
    dev = _device(weights, s, rk, time)
    s = _pitched(s, dev) if s is not None else None
    rk = rk.to(dev).contiguous() if rk is not None else None
    c = c.to(device=dev, dtype=torch.int32).contiguous() if c is not None else None
    if event.dtype == torch.bool:
        event = event.to(torch.float32)
    tm = time.to(device=dev, dtype=torch.float32)
    stime, order = torch.sort(tm, stable=True)                       # the replicate-independent preparation
    sevent = event.to(device=dev, dtype=torch.float32)[order].contiguous()
    order = order.to(torch.int32)
    w = _rows(weights, torch.int32, dev) if weights is not None else None
    ldw = (w.stride(0) if R > 1 else n) if w is not None else 0     # (the stride of a single row is arbitrary)
    lds = (s.stride(0) if n > 1 else Q) if s is not None else 0
    counts = torch.empty((R, 2, 3), dtype=torch.int64, device=dev)
    rowcnt = torch.empty((R, 2 + T), dtype=torch.int64, device=dev)
    sums = torch.empty((R, 2, T, 3), dtype=torch.float64, device=dev)
    taud = tau.to(dev).contiguous()
    L = _lib.lib()
    row_bytes = 8 * n + 8 * -(-n // PAIR_TILE) * (5 + 6 * T)         # R n doubles and the tiles' partial sums
    per = max(1, min(R, _strat.MAX_ROW_BYTES // row_bytes))          # rows per launch
    wsb = L.advmil_concord_rows_workspace_bytes(n, per, T)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for r0 in range(0, R, per):
        k = min(per, R - r0)
        _lib.check(L.advmil_concord_rows(_p(stime), _p(sevent), _p(order), n, _p(w[r0:] if w is not None else None), ldw, k, _p(rk), _p(s),
                                         lds, Q, _p(c), _p(taud), T, _p(counts[r0:]), _p(rowcnt[r0:]), _p(sums[r0:]), _p(ws), wsb, stream),
                   "concord_rows")
    return types.SimpleNamespace(counts=counts, rowcnt=rowcnt, sums=sums, tau=taud, has_risk=rk is not None, has_surv=s is not None,
                                 ldw=ldw, lds=lds, launches=-(-R // per))


def statistics_from_rows(counts, rowcnt, sums, has_risk=True, has_surv=True):
    """counts int64 [..., 2, 3], rowcnt int64 [..., 2 + T], sums float64 [..., 2, T, 3] (numpy or tensors) -> namespace of numpy arrays,
    NaN where undefined or where the source is absent:
      c_harrell [...]     = (conc + tied / 2) / comp of the risk counts                          iff comp > 0
      c_td, c_td_adj [...] = conc / comp, (conc + tied / 2) / comp of the surv counts            iff comp > 0
      c_uno [..., T]      = (conc + tied / 2) / comp of the risk sums of tau[t]                  iff comp > 0 and no case before tau[t] has G = 0
      c_uno_td [..., T]   = the same of the surv sums (Antolini's pairs, Uno's weights)
      n_zero_g [..., T]   = the weight of the cases before tau[t] with G = 0."""
    c = _np(counts)
    rc = _np(rowcnt)
    s = np.asarray(_np(sums), dtype=np.float64)
    zero_g = rc[..., 2:]
    out = types.SimpleNamespace(n_zero_g=zero_g)
    with np.errstate(all="ignore"):
        def ratio(x, half, ok):
            return np.where(ok, (x[..., CONC] + half * x[..., TIED]) / x[..., COMP], np.nan)

        def absent(x):
            return np.full(x.shape, np.nan)
        cr, cs = c[..., RISK, :].astype(np.float64), c[..., SURV, :].astype(np.float64)
        out.c_harrell = ratio(cr, 0.5, c[..., RISK, COMP] > 0)
        out.c_td = ratio(cs, 0.0, c[..., SURV, COMP] > 0)
        out.c_td_adj = ratio(cs, 0.5, c[..., SURV, COMP] > 0)
        out.c_uno = ratio(s[..., RISK, :, :], 0.5, (s[..., RISK, :, COMP] > 0) & (zero_g == 0))
        out.c_uno_td = ratio(s[..., SURV, :, :], 0.5, (s[..., SURV, :, COMP] > 0) & (zero_g == 0))
        if not has_risk:
            out.c_harrell, out.c_uno = absent(out.c_harrell), absent(out.c_uno)
        if not has_surv:
            out.c_td, out.c_td_adj, out.c_uno_td = absent(out.c_td), absent(out.c_td_adj), absent(out.c_uno_td)
    return out


def concordance_ipcw(event, time, risk, tau=None):
    """Uno's C of a risk (higher = earlier event) at the truncation times `tau` (sksurv.metrics.concordance_index_ipcw with the
    censoring distribution estimated on the same cohort and tied_tol = 0). -> namespace: tau float32 [T], c_uno float64 [T] (NaN where
    undefined), c_harrell (the same pairs unweighted), counts int64 [3] (conc, tied, comp), n_zero_g int64 [T]."""
    r = concord_rows(event, time, risk=risk, tau=tau)
    s = statistics_from_rows(r.counts, r.rowcnt, r.sums, True, False)
    return types.SimpleNamespace(tau=_np(r.tau), c_uno=s.c_uno[0], c_harrell=float(s.c_harrell[0]), counts=_np(r.counts)[0, RISK],
                                 n_zero_g=s.n_zero_g[0])


def columns_at_own_times(time, at):
    """The column of the grid `at` [Q] (ascending) that holds a sample's own time, pycox's `idx_at_times` with steps = "post": the last
    grid time at or before time[i], column 0 for a time before the grid. -> int32 numpy [n]."""
    t = torch.as_tensor(time).reshape(-1).to(torch.float32).cpu().numpy()
    a = torch.as_tensor(at).reshape(-1).to(torch.float32).cpu().numpy()
    if a.size == 0 or np.isnan(a).any() or (np.diff(a) < 0).any():
        raise ValueError("at: the grid times must ascend")
    return (np.searchsorted(a, t, side="right") - 1).clip(0, a.size - 1).astype(np.int32)


def concordance_td(event, time, surv, at, method="antolini"):
    """Antolini's time-dependent concordance of surv [n, Q], the predicted survival probabilities on the grid `at` [Q]
    (pycox.evaluation.EvalSurv.concordance_td; a sample's own time is looked up as `columns_at_own_times` does).
    method "antolini": conc / comp; "adj_antolini": (conc + tied / 2) / comp. -> namespace: c_td (NaN without a comparable pair),
    counts int64 [3] (conc, tied, comp)."""
    if method not in ("antolini", "adj_antolini"):
        raise ValueError(f"method: {method!r}, expected 'antolini' or 'adj_antolini'")
    col = columns_at_own_times(time, at)
    surv = torch.as_tensor(surv)
    if surv.dim() != 2 or surv.shape[1] != torch.as_tensor(at).numel():
        raise ValueError(f"surv: expected one column per grid time, got shape {tuple(surv.shape)} for {torch.as_tensor(at).numel()} times")
    r = concord_rows(event, time, surv=surv, col=torch.from_numpy(col))
    s = statistics_from_rows(r.counts, r.rowcnt, r.sums, False, True)
    return types.SimpleNamespace(c_td=float((s.c_td if method == "antolini" else s.c_td_adj)[0]), counts=_np(r.counts)[0, SURV])


def surv_at_own_times(event, time, dist_y_hat=None, hazards=None, chunk=256):
    """What Antolini's concordance needs of a prediction: everybody's survival probability at every observed event time.
    dist_y_hat [n, S]: S sampled times to event per patient -> the share of a patient's samples beyond the time;
    hazards [n, bins] of a discrete-time model, `time` then holds bin indices -> prod_{l <= k} (1 - h_il).
    -> (at float32 numpy [Q]: the distinct event times, ascending; col int32 numpy [n]: `columns_at_own_times(time, at)`; surv float32
    [n, Q] on the device). Built `chunk` columns at a time: the [n, Q, S] comparison of `survival_from_samples` never exists at once.
    More than 4096 distinct event times are refused: round the times (days to weeks) or evaluate a subsample."""
    if (dist_y_hat is None) == (hazards is None):
        raise ValueError("surv_at_own_times: exactly one of dist_y_hat and hazards")
    e = torch.as_tensor(event).reshape(-1).cpu().numpy() != 0
    t = torch.as_tensor(time).reshape(-1).to(torch.float32).cpu().numpy()
    if e.size != t.size:
        raise ValueError("Found input variables with inconsistent numbers of samples")
    if np.isnan(t).any():
        raise ValueError("time: NaN")
    if not e.any():
        raise ValueError("surv_at_own_times: the cohort has no observed event")
    at = np.unique(t[e])
    if at.size > MAX_COLUMNS:
        raise ValueError(f"surv_at_own_times: {at.size} distinct event times, the kernel takes {MAX_COLUMNS} columns; round the times "
                         "or evaluate a subsample")
    col = columns_at_own_times(t, at)
    p = torch.as_tensor(dist_y_hat if hazards is None else hazards)
    if p.dim() != 2 or p.shape[0] != t.size or p.shape[1] < 1:
        raise ValueError(f"{'dist_y_hat' if hazards is None else 'hazards'}: expected [n, S] with n = {t.size}, got shape {tuple(p.shape)}")
    dev = _device(p)
    p = p.to(device=dev, dtype=torch.float32)
    if hazards is not None:
        if (at != np.floor(at)).any() or at.min() < 0 or at.max() >= p.shape[1]:
            raise ValueError(f"time: the event times of a discrete-time model are bin indices in [0, {p.shape[1] - 1}]")
        return at, col, torch.cumprod(1.0 - p, dim=1)[:, torch.from_numpy(at.astype(np.int64)).to(dev)].contiguous()
    surv = torch.empty((t.size, at.size), dtype=torch.float32, device=dev)
    atd = torch.from_numpy(at).to(dev)
    for c0 in range(0, at.size, chunk):
        a = atd[c0:c0 + chunk]
        surv[:, c0:c0 + chunk] = (p[:, None, :] > a[None, :, None]).sum(dim=2).to(torch.float32) / float(p.shape[1])
    return at, col, surv


_NAMES = {"c_uno": "risk", "c_harrell": "risk", "c_td": "surv", "c_td_adj": "surv", "c_uno_td": "surv"}


def bootstrap_concordance(event, time, risk=None, surv=None, col=None, tau=None, n_boot=1000, seed=0, level=0.95, indices=None,
                          max_undefined=0.05):
    """The point estimates and their percentile bootstrap: the cohort and the `n_boot` resamples (`indices` [B, n], default
    bootstrap.resample_indices(n, n_boot, seed): the resamples of the C-index bootstrap) are rows of one call. risk or surv (with col) may
    be None: its statistics are then absent. -> namespace: tau float32 [T]; with risk: c_uno [T], c_harrell; with surv: c_td, c_td_adj,
    c_uno_td [T]; per statistic <name>_samples [B] or [B, T], <name>_lo, <name>_hi (bootstrap._interval: np.nanpercentile at
    50(1 -+ level)); n_undefined: dict statistic -> resamples in which it is undefined (c_uno: at any tau), each capped by
    `max_undefined`."""
    event_t, time_t = torch.as_tensor(event).reshape(-1), torch.as_tensor(time).reshape(-1)
    n = time_t.numel()
    dev = _device(surv if torch.is_tensor(surv) else None, risk if torch.is_tensor(risk) else None, time_t)
    if indices is None:
        indices = resample_indices(n, n_boot, seed)
    W = multiplicities(indices, n, device=dev)
    B = W.shape[0]
    weights = torch.cat([torch.ones((1, n), dtype=torch.int32, device=dev), W])
    r = concord_rows(event_t, time_t, risk=risk, surv=surv, col=col, tau=tau, weights=weights)
    s = statistics_from_rows(r.counts, r.rowcnt, r.sums, r.has_risk, r.has_surv)
    out = types.SimpleNamespace(tau=_np(r.tau), n_undefined={}, launches=r.launches, counts=_np(r.counts)[0])
    for name, source in _NAMES.items():
        if not (r.has_risk if source == "risk" else r.has_surv):
            continue
        v = getattr(s, name)
        point, samples = v[0], v[1:]
        bad = np.isnan(samples) if samples.ndim == 1 else np.isnan(samples).any(axis=1)
        n_undefined = int(bad.sum())
        share = n_undefined / B if B else 0.0
        if share > max_undefined:
            raise ValueError(f"{n_undefined} of {B} bootstrap resamples ({share:.1%}) have no defined {name} "
                             f"(max_undefined = {max_undefined:g})")
        with np.errstate(all="ignore"):
            lo, hi = _interval(samples.T if samples.ndim == 2 else samples, level) if B else (point * np.nan, point * np.nan)
        scalar = samples.ndim == 1
        out.__dict__.update({name: float(point) if scalar else point, name + "_samples": samples,
                             name + "_lo": float(lo) if scalar else lo, name + "_hi": float(hi) if scalar else hi})
        out.n_undefined[name] = n_undefined
    return out
