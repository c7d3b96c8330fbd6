"""Time-dependent evaluation of a predicted survival FUNCTION: the IPCW Brier score of Graf et al. with its integral (IBS), and the
cumulative/dynamic AUC(t) of Uno et al. and Hung & Chiang with its mean -- calibration and discrimination over time, what scikit-survival's
`brier_score`, `integrated_brier_score` and `cumulative_dynamic_auc` answer (its conventions are restated in include/advmil_hip.h, so that
no sksurv is needed), on the device and with bootstrap intervals.

The structure is that of eval/bootstrap.py and eval/stratify.py. A bootstrap resample is a row of integer multiplicities; the sort of the
cohort by time, its tie blocks, the cases and controls of a query time and every comparison of two risks are the same for every row. So
the cohort is sorted ONCE and all rows go through ONE launch (advmil_ipcw_rows, csrc/timedep.hip), which leaves per row and query time
two exact integer counts and six double sums; the statistics are a few numpy operations on them (`statistics_from_rows`).
IPCW = inverse probability of censoring weighting: an observed event counts 1 / G(y_i) times, G the Kaplan-Meier estimate of the
censoring distribution OF THE ROW (a resample re-estimates it, as refitting sksurv on the resampled arrays would).

BS(t) is UNDEFINED where nobody of the row is beyond t, AUC(t) also where the row has no event at or before t; IBS and the mean AUC need
every BS(t) resp. AUC(t) of the row. Undefined entries are NaN; when the share of resamples with an undefined statistic exceeds
`max_undefined` the bootstrap raises, because an interval conditional on "defined" is not the interval that was asked for
(eval/bootstrap.py gives the same reason). There is no CPU fallback."""
import ctypes
import importlib
import types

import numpy as np
import torch

from .. import _lib
from .bootstrap import _NO_DEVICE, _interval, _rows, multiplicities, resample_indices  # noqa: F401
from .stratify import _device, _p

_strat = importlib.import_module(__package__ + ".stratify")      # (the package exports a function of the same name)

MAX_N, MAX_ROWS, MAX_QUERIES = 1 << 16, 1 << 20, 4096


def survival_from_samples(dist_y_hat, at):
    """dist_y_hat [n, S]: S sampled times to event per patient (`test_model(times_test_sample=S)`); at [Q].
    -> float32 [n, Q] on the device: the share of a patient's samples beyond at[q], #{s: y_is > at[q]} / S."""
    d = torch.as_tensor(dist_y_hat)
    if d.dim() != 2 or d.shape[1] < 1:
        raise ValueError(f"dist_y_hat: expected [n, S] with S >= 1, got shape {tuple(d.shape)}")
    dev = _device(d)
    d = d.to(device=dev, dtype=torch.float32)
    at = torch.as_tensor(at).reshape(-1).to(device=dev, dtype=torch.float32)
    return (d[:, None, :] > at[None, :, None]).sum(dim=2).to(torch.float32) / float(d.shape[1])


def survival_from_hazards(hazards, at=None):
    """hazards [n, bins] of a discrete-time model; at: bin indices (default 0 ... bins - 2; one bin: [0]).
    -> float32 [n, Q] on the device: prod_{l <= k} (1 - h_il) at k = at[q]."""
    h = torch.as_tensor(hazards)
    if h.dim() != 2 or h.shape[1] < 1:
        raise ValueError(f"hazards: expected [n, bins], got shape {tuple(h.shape)}")
    dev = _device(h)
    bins = h.shape[1]
    k = torch.arange(max(bins - 1, 1), device=dev) if at is None else torch.as_tensor(at).reshape(-1).to(dev)
    if k.is_floating_point():
        if bool((k != torch.floor(k)).any()):
            raise ValueError("at: bin indices are whole numbers")
        k = k.to(torch.int64)
    if k.numel() and (int(k.min()) < 0 or int(k.max()) >= bins):
        raise ValueError(f"at: bin indices outside [0, {bins - 1}]")
    return torch.cumprod(1.0 - h.to(device=dev, dtype=torch.float32), dim=1)[:, k.to(torch.int64)].contiguous()


def default_times(event, time):
    """The query times when the caller gives none: the deciles 0.1 ... 0.9 of the observed event times (np.quantile, method="lower": times
    of the data), de-duplicated, those at or beyond the largest time of the cohort dropped (nothing is defined there). float32 numpy."""
    e = torch.as_tensor(event).reshape(-1).cpu().numpy() != 0
    t = torch.as_tensor(time).reshape(-1).to(torch.float32).cpu().numpy()
    if not e.any():
        raise ValueError("default_times: the cohort has no observed event")
    at = np.unique(np.quantile(t[e], np.arange(1, 10) / 10, method="lower").astype(np.float32))
    at = at[at < t.max()]
    if at.size == 0:
        raise ValueError("default_times: no decile of the event times lies below the largest time")
    return at


def _matrix(x, n, name, columns):
    """x as float32 [n, c] with c among `columns`, free of NaN (checked where it lies)."""
    x = torch.as_tensor(x)
    if x.dim() == 1:
        x = x.reshape(-1, 1)
    if x.dim() != 2 or x.shape[0] != n:
        raise ValueError("Found input variables with inconsistent numbers of samples")
    if x.shape[1] not in columns:
        raise ValueError(f"{name}: {x.shape[1]} columns, expected {' or '.join(str(c) for c in columns)} (one per query time)")
    x = x.to(torch.float32)
    if bool(torch.isnan(x).any()):
        raise ValueError(f"{name}: NaN")
    return x


def _pitched(x, dev):
    """x [n, c] on the device with unit stride along c; a row pitch (stride(0) > c) is handed to the kernel as it is."""
    x = x.to(dev)
    if x.stride(1) != 1 or x.stride(0) < x.shape[1] or x.data_ptr() % 4:
        x = x.contiguous()
    return x


def ipcw_rows(event, time, at, surv=None, risk=None, weights=None):
    """The launch. event [n] (!= 0: observed), time [n]; at [Q] ascending query times; surv None or [n, Q]: the predicted probability of
    surviving at[q]; risk None, [n] / [n, 1] (one risk for every q) or [n, Q]; weights None (all ones) or int32 [R, n], >= 0, every row
    sum below 2^31. -> namespace of device tensors: counts int64 [R, Q, 2] (N_case, N_ctrl), rowcnt int64 [R, 2] (sum w, sum w e), sums
    float64 [R, Q, 6] (A, B, G(at), S_KM(at), Wc, C: include/advmil_hip.h), at float32 [Q], and ldw, lds, ldr: the row pitches (elements)
    the kernel was handed. More rows than fit a workspace of `stratify.MAX_ROW_BYTES` go through several launches."""
    event, time = torch.as_tensor(event).reshape(-1), torch.as_tensor(time).reshape(-1)
    n = time.numel()
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
        raise ValueError(f"ipcw_rows: n = {n} (1 to 2^16), {R} rows (1 to 2^20)")
    at = torch.as_tensor(at).reshape(-1).to(torch.float32)
    Q = at.numel()
    if not 1 <= Q <= MAX_QUERIES:
        raise ValueError(f"at: {Q} query times (1 to {MAX_QUERIES})")
    if bool(torch.isnan(at).any()) or bool((at[1:] < at[:-1]).any()):
        raise ValueError("at: the query times must ascend")
    if weights is not None:
        if bool((weights < 0).any()):
            raise ValueError("weights: negative multiplicities")
        if int(weights.sum(dim=1, dtype=torch.int64).max()) >= 1 << 31:
            raise ValueError("weights: a row sums to 2^31 or more")
    if bool(torch.isnan(time.to(torch.float32)).any()):
        raise ValueError("time: NaN")
    s = _matrix(surv, n, "surv", (Q,)) if surv is not None else None
    rk = _matrix(risk, n, "risk", (1, Q)) if risk is not None else None
    dev = _device(weights, s, rk, time)
    s = _pitched(s, dev) if s is not None else None
    rk = _pitched(rk, dev) if rk is not None else None
    if event.dtype == torch.bool:
        event = event.to(torch.float32)
    tm = time.to(device=dev, dtype=torch.float32)
    stime, order = torch.sort(tm, stable=True)                       # the replicate-independent preparation
    sevent = event.to(device=dev, dtype=torch.float32)[order].contiguous()
    order = order.to(torch.int32)
    w = _rows(weights, torch.int32, dev) if weights is not None else None
    ldw = (w.stride(0) if R > 1 else n) if w is not None else 0     # (the stride of a single row is arbitrary)
    lds = (s.stride(0) if n > 1 else Q) if s is not None else 0
    ldr = (rk.stride(0) if n > 1 else rk.shape[1]) if rk is not None else 0
    counts = torch.empty((R, Q, 2), dtype=torch.int64, device=dev)
    rowcnt = torch.empty((R, 2), dtype=torch.int64, device=dev)
    sums = torch.empty((R, Q, 6), dtype=torch.float64, device=dev)
    atd = at.to(dev).contiguous()
    L = _lib.lib()
    per = max(1, min(R, _strat.MAX_ROW_BYTES // (8 * n)))            # rows per launch: R n doubles of workspace
    wsb = L.advmil_ipcw_rows_workspace_bytes(n, per, Q)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for r0 in range(0, R, per):
        k = min(per, R - r0)
        _lib.check(L.advmil_ipcw_rows(_p(stime), _p(sevent), _p(order), n, _p(w[r0:] if w is not None else None), ldw, k, _p(atd), Q,
                                      _p(s), lds, _p(rk), ldr, rk.shape[1] if rk is not None else 1, _p(counts[r0:]), _p(rowcnt[r0:]),
                                      _p(sums[r0:]), _p(ws), wsb, stream), "ipcw_rows")
    return types.SimpleNamespace(counts=counts, rowcnt=rowcnt, sums=sums, at=atd, ldw=ldw, lds=lds, ldr=ldr, launches=-(-R // per))


def statistics_from_rows(counts, rowcnt, sums, at):
    """counts int64 [..., Q, 2], rowcnt int64 [..., 2], sums float64 [..., Q, 6] (numpy or tensors), at [Q] -> namespace of numpy arrays:
    brier, auc [..., Q], ibs, mean_auc [...] (NaN where undefined), km [..., Q] = S_KM(at).
      brier    = (A + B / G(at)) / sum w                                             iff N_ctrl > 0
      auc      = C / (Wc N_ctrl)                                                     iff N_ctrl > 0 and N_case > 0
      ibs      = trapezoid of brier over at / (at[Q-1] - at[0])                      iff Q >= 2 and every brier is defined
      mean_auc = sum_q auc_q (S_KM(t_{q-1}) - S_KM(t_q)) / (1 - S_KM(t_{Q-1})), S_KM(t_{-1}) = 1     iff every auc is defined and S_KM(t_{Q-1}) < 1"""
    c = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    rc = rowcnt.cpu().numpy() if torch.is_tensor(rowcnt) else np.asarray(rowcnt)
    s = sums.cpu().numpy() if torch.is_tensor(sums) else np.asarray(sums, dtype=np.float64)
    t = (at.cpu().numpy() if torch.is_tensor(at) else np.asarray(at)).astype(np.float32).astype(np.float64)
    ncase, nctrl = c[..., 0], c[..., 1]
    A, B, G, S, Wc, C = (s[..., k] for k in range(6))
    W = rc[..., 0][..., None].astype(np.float64)
    bs_ok, auc_ok = nctrl > 0, (nctrl > 0) & (ncase > 0)
    with np.errstate(all="ignore"):
        brier = np.where(bs_ok, (A + B / G) / W, np.nan)
        auc = np.where(auc_ok, C / (Wc * nctrl), np.nan)
        Q = t.size
        if Q >= 2:
            ibs = (0.5 * (brier[..., 1:] + brier[..., :-1]) * np.diff(t)).sum(axis=-1) / (t[-1] - t[0])
        else:
            ibs = np.full(brier.shape[:-1], np.nan)
        prev = np.concatenate([np.ones_like(S[..., :1]), S[..., :-1]], axis=-1)
        mean_auc = (auc * (prev - S)).sum(axis=-1) / (1.0 - S[..., -1])
        mean_auc = np.where(S[..., -1] < 1.0, mean_auc, np.nan)
    return types.SimpleNamespace(brier=brier, auc=auc, ibs=ibs, mean_auc=mean_auc, km=S)


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def brier_score(event, time, surv, at):
    """The IPCW Brier score at the times `at` of the predicted survival probabilities surv [n, Q] (sksurv.metrics.brier_score with the
    censoring distribution estimated on the same cohort). -> namespace: at float32 [Q], brier float64 [Q] (NaN where nobody is beyond
    at[q]), counts int64 [Q, 2]."""
    r = ipcw_rows(event, time, at, surv=surv)
    s = statistics_from_rows(r.counts, r.rowcnt, r.sums, r.at)
    return types.SimpleNamespace(at=_np(r.at), brier=s.brier[0], counts=_np(r.counts)[0])


def integrated_brier_score(event, time, surv, at):
    """-> namespace: at, brier [Q], ibs: the trapezoid of the Brier score over `at` divided by at[Q-1] - at[0] (sksurv's
    integrated_brier_score; Q >= 2, NaN when a Brier score is undefined)."""
    at = torch.as_tensor(at).reshape(-1)
    if at.numel() < 2:
        raise ValueError("integrated_brier_score: at least two query times")
    r = ipcw_rows(event, time, at, surv=surv)
    s = statistics_from_rows(r.counts, r.rowcnt, r.sums, r.at)
    return types.SimpleNamespace(at=_np(r.at), brier=s.brier[0], ibs=float(s.ibs[0]))


def cumulative_dynamic_auc(event, time, risk, at):
    """The cumulative/dynamic AUC at the times `at` of risk [n] or [n, Q] (higher = earlier event; sksurv.metrics.cumulative_dynamic_auc
    with the censoring distribution estimated on the same cohort). -> namespace: at, auc float64 [Q] (NaN where there is no case or no
    control), mean_auc (NaN unless every auc is defined), counts int64 [Q, 2]."""
    r = ipcw_rows(event, time, at, risk=risk)
    s = statistics_from_rows(r.counts, r.rowcnt, r.sums, r.at)
    return types.SimpleNamespace(at=_np(r.at), auc=s.auc[0], mean_auc=float(s.mean_auc[0]), counts=_np(r.counts)[0])


def bootstrap_timedep(event, time, at=None, surv=None, risk=None, n_boot=1000, seed=0, level=0.95, indices=None, max_undefined=0.05):
    """The point estimates and their percentile bootstrap: the cohort and the `n_boot` resamples (`indices` [B, n], default
    bootstrap.resample_indices(n, n_boot, seed): the resamples of the C-index bootstrap) are rows of one launch. `at` None:
    default_times(event, time), whose columns surv must then hold. surv or risk may be None: its statistics are then absent.
    -> namespace: at float32 [Q]; with surv: brier [Q], ibs, brier_samples [B, Q], ibs_samples [B], brier_lo, brier_hi [Q], ibs_lo,
    ibs_hi; with risk: auc [Q], mean_auc, auc_samples, mean_auc_samples, auc_lo, auc_hi, mean_auc_lo, mean_auc_hi (bootstrap._interval:
    np.nanpercentile at 50(1 -+ level)); n_undefined: dict statistic -> resamples in which it is undefined (brier, auc: at any query time),
    each capped by `max_undefined`."""
    event_t, time_t = torch.as_tensor(event).reshape(-1), torch.as_tensor(time).reshape(-1)
    n = time_t.numel()
    dev = _device(surv if torch.is_tensor(surv) else None, risk if torch.is_tensor(risk) else None, time_t)
    if at is None:
        at = default_times(event_t, time_t)
    if indices is None:
        indices = resample_indices(n, n_boot, seed)
    W = multiplicities(indices, n, device=dev)
    B = W.shape[0]
    weights = torch.cat([torch.ones((1, n), dtype=torch.int32, device=dev), W])
    r = ipcw_rows(event_t, time_t, at, surv=surv, risk=risk, weights=weights)
    s = statistics_from_rows(r.counts, r.rowcnt, r.sums, r.at)
    out = types.SimpleNamespace(at=_np(r.at), n_undefined={}, launches=r.launches)
    names = (["brier", "ibs"] if surv is not None else []) + (["auc", "mean_auc"] if risk is not None else [])
    for name in names:
        v = getattr(s, name)
        point, samples = v[0], v[1:]
        if name == "ibs" and out.at.size < 2:
            continue
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
