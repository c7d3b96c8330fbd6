"""How wrong is the predicted TIME, and is the predicted DISTRIBUTION calibrated -- what is asked right after the C-index, on the device
and with bootstrap intervals.

The reference's `mae` treats a censored patient with a hinge: one censored early costs almost nothing, whatever the model predicts.
The accepted repairs (Qi et al., ICML 2023, "An Effective Meaningful Way to Evaluate Survival Models") replace the unknown event time of
a censored patient by a surrogate built from the cohort's Kaplan-Meier curve -- the MARGIN time t + E[T - t | T > t] or the
PSEUDO-OBSERVATION N theta - (N - 1) theta^(-i) of the restricted mean theta -- and weight the patient's term by 1 - S_KM(t), how much
the curve knows about them. D-calibration (Haider et al., JMLR 2020) bins every patient's predicted probability of surviving their OWN
time, S_i(t_i), spreads a censored patient over the bins below theirs, and tests the bin masses for uniformity. The definitions, tail
and tie conventions are restated in include/advmil_hip.h.

The structure is that of eval/concordance.py: a bootstrap resample is a row of integer multiplicities; the cohort is sorted ONCE and
all rows go through ONE call (advmil_calib_rows, csrc/calib.hip), which leaves per row four exact counts, the restricted mean, per
prediction column the three numerators and denominators and the bin masses in double; the statistics are a few numpy operations on them
(`statistics_from_rows`). A row costs O(n) with the pseudo-observation as without it (the leave-one-out curves of all tie blocks come
from two more scans), so the only cap on a launch is the workspace's `stratify.MAX_ROW_BYTES`.

The margin and pseudo-observation errors are UNDEFINED in a row without an event (nobody carries weight). Undefined entries are NaN;
when the share of resamples with an undefined statistic exceeds `max_undefined` the bootstrap raises, because an interval conditional
on "defined" is not the interval that was asked for (eval/bootstrap.py gives the same reason). There is no CPU fallback."""
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

MAX_N, MAX_ROWS, MAX_PRED, MIN_BINS, MAX_BINS = 1 << 16, 1 << 20, 8, 2, 32
HINGE, MARGIN, PO = 0, 1, 2                                      # the measure axis of err
NUM, DEN = 0, 1                                                  # the last axis


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def calib_rows(event, time, pred=None, p_own=None, bins=10, gamma=0.0, po=True, weights=None):
    """The validated launch. event [n] (!= 0: observed), time [n] (>= 0); pred None or [n] / [n, P], 1 <= P <= 8 columns of predicted
    times; p_own None or [n] in [0, 1]: the predicted probability of surviving one's own time, binned into `bins` (2 to 32) bins; gamma:
    the hinge margin; po: also the pseudo-observation error; weights None (all ones) or int32 [R, n], >= 0, every row sum below 2^31.
    -> namespace of device tensors: rowcnt int64 [R, 4] (sum w, sum w e, distinct times, weight of the censored samples with
    S_KM = 0), km float64 [R, 3] (restricted mean, S_KM at the largest time, the largest time), err float64 [R, P, 3, 2] (hinge |
    margin | pseudo-observation; numerator | denominator), dcal float64 [R, bins] (include/advmil_hip.h), has_pred, has_p, with_po, and
    ldw, ldp: the row pitches (elements) the kernel was handed. The slots of an absent source are 0. More rows than fit a workspace of
    `stratify.MAX_ROW_BYTES` go through several launches."""
    event, time = torch.as_tensor(event).reshape(-1), torch.as_tensor(time).reshape(-1)
    n = time.numel()
    if pred is None and p_own is None:
        raise ValueError("calib_rows: neither pred (predicted times) nor p_own (survival probabilities at the own time) to score")
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
        raise ValueError(f"calib_rows: n = {n} (1 to 2^16), {R} rows (1 to 2^20)")
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not MIN_BINS <= bins <= MAX_BINS:
        raise ValueError(f"bins: {bins!r} ({MIN_BINS} to {MAX_BINS} bins)")
    gamma = float(gamma)
    if gamma != gamma or abs(gamma) == float("inf"):
        raise ValueError(f"gamma: {gamma}")
    if weights is not None:
        if bool((weights < 0).any()):
            raise ValueError("weights: negative multiplicities")
        if int(weights.sum(dim=1, dtype=torch.int64).max()) >= 1 << 31:
            raise ValueError("weights: a row sums to 2^31 or more")
    t32 = time.to(torch.float32)
    if bool(torch.isnan(t32).any()):
        raise ValueError("time: NaN")
    if bool((t32 < 0).any()):
        raise ValueError("time: negative times (the restricted mean is an integral from 0)")
    if event.is_floating_point() and bool(torch.isnan(event).any()):
        raise ValueError("event: NaN")
    y = p = None
    P = 1
    if pred is not None:
        y = torch.as_tensor(pred)
        if y.dim() == 1:
            y = y.reshape(-1, 1)
        if y.dim() != 2 or y.shape[0] != n:
            raise ValueError("Found input variables with inconsistent numbers of samples")
        P = y.shape[1]
        if not 1 <= P <= MAX_PRED:
            raise ValueError(f"pred: {P} columns (1 to {MAX_PRED})")
        if not (y.is_floating_point() or y.dtype in (torch.int32, torch.int64)):
            raise ValueError(f"pred: expected predicted times, got {y.dtype}")
        y = y.to(torch.float32)
        if bool(torch.isnan(y).any()):
            raise ValueError("pred: NaN")
    if p_own is not None:
        p = torch.as_tensor(p_own).reshape(-1)
        if p.numel() != n:
            raise ValueError("Found input variables with inconsistent numbers of samples")
        if not p.is_floating_point():
            raise ValueError(f"p_own: expected probabilities, got {p.dtype}")
        p = p.to(torch.float32)
        if bool(torch.isnan(p).any()):
            raise ValueError("p_own: NaN")
        if bool(((p < 0) | (p > 1)).any()):
            raise ValueError("p_own: probabilities outside [0, 1]")
    dev = _device(weights, y, p, time)
    y = _pitched(y, dev) if y is not None else None
    p = p.to(dev).contiguous() if p is not None else None
    if event.dtype == torch.bool:
        event = event.to(torch.float32)
    tm = t32.to(dev)
    stime, order = torch.sort(tm, stable=True)                       # the replicate-independent preparation
    sevent = event.to(device=dev, dtype=torch.float32)[order].contiguous()
    order = order.to(torch.int32)
    w = _rows(weights, torch.int32, dev) if weights is not None else None
    ldw = (w.stride(0) if R > 1 else n) if w is not None else 0     # (the stride of a single row is arbitrary)
    ldp = (y.stride(0) if n > 1 else P) if y is not None else 0
    with_po = 1 if po else 0
    rowcnt = torch.empty((R, 4), dtype=torch.int64, device=dev)
    km = torch.empty((R, 3), dtype=torch.float64, device=dev)
    err = torch.empty((R, P, 3, 2), dtype=torch.float64, device=dev)
    dcal = torch.empty((R, int(bins)), dtype=torch.float64, device=dev)
    L = _lib.lib()
    row_bytes = 8 * n * (3 + 2 * with_po)                            # the walk's per-block doubles
    per = max(1, min(R, _strat.MAX_ROW_BYTES // row_bytes))          # rows per launch
    wsb = L.advmil_calib_rows_workspace_bytes(n, per, with_po)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for r0 in range(0, R, per):
        k = min(per, R - r0)
        _lib.check(L.advmil_calib_rows(_p(stime), _p(sevent), _p(order), n, _p(w[r0:] if w is not None else None), ldw, k, _p(y), ldp, P,
                                       _p(p), int(bins), gamma, with_po, _p(rowcnt[r0:]), _p(km[r0:]), _p(err[r0:]), _p(dcal[r0:]), _p(ws),
                                       wsb, stream), "calib_rows")
    return types.SimpleNamespace(rowcnt=rowcnt, km=km, err=err, dcal=dcal, has_pred=y is not None, has_p=p is not None,
                                 with_po=bool(with_po), ldw=ldw, ldp=ldp, launches=-(-R // per))


def chi2_sf(x, df):
    """The upper tail of the chi-square distribution with `df` degrees of freedom at x (numpy, any shape): the regularised upper
    incomplete gamma function Q(df / 2, x / 2), torch.special.gammaincc in float64. NaN stays NaN."""
    x = np.asarray(x, dtype=np.float64)
    a = torch.full(x.shape, df / 2.0, dtype=torch.float64)
    return torch.special.gammaincc(a, torch.from_numpy(np.ascontiguousarray(x / 2.0)).reshape(x.shape)).numpy()


def statistics_from_rows(rowcnt, km, err, dcal, has_pred=True, has_p=True, with_po=True):
    """rowcnt int64 [..., 4], km float64 [..., 3], err float64 [..., P, 3, 2], dcal float64 [..., B] (numpy or tensors) -> namespace of
    numpy arrays, NaN where undefined or where the source is absent:
      mae_hinge, mae_margin, mae_po [..., P] = numerator / denominator                      iff the denominator is > 0
      d_cal_chi2 [...]   = sum_k (N_k - N / B)^2 / (N / B)                                  iff N > 0
      d_cal_p [...]      = the upper tail of chi-square with B - 1 degrees of freedom at d_cal_chi2
      d_cal_bins [..., B] = N_k / N
      rmst [...]         = the restricted mean of the row's Kaplan-Meier curve; n_zero_s [...] = the weight of the censored samples
                           with S_KM = 0 at their time (their margin surrogate is their own time)."""
    rc = _np(rowcnt)
    e = np.asarray(_np(err), dtype=np.float64)
    dc = np.asarray(_np(dcal), dtype=np.float64)
    N = rc[..., 0].astype(np.float64)
    out = types.SimpleNamespace(rmst=np.asarray(_np(km), dtype=np.float64)[..., 0], n_zero_s=rc[..., 3])
    with np.errstate(all="ignore"):
        for j, name, has in ((HINGE, "mae_hinge", has_pred), (MARGIN, "mae_margin", has_pred), (PO, "mae_po", has_pred and with_po)):
            num, den = e[..., j, NUM], e[..., j, DEN]
            setattr(out, name, np.where((den > 0) & has, num / den, np.nan))
        B = dc.shape[-1]
        expect = (N / B)[..., None]
        ok = (N > 0) & has_p
        out.d_cal_chi2 = np.where(ok, ((dc - expect) ** 2 / expect).sum(axis=-1), np.nan)
        out.d_cal_p = chi2_sf(out.d_cal_chi2, B - 1)
        out.d_cal_bins = np.where(ok[..., None], dc / N[..., None], np.nan)
    return out


def time_error(event, time, pred, gamma=0.0):
    """The three absolute errors of the predicted times `pred` [n] or [n, P]. -> namespace: mae_hinge, mae_margin, mae_po float64 [P]
    (NaN where undefined: margin and pseudo-observation in a cohort without an event), rmst, n_zero_s."""
    r = calib_rows(event, time, pred=pred, gamma=gamma)
    s = statistics_from_rows(r.rowcnt, r.km, r.err, r.dcal, True, False)
    return types.SimpleNamespace(mae_hinge=s.mae_hinge[0], mae_margin=s.mae_margin[0], mae_po=s.mae_po[0], rmst=float(s.rmst[0]),
                                 n_zero_s=int(s.n_zero_s[0]))


def d_calibration(event, time, p_own, bins=10):
    """D-calibration of p_own [n], every sample's predicted probability of surviving its own time. -> namespace: d_cal_chi2, d_cal_p
    (a small p: the bin masses are not uniform, the distribution is miscalibrated), d_cal_bins float64 [bins] (the masses over N)."""
    r = calib_rows(event, time, p_own=p_own, bins=bins, po=False)
    s = statistics_from_rows(r.rowcnt, r.km, r.err, r.dcal, False, True, False)
    return types.SimpleNamespace(d_cal_chi2=float(s.d_cal_chi2[0]), d_cal_p=float(s.d_cal_p[0]), d_cal_bins=s.d_cal_bins[0])


def survival_at_own_time(time, dist_y_hat=None, hazards=None):
    """What D-calibration needs of a prediction: S_i(t_i). dist_y_hat [n, S]: S sampled times to event per patient -> the share of a
    patient's samples beyond their own time (the strict > of `survival_from_samples`); hazards [n, bins] of a discrete-time model,
    `time` then holds bin indices k -> prod_{l <= k} (1 - h_il). -> float32 [n] on the device."""
    if (dist_y_hat is None) == (hazards is None):
        raise ValueError("survival_at_own_time: exactly one of dist_y_hat and hazards")
    t = torch.as_tensor(time).reshape(-1).to(torch.float32)
    if bool(torch.isnan(t).any()):
        raise ValueError("time: NaN")
    x = torch.as_tensor(dist_y_hat if hazards is None else hazards)
    name = "dist_y_hat" if hazards is None else "hazards"
    if x.dim() != 2 or x.shape[0] != t.numel() or x.shape[1] < 1:
        raise ValueError(f"{name}: expected [n, S] with n = {t.numel()}, got shape {tuple(x.shape)}")
    dev = _device(x)
    x, t = x.to(device=dev, dtype=torch.float32), t.to(dev)
    if hazards is None:
        return (x > t[:, None]).sum(dim=1).to(torch.float32) / float(x.shape[1])
    if bool((t != torch.floor(t)).any()) or bool((t < 0).any()) or bool((t >= x.shape[1]).any()):
        raise ValueError(f"time: the times of a discrete-time model are bin indices in [0, {x.shape[1] - 1}]")
    return torch.cumprod(1.0 - x, dim=1).gather(1, t.to(torch.int64)[:, None])[:, 0].contiguous()


_NAMES = {"mae_hinge": "pred", "mae_margin": "pred", "mae_po": "pred", "d_cal_chi2": "p", "d_cal_p": "p"}


def bootstrap_calibration(event, time, pred=None, p_own=None, bins=10, gamma=0.0, po=True, n_boot=1000, seed=0, level=0.95, indices=None,
                          max_undefined=0.05):
    """The point estimates and their percentile bootstrap: the cohort and the `n_boot` resamples (`indices` [B, n], default
    bootstrap.resample_indices(n, n_boot, seed): the resamples of the C-index bootstrap) are rows of one call. pred or p_own may be
    None: its statistics are then absent. -> namespace; with pred: mae_hinge, mae_margin, mae_po [P] (mae_po only with `po`); with
    p_own: d_cal_chi2, d_cal_p, d_cal_bins [bins]; per statistic <name>_samples [B] or [B, P], <name>_lo, <name>_hi
    (bootstrap._interval: np.nanpercentile at 50(1 -+ level)); with two prediction columns also <name>_diff (column 0 - column 1, on
    the same resamples), <name>_diff_samples [B], <name>_diff_lo, <name>_diff_hi; n_undefined: dict statistic -> resamples in which
    it is undefined (in any column), each capped by `max_undefined`."""
    event_t, time_t = torch.as_tensor(event).reshape(-1), torch.as_tensor(time).reshape(-1)
    n = time_t.numel()
    dev = _device(pred if torch.is_tensor(pred) else None, p_own if torch.is_tensor(p_own) else None, time_t)
    if indices is None:
        indices = resample_indices(n, n_boot, seed)
    W = multiplicities(indices, n, device=dev)
    B = W.shape[0]
    weights = torch.cat([torch.ones((1, n), dtype=torch.int32, device=dev), W])
    r = calib_rows(event_t, time_t, pred=pred, p_own=p_own, bins=bins, gamma=gamma, po=po, weights=weights)
    s = statistics_from_rows(r.rowcnt, r.km, r.err, r.dcal, r.has_pred, r.has_p, r.with_po)
    out = types.SimpleNamespace(n_undefined={}, launches=r.launches, rowcnt=_np(r.rowcnt)[0], rmst=float(s.rmst[0]))
    if r.has_p:
        out.d_cal_bins = s.d_cal_bins[0]
    for name, source in _NAMES.items():
        if not (r.has_pred if source == "pred" else r.has_p) or (name == "mae_po" and not r.with_po):
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
        if not scalar and samples.shape[1] == 2:                     # two models on the same resamples: the paired difference
            d = samples[:, 0] - samples[:, 1]
            with np.errstate(all="ignore"):
                dlo, dhi = _interval(d, level) if B else (np.nan, np.nan)
            out.__dict__.update({name + "_diff": float(point[0] - point[1]), name + "_diff_samples": d, name + "_diff_lo": float(dlo),
                                 name + "_diff_hi": float(dhi)})
    return out
