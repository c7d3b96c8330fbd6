"""Bootstrap of the concordance index: confidence intervals, paired comparison of two models, and the C-index distribution over the
generator's sampled predictions (`dist_y_hat` of `test_model`).

A bootstrap resample is a vector of multiplicities over the same n patients, and the status of a pair (comparable, concordant,
discordant, tied) does not depend on it; only the pair's weight w_i * w_j does. So every resample and every prediction column is
counted in ONE launch (advmil_cindex_counts_weighted, csrc/evalk.hip), in integers: the counts of resample b are exactly those the
reference's estimator (eval/cindex.py:79-143) gives on the arrays `event[idx], time[idx], estimate[idx]` with
`idx = resample_indices(n, n_boot, seed)[b]`, so anyone can redo a resample with the reference's own function.

A resample is UNDEFINED where the reference would raise or divide by zero: fewer than two samples, no event copy, no event with an
entry (NoComparablePairException), no comparable pair. Its C-index is NaN; when the share of such resamples exceeds `max_undefined`
the functions raise, because an interval conditional on "defined" is not the interval that was asked for. There is no CPU fallback."""
import ctypes
import types

import numpy as np
import torch

from .. import _lib
from .cindex import concordance_index_censored

ROW_TILE = _lib.CINDEX_BOOT_ROW_TILE                    # the kernel walks the samples in strides of this many threads
RESAMPLE_CHUNK = _lib.CINDEX_BOOT_RESAMPLE_CHUNK        # ... and carries this many resamples at a time
MAX_COLUMNS = 64                                        # estimate rows per launch (M of the C entry)
_NO_DEVICE = "advmil_amd.eval needs an MI355X: no ROCm device visible (no CPU fallback)"


def resample_indices(n, n_boot, seed):
    """The resamples of every function here: np.random.RandomState(seed).randint(0, n, size=(n_boot, n)), int64 [n_boot, n]."""
    return np.random.RandomState(seed).randint(0, n, size=(n_boot, n)).astype(np.int64)


def multiplicities(indices, n, device=None):
    """indices [B, k] (values in [0, n)) -> int32 [B, n] on the device: how often each sample occurs in each resample."""
    idx = np.asarray(indices, dtype=np.int64)
    if idx.ndim != 2:
        raise ValueError(f"indices: expected [n_boot, k], got shape {idx.shape}")
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError(f"indices outside [0, {n})")
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_DEVICE)
    B = idx.shape[0]
    flat = (idx + np.arange(B, dtype=np.int64)[:, None] * n).reshape(-1)
    w = np.bincount(flat, minlength=B * n).astype(np.int32).reshape(B, n)
    return torch.from_numpy(w).to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))


def _rows(t, dtype, device):
    """t as [rows, n] of `dtype` on `device` with unit stride along n; a row pitch (stride(0) > n) is handed to the kernel as it is."""
    t = t.to(device=device, dtype=dtype)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.data_ptr() % t.element_size():
        t = t.contiguous()
    return t


def concordance_counts_weighted(event, time, estimate, weights, tied_tol=1e-8):
    """-> int64 device tensor [M, B, 8]: concordant, discordant, tied_risk, tied_time, comparable, events_with_entry, event copies,
    size of resample b (row of `weights`, int32 [B, n]) under estimate row m (`estimate` [n] or [M, n], M <= 64)."""
    weights = torch.as_tensor(weights)
    if weights.dtype != torch.int32:
        raise ValueError(f"weights: expected int32 multiplicities, got {weights.dtype}")
    estimate = torch.as_tensor(estimate)
    if estimate.dim() == 1:
        estimate = estimate.reshape(1, -1)
    event, time = torch.as_tensor(event).reshape(-1), torch.as_tensor(time).reshape(-1)
    n = time.numel()
    if weights.dim() != 2 or estimate.dim() != 2 or not (event.numel() == n == estimate.shape[1] == weights.shape[1]):
        raise ValueError("Found input variables with inconsistent numbers of samples")
    M, B = estimate.shape[0], weights.shape[0]
    if n < 1 or B < 1 or not 1 <= M <= MAX_COLUMNS:
        raise ValueError(f"concordance_counts_weighted: n = {n}, {B} resamples, {M} estimate rows (1 to {MAX_COLUMNS})")
    if bool((weights < 0).any()):
        raise ValueError("weights: negative multiplicities")
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_DEVICE)
    if weights.is_cuda:
        dev = weights.device
    elif estimate.is_cuda:
        dev = estimate.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    if event.dtype == torch.bool:
        event = event.to(torch.float32)
    ev = event.to(device=dev, dtype=torch.float32).contiguous()
    tm = time.to(device=dev, dtype=torch.float32).contiguous()
    est, w = _rows(estimate, torch.float32, dev), _rows(weights, torch.int32, dev)
    out = torch.empty((M, B, 8), dtype=torch.int64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    pitch = lambda t: t.stride(0) if t.shape[0] > 1 else n   # noqa: E731  (the stride of a single row is arbitrary)
    _lib.check(_lib.lib().advmil_cindex_counts_weighted(p(tm), p(ev), p(est), pitch(est), M, p(w), pitch(w), B, n, float(tied_tol),
                                                        p(out), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               "cindex_counts_weighted")
    return out


def samples_from_counts(counts):
    """counts int64 [..., 8] (numpy) -> (float64 C-index per resample, NaN where undefined; bool mask of the undefined ones)."""
    c = np.asarray(counts)
    con, tie, comp, entries, events, size = c[..., 0], c[..., 2], c[..., 4], c[..., 5], c[..., 6], c[..., 7]
    undefined = (size < 2) | (events == 0) | (entries == 0) | (comp == 0)
    samples = np.full(c.shape[:-1], np.nan, dtype=np.float64)
    ok = ~undefined
    samples[ok] = (con[ok] + 0.5 * tie[ok]) / comp[ok]
    return samples, undefined


def _risks(y_true, y_pred):
    """(event, time, risk, device) the way concordance_index forms them (eval/cindex.py:10-41)."""
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_DEVICE)
    y_true, y_pred = torch.as_tensor(y_true), torch.as_tensor(y_pred)
    dev = y_pred.device if y_pred.is_cuda else torch.device("cuda", torch.cuda.current_device())
    y_true = y_true.to(dev, torch.float32).reshape(y_true.shape[0], -1)
    y_pred = y_pred.to(dev, torch.float32).reshape(y_pred.shape[0], -1)
    t, e = y_true[:, 0], y_true[:, 1]
    if y_pred.shape[1] == 1:
        return e, t, -y_pred[:, 0], dev
    return e, t, -torch.cumprod(1.0 - y_pred, dim=1).sum(dim=1), dev


def _interval(samples, level):
    lo, hi = np.nanpercentile(samples, [50.0 * (1.0 - level), 50.0 * (1.0 + level)], axis=-1)
    return lo, hi


def bootstrap_estimates(event, time, estimates, n_boot=1000, seed=0, indices=None, max_undefined=0.05):
    """The shared core: `estimates` [M, n] risks on the device -> (samples float64 [M, B], counts int64 [M, B, 8], n_undefined), all
    rows on the same resamples (`indices` [B, n], default resample_indices(n, n_boot, seed))."""
    n = estimates.shape[1]
    if indices is None:
        indices = resample_indices(n, n_boot, seed)
    w = multiplicities(indices, n, device=estimates.device)
    counts = concordance_counts_weighted(event, time, estimates, w, tied_tol=1e-08).cpu().numpy()
    samples, undefined = samples_from_counts(counts)
    n_undefined = int(undefined[0].sum())                # (what makes a resample undefined does not depend on the estimate)
    share = n_undefined / undefined.shape[1]
    if share > max_undefined:
        raise ValueError(f"{n_undefined} of {undefined.shape[1]} bootstrap resamples ({share:.1%}) have no defined concordance index "
                         f"(max_undefined = {max_undefined:g})")
    return samples, counts, n_undefined


def _se(samples):
    return np.nanstd(samples, ddof=1, axis=-1)


def bootstrap_concordance_index(y_true, y_pred, n_boot=1000, seed=0, level=0.95, indices=None, max_undefined=0.05):
    """Percentile bootstrap of concordance_index(y_true, y_pred). -> namespace: cindex (point estimate), samples float64 [B] (NaN where
    undefined), counts int64 [B, 8], lo, hi (np.nanpercentile at 50(1 -+ level)), se (np.nanstd, ddof=1), n_undefined."""
    e, t, risk, _ = _risks(y_true, y_pred)
    return bootstrap_risk(e, t, risk, n_boot, seed, level, indices, max_undefined)


def bootstrap_risk(event, time, risk, n_boot=1000, seed=0, level=0.95, indices=None, max_undefined=0.05):
    """bootstrap_concordance_index for a risk vector that is already on the device (what concordance_index_censored takes)."""
    e, t = event, time
    cindex = concordance_index_censored(e, t, risk, tied_tol=1e-08, device=risk.device)[0]
    samples, counts, n_undefined = bootstrap_estimates(e, t, risk.reshape(1, -1), n_boot, seed, indices, max_undefined)
    lo, hi = _interval(samples[0], level)
    return types.SimpleNamespace(cindex=cindex, samples=samples[0], counts=counts[0], lo=float(lo), hi=float(hi),
                                 se=float(_se(samples[0])), n_undefined=n_undefined)


def bootstrap_concordance_samples(y_true, dist_y_hat, n_boot=1000, seed=0, level=0.95, indices=None, max_undefined=0.05):
    """`dist_y_hat` [n, S]: the S sampled predictions per patient of `test_model` (S <= 64), every column one model in one launch.
    -> namespace: cindex float64 [S], samples [S, B], counts [S, B, 8], lo, hi, se [S], n_undefined; column s equals
    bootstrap_concordance_index(y_true, dist_y_hat[:, s:s+1], ...)."""
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_DEVICE)
    d = torch.as_tensor(dist_y_hat)
    if d.dim() != 2 or not 1 <= d.shape[1] <= MAX_COLUMNS:
        raise ValueError(f"dist_y_hat: expected [n, S] with 1 <= S <= {MAX_COLUMNS}, got shape {tuple(d.shape)}")
    e, t, _, dev = _risks(y_true, d[:, :1])
    risks = (-d.to(dev, torch.float32)).t().contiguous()
    cindex = np.array([concordance_index_censored(e, t, risks[s], tied_tol=1e-08, device=dev)[0] for s in range(risks.shape[0])])
    samples, counts, n_undefined = bootstrap_estimates(e, t, risks, n_boot, seed, indices, max_undefined)
    lo, hi = _interval(samples, level)
    return types.SimpleNamespace(cindex=cindex, samples=samples, counts=counts, lo=lo, hi=hi, se=_se(samples), n_undefined=n_undefined)


def paired_bootstrap_concordance(y_true, y_pred_a, y_pred_b, n_boot=1000, seed=0, level=0.95, indices=None, max_undefined=0.05):
    """Two models on the same resamples, one launch. -> namespace: cindex_a, cindex_b, delta (C_a - C_b), samples_a, samples_b,
    delta_samples [B], lo, hi of the delta, se, p_value = min(1, 2 min(#(delta <= 0) + 1, #(delta >= 0) + 1) / (B_defined + 1)),
    n_undefined."""
    e, t, risk_a, dev = _risks(y_true, y_pred_a)
    _, _, risk_b, _ = _risks(y_true, torch.as_tensor(y_pred_b).to(dev))
    if risk_a.numel() != risk_b.numel():
        raise ValueError("Found input variables with inconsistent numbers of samples")
    ca = concordance_index_censored(e, t, risk_a, tied_tol=1e-08, device=dev)[0]
    cb = concordance_index_censored(e, t, risk_b, tied_tol=1e-08, device=dev)[0]
    samples, _, n_undefined = bootstrap_estimates(e, t, torch.stack([risk_a, risk_b]), n_boot, seed, indices, max_undefined)
    delta = samples[0] - samples[1]
    d = delta[~np.isnan(delta)]
    p_value = min(1.0, 2.0 * min(int((d <= 0).sum()) + 1, int((d >= 0).sum()) + 1) / (d.size + 1))
    lo, hi = _interval(delta, level)
    return types.SimpleNamespace(cindex_a=ca, cindex_b=cb, delta=ca - cb, samples_a=samples[0], samples_b=samples[1], delta_samples=delta,
                                 lo=float(lo), hi=float(hi), se=float(_se(delta)), p_value=p_value, n_undefined=n_undefined)
