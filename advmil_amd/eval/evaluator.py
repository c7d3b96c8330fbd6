"""eval/evaluator.py of the reference (ContSurv_Evaluator 11-130, DiscSurv_Evaluator 133-210, CoxSurv_Evaluator 213-259) with the same
names, `kws`, `valid_metrics`, `compute(data, metrics) -> dict[str, float]` and failure behaviour. The reference answers every metric
with its own small host computation ending in `.item()`; here one fused launch per family (advmil_surv_metrics_cont / _disc,
advmil_ple_loss, advmil_rank_loss_fwd: csrc/survk.hip) leaves every sum in ONE device array, which is copied to the host once.

`data` is the collector of `test_model`: `y` [n, 2] (time | event), `y_hat`, optional `avg_y_hat` (preferred when present, as in the
reference), optional `f_fake`; on the host or on the device (host tensors are moved once).

How a `kws` callable is dispatched: `advmil_amd.loss.utils.recon_loss` / `rank_loss` / `real_fake_loss` (bare or as a
`functools.partial` with keyword arguments) and instances of this package's `SurvMLE` / `SurvPLE` are recognised, their parameters read
and their arithmetic taken from the fused launch; any other callable is called on the device tensors and `.item()`-ed, as the
reference does. There is no CPU fallback."""
import ctypes
import functools

import numpy as np
import torch

from .. import _lib
from ..loss import utils as LU
from .bootstrap import bootstrap_concordance_index, bootstrap_risk
from .cindex import concordance_index, concordance_index_censored
from .stratify import _risks, stratify_risk
from . import timedep as TD
from . import concordance as CC
from . import calibration as CB

_WHICH = {"bce": 0, "hinge": 1, "wasserstein": 2}
# slots of the result array (doubles): [0, 16) the family's fused sums, [16, 20) rank_loss state, [20, 22) SurvPLE
_RANK, _PLE, _NRES = 16, 20, 24


class MissingFakeScores(TypeError, AttributeError):
    """A metric over `f_fake` was asked of a collector without one (the reference fails on `None` there: TypeError from torch.mean,
    AttributeError from `None.squeeze()`; this is both)."""


def _device_of(data):
    if not torch.cuda.is_available():
        raise RuntimeError("advmil_amd.eval needs an MI355X: no ROCm device visible (no CPU fallback)")
    y = data["y"]
    return y.device if (torch.is_tensor(y) and y.is_cuda) else torch.device("cuda", torch.cuda.current_device())


def _f32(x, dev):
    return torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ws(nbytes, dev):
    return torch.empty((int(nbytes) + 7) // 8, dtype=torch.float64, device=dev)


def _recognise(fn, target, allowed):
    """-> the keyword arguments bound to `target` (this package's function), or None when `fn` is something else."""
    if fn is target:
        return {}
    if isinstance(fn, functools.partial) and fn.func is target and not fn.args and set(fn.keywords) <= set(allowed):
        return dict(fn.keywords)
    return None


def _given(kws, name):
    return kws.get(name) is not None


def _disc_which(kws):
    """(which code | None, generic callable | None) of kws['disc_loss']."""
    if not _given(kws, "disc_loss"):
        return None, None
    k = _recognise(kws["disc_loss"], LU.real_fake_loss, ("which",))
    if k is not None and k.get("which", "bce") in _WHICH:
        return _WHICH[k.get("which", "bce")], None
    return None, kws["disc_loss"]


def _fake_of(data, dev):
    return _f32(data["f_fake"], dev).reshape(-1) if data.get("f_fake") is not None else None


def _mean(total, count):
    return total / count if count > 0 else float("nan")          # torch.mean of an empty selection


def _calibration_dict(b, names, n_boot):
    """The namespace of `bootstrap_calibration` as the dict the evaluators return: the statistics `names`, with `n_boot` > 0 their
    intervals, the paired differences where there are two prediction columns, and `n_undefined`."""
    out = {}
    for k in names:
        for key in (k, k + "_diff"):
            if hasattr(b, key):
                out[key] = getattr(b, key)
                if n_boot > 0:
                    out[key + "_lo"], out[key + "_hi"] = getattr(b, key + "_lo"), getattr(b, key + "_hi")
    if hasattr(b, "d_cal_bins"):
        out["d_cal_bins"] = b.d_cal_bins
    if n_boot > 0:
        out["n_undefined"] = b.n_undefined
    return out


class _Evaluator(object):
    valid_metrics = []

    def _check_metrics(self, metrics):
        for m in metrics:
            assert m in self.valid_metrics

    def _need_fake(self, fake):
        if fake is None:
            raise MissingFakeScores("the collector holds no 'f_fake'")

    def _bootstrap_c_index(self, data, n_boot, seed, level):
        """-> the bootstrap namespace (eval/bootstrap.py) of the estimate vector this evaluator's `c_index` metric passes."""
        dev = _device_of(data)
        y = _f32(data["y"], dev)
        pred = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev).reshape(-1)
        return bootstrap_concordance_index(y, pred.reshape(-1, 1), n_boot=n_boot, seed=seed, level=level)

    def bootstrap(self, data, n_boot=1000, seed=0, level=0.95):
        """Percentile bootstrap of the `c_index` metric over `n_boot` resamples of the patients (every resample in one launch):
        the point estimate `compute` returns, the interval at `level`, the bootstrap standard error and how many resamples had no
        defined C-index (more than 5 % of them: ValueError)."""
        b = self._bootstrap_c_index(data, n_boot, seed, level)
        return {"c_index": b.cindex, "c_index_lo": b.lo, "c_index_hi": b.hi, "c_index_se": b.se, "n_undefined": b.n_undefined}

    def _risk_estimate(self, data):
        """-> (event, time, risk) on the device: the estimate vector `_bootstrap_c_index` hands to the bootstrap."""
        dev = _device_of(data)
        y = _f32(data["y"], dev)
        pred = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev).reshape(-1)
        return _risks(y, pred.reshape(-1, 1))[:3]

    def stratify(self, data, q=0.5, n_perm=0, n_boot=0, seed=0, level=0.95):
        """Split the cohort at the `q`-quantile of the risk the `c_index` metric ranks by and compare the two groups (eval/stratify.py,
        one launch): group sizes and events, Kaplan-Meier medians, the log-rank z, chi2 and p, with `n_perm` > 0 the permutation p-value
        and with `n_boot` > 0 the bootstrap interval of z and how many resamples had no statistic (more than 5 % of them: ValueError)."""
        e, t, risk = self._risk_estimate(data)
        s = stratify_risk(e, t, risk, q=q, n_perm=n_perm, n_boot=n_boot, seed=seed, level=level)
        return {"n_low": s.n_low, "n_high": s.n_high, "events_low": s.events_low, "events_high": s.events_high, "median_low": s.median_low,
                "median_high": s.median_high, "z": s.z, "chi2": s.chi2, "p": s.p, "p_perm": s.p_perm, "z_lo": s.z_lo, "z_hi": s.z_hi,
                "n_undefined": s.n_undefined}

    def _survival_estimate(self, data, times):
        """-> (event, time, at, surv [n, Q] or None, risk [n] or [n, Q]) on the device: what `time_dependent` scores."""
        e, t, risk = self._risk_estimate(data)
        return e, t, (TD.default_times(e, t) if times is None else times), None, risk

    def time_dependent(self, data, times=None, n_boot=0, seed=0, level=0.95):
        """Calibration and discrimination of the predicted survival function over time (eval/timedep.py, one launch): the IPCW Brier
        score `brier` and the cumulative/dynamic AUC `auc` at `times` (default: the deciles of the observed event times below the
        largest time; bin indices for a discrete-time model), their summaries `ibs` and `mean_auc`, NaN where undefined; with
        `n_boot` > 0 the percentile intervals `<key>_lo` / `<key>_hi` at `level` and `n_undefined`, per statistic the resamples in
        which it is undefined (more than 5 % of them: ValueError). An evaluator without a survival function has no `brier` / `ibs`."""
        e, t, at, surv, risk = self._survival_estimate(data, times)
        b = TD.bootstrap_timedep(e, t, at, surv, risk, n_boot=n_boot, seed=seed, level=level)
        out = {"times": b.at}
        for k in ("brier", "ibs", "auc", "mean_auc"):
            if hasattr(b, k):
                out[k] = getattr(b, k)
                if n_boot > 0:
                    out[k + "_lo"], out[k + "_hi"] = getattr(b, k + "_lo"), getattr(b, k + "_hi")
        if n_boot > 0:
            out["n_undefined"] = b.n_undefined
        return out

    def concordance(self, data, tau=None, n_boot=0, seed=0, level=0.95):
        """Global discrimination beyond `c_index` (eval/concordance.py, one call): Uno's C `c_uno` at the truncation times `tau` (None:
        no truncation) and the unweighted `c_harrell` of the risk the `c_index` metric ranks by; for an evaluator with a survival
        function also Antolini's time-dependent concordance `c_td`, its tie-adjusted form `c_td_adj` and `c_uno_td` (Antolini's pairs,
        Uno's weights), the survival function taken at every observed event time. NaN where undefined; with `n_boot` > 0 the percentile
        intervals `<key>_lo` / `<key>_hi` at `level` and `n_undefined` (more than 5 % of the resamples: ValueError)."""
        e, t, risk = self._risk_estimate(data)
        at, col, surv = self._survival_at_event_times(data, e, t)
        b = CC.bootstrap_concordance(e, t, risk=risk, surv=surv, col=col, tau=tau, n_boot=n_boot, seed=seed, level=level)
        out = {"tau": b.tau}
        for k in ("c_uno", "c_harrell", "c_td", "c_td_adj", "c_uno_td"):
            if hasattr(b, k):
                out[k] = getattr(b, k)
                if n_boot > 0:
                    out[k + "_lo"], out[k + "_hi"] = getattr(b, k + "_lo"), getattr(b, k + "_hi")
        if n_boot > 0:
            out["n_undefined"] = b.n_undefined
        return out

    def _survival_at_event_times(self, data, e, t, chunk=256):
        """-> (at, col, surv [n, Q] on the device) from `_survival_estimate` at the distinct event times, `chunk` columns at a time (the
        sampled distribution is compared with `chunk` times at once, never with all of them); (None, None, None) for an evaluator
        without a survival function."""
        ev = e.cpu().numpy() != 0
        if not ev.any():
            raise ValueError("concordance: the cohort has no observed event")
        at = np.unique(t.to(torch.float32).cpu().numpy()[ev])
        parts = []
        for c0 in range(0, at.size, chunk):
            s = self._survival_estimate(data, torch.from_numpy(at[c0:c0 + chunk]).to(t.device))[3]
            if s is None:
                return None, None, None
            if not parts and at.size > CC.MAX_COLUMNS:
                raise ValueError(f"concordance: {at.size} distinct event times, the kernel takes {CC.MAX_COLUMNS} columns; round the "
                                 "times or evaluate a subsample")
            parts.append(s)
        return at, torch.from_numpy(CC.columns_at_own_times(t, at)), torch.cat(parts, dim=1)


class ContSurv_Evaluator(_Evaluator):
    """Performance evaluator for continuous survival model"""

    def __init__(self, **kws):
        self.kws = kws
        self.end_time = kws["end_time"]
        self.valid_metrics = ["c_index", "loss_rank", "loss_recon", "loss_recon_org", "loss_fake_netD", "loss_fake_netG",
                              "avg_fake", "event_t_rae", "nonevent_t_rae", "event_t_nre", "nonevent_t_nre", "mae"]

    def compute(self, data, metrics):
        self._check_metrics(metrics)
        dev = _device_of(data)
        L = _lib.lib()
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        pred = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev).reshape(-1)
        fake = _fake_of(data, dev)
        n = t.numel()
        kws = self.kws
        recon = _recognise(kws["recon_loss"], LU.recon_loss, ("alpha", "gamma", "norm", "cur_alpha")) if _given(kws, "recon_loss") else None
        rank = _recognise(kws["rank_loss"], LU.rank_loss, ("gamma", "norm", "add_weight")) if _given(kws, "rank_loss") else None
        which, disc_fn = _disc_which(kws)
        rc = recon or {}
        alpha = rc.get("alpha", 0.0) if rc.get("cur_alpha") is None else rc["cur_alpha"]
        res = torch.empty(_NRES, dtype=torch.float64, device=dev)
        wsb = L.advmil_surv_metrics_cont_workspace_bytes(n)
        ws = _ws(wsb, dev)
        _lib.check(L.advmil_surv_metrics_cont(_p(t), _p(e), _p(pred), _p(fake), n, float(alpha), float(rc.get("gamma", 1.0)),
                                              int(rc.get("norm", "l1") == "l2"), float(self.end_time), which or 0, _p(res), _p(ws), wsb,
                                              _stream(dev)), "surv_metrics_cont")
        if rank is not None and "loss_rank" in metrics:
            LU._rank_loss_launch(pred, t, e, rank.get("gamma", 1), rank.get("norm", "l1"), rank.get("add_weight", False), res[_RANK:_RANK + 4])
        r = res.cpu().tolist()                                   # the one device-to-host copy
        n_evt, n_non = r[9], r[10]
        out = dict()
        for m in metrics:
            if m == "c_index":
                out[m] = concordance_index(y, pred.reshape(-1, 1))
            elif m == "loss_rank":
                out[m] = 0 if not _given(kws, "rank_loss") else (r[_RANK] if rank is not None else kws["rank_loss"](pred, t, e).item())
            elif m == "loss_recon":
                out[m] = 0 if not _given(kws, "recon_loss") else (r[0] / n if recon is not None else kws["recon_loss"](pred, t, e).item())
            elif m == "loss_recon_org":
                out[m] = 0 if not _given(kws, "recon_loss") else (
                    r[1] / n if recon is not None else kws["recon_loss"](pred, t, e, cur_alpha=0.0).item())
            elif m == "mae":
                out[m] = r[2] / n
            elif m == "loss_fake_netD":
                if not _given(kws, "disc_loss"):
                    out[m] = 0
                else:
                    self._need_fake(fake)
                    out[m] = r[3] / n if disc_fn is None else disc_fn(None, fake).item()
            elif m == "loss_fake_netG":
                self._need_fake(fake)
                out[m] = -r[4] / n
            elif m == "avg_fake":
                self._need_fake(fake)
                out[m] = r[4] / n
            elif m == "event_t_rae":
                out[m] = _mean(r[5], n_evt)
            elif m == "nonevent_t_rae":
                out[m] = _mean(r[6], n_non)
            elif m == "event_t_nre":
                out[m] = _mean(r[7], n_evt)
            elif m == "nonevent_t_nre":
                out[m] = _mean(r[8], n_non)
        return out

    def time_error(self, data, gamma=1.0, n_boot=0, seed=0, level=0.95):
        """How wrong the predicted time is, with the censored patients' unknown event times replaced by Kaplan-Meier surrogates
        (eval/calibration.py, one call): `mae_hinge` (at `gamma` = 1 the `mae` metric), `mae_margin` and `mae_po`, each [P]: column 0 is
        the prediction the `c_index` metric uses, column 1 the median of `dist_y_hat` when the collector holds one -- then also
        `<key>_diff`, column 0 - column 1. NaN where undefined; with `n_boot` > 0 the percentile intervals `<key>_lo` / `<key>_hi` at
        `level` and `n_undefined` (more than 5 % of the resamples: ValueError)."""
        dev = _device_of(data)
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        pred = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev).reshape(-1, 1)
        if data.get("dist_y_hat") is not None:
            dist = _f32(data["dist_y_hat"], dev)
            pred = torch.cat([pred, dist.reshape(dist.shape[0], -1).median(dim=1, keepdim=True).values], dim=1)
        b = CB.bootstrap_calibration(e, t, pred=pred, gamma=gamma, n_boot=n_boot, seed=seed, level=level)
        return _calibration_dict(b, ("mae_hinge", "mae_margin", "mae_po"), n_boot)

    def d_calibration(self, data, bins=10, n_boot=0, seed=0, level=0.95):
        """Is the sampled distribution `dist_y_hat` calibrated (eval/calibration.py, one call): the share of a patient's samples beyond
        their own time is binned into `bins` bins, a censored patient spread over the bins below theirs; `d_cal_chi2`, its p-value
        `d_cal_p` (small: miscalibrated) and the bin masses `d_cal_bins`; with `n_boot` > 0 the percentile intervals and `n_undefined`."""
        if data.get("dist_y_hat") is None:
            raise ValueError("d_calibration scores the predicted distribution: the collector holds no 'dist_y_hat' "
                             "(run test_model with times_test_sample > 1)")
        dev = _device_of(data)
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        dist = _f32(data["dist_y_hat"], dev)
        p = CB.survival_at_own_time(t, dist_y_hat=dist.reshape(dist.shape[0], -1))
        b = CB.bootstrap_calibration(e, t, p_own=p, bins=bins, po=False, n_boot=n_boot, seed=seed, level=level)
        return _calibration_dict(b, ("d_cal_chi2", "d_cal_p"), n_boot)

    def _survival_estimate(self, data, times):
        """The survival function is the empirical one of the generator's sampled times `dist_y_hat` [n, S, 1]; the risk at t is 1 - S(t)."""
        if data.get("dist_y_hat") is None:
            raise ValueError("time_dependent scores the predicted distribution: the collector holds no 'dist_y_hat' "
                             "(run test_model with times_test_sample > 1)")
        dev = _device_of(data)
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        dist = _f32(data["dist_y_hat"], dev)
        dist = dist.reshape(dist.shape[0], -1)
        at = TD.default_times(e, t) if times is None else times
        surv = TD.survival_from_samples(dist, at)
        return e, t, at, surv, 1.0 - surv


class DiscSurv_Evaluator(_Evaluator):
    """Evaluator of a discrete-time model: y[:, 0] is the bin index, y_hat the hazards [n, bins]."""

    def __init__(self, **kws):
        self.kws = kws
        self.valid_metrics = ["c_index", "loss_mle", "loss_mle_org", "loss_fake_netD", "loss_fake_netG", "avg_fake"]

    def compute(self, data, metrics):
        self._check_metrics(metrics)
        dev = _device_of(data)
        L = _lib.lib()
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        hz = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev)
        hz = hz.reshape(hz.shape[0], -1)
        fake = _fake_of(data, dev)
        n, bins = hz.shape
        kws = self.kws
        mle = kws.get("mle_loss")
        fused = type(mle) is LU.SurvMLE
        which, disc_fn = _disc_which(kws)
        res = torch.empty(_NRES, dtype=torch.float64, device=dev)
        risk = torch.empty(n, dtype=torch.float32, device=dev)
        wsb = L.advmil_surv_metrics_disc_workspace_bytes(n)
        ws = _ws(wsb, dev)
        if not 1 <= bins <= 256:
            raise ValueError(f"DiscSurv_Evaluator: {bins} bins; the HIP path takes 1 to 256")
        _lib.check(L.advmil_surv_metrics_disc(_p(hz), hz.stride(0), _p(t), _p(e), _p(fake), n, bins, float(mle.alpha) if fused else 0.0,
                                              float(mle.eps) if fused else 1e-7, which or 0, _p(risk), _p(res), _p(ws), wsb, _stream(dev)),
                   "surv_metrics_disc")
        r = res.cpu().tolist()                                   # the one device-to-host copy
        if r[4] != 0:
            raise ValueError(f"DiscSurv_Evaluator: {int(r[4])} of {n} samples carry a bin index outside [0, {bins - 1}]")
        out = dict()
        for m in metrics:
            if m == "c_index":
                # (one bin: the reference's concordance_index takes an [n, 1] prediction for a time, not for hazards -- eval/cindex.py:34-36)
                out[m] = concordance_index(y, hz) if bins == 1 else concordance_index_censored(e, t, -risk, tied_tol=1e-08, device=dev)[0]
            elif m == "loss_mle":
                assert "mle_loss" in kws
                out[m] = r[0] / n if fused else mle(hz, t, e).item()
            elif m == "loss_mle_org":
                assert "mle_loss" in kws
                out[m] = r[1] / n if fused else mle(hz, t, e, cur_alpha=0.0).item()
            elif m == "loss_fake_netD":
                if not _given(kws, "disc_loss"):
                    out[m] = 0
                else:
                    self._need_fake(fake)
                    out[m] = r[2] / n if disc_fn is None else disc_fn(None, fake).item()
            elif m == "loss_fake_netG":
                self._need_fake(fake)
                out[m] = -r[3] / n
            elif m == "avg_fake":
                self._need_fake(fake)
                out[m] = r[3] / n
        return out


    def _bootstrap_c_index(self, data, n_boot, seed, level):
        dev = _device_of(data)
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        hz = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev)
        hz = hz.reshape(hz.shape[0], -1)
        n, bins = hz.shape
        if bins == 1:
            return bootstrap_concordance_index(y, hz, n_boot=n_boot, seed=seed, level=level)
        if bins > 256:
            raise ValueError(f"DiscSurv_Evaluator: {bins} bins; the HIP path takes 1 to 256")
        L = _lib.lib()
        res = torch.empty(_NRES, dtype=torch.float64, device=dev)
        risk = torch.empty(n, dtype=torch.float32, device=dev)    # the fused pass's risk: the bits `compute` ranks by
        wsb = L.advmil_surv_metrics_disc_workspace_bytes(n)
        ws = _ws(wsb, dev)
        _lib.check(L.advmil_surv_metrics_disc(_p(hz), hz.stride(0), _p(t), _p(e), None, n, bins, 0.0, 1e-7, 0, _p(risk), _p(res), _p(ws), wsb,
                                              _stream(dev)), "surv_metrics_disc")
        return bootstrap_risk(e, t, -risk, n_boot=n_boot, seed=seed, level=level)

    def _risk_estimate(self, data):
        dev = _device_of(data)
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        hz = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev)
        hz = hz.reshape(hz.shape[0], -1)
        n, bins = hz.shape
        if bins == 1:
            return _risks(y, hz)[:3]
        if bins > 256:
            raise ValueError(f"DiscSurv_Evaluator: {bins} bins; the HIP path takes 1 to 256")
        L = _lib.lib()
        res = torch.empty(_NRES, dtype=torch.float64, device=dev)
        risk = torch.empty(n, dtype=torch.float32, device=dev)    # the fused pass's risk: the bits `compute` ranks by
        wsb = L.advmil_surv_metrics_disc_workspace_bytes(n)
        ws = _ws(wsb, dev)
        _lib.check(L.advmil_surv_metrics_disc(_p(hz), hz.stride(0), _p(t), _p(e), None, n, bins, 0.0, 1e-7, 0, _p(risk), _p(res), _p(ws), wsb,
                                              _stream(dev)), "surv_metrics_disc")
        return e, t, -risk

    def d_calibration(self, data, bins=10, n_boot=0, seed=0, level=0.95):
        """Are the predicted hazards calibrated (eval/calibration.py, one call): prod_{l <= k} (1 - h_l) at a patient's own bin k is
        binned into `bins` bins, a censored patient spread over the bins below theirs; `d_cal_chi2`, its p-value `d_cal_p` (small:
        miscalibrated) and the bin masses `d_cal_bins`; with `n_boot` > 0 the percentile intervals and `n_undefined`."""
        dev = _device_of(data)
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        hz = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev)
        p = CB.survival_at_own_time(t, hazards=hz.reshape(hz.shape[0], -1))
        b = CB.bootstrap_calibration(e, t, p_own=p, bins=bins, po=False, n_boot=n_boot, seed=seed, level=level)
        return _calibration_dict(b, ("d_cal_chi2", "d_cal_p"), n_boot)

    def _survival_estimate(self, data, times):
        """The survival function is the product of the hazards' complements; times are bin indices (default: 0 ... bins - 2 below the
        largest observed bin, beyond which nothing is defined); the risk at t is 1 - S(t)."""
        dev = _device_of(data)
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        hz = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev)
        hz = hz.reshape(hz.shape[0], -1)
        if times is None:
            times = torch.arange(max(hz.shape[1] - 1, 1), device=dev, dtype=torch.float32)
            times = times[times < t.max()]
            if times.numel() == 0:
                raise ValueError("time_dependent: no bin index lies below the largest observed bin")
        surv = TD.survival_from_hazards(hz, times)
        return e, t, times, surv, 1.0 - surv


class CoxSurv_Evaluator(_Evaluator):
    """Performance evaluator for Cox-based survival model"""

    def __init__(self, **kws):
        self.kws = kws
        self.valid_metrics = ["c_index", "loss_ple"]

    def compute(self, data, metrics):
        self._check_metrics(metrics)
        dev = _device_of(data)
        L = _lib.lib()
        y = _f32(data["y"], dev)
        t, e = y[:, 0].contiguous(), y[:, 1].contiguous()
        pred = _f32(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"], dev).reshape(-1)
        n = t.numel()
        kws = self.kws
        fused = type(kws.get("ple_loss")) is LU.SurvPLE
        r = None
        if fused and "loss_ple" in metrics:
            res = torch.empty(_NRES, dtype=torch.float64, device=dev)
            wsb = L.advmil_ple_loss_workspace_bytes(n)
            ws = _ws(wsb, dev)
            _lib.check(L.advmil_ple_loss(_p(pred), _p(t), _p(e), n, _p(res[_PLE:_PLE + 2]), _p(ws), wsb, _stream(dev)), "ple_loss")
            r = res[_PLE:_PLE + 2].cpu().tolist()                # the one device-to-host copy
        out = dict()
        for m in metrics:
            if m == "c_index":
                out[m] = concordance_index(y, pred.reshape(-1, 1))
            elif m == "loss_ple":
                out[m] = 0 if not _given(kws, "ple_loss") else (r[0] if fused else kws["ple_loss"](pred, t, e).item())
        return out
