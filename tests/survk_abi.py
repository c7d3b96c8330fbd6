"""The nine C-ABI entries of csrc/survk.hip called directly (ctypes), for tests/test_survk_abi_gpu.py and tools/probe/surv_fuzz.py.
Inputs are numpy arrays; every output and workspace is a fresh torch.empty block, so tests.poison.poisoned_allocations decides what
they hold before the launch. Nothing here touches a device until one of the launch functions is called; the numpy helpers at the end
(hazard draws, the reference's float32 risk, the float64 slots of the continuous pass, the pair state of rank_loss) need none."""
import ctypes

import numpy as np
import torch

from tests.test_evaluator_cpu import fake_terms_f64, recon_f64

WHICH = {"bce": 0, "hinge": 1, "wasserstein": 2}


def _dev():
    return torch.device("cuda", 0)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).to(_dev())


def _lib_stream():
    from advmil_amd import _lib
    return _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _ws(nbytes):
    return torch.empty((int(nbytes) + 7) // 8, dtype=torch.float64, device=_dev())


def metrics_cont(t, e, pred, fake, alpha, gamma, norm, end_time, which):
    """advmil_surv_metrics_cont -> its 16 doubles (numpy)."""
    L, st = _lib_stream()
    td, ed, pd, fd = _up(t), _up(e), _up(pred), _up(fake)
    n = td.numel()
    out = torch.empty(16, dtype=torch.float64, device=_dev())
    wsb = L.advmil_surv_metrics_cont_workspace_bytes(n)
    ws = _ws(wsb)
    rc = L.advmil_surv_metrics_cont(_vp(td), _vp(ed), _vp(pd), _vp(fd), n, float(alpha), float(gamma), int(norm == "l2"), float(end_time),
                                    WHICH[which], _vp(out), _vp(ws), wsb, st)
    assert rc == 0, rc
    return out.cpu().numpy()


def metrics_disc(hz, t, e, fake, alpha, eps, which, pad=0):
    """advmil_surv_metrics_disc on hazards [n, bins] -> (its 16 doubles, risk [n] float32). `pad` > 0: the matrix is handed over with
    a pitch of bins + pad, the padding columns holding NaN."""
    L, st = _lib_stream()
    hz = np.ascontiguousarray(hz, dtype=np.float32)
    n, bins = hz.shape
    if pad:
        wide = np.full((n, bins + pad), np.nan, dtype=np.float32)
        wide[:, :bins] = hz
        hz = wide
    hd = torch.from_numpy(hz).to(_dev())
    td, ed, fd = _up(t), _up(e), _up(fake)
    out = torch.empty(16, dtype=torch.float64, device=_dev())
    risk = torch.empty(n, dtype=torch.float32, device=_dev())
    wsb = L.advmil_surv_metrics_disc_workspace_bytes(n)
    ws = _ws(wsb)
    rc = L.advmil_surv_metrics_disc(_vp(hd), bins + pad, _vp(td), _vp(ed), _vp(fd), n, bins, float(alpha), float(eps), WHICH[which],
                                    _vp(risk), _vp(out), _vp(ws), wsb, st)
    assert rc == 0, rc
    return out.cpu().numpy(), risk.cpu().numpy()


def ple(theta, t, e):
    """advmil_ple_loss -> out2 (numpy, 2 doubles: loss, sum E)."""
    L, st = _lib_stream()
    hd, td, ed = _up(theta), _up(t), _up(e)
    n = hd.numel()
    out = torch.empty(2, dtype=torch.float64, device=_dev())
    wsb = L.advmil_ple_loss_workspace_bytes(n)
    ws = _ws(wsb)
    rc = L.advmil_ple_loss(_vp(hd), _vp(td), _vp(ed), n, _vp(out), _vp(ws), wsb, st)
    assert rc == 0, rc
    return out.cpu().numpy()


def rank(pred, t, e, gamma, norm, add_weight, gout=None):
    """advmil_rank_loss_fwd (and _bwd when `gout` is a number) -> (state4 [4 doubles], loss as float32 scalar, dpred float32 | None)."""
    L, st = _lib_stream()
    pd, td, ed = _up(pred), _up(t), _up(e)
    n = pd.numel()
    l2, aw = int(norm == "l2"), int(bool(add_weight))
    state = torch.empty(4, dtype=torch.float64, device=_dev())
    loss = torch.empty((), dtype=torch.float32, device=_dev())
    wsb = L.advmil_rank_loss_workspace_bytes(n)
    ws = _ws(wsb)
    rc = L.advmil_rank_loss_fwd(_vp(pd), _vp(td), _vp(ed), n, float(gamma), l2, aw, _vp(state), _vp(loss), _vp(ws), wsb, st)
    assert rc == 0, rc
    dpred = None
    if gout is not None:
        g = torch.full((1,), float(gout), dtype=torch.float32, device=_dev())
        dp = torch.empty(n, dtype=torch.float32, device=_dev())
        rc = L.advmil_rank_loss_bwd(_vp(pd), _vp(td), _vp(ed), n, float(gamma), l2, aw, _vp(state), _vp(g), _vp(dp), st)
        assert rc == 0, rc
        dpred = dp.cpu().numpy()
    return state.cpu().numpy(), loss.cpu().numpy().reshape(()), dpred


# ---- numpy sides ------------------------------------------------------------------------------------------------------------------
def hazard_draw(rs, kind, n, bins):
    if kind == "levels_123":
        return rs.choice(np.array([0.1, 0.2, 0.3], dtype=np.float32), size=(n, bins))
    if kind == "levels_19":
        return rs.choice(np.array([0.1, 0.9], dtype=np.float32), size=(n, bins))
    return (np.float32(0.05) + np.float32(0.9) * rs.rand(n, bins).astype(np.float32)).astype(np.float32)


def numpy_risk(hz):
    """The reference's expression (eval/cindex.py), float32 throughout."""
    hz = np.ascontiguousarray(hz, dtype=np.float32)
    r = np.sum(np.cumprod(1.0 - hz, axis=1), axis=1)
    assert r.dtype == np.float32
    return r


def want_cont_slots(t, e, pred, fake, alpha, gamma, norm, end_time, which):
    """-> the eleven slots in float64, each divided by the count the Python layer divides it by (None: nothing to divide by), and
    the two counts."""
    t64, e64, p64 = t.astype(np.float64), e.astype(np.float64), pred.astype(np.float64)
    evt, non = e64 == 1, e64 == 0
    mean = lambda a: float(np.mean(a)) if a.size else None          # noqa: E731
    relu = np.maximum(t64[non] - p64[non], 0.0)
    f = None if fake is None else fake.astype(np.float64)
    return [recon_f64(p64, t64, e64, alpha, gamma, norm), recon_f64(p64, t64, e64, 0.0, gamma, norm), recon_f64(p64, t64, e64, 0.0, 1.0, "l1"),
            0.0 if f is None else float(np.mean(fake_terms_f64(f, which))), 0.0 if f is None else float(np.mean(f)),
            mean(np.abs(t64[evt] - p64[evt]) / end_time), mean(relu / end_time), mean((p64[evt] - t64[evt]) / end_time),
            mean(-relu / end_time)], int(evt.sum()), int(non.sum())


def pair_state_f64(pred, t, e):
    """-> (P, M as the largest float32 pred_i - pred_j over the pairs, Z in float64) from numpy."""
    mask = (t.reshape(-1, 1) < t.reshape(1, -1)) & (e.reshape(-1, 1) == 1)
    x32 = (pred.reshape(-1, 1) - pred.reshape(1, -1))
    assert x32.dtype == np.float32
    P = int(mask.sum())
    if P == 0:
        return 0, 0.0, 0.0
    M = x32[mask].max()
    x64 = pred.astype(np.float64).reshape(-1, 1) - pred.astype(np.float64).reshape(1, -1)
    return P, M, float(np.exp(x64[mask] - x64[mask].max()).sum())
