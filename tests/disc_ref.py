"""float64 numpy restatement of the discrete-time adversarial task's label rows and generator loss (task: disc_gansurv):
get_label_mask (reference utils/func.py:59-64) as model_handler.py:382-383, 399, 445, 460 call it, SurvMLE (loss/utils.py:98-134) with
its clamps, their gradients, and the {total, mle, gen} triple the step logs (model_handler.py:472-494). Pinned against the reference's
own functions by tests/golden/gen_golden_disc.py (tests/golden/ORACLE_PIN_disc.json). No torch, no GPU."""
import numpy as np


def get_label_mask(t, e, bins):
    """t[n], e[n] -> (label[n, bins], mask[n, bins]) as float64. The reference's third-from-last argument is named `c` but receives the
    EVENT indicator: label = (z > t) where e != 0, (z == t) elsewhere; mask = (z <= t)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    e = np.asarray(e, dtype=np.float64).reshape(-1, 1)
    z = np.arange(bins, dtype=np.float64).reshape(1, -1) * np.ones((t.shape[0], 1))
    label = np.where(e != 0, z > t, z == t).astype(np.float64)
    mask = (z <= t).astype(np.float64)
    return label, mask


def real_rows(t, e, bins):
    """The real pairs' label rows label * mask: all zeros for an event bag, one-hot at t for a censored one."""
    label, mask = get_label_mask(t, e, bins)
    return label * mask


def fake_rows(pred, t, e, bins):
    """The fake pairs' label rows pred * mask."""
    return np.asarray(pred, dtype=np.float64) * get_label_mask(t, e, bins)[1]


def surv_mle_terms(hz, t, e, alpha=0.0, eps=1e-7):
    """Per-row SurvMLE terms and their gradient, split by log argument.
    -> dict: term[n]; grad[n, K] = d term / d hz; and per log argument X in ("S_t", "h_t", "S_t1") -- S_padded[t], hz[t], S_padded[t + 1]:
    arg_X[n] its value, clamped_X[n] (bool: the argument lies below eps, the log is the constant log(eps)), grad_X[n, K] its weighted
    share of `grad` (all zeros where clamped: torch's clamp passes the gradient only where the argument is >= the bound)."""
    hz = np.asarray(hz, dtype=np.float64)
    n, K = hz.shape
    ti = np.asarray(t, dtype=np.float64).reshape(-1).astype(np.int64)           # t.long(): truncation
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    assert np.all((ti >= 0) & (ti < K))
    c = 1.0 - e
    S = np.cumprod(1.0 - hz, axis=1)
    Sp = np.concatenate([np.ones((n, 1)), S], axis=1)
    r = np.arange(n)
    a_t, a_h, a_t1 = Sp[r, ti], hz[r, ti], Sp[r, ti + 1]
    unc = -(1.0 - c) * (np.log(np.maximum(a_t, eps)) + np.log(np.maximum(a_h, eps)))
    cen = -c * np.log(np.maximum(a_t1, eps))
    term = (1.0 - alpha) * (cen + unc) + alpha * unc
    cl_t, cl_h, cl_t1 = a_t < eps, a_h < eps, a_t1 < eps
    j = np.arange(K).reshape(1, -1)
    # d log prod_{i<m}(1 - h_i) / d h_j = -1 / (1 - h_j) for j < m (an unclamped product has no zero factor); term = unc + (1 - alpha) cen
    inv = 1.0 / np.where(hz == 1.0, 1.0, 1.0 - hz)
    w_unc, w_cen = (1.0 - c)[:, None], ((1.0 - alpha) * c)[:, None]
    g_t = np.where((j < ti[:, None]) & ~cl_t[:, None], w_unc * inv, 0.0)
    g_h = np.where((j == ti[:, None]) & ~cl_h[:, None], -w_unc / np.where(cl_h, 1.0, a_h)[:, None], 0.0)
    g_t1 = np.where((j <= ti[:, None]) & ~cl_t1[:, None], w_cen * inv, 0.0)
    return dict(term=term, grad=g_t + g_h + g_t1, arg_S_t=a_t, arg_h_t=a_h, arg_S_t1=a_t1, clamped_S_t=cl_t, clamped_h_t=cl_h,
                clamped_S_t1=cl_t1, grad_S_t=g_t, grad_h_t=g_h, grad_S_t1=g_t1)


def surv_mle(hz, t, e, alpha=0.0, eps=1e-7):
    """SurvMLE.forward -> (mean of the terms, its gradient wrt hz)."""
    d = surv_mle_terms(hz, t, e, alpha, eps)
    n = d["term"].shape[0]
    return float(d["term"].mean()), d["grad"] / n


def g_loss(hz, t, e, vis, fake, alpha, eps, coef, n_fake=None, n_vis=None):
    """The generator step's loss without the L1 term (model_handler.py:472-484): SurvMLE over the VISIBLE bags' unmasked hazards (0 when
    none is visible) + coef * (-mean fake). vis: [n] of 0/1 or None = all visible.
    -> (out3 = [total, mle, gen], g_hz[n, K] = d mle / d hz, g_fake[n] = d total / d fake, terms dict of surv_mle_terms)."""
    hz = np.asarray(hz, dtype=np.float64)
    fake = np.asarray(fake, dtype=np.float64).reshape(-1)
    n = hz.shape[0]
    v = np.ones(n) if vis is None else np.asarray(vis, dtype=np.float64).reshape(-1)
    n_fake = n if n_fake is None else n_fake
    n_vis = int(v.sum()) if n_vis is None else n_vis
    d = surv_mle_terms(hz, t, e, alpha, eps)
    if n_vis > 0:
        mle = float((v * d["term"]).sum() / n_vis)
        g_hz = v[:, None] * d["grad"] / n_vis
    else:
        mle, g_hz = 0.0, np.zeros_like(hz)
    gen = float(-fake.sum() / n_fake)
    return np.array([mle + coef * gen, mle, gen]), g_hz, np.full(n, -coef / n_fake), d


# ---- the loss cases shared by the golden generator (run through the reference's SurvMLE in float64) and the kernel tests ------------
LOSS_B, LOSS_K = (1, 5, 16, 32), (1, 4, 7, 32)


def _case(rs, B, K, kind, alpha):
    hz = (1.0 / (1.0 + np.exp(-rs.standard_normal((B, K))))).astype(np.float32)
    t = rs.integers(0, K, size=B)
    t[0] = K - 1                                     # the t + 1 == K gather
    if B > 1:
        t[1] = 0
    elif kind == "censored":
        t[0] = 0
    e = {"event": np.ones(B), "censored": np.zeros(B), "mixed": (np.arange(B) + 1) % 2}[kind]
    fake = rs.standard_normal(B).astype(np.float32)
    return dict(name=f"B{B}_K{K}_{kind}_a{alpha}", hz=hz, t=t.astype(np.float32), e=e.astype(np.float32), fake=fake, alpha=alpha, eps=1e-7)


def loss_cases():
    """B x K x {all-event, all-censored, mixed} x alpha in {0, 0.3}: hazards sigmoid(N(0, 1)) as float32, every batch with t = K - 1 and
    (B > 1) t = 0; plus `extreme`: entries 1e-9 and 1 - 1e-9 (float32: exactly 1), which clamp every kind of log argument."""
    rs = np.random.default_rng(20240607)
    out = []
    for B in LOSS_B:
        for K in LOSS_K:
            for kind in ("event", "censored", "mixed"):
                for alpha in (0.0, 0.3):
                    out.append(_case(rs, B, K, kind, alpha))
    c = _case(rs, 16, 7, "mixed", 0.3)
    c["name"] = "extreme"
    c["t"] = ((np.arange(16) + (np.arange(16) >= 8)) % 7).astype(np.float32)      # rows 0-7: hz[t] itself is 1e-9
    for b in range(16):
        c["hz"][b, b % 7] = 1e-9
        c["hz"][b, (b + 3) % 7] = 1.0 - 1e-9
        c["hz"][b, (b + 5) % 7] = 1e-9 if b % 2 else c["hz"][b, (b + 5) % 7]
    out.append(c)
    return out


def extreme_case_f64():
    """The `extreme` case with the two extreme values carried in float64 (1 - h = 1e-9 instead of 0): restatement-vs-reference only."""
    c = dict(loss_cases()[-1])
    hz = c["hz"].astype(np.float64)
    hz[c["hz"] == np.float32(1e-9)] = 1e-9
    hz[c["hz"] == np.float32(1.0)] = 1.0 - 1e-9
    c["hz"], c["name"] = hz, "extreme_f64"
    return c
