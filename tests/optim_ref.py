"""Float64 restatement of the optimizers behind advmil_optim_step / advmil_amd.optim.FlatOptim: torch.optim.Adam, AdamW and Adadelta,
the reference's optim/nadam.py::Nadam and optim/radam.py::RAdam, and its optim/lookahead.py wrapper -- numpy only, one flat array.
Pinned to those classes by tests/golden/optim_v1.npz (tests/golden/gen_golden_optim.py).

The gradient the update sees is grad * grad_scale + l1_coef * sign(p) (the L1 sub-gradient the HIP kernels fold in); `wd` is the
per-element weight decay (the reference's add_weight_decay filter as an array)."""
import math

import numpy as np

KINDS = ("adam", "adamw", "nadam", "radam", "adadelta")
STATE_NAMES = {k: ("exp_avg", "exp_avg_sq") for k in KINDS}
STATE_NAMES["adadelta"] = ("square_avg", "acc_delta")


def radam_terms(t, lr, beta1, beta2):
    """-> (N_sma, step_size) of optim/radam.py:59-70 at step t."""
    beta2_t = beta2 ** t
    n_max = 2.0 / (1.0 - beta2) - 1.0
    n_sma = n_max - 2.0 * t * beta2_t / (1.0 - beta2_t)
    if n_sma >= 5:
        step_size = lr * math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - beta1 ** t)
    else:
        step_size = lr / (1 - beta1 ** t)
    return n_sma, step_size


def radam_first_rectified_step(beta2=0.999):
    """The first step at which RAdam takes its rectified branch (N_sma >= 5)."""
    t = 1
    while radam_terms(t, 1.0, 0.9, beta2)[0] < 5:
        t += 1
    return t


class Ref:
    """One optimizer over one flat float64 array. Attributes: p, s1, s2 (the two state arrays, STATE_NAMES[kind]), step, m_schedule
    (nadam), slow (lookahead: None until the first sync), la_step."""

    def __init__(self, kind, p0, wd=0.0, lr=1e-3, betas=(0.9, 0.999), eps=None, rho=0.9, schedule_decay=4e-3, l1_coef=0.0,
                 lookahead=False, alpha=0.5, k=6):
        assert kind in KINDS, kind
        self.kind, self.lookahead, self.alpha, self.k = kind, bool(lookahead), float(alpha), int(k)
        self.p = np.array(p0, dtype=np.float64).reshape(-1).copy()
        self.wd = np.broadcast_to(np.asarray(wd, dtype=np.float64), self.p.shape).copy()
        self.lr, self.betas, self.rho, self.schedule_decay, self.l1_coef = float(lr), (float(betas[0]), float(betas[1])), float(rho), float(schedule_decay), float(l1_coef)
        self.eps = float((1e-6 if kind == "adadelta" else 1e-8) if eps is None else eps)
        self.s1, self.s2 = np.zeros_like(self.p), np.zeros_like(self.p)
        self.step, self.m_schedule, self.slow, self.la_step = 0, 1.0, None, 0
        self.rectified = []                 # radam: the branch of every step taken
        self.syncs = []                     # lookahead: (step, "create" | "blend") of every sync

    def do_step(self, grad, grad_scale=1.0):
        p, lr, (b1, b2), eps, wd = self.p, self.lr, self.betas, self.eps, self.wd
        g = np.asarray(grad, dtype=np.float64).reshape(-1) * grad_scale
        if self.l1_coef != 0.0:
            g = g + self.l1_coef * np.sign(p)
        self.step += 1
        t = self.step
        if self.kind == "adadelta":
            g = g + wd * p
            self.s1 = self.rho * self.s1 + (1 - self.rho) * g * g
            delta = np.sqrt(self.s2 + eps) / np.sqrt(self.s1 + eps) * g
            self.s2 = self.rho * self.s2 + (1 - self.rho) * delta * delta
            p = p - lr * delta
        elif self.kind in ("adam", "adamw"):
            if self.kind == "adam":
                g = g + wd * p
            else:
                p = p * (1 - lr * wd)
            self.s1 = b1 * self.s1 + (1 - b1) * g
            self.s2 = b2 * self.s2 + (1 - b2) * g * g
            denom = np.sqrt(self.s2) / math.sqrt(1 - b2 ** t) + eps
            p = p - lr / (1 - b1 ** t) * self.s1 / denom
        elif self.kind == "nadam":
            g = g + wd * p
            sd = self.schedule_decay
            mu_t = b1 * (1.0 - 0.5 * (0.96 ** (t * sd)))
            mu_t1 = b1 * (1.0 - 0.5 * (0.96 ** ((t + 1) * sd)))
            ms_new = self.m_schedule * mu_t
            ms_next = ms_new * mu_t1
            self.m_schedule = ms_new
            self.s1 = b1 * self.s1 + (1 - b1) * g
            self.s2 = b2 * self.s2 + (1 - b2) * g * g
            denom = np.sqrt(self.s2 / (1 - b2 ** t)) + eps
            p = p - lr * (1 - mu_t) / (1 - ms_new) * g / denom
            p = p - lr * mu_t1 / (1 - ms_next) * self.s1 / denom
        else:   # radam
            self.s2 = b2 * self.s2 + (1 - b2) * g * g
            self.s1 = b1 * self.s1 + (1 - b1) * g
            n_sma, step_size = radam_terms(t, lr, b1, b2)
            p = p - wd * lr * p
            if n_sma >= 5:
                p = p - step_size * self.s1 / (np.sqrt(self.s2) + eps)
            else:
                p = p - step_size * self.s1
            self.rectified.append(bool(n_sma >= 5))
        if self.lookahead:
            self.la_step += 1
            if self.la_step % self.k == 0:
                if self.slow is None:               # created as a copy of the fast weights: this sync changes nothing
                    self.slow = p.copy()
                    self.syncs.append((self.step, "create"))
                else:
                    self.syncs.append((self.step, "blend"))
                self.slow = self.slow + self.alpha * (p - self.slow)
                p = self.slow.copy()
        self.p = p
        return p


def bound(p, p64, p0, steps):
    """(error, bound) of the parity check: 2e-5 of the displacement plus two fp32 roundings of the stored parameter per step."""
    p64 = np.asarray(p64, dtype=np.float64)
    err = float(np.abs(np.asarray(p, dtype=np.float64) - p64).max())
    return err, 2e-5 * float(np.abs(p64 - np.asarray(p0, dtype=np.float64)).max()) + 2 * steps * 2.0 ** -24 * float(np.abs(p64).max())


# ---- the seeded run of the fixture (shared by the generator and the tests): two tensors, a no-decay vector and a decayed matrix
FIX_SHAPES = ((1003,), (40, 100))            # 5 003 elements
FIX_STEPS, FIX_HALVE_AT = 16, 8              # the lr is halved before step 9
FIX_LR, FIX_WD = 1e-2, 5e-4
FIX_CASES = ("adamw", "nadam", "radam", "adadelta", "lookahead_adam", "lookahead_nadam", "lookahead_radam")


def fix_inputs():
    """-> (p0 [5003], wd [5003], grads [FIX_STEPS, 5003]) float64, the values float32-exact (the fp32 runs see the same numbers)."""
    rs = np.random.RandomState(20240607)
    n = sum(int(np.prod(s)) for s in FIX_SHAPES)
    p0 = (rs.standard_normal(n) * 0.1).astype(np.float32).astype(np.float64)
    base = rs.standard_normal(n) * 1e-2
    grads = np.stack([(base * (1.0 + 0.5 * rs.standard_normal(n))).astype(np.float32).astype(np.float64) for _ in range(FIX_STEPS)])
    wd = np.concatenate([np.zeros(int(np.prod(FIX_SHAPES[0]))), np.full(int(np.prod(FIX_SHAPES[1])), FIX_WD)])
    return p0, wd, grads


def fix_run(case, p0, wd, grads, steps=FIX_STEPS):
    """The fixture's run through the restatement -> Ref after `steps` steps."""
    name = case.split("_")[-1]
    r = Ref(name, p0, wd=wd, lr=FIX_LR, lookahead=case.startswith("lookahead_"))
    for t in range(steps):
        if t == FIX_HALVE_AT:
            r.lr *= 0.5
        r.do_step(grads[t])
    return r
