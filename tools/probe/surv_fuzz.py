#!/usr/bin/env python3
"""Randomised checks of the survival kernels (csrc/survk.hip) at the C ABI against float64: the continuous evaluator's eleven slots,
the discrete evaluator's four sums plus its risk against numpy's float32 expression BIT FOR BIT, SurvPLE, and rank_loss forward
(loss and the state array) and backward (gradient). Cohorts of 1 to 1500 samples, time and estimate levels on and off, event shares
from 0 to 1 inclusive, every loss kind / norm / alpha / add_weight, theta in [-12, 14], 1 to 256 bins with quantised, saturating and
continuous hazards, a row pitch above the bin count. usage: surv_fuzz.py [cases per family] [seed]

The draws (`draws`) and the float64 sides (`want_*`) need no device; tests/test_evaluator_cpu.py replays the suite's fixed-seed leg
through them. The categorical choices of a family (its KINDS) are cycled by the case number, so every kind occurs from nine cases on;
everything else is drawn.

rank_loss and the l1 hinge: a pair with |gamma + x| < 1e-6 in float64 may take the other branch in float32, which moves the gradient by
one pair's weight -- a property of the data. Such a draw is left out, and the run FAILS if more than 5 % of its rank_loss draws are.
The draws are built so that this does not happen: estimates lie on a dyadic grid (2^-18, or 1/64) with gamma an odd multiple of half
the spacing, or on k/40 with a gamma no difference of levels comes near."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import survk_abi as K  # noqa: E402
from tests.test_evaluator_cpu import TOL, fake_terms_f64, mle_f64, ple_f64, rank_loss_f64  # noqa: E402

FAMILIES = ("cont", "disc", "ple", "rank_fwd", "rank_bwd")
WHICH = ("bce", "hinge", "wasserstein")
RANK_KINDS = (("l1", False), ("l1", True), ("l2", False), ("l2", True))
HAZARDS = ("levels_123", "levels_19", "continuous")
KINDS = {"cont": [(w, nm) for nm in ("l1", "l2") for w in WHICH], "disc": [(h, WHICH[(i + j) % 3]) for j in range(3) for i, h in enumerate(HAZARDS)],
         "ple": ["clamped", "plain"], "rank_fwd": list(RANK_KINDS), "rank_bwd": list(RANK_KINDS)}
MAX_SKIPPED = 0.05
HINGE_MARGIN = 1e-6


def cohort(rnd, rs):
    """-> n, t, e (float32): 1 to 1500 samples (small cohorts favoured), time levels off / 3 / 50, event share 0, 0.1, 0.5, 0.9 or 1."""
    n = rnd.choice((rnd.randint(1, 8), rnd.randint(1, 300), rnd.randint(1, 1500)))
    lv = rnd.choice((0, 3, 50))
    t = rs.rand(n).astype(np.float32)
    if lv:
        t = (np.floor(t * lv) / lv).astype(np.float32)
    share = rnd.choice((0.0, 0.1, 0.5, 0.9, 1.0))
    e = (rs.rand(n) < share).astype(np.float32) if 0.0 < share < 1.0 else np.full(n, share, dtype=np.float32)
    return n, t, e, dict(n=n, time_levels=lv, event_share=share)


def draw_cont(rnd, rs, i):
    which, norm = KINDS["cont"][i % len(KINDS["cont"])]
    n, t, e, info = cohort(rnd, rs)
    lv = rnd.choice((0, 40))
    pred = rs.rand(n).astype(np.float32)
    if lv:
        pred = (np.floor(pred * lv) / lv).astype(np.float32)
    fake = None if rnd.random() < 0.15 else (rnd.choice((2.0, 30.0)) * (2.0 * rs.rand(n) - 1.0)).astype(np.float32)
    return dict(info, kind=(which, norm), t=t, e=e, pred=pred, fake=fake, which=which, norm=norm, est_levels=lv, alpha=rnd.choice((0.0, 0.3, 1.0)),
                gamma=rnd.choice((0.137, 1.0)), end_time=rnd.choice((1.0, 7.5)))


def draw_disc(rnd, rs, i):
    hkind, which = KINDS["disc"][i % len(KINDS["disc"])]
    n, _, e, info = cohort(rnd, rs)
    bins = rnd.choice((rnd.randint(1, 9), rnd.randint(1, 256), rnd.choice((127, 128, 129, 255, 256))))
    hz = K.hazard_draw(rs, hkind, n, bins)
    t = np.floor(rs.rand(n) * bins).astype(np.float32)
    fake = (4.0 * rs.rand(n) - 2.0).astype(np.float32)
    return dict(info, kind=(hkind, which), hz=hz, t=t, e=e, fake=fake, which=which, bins=bins, alpha=rnd.choice((0.0, 0.3, 1.0)), pad=rnd.choice((0, 0, 3)))


def draw_ple(rnd, rs, i):
    kind = KINDS["ple"][i % 2]
    n, t, e, info = cohort(rnd, rs)
    hi = 14.0 if kind == "clamped" else 9.0
    theta = (-12.0 + (hi + 12.0) * rs.rand(n)).astype(np.float32)
    if kind == "clamped":
        theta[rnd.randrange(n)] = 13.5                            # at least one value above the clamp at 10
    return dict(info, kind=kind, theta=theta, t=t, e=e)


def draw_rank(rnd, rs, i, family):
    norm, aw = KINDS[family][i % 4]
    n, t, e, info = cohort(rnd, rs)
    grid = rnd.choice(("fine", "sixtyfourths", "fortieths"))
    u = rs.rand(n)
    if grid == "fine":                                            # estimate levels off: 2^18 levels, practically no ties
        pred, gamma = np.floor(u * 2 ** 18) / 2 ** 18, (2 * rnd.randrange(0, 2 ** 18) + 1) / 2 ** 19
    elif grid == "sixtyfourths":
        pred, gamma = np.floor(u * 64) / 64, (2 * rnd.randrange(0, 64) + 1) / 128
    else:
        pred, gamma = np.floor(u * 40) / 40, 0.137
    scale = rnd.choice((1.0, 16.0)) if grid != "fortieths" else 1.0     # 16: the softmax weights span e^-16 to 1
    pred = (scale * (pred - 0.5)).astype(np.float32)
    return dict(info, kind=(norm, aw), pred=pred, t=t, e=e, gamma=gamma, norm=norm, add_weight=aw, grid=grid, scale=scale,
                gout=rnd.choice((1.0, -2.5)))


def draws(ncase, seed):
    """-> {family: [draw, ...]}: the cases of one run, the same on every machine."""
    rnd = random.Random(seed)
    rs = np.random.RandomState(rnd.randrange(1 << 30))
    out = {}
    for fam in FAMILIES:
        if fam.startswith("rank"):
            out[fam] = [draw_rank(rnd, rs, i, fam) for i in range(ncase)]
        else:
            out[fam] = [{"cont": draw_cont, "disc": draw_disc, "ple": draw_ple}[fam](rnd, rs, i) for i in range(ncase)]
    return out


# ---- float64 sides ----------------------------------------------------------------------------------------------------------------
def want_cont(d):
    return K.want_cont_slots(d["t"], d["e"], d["pred"], d["fake"], d["alpha"], d["gamma"], d["norm"], d["end_time"], d["which"])


def want_disc(d):
    """-> ([mle at alpha, mle at 0, mean fake term, mean fake], numpy's float32 risk)."""
    e64, f = d["e"].astype(np.float64), d["fake"].astype(np.float64)
    return [mle_f64(d["hz"], d["t"], e64, d["alpha"]), mle_f64(d["hz"], d["t"], e64, 0.0), float(np.mean(fake_terms_f64(f, d["which"]))),
            float(np.mean(f))], K.numpy_risk(d["hz"])


def want_ple(d):
    return ple_f64(d["theta"], d["t"], d["e"])


def want_rank(d):
    """-> (loss, gradient, smallest |gamma + x| over the pairs, (P, M, Z))."""
    loss, grad, margin = rank_loss_f64(d["pred"], d["t"], d["e"], d["gamma"], d["norm"], d["add_weight"])
    return loss, grad, margin, K.pair_state_f64(d["pred"], d["t"], d["e"])


def left_out(d, margin):
    """A rank_loss draw is left out only when an l1 hinge could take the other branch in float32."""
    return d["norm"] == "l1" and margin < HINGE_MARGIN


def rel(got, want):
    return abs(got - want) / max(1.0, abs(want))


# ---- the run ----------------------------------------------------------------------------------------------------------------------
def main(ncase, seed):
    cases = draws(ncase, seed)
    worst = {f: 0.0 for f in FAMILIES}

    for d in cases["cont"]:
        out = K.metrics_cont(d["t"], d["e"], d["pred"], d["fake"], d["alpha"], d["gamma"], d["norm"], d["end_time"], d["which"])
        want, n_evt, n_non = want_cont(d)
        tag = ("cont", d["n"], d["kind"], d["alpha"], d["gamma"], d["end_time"], d["event_share"])
        assert out[9] == n_evt and out[10] == n_non and not out[11:].any(), (tag, out[9:])
        for q, div in enumerate((d["n"],) * 5 + (n_evt, n_non, n_evt, n_non)):
            if want[q] is None:
                assert out[q] == 0.0, (tag, q, out[q])
                continue
            err = rel(float(out[q]) / div, want[q])
            worst["cont"] = max(worst["cont"], err)
            assert err <= TOL, (tag, q, float(out[q]) / div, want[q])
    print("cont ok", worst["cont"], flush=True)

    risk_rows = 0
    for d in cases["disc"]:
        out, risk = K.metrics_disc(d["hz"], d["t"], d["e"], d["fake"], d["alpha"], 1e-7, d["which"], pad=d["pad"])
        want, want_risk = want_disc(d)
        tag = ("disc", d["n"], d["bins"], d["kind"], d["alpha"], d["pad"])
        assert out[4] == 0.0 and not out[5:].any(), (tag, out[4:])
        for q in range(4):
            err = rel(float(out[q]) / d["n"], want[q])
            worst["disc"] = max(worst["disc"], err)
            assert err <= TOL, (tag, q, float(out[q]) / d["n"], want[q])
        diff = int((risk.view(np.int32) != want_risk.view(np.int32)).sum())
        assert diff == 0, (tag, "risk bits differ in", diff, "rows")
        risk_rows += d["n"]
    print("disc ok", worst["disc"], "risk bit-equal in", risk_rows, "rows", flush=True)

    for d in cases["ple"]:
        out = K.ple(d["theta"], d["t"], d["e"])
        err = rel(float(out[0]), want_ple(d))
        worst["ple"] = max(worst["ple"], err)
        assert err <= TOL and out[1] == float(d["e"].sum()), ("ple", d["n"], d["kind"], float(out[0]), want_ple(d), out[1])
    print("ple ok", worst["ple"], flush=True)

    skipped = 0
    for fam in ("rank_fwd", "rank_bwd"):
        for d in cases[fam]:
            want_loss, want_grad, margin, (P, M, Z) = want_rank(d)
            if left_out(d, margin):
                skipped += 1
                continue
            state, loss, grad = K.rank(d["pred"], d["t"], d["e"], d["gamma"], d["norm"], d["add_weight"], gout=d["gout"] if fam == "rank_bwd" else None)
            tag = (fam, d["n"], d["kind"], d["gamma"], d["grid"], d["scale"], d["event_share"])
            if fam == "rank_fwd":
                err = abs(float(loss) - want_loss) / abs(want_loss) if want_loss else abs(float(loss))
                assert err <= TOL, (tag, float(loss), want_loss)
                assert state[3] == float(P) and state[2] == (float(M) if d["add_weight"] else 0.0), (tag, state, P, M)
                ez = rel(float(state[1]), Z if d["add_weight"] else float(P))
                assert ez <= TOL, (tag, state[1], Z)
                err = max(err, ez)
            else:
                gmax = float(np.abs(want_grad).max()) * abs(d["gout"])
                dg = float(np.abs(grad.astype(np.float64) - d["gout"] * want_grad).max())
                err = dg / gmax if gmax else dg
                assert err <= TOL, (tag, dg, gmax)
            worst[fam] = max(worst[fam], err)
        print(fam, "ok", worst[fam], flush=True)
    assert skipped <= MAX_SKIPPED * 2 * ncase, ("rank_loss draws left out", skipped, "of", 2 * ncase)
    print("rank_loss draws left out:", skipped, "of", 2 * ncase)
    print("all ok", worst)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 40, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
