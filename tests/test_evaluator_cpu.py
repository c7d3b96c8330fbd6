"""CPU: the survival evaluators' fixture (tests/golden/evaluator_v1.json, results of the reference's eval/evaluator.py and
loss/utils.py::rank_loss) against a float64 restatement of the formulas written HERE, so fixture and restatement pin each other; the
public surface (names, valid_metrics, prepare_evaluator, failure without a device) and the workspace queries.

The restatement (`want_*`, `rank_loss_f64`) is also what tests/test_evaluator_gpu.py and tests/test_rank_loss_gpu.py use where the
fixture holds no value (generic route, n = 3000)."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import cindex_oracle as CO
from tests.golden import gen_golden_evaluator as G

GOLD = json.load(open(G.FIXTURE))
GOLD2 = json.load(open(G.FIXTURE2))      # quantised / saturating hazards (discrete only)
TOL = 2e-5


def close(got, want, tol=TOL):
    if isinstance(want, float) and math.isnan(want):
        return isinstance(got, float) and math.isnan(got)
    return abs(got - want) <= tol * max(1.0, abs(want))


# ---- float64 restatement -------------------------------------------------------------------------------------------------------
def fake_terms_f64(f, which):
    if which == "bce":
        return -(1.0 - np.log(1.0 / (1.0 + np.exp(-f)) + 1e-8))
    if which == "hinge":
        return np.maximum(1.0 + f, 0.0)
    return f


def recon_f64(p, t, e, alpha, gamma, norm):
    obs, cen = e * np.abs(p - t), (1.0 - e) * np.maximum(gamma - (p - t), 0.0)
    if norm == "l2":
        obs, cen = obs * obs, cen * cen
    return float(np.mean((1.0 - alpha) * (obs + cen) + alpha * obs))


def _mean(a):
    return float(np.mean(a)) if a.size else float("nan")


def rank_loss_f64(pred, t, e, gamma, norm, add_weight):
    """-> (loss, d loss / d pred, smallest |gamma + x| over the pairs) in float64 (torch autograd on the pair matrix)."""
    p = torch.tensor(np.asarray(pred, dtype=np.float64).reshape(-1), requires_grad=True)
    t = torch.tensor(np.asarray(t, dtype=np.float64).reshape(-1))
    e = torch.tensor(np.asarray(e, dtype=np.float64).reshape(-1))
    mask = (t.view(-1, 1) < t.view(1, -1)) & (e.view(-1, 1) == 1)
    if not bool(mask.any()):
        return 0.0, np.zeros(p.numel()), float("inf")
    x = p.view(-1, 1) - p.view(1, -1)
    L = torch.relu(gamma + x)
    if norm == "l2":
        L = L * L
    if add_weight:
        w = torch.softmax(x[mask], dim=0)
    else:
        w = torch.full((int(mask.sum()),), 1.0 / int(mask.sum()), dtype=torch.float64)
    loss = (L[mask] * w).sum()
    loss.backward()
    return float(loss.detach()), p.grad.numpy().copy(), float((gamma + x[mask]).detach().abs().min())


def want_cont(y, pred, fake, c, gamma=G.GAMMA):
    y, p, f = y.astype(np.float64), pred.astype(np.float64).reshape(-1), fake.astype(np.float64).reshape(-1)
    t, e = y[:, 0], y[:, 1]
    evt, non = e == 1, e == 0
    return {"loss_rank": rank_loss_f64(p, t, e, gamma, c["norm"], c["add_weight"])[0],
            "loss_recon": recon_f64(p, t, e, c["alpha"], gamma, c["norm"]),
            "loss_recon_org": recon_f64(p, t, e, 0.0, gamma, c["norm"]),
            "loss_fake_netD": float(np.mean(fake_terms_f64(f, c["which"]))),
            "loss_fake_netG": -float(np.mean(f)), "avg_fake": float(np.mean(f)),
            "event_t_rae": _mean(np.abs(t[evt] - p[evt]) / c["end_time"]),
            "nonevent_t_rae": _mean(np.maximum(t[non] - p[non], 0.0) / c["end_time"]),
            "event_t_nre": _mean((p[evt] - t[evt]) / c["end_time"]),
            "nonevent_t_nre": _mean(-np.maximum(t[non] - p[non], 0.0) / c["end_time"]),
            "mae": recon_f64(p, t, e, 0.0, 1.0, "l1")}


def mle_f64(hz, t, e, alpha, eps=1e-7):
    hz = hz.astype(np.float64)
    n = hz.shape[0]
    S = np.concatenate([np.ones((n, 1)), np.cumprod(1.0 - hz, axis=1)], axis=1)
    k = t.astype(np.int64)
    rows = np.arange(n)
    c = 1.0 - e
    unc = -(1.0 - c) * (np.log(np.maximum(S[rows, k], eps)) + np.log(np.maximum(hz[rows, k], eps)))
    cen = -c * np.log(np.maximum(S[rows, k + 1], eps))
    return float(np.mean((1.0 - alpha) * (cen + unc) + alpha * unc))


def want_disc(y, hz, fake, c):
    f = fake.astype(np.float64).reshape(-1)
    t, e = y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)
    return {"loss_mle": mle_f64(hz, t, e, c["alpha"]), "loss_mle_org": mle_f64(hz, t, e, 0.0),
            "loss_fake_netD": float(np.mean(fake_terms_f64(f, c["which"]))), "loss_fake_netG": -float(np.mean(f)),
            "avg_fake": float(np.mean(f))}


def ple_f64(theta, t, e):
    th = np.minimum(theta.astype(np.float64).reshape(-1), 10.0)
    R = (t.reshape(1, -1) >= t.reshape(-1, 1)).astype(np.float64)
    return -float(np.mean((th - np.log((np.exp(th)[None, :] * R).sum(axis=1))) * e.astype(np.float64)))


# ---- 1. fixture vs restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(G.CONT_CASES)))
def test_restatement_reproduces_the_reference_continuous(k):
    y, pred, fake = G.cont_inputs(k)
    for c, gold in zip(G.CONT_CONFIGS, GOLD["continuous"][k]):
        want = want_cont(y, pred, fake, c)
        assert set(gold) == set(want) | {"c_index"}
        for m, v in want.items():
            assert close(v, gold[m]), (k, c, m, v, gold[m])
        if isinstance(gold["c_index"], dict):
            assert gold["c_index"] == {"raises": "ValueError"} and not y[:, 1].any()
            with pytest.raises(ValueError):
                CO.concordance_index(y, pred)
        else:
            assert abs(CO.concordance_index(y, pred) - gold["c_index"]) < 1e-12
    evt = y[:, 1] == 1
    g0 = GOLD["continuous"][k][0]
    assert math.isnan(g0["event_t_rae"]) == (not evt.any()) and math.isnan(g0["nonevent_t_nre"]) == bool(evt.all())


@pytest.mark.parametrize("k", range(len(G.CONT_CASES)))
def test_restatement_reproduces_the_reference_rank_loss_and_gradient(k):
    y, pred, _ = G.cont_inputs(k)
    for (norm, aw), gold in zip(G.RANK_CONFIGS, GOLD["rank_loss"][k]):
        loss, grad, margin = rank_loss_f64(pred, y[:, 0], y[:, 1], G.GAMMA, norm, aw)
        assert margin >= 1e-6, (k, margin)             # no hinge sits where fp32 and float64 could take different branches
        g_ref = G.unpack_f32(gold["grad_f32_b64"]).astype(np.float64)
        assert g_ref.shape == grad.shape
        assert close(loss, gold["loss"]), (k, norm, aw, loss, gold["loss"])
        assert np.abs(grad - g_ref).max() <= TOL * np.abs(g_ref).max(), (k, norm, aw, np.abs(grad - g_ref).max(), np.abs(g_ref).max())
    # the reference answers shape [1] exactly when there is no pair (n = 64 without an event)
    assert [r["shape"] for r in GOLD["rank_loss"][k]] == [[1] if not y[:, 1].any() else []] * 4


@pytest.mark.parametrize("k", range(len(G.DISC_CASES)))
def test_restatement_reproduces_the_reference_discrete(k):
    y, hz, fake = G.disc_inputs(k)
    gold = GOLD["discrete"][k]
    for m, v in want_disc(y, hz, fake, G.DISC_CASES[k]).items():
        assert close(v, gold[m]), (k, m, v, gold[m])
    assert abs(CO.concordance_index(y, hz) - gold["c_index"]) < 1e-12
    assert y[:, 0].min() >= 0 and y[:, 0].max() == G.DISC_CASES[k]["bins"] - 1


@pytest.mark.parametrize("k", range(len(G.DISC2_CASES)))
def test_restatement_reproduces_the_reference_discrete_with_quantised_hazards(k):
    y, hz, fake = G.disc2_inputs(k)
    c, gold = G.DISC2_CASES[k], GOLD2["discrete"][k]
    assert set(gold) == set(want_disc(y, hz, fake, c)) | {"c_index"}
    for m, v in want_disc(y, hz, fake, c).items():
        assert close(v, gold[m]), (k, m, v, gold[m])
    assert abs(CO.concordance_index(y, hz) - gold["c_index"]) < 1e-12
    assert hz.shape == (300, c["bins"]) and y[:, 0].min() >= 0 and y[:, 0].max() <= c["bins"] - 1
    if c["levels"] is not None:
        assert set(np.unique(hz).tolist()) == {float(np.float32(v)) for v in c["levels"]}


def test_quantised_fixture_is_sensitive_to_a_fused_left_to_right_risk():
    """The precondition gen_golden_evaluator.main() asserts against the reference, restated on the oracle: in at least four of the six
    cases the c-index moves when numpy's risk is replaced by a left-to-right sum with one fused multiply-add per bin."""
    moved = 0
    for k in range(len(G.DISC2_CASES)):
        y, hz, _ = G.disc2_inputs(k)
        fused = CO.cindex_counts(y[:, 1].astype(bool), y[:, 0], -G.fused_left_to_right_risk(hz))[0]
        moved += int(abs(fused - GOLD2["discrete"][k]["c_index"]) >= 1e-12)
    assert moved >= G.DISC2_MIN_SENSITIVE, moved


@pytest.mark.parametrize("k", range(len(G.COX_CASES)))
def test_restatement_reproduces_the_reference_cox(k):
    y, theta = G.cox_inputs(k)
    gold = GOLD["cox"][k]
    assert close(ple_f64(theta, y[:, 0], y[:, 1]), gold["loss_ple"])
    assert abs(CO.concordance_index(y, theta) - gold["c_index"]) < 1e-12
    if k == 0:
        assert float(theta.max()) > 10.0 and len(np.unique(y[:, 0])) == len(y)


# ---- 1b. the fixed-seed leg of tools/probe/surv_fuzz.py, replayed without a device -------------------------------------------------
def test_surv_fuzz_fixed_seed_leg_draws_every_kind_and_leaves_out_few():
    """The draws of `surv_fuzz.py 12 110` (tests/test_fuzz_gpu.py): every family meets each of its kinds, the cohorts span what the
    probe promises, and the share of rank_loss draws left out for a hinge within 1e-6 of its kink stays under the probe's cap."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert '("surv_fuzz.py", ("12", "110"))' in open(os.path.join(root, "tests", "test_fuzz_gpu.py")).read()
    spec = importlib.util.spec_from_file_location("surv_fuzz", os.path.join(root, "tools", "probe", "surv_fuzz.py"))
    F = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(F)
    cases = F.draws(12, 110)
    assert list(cases) == list(F.FAMILIES) and all(len(v) == 12 for v in cases.values())
    again = F.draws(12, 110)
    for fam in F.FAMILIES:
        assert {d["kind"] for d in cases[fam]} == set(F.KINDS[fam]), fam
        assert all(1 <= d["n"] <= 1500 for d in cases[fam])
        for a, b in zip(cases[fam], again[fam]):                   # the same draws on every machine
            assert all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)
    every = [d for v in cases.values() for d in v]
    assert {0.0, 1.0} <= {d["event_share"] for d in every} and {0, 3, 50} == {d["time_levels"] for d in every}
    assert {0, 40} == {d["est_levels"] for d in cases["cont"]} and any(d["fake"] is None for d in cases["cont"])
    assert {0.0, 0.3, 1.0} == {d["alpha"] for d in cases["cont"]} == {d["alpha"] for d in cases["disc"]}
    assert min(d["bins"] for d in cases["disc"]) < 8 and max(d["bins"] for d in cases["disc"]) > 128 and {0, 3} == {d["pad"] for d in cases["disc"]}
    assert all(float(d["theta"].min()) >= -12.0 and float(d["theta"].max()) <= 14.0 for d in cases["ple"])
    assert any(float(d["theta"].max()) > 10.0 for d in cases["ple"])
    ranks = cases["rank_fwd"] + cases["rank_bwd"]
    assert {"fine", "sixtyfourths", "fortieths"} == {d["grid"] for d in ranks} and {1.0, 16.0} == {d["scale"] for d in ranks}
    margins = [F.want_rank(d)[2] for d in ranks]
    skipped = sum(F.left_out(d, m) for d, m in zip(ranks, margins))
    assert skipped <= F.MAX_SKIPPED * len(ranks), (skipped, len(ranks))
    assert sum(math.isfinite(m) for m in margins) >= len(ranks) // 2          # most draws do hold pairs
    # the float64 sides answer on every draw
    for d in cases["cont"]:
        assert all(v is None or math.isfinite(v) for v in F.want_cont(d)[0])
    for d in cases["disc"]:
        want, risk = F.want_disc(d)
        assert all(math.isfinite(v) for v in want) and risk.dtype == np.float32 and risk.shape == (d["n"],)
    assert all(math.isfinite(F.want_ple(d)) for d in cases["ple"])


# ---- 2. public surface ----------------------------------------------------------------------------------------------------------
def test_names_valid_metrics_and_prepare_evaluator():
    from advmil_amd.eval import ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator, prepare_evaluator
    from advmil_amd.eval.utils import prepare_evaluator as pe2
    assert pe2 is prepare_evaluator
    c, d, x = prepare_evaluator("continuous", end_time=1.0), prepare_evaluator("discrete"), prepare_evaluator("prohazard")
    assert type(c) is ContSurv_Evaluator and type(d) is DiscSurv_Evaluator and type(x) is CoxSurv_Evaluator
    assert prepare_evaluator("something else", end_time=1.0) is None
    assert c.valid_metrics == GOLD["valid_metrics"]["continuous"]
    assert d.valid_metrics == GOLD["valid_metrics"]["discrete"]
    assert x.valid_metrics == GOLD["valid_metrics"]["cox"]
    assert GOLD["unknown_metric"] == "AssertionError"
    y, pred, _ = G.cont_inputs(1)
    for ev in (c, d, x):
        with pytest.raises(AssertionError):
            ev.compute({"y": torch.from_numpy(y), "y_hat": torch.from_numpy(pred)}, ["no_such_metric"])
    with pytest.raises(KeyError):
        ContSurv_Evaluator()                                       # end_time is required, as in the reference


def test_rank_loss_is_listed_and_refuses_unknown_norms():
    from advmil_amd.loss import utils as LU
    assert "rank_loss" in LU.__doc__
    with pytest.raises(NotImplementedError):
        LU.rank_loss(torch.zeros(3), torch.zeros(3), torch.zeros(3), norm="l3")


# ---- 3. no device ---------------------------------------------------------------------------------------------------------------
def test_without_a_device_compute_and_rank_loss_refuse(monkeypatch):
    from advmil_amd.eval import prepare_evaluator
    from advmil_amd.loss import utils as LU
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    y, pred, fake = (torch.from_numpy(a) for a in G.cont_inputs(1))
    ev = prepare_evaluator("continuous", end_time=1.0, recon_loss=functools.partial(LU.recon_loss, gamma=G.GAMMA))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.compute({"y": y, "y_hat": pred, "f_fake": fake}, ["mae"])
    yd, hz, _ = (torch.from_numpy(a) for a in G.disc_inputs(0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prepare_evaluator("discrete", mle_loss=LU.SurvMLE()).compute({"y": yd, "y_hat": hz}, ["loss_mle"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prepare_evaluator("prohazard", ple_loss=LU.SurvPLE()).compute({"y": y, "y_hat": pred}, ["loss_ple"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LU.rank_loss(pred, y[:, 0], y[:, 1], gamma=G.GAMMA)


# ---- 4. workspace queries -------------------------------------------------------------------------------------------------------
def test_workspace_queries_are_positive_and_monotone():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    L = _lib.lib()
    sizes = [1, 2, 255, 256, 257, 1000, 60000, 262144, 262145, 10 ** 7, 2 ** 31 - 1]
    for name in ("advmil_surv_metrics_cont_workspace_bytes", "advmil_surv_metrics_disc_workspace_bytes",
                 "advmil_ple_loss_workspace_bytes", "advmil_rank_loss_workspace_bytes"):
        got = [getattr(L, name)(n) for n in sizes]
        assert all(v > 0 for v in got), (name, got)
        assert all(a <= b for a, b in zip(got, got[1:])), (name, got)
        assert getattr(L, name)(0) == 0
    assert L.advmil_rank_loss_workspace_bytes(1000) == 4 * 8 * 1000 and L.advmil_ple_loss_workspace_bytes(1000) == 2 * 8 * 1000
    # a workspace one byte short is refused before anything is enqueued
    import ctypes
    p = lambda k: ctypes.c_void_p(0x7F0000001000 + (k << 20))   # noqa: E731
    assert L.advmil_rank_loss_fwd(p(0), p(1), p(2), 1000, 0.1, 0, 0, p(3), p(4), p(5), 4 * 8 * 1000 - 1, None) == -2
    assert L.advmil_ple_loss(p(0), p(1), p(2), 1000, p(3), p(4), 2 * 8 * 1000 - 1, None) == -2
    assert L.advmil_surv_metrics_disc(p(0), 4, p(1), p(2), None, 100, 257, 0.0, 1e-7, 0, p(3), p(4), p(5), 1 << 20, None) == -1    # bins > 256
    assert L.advmil_surv_metrics_disc(p(0), 3, p(1), p(2), None, 100, 4, 0.0, 1e-7, 0, p(3), p(4), p(5), 1 << 20, None) == -1      # pitch < bins
    assert L.advmil_surv_metrics_cont(p(0), p(1), p(2), None, 100, 0.0, 1.0, 0, 1.0, 3, p(3), p(4), 1 << 20, None) == -1           # unknown loss kind
