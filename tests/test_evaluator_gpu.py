"""GPU: ContSurv_Evaluator / DiscSurv_Evaluator / CoxSurv_Evaluator on the HIP path (csrc/survk.hip) against the reference's values
(tests/golden/evaluator_v1.json) at 2e-5 * max(1, |want|) -- this suite's parity tolerance; the reference's own fp32 results lie
within 2.3e-6 of float64, which leaves ~9x for the kernels' ~1-ulp transcendentals --, c_index at 1e-12 as in tests/test_cindex.py."""
import builtins
import functools
import math

import pytest
import torch

from tests.golden import gen_golden_evaluator as G
from tests.poison import assert_same_bits, three_runs
from tests.test_evaluator_cpu import GOLD, GOLD2, TOL, close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T = torch.from_numpy


def cont_kws(c, generic=False):
    from advmil_amd.loss import utils as LU
    recon = functools.partial(LU.recon_loss, alpha=c["alpha"], gamma=G.GAMMA, norm=c["norm"])
    rank = functools.partial(LU.rank_loss, gamma=G.GAMMA, norm=c["norm"], add_weight=c["add_weight"])
    disc = functools.partial(LU.real_fake_loss, which=c["which"])
    if generic:                      # plain lambdas are not recognised: every loss is called on the device tensors and .item()-ed
        return dict(end_time=c["end_time"], recon_loss=lambda *a, **k: recon(*a, **k), rank_loss=lambda *a, **k: rank(*a, **k),
                    disc_loss=lambda *a, **k: disc(*a, **k))
    return dict(end_time=c["end_time"], recon_loss=recon, rank_loss=rank, disc_loss=disc)


def disc_kws(c, generic=False):
    from advmil_amd.loss import utils as LU
    mle, disc = LU.SurvMLE(alpha=c["alpha"]), functools.partial(LU.real_fake_loss, which=c["which"])
    if generic:
        return dict(mle_loss=lambda *a, **k: mle(*a, **k), disc_loss=lambda *a, **k: disc(*a, **k))
    return dict(mle_loss=mle, disc_loss=disc)


def check_against(ev, data, gold):
    """Every metric of the fixture entry: the values in one compute(), each recorded exception on its own."""
    values = [m for m in ev.valid_metrics if not isinstance(gold[m], dict)]
    got = ev.compute(data, values)
    assert list(got) == values
    for m in values:
        assert isinstance(got[m], (float, int)) and not isinstance(got[m], bool), (m, type(got[m]))
        print(f"  {m}: got {got[m]!r} want {gold[m]!r}")
        assert close(float(got[m]), gold[m], 1e-12 if m == "c_index" else TOL), (m, got[m], gold[m])
    for m in ev.valid_metrics:
        if isinstance(gold[m], dict):
            with pytest.raises(Exception) as info:
                ev.compute(data, [m])
            assert gold[m]["raises"] in [k.__name__ for k in type(info.value).__mro__], (m, type(info.value), gold[m])


@pytest.mark.parametrize("k", range(len(G.CONT_CASES)))
def test_continuous_golden_cases(k):
    from advmil_amd.eval import prepare_evaluator
    y, pred, fake = G.cont_inputs(k)
    data = {"y": T(y), "y_hat": T(pred), "f_fake": T(fake)}
    for c, gold in zip(G.CONT_CONFIGS, GOLD["continuous"][k]):
        check_against(prepare_evaluator("continuous", **cont_kws(c)), data, gold)


@pytest.mark.parametrize("k", range(len(G.DISC_CASES)))
def test_discrete_golden_cases(k):
    from advmil_amd.eval import prepare_evaluator
    y, hz, fake = G.disc_inputs(k)
    check_against(prepare_evaluator("discrete", **disc_kws(G.DISC_CASES[k])), {"y": T(y), "y_hat": T(hz), "f_fake": T(fake)}, GOLD["discrete"][k])


@pytest.mark.parametrize("k", range(len(G.DISC2_CASES)))
def test_discrete_golden_cases_with_quantised_hazards(k):
    """tests/golden/evaluator_v2.json: rows that hold the same few hazard levels in another order. The c-index at 1e-12 needs the
    kernel's risk to be the reference's float32 number bit for bit (numpy's pairwise order, no contraction)."""
    from advmil_amd.eval import prepare_evaluator
    y, hz, fake = G.disc2_inputs(k)
    check_against(prepare_evaluator("discrete", **disc_kws(G.DISC2_CASES[k])), {"y": T(y), "y_hat": T(hz), "f_fake": T(fake)}, GOLD2["discrete"][k])


@pytest.mark.parametrize("k", range(len(G.COX_CASES)))
def test_cox_golden_cases(k):
    from advmil_amd.eval import prepare_evaluator
    from advmil_amd.loss.utils import SurvPLE
    y, theta = G.cox_inputs(k)
    check_against(prepare_evaluator("prohazard", ple_loss=SurvPLE()), {"y": T(y), "y_hat": T(theta)}, GOLD["cox"][k])


def test_recorded_failure_and_absence_behaviour():
    from advmil_amd.eval import ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator
    from advmil_amd.loss import utils as LU
    y, pred, fake = G.cont_inputs(1)
    # no callable at all (and None): the loss metrics are 0, the rest as recorded
    for kws in (dict(end_time=1.0), dict(end_time=1.0, recon_loss=None, rank_loss=None, disc_loss=None)):
        check_against(ContSurv_Evaluator(**kws), {"y": T(y), "y_hat": T(pred), "f_fake": T(fake)}, GOLD["no_callables"])
    # a collector without f_fake: the reference fails with TypeError / AttributeError on None
    ev = ContSurv_Evaluator(end_time=1.0, disc_loss=functools.partial(LU.real_fake_loss, which="bce"))
    for m, rec in GOLD["no_f_fake"].items():
        with pytest.raises(TypeError):
            ev.compute({"y": T(y), "y_hat": T(pred)}, [m])
        with pytest.raises(getattr(builtins, rec["raises"])):
            ev.compute({"y": T(y), "y_hat": T(pred)}, [m])
    assert ev.compute({"y": T(y), "y_hat": T(pred)}, ["mae", "c_index"])["mae"] > 0          # the other metrics need no f_fake
    yd, hz, fd = G.disc_inputs(0)
    assert GOLD["disc_without_mle_loss"] == {"raises": "AssertionError"}
    with pytest.raises(AssertionError):
        DiscSurv_Evaluator().compute({"y": T(yd), "y_hat": T(hz), "f_fake": T(fd)}, ["loss_mle"])
    yc, theta = G.cox_inputs(1)
    check_against(CoxSurv_Evaluator(), {"y": T(yc), "y_hat": T(theta)}, GOLD["cox_no_callables"])
    # avg_y_hat is preferred when the collector has one
    a = ContSurv_Evaluator(end_time=1.0).compute({"y": T(y), "y_hat": T(pred) + 5.0, "avg_y_hat": T(pred)}, ["mae", "c_index"])
    assert close(a["mae"], GOLD["no_callables"]["mae"]) and close(a["c_index"], GOLD["no_callables"]["c_index"], 1e-12)


def _same_within(a, b):
    assert list(a) == list(b)
    for m in a:
        assert close(float(a[m]), float(b[m])), (m, a[m], b[m])


def test_fused_route_equals_generic_route():
    from advmil_amd.eval import prepare_evaluator
    from advmil_amd.loss.utils import SurvPLE
    y, pred, fake = G.cont_inputs(4)
    data = {"y": T(y), "y_hat": T(pred), "f_fake": T(fake)}
    for c in G.CONT_CONFIGS:
        fused, generic = prepare_evaluator("continuous", **cont_kws(c)), prepare_evaluator("continuous", **cont_kws(c, generic=True))
        _same_within(fused.compute(data, fused.valid_metrics), generic.compute(data, generic.valid_metrics))
    yd, hz, fd = G.disc_inputs(0)
    data = {"y": T(yd), "y_hat": T(hz), "f_fake": T(fd)}
    fused, generic = prepare_evaluator("discrete", **disc_kws(G.DISC_CASES[0])), prepare_evaluator("discrete", **disc_kws(G.DISC_CASES[0], True))
    _same_within(fused.compute(data, fused.valid_metrics), generic.compute(data, generic.valid_metrics))
    yc, theta = G.cox_inputs(1)
    data = {"y": T(yc), "y_hat": T(theta)}
    ple = SurvPLE()
    _same_within(prepare_evaluator("prohazard", ple_loss=ple).compute(data, ["c_index", "loss_ple"]),
                 prepare_evaluator("prohazard", ple_loss=lambda *a: ple(*a)).compute(data, ["c_index", "loss_ple"]))


def test_host_and_device_collectors_give_identical_floats():
    from advmil_amd.eval import prepare_evaluator
    from advmil_amd.loss.utils import SurvPLE
    y, pred, fake = G.cont_inputs(3)
    ev = prepare_evaluator("continuous", **cont_kws(G.CONT_CONFIGS[1]))
    host = {"y": T(y), "y_hat": T(pred), "f_fake": T(fake)}
    assert ev.compute(host, ev.valid_metrics) == ev.compute({k: v.to(DEV) for k, v in host.items()}, ev.valid_metrics)
    yd, hz, fd = G.disc_inputs(2)
    ev = prepare_evaluator("discrete", **disc_kws(G.DISC_CASES[2]))
    host = {"y": T(yd), "y_hat": T(hz), "f_fake": T(fd)}
    assert ev.compute(host, ev.valid_metrics) == ev.compute({k: v.to(DEV) for k, v in host.items()}, ev.valid_metrics)
    yc, theta = G.cox_inputs(0)
    ev = prepare_evaluator("prohazard", ple_loss=SurvPLE())
    host = {"y": T(yc), "y_hat": T(theta)}
    assert ev.compute(host, ev.valid_metrics) == ev.compute({k: v.to(DEV) for k, v in host.items()}, ev.valid_metrics)


def test_out_of_range_bin_index_raises_and_leaves_the_next_call_intact():
    from advmil_amd.eval import prepare_evaluator
    y, hz, fake = G.disc_inputs(0)
    ev = prepare_evaluator("discrete", **disc_kws(G.DISC_CASES[0]))
    for bad in (4.0, -1.0, 1e9, float("nan")):
        yb = y.copy()
        yb[7, 0] = bad
        with pytest.raises(ValueError, match="bin index"):
            ev.compute({"y": T(yb), "y_hat": T(hz), "f_fake": T(fake)}, ["loss_mle"])
    check_against(ev, {"y": T(y), "y_hat": T(hz), "f_fake": T(fake)}, GOLD["discrete"][0])


def test_results_do_not_move_with_what_the_buffers_held():
    from advmil_amd.eval import prepare_evaluator
    from advmil_amd.loss.utils import SurvPLE
    y, pred, fake = G.cont_inputs(4)                                                          # n = 257
    for c in G.CONT_CONFIGS[:2]:
        ev = prepare_evaluator("continuous", **cont_kws(c))
        data = {"y": T(y).to(DEV), "y_hat": T(pred).to(DEV), "f_fake": T(fake).to(DEV)}
        runs = three_runs(lambda: ev.compute(data, ev.valid_metrics))
        assert not any(math.isnan(v) for v in runs[0].values())
        assert_same_bits(runs)
    yd, hz, fd = G.disc_inputs(0)                                                             # 150 x 4
    ev = prepare_evaluator("discrete", **disc_kws(G.DISC_CASES[0]))
    data = {"y": T(yd), "y_hat": T(hz), "f_fake": T(fd)}
    assert_same_bits(three_runs(lambda: ev.compute(data, ev.valid_metrics)))
    yc, theta = G.cox_inputs(1)                                                               # n = 257
    ev = prepare_evaluator("prohazard", ple_loss=SurvPLE())
    data = {"y": T(yc), "y_hat": T(theta)}
    assert_same_bits(three_runs(lambda: ev.compute(data, ev.valid_metrics)))


def test_test_model_collector_evaluates_through_prepare_evaluator():
    """The collector of a tiny ABMIL handler (7 bags, both event kinds) -> finite metrics, equal to the generic route's."""
    from advmil_amd.eval import prepare_evaluator
    from advmil_amd.model import MyHandler
    from tests.test_eval_batched_gpu import make, nets
    g, d = nets("abmil")
    items = make("abmil", (256, 128, 512, 64, 192, 384, 320))
    col = MyHandler.test_model(g, d, "abmil", items, test_zero_noise=True, batch_bags=3)
    e = col["y"][:, 1]
    assert col["y"].shape == (7, 2) and bool((e == 1).any()) and bool((e == 0).any())
    c = G.CONT_CONFIGS[0]
    fused, generic = prepare_evaluator("continuous", **cont_kws(c)), prepare_evaluator("continuous", **cont_kws(c, generic=True))
    got = fused.compute(col, fused.valid_metrics)
    assert all(math.isfinite(v) for v in got.values()), got
    _same_within(got, generic.compute(col, generic.valid_metrics))


def test_full_size_perfect_order_has_no_rank_loss():
    """n = 60 000 (1.8e9 candidate pairs): a prediction in the order of the times gives loss_rank == 0 for gamma = 0."""
    from advmil_amd.eval import ContSurv_Evaluator
    from advmil_amd.loss import utils as LU
    n = 60000
    g = torch.Generator().manual_seed(0)
    tm = torch.randperm(n, generator=g).to(torch.float32) / n
    ev = (torch.rand(n, generator=g) < 0.5).to(torch.float32)
    data = {"y": torch.stack([tm, ev], dim=1), "y_hat": tm.reshape(-1, 1).clone()}
    for aw in (False, True):
        e = ContSurv_Evaluator(end_time=1.0, rank_loss=functools.partial(LU.rank_loss, gamma=0.0, norm="l1", add_weight=aw))
        got = e.compute(data, ["loss_rank", "c_index", "mae"])
        assert got["loss_rank"] == 0.0 and got["c_index"] == 1.0 and got["mae"] > 0
