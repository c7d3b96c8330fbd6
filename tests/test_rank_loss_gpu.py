"""GPU: advmil_amd.loss.utils.rank_loss (advmil_rank_loss_fwd / _bwd, csrc/survk.hip) against the reference's loss and fp32 pred.grad
(tests/golden/evaluator_v1.json) and against float64 autograd of the restated formula (tests/test_evaluator_cpu.py::rank_loss_f64).
Bounds: loss within 2e-5 relative, max|g - g_ref| <= 2e-5 * max|g_ref| (this suite's parity tolerance)."""
import numpy as np
import pytest
import torch

from tests.golden import gen_golden_evaluator as G
from tests.poison import assert_same_bits, three_runs
from tests.test_evaluator_cpu import GOLD, TOL, rank_loss_f64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def run(pred, t, e, gamma, norm, aw, gout=None):
    """-> (loss tensor, pred.grad as float64 numpy) of the HIP path."""
    from advmil_amd.loss.utils import rank_loss
    p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).to(DEV).requires_grad_(True)
    tt = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(DEV).requires_grad_(True)
    ee = torch.from_numpy(np.ascontiguousarray(e, dtype=np.float32)).to(DEV).requires_grad_(True)
    loss = rank_loss(p, tt, ee, gamma=gamma, norm=norm, add_weight=aw)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    if gout is None:
        loss.backward()
    else:
        (loss * gout).backward()
    assert tt.grad is None and ee.grad is None                  # differentiable in pred_t only
    assert p.grad.shape == p.shape
    return loss.detach(), p.grad.detach().cpu().double().numpy().reshape(-1)


def check(got_loss, got_grad, want_loss, want_grad, what):
    gmax = float(np.abs(want_grad).max())
    dl, dg = abs(float(got_loss) - want_loss), float(np.abs(got_grad - want_grad).max())
    print(f"  {what}: loss {float(got_loss)!r} want {want_loss!r} (diff {dl:.2e}); grad diff {dg:.2e} of max {gmax:.2e}")
    assert dl <= TOL * abs(want_loss), (what, float(got_loss), want_loss)
    assert dg <= TOL * gmax, (what, dg, gmax)


@pytest.mark.parametrize("k", range(len(G.CONT_CASES)))
def test_loss_and_gradient_equal_the_reference(k):
    y, pred, _ = G.cont_inputs(k)
    for (norm, aw), gold in zip(G.RANK_CONFIGS, GOLD["rank_loss"][k]):
        # precondition: in float64 no comparable pair has |gamma + x| < 1e-6 (an l1 hinge there could flip between fp32 and float64)
        assert rank_loss_f64(pred, y[:, 0], y[:, 1], G.GAMMA, norm, aw)[2] >= 1e-6
        loss, grad = run(pred, y[:, 0], y[:, 1], G.GAMMA, norm, aw)
        check(loss, grad, gold["loss"], G.unpack_f32(gold["grad_f32_b64"]).astype(np.float64), (k, norm, aw))


def test_n3000_l2_against_float64_autograd():
    rs = np.random.RandomState(11)
    n = 3000
    t = (np.floor(rs.rand(n) * 400) / 400).astype(np.float32)               # ties in the times
    e = (rs.rand(n) < 0.45).astype(np.float32)
    pred = rs.rand(n).astype(np.float32)
    for aw in (False, True):
        want_loss, want_grad, _ = rank_loss_f64(pred, t, e, G.GAMMA, "l2", aw)
        loss, grad = run(pred, t, e, G.GAMMA, "l2", aw)
        check(loss, grad, want_loss, want_grad, ("n3000", aw))


def test_no_comparable_pair_gives_zero_loss_and_gradient():
    for t, e in (([0.3, 0.7, 0.1, 0.9], [0, 0, 0, 0]), ([0.5, 0.5], [1, 1])):
        for norm, aw in G.RANK_CONFIGS:
            loss, grad = run(np.linspace(0.1, 0.9, len(t)), t, e, G.GAMMA, norm, aw)
            assert loss.shape == () and float(loss) == 0.0 and not grad.any() and np.isfinite(grad).all()
    # ... and the same from the fixture's case without an event
    y, pred, _ = G.cont_inputs(7)
    loss, grad = run(pred, y[:, 0], y[:, 1], G.GAMMA, "l1", True)
    assert float(loss) == 0.0 and not grad.any()


def test_incoming_gradient_scales_and_unknown_norm_raises():
    from advmil_amd.loss.utils import rank_loss
    y, pred, _ = G.cont_inputs(1)
    for norm, aw in G.RANK_CONFIGS:
        l1, g1 = run(pred, y[:, 0], y[:, 1], G.GAMMA, norm, aw)
        l2, g2 = run(pred, y[:, 0], y[:, 1], G.GAMMA, norm, aw, gout=-2.5)
        assert float(l1) == float(l2) and np.abs(g1).max() > 0
        assert np.abs(g2 - (-2.5) * g1).max() <= 1e-6 * np.abs(g1).max()
    with pytest.raises(NotImplementedError):
        rank_loss(torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), norm="l3")
    # [n, 1] columns, as the handlers hold them, are squeezed as the reference does
    p = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    la = rank_loss(p, torch.from_numpy(y[:, :1].copy()).to(DEV), torch.from_numpy(y[:, 1:].copy()).to(DEV), gamma=G.GAMMA)
    la.backward()
    assert p.grad.shape == p.shape and float(la.detach()) == float(run(pred, y[:, 0], y[:, 1], G.GAMMA, "l1", False)[0])


def test_loss_and_gradient_do_not_move_with_what_the_buffers_held():
    y, pred, _ = G.cont_inputs(4)                                            # n = 257
    for norm, aw in G.RANK_CONFIGS:
        def once():
            loss, grad = run(pred, y[:, 0], y[:, 1], G.GAMMA, norm, aw)
            return {"loss": loss, "grad": torch.from_numpy(grad)}
        assert_same_bits(three_runs(once))
