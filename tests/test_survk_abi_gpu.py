"""GPU: the C-ABI entries of csrc/survk.hip at their edges, called directly (tests/survk_abi.py), against the float64 restatements of
tests/test_evaluator_cpu.py (which the CPU suite pins to the reference). Every test runs once per poison pattern, so workspace, out16,
risk and state4 start as NaN / 3.39e38.

Tolerance: this suite's TOL = 2e-5 * max(1, |want|), on the quantity the Python layer reports -- a slot that is a sum is divided by
the count the Python layer divides it by (n, #events, #censored) before it is compared; the counts themselves and every value the
formulas make exact (zeros, integer counts, single fp32 operations) are compared with ==.

The discrete risk is compared with numpy's float32 expression BIT FOR BIT: -risk feeds the concordance index, whose tie rule (1e-8)
turns a last-bit difference into moved pairs (docs/DESIGN_HISTORY.md, "risk in the reference's bits")."""
import numpy as np
import pytest
import torch

from tests import survk_abi as K
from tests.poison import poison  # noqa: F401  (fixture: both poison patterns)
from tests.test_evaluator_cpu import TOL, close, fake_terms_f64, mle_f64, ple_f64, rank_loss_f64

pytestmark = pytest.mark.gpu
WHICH = ("bce", "hinge", "wasserstein")


# ---- 1. the discrete risk in the reference's bits ---------------------------------------------------------------------------------
RISK_BINS = (1, 2, 4, 5, 7, 8, 9, 20, 64, 127, 128, 129, 200, 256)
RISK_DRAWS = ("levels_123", "levels_19", "continuous")


def test_discrete_risk_equals_numpy_float32_bit_for_bit(poison):  # noqa: F811
    n = 300
    rs = np.random.RandomState(20)
    bad = []
    for bins in RISK_BINS:
        t = np.floor(rs.rand(n) * bins).astype(np.float32)
        e = (rs.rand(n) < 0.5).astype(np.float32)
        for kind in RISK_DRAWS:
            hz = K.hazard_draw(rs, kind, n, bins)
            want = K.numpy_risk(hz).view(np.int32)
            for pad in (0, 3):
                out, risk = K.metrics_disc(hz, t, e, None, 0.0, 1e-7, "bce", pad=pad)
                diff = int((risk.view(np.int32) != want).sum())
                print(f"  bins {bins:3d} {kind:10s} ld = bins + {pad}: {diff} of {n} rows differ")
                if diff:
                    bad.append((bins, kind, pad, diff))
                assert out[4] == 0 and np.isfinite(out[:5]).all(), (bins, kind, pad, out[:5])       # the NaN padding is not read
    assert not bad, bad


# ---- 2. advmil_surv_metrics_cont ----------------------------------------------------------------------------------------------------
def cont_cohort(seed, n, p_event=0.5, fake_scale=2.0):
    rs = np.random.RandomState(seed)
    t, pred = rs.rand(n).astype(np.float32), rs.rand(n).astype(np.float32)
    e = (rs.rand(n) < p_event).astype(np.float32)
    fake = (fake_scale * (2.0 * rs.rand(n) - 1.0)).astype(np.float32)
    return t, e, pred, fake


def check_cont(t, e, pred, fake, alpha, gamma, norm, end_time, which, what):
    out = K.metrics_cont(t, e, pred, fake, alpha, gamma, norm, end_time, which)
    want, n_evt, n_non = K.want_cont_slots(t, e, pred, fake, alpha, gamma, norm, end_time, which)
    n = len(t)
    assert out[9] == n_evt and out[10] == n_non, (what, out[9], n_evt, out[10], n_non)
    assert not out[11:].any(), (what, out[11:])
    div = [n, n, n, n, n, n_evt, n_non, n_evt, n_non]
    for q in range(9):
        if want[q] is None:                                          # an empty selection: the sum over it is exactly 0
            assert out[q] == 0.0, (what, q, out[q])
            continue
        got = out[q] / div[q]
        assert close(float(got), want[q]), (what, q, float(got), want[q])
    return out


CONT_N = (1, 255, 256, 257, 3840, 4096, 4097, 262144, 262401)       # 15 / 16 / 17 partial blocks, the grid cap, a second trip for 257 threads


@pytest.mark.parametrize("k", range(len(CONT_N)))
def test_cont_all_slots_at_the_block_and_grid_edges(poison, k):  # noqa: F811
    n = CONT_N[k]
    t, e, pred, fake = cont_cohort(300 + k, n)
    alpha, norm, which, end_time = (0.3, "l1", "bce", 1.0) if k % 3 == 0 else ((0.0, "l2", "hinge", 7.5) if k % 3 == 1 else (1.0, "l1", "wasserstein", 2.0))
    check_cont(t, e, pred, fake, alpha, 0.137, norm, end_time, which, ("n", n))


def test_cont_half_events_null_fake_no_event_all_events_l2_and_large_scores(poison):  # noqa: F811
    # e == 0.5 on a tenth of the rows: weight 0.5 in recon and mae, in none of the slots 5 to 10
    t, e, pred, fake = cont_cohort(320, 1000)
    e[::10] = 0.5
    out = check_cont(t, e, pred, fake, 0.3, 0.137, "l1", 1.0, "bce", "half events")
    assert out[9] + out[10] == 900
    # fake == NULL: slots 3 and 4 are exactly 0
    out = check_cont(t, e, pred, None, 0.3, 0.137, "l2", 1.0, "hinge", "no fake")
    assert out[3] == 0.0 and out[4] == 0.0
    # no event, all events (n = 257)
    for p_event in (0.0, 1.0):
        t, e, pred, fake = cont_cohort(321, 257, p_event=p_event)
        out = check_cont(t, e, pred, fake, 0.5, 0.137, "l1", 3.0, "wasserstein", ("p_event", p_event))
        assert (out[9], out[10]) == ((0.0, 257.0) if p_event == 0.0 else (257.0, 0.0))
    # l2 with gamma = 0.137, alpha = 1
    t, e, pred, fake = cont_cohort(322, 777)
    check_cont(t, e, pred, fake, 1.0, 0.137, "l2", 1.0, "bce", "l2 alpha 1")
    # f_fake = +-30 for the three loss kinds (sigmoid saturates: log(0 + 1e-8) on one side, log(1 + 1e-8) on the other)
    fake = np.where(np.arange(777) % 2 == 0, 30.0, -30.0).astype(np.float32)
    for which in WHICH:
        check_cont(t, e, pred, fake, 0.3, 0.137, "l1", 1.0, which, ("fake +-30", which))


# ---- 3. advmil_surv_metrics_disc ----------------------------------------------------------------------------------------------------
def check_disc(hz, t, e, fake, alpha, which, what, good=None):
    """Slots 0 to 3 against float64 (`good`: the rows with a valid bin index; None = all), -> (out16, risk)."""
    out, risk = K.metrics_disc(hz, t, e, fake, alpha, 1e-7, which)
    n = hz.shape[0]
    g = np.ones(n, dtype=bool) if good is None else good
    for q, a in ((0, alpha), (1, 0.0)):
        want = mle_f64(hz[g], t[g], e[g].astype(np.float64), a) * int(g.sum()) / n
        assert close(float(out[q] / n), want), (what, q, float(out[q] / n), want)
    f = fake.astype(np.float64)
    assert close(float(out[2] / n), float(np.mean(fake_terms_f64(f, which)))), (what, 2)
    assert close(float(out[3] / n), float(np.mean(f))), (what, 3)
    assert out[4] == n - int(g.sum()) and not out[5:].any(), (what, out[4:])
    return out, risk


def test_disc_bin_index_truncation_and_exact_zero_and_one_hazards(poison):  # noqa: F811
    rs = np.random.RandomState(330)
    n, bins = 300, 6
    hz = K.hazard_draw(rs, "continuous", n, bins)
    t = np.floor(rs.rand(n) * bins).astype(np.float32)
    e = (rs.rand(n) < 0.5).astype(np.float32)
    fake = (4.0 * rs.rand(n) - 2.0).astype(np.float32)
    t[0:40] = 2.9                                                   # .long() truncates toward zero: bin 2
    t[40:80] = -0.5                                                 # ... and bin 0
    assert (e[:80] == 0).any() and (e[:80] == 1).any()
    check_disc(hz, t, e, fake, 0.3, "bce", "fractional bin indices")
    # exact 0 and exact 1 hazards; rows whose bin lies after the 1 (S == 0 there: the eps clamps), censored and not
    hz[:, 1] = np.where(np.arange(n) % 3 == 0, 1.0, hz[:, 1]).astype(np.float32)
    hz[:, 0] = np.where(np.arange(n) % 5 == 0, 0.0, hz[:, 0]).astype(np.float32)
    t = np.floor(rs.rand(n) * bins).astype(np.float32)
    after = (np.arange(n) % 3 == 0) & (t >= 2)
    assert (after & (e == 0)).any() and (after & (e == 1)).any() and ((t == 0) & (hz[:, 0] == 0) & (e == 1)).any()
    check_disc(hz, t, e, fake, 0.5, "hinge", "exact 0 and 1 hazards")


def test_disc_bad_bin_indices_are_counted_and_leave_the_good_rows_alone(poison):  # noqa: F811
    rs = np.random.RandomState(331)
    n, bins = 700, 5
    hz = K.hazard_draw(rs, "continuous", n, bins)
    t = np.floor(rs.rand(n) * bins).astype(np.float32)
    e = (rs.rand(n) < 0.5).astype(np.float32)
    fake = (4.0 * rs.rand(n) - 2.0).astype(np.float32)
    rows = np.array([3, 255, 256, 511, 699])
    tb = t.copy()
    tb[rows] = np.array([bins, -1.0, 1e9, np.nan, np.inf], dtype=np.float32)
    good = np.ones(n, dtype=bool)
    good[rows] = False
    out_bad, _ = check_disc(hz, tb, e, fake, 0.3, "wasserstein", "bad rows", good=good)
    assert out_bad[4] == 5.0
    # the same launch with those five rows made valid AND worth exactly 0 (bin 0, an event, hazard 1: -(log 1 + log 1) = 0): every
    # partial sum meets the same addends in the same order, so slots 0 to 3 must not move by a bit
    h0, e0 = hz.copy(), e.copy()
    h0[rows, 0], e0[rows] = 1.0, 1.0
    t0 = t.copy()
    t0[rows] = 0.0
    out_ok, _ = K.metrics_disc(h0, t0, e0, fake, 0.3, 1e-7, "wasserstein")
    assert out_ok[4] == 0.0
    assert out_bad[:4].tobytes() == out_ok[:4].tobytes(), (out_bad[:4], out_ok[:4])


def test_disc_256_bins_of_small_hazards(poison):  # noqa: F811
    from advmil_amd.loss.utils import SurvMLE
    rs = np.random.RandomState(332)
    n, bins = 300, 256
    hz = (0.02 * rs.rand(n, bins)).astype(np.float32)
    t = np.floor(rs.rand(n) * bins).astype(np.float32)
    t[:3] = (0.0, 255.0, 128.0)
    e = (rs.rand(n) < 0.5).astype(np.float32)
    fake = (4.0 * rs.rand(n) - 2.0).astype(np.float32)
    for alpha in (0.0, 0.3):
        # precondition (CPU): the reference's own arithmetic -- the running product in float32 -- lies within TOL / 4 of float64 on this
        # input, which leaves the kernel three quarters of the tolerance
        f32 = float(SurvMLE(alpha=alpha)(torch.from_numpy(hz), torch.from_numpy(t), torch.from_numpy(e)))
        want = mle_f64(hz, t, e.astype(np.float64), alpha)
        assert abs(f32 - want) <= TOL / 4 * max(1.0, abs(want)), (alpha, f32, want)
    _, risk = check_disc(hz, t, e, fake, 0.3, "bce", "256 bins")
    assert np.array_equal(risk.view(np.int32), K.numpy_risk(hz).view(np.int32))


# ---- 4. advmil_ple_loss ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 256, 257, 1025))
def test_ple_three_time_levels_and_the_clamp_at_ten(poison, n):  # noqa: F811
    rs = np.random.RandomState(340 + n)
    t = (np.floor(rs.rand(n) * 3) / 3).astype(np.float32)
    e = (rs.rand(n) < 0.5).astype(np.float32)
    e[0] = 1.0
    theta = (3.0 * rs.randn(n)).astype(np.float32)
    theta[0] = 10.0                                                 # exactly the clamp
    theta[-1] = 10.0 if n == 1 else 12.0                            # ... and above it
    out = K.ple(theta, t, e)
    want = ple_f64(theta, t, e)
    assert close(float(out[0]), want), (n, float(out[0]), want)
    assert out[1] == float(e.sum())
    if n == 1:
        assert abs(out[0]) <= 1e-6                                   # theta - log(exp(theta)): one fp32 exp and one double log
    out0 = K.ple(theta, t, np.zeros(n, dtype=np.float32))
    assert out0[0] == 0.0 and out0[1] == 0.0


# ---- 5. advmil_rank_loss_fwd / _bwd ---------------------------------------------------------------------------------------------------
RANK_CONFIGS = (("l1", False), ("l1", True), ("l2", False), ("l2", True))
GAMMA_L1 = 17.0 / 128.0      # an odd multiple of 1/128: with pred on multiples of 1/64 every |gamma + x| is at least 1/128


def grid_pred(rs, n, lo, hi):
    """pred on multiples of 1/64 in [lo, hi]."""
    return (np.floor(rs.rand(n) * (hi - lo) * 64) / 64 + lo).astype(np.float32)


def check_rank(pred, t, e, gamma, norm, aw, what):
    state, loss, grad = K.rank(pred, t, e, gamma, norm, aw, gout=1.0)
    want_loss, want_grad, margin = rank_loss_f64(pred, t, e, gamma, norm, aw)
    assert margin >= 1e-6, (what, margin)
    gmax = float(np.abs(want_grad).max())
    assert abs(float(loss) - want_loss) <= TOL * abs(want_loss), (what, float(loss), want_loss)
    assert float(np.float32(state[0])) == float(loss)
    assert float(np.abs(grad.astype(np.float64) - want_grad).max()) <= TOL * gmax, (what, float(np.abs(grad - want_grad).max()), gmax)
    return state


def test_rank_one_sample_and_two_samples_in_both_orders(poison):  # noqa: F811
    for norm, aw in RANK_CONFIGS:
        state, loss, grad = K.rank([0.4], [0.5], [1.0], GAMMA_L1, norm, aw, gout=1.0)
        assert not state.any() and float(loss) == 0.0 and grad.tolist() == [0.0]
        for t in ((0.25, 0.75), (0.75, 0.25)):
            pred, e = np.array([0.5, 0.25], dtype=np.float32), np.array([1.0, 1.0], dtype=np.float32)
            state = check_rank(pred, np.array(t, dtype=np.float32), e, GAMMA_L1, norm, aw, (norm, aw, t))
            x = 0.25 if t[0] < t[1] else -0.25
            assert state[3] == 1.0 and state[1] == 1.0 and state[2] == (x if aw else 0.0)       # one pair: Z = exp(0) = 1, M = x
    # the later sample holds the event only: no pair
    state, loss, grad = K.rank([0.5, 0.25], [0.25, 0.75], [0.0, 1.0], GAMMA_L1, "l1", True, gout=1.0)
    assert not state.any() and float(loss) == 0.0 and not grad.any()


def test_rank_state_array_at_n1000_with_50_time_levels(poison):  # noqa: F811
    rs = np.random.RandomState(350)
    n = 1000
    t = (np.floor(rs.rand(n) * 50) / 50).astype(np.float32)
    e = (rs.rand(n) < 0.4).astype(np.float32)
    pred = grid_pred(rs, n, 0.0, 1.0)
    P, M, Z = K.pair_state_f64(pred, t, e)
    assert P > 0
    for norm, aw in RANK_CONFIGS:
        state = check_rank(pred, t, e, GAMMA_L1, norm, aw, ("n1000", norm, aw))
        assert state[3] == float(P), (state[3], P)
        if aw:
            assert state[2] == float(M), (state[2], float(M))       # a single float32 subtraction on both sides
            assert close(float(state[1]), Z), (float(state[1]), Z)
        else:
            assert state[1] == state[3] and state[2] == 0.0


def test_rank_softmax_weights_with_pred_spread_over_sixteen_units(poison):  # noqa: F811
    """pred over [-8, 8]: the per-anchor rescale exp(m_i - M) of the merge spans e^-16 to 1 (with pred in [0, 1] it never leaves [e^-1, 1])."""
    rs = np.random.RandomState(351)
    n = 700
    t = (np.floor(rs.rand(n) * 30) / 30).astype(np.float32)
    e = (rs.rand(n) < 0.5).astype(np.float32)
    pred = grid_pred(rs, n, -8.0, 8.0)
    P, M, Z = K.pair_state_f64(pred, t, e)
    for norm in ("l1", "l2"):
        state = check_rank(pred, t, e, GAMMA_L1, norm, True, ("spread", norm))
        assert state[3] == float(P) and state[2] == float(M) and close(float(state[1]), Z)


def test_rank_two_calls_interleaved_keep_their_own_state(poison):  # noqa: F811
    from advmil_amd.loss.utils import rank_loss
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(352)
    inputs = []
    for n in (300, 517):
        inputs.append((grid_pred(rs, n, 0.0, 2.0), (np.floor(rs.rand(n) * 20) / 20).astype(np.float32), (rs.rand(n) < 0.5).astype(np.float32)))

    def fwd(k, norm, aw):
        pred, t, e = inputs[k]
        p = torch.from_numpy(pred).to(dev).requires_grad_(True)
        return p, rank_loss(p, torch.from_numpy(t).to(dev), torch.from_numpy(e).to(dev), gamma=GAMMA_L1, norm=norm, add_weight=aw)

    for norm, aw in RANK_CONFIGS:
        alone = []
        for k in (0, 1):
            p, loss = fwd(k, norm, aw)
            loss.backward()
            alone.append(p.grad.clone())
        (p0, l0), (p1, l1) = fwd(0, norm, aw), fwd(1, norm, aw)     # both forwards before either backward
        l0.backward()
        l1.backward()
        for got, want in zip((p0.grad, p1.grad), alone):
            assert float(want.abs().max()) > 0
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (norm, aw)
