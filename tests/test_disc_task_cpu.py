"""CPU: the discrete-time adversarial task (task: disc_gansurv) off the device -- the float64 restatement (tests/disc_ref.py) against the
reference's own get_label_mask / SurvMLE (tests/golden/golden_disc_v1.npz, section (a)), the label and mask rows the step plan builds on
the host against the reference's rows, and the config checks of the reference's model_handler.py:786, 806-810."""
import os

import numpy as np
import pytest

from advmil_amd.config import default_cfg
from tests import disc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gd():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_disc_v1.npz"))


def disc_cfg(**over):
    cfg = default_cfg(task="disc_gansurv", time_format="quantile", time_bins=4, gen_dims="384-4", disc_nety_in_dim=4)
    cfg.update(over)
    return cfg


def test_restatement_matches_the_reference_functions(gd):
    for K in (1, 4, 7):
        t, e = gd[f"LM_K{K}_t"], gd[f"LM_K{K}_e"]
        label, mask = R.get_label_mask(t, e, K)
        assert np.array_equal(label, gd[f"LM_K{K}_label"]) and np.array_equal(mask, gd[f"LM_K{K}_mask"])
        assert np.array_equal(R.real_rows(t, e, K), gd[f"LM_K{K}_real"])
    cases = R.loss_cases() + [R.extreme_case_f64()]
    assert len(cases) == 4 * 4 * 3 * 2 + 2
    for c in cases:
        v, g = R.surv_mle(c["hz"], c["t"], c["e"], c["alpha"], c["eps"])
        assert abs(v - float(gd[f"MLE_{c['name']}_value"])) <= 1e-12, c["name"]
        assert float(np.abs(g - gd[f"MLE_{c['name']}_grad"]).max()) <= 1e-12, c["name"]


def test_the_extreme_case_clamps_every_kind_of_log_argument():
    c = R.loss_cases()[-1]
    d = R.surv_mle_terms(c["hz"], c["t"], c["e"], c["alpha"], c["eps"])
    for k in ("S_t", "h_t", "S_t1"):
        cl = d[f"clamped_{k}"]
        assert cl.any() and not cl.all(), k
        assert not d[f"grad_{k}"][cl].any(), k                     # a clamped argument contributes exactly nothing


def test_plan_label_rows_equal_the_reference_rows(gd):
    from advmil_amd.model.model_handler import disc_label_rows
    for K in (1, 4, 7):
        t, e = gd[f"LM_K{K}_t"], gd[f"LM_K{K}_e"]
        assert {0, K - 1} <= set(t.reshape(-1).astype(int).tolist()) and set(e.reshape(-1).tolist()) == {0.0, 1.0}
        real, mask = disc_label_rows(np.concatenate([t, e], axis=1), K)
        assert real.dtype == np.float32 and mask.dtype == np.float32 and real.shape == mask.shape == (2 * K, K)
        assert np.array_equal(real, gd[f"LM_K{K}_real"]) and np.array_equal(mask, gd[f"LM_K{K}_mask"])
        ev = e.reshape(-1) == 1
        assert not real[ev].any()                                  # an event bag's real row is all zeros ...
        assert np.array_equal(real[~ev], np.eye(K, dtype=np.float32)[t.reshape(-1).astype(int)[~ev]])       # ... a censored one's one-hot at t
    for bad in (0.5, -1.0, 4.0, float("nan")):
        with pytest.raises(ValueError, match="bin index"):
            disc_label_rows(np.array([[1.0, 1.0], [bad, 0.0]]), 4)


def test_check_configs_accepts_the_discrete_task_and_rejects_each_violation():
    from advmil_amd.model.model_handler import _check_configs
    _check_configs(disc_cfg())
    _check_configs(default_cfg())
    for over in (dict(time_format="ratio"), dict(time_format="origin"), dict(gen_out_scale="none"), dict(gen_out_scale="exp"),
                 dict(time_bins=5), dict(disc_nety_in_dim=1), dict(gen_dims="384-1"), dict(gen_dims="384-8"), dict(log_plot=True)):
        with pytest.raises(AssertionError):
            _check_configs(disc_cfg(**over))
    with pytest.raises(AssertionError, match="HIP path covers"):
        _check_configs(default_cfg(task="surv_reg"))


def test_loss_entry_points_refuse_bad_shapes_before_any_launch():
    """1 <= B <= 32, 1 <= K <= 32 (advmil_gan_g_loss_disc), non-empty rows (advmil_mask_rows): ADVMIL_EINVAL from the host-side checks --
    no device is present here, so a call that got as far as a launch would answer with a hipError_t instead."""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    L = _lib.lib()
    p = lambda k: ctypes.c_void_p(0x7F0000001000 + (k << 20))   # noqa: E731  (fake addresses: never dereferenced)
    call = lambda B, K, hz=p(0): L.advmil_gan_g_loss_disc(hz, p(1), p(2), None, p(3), B, K, 0.0, 1e-7, 0.004, 1.0, 1.0, p(4), p(5), p(6), None)   # noqa: E731
    for B, K in ((33, 4), (0, 4), (-1, 4), (4, 0), (4, 33), (4, -1)):
        assert call(B, K) == -1, (B, K)
    assert call(4, 4, None) == -1
    assert L.advmil_mask_rows(p(0), p(1), 0, 4, p(2), None) == -1 and L.advmil_mask_rows(p(0), p(1), 4, 0, p(2), None) == -1
    assert L.advmil_mask_rows(p(0), p(1), 1 << 31, 2, p(2), None) == -1 and L.advmil_mask_rows(p(0), None, 4, 4, p(2), None) == -1
