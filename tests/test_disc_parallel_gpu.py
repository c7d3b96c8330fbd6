"""GPU: task = disc_gansurv under bag-parallel (2 / 4 ranks sharing the one GPU over gloo) against the single-process run over the same
global step batches, with the SHIPPED DROPOUT RATES ON -- the protocol and the comparison rules of tests/test_parallel_gpu.py. World-size
invariance of both phases: same dropout masks / generator noise per bag, global denominators (n_fake, n_vis, every bag a real pair), summed
gradient arenas, all-reduced logs, the epoch collector all-gathered in global bag order with y_hat as [n, K]. `wolabel`: on the first step
rank 1 holds no visible label while rank 0 does -- it contributes exactly zero to the SurvMLE term and still takes part in every
collective."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CASES = [("abmil", 2), ("patch", 2), ("abmil-wolabel", 2), ("abmil-bp8", 4)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind,world", _CASES, ids=[f"{k}-w{w}" for k, w in _CASES])
def test_multi_rank_discrete_step_equals_single_rank_with_dropout_on(kind, world, tmp_path):
    from tests import dp_worker_disc as W
    want = W.run(kind, 1, 0)
    out = str(tmp_path / "r0.pt")
    port = str(34300 + os.getpid() % 1500)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, "-m", "tests.dp_worker_disc", str(r), str(world), port, out, kind], cwd=ROOT, env=env)
             for r in range(world)]
    try:
        for p in procs:
            assert p.wait(timeout=500) == 0
    finally:
        for p in procs:                       # a failed rank must not leave its peers waiting in a collective
            if p.poll() is None:
                p.kill()
    got = torch.load(out, weights_only=False)
    nb = 16 if kind.endswith("-bp8") else 8
    # the fused width-K head ran in both phases of both steps, on the rank and in the single process; no step graph under world > 1
    assert got["heads"] == want["heads"] == [W.BINS] * 4
    assert got["graphs"]["captured"] == 0 and got["graphs"]["replayed"] == 0 and got["graphs"]["eager"] == 2
    # epoch collector in global bag order
    assert tuple(got["cl"]["y_hat"].shape) == tuple(want["cl"]["y_hat"].shape) == (nb, W.BINS)
    for k in ("y", "y_hat", "f_fake"):
        a, b = got["cl"][k].double().reshape(-1), want["cl"][k].double().reshape(-1)
        assert a.shape == b.shape and float((a - b).abs().max()) < 2e-6, (k, float((a - b).abs().max()))
    # logged losses: the reduced values, equal to the single-process step's
    assert len(got["logs"]) == len(want["logs"]) == 4
    for la, lb in zip(got["logs"], want["logs"]):
        for key in lb:
            if key == "i_batch":             # the rank's own loader position (local bags seen so far)
                continue
            assert abs(float(la[key]) - float(lb[key])) < 2e-6, (key, la[key], lb[key])
    if kind.endswith("-wolabel"):            # the supervised term is live (some label is visible in every step)
        assert all(abs(float(lg["train_batch/netG/Loss_G_time"])) > 1e-3 for lg in want["logs"][1::2])
    # weights after two optimizer steps: the per-tensor and per-entry rules of tests/test_parallel_gpu.py
    from advmil_amd import synth
    from tests import helpers as H
    kind = kind.split("-")[0]
    for tag, prefix in (("G", f"G-{kind}:"), ("D", "D-prj:")):
        for k in want[tag]:
            p0 = H.T(synth.param(H.PARAM_SEED, prefix + k, tuple(want[tag][k].shape))).double()
            da, db = float((got[tag][k].double() - p0).norm()), float((want[tag][k].double() - p0).norm())
            assert abs(da - db) <= 5e-3 * db + max(5e-5, 2 * 8e-5 * want[tag][k].numel() ** 0.5 if db < 2e-4 else 0.0), (tag, k, da, db)
            dw_ = (got[tag][k].double() - want[tag][k].double()).abs()
            assert int((dw_ > 2.5 * 8e-5).sum()) <= max(1, dw_.numel() // 10000), (tag, k, int((dw_ > 2.5 * 8e-5).sum()))
            assert float(dw_.max()) <= 2.05 * 8e-5 * 2, (tag, k, float(dw_.max()))
