"""GPU: the handlers with the optimizers create_optimizer gained (advmil_amd.optim.FlatOptim) -- MyHandler's generator with
opt_netG in {adamw, lookahead_radam} (D stays FlatAdam, as in the reference), BaselineHandler with opt_net: nadam -- at tiny ABMIL
bags (4 bags x 32 patches). Every optimizer step is intercepted: the update it makes equals the float64 restatement
(tests/optim_ref.py) applied to the gradient it was given, the L1 fold and the decay filter included; save -> resume -> the next
step is identical; the replayed step-graph loop equals the eager one bit for bit (the pattern of tests/test_step_graphs_gpu.py)."""
import numpy as np
import pytest
import torch

from advmil_amd.config import default_baseline_cfg, default_cfg
from tests import helpers as H
from tests import optim_ref as R
from tests.poison import poison  # noqa: F401  (fixture)
from tests.test_parity_gpu import DEV, load_synth, zero_dropout

pytestmark = pytest.mark.gpu
NB, ROWS = 4, 32


class Watch:
    """Wraps opt.step: snapshots the parameter and gradient arenas before each call and holds the restatement that follows it."""

    def __init__(self, opt):
        from advmil_amd.optim import FlatOptim
        assert isinstance(opt, FlatOptim)
        self.opt, self.inner, self.worst = opt, opt.step, []
        g0 = opt.param_groups[0]
        self.ref = R.Ref(opt.kind, opt.flat_param.cpu().numpy(), wd=opt.flat_wd.cpu().numpy().astype(np.float64), lr=g0["lr"],
                         l1_coef=opt.l1_coef, lookahead=opt.lookahead, k=g0.get("lookahead_k", 6), alpha=g0.get("lookahead_alpha", 0.5))
        opt.step = self.step

    def step(self, *a, **k):
        p0 = self.opt.flat_param.cpu().numpy().astype(np.float64)
        g = self.opt.flat_grad.cpu().numpy().astype(np.float64)
        self.inner(*a, **k)
        self.ref.p = p0.copy()               # each step is judged from the weights it started from (the states run on in float64)
        self.ref.lr = self.opt.param_groups[0]["lr"]
        self.ref.do_step(g, grad_scale=k.get("grad_scale", 1.0))
        err, bnd = R.bound(self.opt.flat_param.cpu().numpy(), self.ref.p, p0, 1)
        self.worst.append((err, bnd))
        assert err <= bnd, (len(self.worst), err, bnd)
        assert float(np.abs(g).max()) > 0.0


def g_batch(base):
    xs = [[H.bag(base + i, ROWS, DEV), torch.zeros(1, 1, device=DEV)] for i in range(NB)]
    ys_host = [H.label(base + i) for i in range(NB)]
    nz = [[H.noise_tensor("opt", base + i, 192, DEV)] for i in range(NB)]
    return xs, ys_host, [y.to(DEV) for y in ys_host], nz


@pytest.mark.parametrize("name,steps", [("adamw", 3), ("lookahead_radam", 13)])
def test_generator_steps_equal_restatement_and_resume(name, steps, tmp_path, poison):
    from advmil_amd.model import MyHandler
    from advmil_amd.optim import FlatAdam
    cfg = default_cfg(bcb_mode="abmil", bp_every_batch=NB, opt_netG=name, save_path=str(tmp_path))
    xs, ys_host, ys, nz = g_batch(500)

    def run(h, n):
        for _ in range(n):
            h._update_disc(0, xs, ys, ys_host=ys_host, noise=nz)
            h._update_gen(0, xs, ys, ys_host=ys_host, noise=nz)

    a = MyHandler(cfg, device=DEV); zero_dropout(a.netG); zero_dropout(a.netD)
    assert type(a.optimizerD) is FlatAdam and a.optimizerG.l1_coef == pytest.approx(1e-5) and a.optimizerG._has_wd
    w = Watch(a.optimizerG)
    run(a, steps)
    assert len(w.worst) == steps and int(a.optimizerG.step_t) == steps
    if name == "lookahead_radam":
        assert w.ref.syncs == [(6, "create"), (12, "blend")] and w.ref.rectified[0] is False and w.ref.rectified[-1] is True
    # the scheduler the handler builds drives the new class
    lr0 = a.optimizerG.param_groups[0]["lr"]
    for _ in range(12):
        a.steplr.step(1.0)
    assert a.optimizerG.param_groups[0]["lr"] == lr0 * 0.5 == a.optimizerG.param_groups[1]["lr"]
    run(a, 1)                                # ... and the step after it uses the new rate (checked by the watch)
    a.save_model(steps + 1, "last", "train")
    run(a, 1)
    b = MyHandler(cfg, device=DEV); zero_dropout(b.netG); zero_dropout(b.netD)
    b.resume_model("last", "train")
    run(b, 1)
    for pa, pb in ((a.optimizerG, b.optimizerG), (a.optimizerD, b.optimizerD)):
        assert torch.equal(pa.flat_param, pb.flat_param) and torch.equal(pa.flat_m, pb.flat_m) and torch.equal(pa.flat_v, pb.flat_v)
        assert int(pa.step_t) == int(pb.step_t) == steps + 2
    assert torch.equal(a.optimizerG.planes.hi.view(torch.int16), b.optimizerG.planes.hi.view(torch.int16))
    if a.optimizerG.lookahead:
        assert torch.equal(a.optimizerG.flat_slow, b.optimizerG.flat_slow)


def test_baseline_handler_with_nadam(tmp_path, poison):
    from advmil_amd.model import BaselineHandler
    cfg = default_baseline_cfg(bcb_mode="abmil", task="surv_reg", bp_every_batch=NB, opt_net="nadam", save_path=str(tmp_path))
    xs = [[H.bag(600 + i, ROWS, DEV), torch.zeros(1, 1, device=DEV)] for i in range(NB)]
    ys = [H.label(600 + i).to(DEV) for i in range(NB)]
    a = BaselineHandler(cfg, device=DEV); zero_dropout(a.net)
    w = Watch(a.optimizer)
    for _ in range(3):
        a._update_network(0, xs, ys)
    assert len(w.worst) == 3 and a.optimizer.kind == "nadam" and a.optimizer.l1_coef == pytest.approx(1e-5)
    a.save_model(1, "last")
    a._update_network(0, xs, ys)
    b = BaselineHandler(cfg, device=DEV); zero_dropout(b.net)
    b.resume_model("last")
    ms3 = float(np.prod([0.9 * (1.0 - 0.5 * 0.96 ** (t * 4e-3)) for t in (1, 2, 3)]))       # the schedule product the checkpoint held
    assert b.optimizer.state_dict()["state"][0]["m_schedule"] == pytest.approx(ms3, rel=1e-13)
    b._update_network(0, xs, ys)
    assert torch.equal(a.optimizer.flat_param, b.optimizer.flat_param) and torch.equal(a.optimizer.flat_m, b.optimizer.flat_m)
    assert torch.equal(a.optimizer.m_sched[0:1], b.optimizer.m_sched[0:1]) and int(a.optimizer.step_t) == int(b.optimizer.step_t) == 4


# ---- the shape-keyed step graphs of the epoch loop: 8 resident step batches of one key, two epochs = 16 generator steps (the
# lookahead syncs at 6 and 12 fall into replayed steps)
def _epochs(name, graphs):
    from advmil_amd import synth
    from advmil_amd.model import MyHandler
    h = MyHandler(default_cfg(bcb_mode="abmil", bp_every_batch=NB, gemm_mode="bf16x3", step_graphs=1, step_graphs_max=8 if graphs else 0,
                              bag_cache_gb=1, opt_netG=name), device=DEV)
    load_synth(h.netG, "G-abmil:"); load_synth(h.netD, "D-prj:")
    h.optimizerG.refresh_planes(); h.optimizerD.refresh_planes()
    h.rng.reset(77)
    n = NB * 8
    h.patient_id.update({"train": [f"t{i}" for i in range(n)], "label_visible": [f"t{i}" for i in range(n)]})
    loader = [(torch.tensor([[i]], dtype=torch.int), [H.T(synth.bag(H.DATA_SEED, 700 + i, ROWS)).pin_memory(), torch.zeros(1, 1)],
               torch.tensor([[0.2 + 0.013 * i, float(i % 2)]])) for i in range(n)]
    cls = [h._train_each_epoch(loader, "train", "wlabel") for _ in range(2)]
    torch.cuda.synchronize()
    return h, cls, h.pop_logs()


@pytest.mark.parametrize("name", ["lookahead_radam", "adamw"])
def test_replayed_step_graphs_equal_eager_steps(name):
    from advmil_amd import ops
    prev = ops.get_gemm_mode()
    try:
        hg, cg, lg = _epochs(name, True)
        he, ce, le = _epochs(name, False)
    finally:
        ops.set_gemm_mode(prev)
    assert hg.step_graph_stats["replayed"] >= 10 and hg.step_graph_stats["captured"] >= 1, hg.step_graph_stats
    assert he.step_graph_stats == {"replayed": 0, "captured": 0, "eager": 16}, he.step_graph_stats
    for a, b in zip(cg, ce):
        for k in ("y", "y_hat", "f_fake"):
            assert torch.equal(a[k], b[k]), k
    assert len(lg) == len(le)
    for a, b in zip(lg, le):
        assert a == b, (a, b)
    for k in ("flat_param", "flat_m", "flat_v") + (("flat_slow",) if hg.optimizerG.lookahead else ()):
        assert torch.equal(getattr(hg.optimizerG, k), getattr(he.optimizerG, k)), k
    assert torch.equal(hg.optimizerD.flat_param, he.optimizerD.flat_param)
    assert int(hg.optimizerG.step_t) == int(he.optimizerG.step_t) == 16
