"""GPU: the discrete-time adversarial task (task: disc_gansurv) on the HIP step.
 * advmil_gan_g_loss_disc / advmil_mask_rows against the float64 restatement tests/disc_ref.py (itself pinned to the reference's SurvMLE /
   get_label_mask: tests/golden/ORACLE_PIN_disc.json), value and analytic gradient, under both allocation-poisoning patterns;
 * two optimizer steps of MyHandler._train_each_epoch, and MyHandler.test_model, against the reference's own handler
   (tests/golden/golden_disc_v1.npz; bounds of tests/test_parity_gpu.py::test_G4_two_optimizer_steps_vs_reference);
 * one epoch of ragged bags with the shipped dropout per backbone: finite, no eager Linear / LayerNorm, no step graph captured."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from advmil_amd import synth
from advmil_amd.config import default_cfg
from tests import disc_ref as R
from tests import helpers as H
from tests.poison import poison  # noqa: F401  (fixture: both poison patterns)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5
BINS = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.loss_cases()


@pytest.fixture(scope="module")
def gd():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_disc_v1.npz"))


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import _lib
    from advmil_amd import ops as _ops
    _lib.lib()
    return _ops


def dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).requires_grad_(grad)


def vis_variants(B):
    """(vis array | None, n_vis): NULL, partial (every other bag; B == 1: an explicit all-ones mask), all-zero with inv_nv = 0."""
    part = (np.arange(B) % 2 == 0).astype(np.float32)
    return ((None, B), (part, int(part.sum())), (np.zeros(B, dtype=np.float32), 0))


def run_loss(ops, c, vis, n_vis, coef=0.004, root=True, go=None):
    hz, fake = dev(c["hz"], True), dev(c["fake"], True)
    total, st = ops.gan_g_loss_disc(hz, fake, dev(c["t"]), dev(c["e"]), None if vis is None else dev(vis), c["alpha"], c["eps"], coef,
                                    hz.shape[0], n_vis, root=root)
    torch.autograd.backward(total, grad_tensors=go)
    return (float(total.detach()), st.double().cpu().numpy(), hz.grad.double().cpu().numpy(), fake.grad.double().cpu().numpy())


def check_loss(ops, c, vis, n_vis, coef=0.004):
    total, st, g_hz, g_fake = run_loss(ops, c, vis, n_vis, coef)
    out3, r_hz, r_fake, d = R.g_loss(c["hz"], c["t"], c["e"], vis, c["fake"], c["alpha"], c["eps"], coef, c["hz"].shape[0], n_vis)
    tag = (c["name"], None if vis is None else vis.tolist())
    assert abs(total - out3[0]) <= TOL and float(np.abs(st - out3).max()) <= TOL, (tag, st, out3)
    assert float(np.abs(g_hz - r_hz).max()) <= TOL * max(1.0, float(np.abs(r_hz).max())), tag
    assert float(np.abs(g_fake - r_fake).max()) <= TOL * max(1.0, float(np.abs(r_fake).max())), tag
    if n_vis == 0:
        assert st[1] == 0.0 and not g_hz.any(), tag
    return g_hz, r_hz, d


@pytest.mark.parametrize("B", R.LOSS_B)
def test_loss_kernel_vs_restatement(ops, poison, B):  # noqa: F811
    """B x K in {1, 4, 7, 32} x {all-event, all-censored, mixed} x alpha in {0, 0.3} x vis in {NULL, partial, all-zero}."""
    cases = [c for c in CASES[:-1] if c["hz"].shape[0] == B]
    assert len(cases) == 4 * 3 * 2 and {c["hz"].shape[1] for c in cases} == set(R.LOSS_K)
    assert {(c["hz"].shape[1], c["t"][0]) for c in cases} >= {(K, K - 1.0) for K in R.LOSS_K} | {(K, 0.0) for K in R.LOSS_K if B == 1}
    for c in cases:
        K = c["hz"].shape[1]
        assert set(c["t"][:2].tolist()) == {0.0, K - 1.0} or (B == 1 and c["t"][0] in (0.0, K - 1.0))
        for vis, n_vis in vis_variants(B):
            check_loss(ops, c, vis, n_vis)


def test_loss_kernel_clamped_arguments_have_exactly_zero_gradient(ops, poison):  # noqa: F811
    """Hazards 1e-9 and 1 - 1e-9: every log argument the restatement reports as clamped contributes an exactly zero gradient."""
    c = CASES[-1]
    assert c["name"] == "extreme"
    for vis, n_vis in vis_variants(16)[:2]:
        g_hz, r_hz, d = check_loss(ops, c, vis, n_vis)
        ti = c["t"].astype(int)[:, None]
        j = np.arange(7)[None, :]
        support = {"S_t": j < ti, "h_t": j == ti, "S_t1": j <= ti}
        seen = 0
        for k, sup in support.items():
            cl = d[f"clamped_{k}"][:, None] & sup
            assert cl.any(), k
            others = sum(d[f"grad_{q}"] for q in support if q != k)
            only = cl & (others == 0.0)                          # elements this log alone could have reached
            assert only.any(), k
            assert not g_hz[only].any(), k
            seen += int(only.sum())
        assert seen >= 3
        assert not g_hz[r_hz == 0.0].any()                       # ... and nothing anywhere the restatement has an exact zero


def test_loss_kernel_upstream_gradient_and_coef(ops):
    c = CASES[4 * 3 * 2 * 2 + 9]                                  # a 16-bag case
    B = c["hz"].shape[0]
    _, _, g1, f1 = run_loss(ops, c, None, B, coef=0.5)
    _, _, g2, f2 = run_loss(ops, c, None, B, coef=0.5, root=False, go=torch.tensor(2.0, device=DEV))
    assert np.array_equal(2.0 * g1, g2) and np.array_equal(2.0 * f1, f2)
    assert np.all(f1 == np.float32(-0.5) / np.float32(B))


def test_loss_kernel_argument_errors_return_einval(ops):
    from advmil_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(33 * 33 + 64, device=DEV)
    p = lambda o=0: ctypes.c_void_p(buf.data_ptr() + 4 * o)     # noqa: E731
    call = lambda B, K: L.advmil_gan_g_loss_disc(p(), p(), p(), None, p(), B, K, 0.0, 1e-7, 0.004, 1.0, 1.0, p(), p(), p(), None)   # noqa: E731
    assert call(33, 4) == -1 and call(4, 0) == -1 and call(4, 33) == -1 and call(0, 4) == -1
    assert L.advmil_gan_g_loss_disc(None, p(), p(), None, p(), 4, 4, 0.0, 1e-7, 0.004, 1.0, 1.0, p(), p(), p(), None) == -1
    assert L.advmil_mask_rows(p(), p(), 0, 4, p(), None) == -1 and L.advmil_mask_rows(p(), None, 4, 4, p(), None) == -1
    torch.cuda.synchronize()
    assert not buf.any()                                          # nothing was launched
    with pytest.raises(_lib.AdvmilHipError, match="invalid argument"):
        ops.gan_g_loss_disc(torch.zeros(33, 4, device=DEV), torch.zeros(33, device=DEV), torch.zeros(33, device=DEV),
                            torch.zeros(33, device=DEV), None, 0.0, 1e-7, 0.004, 33, 33)


@pytest.mark.parametrize("B,K", [(1, 1), (5, 7), (32, 32), (16, 4), (1100, 300)])
def test_mask_rows_forward_and_backward_are_exact(ops, poison, B, K):  # noqa: F811
    rs = np.random.default_rng(B * 1000 + K)
    x, go = rs.standard_normal((B, K)).astype(np.float32), rs.standard_normal((B, K)).astype(np.float32)
    m = (rs.random((B, K)) < 0.5).astype(np.float32)
    xt = dev(x, True)
    y = ops.mask_rows(xt, dev(m))
    y.backward(dev(go))
    assert np.array_equal(y.detach().cpu().numpy(), x * m) and np.array_equal(xt.grad.cpu().numpy(), go * m)
    out = torch.empty(B, K, device=DEV)
    with torch.no_grad():
        assert ops.mask_rows(dev(x), dev(m), out=out) is out
    assert np.array_equal(out.cpu().numpy(), x * m)


# ------------------------------------------------------------------------------------------------------------------------------
# the step against the reference's own handler
# ------------------------------------------------------------------------------------------------------------------------------
def disc_cfg(kind, **over):
    cfg = dict(task="disc_gansurv", time_format="quantile", time_bins=BINS, gen_dims=f"384-{BINS}", disc_nety_in_dim=BINS, bcb_mode=kind)
    cfg.update(over)
    return default_cfg(**cfg)


def bin_label(i):
    y = synth.label(H.DATA_SEED, i).copy()
    y[0, 0] = np.floor(BINS * y[0, 0])
    return H.T(y)


def close(a, b, tol=TOL):
    a = torch.as_tensor(np.asarray(a.detach().float().cpu() if torch.is_tensor(a) else a)).double().reshape(-1)
    b = torch.as_tensor(np.asarray(b)).double().reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    d = float((a - b).abs().max())
    assert d <= tol, d
    return d


def load_synth(module, prefix):
    sd = {k: H.T(synth.param(H.PARAM_SEED, prefix + k, tuple(v.shape))) for k, v in module.state_dict().items()}
    module.load_state_dict(sd, strict=True)
    return {k: v.clone() for k, v in sd.items()}


def zero_dropout(net):
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
        if hasattr(m, "drop_p"):
            m.drop_p = 0.0


def two_steps_vs_reference(gd, name, kind, tag, mode="wlabel", visible=lambda i: True, **over):
    from advmil_amd.model import MyHandler
    h = MyHandler(disc_cfg(kind, **over), device=DEV)
    PG0, PD0 = load_synth(h.netG, f"G-{kind}:"), load_synth(h.netD, "D-prj:")
    zero_dropout(h.netG); zero_dropout(h.netD)
    nb = 32
    width = int(gd[f"{name}_noise_width"])
    h.patient_id["train"] = [str(i) for i in range(nb)]
    h.patient_id["label_visible"] = [str(i) for i in range(nb) if visible(i)]
    h.noise_hook = lambda ph, i: [H.noise_tensor(f"{tag}{ph}:{kind}", i, width, DEV)]
    loader = [(torch.tensor([[i]], dtype=torch.int), [H.bag(i, 512), torch.zeros(1, 1)], bin_label(i)) for i in range(nb)]
    cl = h._train_each_epoch(loader, "train", mode=mode)
    logs = h.pop_logs()
    ref = gd[f"{name}_logs"]
    for s in range(2):
        d, g = logs[2 * s], logs[2 * s + 1]
        got = [d["train_batch/netD/Loss_D"], d["train_batch/netD/D_real"], d["train_batch/netD/D_fake"],
               g["train_batch/netG/Loss_G_fake"], g["train_batch/netG/Loss_G_time"], g["train_batch/netG/Loss_G_total"],
               g["train_batch/netG/D_fake_avg"]]
        print(name, "step", s, "logs", got, "ref", ref[s].tolist())
        close(torch.tensor(got, dtype=torch.float64), ref[s])
    assert tuple(cl["y_hat"].shape) == (nb, BINS) and tuple(cl["f_fake"].shape) == (nb,)
    close(cl["y_hat"], gd[f"{name}_y_hat"])
    close(cl["f_fake"], gd[f"{name}_f_fake"])
    close(cl["y"], gd[f"{name}_y"], 0.0)
    for t_, net, P0 in (("G", h.netG, PG0), ("D", h.netD, PD0)):
        sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        keys = [str(k) for k in gd[f"{name}_keys{t_}"]]
        dn = np.array([float((sd[k].double() - P0[k].double()).norm()) for k in keys])
        ref_dn = gd[f"{name}_d{t_}_stats"][:, 1]
        assert np.all(np.abs(dn - ref_dn) <= 5e-3 * ref_dn + 5e-5), float(np.abs(dn - ref_dn).max())
    gk = [str(k) for k in gd[f"{name}_gradG2_keys"]]
    named = dict(h.netG.named_parameters())
    gn = np.array([float((named[k].grad.double() + 1e-5 * torch.sign(named[k].detach().double())).norm()) for k in gk])
    assert np.allclose(gn, gd[f"{name}_gradG2_norm"], rtol=5e-3, atol=5e-6), np.abs(gn - gd[f"{name}_gradG2_norm"]).max()
    assert h.step_graph_stats["captured"] == 0 and h.step_graph_stats["replayed"] == 0 and h.step_graph_stats["eager"] == 2
    return h


@pytest.mark.parametrize("kind,gemm_mode", [("abmil", "exact"), ("abmil", "bf16x3"), ("patch", "exact")])
def test_two_optimizer_steps_vs_reference(gd, ops, poison, kind, gemm_mode):  # noqa: F811
    """The reference's own _train_each_epoch with task=disc_gansurv (dropout p=0, injected noise, 2 x 16 bags of 512) vs ours."""
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(gemm_mode)
    try:
        two_steps_vs_reference(gd, f"D4_{kind}", kind, "D4")
    finally:
        ops.set_gemm_mode(prev)


def test_two_steps_with_invisible_labels_keep_every_real_pair(gd, poison):  # noqa: F811
    """mode='wolabel', every third bag's label invisible: the supervised term drops those bags, the real pairs do not."""
    two_steps_vs_reference(gd, "D4c_abmil", "abmil", "D4c", mode="wolabel", visible=lambda i: i % 3 != 0)


def test_test_model_vs_reference(gd, poison):  # noqa: F811
    from types import SimpleNamespace
    from advmil_amd.model import Generator, MyHandler, PrjDiscriminator, load_backbone
    kind = "abmil"
    g = Generator(384, BINS, load_backbone(kind, [1024, 384, 384]), SimpleNamespace(noise=[0, 1], hops=1, noise_dist="uniform"),
                  False, 0.6, "sigmoid").to(DEV)
    ax = SimpleNamespace(in_dim=1024, out_dim=128, ksize=1, backbone="avgpool", dropout=0.25)
    ay = SimpleNamespace(in_dim=BINS, hid_dims=[64, 128], norm=False, dropout=0.0)
    d = PrjDiscriminator(ax, ay, prj_path="x", inner_product="instance").to(DEV)
    load_synth(g, f"G-{kind}:"); load_synth(d, "D-prj:")
    nb, S = 8, 3
    loader = [(torch.tensor([[i]], dtype=torch.int), [H.bag(i, 512), torch.zeros(1, 1)], bin_label(i)) for i in range(nb)]
    res = MyHandler.test_model(g, d, kind, loader, times_test_sample=1, test_zero_noise=True)
    assert tuple(res["y_hat"].shape) == (nb, BINS) and "avg_y_hat" not in res
    close(res["y_hat"], gd["D5_zero_y_hat"]); close(res["f_fake"], gd["D5_zero_f_fake"])
    noises = [[H.noise_tensor(f"D5:{kind}:{i}", k, 192, DEV) for k in range(S + 1)] for i in range(nb)]
    res = MyHandler.test_model(g, d, kind, loader, times_test_sample=S, test_zero_noise=False, noise=noises)
    assert tuple(res["dist_y_hat"].shape) == (nb, S, BINS) and tuple(res["avg_y_hat"].shape) == (nb, BINS)
    for k in ("y_hat", "f_fake", "dist_y_hat", "avg_y_hat"):
        close(res[k], gd[f"D5_noise_{k}"])


# ------------------------------------------------------------------------------------------------------------------------------
# dropout on, ragged bags
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_aten(monkeypatch):
    calls = []

    def boom(name):
        def f(*a, **k):
            calls.append(name)
            raise AssertionError(f"eager torch.nn.functional.{name} reached from the product path")
        return f
    monkeypatch.setattr(F, "linear", boom("linear"))
    monkeypatch.setattr(F, "layer_norm", boom("layer_norm"))
    return calls


@pytest.mark.parametrize("kind", ["abmil", "cluster", "patch"])
def test_one_ragged_epoch_with_the_shipped_dropout(no_aten, poison, kind):  # noqa: F811
    from advmil_amd.model import MyHandler
    lens = (256, 512, 128, 64)
    h = MyHandler(disc_cfg(kind, bp_every_batch=len(lens)), device=DEV)
    loader = []
    for i, n in enumerate(lens):
        x = H.bag(300 + i, 512)[:, :n].contiguous()
        ext = H.T(synth.cluster_ids(0, 300 + i, n)) if kind == "cluster" else torch.zeros(1, 1)
        loader.append((torch.tensor([[i]], dtype=torch.int), [x, ext], bin_label(i)))
    cl = h._train_each_epoch(loader, "train")
    logs = h.pop_logs()
    assert tuple(cl["y_hat"].shape) == (len(lens), BINS)
    assert bool(torch.isfinite(cl["y_hat"]).all()) and bool(torch.isfinite(cl["f_fake"]).all())
    assert all(np.isfinite(v) for d in logs for v in d.values())
    for p in list(h.netG.parameters()) + list(h.netD.parameters()):
        assert bool(torch.isfinite(p).all())
    assert no_aten == []
    assert h.step_graph_stats["captured"] == 0 and h.step_graph_stats["replayed"] == 0


def test_constructor_limits_and_plan_label_checks():
    from advmil_amd.model import MyHandler
    with pytest.raises(ValueError, match="32"):
        MyHandler(disc_cfg("abmil", time_bins=33, gen_dims="384-33", disc_nety_in_dim=33), device=DEV)
    h = MyHandler(disc_cfg("abmil", bp_every_batch=1), device=DEV)
    assert h.nbins == BINS and h.ret_metrics == ["c_index", "loss_mle_org"] and type(h.evaluator).__name__ == "DiscSurv_Evaluator"
    assert h.metrics_list == ["c_index", "loss_mle", "loss_mle_org", "loss_fake_netD", "loss_fake_netG", "avg_fake"]
    xs = [[H.bag(0, 64, DEV), None]]
    for bad in (0.37, 4.0, -1.0):                                 # refused on the host, when the plan is built: nothing is launched
        y = torch.tensor([[bad, 1.0]])
        with pytest.raises(ValueError, match="bin index"):
            h._plan(xs, [y.to(DEV)], "wlabel", None, [y])
    plan = h._plan(xs, [torch.tensor([[2.0, 0.0]], device=DEV)], "wlabel", None, [torch.tensor([[2.0, 0.0]])])
    assert plan.n_real == 1 and tuple(plan.t2.shape) == (2, BINS)
    assert plan.t2[1].tolist() == [0.0, 0.0, 1.0, 0.0] and plan.lab_mask[0].tolist() == [1.0, 1.0, 1.0, 0.0]
