"""The generator's bag-level head with an output layer of width K (advmil_gheadk_fwd / advmil_gheadk_bwd, the wide form of csrc/ghead.hip;
task disc_gansurv: hazards over K bins): against the float64 restatement of tests/ghead_ref.py -- the kernel's own dropout masks and
noise regenerated on the host from the recorded sites --, against the layer-by-layer path it replaces (same call sites, same draws), and
inside one step of the handler.

Bounds: those of tests/test_ghead_gpu.py (2e-6 on pred, 5e-6 on gradients, relative to the tensor's largest entry). At K = 32 the bound in
force is the larger of that and 4 x the error of the SAME restatement evaluated in float32 torch on the CPU against float64 (the rule of the
GENConv pins): a 32-row output layer sums 32 products into every element of the second layer's gradient, which the width-1 bound was not
sized for. Every comparison prints its ratio error / bound (pytest -s)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from advmil_amd import ops, synth
from advmil_amd.optim import FlatAdam
from tests.ghead_ref import HEAD_KEYS, close, ref, rel_err
from tests.poison import poison  # noqa: F401  (fixture: both poison patterns)
from tests.test_parity_gpu import DEV

pytestmark = pytest.mark.gpu
SEED = 11
# kind -> (backbone kind, backbone dims, width of the features `finish` takes): abmil has rho (384 -> 384 -> 192), patch has none
# (384 -> 192: the output share is K-split), g128 is PatchGCN's widths (128 -> 64)
KINDS = {"abmil": ("abmil", [1024, 384, 384], 384), "patch": ("patch", [1024, 384, 384], 384), "g128": ("graph", [1024, 128, 128], 128)}


def build(kind, K, noise=(0, 1), out_scale="sigmoid"):
    from advmil_amd.model import Generator, load_backbone
    bcb, dims, d0 = KINDS[kind]
    g = Generator(d0, K, load_backbone(bcb, dims), SimpleNamespace(noise=list(noise), hops=1, noise_dist="uniform"), False, 0.6, out_scale).to(DEV)
    sd = {k: torch.from_numpy(synth.param(7, f"Gk-{kind}:" + k, tuple(v.shape))).to(DEV) for k, v in g.state_dict().items()}
    g.load_state_dict(sd)
    return g


def weights(B, K):
    """w[B, K], different in every column and row: a swapped k (or b) shows in the loss's gradient."""
    return (0.5 + torch.arange(B, dtype=torch.float32).reshape(B, 1) / max(B, 2) + 0.37 * torch.arange(K, dtype=torch.float32).reshape(1, K)
            * (1.0 - 2.0 * (torch.arange(K).reshape(1, K) % 2).float())).to(DEV)


def run(kind, B, K, fused, train=True, zero_noise=False, inject=False, noise=(0, 1), frozen=False, out_scale="sigmoid", g=None):
    old, real, taken = ops.GHEAD, ops.ghead, []
    ops.GHEAD = fused
    ops.ghead = lambda *a, **k: (taken.append(1), real(*a, **k))[1]       # (did `finish` take the fused launches?)
    try:
        g = build(kind, K, noise, out_scale) if g is None else g
        d0, d2 = KINDS[kind][2], g.MLPs[0][0].out_features
        g.train(train)
        opt = FlatAdam(g, lr=1e-4)
        opt.zero_grad()
        rng = ops.DeviceRng(DEV, seed=SEED)
        rng.record = True
        for m in g.modules():
            m.rng = rng
        gen = torch.Generator().manual_seed(5)
        feats = torch.randn(B, d0, generator=gen).to(DEV).requires_grad_(True)
        nz = [torch.rand(B, d2, generator=gen).to(DEV)] if inject else None
        if frozen:
            for p in g.parameters():
                p.requires_grad_(False)
        pred = g.finish(feats, zero_noise=zero_noise, noise=nz)
        w = weights(B, K)
        (pred * w).sum().backward()
        torch.cuda.synchronize()
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in g.named_parameters()}
        return dict(pred=pred.detach(), dfeats=feats.grad, grads=grads, log=list(rng.log), g=g, feats=feats, w=w, nz=nz, kind=kind,
                    fusable=bool(taken), out_scale=out_scale, seed=SEED)
    finally:
        ops.GHEAD, ops.ghead = old, real


def check_vs_float64(r, zero_noise=False, wide=False):
    """Project bounds; wide (K = 32): the larger of them and 4 x the float32 restatement's own error against float64."""
    p64, dx64, g64 = ref(r, zero_noise)
    tol_p, tol_g = {}, {}
    if wide:
        p32, dx32, g32 = ref(r, zero_noise, torch.float32)
        def t(a32, a64, proj):
            d, scale = rel_err(a32, a64)
            return max(proj, 4.0 * d / scale)
        tol_p["pred"] = t(p32, p64, 2e-6)
        tol_g["d feats"] = t(dx32, dx64, 5e-6)
        for k in g64:
            if k.startswith(HEAD_KEYS) and g64[k] is not None:
                tol_g[k] = t(g32[k], g64[k], 5e-6)
    worst = [0.0]
    close(r["pred"], p64, tol_p.get("pred", 2e-6), "pred", worst)
    close(r["dfeats"], dx64, tol_g.get("d feats", 5e-6), "d feats", worst)
    n = 0
    for k, g in r["grads"].items():
        if k.startswith(HEAD_KEYS):
            close(g, g64[k], tol_g.get(k, 5e-6), k, worst)
            n += 1
    assert n == (6 if r["kind"] == "abmil" else 4)
    print(f"  worst ratio {worst[0]:.3f} (bounds in force: pred {tol_p.get('pred', 2e-6):.2e}, largest gradient bound "
          f"{max(list(tol_g.values()) + [5e-6]):.2e})")
    return worst[0]


SHAPES = [(1, 3), (3, 5), (32, 2), (3, 32), (32, 32)]


@pytest.mark.parametrize("B,K", SHAPES, ids=[f"B{b}-K{k}" for b, k in SHAPES])
@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_head_vs_float64_with_the_kernels_own_masks_and_noise(poison, kind, B, K):  # noqa: F811
    r = run(kind, B, K, True)
    assert r["fusable"]
    assert [e[0] for e in r["log"]] == (["abmil_rho"] if kind == "abmil" else []) + ["gen_mlp0.2", "noise"]
    assert tuple(r["pred"].shape) == (B, K)
    print(f"{kind} B={B} K={K}")
    check_vs_float64(r, wide=K == 32)


@pytest.mark.parametrize("kind", ["abmil", "patch"])
@pytest.mark.parametrize("variant", ["train", "eval", "zero_noise", "inject", "no_noise"])
def test_fused_head_equals_the_layer_by_layer_path(poison, kind, variant):  # noqa: F811
    kw = dict(train=variant != "eval", zero_noise=variant == "zero_noise", inject=variant == "inject",
              noise=(0, 0) if variant == "no_noise" else (0, 1))
    a, b = run(kind, 8, 4, True, **kw), run(kind, 8, 4, False, **kw)
    assert a["fusable"] and not b["fusable"]
    assert a["log"] == b["log"]                   # same sites: order, tag, id, shape and rate
    if variant == "train":
        assert [e[0] for e in a["log"]] == (["abmil_rho"] if kind == "abmil" else []) + ["gen_mlp0.2", "noise"]
    close(a["pred"], b["pred"], 2e-6, "pred")
    close(a["dfeats"], b["dfeats"], 5e-6, "d feats")
    for k in a["grads"]:
        if k.startswith(HEAD_KEYS):
            assert (a["grads"][k] is None) == (b["grads"][k] is None), k
            if a["grads"][k] is not None:
                close(a["grads"][k], b["grads"][k], 5e-6, k)


def test_fused_head_with_frozen_parameters_hands_back_the_input_gradient_only(poison):  # noqa: F811
    a, b = run("abmil", 4, 4, True, frozen=True), run("abmil", 4, 4, False, frozen=True)
    assert a["fusable"]
    close(a["pred"], b["pred"], 2e-6, "pred")
    close(a["dfeats"], b["dfeats"], 5e-6, "d feats")
    assert float(a["dfeats"].abs().max()) > 0.0
    assert all(g is None or float(g.abs().max()) == 0.0 for g in a["grads"].values())


def test_fused_head_without_an_output_scale(poison):  # noqa: F811
    """out_act = 0 (out_scale 'none'): the identity, per element."""
    r = run("abmil", 5, 3, True, out_scale="none")
    assert r["fusable"]
    check_vs_float64(r)


@pytest.mark.parametrize("kind", ["abmil", "patch"])
def test_two_identical_calls_give_identical_bits(poison, kind):  # noqa: F811
    a, b = run(kind, 7, 5, True), run(kind, 7, 5, True)
    assert torch.equal(a["pred"], b["pred"]) and torch.equal(a["dfeats"], b["dfeats"])
    for k in a["grads"]:
        assert (a["grads"][k] is None) == (b["grads"][k] is None)
        if a["grads"][k] is not None:
            assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", ["abmil", "patch"])
def test_a_one_row_head_through_the_wide_entry(poison, monkeypatch, kind, B):  # noqa: F811
    """K = 1 is inside advmil_gheadk_t's limits, but ops routes one-row heads to advmil_ghead_*: here ops._ghead_entry loses that route, so
    the wide form of the shared source runs at K = 1 -- against float64 at the project bounds, and against the same head through the width-1
    entry at the same bounds (the two sum in different orders: no exact equality)."""
    from advmil_amd import _lib
    narrow = run(kind, B, 1, True)
    taken = []

    def wide_entry(spec):
        L, K = _lib.lib(), spec.W1.shape[0]
        taken.append(K)
        return (_lib.GHeadK, (lambda B, d0, d1, d2: L.advmil_gheadk_workspace_bytes(B, d0, d1, d2, K)), L.advmil_gheadk_fwd,
                L.advmil_gheadk_bwd, "gheadk")
    monkeypatch.setattr(ops, "_ghead_entry", wide_entry)
    r = run(kind, B, 1, True)
    assert narrow["fusable"] and r["fusable"] and taken == [1, 1]          # (forward and backward)
    assert r["log"] == narrow["log"] and tuple(r["pred"].shape) == (B, 1)
    print(f"{kind} B={B} K=1 through advmil_gheadk_*")
    check_vs_float64(r)
    close(r["pred"], narrow["pred"], 2e-6, "pred vs width-1 entry")
    close(r["dfeats"], narrow["dfeats"], 5e-6, "d feats vs width-1 entry")
    for k in r["grads"]:
        if k.startswith(HEAD_KEYS):
            close(r["grads"][k], narrow["grads"][k], 5e-6, k + " vs width-1 entry")


def test_pred_out_buffer_is_written_in_place_only_without_grad(poison):  # noqa: F811
    B, K = 6, 4
    g = build("abmil", K).eval()
    FlatAdam(g, lr=1e-4).zero_grad()
    rng = ops.DeviceRng(DEV, seed=SEED)
    for m in g.modules():
        m.rng = rng
    feats = torch.randn(B, 384, generator=torch.Generator().manual_seed(5)).to(DEV)
    buf = torch.full((2 * B, K), -7.0, device=DEV)
    with torch.no_grad():
        want = g.finish(feats, zero_noise=True).clone()
        out = g.finish(feats, zero_noise=True, pred_out=buf[:B])
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf[:B], want) and bool((buf[B:] == -7.0).all())
    with torch.no_grad():                         # a buffer of another shape is not taken
        out = g.finish(feats, zero_noise=True, pred_out=buf[:B, :1])
    assert out.data_ptr() != buf.data_ptr() and torch.equal(out, want)
    buf.fill_(-7.0)
    out = g.finish(feats.clone().requires_grad_(True), zero_noise=True, pred_out=buf[:B])      # under grad: ignored
    assert out.data_ptr() != buf.data_ptr() and out.requires_grad and torch.equal(out.detach(), want) and bool((buf == -7.0).all())


def disc_cfg(kind, bins, **over):
    from advmil_amd.config import default_cfg
    cfg = dict(task="disc_gansurv", time_format="quantile", time_bins=bins, gen_dims=f"384-{bins}", disc_nety_in_dim=bins, bcb_mode=kind)
    cfg.update(over)
    return default_cfg(**cfg)


@pytest.mark.parametrize("bins", [4, 32])
def test_the_handlers_generator_takes_the_fused_head(bins):
    from advmil_amd.model import MyHandler
    h = MyHandler(disc_cfg("abmil", bins), device=DEV)
    h.netG.train()
    spec = h.netG._head_spec(torch.randn(16, 384, device=DEV), False, None)
    assert spec is not None and spec.W1.shape[0] == bins


def test_a_33_wide_head_runs_layer_by_layer_and_is_still_correct(poison):  # noqa: F811
    r = run("abmil", 3, 33, True)                 # (fused path ALLOWED: the head itself declines)
    assert not r["fusable"]
    assert [e[0] for e in r["log"]] == ["abmil_rho", "gen_mlp0.2", "noise"]
    check_vs_float64(r, wide=True)


def test_fused_head_is_what_the_discrete_step_runs(poison, monkeypatch):  # noqa: F811
    """One disc_gansurv step of MyHandler (4 ragged bags, the shipped dropout, two generator updates): the fused head runs in both phases --
    once in the D phase (no grad, generator in eval mode) and once in each of the G phase's two forwards (training mode, graph kept); a
    silent fall-back to the layer-by-layer path would pass every parity test."""
    from advmil_amd.model import MyHandler
    from tests import helpers as H

    def bin_label(i):
        y = synth.label(H.DATA_SEED, i).copy()
        y[0, 0] = np.floor(4 * y[0, 0])
        return H.T(y)
    calls = []
    real = ops.ghead

    def counted(x, spec, pred_out=None):
        calls.append((torch.is_grad_enabled(), tuple(x.shape), int(spec.W1.shape[0])))
        return real(x, spec, pred_out)
    monkeypatch.setattr(ops, "ghead", counted)
    lens = (256, 512, 128, 64)
    h = MyHandler(disc_cfg("abmil", 4, bp_every_batch=len(lens), gen_updates=2), device=DEV)
    loader = [(torch.tensor([[i]], dtype=torch.int), [H.bag(300 + i, 512)[:, :n].contiguous(), torch.zeros(1, 1)], bin_label(i))
              for i, n in enumerate(lens)]
    cl = h._train_each_epoch(loader, "train")
    assert calls == [(False, (4, 384), 4), (True, (4, 384), 4), (True, (4, 384), 4)], calls
    assert tuple(cl["y_hat"].shape) == (4, 4) and bool(torch.isfinite(cl["y_hat"]).all())
    assert h.step_graph_stats["captured"] == 0 and h.step_graph_stats["replayed"] == 0
