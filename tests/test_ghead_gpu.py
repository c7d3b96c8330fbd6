"""The generator's bag-level head as two launches each way (advmil_ghead_fwd / advmil_ghead_bwd, csrc/ghead.hip; reference
model/GANSurv.py:13-46 behind the backbone's pooling, model/backbone.py:66-70 rho): against the float64 restatement of tests/ghead_ref.py
with the kernel's own dropout masks / noise regenerated on the host, and against the layer-by-layer path it replaces (same call sites, same
draws)."""
import pytest
import torch

from advmil_amd import ops, synth
from advmil_amd.optim import FlatAdam
from tests.ghead_ref import HEAD_KEYS, close, ref
from tests.test_parity_gpu import DEV, build_generator, load_synth

pytestmark = pytest.mark.gpu


def _run(kind, B, fused, train=True, zero_noise=False, inject=False, noise=(0, 1), seed=11, frozen=False):
    old = ops.GHEAD
    ops.GHEAD = fused
    try:
        g = build_generator(kind)
        if list(noise) != [0, 1]:
            from types import SimpleNamespace
            from advmil_amd.model import Generator, load_backbone
            g = Generator(384, 1, load_backbone(kind, [1024, 384, 384]), SimpleNamespace(noise=list(noise), hops=1, noise_dist="uniform"),
                          False, 0.6, "sigmoid").to(DEV)
            sd = {k: torch.from_numpy(synth.param(7, "Gx:" + k, tuple(v.shape))).to(DEV) for k, v in g.state_dict().items()}
            g.load_state_dict(sd)
        else:
            load_synth(g, f"G-{kind}:")
        g.train(train)
        opt = FlatAdam(g, lr=1e-4)
        opt.zero_grad()
        rng = ops.DeviceRng(DEV, seed=seed)
        rng.record = True
        for m in g.modules():
            m.rng = rng
        gen = torch.Generator().manual_seed(5)
        feats = torch.randn(B, 384, generator=gen).to(DEV).requires_grad_(True)
        nz = [torch.rand(B, 192, generator=gen).to(DEV)] if inject else None
        if frozen:
            for p in g.parameters():
                p.requires_grad_(False)
        pred = g.finish(feats, zero_noise=zero_noise, noise=nz)
        w = torch.linspace(0.5, 1.5, B, device=DEV).reshape(B, 1)
        (pred * w).sum().backward()
        torch.cuda.synchronize()
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in g.named_parameters()}
        return dict(pred=pred.detach(), dfeats=feats.grad, grads=grads, log=list(rng.log), g=g, feats=feats, w=w, nz=nz, kind=kind,
                    out_scale="sigmoid", seed=seed)
    finally:
        ops.GHEAD = old


@pytest.mark.parametrize("kind", ["abmil", "patch"])
@pytest.mark.parametrize("B", [1, 3, 16, 32])
def test_fused_head_vs_float64_with_the_kernels_own_masks_and_noise(kind, B):
    r = _run(kind, B, True)
    tags = [e[0] for e in r["log"]]
    assert tags == (["abmil_rho"] if kind == "abmil" else []) + ["gen_mlp0.2", "noise"]
    pred, dx, gp = ref(r)
    close(r["pred"], pred, 2e-6, "pred")
    close(r["dfeats"], dx, 5e-6, "d feats")
    for k, g in r["grads"].items():
        if k.startswith(HEAD_KEYS):
            close(g, gp[k], 5e-6, k)


@pytest.mark.parametrize("kind", ["abmil", "patch"])
@pytest.mark.parametrize("variant", ["train", "eval", "zero_noise", "inject", "no_noise"])
def test_fused_head_equals_the_layer_by_layer_path(kind, variant):
    kw = dict(train=variant != "eval", zero_noise=variant == "zero_noise", inject=variant == "inject",
              noise=(0, 0) if variant == "no_noise" else (0, 1))
    a, b = _run(kind, 8, True, **kw), _run(kind, 8, False, **kw)
    assert [e[:1] + e[2:] for e in a["log"]] == [e[:1] + e[2:] for e in b["log"]]         # same sites, shapes and rates, in the same order
    assert [e[1] for e in a["log"]] == [e[1] for e in b["log"]]
    close(a["pred"], b["pred"], 2e-6, "pred")
    close(a["dfeats"], b["dfeats"], 5e-6, "d feats")
    for k in a["grads"]:
        if k.startswith(HEAD_KEYS):
            assert (a["grads"][k] is None) == (b["grads"][k] is None), k
            if a["grads"][k] is not None:
                close(a["grads"][k], b["grads"][k], 5e-6, k)


def test_fused_head_with_frozen_parameters_hands_back_the_input_gradient_only():
    a, b = _run("abmil", 4, True, frozen=True), _run("abmil", 4, False, frozen=True)
    close(a["pred"], b["pred"], 2e-6, "pred")
    close(a["dfeats"], b["dfeats"], 5e-6, "d feats")
    assert all(g is None or float(g.abs().max()) == 0.0 for g in a["grads"].values())


def test_fused_head_is_what_the_step_runs():
    """The shipped configuration takes the fused launches (a silent fall-back to the layer-by-layer path would pass every parity test)."""
    g = build_generator("abmil").train()
    FlatAdam(g, lr=1e-4).zero_grad()
    feats = torch.randn(16, 384, device=DEV)
    assert g._head_spec(feats, False, None) is not None
