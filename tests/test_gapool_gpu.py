"""GPU: the gated-attention region embedding (disc_netx_backbone: gapool).
 * advmil_gapool16_fwd / _bwd (csrc/gapool16.hip) against the float64 restatement tests/gapool_ref.py over every shape at which the
   kernels take another path, three score regimes, both allocation-poisoning patterns; bounds of tests/test_row_walks_gpu.py::BOUND;
 * the layer (GAPoolPatchEmbedding.embed_rows) forward and every parameter gradient against the restatement, parameters inside and
   outside a FlatAdam arena, dup = 2 against the layer stacked twice;
 * the discriminators and two passes of the training step against the reference's own run (tests/golden/gapool_v1.npz);
 * the epoch loop: replayed step graphs against the eager loop bit for bit, batched evaluation against per-bag evaluation."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from advmil_amd import synth
from advmil_amd.config import default_cfg
from tests import gapool_ref as R
from tests import helpers as H
from tests.poison import poison  # noqa: F401  (fixture: both poison patterns)
from tests.test_row_walks_gpu import BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5                       # tests/test_parity_gpu.py (G3, G4) and tests/test_disc_task_gpu.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = "net_pair_one.embedding."
KB = dict(A=BOUND["A"], emb=BOUND["pooled"], ds=BOUND["grad"], dz=BOUND["grad"])
WORST = [0.0, None]


@pytest.fixture(scope="module")
def gp():
    return np.load(os.path.join(ROOT, "tests", "golden", "gapool_v1.npz"))


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import _lib
    from advmil_amd import ops as _ops
    _lib.lib()
    return _ops


def relerr(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def judge(case, err, bound):
    """Print every figure and the worst error over its bound so far, then assert."""
    for k in err:
        if err[k] / bound[k] > WORST[0]:
            WORST[:] = [err[k] / bound[k], f"{case}/{k}"]
    print(f"[gapool16] {case}: " + " ".join(f"{k} {err[k]:.2e}/{bound[k]:.1e}" for k in err) + f"   worst so far {WORST[0]:.3f} ({WORST[1]})")
    for k in err:
        assert err[k] < bound[k], (case, k, err[k], bound[k])


# ------------------------------------------------------------------------------------------------------------------------------
# the two kernels
# ------------------------------------------------------------------------------------------------------------------------------
KCase = SimpleNamespace
# R = 5 / 17: one region more than a backward / forward workgroup's share (4 / 16; a wave's share is 1 / 4); R = 6000: past the grid cap
# of either kernel (4096 regions per trip on 256 compute units): a second, ragged trip of the grid-stride loop (49 MB of z).
K_CASES = ([KCase(R=3, d=d, pad=0, dup=1, acc=0, regime="unit") for d in (8, 128, 132, 384)] +
           [KCase(R=1, d=128, pad=0, dup=1, acc=0, regime="unit"), KCase(R=1, d=384, pad=0, dup=2, acc=1, regime="unit"),
            KCase(R=5, d=128, pad=0, dup=2, acc=1, regime="unit"), KCase(R=5, d=8, pad=0, dup=1, acc=0, regime="unit"),
            KCase(R=17, d=384, pad=0, dup=2, acc=0, regime="unit"), KCase(R=17, d=132, pad=4, dup=1, acc=1, regime="unit"),
            KCase(R=17, d=128, pad=0, dup=1, acc=0, regime="unit"), KCase(R=6000, d=128, pad=0, dup=1, acc=0, regime="unit")] +
           [KCase(R=5, d=d, pad=0, dup=1, acc=0, regime=g) for d in (8, 128, 384) for g in ("far", "equal")])


def kid(c):
    return f"R{c.R}-d{c.d}-{c.regime}" + (f"-pad{c.pad}" if c.pad else "") + ("-dup" if c.dup == 2 else "") + ("-acc" if c.acc else "")


_INPUTS = {}


def k_inputs(c):
    """Host inputs and the float64 reference of a case, made once and never written."""
    key = kid(c)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * c.R + c.d + c.dup)
        N = 16 * c.R
        z = torch.randn(N, c.d, generator=g)
        if c.regime == "unit":
            s = torch.randn(N, generator=g)
        elif c.regime == "equal":
            s = torch.full((N,), 0.75)
        else:                                         # +-3e4 with one dominant row per region
            s = torch.where(torch.rand(N, generator=g) < 0.5, torch.tensor(-3e4), torch.tensor(-2.9e4))
            dom = torch.randint(0, 16, (c.R,), generator=g)
            s[torch.arange(c.R) * 16 + dom] = 3e4
        demb = torch.randn(c.dup * c.R, c.d, generator=g)
        dz0 = torch.randn(N, c.d, generator=g)
        emb, A = R.pool_fwd(s.numpy(), z.numpy(), c.dup)
        ds, dz = R.pool_bwd(demb.numpy(), A, z.numpy(), c.dup)
        _INPUTS[key] = dict(s=s, z=z, demb=demb, dz0=dz0, emb=emb, A=A, ds=ds, dz=dz + (dz0.double().numpy() if c.acc else 0.0))
    return _INPUTS[key]


def pitched(x, pad):
    if not pad:
        return x.to(DEV)
    wide = torch.full((x.shape[0], x.shape[1] + pad), 77.0)
    wide[:, :x.shape[1]] = x
    v = wide.to(DEV)[:, :x.shape[1]]
    assert v.stride(0) == x.shape[1] + pad and v.data_ptr() % 16 == 0
    return v


def launch(c, inp):
    from advmil_amd import _lib
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N = 16 * c.R
    s, z, demb = inp["s"].to(DEV), pitched(inp["z"], c.pad), inp["demb"].to(DEV)
    A, emb = torch.empty(N, device=DEV), torch.empty(c.dup * c.R, c.d, device=DEV)
    ds, dz = torch.empty(N, device=DEV), (inp["dz0"].to(DEV) if c.acc else torch.empty(N, c.d, device=DEV))
    assert L.advmil_gapool16_fwd(p(s), p(z), z.stride(0), N, c.d, p(A), p(emb), c.dup, st) == 0
    assert L.advmil_gapool16_bwd(p(demb), p(A), p(z), z.stride(0), N, c.d, c.dup, p(ds), p(dz), c.acc, st) == 0
    torch.cuda.synchronize()
    return dict(A=A, emb=emb, ds=ds, dz=dz)


@pytest.mark.parametrize("c", K_CASES, ids=kid)
def test_pooling_kernels_vs_restatement(poison, c):  # noqa: F811
    inp = k_inputs(c)
    got = launch(c, inp)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), k
    judge(kid(c), {k: relerr(got[k], inp[k]) for k in KB}, KB)
    if c.dup == 2:
        assert torch.equal(got["emb"][:c.R], got["emb"][c.R:])
    A = got["A"].cpu()
    if c.regime == "far":                             # weights exactly 0 or 1, one 1 per region, the pooled row IS the dominant row
        assert bool(((A == 0) | (A == 1)).all()) and bool((A.reshape(-1, 16).sum(1) == 1).all())
        dom = A.reshape(-1, 16).argmax(1) + 16 * torch.arange(c.R)
        assert torch.equal(got["emb"].cpu()[:c.R], inp["z"][dom])
        assert not bool(got["ds"].any())
    if c.regime == "equal":
        assert bool((A == 1.0 / 16).all())


def test_pooling_kernels_are_deterministic_and_carry_nan(ops, poison):  # noqa: F811
    """The same bits from the op twice; a NaN score poisons its region's weights and pooled row and nothing else, a NaN in z its column."""
    c = KCase(R=17, d=128, pad=0, dup=1, acc=0, regime="unit")
    inp = k_inputs(c)
    a, b = launch(c, inp), launch(c, inp)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    s, z = inp["s"].clone(), inp["z"].clone()
    s[16 * 3 + 5] = float("nan")
    z[16 * 9 + 2, 7] = float("nan")
    emb, A = ops.gapool16(s.to(DEV), z.to(DEV))
    bad = torch.isnan(emb).cpu()
    want = torch.zeros(17, 128, dtype=torch.bool)
    want[3, :] = True
    want[9, 7] = True
    assert torch.equal(bad, want)
    assert bool(torch.isnan(A[48:64]).all()) and not bool(torch.isnan(A[:48]).any()) and not bool(torch.isnan(A[64:]).any())


def test_op_backward_and_argument_errors(ops, poison):  # noqa: F811
    from advmil_amd import _lib
    c = KCase(R=5, d=132, pad=0, dup=2, acc=0, regime="unit")
    inp = k_inputs(c)
    s, z = inp["s"].to(DEV).requires_grad_(True), inp["z"].to(DEV).requires_grad_(True)
    emb, A = ops.gapool16(s, z, dup=2)
    assert not A.requires_grad
    emb.backward(inp["demb"].to(DEV))
    judge("op-" + kid(c), dict(A=relerr(A, inp["A"]), emb=relerr(emb, inp["emb"]), ds=relerr(s.grad, inp["ds"]), dz=relerr(z.grad, inp["dz"])), KB)
    with pytest.raises(_lib.AdvmilHipError, match="invalid argument"):
        ops.gapool16(torch.zeros(24, device=DEV), torch.zeros(24, 128, device=DEV))
    with pytest.raises(_lib.AdvmilHipError, match="invalid argument"):
        ops.gapool16(torch.zeros(16, device=DEV), torch.zeros(16, 130, device=DEV))
    with pytest.raises(ValueError):
        ops.gapool16(torch.zeros(16, device=DEV), torch.zeros(16, 128, device=DEV), dup=3)


# ------------------------------------------------------------------------------------------------------------------------------
# the layer
# ------------------------------------------------------------------------------------------------------------------------------
# bag index per (d, N): picked on the host so that every pre-ReLU value of the float64 forward is at least LN_MARGIN away from 0. The
# device's pre-ReLU values differ from the float64 ones by the fp32 round-off of a 1024-term dot product of |x w| <= 0.4 and of the
# normalisation: about sqrt(1024) 2^-24 0.4 = 1e-6; the margin is 20 times that, so no ReLU mask can differ and no entry is left out.
LAYER_BAG = {(128, 16): 20, (128, 80): 20, (384, 16): 20, (384, 80): 22}
LN_MARGIN = 2e-5
LB = dict(emb=BOUND["pooled"], A=BOUND["A"], grad=BOUND["grad"])


def layer_params(d):
    return {k: synth.param(H.PARAM_SEED, PREFIX + k, s) for k, s in R.shapes(1024, d).items()}


def build_layer(d, P=None, fc2_zero=False):
    from advmil_amd.model.backbone_utils import GAPoolPatchEmbedding
    m = GAPoolPatchEmbedding(1024, d, 4, False, 1)
    P = dict(layer_params(d) if P is None else P)
    if fc2_zero:
        P["pool.fc2.weight"] = np.zeros_like(P["pool.fc2.weight"])
    m.load_state_dict({k: H.T(v) for k, v in P.items()}, strict=True)
    return m.to(DEV), P


_LREF = {}


def layer_ref(d, N):
    if (d, N) not in _LREF:
        P = layer_params(d)
        x = synth.bag(H.DATA_SEED, LAYER_BAG[(d, N)], N)[0]
        f = R.layer_fwd(P, x)
        w1 = synth.normal(synth.stream_key(3, f"gapool_w1:{d}:{N}"), (N // 16) * d).reshape(N // 16, d)
        w2 = synth.normal(synth.stream_key(3, f"gapool_w2:{d}:{N}"), (N // 16) * d).reshape(N // 16, d)
        _LREF[(d, N)] = dict(P=P, x=x, f=f, w1=w1, w2=w2, G1=R.layer_bwd(P, f, w1), G12=R.layer_bwd(P, f, np.concatenate([w1, w2]), dup=2))
    return _LREF[(d, N)]


def grad_errors(m, G, scale=1.0):
    """Largest error of a parameter gradient, relative to that gradient's largest entry. pool.fc2.bias: its gradient is sum ds, and the ds
    of every region sum to exactly 0 (a softmax's gradient), so it is measured against its uncancelled magnitude sum |ds| instead."""
    named = dict(m.named_parameters())
    assert set(named) == set(R.KEYS)
    err = {k: relerr(named[k].grad, scale * G[k]) for k in R.KEYS if k != "pool.fc2.bias"}
    err["pool.fc2.bias"] = float(abs(float(named["pool.fc2.bias"].grad) - scale * float(G["pool.fc2.bias"][0])) / (scale * G["ds_mag"]))
    print("    " + " ".join(f"{k} {v:.1e}" for k, v in err.items()))
    return max(err.values())


@pytest.mark.parametrize("arena", [False, True], ids=["plain", "arena"])
@pytest.mark.parametrize("d,N", sorted(LAYER_BAG))
def test_layer_forward_and_gradients_vs_restatement(ops, poison, d, N, arena):  # noqa: F811
    ref = layer_ref(d, N)
    margin = R.relu_margin(ref["f"])
    print(f"[gapool layer] d={d} N={N}: pre-ReLU margin {margin:.2e} (share of entries left out: 0)")
    assert margin > LN_MARGIN
    m, _ = build_layer(d)
    opt = None
    if arena:
        from advmil_amd.optim import FlatAdam
        opt = FlatAdam(m, lr=1e-3)
        opt.zero_grad()
    x = H.T(ref["x"], DEV)
    passes = 2 if arena else 1                        # the arena's slots take the second backward on top of the first
    for _ in range(passes):
        emb = m.embed_rows(x)
        assert emb.shape == (N // 16, d)
        emb.backward(H.T(ref["w1"], DEV))
    if arena:
        for p in m.parameters():
            assert p.grad.untyped_storage().data_ptr() == opt.flat_grad.untyped_storage().data_ptr()
    judge(f"layer-d{d}-N{N}-{'arena' if arena else 'plain'}",
          dict(emb=relerr(emb, ref["f"]["emb"]), A=relerr(m.last_attention, ref["f"]["A"]), grad=grad_errors(m, ref["G1"], float(passes))), LB)
    got3 = m(x.unsqueeze(0))
    assert got3.shape == (1, N // 16, d) and torch.equal(got3[0], emb)
    with pytest.raises(ValueError, match="batch_size 1"):
        m(torch.zeros(2, 16, 1024, device=DEV))


@pytest.mark.parametrize("d,N", [(128, 80), (384, 16)])
def test_layer_dup2_is_the_layer_stacked_twice(ops, poison, d, N):  # noqa: F811
    ref = layer_ref(d, N)
    m, _ = build_layer(d)
    x = H.T(ref["x"], DEV)
    with torch.no_grad():
        one = m.embed_rows(x)
    two = m.embed_rows(x, 2)
    assert two.shape == (2 * (N // 16), d) and torch.equal(two, torch.cat([one, one]))
    two.backward(torch.cat([H.T(ref["w1"], DEV), H.T(ref["w2"], DEV)]))
    judge(f"layer-dup2-d{d}-N{N}", dict(emb=relerr(two, np.concatenate([ref["f"]["emb"]] * 2)), grad=grad_errors(m, ref["G12"])),
          dict(emb=LB["emb"], grad=LB["grad"]))


def test_zero_score_weights_make_the_layer_the_mean_pool(ops, poison):  # noqa: F811
    """pool.fc2.weight = 0: every score is the bias, every weight 1/16 -> the embedding is ops.ln_relu_mean16 of the same y (which sums in
    another order: 1e-6 of the largest entry)."""
    d, N = 128, 80
    m, _ = build_layer(d, fc2_zero=True)
    x = H.T(synth.bag(H.DATA_SEED, 20, N)[0], DEV)
    with torch.no_grad():
        emb = m.embed_rows(x)
        y = ops.linear_act(x, m.conv.weight, m.conv.bias, "none")
        avg = ops.ln_relu_mean16(y, m.norm.weight, m.norm.bias, m.norm.eps)
    assert bool((m.last_attention == 1.0 / 16).all())
    err = float((emb - avg).abs().max() / avg.abs().max())
    print(f"[gapool layer] zero scorer vs mean16: {err:.2e}/1.0e-06")
    assert err <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------------
# parity with the reference's own run
# ------------------------------------------------------------------------------------------------------------------------------
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


def build_disc(disc_type="prj", iprd="instance", prj="x"):
    from advmil_amd.model import Discriminator, PrjDiscriminator
    ax = SimpleNamespace(in_dim=1024, out_dim=128, ksize=1, backbone="gapool", dropout=0.25)
    ay = SimpleNamespace(in_dim=1, hid_dims=[64, 128], norm=False, dropout=0.0)
    d = PrjDiscriminator(ax, ay, prj_path=prj, inner_product=iprd) if disc_type == "prj" else Discriminator(ax, ay)
    return d.to(DEV)


@pytest.mark.parametrize("disc_type,iprd,prj", [("prj", "instance", "x"), ("prj", "bag", "x"), ("cat", "bag", None)])
def test_discriminators_vs_reference(gp, poison, disc_type, iprd, prj):  # noqa: F811
    d = build_disc(disc_type, iprd, prj).eval()
    load_synth(d, "D-prj:" if disc_type == "prj" else "D-cat:")
    assert sorted(d.state_dict()) == [str(k) for k in gp[f"Dg_{disc_type}-{iprd}-{prj}_keys"]]
    t = torch.tensor([[0.37]], device=DEV)
    for N in (64, 512):
        with torch.no_grad():
            f = d(H.bag(3, N, DEV), t)
        print(f"[gapool D] {disc_type}-{iprd}-{prj} N={N}:", close(f, gp[f"Dg_{disc_type}-{iprd}-{prj}_N{N}_f"]))


STEP_LENS, STEP_EVENTS = (32, 64, 16, 48), (1.0, 0.0, 1.0, 1.0)


def step_label(i):
    y = synth.label(H.DATA_SEED, i).copy()
    y[0, 1] = STEP_EVENTS[i]
    return H.T(y)


@pytest.mark.parametrize("kind,gemm_mode", [("abmil", "exact"), ("abmil", "bf16x3"), ("patch", "exact")])
def test_two_passes_of_the_step_vs_reference(gp, ops, poison, kind, gemm_mode):  # noqa: F811
    """The reference's own _train_each_epoch twice over 4 ragged bags (each pass one _update_disc and one _update_gen; dropout p = 0,
    injected noise, disc_netx_backbone: gapool) vs ours; bounds of tests/test_disc_task_gpu.py::two_steps_vs_reference."""
    from advmil_amd.model import MyHandler
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(gemm_mode)
    try:
        h = MyHandler(default_cfg(bcb_mode=kind, bp_every_batch=4, disc_netx_backbone="gapool"), device=DEV)
        assert type(h.netD.net_pair_one.embedding).__name__ == "GAPoolPatchEmbedding"
        PG0, PD0 = load_synth(h.netG, f"G-{kind}:"), load_synth(h.netD, "D-prj:")
        zero_dropout(h.netG); zero_dropout(h.netD)
        nb, name = len(STEP_LENS), f"S_{kind}"
        h.patient_id["label_visible"] = h.patient_id["train"] = [str(i) for i in range(nb)]
        loader = [(torch.tensor([[i]], dtype=torch.int), [H.bag(i, STEP_LENS[i]), torch.zeros(1, 1)], step_label(i)) for i in range(nb)]
        ref = gp[f"{name}_logs"]
        for ep in range(2):
            h.noise_hook = lambda ph, i, ep=ep: [H.noise_tensor(f"GP{ep}{ph}:{kind}", i, 192, DEV)]
            cl = h._train_each_epoch(loader, "train")
            logs = h.pop_logs()
            assert len(logs) == 2
            d, g = logs
            got = [d["train_batch/netD/Loss_D"], d["train_batch/netD/D_real"], d["train_batch/netD/D_fake"],
                   g["train_batch/netG/Loss_G_fake"], g["train_batch/netG/Loss_G_time"], g["train_batch/netG/Loss_G_total"],
                   g["train_batch/netG/D_fake_avg"]]
            print(name, gemm_mode, "pass", ep, "logs", got, "ref", ref[ep].tolist())
            close(torch.tensor(got, dtype=torch.float64), ref[ep])
            close(cl["y_hat"], gp[f"{name}_y_hat"][ep])
            close(cl["f_fake"], gp[f"{name}_f_fake"][ep])
            close(cl["y"], gp[f"{name}_y"], 0.0)
        for t_, net, P0 in (("G", h.netG, PG0), ("D", h.netD, PD0)):
            sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
            keys = [str(k) for k in gp[f"{name}_keys{t_}"]]
            assert sorted(sd) == keys
            dn = np.array([float((sd[k].double() - P0[k].double()).norm()) for k in keys])
            ref_dn = gp[f"{name}_d{t_}_stats"][:, 1]
            assert np.all(np.abs(dn - ref_dn) <= 5e-3 * ref_dn + 5e-5), float(np.abs(dn - ref_dn).max())
        gk = [str(k) for k in gp[f"{name}_gradG2_keys"]]
        named = dict(h.netG.named_parameters())
        gn = np.array([float((named[k].grad.double() + 1e-5 * torch.sign(named[k].detach().double())).norm()) for k in gk])
        assert np.allclose(gn, gp[f"{name}_gradG2_norm"], rtol=5e-3, atol=5e-6), np.abs(gn - gp[f"{name}_gradG2_norm"]).max()
    finally:
        ops.set_gemm_mode(prev)


# ------------------------------------------------------------------------------------------------------------------------------
# the epoch loop
# ------------------------------------------------------------------------------------------------------------------------------
_LOOP = []


def _loop_loader():
    """24 ragged pinned host bags (the first 6 step batches of tests/test_step_graphs_gpu.py), made once."""
    from tests.test_step_graphs_gpu import EVENTS, LENS
    if _LOOP:
        return _LOOP
    loader, i = _LOOP, 0
    for bl, be in zip(LENS[:6], EVENTS[:6]):
        for m, e in zip(bl, be):
            x = H.T(synth.bag(H.DATA_SEED, 400 + i, m)).pin_memory()
            loader.append((torch.tensor([[i]], dtype=torch.int), [x, torch.zeros(1, 1)], torch.tensor([[0.2 + 0.013 * i, float(e)]])))
            i += 1
    return loader


def _epochs(loader, graphs):
    from advmil_amd.model import MyHandler
    h = MyHandler(default_cfg(bcb_mode="abmil", bp_every_batch=4, gemm_mode="bf16x3", step_graphs=1, step_graphs_max=24 if graphs else 0,
                              bag_cache_gb=2, disc_netx_backbone="gapool"), device=DEV)
    load_synth(h.netG, "G-abmil:"); load_synth(h.netD, "D-prj:")
    h.optimizerG.refresh_planes(); h.optimizerD.refresh_planes()
    h.rng.reset(77)
    n = len(loader)
    h.patient_id.update({"train": [f"t{i}" for i in range(n)], "label_visible": [f"t{i}" for i in range(n)]})
    cls = [h._train_each_epoch(loader, "train", "wlabel") for _ in range(2)]
    torch.cuda.synchronize()
    return h, cls, h.pop_logs()


def test_replayed_step_graphs_equal_the_eager_loop(ops, poison):  # noqa: F811
    """An abmil handler with the gapool discriminator on ragged host bags, shipped dropout on: the steps replayed from HIP graphs leave
    the same bits as the same epochs with no graph ever captured (tests/test_step_graphs_gpu.py, its bag sizes)."""
    prev = ops.get_gemm_mode()
    try:
        loader = _loop_loader()
        hg, cg, lg = _epochs(loader, True)
        he, ce, le = _epochs(loader, False)
    finally:
        ops.set_gemm_mode(prev)
    print("[gapool loop]", hg.step_graph_stats, he.step_graph_stats)
    assert hg.step_graph_stats["replayed"] >= 2 and hg.step_graph_stats["captured"] >= 2
    assert he.step_graph_stats == {"replayed": 0, "captured": 0, "eager": 12}, he.step_graph_stats
    for a, b in zip(cg, ce):
        for k in ("y", "y_hat", "f_fake"):
            assert torch.equal(a[k], b[k]), k
        assert bool(torch.isfinite(a["y_hat"]).all()) and bool(torch.isfinite(a["f_fake"]).all())
    assert len(lg) == len(le) == 2 * 6 * 2
    for a, b in zip(lg, le):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], (k, a[k], b[k])
    assert torch.equal(hg.optimizerG.flat_param, he.optimizerG.flat_param) and torch.equal(hg.optimizerD.flat_param, he.optimizerD.flat_param)


def test_batched_evaluation_equals_per_bag_evaluation(poison):  # noqa: F811
    from advmil_amd.model import MyHandler
    from tests.test_parity_gpu import build_generator
    g, d = build_generator("abmil"), build_disc()
    load_synth(g, "G-abmil:"); load_synth(d, "D-prj:")
    lens = (256, 128, 512, 64, 192, 384, 320)
    items = [(torch.tensor([[i]], dtype=torch.int), [H.bag(700 + i, n), torch.zeros(1, 1)], H.label(i)) for i, n in enumerate(lens)]
    one = MyHandler.test_model(g, d, "abmil", items, test_zero_noise=True, batch_bags=1)
    bat = MyHandler.test_model(g, d, "abmil", items, test_zero_noise=True, batch_bags=4)
    for k in ("y_hat", "f_fake"):
        assert one[k].shape == bat[k].shape and bool(torch.isfinite(one[k]).all())
        err = float((one[k].double() - bat[k].double()).abs().max())
        print(f"[gapool eval] {k}: batched vs per bag {err:.2e}/2.0e-06")
        assert err <= 2e-6, k
    assert torch.equal(one["y"], bat["y"]) and bat["idx"].reshape(-1).tolist() == list(range(len(lens)))
