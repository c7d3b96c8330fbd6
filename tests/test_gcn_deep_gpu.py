"""GPU: PatchGCN at full depth (num_layers > 1, edge_agg = 'latent').
 * advmil_gcn_res_fwd / _bwd (csrc/gcnres.hip) against tests/gcn_ref.py::res_block in float64, forward and backward: every width class
   of the kernel (half a wave per row up to d = 128, a wave with one / two float4 groups above), row counts around the 16-row
   workgroup, dense and as column block 1 of a [N, 3 d] buffer, p in {0, 0.1}, both accumulate switches, a non-identity rng_row, rows
   near 1e3; both allocation-poisoning patterns. Bounds: tests/test_row_walks_gpu.py::BOUND (ln_out 1e-5 for out / mean / rstd, ln_grad
   5e-5 for the gradients, max-relative); the `bigmean` case max(that, 4 e32), e32 = the same restatement in float32 on the host
   against its float64 self.
   ReLU branch flips: the input seed of every case was picked on the host (SEED_K) so that the float64 LayerNorm output's smallest
   magnitude is at least 64 * 2^-24 of its largest; the test asserts that before it launches, so no entry can take the other branch in
   float32 and none is left out of a comparison.
 * determinism, NaN containment, the op's argument errors;
 * the model at num_layers 2 and 3 against tests/gcn_ref.py::patch_gcn_deep, dropout off and on (masks rebuilt from the RNG log), at
   the tolerances of tests/test_parity_gpu.py::test_patchgcn_vs_oracle;
 * latent edges, slab against per-bag features, one G+D step through MyHandler replayed from a HIP graph against the eager step.

Measured on an MI355X when this file was written (every body prints its figures), worst error over the bound in force:
  kernels, `offset` rows   0.022  out 2.2e-7 of 1e-5 (65 x 384, column block, p = 0.1); every gradient <= 2e-7 of 5e-5
  kernels, rows near 1e3   0.010  rstd 1.0e-7 of 1e-5; out 2.3e-7, dh 1.4e-7, dgamma 1.3e-7 -- the project's own bounds held, the
                                  widened ones (out 8.7e-5, dh 6e-5, dgamma 1.5e-4 from e32 = 2.2e-5 / 1.5e-5 / 3.7e-5) never came into force
  model L = 2              pred 3.0e-8 of 2e-5; worst gradient 0.15 (eval) / 0.14 (train) of 2e-4 scale + 1e-8
  model L = 3              pred 3.0e-8; worst gradient 0.77 (eval) / 0.80 (train) of the same bound: no widening by e32 was needed
Both allocation-poisoning patterns give the same figures.
"""
import collections
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from advmil_amd import synth
from advmil_amd.config import default_cfg
from tests import gcn_ref as R
from tests import helpers as H
from tests.poison import poison  # noqa: F401  (fixture: both poison patterns)
from tests.test_parity_gpu import close, load_synth
from tests.test_row_walks_gpu import BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = [1024, 128, 128]
KB = dict(out=BOUND["ln_out"], mean=BOUND["ln_out"], rstd=BOUND["ln_out"], dh=BOUND["ln_grad"], dx=BOUND["ln_grad"],
          dgamma=BOUND["ln_grad"], dbeta=BOUND["ln_grad"])
MARGIN = 64 * 2.0 ** -24
SEED_STREAM, SID = 20231, 5
WORST = {}


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def judge(family, case, err, bound):
    """Print every figure and the family's worst error over its bound so far, then assert."""
    for k in err:
        if err[k] / bound[k] >= WORST.get(family, (0.0, None))[0]:
            WORST[family] = (err[k] / bound[k], f"{case}/{k}")
    print(f"[{family}] {case}: " + " ".join(f"{k} {err[k]:.2e}/{bound[k]:.1e}" for k in err) +
          f"   worst so far {WORST[family][0]:.3f} ({WORST[family][1]})")
    for k in err:
        assert err[k] < bound[k], (family, case, k, err[k], bound[k])


# ------------------------------------------------------------------------------------------------------------------------------
# the two kernels
# ------------------------------------------------------------------------------------------------------------------------------
KCase = collections.namedtuple("KCase", "N d block p dxacc acc rr content")
SHAPES = ((1, 4), (15, 100), (64, 128), (65, 384), (65, 512), (513, 128))
K_CASES = ([KCase(N, d, 0, 0.0, 0, 0, 0, "offset") for N, d in SHAPES] +
           [KCase(N, d, 1, 0.1, 1, 1, 0, "offset") for N, d in SHAPES] +
           [KCase(15, 100, 0, 0.1, 0, 1, 0, "offset"), KCase(15, 100, 1, 0.0, 1, 0, 0, "offset"),
            KCase(65, 384, 1, 0.0, 0, 1, 0, "offset"), KCase(65, 512, 0, 0.1, 1, 0, 0, "offset"),
            KCase(64, 128, 0, 0.1, 0, 0, 1, "offset"), KCase(513, 128, 1, 0.1, 0, 0, 1, "offset"),
            KCase(64, 128, 0, 0.0, 0, 0, 0, "bigmean"), KCase(64, 128, 1, 0.1, 1, 1, 0, "bigmean")])

# k of the input seed 31 N + d + content + 1000 k: the first k whose float64 LayerNorm output keeps MARGIN (found on the host)
SEED_K = {(1, 4, "offset"): 0, (15, 100, "offset"): 1, (64, 128, "offset"): 0, (65, 384, "offset"): 1, (65, 512, "offset"): 0,
          (513, 128, "offset"): 0, (64, 128, "bigmean"): 0}


def kid(c):
    return (f"N{c.N}-d{c.d}-{'block' if c.block else 'dense'}-p{c.p}" + ("-dxacc" if c.dxacc else "") + ("-acc" if c.acc else "") +
            ("-rr" if c.rr else "") + ("-bigmean" if c.content == "bigmean" else ""))


def res_inputs(N, d, content, k):
    """tests/test_row_walks_gpu.py::ln_inputs(..., 'offset' | 'bigmean') for h, plus the block's other operands."""
    g = torch.Generator().manual_seed(31 * N + d + {"offset": 0, "bigmean": 1}[content] + 1000 * k)
    if content == "offset":
        h = torch.randn(N, d, generator=g) * (0.5 + torch.rand(N, 1, generator=g)) + 2.0 * torch.randn(N, 1, generator=g)
    else:
        h = 1e3 + torch.randn(N, d, generator=g)
    return dict(h=h, gamma=1 + 0.1 * torch.randn(d, generator=g), beta=0.1 * torch.randn(d, generator=g), x=torch.randn(N, d, generator=g),
                dout=torch.randn(N, d, generator=g), dx0=torch.randn(N, d, generator=g))


def margin(inp):
    """smallest over largest magnitude of the float64 LayerNorm output (the ReLU's input)."""
    pre = R.layer_norm(inp["h"].double(), inp["gamma"].double(), inp["beta"].double()).abs()
    return float(pre.min() / pre.max())


def rng_rows(c):
    """A non-identity row map: row m draws at row 3 N - 1 - 2 m of the stream."""
    return 3 * c.N - 1 - 2 * torch.arange(c.N, dtype=torch.int64) if c.rr else None


def keep_mask(c):
    """The mirror's keep decisions [N, d] of a case (None at p = 0)."""
    if c.p <= 0.0:
        return None
    rr = rng_rows(c)
    rows = int(rr.max()) + 1 if rr is not None else c.N
    keep = torch.as_tensor(synth.dropout_keep(SEED_STREAM, SID, rows * c.d, c.p)).reshape(rows, c.d)
    return keep[rr] if rr is not None else keep


def restate(inp, c, dtype=torch.float64):
    h, x, gm, bt = (inp[k].detach().clone().to(dtype).requires_grad_(True) for k in ("h", "x", "gamma", "beta"))
    keep = keep_mask(c)
    scale = None if keep is None else keep.to(dtype) / torch.tensor(1.0 - c.p, dtype=dtype)
    out = R.res_block(h, x, gm, bt, scale)
    (out * inp["dout"].to(dtype)).sum().backward()
    with torch.no_grad():
        mean = h.mean(1)
        rstd = torch.rsqrt(((h - mean[:, None]) ** 2).mean(1) + 1e-5)
    r = dict(out=out.detach(), mean=mean, rstd=rstd, dh=h.grad, dx=x.grad, dgamma=gm.grad, dbeta=bt.grad)
    return {k: v.double() for k, v in r.items()}


_REFS = {}


def k_reference(c):
    """Inputs, float64 reference and (bigmean) the float32 host error of a case: made once, never written."""
    key = (c.N, c.d, c.content, c.p, c.rr)
    if key not in _REFS:
        inp = res_inputs(c.N, c.d, c.content, SEED_K[(c.N, c.d, c.content)])
        ref = restate(inp, c)
        e32 = None
        if c.content == "bigmean":
            r32 = restate(inp, c, torch.float32)
            e32 = {k: relerr(r32[k], ref[k]) for k in ref}
        _REFS[key] = (inp, ref, e32)
    return _REFS[key]


def column_block(x, block, fill=77.0):
    """x [N, d] on the device: dense, or column block 1 of a [N, 3 d] buffer (the other blocks hold `fill`)."""
    if not block:
        return x.to(DEV).contiguous(), None
    N, d = x.shape
    wide = torch.full((N, 3 * d), fill)
    wide[:, d:2 * d] = x
    wide = wide.to(DEV)
    v = wide[:, d:2 * d]
    assert v.stride(0) == 3 * d and v.data_ptr() % 16 == 0
    return v, wide


def launch(c, inp):
    from advmil_amd import _lib
    L = _lib.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, d = c.N, c.d
    h, gm, bt = (inp[k].to(DEV) for k in ("h", "gamma", "beta"))
    x, _ = column_block(inp["x"], c.block)
    dout, _ = column_block(inp["dout"], c.block)
    fresh = lambda: column_block(torch.full((N, d), -55.0), 1) if c.block else (torch.empty(N, d, device=DEV), None)   # noqa: E731
    out, out_wide = fresh()
    dx, dx_wide = column_block(inp["dx0"], c.block) if c.dxacc else fresh()
    seed = torch.tensor([SEED_STREAM], dtype=torch.int64, device=DEV) if c.p > 0 else None
    rr = rng_rows(c)
    rr = None if rr is None else rr.to(DEV)
    mean, rstd, dh = torch.empty(N, device=DEV), torch.empty(N, device=DEV), torch.empty(N, d, device=DEV)
    dg = torch.full((d,), 0.25, device=DEV) if c.acc else torch.empty(d, device=DEV)
    db = torch.full((d,), -0.25, device=DEV) if c.acc else torch.empty(d, device=DEV)
    wsb = L.advmil_gcn_res_bwd_workspace_bytes(N, d)
    ws = torch.empty(wsb // 4, device=DEV)
    assert L.advmil_gcn_res_fwd(p(h), p(x), x.stride(0), p(gm), p(bt), 1e-5, N, d, c.p, p(seed), SID, p(rr), p(out), out.stride(0), p(mean),
                                p(rstd), st) == 0
    assert L.advmil_gcn_res_bwd(p(dout), dout.stride(0), p(h), p(gm), p(bt), p(mean), p(rstd), N, d, c.p, p(seed), SID, p(rr), p(dh), p(dx),
                                dx.stride(0), c.dxacc, p(dg), p(db), c.acc, p(ws), wsb, st) == 0
    torch.cuda.synchronize()
    for wide in (out_wide, dx_wide):             # nothing outside the column block was written
        if wide is not None:
            assert bool((wide[:, :d] == 77.0).all()) and bool((wide[:, 2 * d:] == 77.0).all())
    return dict(out=out.contiguous(), mean=mean, rstd=rstd, dh=dh, dx=dx.contiguous(), dgamma=dg, dbeta=db)


def test_every_case_has_its_margin_and_every_switch_is_reached():
    for key, k in SEED_K.items():
        assert margin(res_inputs(*key, k)) >= MARGIN, key
    for field, values in (("block", (0, 1)), ("p", (0.0, 0.1)), ("dxacc", (0, 1)), ("acc", (0, 1)), ("rr", (0, 1))):
        for N, d in SHAPES:
            if field != "rr":
                assert {getattr(c, field) for c in K_CASES if (c.N, c.d) == (N, d)} == set(values), (field, N, d)
    assert any(c.rr for c in K_CASES) and any(c.content == "bigmean" for c in K_CASES)


@pytest.mark.parametrize("c", K_CASES, ids=kid)
def test_kernels_vs_restatement(poison, c):  # noqa: F811
    inp, ref, e32 = k_reference(c)
    assert margin(inp) >= MARGIN                      # no ReLU branch can flip in float32: every entry is compared
    got = launch(c, inp)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), k
    want = dict(ref)
    if c.dxacc:
        want["dx"] = ref["dx"] + inp["dx0"].double()
    if c.acc:
        want["dgamma"], want["dbeta"] = ref["dgamma"] + 0.25, ref["dbeta"] - 0.25
    bound = {k: max(v, 4 * e32[k]) for k, v in KB.items()} if e32 else KB
    judge("gcn_res-" + c.content, kid(c), {k: relerr(got[k], want[k]) for k in KB}, bound)
    keep = keep_mask(c)
    if keep is not None:                              # what the mirror drops is exactly zero (dx: exactly what was there before)
        assert int(keep.sum()) > 0 and (keep.numel() < 64 or int((~keep).sum()) > 0)      # (1 x 4: nothing happens to be dropped)
        assert bool((got["out"].cpu()[~keep] == 0.0).all())
        base = inp["dx0"] if c.dxacc else torch.zeros(c.N, c.d)
        assert torch.equal(got["dx"].cpu()[~keep], base[~keep])
        assert bool((got["out"].cpu()[keep] != 0.0).any())


def test_kernels_are_deterministic_and_contain_a_nan(poison):  # noqa: F811
    from advmil_amd import ops
    c = KCase(65, 384, 1, 0.1, 0, 0, 0, "offset")
    inp, _, _ = k_reference(c)
    a, b = launch(c, inp), launch(c, inp)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    h = inp["h"].clone()
    h[33, 7] = float("nan")
    gm, bt, x = inp["gamma"].to(DEV), inp["beta"].to(DEV), inp["x"].to(DEV)
    clean = ops.gcn_res(inp["h"].to(DEV), x, gm, bt)
    out = ops.gcn_res(h.to(DEV), x, gm, bt)
    bad = torch.isnan(out).cpu()
    assert bool(bad[33].all()) and int(bad.sum()) == c.d
    rows = torch.arange(c.N) != 33
    assert torch.equal(out.cpu()[rows], clean.cpu()[rows])


def test_op_backward_arena_free_and_argument_errors(poison):  # noqa: F811
    from advmil_amd import _lib, ops
    c = KCase(15, 100, 0, 0.0, 0, 0, 0, "offset")
    inp, ref, _ = k_reference(c)
    h, x, gm, bt = (inp[k].to(DEV).requires_grad_(True) for k in ("h", "x", "gamma", "beta"))
    out = ops.gcn_res(h, x, gm, bt, 1e-5)
    out.backward(inp["dout"].to(DEV))
    judge("gcn_res-op", kid(c), dict(out=relerr(out, ref["out"]), dh=relerr(h.grad, ref["dh"]), dx=relerr(x.grad, ref["dx"]),
                                     dgamma=relerr(gm.grad, ref["dgamma"]), dbeta=relerr(bt.grad, ref["dbeta"])), KB)
    with pytest.raises(_lib.AdvmilHipError, match="invalid argument"):
        ops.gcn_res(torch.zeros(16, 130, device=DEV), torch.zeros(16, 130, device=DEV), torch.ones(130, device=DEV), torch.zeros(130, device=DEV))
    with pytest.raises(ValueError):
        ops.gcn_res(torch.zeros(16, 128, device=DEV), torch.zeros(8, 128, device=DEV), torch.ones(128, device=DEV), torch.zeros(128, device=DEV))


# ------------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------------
# what the commit before this feature issued for the same forward + backward (recorded from its own run through _lib.check)
SHIPPED_DEPTH_ONE_CALLS = [
    "gemm_plan", "gemm_f32[200x128x1024]", "genconv_fwd", "gemm_plan", "gemm_f32[200x256x128]", "ln_relu_fwd", "gemm_plan",
    "gemm_f32[200x128x256]", "gemm_f32[200x128x256]", "gemm_f32[200x256x128]", "gate_score_fwd", "softmax_pool_fwd",
    "small_linear_fwd[1x64x128]", "skinny_linear_fwd", "skinny_linear_bwd", "small_linear_bwd[1x64x128]", "softmax_pool_bwd",
    "gemm_plan_planes", "gate_bwd", "gemm_plan", "gemm_f32[200x128x256]", "gemm_plan", "gemm_f32[256x128x200]", "act_dropout_bwd",
    "gemm_plan", "gemm_f32[128x256x200]", "gemm_plan", "gemm_f32[200x256x128]", "colsum", "gemm_f32[128x256x200]",
    "gemm_f32[200x256x128]", "ln_relu_bwd", "colsum", "gemm_f32[256x128x200]", "gemm_f32[200x128x256]", "genconv_bwd",
    "act_dropout_bwd", "gemm_plan", "gemm_f32[128x1024x200]"]


def build_generator(L, edge_agg="spatial"):
    from advmil_amd.model import Generator, load_backbone
    bb = load_backbone("graph", DIMS, num_layers=L, edge_agg=edge_agg)
    return Generator(128, 1, bb, SimpleNamespace(noise=[0, 1], hops=1, noise_dist="uniform"), False, 0.6, "sigmoid").to(DEV)


def graph_data(N, seed=9, k_spatial=8, k_latent=4):
    x = H.bag(seed, 512, DEV)[0, :N].contiguous()
    return SimpleNamespace(x=x, edge_index=H.T(synth.grid_knn_graph(N, k_spatial), DEV), edge_latent=H.T(synth.grid_knn_graph(N, k_latent), DEV))


@pytest.mark.parametrize("p_on", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("L", [2, 3])
def test_deep_patchgcn_vs_restatement(L, p_on):
    """tests/test_parity_gpu.py::test_patchgcn_vs_oracle at depth L: forward and every parameter gradient against the float64
    restatement. PARITY UNPINNED against upstream torch_geometric (absent): self-consistency only."""
    from advmil_amd import ops
    N = 500                                               # not a multiple of 16 / 64: ragged node count
    g = build_generator(L)
    PG = load_synth(g, f"G-graph{L}:")
    g.train(p_on)
    rng = ops.DeviceRng(DEV, seed=77); rng.record = True
    for m in g.modules():
        m.rng = rng
    data = graph_data(N)
    nz = [H.noise_tensor("gcn", 0, 64, DEV)]
    pred = g(data, None, noise=nz)
    pred.sum().backward()
    masks = None
    if p_on:
        def mk(tag):
            e = [e for e in rng.log if e[0] == tag][0]
            return torch.as_tensor(synth.dropout_keep(77, e[1], int(np.prod(e[2])), e[3]).reshape(e[2])).double() / (1 - e[3])
        def small(tag, p, shape):
            e = [e for e in rng.log if e[0] == tag][0]
            u = synth.kernel_uniform(77, e[1], int(np.prod(shape))).reshape(shape)
            return torch.as_tensor((u >= np.float32(p))).double() / (1 - p)
        masks = {"fc": mk("gcn_fc"), "phi": mk("gcn_phi"), "att_a": mk("gate_att_a"), "att_b": mk("gate_att_b"),
                 "mlp0": small("gen_mlp0.2", 0.6, (1, 64))}
        for l in range(1, L):
            masks[f"res{l}"] = mk(f"gcn_res{l}")
            assert [e[3] for e in rng.log if e[0] == f"gcn_res{l}"] == [0.1]
    Pr = {k: v.double().cpu().clone().requires_grad_(True) for k, v in PG.items()}
    pr = R.generator_deep(Pr, data.x.double().cpu(), data.edge_index.cpu(), L, [nz[0].double().cpu()], masks)
    pr.sum().backward()
    worst = [close(pred, pr), 0.0]
    for k, p in g.named_parameters():
        want = Pr[k].grad
        if want is None or k.startswith("backbone.layers.0.norm."):
            assert k.startswith("backbone.layers.0.norm.") or want is not None, k
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        scale = float(want.abs().max()) + 1e-12
        err = float((p.grad.double().cpu() - want).abs().max())
        worst[1] = max(worst[1], err / (2e-4 * scale + 1e-8))
        assert err <= 2e-4 * scale + 1e-8, (k, err, scale)
    print(f"[deep-patchgcn] L{L} {'train' if p_on else 'eval'}: pred {worst[0]:.2e}/2.0e-05  worst gradient error over bound {worst[1]:.3f}")


def test_latent_edges_are_the_edge_set_in_use():
    g_lat, g_spa = build_generator(2, "latent").eval(), build_generator(2, "spatial").eval()
    load_synth(g_lat, "G-graph2:"); load_synth(g_spa, "G-graph2:")
    N = 300
    data = graph_data(N)
    assert data.edge_latent.shape != data.edge_index.shape
    swapped = SimpleNamespace(x=data.x, edge_index=data.edge_latent)
    nz = [H.noise_tensor("gcn", 0, 64, DEV)]
    with torch.no_grad():
        a = g_lat(data, None, noise=nz)
        b = g_spa(swapped, None, noise=nz)
        c = g_spa(data, None, noise=nz)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    with pytest.raises(AttributeError):
        with torch.no_grad():
            g_lat(SimpleNamespace(x=data.x, edge_index=data.edge_index), None, noise=nz)
    with pytest.raises(AttributeError):
        seg_lens = [N, N]
        from advmil_amd import ops
        with torch.no_grad():
            g_lat.backbone.features_multi(torch.cat([data.x, data.x]), ops.Segments(seg_lens, DEV), [SimpleNamespace(x=data.x, edge_index=data.edge_index)] * 2)


@pytest.mark.parametrize("edge_agg", ["spatial", "latent"])
def test_deep_slab_features_equal_per_bag_features(edge_agg):
    """tests/test_parity_gpu.py::test_slab_features_equal_per_bag_features at L = 2, for either edge set."""
    from advmil_amd import ops
    from advmil_amd.model import load_backbone
    bb = load_backbone("graph", DIMS, num_layers=2, edge_agg=edge_agg).to(DEV).eval()
    lens = [64, 512, 208]
    exts = [graph_data(n, seed=20 + i) for i, n in enumerate(lens)]
    seg = ops.Segments(lens, DEV)
    X = torch.cat([e.x for e in exts], dim=0)
    with torch.no_grad():
        multi = bb.features_multi(X, seg, exts)
        single = torch.cat([bb.features_multi(e.x, None, [e]) for e in exts], dim=0)
    assert multi.shape == single.shape == (3, DIMS[1])
    close(multi, single, 1e-5)


def test_depth_one_issues_the_launches_of_the_shipped_model(monkeypatch):
    """num_layers = 1, 'spatial': the C-ABI calls of a training forward + backward are the shipped model's, none of them the new kernel."""
    from advmil_amd import _lib
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, name="": (calls.append(name), real(rc, name))[1])
    out = {}
    for L in (1, 2):
        del calls[:]
        g = build_generator(L).train()
        pred = g(graph_data(200), None, noise=[H.noise_tensor("gcn", 0, 64, DEV)])
        pred.sum().backward()
        torch.cuda.synchronize()
        out[L] = list(calls)
    launches = lambda names: [n for n in names if not n.startswith("gemm_plan")]      # noqa: E731  (plan queries: host only, memoised per process)
    assert launches(out[1]) == launches(SHIPPED_DEPTH_ONE_CALLS), out[1]
    extra = collections.Counter(out[2]) - collections.Counter(out[1])
    for name in ("genconv_fwd", "genconv_bwd", "ln_relu_fwd", "ln_relu_bwd", "gcn_res_fwd", "gcn_res_bwd"):
        assert extra[name] == 1, (name, extra)


# ------------------------------------------------------------------------------------------------------------------------------
# the handler
# ------------------------------------------------------------------------------------------------------------------------------
def _step_handler(warmup):
    from advmil_amd.graphed import GraphedStep
    from advmil_amd.model import MyHandler
    h = MyHandler(default_cfg(bcb_mode="graph", bcb_dims="1024-128-128", gen_dims="128-1", bcb_gcn_layers=2, bp_every_batch=2), device=DEV)
    assert h.netG.backbone.num_layers == 2 and h.netG.training
    load_synth(h.netG, "G-graph2:"); load_synth(h.netD, "D-prj:")
    h.rng.reset(4321)
    xs = []
    for i in range(2):
        d = graph_data(256, seed=40 + i)
        xs.append([d.x.unsqueeze(0), d])
    ys_host = [H.label(i) for i in range(2)]
    ys = [y.to(DEV) for y in ys_host]
    g = GraphedStep(h, xs, ys, ys_host, warmup=warmup, keep_warmup=True)
    return h, g


def test_graphed_deep_step_equals_the_eager_step_bit_for_bit():
    """One warm-up step + one replay of the captured G+D step against two eager steps (dropout ON: the replay re-draws the block's mask
    from the device seed): the second step's losses and the weights behind it."""
    from advmil_amd import ops
    prev = ops.get_gemm_mode()
    try:
        he, _ = _step_handler(2)                          # two eager steps (and a capture that is never replayed)
        torch.cuda.synchronize()
        eager_logs = [he.resolve_log(d) for d in he.history[-2:]]
        hg, g = _step_handler(1)
        g.replay()
        torch.cuda.synchronize()
        graph_logs = [hg.resolve_log(d) for d in g.logs]
    finally:
        ops.set_gemm_mode(prev)
    assert len(eager_logs) == len(graph_logs) == 2
    for a, b in zip(graph_logs, eager_logs):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], (k, a[k], b[k])
    assert torch.equal(hg.optimizerG.flat_param, he.optimizerG.flat_param) and torch.equal(hg.optimizerD.flat_param, he.optimizerD.flat_param)
    assert int(hg.optimizerG.step_t.item()) == int(he.optimizerG.step_t.item()) == 2


# ------------------------------------------------------------------------------------------------------------------------------
# bag-parallel
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_two_rank_deep_step_equals_single_rank_with_dropout_on(tmp_path):
    """tests/test_parallel_gpu.py::test_multi_rank_step_equals_single_rank_with_dropout_on for a two-layer PatchGCN (W = 2 over gloo on
    the one GPU): the block's dropout is drawn through the `patch` row map of its site (ops.SITE_LAYOUTS['gcn_res']), so each rank's
    rows draw what the single process draws for them. Same comparison rules as that test."""
    import os
    import subprocess
    import sys
    from tests import dp_worker_gcn
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    want = dp_worker_gcn.run(2, 1, 0)
    out = str(tmp_path / "r0.pt")
    port = str(31300 + os.getpid() % 1500)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, "-m", "tests.dp_worker_gcn", str(r), "2", port, out, "2"], cwd=root, env=env) for r in range(2)]
    try:
        for p in procs:
            assert p.wait(timeout=500) == 0
    finally:
        for p in procs:                       # a failed rank must not leave its peer waiting in a collective
            if p.poll() is None:
                p.kill()
    got = torch.load(out, weights_only=False)
    for k in ("y", "y_hat", "f_fake"):
        a, b = got["cl"][k].double().reshape(-1), want["cl"][k].double().reshape(-1)
        assert a.shape == b.shape and float((a - b).abs().max()) < 2e-6, (k, float((a - b).abs().max()))
    assert len(got["logs"]) == len(want["logs"]) == 4
    for la, lb in zip(got["logs"], want["logs"]):
        for key in lb:
            if key != "i_batch":              # the rank's own loader position
                assert abs(float(la[key]) - float(lb[key])) < 2e-6, (key, la[key], lb[key])
    lr = 8e-5
    for tag, prefix in (("G", "G-graph2:"), ("D", "D-prj:")):
        for k in want[tag]:
            p0 = H.T(synth.param(H.PARAM_SEED, prefix + k, tuple(want[tag][k].shape))).double()
            da, db = float((got[tag][k].double() - p0).norm()), float((want[tag][k].double() - p0).norm())
            assert abs(da - db) <= 5e-3 * db + max(5e-5, 2 * lr * want[tag][k].numel() ** 0.5 if db < 2e-4 else 0.0), (tag, k, da, db)
            dw = (got[tag][k].double() - want[tag][k].double()).abs()
            assert int((dw > 2.5 * lr).sum()) <= max(1, dw.numel() // 10000), (tag, k, int((dw > 2.5 * lr).sum()))
            assert float(dw.max()) <= 2.05 * lr * 2, (tag, k, float(dw.max()))
