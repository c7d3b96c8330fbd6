"""GPU: each C-ABI kernel against a float64 torch-CPU restatement of the same op (the kernels are
floating point, so the per-op reference is plain torch; the path-level oracle tests live in
test_parity_gpu.py). Tolerances are written per test."""
import numpy as np
import pytest
import torch

from advmil_amd import synth
from tests import helpers as H
from tests.poison import PATTERNS, poisoned_allocations

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import ops as _ops
    from advmil_amd import _lib
    _lib.lib()
    return _ops


def rnd(tag, *shape, scale=1.0):
    n = int(np.prod(shape))
    return H.T(synth.normal(synth.stream_key(11, tag), n).reshape(shape) * np.float32(scale))


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


ACT = {0: lambda v: v, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid}


@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, False), (False, True)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (200, 72, 100), (512, 384, 1024), (384, 1024, 520), (16, 64, 128), (260, 196, 36)])
def test_gemm_layouts(ops, a_kc, b_kc, M, N, K):
    A = rnd(f"A{M}{K}", M, K); B = rnd(f"B{K}{N}", K, N)      # asymmetric, non-square
    ref = A.double() @ B.double()
    Ad = (A if a_kc else A.t().contiguous()).to(DEV)
    Bd = (B.t().contiguous() if b_kc else B).to(DEV)
    for splits in (1, 3):
        for tile in (0, 22, 23, 13, 12, 11):
            C = ops.gemm(Ad, Bd, a_kc, b_kc, M, N, K, splits=splits, tile=tile)
            assert relerr(C, ref) < 2e-6, (splits, tile, relerr(C, ref))


def test_gemm_epilogue_all(ops):
    M, N, K = 200, 256, 96
    A = rnd("eA", M, K); W = rnd("eW", N, K); bias = rnd("eb", N); rowv = rnd("er", M); colv = rnd("ec", N)
    maskref = rnd("em", M, N); C0 = rnd("eC", M, N)
    pre = 0.5 * (A.double() @ W.double().t()) + bias.double() + rowv.double()[:, None] * colv.double()[None, :]
    v = torch.cat([torch.tanh(pre[:, :128]), torch.sigmoid(pre[:, 128:])], dim=1)
    v = v * (maskref.double() > 0) * 1.25 + C0.double()
    for splits in (1, 2):
        for tile in (0, 23, 13, 11):
            out = C0.clone().to(DEV)
            ops.gemm(A.to(DEV), W.to(DEV), True, True, M, N, K, out=out, bias=bias.to(DEV), act0=2, act1=3, act_split=128,
                     rowv=rowv.to(DEV), colv=colv.to(DEV), maskref=maskref.to(DEV), mask_scale=1.25, accumulate=True, alpha=0.5,
                     splits=splits, tile=tile)
            assert relerr(out, v) < 2e-6, (splits, tile)


def test_gemm_strided_output(ops):
    M, N, K = 64, 32, 64
    A = rnd("sA", M, K); W = rnd("sW", N, K)
    out = torch.zeros(M, 96, device=DEV)
    ops.gemm(A.to(DEV), W.to(DEV), True, True, M, N, K, out=out[:, 32:64], ldc=96)
    ref = torch.zeros(M, 96, dtype=torch.float64); ref[:, 32:64] = A.double() @ W.double().t()
    assert relerr(out, ref) < 2e-6


def test_gemm_dropout_matches_host_rng(ops):
    M, N, K, p = 96, 64, 32, 0.25
    A = rnd("dA", M, K); W = rnd("dW", N, K)
    rng = ops.DeviceRng(DEV, seed=1234)
    sid = rng.site("t")
    for splits in (1, 2):
        y = ops.gemm(A.to(DEV), W.to(DEV), True, True, M, N, K, act0=1, drop_p=p, seed=rng.seed, stream_id=sid, splits=splits)
        keep = synth.dropout_keep(1234, sid, M * N, p).reshape(M, N)
        ref = torch.relu(A.double() @ W.double().t()) * H.T(keep).double() / (1 - p)
        assert relerr(y, ref) < 2e-6
    assert 0.70 < keep.mean() < 0.80


def test_gemm_rejects_bad_args(ops):
    from advmil_amd._lib import AdvmilHipError
    A = torch.zeros(8, 6, device=DEV); B = torch.zeros(8, 6, device=DEV)
    with pytest.raises(AdvmilHipError):
        ops.gemm(A, B, True, True, 8, 8, 6)        # K % 4 != 0
    with pytest.raises(RuntimeError):
        ops.gemm(torch.zeros(8, 8), torch.zeros(8, 8), True, True, 8, 8, 8)   # CPU tensors: no fallback


@pytest.mark.parametrize("N,D,p", [(512, 384, 0.0), (1000, 128, 0.25), (37, 384, 0.25), (8, 384, 0.0)])
def test_gated_pool_fwd_bwd(ops, N, D, p):
    h = rnd(f"gh{N}", N, D); Wa = rnd("gWa", D, D, scale=0.05); Wb = rnd("gWb", D, D, scale=0.05)
    ba = rnd("gba", D, scale=0.1); bb = rnd("gbb", D, scale=0.1); wc = rnd("gwc", 1, D, scale=0.3); bc = rnd("gbc", 1)
    gp = rnd("ggp", D); gA = rnd("ggA", N)
    leaves = [t.clone().to(DEV).requires_grad_(True) for t in (h, Wa, ba, Wb, bb, wc, bc)]
    rng = ops.DeviceRng(DEV, seed=77)
    pooled, A, s = ops.gated_attn_pool(*leaves, p=p, rng=rng)
    (pooled * gp.to(DEV)).sum().add((A * gA.to(DEV)).sum()).backward()
    # reference (float64 CPU) with the kernel's masks regenerated on the host
    ma = mb = None
    if p > 0:
        ma = H.T(synth.dropout_keep(77, 1, N * D, p).reshape(N, D)).double() / (1 - p)
        mb = H.T(synth.dropout_keep(77, 2, N * D, p).reshape(N, D)).double() / (1 - p)
    ref = [t.clone().double().requires_grad_(True) for t in (h, Wa, ba, Wb, bb, wc, bc)]
    rh, rWa, rba, rWb, rbb, rwc, rbc = ref
    a = torch.tanh(rh @ rWa.t() + rba); b = torch.sigmoid(rh @ rWb.t() + rbb)
    if p > 0:
        a = a * ma; b = b * mb
    sr = ((a * b) @ rwc.t() + rbc).reshape(-1)
    Ar = torch.softmax(sr, 0)
    pr = Ar @ rh
    (pr * gp.double()).sum().add((Ar * gA.double()).sum()).backward()
    assert relerr(s, sr) < 1e-5
    assert relerr(A, Ar) < 1e-5
    assert relerr(pooled, pr) < 1e-5
    for got, want, name in zip(leaves, ref, "h Wa ba Wb bb wc bc".split()):
        if name == "bc":   # softmax is shift invariant: d/dbc == 0 exactly; the kernel sums ds to round-off
            assert float(got.grad.abs().max()) < 1e-5
        else:
            assert relerr(got.grad, want.grad) < 5e-5, name


@pytest.mark.parametrize("N,d", [(512, 128), (64, 384), (16, 200)])
def test_ln_relu_mean16(ops, N, d):
    y = rnd(f"ly{N}{d}", N, d); g = 1 + 0.1 * rnd("lg", d); b = 0.1 * rnd("lb", d); ge = rnd("le", N // 16, d)
    lv = [t.clone().to(DEV).requires_grad_(True) for t in (y, g, b)]
    emb = ops.ln_relu_mean16(*lv)
    (emb * ge.to(DEV)).sum().backward()
    rv = [t.clone().double().requires_grad_(True) for t in (y, g, b)]
    z = torch.relu(torch.nn.functional.layer_norm(rv[0], (d,), rv[1], rv[2], 1e-5)).reshape(N // 16, 16, d).mean(1)
    (z * ge.double()).sum().backward()
    assert relerr(emb, z) < 1e-5
    for got, want in zip(lv, rv):
        assert relerr(got.grad, want.grad) < 5e-5
    # the same backward also hands out the column sums of dy (bias gradient of the FC that produced y), added into an accumulator
    acc = torch.full((d,), 0.5, device=DEV)
    lv2 = [t.clone().to(DEV).requires_grad_(True) for t in (y, g, b)]
    (ops.ln_relu_mean16(*lv2, ycol_grad=acc) * ge.to(DEV)).sum().backward()
    assert relerr(acc, rv[0].grad.sum(0) + 0.5) < 5e-5
    assert torch.equal(lv2[0].grad, lv[0].grad)


@pytest.mark.parametrize("act,p", [("relu", 0.25), ("tanh", 0.0), ("sigmoid", 0.25), ("none", 0.0), ("none", 0.5)])
def test_linear_act_autograd(ops, act, p):
    M, K, N = 300, 128, 64
    x = rnd("lx", M, K); W = rnd("lW", N, K, scale=0.1); b = rnd("lbb", N, scale=0.1); gy = rnd("lgy", M, N)
    lv = [t.clone().to(DEV).requires_grad_(True) for t in (x, W, b)]
    rng = ops.DeviceRng(DEV, seed=5)
    y = ops.linear_act(lv[0], lv[1], lv[2], act, p, rng)
    (y * gy.to(DEV)).sum().backward()
    rv = [t.clone().double().requires_grad_(True) for t in (x, W, b)]
    yr = ACT[ops._ACT[act]](rv[0] @ rv[1].t() + rv[2])
    if p > 0:
        yr = yr * H.T(synth.dropout_keep(5, 1, M * N, p).reshape(M, N)).double() / (1 - p)
    (yr * gy.double()).sum().backward()
    assert relerr(y, yr) < 1e-5
    for got, want, nm in zip(lv, rv, "x W b".split()):
        assert relerr(got.grad, want.grad) < 5e-5, nm


def test_colsum_and_abs_sum_and_uniform(ops):
    x = rnd("cx", 1000, 2048)
    assert relerr(ops.colsum(x.to(DEV), 1000, 2048), x.double().sum(0)) < 1e-5
    assert relerr(ops.abs_sum(x.to(DEV).reshape(-1)), x.double().abs().sum().reshape(1)) < 1e-5
    rng = ops.DeviceRng(DEV, seed=99)
    u = rng.uniform(1000)
    assert np.array_equal(u.cpu().numpy(), synth.kernel_uniform(99, 1, 1000))
    rng.advance(3)
    u2 = rng.uniform(10)
    assert np.array_equal(u2.cpu().numpy(), synth.kernel_uniform(102, 2, 10))


def test_adam_matches_oracle(ops):
    from oracle import advmil_oracle as O
    n = 5000
    p0 = rnd("ap", n, scale=0.1); wdmask = torch.zeros(n); wdmask[:3000] = 5e-4
    P = {"w.weight": p0[:3000].reshape(30, 100).clone(), "w.bias": p0[3000:].clone()}
    st = {}
    pd = p0.clone().to(DEV); m = torch.zeros(n, device=DEV); v = torch.zeros(n, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for it in range(3):
        g = rnd(f"ag{it}", n, scale=0.01)
        G = {"w.weight": g[:3000].reshape(30, 100), "w.bias": g[3000:]}
        # oracle: L1 subgradient enters through the loss; here it is folded into the kernel
        Gl1 = {k: G[k] + 1e-5 * torch.sign(P[k]) for k in P}
        P = O.adam_step(P, Gl1, st, 8e-5, 5e-4, decay_filter=True)
        ops.adam_step(pd, g.to(DEV), m, v, wdmask.to(DEV), step, 8e-5, l1_coef=1e-5)
    ref = torch.cat([P["w.weight"].reshape(-1), P["w.bias"]])
    assert float((pd.cpu() - ref).abs().max()) < 1e-7
    assert int(step.item()) == 3


@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, False)])
def test_gemm_split_bf16x3_mode(ops, a_kc, b_kc):
    """bf16x3 arithmetic of the fp32 engine: products of the hi/lo bf16 splits on the bf16 matrix pipe, fp32 accumulate.
    Error model: ~2^-17 |a||b| per product -> a few 1e-6 of the result scale at K ~ 1000 (exact fp32 MFMA: ~1e-7)."""
    M, N, K = 520, 200, 1000
    A = rnd("xA", M, K); B = rnd("xB", K, N)
    ref = A.double() @ B.double()
    Ad = (A if a_kc else A.t().contiguous()).to(DEV)
    Bd = (B.t().contiguous() if b_kc else B).to(DEV)
    prev = ops.get_gemm_mode()
    try:
        ops.set_gemm_mode("bf16x3")
        for tile in (22, 23, 13, 12, 11):
            for splits in (1, 2):
                C = ops.gemm(Ad, Bd, a_kc, b_kc, M, N, K, splits=splits, tile=tile)
                err = relerr(C, ref)
                assert err < 1.5e-5, (tile, splits, err)
        ops.set_gemm_mode("exact")
        assert relerr(ops.gemm(Ad, Bd, a_kc, b_kc, M, N, K), ref) < 2e-6
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, False), (False, True)])
@pytest.mark.parametrize("shape", [(512, 384, 1024, 0), (200, 136, 72, 11), (384, 256, 4096, 22)])
def test_gemm_planes_bit_identical_to_on_the_fly_split(ops, a_kc, b_kc, shape):
    """bf16x3 mode: operands given as pre-split planes (any subset) give bit-identical results to the in-kernel split, and
    the planes the epilogue emits equal split_planes(C)."""
    M, N, K, tile = shape
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("bf16x3")
    try:
        g = torch.Generator(device="cuda").manual_seed(5)
        A = torch.randn((M, K) if a_kc else (K, M), device="cuda", generator=g)
        B = torch.randn((N, K) if b_kc else (K, N), device="cuda", generator=g)
        bias = torch.randn(N, device="cuda", generator=g)
        pa, pb = ops.split_planes(A), ops.split_planes(B)
        # planes hold exactly bf16(x) and bf16(x - bf16(x))
        assert torch.equal(pa.hi, A.to(torch.bfloat16))
        assert torch.equal(pa.lo, (A - A.to(torch.bfloat16).float()).to(torch.bfloat16))
        ref = ops.gemm(A, B, a_kc, b_kc, M, N, K, bias=bias, act0=1, tile=tile)
        for use_a, use_b in [(True, False), (False, True), (True, True)]:
            cp = ops.Planes.empty_like(ref)
            got = ops.gemm(A, B, a_kc, b_kc, M, N, K, bias=bias, act0=1, tile=tile, a_planes=pa if use_a else None,
                           b_planes=pb if use_b else None, c_planes=cp)
            assert torch.equal(got, ref), (use_a, use_b)
            want = ops.split_planes(got)
            assert torch.equal(cp.hi, want.hi) and torch.equal(cp.lo, want.lo)
        # split-K path: planes in, planes out of the reduce launch
        cp = ops.Planes.empty_like(ref)
        r2 = ops.gemm(A, B, a_kc, b_kc, M, N, K, splits=2, tile=tile)
        g2 = ops.gemm(A, B, a_kc, b_kc, M, N, K, splits=2, tile=tile, a_planes=pa, b_planes=pb, c_planes=cp)
        assert torch.equal(g2, r2)
        assert torch.equal(cp.hi, g2.to(torch.bfloat16))
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(384, 1024, 32768), (768, 384, 16384), (128, 1024, 65536), (256, 256, 8192 + 96), (512, 256, 16384)])
def test_gemm_tn_planes_kernel_bit_identical_to_generic(ops, M, N, K):
    """The LDS-DMA fed TN contraction over two plane-held [K, .] operands (deep-K weight gradients, tile codes 91-93) against the
    generic kernel with the same split count: every partial sum is accumulated in the same k order, so the results are EQUAL --
    plain, and accumulated into an existing gradient (the arena form); and within 2e-5 of a float64 product."""
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("bf16x3")
    try:
        tile, sp = ops.gemm_plan_tn_planes(M, N, K)
        planned = tile != 0
        if not planned:                          # too few tiles for the plan to pick the kernel: drive the 256x256 form directly
            assert M % 256 == 0 and N % 256 == 0
            tile, sp = 93, 4
        assert tile in (91, 92, 93) and sp >= 1, (tile, sp)
        g = torch.Generator(device="cuda").manual_seed(11)
        A = torch.randn(K, M, device="cuda", generator=g)
        B = torch.randn(K, N, device="cuda", generator=g)
        pa, pb = ops.split_planes(A), ops.split_planes(B)
        with poisoned_allocations(PATTERNS[0]):      # (fresh output and split-K workspace blocks hold NaN / 3.39e38, not an earlier result)
            ref = ops.gemm(A, B, False, False, M, N, K, tile=22, splits=sp, a_planes=pa, b_planes=pb)
        with poisoned_allocations(PATTERNS[1]):
            got = ops.gemm(None, B, False, False, M, N, K, a_planes=pa, b_planes=pb, tile=tile, splits=sp)     # (A as planes only)
        assert torch.equal(got, ref)
        base = torch.randn(M, N, device="cuda", generator=g)
        acc_ref, acc_got = base.clone(), base.clone()
        with poisoned_allocations(PATTERNS[0]):
            ops.gemm(A, B, False, False, M, N, K, out=acc_ref, ldc=N, accumulate=True, tile=22, splits=sp, a_planes=pa, b_planes=pb)
        with poisoned_allocations(PATTERNS[1]):
            ops.gemm(None, B, False, False, M, N, K, out=acc_got, ldc=N, accumulate=True, a_planes=pa, b_planes=pb,
                     **({} if planned else dict(tile=tile, splits=sp)))                # (planned shapes: the plan picks the kernel itself)
        assert torch.equal(acc_got, acc_ref)
        want = (A.double().t() @ B.double())
        assert float((got.double() - want).abs().max()) <= 2e-5 * float(want.abs().max())        # (bf16x3: ~2^-17 per product)
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("tile,N,K,R", [(34, 384, 1024, 8192), (34, 192, 264, 4104), (24, 128, 1024, 8192), (24, 136, 520, 4104)])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_weight_gradient_from_planes_only_activation_backward(ops, tile, N, K, R, p):
    """First-layer weight gradient dpre^T X with dpre written as hi/lo planes ONLY by the activation backward (no fp32 copy) and the
    contraction taking both operands pre-split (tiles 34 / 24, [k][m] layout on both sides; the 192-row tile stages 1.5 pieces per
    thread): bit-identical to the fp32 dpre split on the fly, ragged edges included."""
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("bf16x3")
    try:
        g = torch.Generator(device="cuda").manual_seed(17)
        X = torch.randn(R, K, device="cuda", generator=g)
        dy = torch.randn(R, N, device="cuda", generator=g)
        y = torch.relu(torch.randn(R, N, device="cuda", generator=g))
        seed = torch.tensor([77], dtype=torch.int64, device="cuda") if p else None
        dpre, db0 = ops.act_dropout_bwd(dy, y, ops.ACT_RELU, R, N, p, seed, 5)
        pl = ops.Planes(torch.empty(R, N, dtype=torch.bfloat16, device="cuda"), torch.empty(R, N, dtype=torch.bfloat16, device="cuda"))
        none, db1 = ops.act_dropout_bwd(dy, y, ops.ACT_RELU, R, N, p, seed, 5, planes=pl, planes_only=True)
        assert none is None and torch.equal(db0, db1)
        want = ops.split_planes(dpre)
        assert torch.equal(pl.hi, want.hi) and torch.equal(pl.lo, want.lo)
        px = ops.split_planes(X)
        for splits in (1, 4):
            ref = ops.gemm(dpre, X, False, False, N, K, R, tile=tile, splits=splits)
            got = ops.gemm(None, X, False, False, N, K, R, tile=tile, splits=splits, a_planes=pl, b_planes=px)
            assert torch.isfinite(got).all() and torch.equal(got, ref), splits
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("d,N,C", [(128, 8192, 1024), (384, 4096 + 256, 1024)])
def test_layernorm_backward_hands_dy_over_as_operand_planes(ops, d, N, C):
    """Region embedding FC -> LayerNorm -> ReLU -> mean16 (AVGPoolPatchEmbedding, reference model/backbone_utils.py:158-168): in bf16x3 mode
    the LayerNorm backward writes dy as hi / lo operand planes ONLY and the FC's weight gradient dy^T X takes both operands pre-split
    (ops.DY_PLANES). (1) the kernel's planes equal the split of its own fp32 dy bit for bit, gamma / beta / column-sum gradients unchanged;
    (2) the layer's weight gradient with the hand-over equals the one without it (same contraction kernel, same products: equal),
    and the token entry is consumed."""
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("bf16x3")
    try:
        g = torch.Generator(device="cuda").manual_seed(23)
        y = torch.randn(N, d, device="cuda", generator=g)
        gamma = 1.0 + 0.1 * torch.randn(d, device="cuda", generator=g)
        beta = 0.1 * torch.randn(d, device="cuda", generator=g)
        demb = torch.randn(N // 16, d, device="cuda", generator=g)
        emb, mean, rstd = ops.ln_relu_mean16_fwd(y, gamma, beta, N, d, 1e-5)
        yc0, yc1 = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
        dy, dg0, db0 = ops.ln_relu_mean16_bwd(demb, y, gamma, beta, mean, rstd, N, d, ycol_out=yc0)
        pl = ops.Planes.alloc((N, d), y.device)
        _, dg1, db1 = ops.ln_relu_mean16_bwd(demb, y, gamma, beta, mean, rstd, N, d, ycol_out=yc1, planes=pl)
        want = ops.split_planes(dy)
        assert torch.equal(pl.hi, want.hi) and torch.equal(pl.lo, want.lo)
        assert torch.equal(dg0, dg1) and torch.equal(db0, db1) and torch.equal(yc0, yc1)
        # the layer: X is a resident slab (its planes registered), the FC has a constant bias, its weight the only gradient
        X = torch.randn(N, C, device="cuda", generator=g)
        X._advmil_planes = ops.split_planes(X)
        W = (torch.randn(d, C, device="cuda", generator=g) / C ** 0.5).requires_grad_(True)
        b = torch.zeros(d, device="cuda")
        gam, bet = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        grads, took, real = [], [], ops.ln_relu_mean16_bwd

        def spy(*a, **k):
            took.append(k.get("planes") is not None)
            return real(*a, **k)
        ops.ln_relu_mean16_bwd = spy
        for on in (False, True):
            ops.LN_DY_PLANES = on
            ops.DY_PLANES.clear()
            W.grad = None
            ycol = torch.zeros(d, device="cuda")
            out = ops.ln_relu_mean16(ops.linear_act(X, W, b, "none"), gam, bet, 1e-5, ycol_grad=ycol)
            (out * demb).sum().backward()
            assert not ops.DY_PLANES                                   # handed over and consumed (or never made)
            grads.append((W.grad.clone(), ycol))
        ops.ln_relu_mean16_bwd = real
        assert took == [False, True]                                   # the second pass really went through the planes-only form
        assert torch.isfinite(grads[1][0]).all()
        assert torch.equal(grads[0][1], grads[1][1])
        scale = float(grads[0][0].abs().max())
        assert float((grads[0][0] - grads[1][0]).abs().max()) <= 2e-6 * scale        # (equal when both take the same tile; else fp32 order)
    finally:
        ops.LN_DY_PLANES = True
        if "real" in locals():
            ops.ln_relu_mean16_bwd = real
        ops.set_gemm_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, False), (False, True)])
@pytest.mark.parametrize("tile", [43, 42, 34, 24])
def test_gemm_bf16x3_eight_wave_tiles(ops, a_kc, b_kc, tile):
    """The 512-thread 256x192 / 256x128 tiles of the bf16x3 variant: same arithmetic as the 128x128 tile (bit-identical: each
    output element sees the same products in the same k order), ragged edges included."""
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("bf16x3")
    try:
        g = torch.Generator(device="cuda").manual_seed(11)
        for M, N, K in [(1000, 392, 264), (256, 192, 64), (520, 200, 1032)]:
            A = torch.randn((M, K) if a_kc else (K, M), device="cuda", generator=g)
            B = torch.randn((N, K) if b_kc else (K, N), device="cuda", generator=g)
            bias = torch.randn(N, device="cuda", generator=g)
            ref = ops.gemm(A, B, a_kc, b_kc, M, N, K, bias=bias, act0=1, tile=22)
            got = ops.gemm(A, B, a_kc, b_kc, M, N, K, bias=bias, act0=1, tile=tile)
            assert torch.equal(got, ref), (M, N, K, float((got - ref).abs().max()))
            # and independently: float64 on the host (the split-bf16 products drop ~2^-17 relative per product)
            A64, B64 = A.cpu().double(), B.cpu().double()
            want = torch.relu((A64 if a_kc else A64.t()) @ (B64.t() if b_kc else B64) + bias.cpu().double())
            assert relerr(got, want) < 2e-5, (M, N, K, relerr(got, want))
            r2 = ops.gemm(A, B, a_kc, b_kc, M, N, K, splits=3, tile=22)
            g2 = ops.gemm(A, B, a_kc, b_kc, M, N, K, splits=3, tile=tile)
            assert torch.equal(g2, r2)
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["exact", "bf16x3"])
@pytest.mark.parametrize("tile", [22, 23, 43, 83])
def test_gemm_streaming_epilogue_modes(ops, mode, tile):
    """Whole-tile launches of the 128x128+ tiles take the streaming epilogue (side data parked in LDS, per-element operand one
    sub-tile ahead). Every mode it serves is checked against float64 on the host -- dropout masks regenerated from the counter
    RNG through a shuffled row map -- and bit for bit against the 64x64 tile, which always takes the generic epilogue."""
    if tile == 83 and mode != "bf16x3":
        pytest.skip("the plane-fed kernel is the bf16x3 path")
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        M, N, K, p = 768, 768, 96, 0.25
        tol = 3e-5 if mode == "bf16x3" else 5e-6       # (hardware exp / rcp in tanh and sigmoid: ~1 ulp each)
        g = torch.Generator(device="cuda").manual_seed(5)
        A = 0.1 * torch.randn(M, K, device="cuda", generator=g); W = torch.randn(N, K, device="cuda", generator=g)
        bias = torch.randn(N, device="cuda", generator=g)
        pre = A.cpu().double() @ W.cpu().double().t()          # ~N(0, 1): errors are judged on the scale of the activations' range
        kw = dict(a_planes=ops.split_planes(A), b_planes=ops.split_planes(W)) if tile == 83 else {}

        def both(**e):
            outs = []
            for t in (tile, 11):
                if "out" in e:
                    e["out"] = e["out0"].clone()
                outs.append(ops.gemm(A, W, True, True, M, N, K, tile=t, splits=1, **{k: v for k, v in e.items() if k != "out0"},
                                     **(kw if t == tile else {})))
            assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
            return outs[0]

        # bias + two activations split at a 32-column boundary, planes of the result
        cpl = ops.Planes(torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), torch.empty(M, N, dtype=torch.bfloat16, device="cuda"))
        y = ops.gemm(A, W, True, True, M, N, K, bias=bias, act0=2, act1=3, act_split=384, alpha=0.5, tile=tile, splits=1, c_planes=cpl, **kw)
        want = 0.5 * pre + bias.cpu().double()
        want = torch.cat([torch.tanh(want[:, :384]), torch.sigmoid(want[:, 384:])], dim=1)
        assert relerr(y, want) < tol
        assert torch.equal(y, both(bias=bias, act0=2, act1=3, act_split=384, alpha=0.5))
        ref_pl = ops.split_planes(y)
        assert torch.equal(cpl.hi, ref_pl.hi) and torch.equal(cpl.lo, ref_pl.lo)
        # relu + dropout through a row map (bag-parallel form)
        rng = ops.DeviceRng("cuda", seed=77)
        sid = rng.site("t")
        rmap = torch.randperm(M, generator=torch.Generator().manual_seed(3)).to(torch.int64)
        y = both(bias=bias, act0=1, drop_p=p, seed=rng.seed, stream_id=sid, rng_row=rmap.cuda())
        keep = H.T(synth.dropout_keep(77, sid, M * N, p).reshape(M, N)).double()[rmap]
        assert relerr(y, torch.relu(pre + bias.cpu().double()) * keep / (1 - p)) < tol
        # rank-1 term per bag: + rowv[m] * colv[rowseg[m], n]
        rowv = torch.randn(M, device="cuda", generator=g); colv = torch.randn(4, N, device="cuda", generator=g)
        rowseg = torch.arange(M, device="cuda", dtype=torch.int32) // (M // 4)
        y = both(rowv=rowv, colv=colv, rowseg=rowseg)
        assert relerr(y, pre + rowv.cpu().double()[:, None] * colv.cpu().double()[rowseg.cpu().long()]) < tol
        # mask of a reference activation, and accumulation into the output
        mref = torch.randn(M, N, device="cuda", generator=g)
        y = both(maskref=mref, mask_scale=1.25)
        assert relerr(y, pre * (mref.cpu().double() > 0) * 1.25) < tol
        C0 = torch.randn(M, N, device="cuda", generator=g)
        y = both(out=None, out0=C0, accumulate=True, bias=bias)
        assert relerr(y, pre + bias.cpu().double() + C0.cpu().double()) < tol
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("M,want_tile", [(65536, 85), (16384, 86)])
def test_gemm_two_layers_in_one_launch(ops, M, want_tile):
    """advmil_epilogue_t's two-layer form (tile 85: 256x256; tile 86: 256x128, the slab of a 2-bag step): act1(x W1^T + b1) and
    act2(x W2^T + b2) from one plane-fed launch over stacked weight planes, two outputs, planes of the first. Bit-identical to the two
    separate plane-fed launches, and within the bf16x3 tolerance of float64 on the host; bad arguments are refused."""
    from advmil_amd._lib import AdvmilHipError
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("bf16x3")
    try:
        K, N1, N2 = 256, 384, 128
        assert ops.gemm_two_layers_tile(M, N1, N2, K) == want_tile
        g = torch.Generator(device="cuda").manual_seed(2)
        x = torch.randn(M, K, device="cuda", generator=g)
        W1 = 0.1 * torch.randn(N1, K, device="cuda", generator=g); W2 = 0.1 * torch.randn(N2, K, device="cuda", generator=g)
        b1 = torch.randn(N1, device="cuda", generator=g); b2 = torch.randn(N2, device="cuda", generator=g)
        xpl, p1, p2 = ops.split_planes(x), ops.split_planes(W1), ops.split_planes(W2)
        y1, y2, cpl = ops.gemm_two_layers(x, xpl, W1, p1, b1, 1, W2, p2, b2, 0, True)
        c1 = ops.Planes(torch.empty(M, N1, dtype=torch.bfloat16, device="cuda"), torch.empty(M, N1, dtype=torch.bfloat16, device="cuda"))
        r1 = ops.gemm(x, W1, True, True, M, N1, K, bias=b1, act0=1, a_planes=xpl, b_planes=p1, c_planes=c1, tile=83, splits=1)
        r2 = ops.gemm(x, W2, True, True, M, N2, K, bias=b2, act0=0, a_planes=xpl, b_planes=p2, tile=82, splits=1)
        assert torch.equal(y1, r1) and torch.equal(y2, r2) and torch.equal(cpl.hi, c1.hi) and torch.equal(cpl.lo, c1.lo)
        rows = torch.arange(0, M, 997, device="cuda")
        x64 = x[rows].cpu().double()
        assert relerr(y1[rows], torch.relu(x64 @ W1.cpu().double().t() + b1.cpu().double())) < 2e-5
        assert relerr(y2[rows], x64 @ W2.cpu().double().t() + b2.cpu().double()) < 2e-5
        with pytest.raises(AdvmilHipError):       # the two-layer form exists for the plain 256x256 tile only
            ops.gemm(x, W1, True, True, M, N1, K, a_planes=xpl, b_planes=p1, tile=85, splits=1, drop_p=0.5, seed=ops.DeviceRng("cuda", 1).seed)
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["exact", "bf16x3"])
@pytest.mark.parametrize("tile", [0, 22, 23, 12, 11, 43])
def test_gemm_fused_gate_score(ops, mode, tile):
    """Gate-score mode of the contraction (interleaved branch rows, score reduced in the epilogue, no [N,2D] store) equals the
    two-launch path (gate contraction + gate_score kernel)."""
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        g = torch.Generator(device="cuda").manual_seed(21)
        N, D = 1000, 384
        h = torch.randn(N, D, device="cuda", generator=g)
        Wa, Wb = torch.randn(D, D, device="cuda", generator=g) * 0.05, torch.randn(D, D, device="cuda", generator=g) * 0.05
        ba, bb = torch.randn(D, device="cuda", generator=g) * 0.1, torch.randn(D, device="cuda", generator=g) * 0.1
        wc, bc = torch.randn(D, device="cuda", generator=g) * 0.1, torch.randn(1, device="cuda", generator=g)
        ab = ops.gemm(h, torch.cat([Wa, Wb]), True, True, N, 2 * D, D, bias=torch.cat([ba, bb]), act0=2, act1=3, act_split=D)
        want = ops.gate_score(ab, wc, bc, N, D)
        Wi = torch.stack((Wa, Wb), dim=1).reshape(2 * D, D)
        bi = torch.stack((ba, bb), dim=1).reshape(2 * D)
        part = ops.gemm(h, Wi, True, True, N, 2 * D, D, bias=bi, gate_wc=wc, tile=tile)
        got = part.sum(dim=1) + bc
        assert float((got - want).abs().max()) < 2e-5, float((got - want).abs().max())
        # and independently: float64 on the host
        h64 = h.cpu().double()
        a64 = torch.tanh(h64 @ Wa.cpu().double().t() + ba.cpu().double())
        b64 = torch.sigmoid(h64 @ Wb.cpu().double().t() + bb.cpu().double())
        want64 = (a64 * b64) @ wc.cpu().double() + bc.cpu().double()
        assert float((got.cpu().double() - want64).abs().max()) < 2e-5
    finally:
        ops.set_gemm_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["bce", "hinge", "wasserstein"])
def test_fused_gan_losses_match_composed_torch(ops, which):
    """advmil_gan_d_loss / advmil_gan_g_loss (value + analytic gradients in one launch) against the composed torch losses."""
    from advmil_amd.loss.utils import real_fake_terms, recon_terms
    g = torch.Generator(device="cuda").manual_seed(8)
    nb = 16
    fake = (torch.randn(nb, device="cuda", generator=g) * 2).requires_grad_(True)
    real = (torch.randn(nb, device="cuda", generator=g) * 2).requires_grad_(True)
    mask = (torch.rand(nb, device="cuda", generator=g) < 0.5).float()
    n_real, n_fake = 11.0, 32.0           # global denominators differ from the local counts under bag-parallel
    # the composed reference runs on the HOST in float64 (same formulas, torch CPU): independent of every device kernel
    fake_c, real_c = fake.detach().cpu().double().requires_grad_(True), real.detach().cpu().double().requires_grad_(True)
    tr, tf = real_fake_terms(real_c, fake_c, which)
    want = tf.sum() / n_fake + (tr * mask.cpu().double()).sum() / n_real
    want.backward()
    wf, wr = fake_c.grad.float().to("cuda"), real_c.grad.float().to("cuda")
    got, st = ops.gan_d_loss(fake, real, mask, which, n_fake, n_real)
    (got * 1.5).backward()
    assert abs(float(got) - float(want)) < 1e-6 and abs(float(st[1]) - float((real * mask).sum())) < 1e-5
    assert float((fake.grad / 1.5 - wf).abs().max()) < 1e-7 and float((real.grad / 1.5 - wr).abs().max()) < 1e-7
    got2, _ = ops.gan_d_loss(fake.detach().requires_grad_(True), None, None, which, n_fake, 0)       # no real pair in the step
    assert abs(float(got2) - float(tf.sum() / n_fake)) < 1e-6
    # generator loss
    for norm, alpha, gamma, vis in [("l1", 0.0, 0.0, None), ("l2", 0.3, 0.2, (torch.rand(nb, device="cuda", generator=g) < 0.6).float())]:
        pred = torch.rand(nb, 1, device="cuda", generator=g).requires_grad_(True)
        ff = torch.randn(nb, device="cuda", generator=g).requires_grad_(True)
        t, e = torch.rand(nb, 1, device="cuda", generator=g), (torch.rand(nb, 1, device="cuda", generator=g) < 0.5).float()
        pred_c, ff_c = pred.detach().cpu().double().requires_grad_(True), ff.detach().cpu().double().requires_grad_(True)
        terms = recon_terms(pred_c, t.cpu().double(), e.cpu().double(), alpha, gamma, norm)
        n_vis = 9.0
        reg = (terms if vis is None else terms * vis.cpu().double()).sum() / n_vis
        gen = -ff_c.sum() / n_fake
        want = reg + 0.004 * gen
        want.backward()
        wp, wf = pred_c.grad.float().to("cuda"), ff_c.grad.float().to("cuda")
        got, st = ops.gan_g_loss(pred, ff, t, e, vis, alpha, gamma, norm, 0.004, n_fake, n_vis)
        got.backward()
        assert abs(float(got) - float(want)) < 1e-6 and abs(float(st[1]) - float(reg)) < 1e-6 and abs(float(st[2]) - float(gen)) < 1e-6
        assert float((pred.grad - wp).abs().max()) < 1e-7 and float((ff.grad - wf).abs().max()) < 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("D", [384, 128, 20])
def test_gate_interleave_and_partial_sum(ops, D):
    """Operand layout of the fused gate score: interleaved branch rows (fp32 + planes) + interleaved bias in one launch; the epilogue's
    per-column-block partials summed (+ bc) in one launch."""
    g = torch.Generator(device="cuda").manual_seed(41)
    Wa, Wb = torch.randn(D, D, device="cuda", generator=g), torch.randn(D, D, device="cuda", generator=g)
    ba, bb = torch.randn(D, device="cuda", generator=g), torch.randn(D, device="cuda", generator=g)
    Wi, bi, pl = ops.gate_interleave(Wa, ba, Wb, bb, D, planes=True)
    assert torch.equal(Wi, torch.stack((Wa, Wb), dim=1).reshape(2 * D, D)) and torch.equal(bi, torch.stack((ba, bb), dim=1).reshape(2 * D))
    want = ops.split_planes(Wi)
    assert torch.equal(pl.hi, want.hi) and torch.equal(pl.lo, want.lo)
    assert ops.gate_interleave(Wa, ba, Wb, bb, D)[2] is None
    part = torch.randn(5000, 6, device="cuda", generator=g)
    bc = torch.randn(1, device="cuda", generator=g)
    s = ops.gate_partial_sum(part, bc)
    ref = part.double().sum(dim=1) + bc.double()
    assert float((s.double() - ref).abs().max()) < 1e-6 * (1.0 + float(ref.abs().max()))
    assert float((ops.gate_partial_sum(part).double() - part.double().sum(dim=1)).abs().max()) < 1e-6 * (1.0 + float(ref.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("B,d", [(16, 128), (32, 128), (3, 200), (1, 1)])
@pytest.mark.parametrize("mode", ["instance_x", "bag_x", "instance_y", "none"])
def test_prj_head_fwd_bwd(ops, B, d, mode):
    """out = <u, t> + prj_layer(src) in one launch each way (GANSurv.py:96-105) against the float64 composition on the host; `bag_x`
    passes the same tensor as u and src (autograd sums the two gradients), `instance_y` projects the label embedding."""
    g = torch.Generator(device="cuda").manual_seed(29)
    hx = torch.randn(B, d, device="cuda", generator=g).requires_grad_(True)
    ins = torch.randn(B, d, device="cuda", generator=g).requires_grad_(True)
    ht = torch.randn(B, d, device="cuda", generator=g).requires_grad_(True)
    W = (torch.randn(1, d, device="cuda", generator=g) * 0.3).requires_grad_(True)
    b = torch.randn(1, device="cuda", generator=g).requires_grad_(True)
    wgt = torch.randn(B, 1, device="cuda", generator=g)

    def run(hx, ins, ht, W, b, f):
        u = hx if mode.startswith("bag") else ins
        if mode == "none":
            return f(u, ht, None, None, None)
        return f(u, ht, hx if mode.endswith("_x") else ht, W, b)

    out = run(hx, ins, ht, W, b, ops.prj_head)
    assert out.shape == (B, 1)
    (out * wgt).sum().backward()
    c = [t.detach().cpu().double().requires_grad_(True) for t in (hx, ins, ht, W, b)]
    ref = run(*c, lambda u, t, src, W_, b_: (u * t).sum(-1, keepdim=True) + (0 if src is None else torch.nn.functional.linear(src, W_, b_)))
    (ref * wgt.cpu().double()).sum().backward()
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) < 1e-5 * (1.0 + float(ref.abs().max()))
    for a, r in zip((hx, ins, ht, W, b), c):
        if r.grad is None:
            assert a.grad is None or float(a.grad.abs().max()) == 0.0
            continue
        assert a.grad is not None
        assert float((a.grad.cpu().double() - r.grad).abs().max()) < 1e-5 * (1.0 + float(r.grad.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,N", [(16, 1, 64), (32, 128, 1), (5, 192, 1), (1, 1, 1)])
@pytest.mark.parametrize("act", ["none", "relu"])
def test_skinny_linear_fwd_bwd(ops, B, K, N, act):
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randn(B, K, device="cuda", generator=g).requires_grad_(True)
    W = (torch.randn(N, K, device="cuda", generator=g) * 0.3).requires_grad_(True)
    b = torch.randn(N, device="cuda", generator=g).requires_grad_(True)
    w = torch.randn(B, N, device="cuda", generator=g)
    y = ops.skinny_linear(x, W, b, act)
    (y * w).sum().backward()
    got = (y.detach().clone(), x.grad.clone(), W.grad.clone(), b.grad.clone())
    # reference on the HOST in float64
    xc, Wc, bc_ = (t.detach().cpu().double().requires_grad_(True) for t in (x, W, b))
    ref = torch.nn.functional.linear(xc, Wc, bc_)
    ref = torch.relu(ref) if act == "relu" else ref
    (ref * w.cpu().double()).sum().backward()
    for a, c in zip(got, (ref.detach(), xc.grad, Wc.grad, bc_.grad)):
        assert float((a.cpu().double() - c).abs().max()) < 1e-5 * (1.0 + float(c.abs().max()))


def test_stage_bag_copies_rows_and_derives_or_copies_planes():
    """advmil_stage_bag (ingest of a cached bag into the step slab, one launch): the copy form moves the fp32 rows and both planes; the
    split form (no source planes) derives hi / lo on the way, bit for bit what advmil_split_planes gives; in place (src == dst) it only
    writes the planes; misaligned / inconsistent arguments are refused."""
    import ctypes
    from advmil_amd import _lib, ops
    dev = torch.device("cuda:0")
    x = torch.randn(1040, 1024, device=dev)
    want = ops.split_planes(x)
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    slab = torch.full((2048, 1024), float("nan"), device=dev)
    pl = ops.Planes.alloc((2048, 1024), dev)
    pl.hi.zero_(); pl.lo.zero_()
    a = 512
    nb = x.numel() * 4
    assert L.advmil_stage_bag(slab.data_ptr() + a * 4096, x.data_ptr(), nb, pl.hi.data_ptr() + a * 2048, None, pl.lo.data_ptr() + a * 2048,
                              None, nb // 2, st) == 0
    assert torch.equal(slab[a:a + 1040], x) and torch.isnan(slab[:a]).all() and torch.isnan(slab[a + 1040:]).all()
    assert torch.equal(pl.hi[a:a + 1040].view(torch.int16), want.hi.view(torch.int16))
    assert torch.equal(pl.lo[a:a + 1040].view(torch.int16), want.lo.view(torch.int16))
    assert int(pl.hi[:a].view(torch.int16).abs().max()) == 0 and int(pl.hi[a + 1040:].view(torch.int16).abs().max()) == 0
    # copy form
    slab2 = torch.zeros(1040, 1024, device=dev)
    pl2 = ops.Planes.alloc((1040, 1024), dev)
    assert L.advmil_stage_bag(slab2.data_ptr(), x.data_ptr(), nb, pl2.hi.data_ptr(), want.hi.data_ptr(), pl2.lo.data_ptr(),
                              want.lo.data_ptr(), nb // 2, st) == 0
    assert torch.equal(slab2, x) and torch.equal(pl2.hi.view(torch.int16), want.hi.view(torch.int16))
    assert torch.equal(pl2.lo.view(torch.int16), want.lo.view(torch.int16))
    # in place: planes only
    pl3 = ops.Planes.alloc((1040, 1024), dev)
    assert L.advmil_stage_bag(x.data_ptr(), x.data_ptr(), nb, pl3.hi.data_ptr(), None, pl3.lo.data_ptr(), None, nb // 2, st) == 0
    assert torch.equal(pl3.lo.view(torch.int16), want.lo.view(torch.int16)) and torch.equal(slab2, x)
    EINVAL = -1
    assert L.advmil_stage_bag(slab2.data_ptr(), x.data_ptr(), nb, pl2.hi.data_ptr(), None, pl2.lo.data_ptr(), None, nb // 2 - 16, st) == EINVAL
    assert L.advmil_stage_bag(slab2.data_ptr() + 4, x.data_ptr(), nb - 16, None, None, None, None, 0, st) == EINVAL
    assert L.advmil_stage_bag(slab2.data_ptr(), x.data_ptr(), nb, pl2.hi.data_ptr(), want.hi.data_ptr(), pl2.lo.data_ptr(), None, nb // 2, st) == EINVAL


def test_genconv_on_random_graph_and_without_edges(C=128):
    """(C: the width -- 128 takes the float4 kernels, any other the generic ones; tests/test_poison_kernels_gpu.py calls this with both.)
    The GENConv aggregation on a graph that is not a k-NN grid (random in-degrees, a hub, an isolated node, self loops) against
    float64 -- the kernels only see CSR arrays --, and a graph without edges: out = x, identity gradient (the kernels take no empty
    edge arrays; tools/probe/graph_fuzz.py)."""
    from advmil_amd import ops
    g = torch.Generator().manual_seed(3)
    N, E = 300, 2400
    src = torch.randint(0, N, (E,), generator=g); dst = torch.randint(1, N, (E,), generator=g)      # node 0 receives nothing
    dst[:600] = 7                                                                                      # a hub
    src[600:640] = dst[600:640]                                                                        # self loops
    ei = torch.stack([src, dst])
    x = torch.randn(N, C, generator=g); t = torch.tensor([1.7]); go = torch.randn(N, C, generator=g)
    xd, td = x.clone().to(DEV).requires_grad_(True), t.clone().to(DEV).requires_grad_(True)
    out = ops.genconv_aggregate(xd, td, ops.GraphCSR(ei.to(DEV), N))
    (out * go.to(DEV)).sum().backward()
    xr, tr = x.clone().double().requires_grad_(True), t.clone().double().requires_grad_(True)
    msg = torch.relu(xr[src]) + 1e-7
    z = msg * tr
    zmax = torch.full((N, C), -float("inf"), dtype=torch.float64).scatter_reduce(0, dst[:, None].expand(-1, C), z.detach(), reduce="amax", include_self=True)
    e = torch.exp(z - zmax[dst])
    w = e / torch.zeros(N, C, dtype=torch.float64).index_add_(0, dst, e)[dst]
    orf = torch.zeros(N, C, dtype=torch.float64).index_add_(0, dst, w * msg) + xr
    (orf * go.double()).sum().backward()
    assert relerr(out, orf) < 4e-6 and relerr(xd.grad, xr.grad) < 2e-5
    assert abs(float(td.grad) - float(tr.grad)) < 2e-6 * float((go.double()[dst].abs() * w * msg * (msg + (orf - xr)[dst])).sum())
    assert torch.equal(out[0], xd.detach()[0])                                                        # the isolated node
    x0 = x.clone().to(DEV).requires_grad_(True)
    o0 = ops.genconv_aggregate(x0, td.detach().clone().requires_grad_(True), ops.GraphCSR(torch.zeros(2, 0, dtype=torch.long, device=DEV), N))
    o0.backward(go.to(DEV))
    assert torch.equal(o0.detach(), x0.detach()) and torch.equal(x0.grad, go.to(DEV))


@pytest.mark.parametrize("M,N,K", [(1, 384, 384), (2, 192, 768), (16, 384, 768), (32, 128, 64), (16, 64, 128), (5, 30, 36), (3, 7, 8), (17, 260, 1028)])
@pytest.mark.parametrize("act", ["none", "relu"])
def test_small_linear_kernels_vs_float64_and_vs_the_contraction_path(M, N, K, act):
    """[B <= 32, d] linear layers (csrc/optim.hip small_linear_*: the generator's rho / hop MLP, the discriminator's bag-level MLPs,
    reference model/GANSurv.py:30-49, 89-105): forward and every gradient against float64; with dropout, against the contraction
    engine's epilogue on the same call site (same counter-RNG draw: the masks must coincide element for element)."""
    from advmil_amd import ops
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    x = torch.randn(M, K, generator=g).to(DEV).requires_grad_(True)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).requires_grad_(True)
    b = torch.randn(N, generator=g).to(DEV).requires_grad_(True)
    go = torch.randn(M, N, generator=g).to(DEV)
    assert ops.SMALL_LINEAR
    rows0, ops.SMALL_LINEAR_ROWS = ops.SMALL_LINEAR_ROWS, 32        # (the model path takes these kernels up to SMALL_LINEAR_ROWS rows only)
    y = ops.linear_act(x, W, b, act)
    y.backward(go)
    xd, Wd, bd = (t.detach().double().requires_grad_(True) for t in (x, W, b))
    pre = xd @ Wd.t() + bd
    yr = torch.relu(pre) if act == "relu" else pre
    yr.backward(go.double())
    for got, ref in ((y, yr), (x.grad, xd.grad), (W.grad, Wd.grad), (b.grad, bd.grad)):
        assert float((got.detach().double() - ref.detach()).abs().max()) <= 3e-6 * max(1.0, float(ref.detach().abs().max())), (M, N, K)
    # dropout: the same site drawn by both paths
    outs = []
    for small in (True, False):
        ops.SMALL_LINEAR = small
        try:
            rng = ops.DeviceRng(DEV, seed=77)
            xs, Ws, bs = (t.detach().clone().requires_grad_(True) for t in (x, W, b))
            if not small and (K % 4 or N % 4):
                continue
            yd = ops.linear_act(xs, Ws, bs, act, 0.25, rng, "site")
            yd.backward(go)
            outs.append((yd.detach(), xs.grad, Ws.grad, bs.grad))
        finally:
            ops.SMALL_LINEAR = True
    ops.SMALL_LINEAR_ROWS = rows0
    if len(outs) == 2:
        assert float((outs[0][0] == 0).float().mean()) > 0.1                       # something was dropped
        assert bool(((outs[0][0] == 0) == (outs[1][0] == 0)).all()) or act == "relu"      # (relu zeros coincide too, up to round-off at 0)
        for a, c in zip(outs[0], outs[1]):
            assert float((a - c).abs().max()) <= 2e-5 * max(1.0, float(c.abs().max()))


@pytest.mark.gpu
def test_clock_stamps_bracket_a_launch_inside_a_captured_graph(ops):
    """bench.py's in-step timing (ops.Stamps / advmil_stamp_clock): one-thread kernels that write the device wall clock are ordinary graph
    nodes; a pair around a contraction inside a captured graph reads back a duration in the range HIP events give for the same launch
    back to back, on every replay."""
    M, N, K = 8192, 384, 1024
    g = torch.Generator(device="cuda").manual_seed(3)
    A = torch.randn(M, K, device="cuda", generator=g)
    B = torch.randn(N, K, device="cuda", generator=g)
    out = torch.empty(M, N, device="cuda")
    for _ in range(3):
        ops.gemm(A, B, True, True, M, N, K, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        ops.gemm(A, B, True, True, M, N, K, out=out)
    e1.record()
    torch.cuda.synchronize()
    ref_us = e0.elapsed_time(e1) * 100.0
    st = ops.Stamps(A.device, cap=16)
    assert st.khz > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            st.mark(("b", "gemm", (M, N, K, 1), 2.0 * M * N * K))
            ops.gemm(A, B, True, True, M, N, K, out=out)
            st.mark(("e", "gemm", (M, N, K, 1), 2.0 * M * N * K))
    seen = []
    for _ in range(4):
        graph.replay()
        torch.cuda.synchronize()
        (name, shape, flops, us), = st.durations_us()
        assert name == "gemm" and shape == (M, N, K, 1)
        seen.append(us)
    assert all(0.5 * ref_us < u < 3.0 * ref_us + 20.0 for u in seen), (seen, ref_us)


@pytest.mark.gpu
def test_segmented_row_mean_backward_is_one_launch_and_exact(ops):
    """ops.segmented_mean_rows (the per-bag mean of the region features, projection discriminator RLIP): forward against torch, backward
    dh[n] = dpooled[seg(n)] / len(seg) through advmil_seg_scale_rows -- equal to the index_select * weight form it replaces."""
    lens = [512, 16, 1040, 256]
    seg = ops.Segments(lens, torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(2)
    h = torch.randn(sum(lens), 128, device="cuda", generator=g, requires_grad=True)
    go = torch.randn(len(lens), 128, device="cuda", generator=g)
    out = ops.segmented_mean_rows(h, seg)
    out.backward(go)
    want, wantg, r0 = [], torch.empty_like(h), 0
    for i, n in enumerate(lens):
        want.append(h.detach()[r0:r0 + n].double().mean(0))
        wantg[r0:r0 + n] = go[i] * (1.0 / n)
        r0 += n
    assert float((out.detach().double() - torch.stack(want)).abs().max()) < 2e-6
    assert float((h.grad - wantg).abs().max()) <= 1e-7 * float(wantg.abs().max()) + 1e-12
