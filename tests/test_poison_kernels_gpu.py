"""GPU: every kernel family at its ragged edge under allocation poisoning (tests/poison.py; DESIGN.md section 2, "Allocation poisoning").

Each case is one direct call into advmil_amd.ops -- forward and backward where the op has one -- at the smallest shapes where the
launched work exceeds the real work (ragged bags under a grid sized by the longest one, sizes that are no multiple of the tile, split-K
partial slabs, per-block partial rows), run four times: plain, plain again, with every fresh allocation filled with 0xFF (NaN / -1)
and with 0x7F (3.39e38 / 2139062143). Asserted:

  (a) plain == plain, bit for bit (determinism; the precondition of (b));
  (b) both poisoned runs == plain, bit for bit, on every returned tensor, gradient, emitted plane and saved statistic;
  (c) everything is finite;
  (d) under 0xFF the op agrees with its float64 restatement at the tolerance its family's own test asserts: where that restatement
      lives inside a test function of test_kernels_gpu / test_attention_gpu / test_cindex, the function itself is called with this
      module's shapes while the allocations are poisoned (`under_ff`); `_run` / `_ref64` of the fused small networks are imported.
      No tolerance is introduced here.

A case that is not run-to-run deterministic ((a) fails), or whose result moves with the pattern, is a finding: it is named here with
the read or the unwritten element and its fix, and stays in the suite. Found so far: none by the poisoning (every case passed when the module was introduced, and the row-kernel walks added later did too). The
float64 bodies those walks share with tests/test_row_walks_gpu.py found one fault of their own, named there: LayerNorm rows with a mean
large against their spread missed the 1e-5 output bound; fixed in csrc/pool.hip (ln_recentre)."""
import ctypes

import numpy as np
import pytest
import torch

from advmil_amd import synth
from tests import helpers as H
from tests import poison as P
from tests import test_attention_gpu as TA
from tests import test_attn_walks_gpu as TAW
from tests import test_gemm_walks_gpu as TW
from tests import test_genconv_gpu as TG
from tests import test_kernels_gpu as TK
from tests import test_row_walks_gpu as TR
from tests.test_kernels_gpu import relerr, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import ops as _ops
    from advmil_amd import _lib
    _lib.lib()
    return _ops


class gemm_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from advmil_amd import ops
        self.prev = ops.get_gemm_mode()
        ops.set_gemm_mode(self.mode)

    def __exit__(self, *exc):
        from advmil_amd import ops
        ops.set_gemm_mode(self.prev)
        return False


def runs(fn):
    """(a), (b), (c); -> the 0xFF run's result tree for (d)."""
    trees = P.three_runs(fn)
    P.assert_same_bits(trees)
    for t in trees:
        P.assert_finite(t)
    return trees[2]


def under_ff(test_fn, *args, **kw):
    """(d) through a family's own float64 test body, its allocations poisoned."""
    with P.poisoned_allocations(P.NAN_BYTE):
        return test_fn(*args, **kw)


def dev(*ts):
    return [t.to(DEV) for t in ts]


GEMM_TOL = {"exact": 2e-6, "bf16x3": 1.5e-5}            # test_gemm_layouts / test_gemm_split_bf16x3_mode


# ------------------------------------------------------------------------------------------------------------------------------
# generic contraction
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "bf16x3"])
@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, False), (False, True)])
@pytest.mark.parametrize("M,N,K", [(260, 196, 36), (200, 72, 100)])
def test_gemm_layouts_and_split_k(ops, mode, a_kc, b_kc, M, N, K):
    A = rnd(f"A{M}{K}", M, K); B = rnd(f"B{K}{N}", K, N)
    ref = A.double() @ B.double()
    Ad = (A if a_kc else A.t().contiguous()).to(DEV)
    Bd = (B.t().contiguous() if b_kc else B).to(DEV)
    C0 = rnd(f"C{M}{N}", M, N).to(DEV)

    def fn():
        out = {sp: ops.gemm(Ad, Bd, a_kc, b_kc, M, N, K, splits=sp) for sp in (1, 3)}
        for sp in (1, 3):                                        # accumulate=True: C0 += A B through the split-K workspace
            acc = C0.clone()
            ops.gemm(Ad, Bd, a_kc, b_kc, M, N, K, out=acc, ldc=N, accumulate=True, splits=sp)
            out[f"acc{sp}"] = acc
        return out
    with gemm_mode(mode):
        got = runs(fn)
    for sp in (1, 3):
        assert relerr(got[sp], ref) < GEMM_TOL[mode], (sp, relerr(got[sp], ref))
        assert relerr(got[f"acc{sp}"], ref + C0.cpu().double()) < GEMM_TOL[mode], sp


@pytest.mark.parametrize("splits", [1, 3])
def test_gemm_emits_the_planes_of_its_result(ops, splits):
    M, N, K = 260, 196, 36
    A, B, bias = dev(rnd("pA", M, K), rnd("pB", N, K), rnd("pb", N))

    def fn():
        cp = ops.Planes.alloc((M, N), A.device)
        C = ops.gemm(A, B, True, True, M, N, K, bias=bias, act0=1, splits=splits, c_planes=cp)
        return C, cp
    with gemm_mode("bf16x3"):
        C, cp = runs(fn)
        want = ops.split_planes(C)
    assert torch.equal(cp["hi"], want.hi) and torch.equal(cp["lo"], want.lo)
    assert relerr(C, torch.relu(A.cpu().double() @ B.cpu().double().t() + bias.cpu().double())) < GEMM_TOL["bf16x3"]


@pytest.mark.parametrize("mode", ["exact", "bf16x3"])
@pytest.mark.parametrize("splits", [1, 3])
def test_gemm_strided_output_stays_inside_its_block(ops, mode, splits):
    """out = buf[:, 32:64] of a fresh [64, 96] buffer: the block equals the plain run's, and the 64 columns outside it still hold the
    pattern byte exactly -- the poison reached device memory, and the kernel (split-K reduce included) stays inside its block."""
    M, N, K = 64, 32, 64
    A, W = dev(rnd("sA", M, K), rnd("sW", N, K))
    ref = A.cpu().double() @ W.cpu().double().t()

    def fn():
        buf = torch.empty(M, 96, device=DEV)
        ops.gemm(A, W, True, True, M, N, K, out=buf[:, 32:64], ldc=96, splits=splits)
        return buf
    with gemm_mode(mode):
        plain = [fn()[:, 32:64].clone() for _ in range(2)]
        assert torch.equal(plain[0], plain[1])
        for byte in P.PATTERNS:
            with P.poisoned_allocations(byte):
                buf = fn()
            assert torch.equal(buf[:, 32:64], plain[0]) and bool(torch.isfinite(buf[:, 32:64]).all()), byte
            raw = buf.view(torch.uint8).reshape(M, 96, 4)
            assert bool((raw[:, :32] == byte).all()) and bool((raw[:, 64:] == byte).all()), byte
            if byte == P.NAN_BYTE:
                assert relerr(buf[:, 32:64], ref) < GEMM_TOL[mode]


@pytest.mark.parametrize("mode", ["exact", "bf16x3"])
def test_gemm_dropout_epilogue(ops, mode):
    M, N, K, p = 200, 72, 100, 0.25
    A, W = dev(rnd("dA", M, K), rnd("dW", N, K))
    rng = ops.DeviceRng(DEV, seed=1234)
    sid = rng.site("t")
    with gemm_mode(mode):
        got = runs(lambda: {sp: ops.gemm(A, W, True, True, M, N, K, act0=1, drop_p=p, seed=rng.seed, stream_id=sid, splits=sp) for sp in (1, 3)})
    keep = synth.dropout_keep(1234, sid, M * N, p).reshape(M, N)
    ref = torch.relu(A.cpu().double() @ W.cpu().double().t()) * H.T(keep).double() / (1 - p)
    for sp in (1, 3):
        assert relerr(got[sp], ref) < GEMM_TOL[mode], sp


@pytest.mark.parametrize("mode", ["exact", "bf16x3"])
def test_gemm_fused_gate_score_partials(ops, mode):
    """gate_wc mode at 1000 rows (no multiple of any tile): the per-column-block partial scores; (d) = test_gemm_fused_gate_score."""
    g = torch.Generator(device="cuda").manual_seed(21)
    N, D = 1000, 384
    h = torch.randn(N, D, device="cuda", generator=g)
    Wi = torch.randn(2 * D, D, device="cuda", generator=g) * 0.05
    bi = torch.randn(2 * D, device="cuda", generator=g) * 0.1
    wc = torch.randn(D, device="cuda", generator=g) * 0.1
    with gemm_mode(mode):
        runs(lambda: {t: ops.gemm(h, Wi, True, True, N, 2 * D, D, bias=bi, gate_wc=wc, tile=t) for t in (0, 22, 11)})
    for tile in (0, 22, 11):
        under_ff(TK.test_gemm_fused_gate_score, ops, mode, tile)


# ------------------------------------------------------------------------------------------------------------------------------
# 8-wave tiles, plane-fed NT / TN, grouped TN, deferred merges
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [43, 42, 34, 24])
def test_gemm_eight_wave_tiles(ops, tile):
    M, N, K = 520, 200, 1032
    g = torch.Generator(device="cuda").manual_seed(11)
    with gemm_mode("bf16x3"):
        for a_kc, b_kc in [(True, True), (True, False), (False, False), (False, True)]:
            A = torch.randn((M, K) if a_kc else (K, M), device="cuda", generator=g)
            B = torch.randn((N, K) if b_kc else (K, N), device="cuda", generator=g)
            bias = torch.randn(N, device="cuda", generator=g)
            got = runs(lambda: (ops.gemm(A, B, a_kc, b_kc, M, N, K, bias=bias, act0=1, tile=tile),
                                ops.gemm(A, B, a_kc, b_kc, M, N, K, splits=3, tile=tile)))
            A64, B64 = A.cpu().double(), B.cpu().double()
            pre = (A64 if a_kc else A64.t()) @ (B64.t() if b_kc else B64)
            assert relerr(got[0], torch.relu(pre + bias.cpu().double())) < 2e-5 and relerr(got[1], pre) < 2e-5       # test_gemm_bf16x3_eight_wave_tiles


@pytest.mark.parametrize("tile", [82, 83])
def test_plane_fed_nt_tiles(ops, tile):
    """768 x 768 x 96 with the planes of the result, and with the per-bag rank-1 term (tolerance: test_gemm_streaming_epilogue_modes)."""
    M, N, K = 768, 768, 96
    g = torch.Generator(device="cuda").manual_seed(5)
    A = 0.1 * torch.randn(M, K, device="cuda", generator=g); W = torch.randn(N, K, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    rowv = torch.randn(M, device="cuda", generator=g); colv = torch.randn(4, N, device="cuda", generator=g)
    rowseg = torch.arange(M, device="cuda", dtype=torch.int32) // (M // 4)
    pre = A.cpu().double() @ W.cpu().double().t()
    with gemm_mode("bf16x3"):
        kw = dict(a_planes=ops.split_planes(A), b_planes=ops.split_planes(W), tile=tile, splits=1)

        def fn():
            cp = ops.Planes.alloc((M, N), A.device)
            y = ops.gemm(A, W, True, True, M, N, K, bias=bias, act0=2, act1=3, act_split=384, alpha=0.5, c_planes=cp, **kw)
            return y, cp, ops.gemm(A, W, True, True, M, N, K, rowv=rowv, colv=colv, rowseg=rowseg, **kw)
        y, cp, r1 = runs(fn)
        want = ops.split_planes(y)
    assert torch.equal(cp["hi"], want.hi) and torch.equal(cp["lo"], want.lo)
    z = 0.5 * pre + bias.cpu().double()
    assert relerr(y, torch.cat([torch.tanh(z[:, :384]), torch.sigmoid(z[:, 384:])], dim=1)) < 3e-5
    assert relerr(r1, pre + rowv.cpu().double()[:, None] * colv.cpu().double()[rowseg.cpu().long()]) < 3e-5


@pytest.mark.parametrize("M,want_tile", [(16384, 86), (65536, 85)])
def test_plane_fed_two_layer_launch(ops, M, want_tile):
    K, N1, N2 = 256, 384, 128
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(M, K, device="cuda", generator=g)
    W1 = 0.1 * torch.randn(N1, K, device="cuda", generator=g); W2 = 0.1 * torch.randn(N2, K, device="cuda", generator=g)
    b1 = torch.randn(N1, device="cuda", generator=g); b2 = torch.randn(N2, device="cuda", generator=g)
    with gemm_mode("bf16x3"):
        assert ops.gemm_two_layers_tile(M, N1, N2, K) == want_tile
        xpl, p1, p2 = ops.split_planes(x), ops.split_planes(W1), ops.split_planes(W2)
        y1, y2, cpl = runs(lambda: ops.gemm_two_layers(x, xpl, W1, p1, b1, 1, W2, p2, b2, 0, True))
        want = ops.split_planes(y1)
    assert torch.equal(cpl["hi"], want.hi) and torch.equal(cpl["lo"], want.lo)
    rows = torch.arange(0, M, 997, device="cuda")
    x64 = x[rows].cpu().double()
    assert relerr(y1[rows], torch.relu(x64 @ W1.cpu().double().t() + b1.cpu().double())) < 2e-5      # test_gemm_two_layers_in_one_launch
    assert relerr(y2[rows], x64 @ W2.cpu().double().t() + b2.cpu().double()) < 2e-5


@pytest.mark.parametrize("M,N,K,forced", [(256, 256, 8192 + 96, (93, 4)), (768, 384, 16384, None)])
def test_plane_fed_tn(ops, M, N, K, forced):
    g = torch.Generator(device="cuda").manual_seed(11)
    A = torch.randn(K, M, device="cuda", generator=g)
    B = torch.randn(K, N, device="cuda", generator=g)
    base = torch.randn(M, N, device="cuda", generator=g)
    with gemm_mode("bf16x3"):
        tile, sp = forced or ops.gemm_plan_tn_planes(M, N, K)
        assert tile in (91, 92, 93) and sp >= 1, (tile, sp)
        pa, pb = ops.split_planes(A), ops.split_planes(B)

        def fn():
            plain = ops.gemm(None, B, False, False, M, N, K, a_planes=pa, b_planes=pb, tile=tile, splits=sp)
            acc = base.clone()
            ops.gemm(None, B, False, False, M, N, K, out=acc, ldc=N, accumulate=True, a_planes=pa, b_planes=pb, tile=tile, splits=sp)
            return plain, acc
        plain, acc = runs(fn)
    want = A.double().t() @ B.double()
    assert float((plain.double() - want).abs().max()) <= 2e-5 * float(want.abs().max())              # test_gemm_tn_planes_kernel_...
    assert float((acc.double() - want - base.double()).abs().max()) <= 2e-5 * float(want.abs().max())


@pytest.mark.parametrize("mode", ["bf16x3", "exact"])
@pytest.mark.parametrize("defer", [False, True])
def test_grouped_tn_launch(ops, mode, defer):
    K = 512
    g = torch.Generator().manual_seed(K)
    shapes = [(256, 128), (128, 64), (64, 128), (68, 36)]
    AB = [(torch.randn(K, M, generator=g).to(DEV), torch.randn(K, N, generator=g).to(DEV)) for (M, N) in shapes]
    base = [torch.randn(M, N, generator=g).to(DEV) for (M, N) in shapes]
    acc = [True, True, False, True]

    def fn():
        got = [c.clone() for c in base]
        calls = [(A, B, o, a) for (A, B), o, a in zip(AB, got, acc)]
        if defer:
            with ops.deferred_sums():
                ops.gemm_tn_group(calls)
        else:
            ops.gemm_tn_group(calls)
        return got
    with gemm_mode(mode):
        got = runs(fn)
    for o, (A, B), c0, a in zip(got, AB, base, acc):
        ref = A.double().t() @ B.double() + (c0.double() if a else 0)
        assert float((o.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())               # test_group_launch_equals_the_plain_launches


def test_deferred_split_k_merge_reads_its_kept_workspace_at_the_flush(ops):
    """A split-K weight gradient queued inside deferred_sums(): its partials sit in a kept workspace until the exit's flush, with other
    workspaces handed out in between."""
    from advmil_amd import _lib
    M, N, K = 128, 64, 16384
    g = torch.Generator(device=DEV).manual_seed(3)
    a = torch.randn(K, M, device=DEV, generator=g); b = torch.randn(K, N, device=DEV, generator=g)
    base = torch.randn(M, N, device=DEV, generator=g)
    x = torch.randn(4096, 64, device=DEV, generator=g)

    def fn():
        o = base.clone()
        cs = torch.zeros(64, device=DEV)
        ops.ARENA_STORAGES.add(o.untyped_storage().data_ptr())
        try:
            with ops.deferred_sums():
                ops.gemm(a, b, False, False, M, N, K, out=o, ldc=N, accumulate=True)
                assert _lib.lib().advmil_pending_sums(ops._stream()) == 1
                ops.colsum(x, 4096, 64, out=cs)                  # a second queued merge with a workspace of its own
                fresh = ops.colsum(x, 4096, 64)                  # and an undeferred one in between
        finally:
            ops.ARENA_STORAGES.discard(o.untyped_storage().data_ptr())
        return o, cs, fresh
    with gemm_mode("bf16x3"):
        assert ops.gemm_plan(M, N, K, False, False)[1] > 1
        o, cs, fresh = runs(fn)
        o1 = base.clone()
        ops.gemm(a, b, False, False, M, N, K, out=o1, ldc=N, accumulate=True)
    assert torch.equal(o, o1)                                    # test_split_k_weight_gradient_goes_through_the_queue
    assert relerr(fresh, x.double().sum(0)) < 1e-5
    ref = base.double() + a.double().t() @ b.double()
    assert float((o.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())                    # (the split-K bound of the grouped / TN tests)
    assert relerr(cs, x.double().sum(0)) < 1e-5                                                      # test_colsum_and_abs_sum_and_uniform


# ------------------------------------------------------------------------------------------------------------------------------
# segmented pooling
# ------------------------------------------------------------------------------------------------------------------------------
POOL_LENS = [513, 1, 4096, 77]


@pytest.mark.parametrize("D", [128, 384])
@pytest.mark.parametrize("lens,cap", [(POOL_LENS, None), (POOL_LENS, 8192), (POOL_LENS + [3600], 8192)], ids=["own", "cap_total", "cap_8192"])
def test_segmented_softmax_pooling(ops, D, lens, cap):
    """softmax_pool, softmax_pool_mean, the planes form and the backward on ragged bags under a grid sized by the longest one; `cap`:
    seg.max_len raised by hand to min(total rows, 8192), as StaticStepPlan.bag_cap does, so the grid exceeds even the longest bag (the
    library refuses a max_len above the row total: on the 4 687 rows of POOL_LENS the cap is the total, 591 rows past the longest bag;
    with a fifth bag the slab admits the full 8192)."""
    N, nb = sum(lens), len(lens)
    g = torch.Generator().manual_seed(1)
    h = torch.randn(N, D, generator=g).to(DEV)
    s = (3.0 * torch.randn(N, generator=g)).to(DEV)
    dp = torch.randn(nb, D, generator=g).to(DEV)
    dA = torch.randn(N, generator=g).to(DEV)
    seg = ops.Segments(lens, DEV)
    if cap:
        seg.max_len = min(N, cap)
        assert seg.max_len > max(lens)
    hpl = ops.split_planes(h)

    def fn():
        A, pooled = ops.softmax_pool(s, h, N, D, seg)
        A1, p1, m1 = ops.softmax_pool_mean(s, h, N, D, seg)
        A2, p2 = ops.softmax_pool(s, h, N, D, seg, hpl)
        return dict(A=A, pooled=pooled, A1=A1, p1=p1, mean=m1, A2=A2, p2=p2, ds=ops.softmax_pool_bwd(dp, dA, A, h, N, D, seg),
                    ds2=ops.softmax_pool_bwd(dp, dA, A2, h, N, D, seg, hpl))
    r = runs(fn)
    assert torch.equal(r["A"], r["A1"]) and torch.equal(r["pooled"], r["p1"]) and torch.equal(r["A"], r["A2"])   # test_pooling_with_the_mean_..., test_pooling_from_planes_...

    def ref(h64):
        s64 = s.double().requires_grad_(True)
        o, Ar, pr, mr = 0, [], [], []
        for n in lens:
            a = torch.softmax(s64[o:o + n], 0)
            Ar.append(a); pr.append(a @ h64[o:o + n]); mr.append(h64[o:o + n].mean(0))
            o += n
        Ar, pr = torch.cat(Ar), torch.stack(pr)
        ((pr * dp.double()).sum() + (Ar * dA.double()).sum()).backward()
        return Ar.detach(), pr.detach(), torch.stack(mr), s64.grad
    Ad, pref, mref, dsref = ref(h.double())
    _, pref2, _, dsref2 = ref(ops.planes_f32(hpl).double())       # what the plane-fed form sees: hi + lo
    assert float(((r["A"].double() - Ad).abs() / Ad).max()) < 2e-5                                 # test_softmax_pool_and_layernorm_every_entry_at_slab_size
    assert float((r["pooled"].double() - pref).abs().max()) < 1e-5
    assert float((r["p2"].double() - pref2).abs().max()) < 2e-6                            # test_pooling_from_planes_equals_pooling_of_hi_plus_lo
    assert float((r["mean"].double() - mref).abs().max()) <= 1e-5 * float(mref.abs().max()) + 1e-7   # test_pooling_with_the_mean_from_the_same_pass
    assert relerr(r["ds"], dsref) < 5e-5 and relerr(r["ds2"], dsref2) < 5e-5                        # the gradient bound of test_gated_pool_fwd_bwd


# ------------------------------------------------------------------------------------------------------------------------------
# row kernels
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(37, 384), (1000, 128)])
def test_gated_attention_pool(ops, N, D):
    p = 0.25
    h = rnd(f"gh{N}", N, D); Wa = rnd("gWa", D, D, scale=0.05); Wb = rnd("gWb", D, D, scale=0.05)
    ba = rnd("gba", D, scale=0.1); bb = rnd("gbb", D, scale=0.1); wc = rnd("gwc", 1, D, scale=0.3); bc = rnd("gbc", 1)
    gp, gA = dev(rnd("ggp", D), rnd("ggA", N))

    def fn():
        leaves = [t.clone().to(DEV).requires_grad_(True) for t in (h, Wa, ba, Wb, bb, wc, bc)]
        pooled, A, s = ops.gated_attn_pool(*leaves, p=p, rng=ops.DeviceRng(DEV, seed=77))
        (pooled * gp).sum().add((A * gA).sum()).backward()
        return pooled, A, s, [t.grad for t in leaves]
    runs(fn)
    under_ff(TK.test_gated_pool_fwd_bwd, ops, N, D, p)


@pytest.mark.parametrize("N,D", [(37, 384), (1000, 128)])
def test_gate_score_and_gate_backward(ops, N, D):
    p = 0.25
    g = torch.Generator().manual_seed(N)
    ab = torch.cat([torch.tanh(torch.randn(N, D, generator=g)), torch.sigmoid(torch.randn(N, D, generator=g))], dim=1).to(DEV)
    wc, bc, ds = dev(0.3 * torch.randn(D, generator=g), torch.randn(1, generator=g), torch.randn(N, generator=g))
    seed = torch.tensor([77], dtype=torch.int64, device=DEV)

    def fn():
        s = ops.gate_score(ab, wc, bc, N, D, p, seed, 1, 2)
        pl = ops.Planes.alloc((N, 2 * D), ab.device)
        dG, dwc, dbc, dbias = ops.gate_bwd(ab, ds, wc, N, D, p, seed, 1, 2, planes=pl)
        acc = [torch.ones(D, device=DEV), torch.ones(1, device=DEV), torch.ones(2 * D, device=DEV)]
        ops.gate_bwd(ab, ds, wc, N, D, p, seed, 1, 2, dwc=acc[0], dbc=acc[1], dbias=acc[2], planes=ops.Planes.alloc((N, 2 * D), ab.device), planes_only=True)
        return s, dG, dwc, dbc, dbias, pl, acc
    s, dG, dwc, dbc, dbias, pl, acc = runs(fn)
    ma = H.T(synth.dropout_keep(77, 1, N * D, p).reshape(N, D)).double() / (1 - p)
    mb = H.T(synth.dropout_keep(77, 2, N * D, p).reshape(N, D)).double() / (1 - p)
    a64, b64 = ab.cpu().double()[:, :D] * ma, ab.cpu().double()[:, D:] * mb
    assert relerr(s, (a64 * b64) @ wc.cpu().double() + bc.cpu().double()) < 1e-5                    # test_gated_pool_fwd_bwd's score bound
    want = ops.split_planes(dG)
    assert torch.equal(pl["hi"], want.hi) and torch.equal(pl["lo"], want.lo)
    for got, plain in zip(acc, (dwc, dbc, dbias)):                                                   # the accumulating form adds the same sums
        assert relerr(got - 1.0, plain) < 5e-5


@pytest.mark.parametrize("M,N", [(517, 128), (33, 1056)])
def test_activation_dropout_backward(ops, M, N):
    """fp32 form, planes-only form, the bit mask and the column sums (whose per-block partial rows a ragged M leaves part-filled)."""
    p = 0.25
    g = torch.Generator().manual_seed(17)
    dy = torch.randn(M, N, generator=g).to(DEV)
    y = torch.relu(torch.randn(M, N, generator=g)).to(DEV)
    seed = torch.tensor([77], dtype=torch.int64, device=DEV)

    def fn():
        dpre, db0 = ops.act_dropout_bwd(dy, y, ops.ACT_RELU, M, N, p, seed, 5)
        pl = ops.Planes.alloc((M, N), dy.device)
        none, db1 = ops.act_dropout_bwd(dy, y, ops.ACT_RELU, M, N, p, seed, 5, planes=pl, planes_only=True)
        assert none is None
        acc = torch.ones(N, device=DEV)
        ops.act_dropout_bwd(dy, y, ops.ACT_RELU, M, N, p, seed, 5, db_out=acc)
        bits = torch.empty(M, N // 32, dtype=torch.int32, device=DEV)
        yd, _ = ops.act_dropout_bwd(y, y, ops.ACT_NONE, M, N, p, seed, 3, want_bias=False, bits=bits)
        return dict(dpre=dpre, db0=db0, db1=db1, pl=pl, acc=acc, bits=bits, yd=yd)
    r = runs(fn)
    keep = H.T(synth.dropout_keep(77, 5, M * N, p).reshape(M, N)).double() / (1 - p)
    ref = dy.cpu().double() * (y.cpu() > 0) * keep
    assert relerr(r["dpre"], ref) < 5e-5 and relerr(r["db0"], ref.sum(0)) < 5e-5                    # test_linear_act_autograd's gradient bound
    want = ops.split_planes(r["dpre"])
    assert torch.equal(r["pl"]["hi"], want.hi) and torch.equal(r["pl"]["lo"], want.lo) and torch.equal(r["db0"], r["db1"])
    assert relerr(r["acc"] - 1.0, r["db0"]) < 5e-5
    b = r["bits"].cpu().numpy().view("uint32")
    un = ((b[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(M, N).astype(bool)
    assert (un == (r["yd"].cpu().numpy() > 0)).all()                                                # test_dropout_pass_leaves_the_keep_mask_...


def test_colsum_dropout_planes_and_segment_row_scaling(ops):
    g = torch.Generator().manual_seed(8)
    x = rnd("cx", 1000, 2048).to(DEV)
    x2 = torch.randn(517, 128, generator=g).to(DEV)
    M, N = 1000, 128
    y0 = ops.planes_f32(ops.split_planes(torch.randn(M, N, generator=g).relu_().to(DEV)))          # values that ARE hi + lo
    pl = ops.split_planes(y0)
    seed = torch.tensor([21], dtype=torch.int64, device=DEV)
    rr = torch.randperm(M, generator=g).to(DEV)
    lens = [512, 16, 1040, 256, 1]
    seg = ops.Segments(lens, DEV)
    h0 = torch.randn(sum(lens), 128, generator=g).to(DEV)
    go = torch.randn(len(lens), 128, generator=g).to(DEV)

    def fn():
        acc = torch.ones(128, device=DEV)
        ops.colsum(x2, 517, 128, out=acc)
        tpl, tbits = ops.dropout_planes(pl, M, N, 0.25, seed, 5, rr)
        _, _, gb = ops.dropout_planes(pl, M, N, 0.25, seed, 5, None, gate=(0.25, 6, 7))
        h = h0.clone().requires_grad_(True)
        out = ops.segmented_mean_rows(h, seg)
        out.backward(go)
        return dict(c=ops.colsum(x, 1000, 2048), c2=ops.colsum(x2, 517, 128), acc=acc, a=ops.abs_sum(x.reshape(-1)), tpl=tpl, tbits=tbits,
                    gb=list(gb), mean=out, dh=h.grad)
    r = runs(fn)
    assert relerr(r["c"], x.double().sum(0)) < 1e-5 and relerr(r["c2"], x2.double().sum(0)) < 1e-5   # test_colsum_and_abs_sum_and_uniform
    assert relerr(r["acc"] - 1.0, x2.double().sum(0)) < 1e-5 and relerr(r["a"], x.double().abs().sum().reshape(1)) < 1e-5
    rpl = ops.Planes.alloc((M, N), DEV)                                                             # test_dropout_of_planes_equals_the_fp32_replay
    rbits = torch.empty(M, N // 32, dtype=torch.int32, device=DEV)
    ops.act_dropout_bwd(y0, y0, ops.ACT_NONE, M, N, 0.25, seed, 5, want_bias=False, planes=rpl, bits=rbits, rng_row=rr)
    assert torch.equal(r["tpl"]["hi"], rpl.hi) and torch.equal(r["tpl"]["lo"], rpl.lo) and torch.equal(r["tbits"], rbits)
    want, wantg, r0 = [], torch.zeros_like(h0), 0
    for i, n in enumerate(lens):
        want.append(h0[r0:r0 + n].double().mean(0)); wantg[r0:r0 + n] = go[i] * (1.0 / n)
        r0 += n
    assert float((r["mean"].double() - torch.stack(want)).abs().max()) < 2e-6                        # test_segmented_row_mean_backward_...
    assert float((r["dh"] - wantg).abs().max()) <= 1e-7 * float(wantg.abs().max()) + 1e-12


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(16, 200), (64, 384), (512, 128), (48, 256), (32, 512)])
def test_ln_relu_mean16(ops, N, d):
    y = rnd(f"ly{N}{d}", N, d).to(DEV); gm = (1 + 0.1 * rnd("lg", d)).to(DEV); bt = (0.1 * rnd("lb", d)).to(DEV)
    ge = rnd("le", N // 16, d).to(DEV)
    dup_ok = ops.ln_relu_mean16_dup_ok(d)

    def fn():
        out = {}
        for name, kw in (("plain", {}), ("ycol", dict(ycol_grad=torch.full((d,), 0.5, device=DEV)))) + ((("dup", dict(dup=2)),) if dup_ok else ()):
            lv = [t.clone().requires_grad_(True) for t in (y, gm, bt)]
            emb = ops.ln_relu_mean16(*lv, **kw)
            gg = torch.cat([ge, ge]) if name == "dup" else ge
            (emb * gg).sum().backward()
            out[name] = [emb, [t.grad for t in lv], kw.get("ycol_grad")]
        emb, mean, rstd = ops.ln_relu_mean16_fwd(y, gm, bt, N, d, 1e-5)
        pl = ops.Planes.alloc((N, d), y.device)
        yc = torch.zeros(d, device=DEV)
        _, dg1, db1 = ops.ln_relu_mean16_bwd(ge, y, gm, bt, mean, rstd, N, d, ycol_out=yc, planes=pl)
        out["planes"] = [emb, mean, rstd, pl, dg1, db1, yc]
        return out
    r = runs(fn)
    assert torch.equal(r["ycol"][1][0], r["plain"][1][0])
    want = ops.split_planes(r["plain"][1][0])                                                        # test_layernorm_backward_hands_dy_over_as_operand_planes
    assert torch.equal(r["planes"][3]["hi"], want.hi) and torch.equal(r["planes"][3]["lo"], want.lo)
    if dup_ok:                                                                                       # [emb; emb], the backward sums the halves: 2 x the gradients
        assert torch.equal(r["dup"][0][:N // 16], r["plain"][0]) and torch.equal(r["dup"][0][N // 16:], r["plain"][0])
        assert relerr(r["dup"][1][0], 2.0 * r["plain"][1][0]) < 5e-5
    under_ff(TK.test_ln_relu_mean16, ops, N, d)


def test_ln_relu_rows_and_add_dropout_layer_norm(ops):
    N, d = 37, 256
    y = rnd("lr", N, d).to(DEV); gm = (1 + 0.1 * rnd("lrg", d)).to(DEV); bt = (0.1 * rnd("lrb", d)).to(DEV); go = rnd("lro", N, d).to(DEV)

    def fn():
        lv = [t.clone().requires_grad_(True) for t in (y, gm, bt)]
        out = ops.ln_relu(*lv)
        (out * go).sum().backward()
        res = {"ln_relu": [out, [t.grad for t in lv]]}
        for R, dd in ((37, 128), (210, 384)):
            x, o, gy = dev(TA.rnd(f"lx{R}", R, dd), TA.rnd(f"lo{R}", R, dd), TA.rnd(f"lg{R}", R, dd))
            ga, ba = (1.0 + 0.1 * TA.rnd("lgam", dd)).to(DEV), (0.05 * TA.rnd("lbet", dd)).to(DEV)
            lv = [t.clone().requires_grad_(True) for t in (x, o, ga, ba)]
            yy = ops.add_dropout_layer_norm(*lv, 1e-5, 0.25, ops.DeviceRng(DEV, seed=9), "ln_site")
            (yy * gy).sum().backward()
            res[(R, dd)] = [yy, [t.grad for t in lv]]
        return res
    r = runs(fn)
    rv = [t.cpu().double().requires_grad_(True) for t in (y, gm, bt)]
    z = torch.relu(torch.nn.functional.layer_norm(rv[0], (d,), rv[1], rv[2], 1e-5))
    (z * go.cpu().double()).sum().backward()
    assert relerr(r["ln_relu"][0], z) < 1e-5                                                         # (the LayerNorm + ReLU bounds of test_ln_relu_mean16)
    for got, ref in zip(r["ln_relu"][1], rv):
        assert relerr(got, ref.grad) < 5e-5
    for R, dd in ((37, 128), (210, 384)):
        under_ff(TA.test_add_dropout_layer_norm_vs_float64, ops, R, dd, 0.25)


# ------------------------------------------------------------------------------------------------------------------------------
# the walks of the row kernels that the shipped widths do not reach (tests/test_row_walks_gpu.py)
# ------------------------------------------------------------------------------------------------------------------------------
ROW_WALKS = [
    # the float4 map behind the statistics pass: ragged bags under a raised max_len (blocks past every segment's end write zero rows)
    (TR.launch_pool, TR.body_pool, TR.PoolCase(20, (513, 1, 300, 77), 0, "a", True, "stats4", 32)),
    # the backward's scalar and float4 rows: 4100-row and 1-row bags under one grid, rows past the end inside a wave's four
    (TR.launch_pool_bwd, TR.body_pool_bwd, TR.PoolBwdCase("scalar", 6, 2, True, True)),
    (TR.launch_pool_bwd, TR.body_pool_bwd, TR.PoolBwdCase("float4", 260, 4, True, True)),
    # the gate score's float4 rows with idle lanes (5 float4 per branch half) and its scalar rows
    (TR.launch_gate_score, TR.body_gate_score, TR.GateScoreCase("float4", 20, 37, 0.25, False)),
    (TR.launch_gate_score, TR.body_gate_score, TR.GateScoreCase("scalar", 516, 37, 0.25, False)),
    # the generic LayerNorm at QT = 4 with one column in its last group
    (TR.launch_ln, TR.body_ln, TR.LnCase(129, 48, "offset", True, False, 1, False, "generic", 4)),
    # colsum straight into its destination, stored and added (no partial rows, no merge)
    (TR.launch_colsum, TR.body_colsum, TR.ColsumCase(32, 260, False, True, "direct", 1)),
    (TR.launch_colsum, TR.body_colsum, TR.ColsumCase(32, 260, True, True, "direct", 1)),
]


@pytest.mark.parametrize("launch,body,case", ROW_WALKS, ids=[f"{b.__name__}-{'-'.join(str(v) for v in c)}" for _, b, c in ROW_WALKS])
def test_row_kernel_walks(ops, launch, body, case):
    """Each case asserts its walk on the host (the mirrors of tests/test_row_walks_gpu.py), runs four times for the bit comparison and
    once more through its family's float64 body while the allocations are poisoned."""
    runs(lambda: launch(case))
    under_ff(body, case)


# ------------------------------------------------------------------------------------------------------------------------------
# the walks of the plane-fed contraction kernels (tests/test_gemm_walks_gpu.py): one case of each family
# ------------------------------------------------------------------------------------------------------------------------------
GEMM_WALKS = [
    # persistent NT kernel, single-plane A (the epilogue's LDS area lies behind the ring), rank-1 term + bit mask + column sums, pitches > extent
    TW.Case("nt", 82, "NT", 768, 256, 96, 1, 2, 8, 24, ldc_pad=4, epi=TW.Epi(rowv=True, rowseg=True, maskbits=True, colsum=True), feed="stale"),
    # the two-layer form with layer 1 as planes only (no fp32 C at all)
    TW.Case("nt", 86, "NT", 768, 256, 64, 2, 2, 24, 8, epi=TW.two_layers(256, "only")),
    # TN kernel: ten groups under a grid of sixteen (six workgroups leave at once), partial tiles in a fresh workspace, the reduce kernel
    TW.Case("tn", 91, "TN", 640, 256, 224, 2, 1, splits=2, epi=TW.Epi(bias=True, act0=1)),
    # ... a last split of one chunk under the three-slot ring, folded by the merge queue
    TW.Case("tn", 92, "TN", 512, 128, 224, 2, 2, 8, 24, splits=3, epi=TW.Epi(accumulate=True)),
    # register-staged planes: the predicated tail of the 192-row tile, ragged N and K, split-K
    TW.Case("pre", 34, "TN", 192, 264, 264, 2, 2, b_pad=8, splits=3, epi=TW.Epi(accumulate=True), feed="stale"),
    TW.Case("pre", 11, "TT", 200, 136, 72, 1, 2, splits=3, epi=TW.Epi(alpha=0.5, bias=True, act0=1)),
]


@pytest.mark.parametrize("case", GEMM_WALKS, ids=TW.case_id)
def test_contraction_walks(ops, case):
    """Each case asserts its walk on the host, runs four times for the bit comparison and once more against the exact oracle while the
    allocations are poisoned (torch.equal: no tolerance)."""
    runs(lambda: TW.launch(case))
    under_ff(TW.body, case)


def test_contraction_walk_gate_score_tile(ops):
    case = TW.GATE_CASES[0]
    runs(lambda: TW.launch_gate(case)[0])
    under_ff(TW.test_plane_fed_gate_score_tile, case)


# ------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["one", "two"])
def bwd_form(request, ops):
    prev = ops.ATTN_BWD
    ops.ATTN_BWD = request.param
    yield request.param
    ops.ATTN_BWD = prev


def _mha(ops, lens, hd, p, seed, tag):
    d = TA.NH * hd
    Lt = sum(lens)
    qkv = TA.rnd(f"{tag}{lens}", Lt, 3 * d, scale=0.7).to(DEV); go = TA.rnd(f"{tag}g{lens}", Lt, d).to(DEV)
    seg = ops.Segments(lens, DEV)

    def fn():
        a = qkv.clone().requires_grad_(True)
        o = ops.mha(a, TA.NH, p, ops.DeviceRng(DEV, seed=seed), seg=seg)
        (o * go).sum().backward()
        return o, a.grad
    return fn


def test_attention_ragged_bags(ops, bwd_form):
    """Both backward forms on [700, 257, 33, 1025, 1]: the single-pass form's ceil(max_len / 256) x Ltot x D partial slabs are mostly
    unwritten for the short bags."""
    lens = [700, 257, 33, 1025, 1]
    runs(_mha(ops, lens, TA.HD, 0.25, 77, "q"))
    under_ff(TA.test_mha_fused_fwd_bwd_vs_float64, ops, "exact", bwd_form, lens, 0.25)


@pytest.mark.parametrize("hd", [16, 64])
def test_attention_other_head_dims(ops, bwd_form, hd):
    runs(_mha(ops, [130, 64, 300], hd, 0.25, 78, f"hd{hd}"))
    under_ff(TA.test_mha_other_head_dims, ops, bwd_form, hd)


def test_attention_forward_with_the_log_sum_exp_given(ops):
    lens, hd = [700, 257, 33, 1025, 1], TA.HD
    d, Lt = TA.NH * hd, sum(lens)
    qkv = TA.rnd(f"lse{hd}{lens}", Lt, 3 * d, scale=0.7).to(DEV); go = TA.rnd(f"lseg{hd}{lens}", Lt, d).to(DEV)
    seg = ops.Segments(lens, DEV)

    def fn():
        planes = ops.split_planes(qkv)
        with torch.no_grad():
            ops.MhaFn.apply(qkv, TA.NH, 0.0, None, 0, seg, None, planes)                            # eval-mode pass: leaves the log-sum-exp
        lse = ops.MhaFn.last_lse
        rng = ops.DeviceRng(DEV, seed=81)
        sid = rng.site("mha_attn", (Lt, TA.NH), 0.25)
        a = qkv.clone().requires_grad_(True)
        o = ops.MhaFn.apply(a, TA.NH, 0.25, rng.seed, sid, seg, None, planes, lse)
        assert ops.MhaFn.last_lse is lse
        (o * go).sum().backward()
        return o, a.grad, lse
    runs(fn)
    under_ff(TA.test_forward_with_the_log_sum_exp_given_equals_the_plain_forward, ops, hd, lens)


ATTN_WALKS = [
    # a cap above the longest bag: workgroups that return in every main grid and in the reduce grid, partial slabs sized by the cap
    (TAW.RAISED[0], TAW.body_raised_max_len),
    # five key blocks under the single-pass form: one unrolled group + remainder in the reduce, every partial slab freshly allocated
    (next(c for c in TAW.SINGLE_PASS if c.lens == (1025,) and c.hd == 48), lambda ops, c, frm: TAW.run(ops, c, frm)),
]


@pytest.mark.parametrize("case,body", ATTN_WALKS, ids=[TAW.cid(c) for c, _ in ATTN_WALKS])
def test_attention_walks(ops, case, body):
    """Two walks of tests/test_attn_walks_gpu.py under the single-pass backward: four runs for the bit comparison (O, lse, the
    gradients and D), once more through the walk file's own float64 body while the allocations are poisoned."""
    prev = ops.ATTN_BWD
    ops.ATTN_BWD = "one"
    try:
        assert TAW.facts(case).bags[-1].nkb == (5 if case.max_len is None else 2)
        runs(lambda: TAW.launch(ops, case))
        under_ff(body, ops, case, "one")
    finally:
        ops.ATTN_BWD = prev


def test_in_projection_that_writes_qkv_as_planes_only(ops):
    """The ESAT layer over a ragged slab in bf16x3: q | k | v leave the in-projection as operand planes only."""
    from advmil_amd.model.esat import HipTransformerEncoderLayer
    with gemm_mode("bf16x3"):
        torch.manual_seed(5)
        layer = HipTransformerEncoderLayer(384, 8, 384, 0.25).cuda()
        layer.train(True)
        g = torch.Generator(device="cuda").manual_seed(9)
        lens = [2048, 1536, 512, 1040]
        x = torch.randn(sum(lens), 384, device="cuda", generator=g)
        go = torch.randn(sum(lens), 384, device="cuda", generator=g)
        seg = ops.Segments(lens, x.device)

        def fn():
            layer.rng = ops.DeviceRng(x.device, seed=77)
            for p_ in layer.parameters():
                p_.grad = None
            xi = x.clone().requires_grad_(True)
            y = layer.forward_rows(xi, seg)
            (y * go).sum().backward()
            return y, xi.grad, [p_.grad for p_ in layer.parameters()]
        assert ops.ATTN_QKV_PLANES
        runs(fn)
    for training in (False, True):
        under_ff(TA.test_in_projection_writes_qkv_as_operand_planes_only, ops, training)


# ------------------------------------------------------------------------------------------------------------------------------
# fused small networks
# ------------------------------------------------------------------------------------------------------------------------------
def _pick(r, keys):
    return {k: r[k] for k in keys}


@pytest.mark.parametrize("kind", ["abmil", "patch"])
@pytest.mark.parametrize("B", [1, 3])
def test_generator_head(kind, B):
    from tests import ghead_ref as GR, test_ghead_gpu as TG
    raw = []

    def fn():
        raw.append(TG._run(kind, B, True))
        return _pick(raw[-1], ("pred", "dfeats", "grads"))
    runs(fn)
    r = raw[2]                                                   # the 0xFF run against float64 (test_fused_head_vs_float64_...)
    pred, dx, gp = GR.ref(r)
    GR.close(r["pred"], pred, 2e-6, "pred")
    GR.close(r["dfeats"], dx, 5e-6, "d feats")
    for k, g in r["grads"].items():
        if k.startswith(GR.HEAD_KEYS):
            GR.close(g, gp[k], 5e-6, k)


@pytest.mark.parametrize("iprd,prj", [("instance", "x"), ("bag", "x"), ("instance", "y"), ("bag", None)])
@pytest.mark.parametrize("B", [1, 4])
def test_discriminator_tail(iprd, prj, B):
    from tests import test_tail_gpu as TT
    raw = []

    def fn():
        raw.append(TT._run(iprd, prj, B, True))
        return _pick(raw[-1], ("f", "deb", "dim", "dt", "grads"))
    runs(fn)
    r = raw[2]                                                   # test_fused_tail_vs_float64_with_the_kernels_own_masks
    out, deb, dim_, dt, gp = TT._ref64(r, iprd, prj)
    TT._close(r["f"], out, 2e-6, "f")
    TT._close(r["deb"], deb, 5e-6, "d emb_bag")
    TT._close(r["dt"], dt, 5e-6, "d t")
    if iprd == "instance":
        TT._close(r["dim"], dim_, 5e-6, "d ins_mean")
    for k, g in r["grads"].items():
        if gp.get(k) is None or not (k.startswith("net_pair_one.fc2") or k.startswith("net_pair_two") or k.startswith("prj_layer")):
            continue
        TT._close(g, gp[k], 5e-6, k)


@pytest.mark.parametrize("lens", [[37], [1, 300], [512, 96, 130]])
@pytest.mark.parametrize("want_mean,e_grad", [(True, True), (False, False)])
def test_region_chain(lens, want_mean, e_grad):
    """The fused region network against the layer-by-layer path it replaces, the reference of its own test (test_region_gpu.py)."""
    from advmil_amd import ops
    from tests import test_region_gpu as TR
    keys = ("pooled", "fc", "mean", "de", "grads", "A")
    with gemm_mode("bf16x3"):
        raw = []

        def fn():
            raw.append(TR._run(lens, True, True, want_mean=want_mean, e_grad=e_grad))
            return _pick(raw[-1], keys)
        runs(fn)
        a, b = raw[2], TR._run(lens, False, True, want_mean=want_mean, e_grad=e_grad)
    assert a["log"] == b["log"] and any(t == "dx_fc1" for (t, _, _, _) in a["log"])
    TR._close(a["fc"], b["fc"], 1e-6, "fc_ins")
    TR._close(a["A"], b["A"], 2e-5, "attention weights")
    TR._close(a["pooled"], b["pooled"], 1e-5, "pooled")
    if want_mean:
        TR._close(a["mean"], b["mean"], 1e-5, "mean")
    if e_grad:
        TR._close(a["de"], b["de"], 5e-5, "d e")
    else:
        assert a["de"] is None
    for k in a["grads"]:
        TR._close(a["grads"][k], b["grads"][k], 5e-5, k)


def test_region_chain_direct_walk():
    """The entry points of csrc/region.hip themselves (tests/test_region_walks_gpu.py), forward and backward, at bags [30, 1, 20, 77, 64]
    with both draws on and a row map: three tiles whose first holds three segment ends, tail rows the kernels skip, a partial row per tile
    with three columns nobody writes. Four runs for the bit comparison, then the walk file's own float64 body under 0xFF."""
    from tests import test_region_walks_gpu as TRW
    c = TRW.POISON_CASE
    assert c.lens == (30, 1, 20, 77, 64) and c.mode == "both"

    def fn():
        fw = TRW.launch_fwd(sum(c.lens), c.mode, c.rmap)
        return dict(fw=fw, bw=TRW.launch_bwd(c, fw, nan_ws=False))
    runs(fn)
    under_ff(TRW.body_bwd, c, False)


@pytest.mark.parametrize("M,N,K", [(5, 30, 36), (17, 260, 1028)])
def test_small_linear(ops, M, N, K):
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    x0 = torch.randn(M, K, generator=g).to(DEV); W0 = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b0 = torch.randn(N, generator=g).to(DEV); go = torch.randn(M, N, generator=g).to(DEV)
    rows0, ops.SMALL_LINEAR_ROWS = ops.SMALL_LINEAR_ROWS, 32

    def fn():
        out = {}
        for act, p in (("none", 0.0), ("relu", 0.0), ("relu", 0.25)):
            x, W, b = (t.clone().requires_grad_(True) for t in (x0, W0, b0))
            y = ops.linear_act(x, W, b, act, p, ops.DeviceRng(DEV, seed=77), "site")
            y.backward(go)
            out[(act, p)] = [y, x.grad, W.grad, b.grad]
        return out
    try:
        runs(fn)
    finally:
        ops.SMALL_LINEAR_ROWS = rows0
    for act in ("none", "relu"):
        under_ff(TK.test_small_linear_kernels_vs_float64_and_vs_the_contraction_path, M, N, K, act)


def test_skinny_linear_and_projection_head(ops):
    g = torch.Generator(device="cuda").manual_seed(13)
    B, K, N, d = 5, 192, 1, 200
    x0 = torch.randn(B, K, device="cuda", generator=g); W0 = torch.randn(N, K, device="cuda", generator=g) * 0.3
    b0 = torch.randn(N, device="cuda", generator=g); w = torch.randn(B, N, device="cuda", generator=g)
    hx0, ht0 = torch.randn(3, d, device="cuda", generator=g), torch.randn(3, d, device="cuda", generator=g)
    Wp0, bp0, wg = torch.randn(1, d, device="cuda", generator=g) * 0.3, torch.randn(1, device="cuda", generator=g), torch.randn(3, 1, device="cuda", generator=g)

    def fn():
        out = {}
        for act in ("none", "relu"):
            x, W, b = (t.clone().requires_grad_(True) for t in (x0, W0, b0))
            y = ops.skinny_linear(x, W, b, act)
            (y * w).sum().backward()
            out[act] = [y, x.grad, W.grad, b.grad]
        hx, ht, Wp, bp = (t.clone().requires_grad_(True) for t in (hx0, ht0, Wp0, bp0))
        o = ops.prj_head(hx, ht, hx, Wp, bp)                     # `bag_x`: the same tensor as u and src
        (o * wg).sum().backward()
        out["prj"] = [o, hx.grad, ht.grad, Wp.grad, bp.grad]
        return out
    runs(fn)
    for act in ("none", "relu"):
        under_ff(TK.test_skinny_linear_fwd_bwd, ops, B, K, N, act)
    for mode in ("instance_x", "bag_x", "instance_y", "none"):
        under_ff(TK.test_prj_head_fwd_bwd, ops, 3, d, mode)


# ------------------------------------------------------------------------------------------------------------------------------
# GENConv, Adam, the rest
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 96])
def test_genconv(ops, C):
    """The hub / isolated-node / self-loop graph of test_genconv_on_random_graph_and_without_edges; C = 96 takes the generic kernels."""
    g = torch.Generator().manual_seed(3)
    N, E = 300, 2400
    src = torch.randint(0, N, (E,), generator=g); dst = torch.randint(1, N, (E,), generator=g)
    dst[:600] = 7
    src[600:640] = dst[600:640]
    ei = torch.stack([src, dst]).to(DEV)
    x = torch.randn(N, C, generator=g).to(DEV); t = torch.tensor([1.7], device=DEV); go = torch.randn(N, C, generator=g).to(DEV)

    def fn():
        xd, td = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
        out = ops.genconv_aggregate(xd, td, ops.GraphCSR(ei, N))
        (out * go).sum().backward()
        return out, xd.grad, td.grad
    runs(fn)
    under_ff(TK.test_genconv_on_random_graph_and_without_edges, C)


@pytest.mark.parametrize("C", [128, 96])
@pytest.mark.parametrize("name", ["ladder_s2", "unstaged_forward", "unstaged_backward"])
def test_genconv_walks(ops, name, C):
    """The launches of tests/test_genconv_gpu.py where launched work exceeds real work: the S = 2 degree ladder with its 5-node last
    tile (tiles past N, half-waves past the tile's nodes, dt partials of empty workgroups) and the tiles of more than 2048 edges in the
    forward's and in the backward's CSR image (the clamped LDS read of an unstaged tile); C = 96 walks the same graphs a wave per node."""
    ei, N = TG.named_graph(name)                                 # (asserts on the host that the graph is where its name says)
    x, go = TG.inputs(N, C, seed=C)
    eid, x, go = dev(ei, x, go)
    t = torch.tensor([1.7], device=DEV)

    def fn():
        xd, td = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
        out = ops.genconv_aggregate(xd, td, ops.GraphCSR(eid, N))
        (out * go).sum().backward()
        return out, xd.grad, td.grad
    runs(fn)
    under_ff(TG.named_case, name, C)


def test_adam_with_a_scalar_tail(ops):
    """n = 5003 (n % 4 = 3: the scalar tail runs), weight-decay mask, L1 term, grad_scale != 1, planes out, abs_partial, clear_grad;
    three steps against oracle.adam_step in float64 at test_adam_matches_oracle's bound."""
    from oracle import advmil_oracle as O
    n, nw = 5003, 3000
    p0 = rnd("ap", n, scale=0.1)
    wdmask = torch.zeros(n); wdmask[:nw] = 5e-4
    gs = [rnd(f"ag{it}", n, scale=0.01) for it in range(3)]
    nblk = ops.adam_blocks(n)

    def fn():
        pd = torch.empty(n, device=DEV).copy_(p0)
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        wd = wdmask.to(DEV)
        out = []
        for it in range(3):
            grad = torch.empty(n, device=DEV).copy_(gs[it] * 4.0)
            pl = ops.Planes.alloc((n,), pd.device)
            ap = torch.empty(nblk, dtype=torch.float32, device=DEV)
            before = pd.clone()
            ops.adam_step(pd, grad, m, v, wd, step, 8e-5, grad_scale=0.25, l1_coef=1e-5, planes=pl, abs_partial=ap, clear_grad=True)
            out.append(dict(p=pd.clone(), m=m.clone(), v=v.clone(), grad=grad, pl=pl, ap=ap, before=before, abs=ops.abs_sum(before)))
        out.append(step)
        return out
    r = runs(fn)
    P_ = {"w.weight": p0[:nw].reshape(30, 100).clone(), "w.bias": p0[nw:].clone()}
    st = {}
    for it in range(3):
        G = {"w.weight": gs[it][:nw].reshape(30, 100), "w.bias": gs[it][nw:]}
        Gl1 = {k: G[k] + 1e-5 * torch.sign(P_[k]) for k in P_}
        P_ = O.adam_step(P_, Gl1, st, 8e-5, 5e-4, decay_filter=True)
        ref = torch.cat([P_["w.weight"].reshape(-1), P_["w.bias"]])
        o = r[it]
        assert float((o["p"].cpu() - ref).abs().max()) < 1e-7, it                                   # test_adam_matches_oracle
        want = ops.split_planes(o["p"])
        assert torch.equal(o["pl"]["hi"], want.hi) and torch.equal(o["pl"]["lo"], want.lo)
        assert float(o["grad"].abs().max()) == 0.0 and not bool(torch.signbit(o["grad"]).any())     # cleared behind its read, tail included
        want_abs = o["before"].double().abs().sum()
        assert relerr(o["ap"].double().sum().reshape(1), want_abs.reshape(1)) < 1e-5                 # test_colsum_and_abs_sum_and_uniform
        assert relerr(o["abs"], want_abs.reshape(1)) < 1e-5
    assert int(r[3].item()) == 3


def test_stage_bag_uniform_dropout_and_cindex(ops):
    from advmil_amd import _lib
    from advmil_amd.eval import concordance_index_censored
    from oracle import cindex_oracle as CO
    L = _lib.lib()
    x = torch.randn(1040, 1024, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    xs = torch.randn(37, 129, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    rs = np.random.RandomState(3)
    n = 1000
    tm = (np.floor(rs.rand(n) * 37) / 37).astype(np.float32)     # ties in time and in risk
    ev = rs.rand(n) < 0.45
    est = (np.floor(rs.rand(n) * 200) / 200).astype(np.float32)
    nb = x.numel() * 4

    def fn():
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        slab = torch.empty(1040, 1024, device=DEV)
        pl = ops.Planes.alloc((1040, 1024), x.device)
        assert L.advmil_stage_bag(slab.data_ptr(), x.data_ptr(), nb, pl.hi.data_ptr(), None, pl.lo.data_ptr(), None, nb // 2, st) == 0
        rng = ops.DeviceRng(DEV, seed=99)
        u = rng.uniform(1000)
        xi = xs.clone().requires_grad_(True)
        y = ops.dropout(xi, 0.25, rng, "t")
        y.backward(xs)
        c = concordance_index_censored(torch.from_numpy(ev), torch.from_numpy(tm), torch.from_numpy(est))
        return dict(slab=slab, pl=pl, u=u, y=y, dx=xi.grad, c=[float(c[0])] + [int(v) for v in c[1:]])
    r = runs(fn)
    want = ops.split_planes(x)
    assert torch.equal(r["slab"], x) and torch.equal(r["pl"]["hi"], want.hi) and torch.equal(r["pl"]["lo"], want.lo)   # test_stage_bag_copies_rows_...
    assert np.array_equal(r["u"].cpu().numpy(), synth.kernel_uniform(99, 1, 1000))                  # test_colsum_and_abs_sum_and_uniform
    keep = H.T(synth.dropout_keep(99, 2, xs.numel(), 0.25).reshape(xs.shape)).to(DEV)
    assert torch.equal(r["y"] != 0, (keep != 0) & (xs != 0)) and torch.equal(r["dx"], r["y"])
    assert relerr(r["y"], xs.cpu().double() * keep.cpu().double() / 0.75) < 2e-6                    # (one fp32 product per element: test_gemm_layouts' bound)
    wc = CO.cindex_counts(ev, tm, est)
    assert tuple(r["c"][1:]) == tuple(wc[1:]) and abs(r["c"][0] - wc[0]) < 1e-15                    # test_hip_counts_equal_oracle_on_larger_inputs_and_errors


@pytest.mark.parametrize("which", ["bce", "hinge", "wasserstein"])
def test_gan_losses_with_a_partial_real_mask(ops, which):
    g = torch.Generator(device="cuda").manual_seed(8)
    nb = 16
    fake0 = torch.randn(nb, device="cuda", generator=g) * 2; real0 = torch.randn(nb, device="cuda", generator=g) * 2
    mask = (torch.rand(nb, device="cuda", generator=g) < 0.5).float()
    pred0 = torch.rand(nb, 1, device="cuda", generator=g); t = torch.rand(nb, 1, device="cuda", generator=g)
    e = (torch.rand(nb, 1, device="cuda", generator=g) < 0.5).float(); vis = (torch.rand(nb, device="cuda", generator=g) < 0.6).float()
    assert 0 < float(mask.sum()) < nb

    def fn():
        fake, real, pred, ff = (v.clone().requires_grad_(True) for v in (fake0, real0, pred0, fake0))
        got, st = ops.gan_d_loss(fake, real, mask, which, 32.0, 11.0)
        (got * 1.5).backward()
        g2, st2 = ops.gan_g_loss(pred, ff, t, e, vis, 0.3, 0.2, "l2", 0.004, 32.0, 9.0)
        g2.backward()
        return got, st, fake.grad, real.grad, g2, st2, pred.grad, ff.grad
    runs(fn)
    under_ff(TK.test_fused_gan_losses_match_composed_torch, ops, which)
