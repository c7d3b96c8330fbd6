"""GPU: every walk of the pooling, gate and LayerNorm row kernels (csrc/pool.hip) against float64 restatements of the operations.

pool.hip picks its code path from the shape. Softmax pooling: the two-launch `online` form (D % 8 == 0, D >= 16, at most 2048 blocks per
segment), else a statistics pass + the 8-column map (`stats8`) or the float4 map (`stats4`: D % 8 == 4 or D == 8); rows per block
32 .. 512 from the longest segment. Its backward: planes, float4 or scalar rows. The gate score: two rows per wave at D == 384, float4
rows up to D == 512, scalar rows. LayerNorm-ReLU(-mean16): the 16-byte kernels (d % 128 == 0 and every pointer aligned: NV = d / 128) or
the generic ones (QT = 2 / 4 / 6 / 8 groups of 64 columns). colsum / act_dropout_bwd: `direct` when one block sees every row and the
destination is 16-byte aligned, else partial rows + a merge; columns in chunks of 1024. Each case below names its walk and ASSERTS IT ON
THE HOST with the plain-Python mirrors of this file before it launches; tests/test_row_walks_plan_cpu.py pins the mirrors' constants
to the source text and to the library's own workspace arithmetic. `test_every_walk_is_reached` fails if the parametrisation loses one.

One float64 body per operation (`body_pool`, `body_pool_bwd`, `body_gate_score`, `body_gate_bwd`, `body_ln`, `body_ln_rows`,
`body_colsum`, `body_act_bwd`), shared by all cases and run under poisoned allocations by tests/test_poison_kernels_gpu.py.

Bounds: the project's own (BOUND below; the tests they come from are named there). They were measured at D <= 384, segments <= 8192
rows and scores of 3 * randn. Outside that -- D >= 1016, segments >= 32769 rows, the score regimes `b` (block maxima 60 .. 130 apart)
and `d` (scores near +-3e4), d = 500 / 512 with offset rows, the 65539- and 32801-row sums -- the bound is max(project bound, 4 e32),
e32 = the error of the SAME restatement evaluated in float32 on the host (exp(x) written exp2(float32(x * log2 e)) as in common.h)
against its float64 self; 4 for the different summation order. Never a figure taken from the kernels.

Measured on an MI355X when this file was written, worst error over the bound in force, per family (every body prints its figures;
`test_every_walk_is_reached` prints the worst of each family):
  pooling forward   0.23  planes `pooled` 4.6e-7 of 2e-6 (score regime a, D = 40); A per entry <= 4.0e-6 of 2e-5 (regime b); the
                          1 049 089-row stats8 case: A 1.7e-7, per entry 2.7e-6, pooled 2.6e-7; 500 000 rows: pooled 3.6e-7
                          (e32 6.7e-6, so the bound in force there is 2.7e-5; the project's 1e-5 would have held too)
  pooling backward  0.005 ds 2.4e-7 of 5e-5 (scalar rows, D = 130)
  gate score        0.034 3.4e-7 of 1e-5 (D = 384, N = 1); N = 65539: 9.8e-8
  gate backward     0.009 4.6e-7 of 5e-5; N = 32801: dwc 2.9e-7
  LayerNorm mean16  0.12  dgamma 5.8e-6 of 5e-5 (rows near 1e3); every other figure <= 2e-7 of 1e-5 / 5e-5
  LayerNorm rows    0.031 emb 3.1e-7 of 1e-5
  colsum            0.017 1.7e-7 of 1e-5; act_dropout_bwd 0.004
No case outside the measured regime needed its widened bound.

Found by this file: rows near 1e3 (`bigmean`) missed the 1e-5 bound of the LayerNorm output, 1.67e-5 (16-byte kernel) and 1.58e-5
(generic kernel) -- the rounding of the row mean, up to an ulp of 1e3, shifts every normalised value of the row, and torch's own float32
layer_norm is 2.0e-5 from float64 on the same rows. The forward kernels now centre such rows a second time by the mean of the
once-centred row (csrc/pool.hip::ln_recentre): 1.1e-7 / 8e-8. Rows whose mean is small against their spread keep their bits.
"""
import collections

import numpy as np
import pytest
import torch

from advmil_amd import synth
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# csrc/pool.hip (tests/test_row_walks_plan_cpu.py pins them)
ROWS_PER_BLOCK, RPB_DIV, RPB_CAP = 32, 1024, 512
POOL_ONLINE_MAX_NBLK = 2048
PBD_ROWS = 4
LN_BWD_MAXBLK = 2048
GATE_SCORE_MAXBLK = 8192
GATE_PAIR_D4, GATE_F4_MAX_D4 = 96, 128
COLSUM_CHUNK = 1024
LN_QT_STEPS = ((128, 2), (256, 4), (384, 6), (512, 8))

LOG2E = 1.44269504088896340736
TINY = 2.0 ** -126

BOUND = dict(
    score=1e-5, A=1e-5, pooled=1e-5,         # test_gated_pool_fwd_bwd (max-relative)
    A_entry=2e-5, pooled_planes=2e-6,        # test_segmented_softmax_pooling (per entry, relative; absolute)
    mean=1e-5,                               # test_segmented_softmax_pooling: 1e-5 of max + 1e-7 = 1e-5 (max + 1e-2)
    grad=5e-5,                               # test_gated_pool_fwd_bwd: every gradient
    ln_out=1e-5, ln_grad=5e-5,               # test_ln_relu_mean16
    colsum=1e-5,                             # test_colsum_and_abs_sum_and_uniform
)

LADDER = (1, 31, 32, 33, 513)
BWD_LENS = (1, 3, 4, 5, 15, 16, 17, 33, 4100)

PoolWalk = collections.namedtuple("PoolWalk", "form rpb nblk")
LnWalk = collections.namedtuple("LnWalk", "kernel width")            # ("ln4", NV) or ("generic", QT)
ColsumWalk = collections.namedtuple("ColsumWalk", "form chunks rpb nblk")


# ------------------------------------------------------------------------------------------------------------------------------
# host side: which walk a shape takes
# ------------------------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def rows_per_block(rows):
    r = ceil_div(rows, RPB_DIV)
    r = ceil_div(r, 32) * 32
    return min(max(r, ROWS_PER_BLOCK), RPB_CAP)


def pool_walk(max_len, D, planes=False, mean=False):
    """form / rows per block / blocks per segment of softmax_pool_fwd_impl; None where the host check refuses the call."""
    if D <= 0 or D % 4 or D > 1024 or (planes and (D % 8 or D < 16 or mean)):
        return None
    rpb = rows_per_block(max_len)
    nblk = ceil_div(max_len, rpb)
    wide = D % 8 == 0 and D >= 16
    if wide and nblk <= POOL_ONLINE_MAX_NBLK:
        return PoolWalk("online", rpb, nblk)
    if planes or mean:
        return None                                   # the mean and the planes ride in the two-launch form only
    return PoolWalk("stats8" if wide else "stats4", rpb, nblk)


def pool_bwd_walk(D, ldh, planes=False):
    if ldh < D or ldh % 4 or (planes and (D % 8 or ldh % 8)):
        return None
    return "planes" if planes else ("float4" if D % 4 == 0 else "scalar")


def pool_bwd_partials(max_len):
    return ceil_div(max_len, 4 * PBD_ROWS)


def gate_score_walk(D):
    if D % 4 == 0 and D // 4 == GATE_PAIR_D4:
        return "pair"
    return "float4" if D % 4 == 0 and D // 4 <= GATE_F4_MAX_D4 else "scalar"


def gate_score_blocks(N):
    return min(ceil_div(N, 4), GATE_SCORE_MAXBLK)


def ln_walk(d, aligned, planes=False, dup=1):
    """The 16-byte kernel with NV, or the generic kernel with QT; None where the host check refuses (planes / dup off the 16-byte form)."""
    if d <= 0 or d > 512:
        return None
    if d % 128 == 0 and aligned:
        return LnWalk("ln4", d // 128)
    if planes or dup != 1:
        return None
    return LnWalk("generic", next(q for lim, q in LN_QT_STEPS if d <= lim))


def ln_bwd_blocks(nreg):
    return min(nreg, LN_BWD_MAXBLK)


def colsum_walk(M, N, aligned):
    rpb = rows_per_block(M)
    nblk = ceil_div(M, rpb)
    return ColsumWalk("direct" if nblk == 1 and aligned else "merged", ceil_div(N, COLSUM_CHUNK), rpb, nblk)


# ------------------------------------------------------------------------------------------------------------------------------
# shared helpers
# ------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ops():
    from advmil_amd import ops
    from advmil_amd import _lib
    _lib.lib()
    return ops


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def pitched(x, pad, fill=77.0):
    """x [N, D] on the device as a column view of a [N, D + pad] buffer (row pitch D + pad; the pad columns hold `fill`)."""
    if not pad:
        t = x.to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    N, D = x.shape
    wide = torch.full((N, D + pad), fill)
    wide[:, :D] = x
    v = wide.to(DEV)[:, :D]
    assert v.stride(0) == D + pad and v.data_ptr() % 16 == 0
    return v


def off_by_one_float(x):
    """x on the device as a contiguous view one float into a larger buffer: 4 bytes off 16-byte alignment."""
    n = x.numel()
    buf = torch.zeros(n + 8, device=DEV)
    v = buf[1:1 + n].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


_REFS, _INPUTS = {}, {}
WORST = {}                                            # family -> (error / bound, case, figure): printed by every body


def cached(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


def judge(family, case, err, bound):
    """Print every figure, keep the family's worst ratio, then assert."""
    line = " ".join(f"{k} {err[k]:.2e}/{bound[k]:.1e}" for k in err)
    print(f"[{family}] {case}: {line}")
    for k in err:
        r = err[k] / bound[k]
        if r > WORST.get(family, (0.0,))[0]:
            WORST[family] = (r, case, k)
    for k in err:
        assert err[k] < bound[k], (family, case, k, err[k], bound[k])


def widen(bound, e32):
    """max(project bound, 4 e32) for the figures a case has outside the measured regime."""
    return {k: max(v, 4 * e32[k]) if e32 and k in e32 else v for k, v in bound.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# softmax pooling
# ------------------------------------------------------------------------------------------------------------------------------
PoolCase = collections.namedtuple("PoolCase", "D lens pad regime cap form rpb")


def pool_case_id(c):
    lens = "ladder" if c.lens == LADDER else "x".join(str(v) for v in c.lens[:3]) + ("..." if len(c.lens) > 3 else "")
    return f"{c.form}{c.rpb}-D{c.D}-{lens}-pad{c.pad}-{c.regime}{'-cap' if c.cap else ''}"


def _pool_cases():
    out = []
    for cap in (False, True):
        for D in (16, 24, 40, 128, 384, 1016, 1024):
            for pad in (0, 8):
                out.append(PoolCase(D, LADDER, pad, "a", cap, "online", 32))
        out.append(PoolCase(16, (32801, 5), 0, "a", cap, "online", 64))
        out.append(PoolCase(16, (500000, 700), 0, "a", cap, "online", 512))
        for D in (4, 8, 12, 20, 100, 1020):
            for pad in (0, 8):
                out.append(PoolCase(D, LADDER, pad, "a", cap, "stats4", 32))
        out.append(PoolCase(4, (32801, 5), 0, "a", cap, "stats4", 64))
        out.append(PoolCase(4, (500000, 700), 0, "a", cap, "stats4", 512))
        out.append(PoolCase(16, (1049089, 77), 0, "a", cap, "stats8", 512))
    return out


def _regime_cases():
    out = []
    for form, D in (("online", 40), ("stats4", 20)):
        for regime in ("a", "b", "c", "d+", "d-"):
            out.append(PoolCase(D, (96, 96, 96, 96), 0, regime, False, form, 32))
        out.append(PoolCase(D, (1, 1, 1, 1, 1), 0, "e", False, form, 32))
    return out


POOL_CASES = _pool_cases()
REGIME_CASES = _regime_cases()
REGIME_B_OFFSETS = ((0.0, -60.0, -130.0), (-130.0, 0.0, -60.0), (-85.0, -86.0, 0.0), (0.0, -60.0, -130.0))


def pool_scores(lens, regime, g):
    N = sum(lens)
    if regime == "c":
        return torch.full((N,), 0.7)
    if regime == "b":               # three blocks of 32 rows per segment: block offset + randn; segment 3: one outlier row carries block 1
        assert all(n == 3 * ROWS_PER_BLOCK for n in lens) and len(lens) == len(REGIME_B_OFFSETS)
        s = torch.randn(N, generator=g)
        for k, offs in enumerate(REGIME_B_OFFSETS):
            for j, o in enumerate(offs):
                s[96 * k + 32 * j:96 * k + 32 * j + 32] += o
        s[96 * 3 + 32 + 7] += 50.0
        return s
    s = 3.0 * torch.randn(N, generator=g)
    if regime in ("d+", "d-"):
        s = s + (3e4 if regime == "d+" else -3e4)     # rounded to float32 here: the input IS the rounded score
    return s


def pool_inputs(D, lens, regime):
    def make():
        g = _gen(1000 * D + len(lens) + sum(lens) % 997)
        N = sum(lens)
        return dict(h=torch.randn(N, D, generator=g), s=pool_scores(lens, regime, g), dp=torch.randn(len(lens), D, generator=g),
                    dA=torch.randn(N, generator=g))
    return cached(_INPUTS, ("pool", D, lens, regime), make)


def restate_pool(s, h, lens, dp, dA, dtype=torch.float64):
    """a = softmax(s) per segment, pooled = a @ h, mean = h.mean(0), ds by autograd of (pooled * dp).sum() + (a * dA).sum()."""
    sr = s.detach().to(dtype).requires_grad_(True)
    hr = h.detach().to(dtype)
    A, P, Mn, o = [], [], [], 0
    for n in lens:
        x = sr[o:o + n]
        if dtype == torch.float64:
            a = torch.softmax(x, 0)
        else:                                         # common.h: exp(x) = exp2(float32(x * log2 e))
            e = torch.exp2((x - x.detach().max()) * LOG2E)
            a = e / e.sum()
        A.append(a); P.append(a @ hr[o:o + n]); Mn.append(hr[o:o + n].mean(0))
        o += n
    A, P = torch.cat(A), torch.stack(P)
    loss = (P * dp.to(dtype)).sum()
    if dA is not None:
        loss = loss + (A * dA.to(dtype)).sum()
    loss.backward()
    return dict(A=A.detach().double(), pooled=P.detach().double(), mean=torch.stack(Mn).double(), ds=sr.grad.double())


def pool_errors(got, ref, tiny=False):
    """The figures the project's bounds are stated in, for whatever `got` holds. tiny: entries of A below 2^-126 in float64 are held to
    an absolute 2^-126 (hardware may flush them) and leave the relative figure."""
    err = {}
    if "A" in got:
        A, Ar = got["A"].detach().cpu().double(), ref["A"]
        d = (A - Ar).abs()
        err["A"] = float(d.max() / Ar.max())
        big = Ar >= TINY if tiny else torch.ones_like(Ar, dtype=torch.bool)
        if tiny:
            assert float(big.double().mean()) >= 1.0 / 3.0 - 1e-12, float(big.double().mean())     # the relative check still bites
            assert float(d[~big].max() if bool((~big).any()) else 0.0) <= TINY
        err["A_entry"] = float((d[big] / Ar[big]).max())
    for k in ("pooled", "ds"):
        if k in got:
            err[k] = relerr(got[k], ref[k])
    if "pooled_planes" in got:
        err["pooled_planes"] = float((got["pooled_planes"].detach().cpu().double() - ref["pooled"]).abs().max())
    if "mean" in got:
        err["mean"] = float((got["mean"].detach().cpu().double() - ref["mean"]).abs().max() / (ref["mean"].abs().max() + 1e-2))
    return err


POOL_BOUND = dict(A=BOUND["A"], A_entry=BOUND["A_entry"], pooled=BOUND["pooled"], pooled_planes=BOUND["pooled_planes"],
                  mean=BOUND["mean"], ds=BOUND["grad"])


def pool_reference(key, s, h, lens, dp, dA, e32, planes_image=False):
    def make():
        ref = restate_pool(s, h, lens, dp, dA)
        ref["e32"] = None
        if e32:
            r32 = restate_pool(s, h, lens, dp, dA, torch.float32)
            got = dict(A=r32["A"], pooled=r32["pooled"], ds=r32["ds"], mean=r32["mean"])
            if planes_image:
                got["pooled_planes"] = r32["pooled"]
            ref["e32"] = pool_errors(got, ref, tiny=False)
            if bool((ref["A"] < TINY).any()):                  # (flushed entries: the relative figure of the rest)
                ref["e32"]["A_entry"] = pool_errors(dict(A=r32["A"]), ref, tiny=True)["A_entry"]
        return ref
    return cached(_REFS, key, make)


def pool_outside_regime(c):
    return c.D >= 1016 or max(c.lens) >= 32769 or c.regime in ("b", "d+", "d-")


def pool_device(c):
    def make():
        ops = _ops()
        inp = pool_inputs(c.D, c.lens, c.regime)
        d = dict(h=pitched(inp["h"], c.pad), s=inp["s"].to(DEV), dp=inp["dp"].to(DEV), dA=inp["dA"].to(DEV), hpl=None, himg=None)
        if pool_walk(max(c.lens), c.D, planes=True) is not None:
            base = d["h"] if not c.pad else d["h"]._base
            wpl = ops.split_planes(base)
            img = ops.planes_f32(wpl)
            d["hpl"] = ops.Planes(wpl.hi[:, :c.D], wpl.lo[:, :c.D])
            d["himg"] = img[:, :c.D].cpu()
            assert d["hpl"].hi.stride(0) == c.D + c.pad and d["hpl"].hi.data_ptr() % 16 == 0 and d["hpl"].lo.data_ptr() % 16 == 0
        return d
    return cached(_INPUTS, ("pooldev", c.D, c.lens, c.regime, c.pad), make)


def pool_segments(c):
    ops = _ops()
    seg = ops.Segments(list(c.lens), DEV)
    if c.cap:                                         # raised above the longest bag, as StaticStepPlan.bag_cap does (<= the row total)
        seg.max_len = sum(c.lens)
        assert seg.max_len > max(c.lens)
    return seg


def launch_pool(c):
    """Every forward form the walk admits, and the backward from the kernels' own A -> dict of device tensors."""
    ops = _ops()
    d = pool_device(c)
    seg = pool_segments(c)
    N, D = sum(c.lens), c.D
    w = pool_walk(seg.max_len, D)
    assert w is not None and (w.form, w.rpb) == (c.form, c.rpb), (w, c)
    assert d["h"].stride(0) == D + c.pad
    A, pooled = ops.softmax_pool(d["s"], d["h"], N, D, seg)
    out = dict(A=A, pooled=pooled, ds=ops.softmax_pool_bwd(d["dp"], d["dA"], A, d["h"], N, D, seg))
    if pool_walk(seg.max_len, D, mean=True) is not None:
        assert c.form == "online"
        out["A_mean"], out["pooled_mean"], out["mean"] = ops.softmax_pool_mean(d["s"], d["h"], N, D, seg)
    if d["hpl"] is not None:
        assert c.form == "online" and pool_bwd_walk(D, D + c.pad, planes=True) == "planes"
        out["A_planes"], out["pooled_planes"] = ops.softmax_pool(d["s"], d["h"], N, D, seg, d["hpl"])
        out["ds_planes"] = ops.softmax_pool_bwd(d["dp"], d["dA"], out["A_planes"], d["h"], N, D, seg, d["hpl"])
    return out


def body_pool(c):
    """Launch, compare with float64 (the planes forms with the same body on planes_f32(hpl)) -> the launch's result."""
    inp = pool_inputs(c.D, c.lens, c.regime)
    wide = pool_outside_regime(c)
    key = ("pool", c.D, c.lens, c.regime)
    ref = pool_reference(key, inp["s"], inp["h"], c.lens, inp["dp"], inp["dA"], wide)
    got = launch_pool(c)
    tiny = c.regime == "b"
    case = pool_case_id(c)
    judge("pool", case, pool_errors(dict(A=got["A"], pooled=got["pooled"], ds=got["ds"]), ref, tiny), widen(
        {k: POOL_BOUND[k] for k in ("A", "A_entry", "pooled", "ds")}, ref["e32"]))
    if "mean" in got:
        assert torch.equal(got["A_mean"], got["A"]) and torch.equal(got["pooled_mean"], got["pooled"])     # test_pooling_with_the_mean_from_the_same_pass
        judge("pool", case + "/mean", pool_errors(dict(mean=got["mean"]), ref), widen(dict(mean=POOL_BOUND["mean"]), ref["e32"]))
    if "A_planes" in got:
        assert torch.equal(got["A_planes"], got["A"])                                                   # test_pooling_from_planes_equals_pooling_of_hi_plus_lo
        ref2 = pool_reference(key + ("planes", c.pad), inp["s"], pool_device(c)["himg"], c.lens, inp["dp"], inp["dA"], wide, planes_image=True)
        judge("pool", case + "/planes", pool_errors(dict(pooled_planes=got["pooled_planes"], ds=got["ds_planes"]), ref2),
              widen(dict(pooled_planes=POOL_BOUND["pooled_planes"], ds=POOL_BOUND["ds"]), ref2["e32"]))
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), (case, k)
    return got


@pytest.mark.parametrize("c", POOL_CASES, ids=pool_case_id)
def test_softmax_pooling_walks(c):
    """The forward table: online at 32 / 64 / 512 rows per block (512: the wts[] loop's second pass, 977 blocks), the float4 map, and
    the statistics + 8-column + merge trio at 2050 blocks, whose 77-row second segment leaves 2049 empty blocks; D = 24 leaves thread
    255 idle, D = 1016 walks two rows per pass with 254 threads; pitch D and D + 8; plain, mean and planes forms; own and raised max_len."""
    if c.lens == (500000, 700):
        assert pool_walk(500000, 16) == PoolWalk("online", 512, 977)
    if c.lens == (1049089, 77):
        assert pool_walk(1049089, 16) == PoolWalk("stats8", 512, 2050)
    body_pool(c)


@pytest.mark.parametrize("c", REGIME_CASES, ids=pool_case_id)
def test_softmax_pooling_score_regimes(c):
    """Segments of three 32-row blocks (= rows per block): a 3 randn; b block offsets 60 .. 130 apart, in three orders, and one block
    whose maximum is a single outlier row (c_j = exp(m_j - M) of the merge far from 1, whole blocks flushed); c all scores equal;
    d scores near +-3e4; e segments of one row."""
    assert rows_per_block(max(c.lens)) == ROWS_PER_BLOCK
    if c.regime == "b":
        s = pool_inputs(c.D, c.lens, c.regime)["s"].view(4, 3, 32)
        m = s.max(2).values
        assert [int(v) for v in m.argmax(1)] == [0, 1, 2, 0] and float((m.max(1).values - m.min(1).values).min()) > 80
        assert int(s[3, 1].argmax()) == 7 and float(s[3, 1, 7] - s[3, 1].sort().values[-2]) > 40          # the outlier row
    body_pool(c)


PoolBwdCase = collections.namedtuple("PoolBwdCase", "walk D pad dA cap")
POOL_BWD_CASES = [PoolBwdCase(walk, D, pad, dA, cap)
                  for walk, dims in (("planes", ((16, 0), (24, 8), (384, 0))), ("float4", ((20, 0), (256, 0), (260, 4), (1024, 0))),
                                     ("scalar", ((6, 2), (130, 2))))
                  for D, pad in dims for dA, cap in ((True, False), (False, False), (True, True))]


def pool_bwd_case_id(c):
    return f"{c.walk}-D{c.D}-pad{c.pad}-{'dA' if c.dA else 'nodA'}{'-cap' if c.cap else ''}"


def pool_bwd_device(c):
    def make():
        ops = _ops()
        inp = pool_inputs(c.D, BWD_LENS, "a")
        A64 = torch.cat([torch.softmax(v, 0) for v in inp["s"].double().split(list(BWD_LENS))])
        d = dict(h=pitched(inp["h"], c.pad), A=A64.float().to(DEV), dp=inp["dp"].to(DEV), dA=inp["dA"].to(DEV), hpl=None, himg=None)
        if c.walk == "planes":
            base = d["h"] if not c.pad else d["h"]._base
            wpl = ops.split_planes(base)
            d["hpl"] = ops.Planes(wpl.hi[:, :c.D], wpl.lo[:, :c.D])
            d["himg"] = ops.planes_f32(wpl)[:, :c.D].cpu()
        return d
    return cached(_INPUTS, ("poolbwd", c.walk, c.D, c.pad), make)


def launch_pool_bwd(c):
    ops = _ops()
    d = pool_bwd_device(c)
    seg = ops.Segments(list(BWD_LENS), DEV)
    if c.cap:
        seg.max_len = sum(BWD_LENS)
    N, ldh = sum(BWD_LENS), c.D + c.pad
    assert pool_bwd_walk(c.D, ldh, c.walk == "planes") == c.walk and d["h"].stride(0) == ldh and ldh % 4 == 0
    assert pool_bwd_partials(seg.max_len) > 256                    # pool_bwd_ds_kernel folds its partials in more than one pass
    if c.walk == "scalar":
        assert pool_walk(seg.max_len, c.D) is None                 # the forward refuses this D: A is the float64 softmax rounded to float32
    return dict(ds=ops.softmax_pool_bwd(d["dp"], d["dA"] if c.dA else None, d["A"], d["h"], N, c.D, seg, d["hpl"]))


def body_pool_bwd(c):
    inp = pool_inputs(c.D, BWD_LENS, "a")
    h = pool_bwd_device(c)["himg"] if c.walk == "planes" else inp["h"]
    wide = c.D >= 1016
    ref = pool_reference(("poolbwd", c.D, c.walk == "planes", c.pad if c.walk == "planes" else 0, c.dA), inp["s"], h, BWD_LENS, inp["dp"],
                         inp["dA"] if c.dA else None, wide)
    got = launch_pool_bwd(c)
    judge("pool_bwd", pool_bwd_case_id(c), dict(ds=relerr(got["ds"], ref["ds"])), widen(dict(ds=BOUND["grad"]), ref["e32"]))
    assert bool(torch.isfinite(got["ds"]).all())
    return got


@pytest.mark.parametrize("c", POOL_BWD_CASES, ids=pool_bwd_case_id)
def test_softmax_pooling_backward_walks(c):
    """Segments 1 .. 17 rows around the four rows a wave owns and the sixteen a workgroup owns, and one of 4100 (more than 256
    partials); planes, float4 (64 float4 per row: one pass; 65: a ragged second one) and scalar rows (D % 4 != 0, pitches 8 and 132)."""
    body_pool_bwd(c)


# ------------------------------------------------------------------------------------------------------------------------------
# gate score and gate backward
# ------------------------------------------------------------------------------------------------------------------------------
GATE_SEED, GATE_SA, GATE_SB = 77, 1, 2
GateScoreCase = collections.namedtuple("GateScoreCase", "walk D N p perm")
GATE_SCORE_CASES = (
    [GateScoreCase("pair", 384, N, p, False) for N in (1, 2, 37) for p in (0.0, 0.25)] + [GateScoreCase("pair", 384, 65539, 0.0, False)]
    + [GateScoreCase("float4", D, 37, p, False) for D in (4, 20, 256, 260, 512) for p in (0.0, 0.25)]
    + [GateScoreCase("float4", 4, 32771, p, False) for p in (0.0, 0.25)]
    + [GateScoreCase("scalar", D, 37, p, False) for D in (6, 516) for p in (0.0, 0.25)]
    + [GateScoreCase("pair", 384, 37, 0.25, True), GateScoreCase("float4", 260, 37, 0.25, True), GateScoreCase("scalar", 516, 37, 0.25, True)])


def gate_case_id(c):
    return "-".join(f"{k}{v}" if k not in ("walk",) else str(v) for k, v in c._asdict().items())


def gate_inputs(N, D):
    def make():
        g = _gen(7 * N + D)
        ab = torch.cat([torch.tanh(torch.randn(N, D, generator=g)), torch.sigmoid(torch.randn(N, D, generator=g))], dim=1)
        return dict(ab=ab, wc=0.3 * torch.randn(D, generator=g), bc=torch.randn(1, generator=g), ds=torch.randn(N, generator=g) + 0.5,
                    perm=torch.randperm(N, generator=g))
    return cached(_INPUTS, ("gate", N, D), make)


def gate_masks(N, D, p, perm, dtype=torch.float64):
    """The two branch masks (keep / (1 - p)) regenerated on the host; element index rng_row[n] * D + j."""
    if p == 0.0:
        one = torch.ones(1, 1, dtype=dtype)
        return one, one
    out = []
    for sid in (GATE_SA, GATE_SB):
        keep = H.T(synth.dropout_keep(GATE_SEED, sid, N * D, p).reshape(N, D))
        if perm is not None:
            keep = keep[perm]
        out.append(keep.to(dtype) / (1 - p))
    return out


def restate_gate_score(inp, N, D, p, perm, dtype=torch.float64, chunk=8192):
    ma, mb = gate_masks(N, D, p, perm, dtype)
    wc, bc = inp["wc"].to(dtype), inp["bc"].to(dtype)
    out = []
    for r0 in range(0, N, chunk):                      # in row chunks: the 65539 x 768 case in float64
        ab = inp["ab"][r0:r0 + chunk].to(dtype)
        sl = slice(r0, r0 + chunk) if p > 0 else slice(None)
        out.append((ab[:, :D] * ma[sl] * (ab[:, D:] * mb[sl])) @ wc + bc)
    return torch.cat(out).double()


def launch_gate_score(c):
    ops = _ops()
    def make():
        inp = gate_inputs(c.N, c.D)
        return {k: inp[k].to(DEV) for k in ("ab", "wc", "bc", "perm")}
    d = cached(_INPUTS, ("gatedev", c.N, c.D), make)
    assert gate_score_walk(c.D) == c.walk
    seed = torch.tensor([GATE_SEED], dtype=torch.int64, device=DEV)
    return dict(s=ops.gate_score(d["ab"], d["wc"], d["bc"], c.N, c.D, c.p, seed, GATE_SA, GATE_SB, rng_row=d["perm"] if c.perm else None))


def body_gate_score(c):
    inp = gate_inputs(c.N, c.D)
    perm = inp["perm"] if c.perm else None
    wide = c.N >= 32769

    def make():
        ref = dict(s=restate_gate_score(inp, c.N, c.D, c.p, perm), e32=None)
        if wide:
            ref["e32"] = dict(score=relerr(restate_gate_score(inp, c.N, c.D, c.p, perm, torch.float32), ref["s"]))
        return ref
    ref = cached(_REFS, ("gate_score",) + tuple(c), make)
    got = launch_gate_score(c)
    judge("gate_score", gate_case_id(c), dict(score=relerr(got["s"], ref["s"])), widen(dict(score=BOUND["score"]), ref["e32"]))
    return got


@pytest.mark.parametrize("c", GATE_SCORE_CASES, ids=gate_case_id)
def test_gate_score_walks(c):
    """Two rows per wave (D = 384; N = 1 and 37: the odd last row; N = 65539: rows 65536 and 65538 are the first waves' second
    grid-stride pass), float4 rows (64 and 65 float4 per branch half; N = 32771 at D = 4: 8193 row groups on 8192 workgroups) and scalar
    rows; p = 0 and 0.25 with the masks regenerated on the host, and one rng_row permutation per walk."""
    if c.N == 65539:
        assert gate_score_blocks(c.N) == GATE_SCORE_MAXBLK and 2 * 4 * GATE_SCORE_MAXBLK == 65536 < c.N
    if c.N == 32771:
        assert ceil_div(c.N, 4) == GATE_SCORE_MAXBLK + 1
    body_gate_score(c)


GateBwdCase = collections.namedtuple("GateBwdCase", "D N p perm pair32")
GATE_BWD_CASES = ([GateBwdCase(D, N, p, False, False) for D in (4, 20, 384, 1020, 1024) for N in (1, 31, 32, 33) for p in (0.0, 0.25)]
                  + [GateBwdCase(4, 32801, p, False, False) for p in (0.0, 0.25)]
                  + [GateBwdCase(D, 33, p, False, True) for D in (32, 384) for p in (0.0, 0.25)]
                  + [GateBwdCase(384, 33, 0.25, True, False), GateBwdCase(384, 33, 0.25, True, True)])


def pair32_columns(D):
    """Column of a_j and of b_j in the pair32 row layout: blocks of 32, a_j at 64 (j / 32) + j % 32, b_j 32 further."""
    j = torch.arange(D)
    ca = 64 * (j // 32) + j % 32
    return torch.cat([ca, ca + 32])


def restate_gate_bwd(inp, N, D, p, perm, dtype=torch.float64):
    """Closed form of d s / d (pre-activations) with a = tanh, b = sigmoid held as outputs: dG = [dGa | dGb], dwc, dbc, dbias."""
    ma, mb = gate_masks(N, D, p, perm, dtype)
    ab, wc, ds = inp["ab"].to(dtype), inp["wc"].to(dtype), inp["ds"].to(dtype)[:, None]
    a, b = ab[:, :D], ab[:, D:]
    ad, bd = a * ma, b * mb
    ga = ds * wc * bd * ma * (1 - a * a)
    gb = ds * wc * ad * mb * b * (1 - b)
    dG = torch.cat([ga, gb], 1)
    return dict(dG=dG.double(), dwc=(ds * ad * bd).sum(0).double(), dbc=ds.sum().reshape(1).double(), dbias=dG.sum(0).double())


def launch_gate_bwd(c):
    """The plain form, the planes output beside it, and the planes-only accumulating form."""
    ops = _ops()
    def make():
        inp = gate_inputs(c.N, c.D)
        d = {k: inp[k].to(DEV) for k in ("ab", "wc", "ds", "perm")}
        d["ab32"] = torch.zeros_like(inp["ab"]).index_copy_(1, pair32_columns(c.D), inp["ab"]).to(DEV) if c.D % 32 == 0 else None
        return d
    d = cached(_INPUTS, ("gatebwddev", c.N, c.D), make)
    ab = d["ab32"] if c.pair32 else d["ab"]
    seed = torch.tensor([GATE_SEED], dtype=torch.int64, device=DEV)
    kw = dict(rng_row=d["perm"] if c.perm else None, pair32=c.pair32)
    pl = ops.Planes.alloc((c.N, 2 * c.D), ab.device)
    dG, dwc, dbc, dbias = ops.gate_bwd(ab, d["ds"], d["wc"], c.N, c.D, c.p, seed, GATE_SA, GATE_SB, planes=pl, **kw)
    acc = [torch.ones(c.D, device=DEV), torch.ones(1, device=DEV), torch.ones(2 * c.D, device=DEV)]
    pl2 = ops.Planes.alloc((c.N, 2 * c.D), ab.device)
    none = ops.gate_bwd(ab, d["ds"], d["wc"], c.N, c.D, c.p, seed, GATE_SA, GATE_SB, dwc=acc[0], dbc=acc[1], dbias=acc[2], planes=pl2,
                        planes_only=True, **kw)[0]
    assert none is None
    return dict(dG=dG, dwc=dwc, dbc=dbc, dbias=dbias, pl=pl, pl2=pl2, acc=acc)


GATE_BWD_BOUND = {k: BOUND["grad"] for k in ("dG", "dwc", "dbc", "dbias", "acc_dwc", "acc_dbc", "acc_dbias")}


def body_gate_bwd(c):
    ops = _ops()
    inp = gate_inputs(c.N, c.D)
    perm = inp["perm"] if c.perm else None
    wide = c.N >= 32769

    def make():
        ref = restate_gate_bwd(inp, c.N, c.D, c.p, perm)
        ref["e32"] = None
        if wide:
            r32 = restate_gate_bwd(inp, c.N, c.D, c.p, perm, torch.float32)
            e = {k: relerr(r32[k], ref[k]) for k in ("dG", "dwc", "dbc", "dbias")}
            ref["e32"] = dict(e, acc_dwc=e["dwc"], acc_dbc=e["dbc"], acc_dbias=e["dbias"])
        return ref
    ref = cached(_REFS, ("gate_bwd", c.D, c.N, c.p, c.perm), make)
    assert rows_per_block(c.N) == (64 if c.N == 32801 else 32)
    got = launch_gate_bwd(c)
    dG = got["dG"].cpu()
    if c.pair32:
        dG = dG[:, pair32_columns(c.D)]
    err = dict(dG=relerr(dG, ref["dG"]), dwc=relerr(got["dwc"], ref["dwc"]), dbc=relerr(got["dbc"], ref["dbc"]), dbias=relerr(got["dbias"], ref["dbias"]))
    for k, t in zip(("dwc", "dbc", "dbias"), got["acc"]):              # the accumulating form adds the same sums
        err["acc_" + k] = relerr(t - 1.0, ref[k])
    judge("gate_bwd", gate_case_id(c), err, widen(GATE_BWD_BOUND, ref["e32"]))
    want = ops.split_planes(got["dG"])                                  # the planes are the split of the fp32 output, bit for bit
    for pl in (got["pl"], got["pl2"]):
        assert torch.equal(pl.hi, want.hi) and torch.equal(pl.lo, want.lo)
    return got


@pytest.mark.parametrize("c", GATE_BWD_CASES, ids=gate_case_id)
def test_gate_backward_walks(c):
    """One to 256 rows per pass (D = 1024 .. 4), D = 1020 with thread 255 idle, rows one short of, on and one past the 32-row block,
    64 rows per block at N = 32801, the pair32 row layout, the planes and the planes-only output and the accumulating form."""
    body_gate_bwd(c)


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm -> ReLU (-> mean over 16 rows)
# ------------------------------------------------------------------------------------------------------------------------------
LnCase = collections.namedtuple("LnCase", "d N content aligned planes dup acc kernel width")


def ln_case_id(c):
    return (f"{c.kernel}{c.width}-d{c.d}-N{c.N}-{c.content}" + ("" if c.aligned else "-off4") + ("-planes" if c.planes else "")
            + ("-dup" if c.dup == 2 else "") + ("-acc" if c.acc else ""))


def _ln_cases():
    qt = lambda d: next(q for lim, q in LN_QT_STEPS if d <= lim)   # noqa: E731
    out = [LnCase(d, 48, "offset", True, False, 1, False, "generic", qt(d)) for d in (4, 60, 64, 65, 129, 200, 320, 385, 500)]
    out += [LnCase(d, 48, "offset", False, False, 1, False, "generic", qt(d)) for d in (128, 256, 384, 512)]
    for d in (128, 256, 384, 512):
        out += [LnCase(d, 48, "offset", True, False, 1, False, "ln4", d // 128), LnCase(d, 48, "offset", True, True, 1, False, "ln4", d // 128),
                LnCase(d, 48, "offset", True, False, 2, False, "ln4", d // 128)]
    out += [LnCase(128, 16 * 2051, "offset", True, False, 1, False, "ln4", 1), LnCase(128, 16 * 2051, "offset", False, False, 1, False, "generic", 2)]
    out += [LnCase(128, 48, "offset", True, False, 1, True, "ln4", 1), LnCase(128, 48, "offset", False, False, 1, True, "generic", 2)]
    for content in ("bigmean", "const"):
        out += [LnCase(128, 32, content, True, False, 1, False, "ln4", 1), LnCase(128, 32, content, False, False, 1, False, "generic", 2)]
    return out


LN_CASES = _ln_cases()
LN_RELU_MARGIN = 2e-4       # bigmean: |pre-ReLU| of every entry stays clear of the kernels' round-off in z (rows near 1e3: 2^-14 per ulp)


def ln_inputs(N, d, content, rows=False):
    def make():
        g = _gen(31 * N + d + {"offset": 0, "bigmean": 1, "const": 2}[content])
        if content == "offset":                       # rows of their own scale and offset
            y = torch.randn(N, d, generator=g) * (0.5 + torch.rand(N, 1, generator=g)) + 2.0 * torch.randn(N, 1, generator=g)
        elif content == "bigmean":
            y = 1e3 + torch.randn(N, d, generator=g)
        else:
            y = torch.randn(N, 1, generator=g).expand(N, d).contiguous()
        return dict(y=y, gamma=1 + 0.1 * torch.randn(d, generator=g), beta=0.1 * torch.randn(d, generator=g),
                    ge=torch.randn(N if rows else N // 16, d, generator=g))
    return cached(_INPUTS, ("ln", N, d, content, rows), make)


def restate_ln(inp, N, d, pool16, dtype=torch.float64, eps=1e-5):
    y, gm, bt = (inp[k].detach().to(dtype).requires_grad_(True) for k in ("y", "gamma", "beta"))
    pre = torch.nn.functional.layer_norm(y, (d,), gm, bt, eps)
    z = torch.relu(pre)
    emb = z.reshape(N // 16, 16, d).mean(1) if pool16 else z
    (emb * inp["ge"].to(dtype)).sum().backward()
    with torch.no_grad():
        mean = y.mean(1)
        rstd = torch.rsqrt(((y - mean[:, None]) ** 2).mean(1) + eps)
    return dict(emb=emb.detach().double(), mean=mean.double(), rstd=rstd.double(), dy=y.grad.double(), dgamma=gm.grad.double(),
                dbeta=bt.grad.double(), ycol=y.grad.sum(0).double(), pre_min=float(pre.detach().abs().min()),
                dz_mag=float(((pre.detach() > 0) * inp["ge"].to(dtype).repeat_interleave(16 if pool16 else 1, 0) / (16 if pool16 else 1)).abs().sum(0).max()))


def launch_ln(c):
    ops = _ops()
    def make():
        inp = ln_inputs(c.N, c.d, c.content)
        d = {k: inp[k].to(DEV) for k in ("gamma", "beta", "ge")}
        d["y"] = inp["y"].to(DEV) if c.aligned else off_by_one_float(inp["y"])
        return d
    dv = cached(_INPUTS, ("lndev", c.N, c.d, c.content, c.aligned), make)
    y = dv["y"]
    w = ln_walk(c.d, y.data_ptr() % 16 == 0, c.planes, c.dup)
    assert w == LnWalk(c.kernel, c.width), (w, c)
    assert c.dup == 1 or ops.ln_relu_mean16_dup_ok(c.d)
    nreg = c.N // 16
    epl = ops.Planes.alloc((nreg, c.d), y.device) if c.planes else None
    emb, mean, rstd = ops.ln_relu_mean16_fwd(y, dv["gamma"], dv["beta"], c.N, c.d, 1e-5, planes=epl, dup=c.dup)
    demb = torch.cat([dv["ge"], dv["ge"]]) if c.dup == 2 else dv["ge"]
    ycol = torch.full((c.d,), 0.5, device=DEV)
    dg0 = torch.full((c.d,), 0.25, device=DEV) if c.acc else None
    db0 = torch.full((c.d,), -0.25, device=DEV) if c.acc else None
    dy, dg, db = ops.ln_relu_mean16_bwd(demb, y, dv["gamma"], dv["beta"], mean, rstd, c.N, c.d, dg_out=dg0, db_out=db0, ycol_out=ycol, dup=c.dup)
    out = dict(emb=emb, mean=mean, rstd=rstd, dy=dy, dgamma=dg, dbeta=db, ycol=ycol)
    if c.planes:                                      # dy as operand planes only, and the embedding's planes
        dpl = ops.Planes.alloc((c.N, c.d), y.device)
        _, dg2, db2 = ops.ln_relu_mean16_bwd(demb, y, dv["gamma"], dv["beta"], mean, rstd, c.N, c.d, planes=dpl, dup=c.dup)
        out.update(epl=epl, dpl=dpl, dgamma2=dg2, dbeta2=db2)
    return out


LN_BOUND = dict(emb=BOUND["ln_out"], mean=BOUND["ln_out"], rstd=BOUND["ln_out"], dy=BOUND["ln_grad"], dgamma=BOUND["ln_grad"],
                dbeta=BOUND["ln_grad"], ycol=BOUND["ln_grad"])


def ln_errors(got, ref, c):
    k2 = 2.0 if c.dup == 2 else 1.0                   # [emb; emb] fed two stacked passes: the backward sums the halves of demb
    nreg = c.N // 16
    emb = got["emb"][:nreg]
    dgamma = relerr(got["dgamma"] - (0.25 if c.acc else 0.0), k2 * ref["dgamma"])
    if c.content == "const":      # x-hat is exactly 0 in float64, so dgamma = sum dz x-hat is: measured against its uncancelled magnitude sum |dz| (|x-hat| <= 1)
        dgamma = float(got["dgamma"].detach().cpu().double().abs().max() / ref["dz_mag"])
    return dict(emb=relerr(emb, ref["emb"]), mean=relerr(got["mean"], ref["mean"]), rstd=relerr(got["rstd"], ref["rstd"]),
                dy=relerr(got["dy"], k2 * ref["dy"]), dgamma=dgamma,
                dbeta=relerr(got["dbeta"] + (0.25 if c.acc else 0.0), k2 * ref["dbeta"]), ycol=relerr(got["ycol"] - 0.5, k2 * ref["ycol"]))


def body_ln(c):
    ops = _ops()
    inp = ln_inputs(c.N, c.d, c.content)
    wide = c.d >= 500 and c.content == "offset"

    def make():
        ref = restate_ln(inp, c.N, c.d, True)
        ref["e32"] = None
        if wide:
            r32 = restate_ln(inp, c.N, c.d, True, torch.float32)
            ref["e32"] = {k: relerr(r32[k], ref[k]) for k in LN_BOUND}
        return ref
    ref = cached(_REFS, ("ln", c.N, c.d, c.content), make)
    if c.content == "bigmean":
        assert ref["pre_min"] > LN_RELU_MARGIN, ref["pre_min"]
    got = launch_ln(c)
    judge("ln", ln_case_id(c), ln_errors(got, ref, c), widen(LN_BOUND, ref["e32"]))
    if c.dup == 2:
        nreg = c.N // 16
        assert torch.equal(got["emb"][:nreg], got["emb"][nreg:])
    if c.planes:
        we, wd = ops.split_planes(got["emb"]), ops.split_planes(got["dy"])
        assert torch.equal(got["epl"].hi, we.hi) and torch.equal(got["epl"].lo, we.lo)
        assert torch.equal(got["dpl"].hi, wd.hi) and torch.equal(got["dpl"].lo, wd.lo)            # test_layernorm_backward_hands_dy_over_as_operand_planes
        assert torch.equal(got["dgamma2"], got["dgamma"]) and torch.equal(got["dbeta2"], got["dbeta"])
    if c.content == "const":                          # every row constant: the output is relu(beta), rstd = rsqrt(eps)
        want = torch.relu(inp["beta"].double())
        assert float((got["emb"].cpu().double() - want).abs().max()) <= BOUND["ln_out"] * float(want.max())
        assert relerr(got["rstd"], torch.full((c.N,), 1e-5, dtype=torch.float64).rsqrt()) < BOUND["ln_out"]
    for k in ("emb", "mean", "rstd", "dy", "dgamma", "dbeta", "ycol"):
        assert bool(torch.isfinite(got[k]).all()), k
    return got


@pytest.mark.parametrize("c", LN_CASES, ids=ln_case_id)
def test_layernorm_mean16_walks(c):
    """QT 2 / 4 / 6 / 8 with ragged last column groups; d % 128 == 0 one float off alignment (leaves the 16-byte kernels); NV 1 .. 4
    with the planes outputs and dup = 2; 2051 regions on 2048 workgroups (the backward's grid-stride) on either family; the accumulating
    form; rows near 1e3 (the kernels centre before squaring) and constant rows."""
    if c.N == 16 * 2051:
        assert ln_bwd_blocks(c.N // 16) == LN_BWD_MAXBLK < c.N // 16
    body_ln(c)


LnRowsCase = collections.namedtuple("LnRowsCase", "d N")
LN_ROWS_CASES = [LnRowsCase(d, N) for d in (256, 200) for N in (1, 15, 16, 17, 37)]


def launch_ln_rows(c):
    ops = _ops()
    inp = ln_inputs(c.N, c.d, "offset", rows=True)
    lv = [inp[k].to(DEV).requires_grad_(True) for k in ("y", "gamma", "beta")]
    out = ops.ln_relu(*lv)
    (out * inp["ge"].to(DEV)).sum().backward()
    return dict(emb=out.detach(), dy=lv[0].grad, dgamma=lv[1].grad, dbeta=lv[2].grad)


def body_ln_rows(c):
    inp = ln_inputs(c.N, c.d, "offset", rows=True)
    ref = cached(_REFS, ("lnrows", c.N, c.d), lambda: restate_ln(inp, c.N, c.d, False))
    assert ln_walk(c.d, False).kernel == "generic"                     # the rows form has no 16-byte kernel
    got = launch_ln_rows(c)
    judge("ln_rows", f"d{c.d}-N{c.N}", {k: relerr(got[k], ref[k]) for k in ("emb", "dy", "dgamma", "dbeta")},
          {k: LN_BOUND[k] for k in ("emb", "dy", "dgamma", "dbeta")})
    return got


@pytest.mark.parametrize("c", LN_ROWS_CASES, ids=lambda c: f"d{c.d}-N{c.N}")
def test_layernorm_rows_form(c):
    """ln_relu (pool16 = 0): row counts around the 16-row region, at d = 256 and at d = 200."""
    body_ln_rows(c)


# ------------------------------------------------------------------------------------------------------------------------------
# colsum and act_dropout_bwd
# ------------------------------------------------------------------------------------------------------------------------------
ColsumCase = collections.namedtuple("ColsumCase", "M N acc aligned form chunks")
COLSUM_CASES = ([ColsumCase(M, 260, acc, al, "direct" if al else "merged", 1) for M in (1, 32) for acc in (False, True) for al in (True, False)]
                + [ColsumCase(M, N, False, True, form, ch) for N, ch in ((1024, 1), (1028, 2), (2052, 3)) for M, form in ((32, "direct"), (100, "merged"))]
                + [ColsumCase(32801, 4, acc, True, "merged", 1) for acc in (False, True)])


def colsum_case_id(c):
    return f"{c.form}-M{c.M}-N{c.N}" + ("-acc" if c.acc else "") + ("" if c.aligned else "-off4")


def colsum_input(M, N):
    return cached(_INPUTS, ("colsum", M, N), lambda: torch.randn(M, N, generator=_gen(M + 3 * N)) + 0.25)


def launch_colsum(c):
    ops = _ops()
    x = cached(_INPUTS, ("colsumdev", c.M, c.N), lambda: colsum_input(c.M, c.N).to(DEV))
    out = torch.ones(c.N, device=DEV) if c.aligned else off_by_one_float(torch.ones(c.N))
    w = colsum_walk(c.M, c.N, out.data_ptr() % 16 == 0)
    assert (w.form, w.chunks) == (c.form, c.chunks) and w.rpb == (64 if c.M == 32801 else 32), (w, c)
    if c.acc:
        ops.colsum(x, c.M, c.N, out=out)
        return dict(sum=out - 1.0)
    # the store form through the C entry point, so that the destination can be the misaligned view
    from advmil_amd import _lib
    L = _lib.lib()
    wsb = L.advmil_colsum_workspace_bytes(c.M, c.N)
    ws = ops._ws(wsb, x.device)
    _lib.check(L.advmil_colsum(ops._p(x), c.M, c.N, ops._p(out), 0, ops._p(ws), wsb, ops._stream()), "colsum")
    return dict(sum=out.clone())


def body_colsum(c):
    x = colsum_input(c.M, c.N)
    wide = c.M >= 32769

    def make():
        ref = dict(sum=x.double().sum(0), e32=None)
        if wide:
            ref["e32"] = dict(colsum=relerr(x.sum(0), ref["sum"]))
        return ref
    ref = cached(_REFS, ("colsum", c.M, c.N), make)
    got = launch_colsum(c)
    judge("colsum", colsum_case_id(c), dict(colsum=relerr(got["sum"], ref["sum"])), widen(dict(colsum=BOUND["colsum"]), ref["e32"]))
    return got


@pytest.mark.parametrize("c", COLSUM_CASES, ids=colsum_case_id)
def test_colsum_walks(c):
    """direct (one block sees every row; store and add) and, with the destination one float off alignment, the merged walk with the
    same sums; one, two and three column chunks (the last 4 columns wide); 64 rows per block at M = 32801."""
    body_colsum(c)


ActBwdCase = collections.namedtuple("ActBwdCase", "act p M N acc bits")
ACT_BWD_CASES = ([ActBwdCase(act, p, 32, 260, acc, False) for act in ("none", "relu", "tanh", "sigmoid") for p in (0.0, 0.25) for acc in (False, True)]
                 + [ActBwdCase("relu", 0.25, 100, 2052, False, False), ActBwdCase("relu", 0.25, 33, 1056, False, True),
                    ActBwdCase("relu", 0.25, 32, 1056, False, True)])
ACT_SID = 5
ACT64 = {"none": lambda v: v, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}
ACT_GRAD = {"none": lambda a: torch.ones_like(a), "relu": lambda a: (a > 0).to(a.dtype), "tanh": lambda a: 1 - a * a, "sigmoid": lambda a: a * (1 - a)}


def act_bwd_inputs(c):
    def make():
        g = _gen(c.M + c.N)
        pre = torch.randn(c.M, c.N, generator=g)
        a = ACT64[c.act](pre)                          # float32 activation output
        keep = H.T(synth.dropout_keep(GATE_SEED, ACT_SID, c.M * c.N, c.p).reshape(c.M, c.N)) if c.p > 0 else torch.ones(c.M, c.N, dtype=torch.bool)
        y = a * keep / (1 - c.p)                       # what the forward left: dropout(act(pre))
        return dict(a=a, keep=keep, y=y, dy=torch.randn(c.M, c.N, generator=g) + 0.25)
    return cached(_INPUTS, ("act", c.act, c.p, c.M, c.N), make)


def launch_act_bwd(c):
    ops = _ops()
    inp = act_bwd_inputs(c)
    dv = cached(_INPUTS, ("actdev", c.act, c.p, c.M, c.N), lambda: dict(y=inp["y"].to(DEV), dy=inp["dy"].to(DEV)))
    w = colsum_walk(c.M, c.N, True)
    seed = torch.tensor([GATE_SEED], dtype=torch.int64, device=DEV)
    acc = torch.ones(c.N, device=DEV) if c.acc else None
    bits = torch.empty(c.M, c.N // 32, dtype=torch.int32, device=DEV) if c.bits else None
    pl = ops.Planes.alloc((c.M, c.N), DEV)
    assert (acc is None or acc.data_ptr() % 16 == 0) and w.form == ("direct" if c.M <= 32 else "merged")
    dpre, db = ops.act_dropout_bwd(dv["dy"], dv["y"], ops._ACT[c.act], c.M, c.N, c.p, seed, ACT_SID, db_out=acc, planes=pl, bits=bits)
    out = dict(dpre=dpre, db=(db - 1.0) if c.acc else db, pl=pl)
    if c.bits:
        out["bits"] = bits
    return out


def body_act_bwd(c):
    ops = _ops()
    inp = act_bwd_inputs(c)
    ref = inp["dy"].double() * inp["keep"].double() / (1 - c.p) * ACT_GRAD[c.act](inp["a"].double())
    got = launch_act_bwd(c)
    judge("act_bwd", "-".join(str(v) for v in c), dict(dpre=relerr(got["dpre"], ref), db=relerr(got["db"], ref.sum(0))),
          dict(dpre=BOUND["grad"], db=BOUND["grad"]))
    want = ops.split_planes(got["dpre"])
    assert torch.equal(got["pl"].hi, want.hi) and torch.equal(got["pl"].lo, want.lo)
    if c.bits:                                        # one bit per element, 32 columns per word: dpre > 0
        b = got["bits"].cpu().numpy().view("uint32")
        un = ((b[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(c.M, c.N).astype(bool)
        assert (un == (got["dpre"].cpu().numpy() > 0)).all()
    return got


@pytest.mark.parametrize("c", ACT_BWD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_activation_dropout_backward_walks(c):
    """dy * keep * act'(y) with the masks regenerated on the host, every activation at p = 0 and 0.25; the bias gradient stored and
    added, direct (M = 32) and merged (M = 33, 100); three column chunks; the bit mask at N = 1056 (last chunk 32 columns wide)."""
    if c.N == 1056:
        assert c.N - COLSUM_CHUNK == 32
    body_act_bwd(c)


# ------------------------------------------------------------------------------------------------------------------------------
# the parametrisation reaches every walk the mirrors name
# ------------------------------------------------------------------------------------------------------------------------------
def walks_reached():
    """Worked out on the host from the case lists alone (tests/test_row_walks_plan_cpu.py calls this too)."""
    got = set()
    for c in POOL_CASES + REGIME_CASES:
        mlen = sum(c.lens) if c.cap else max(c.lens)
        w = pool_walk(mlen, c.D)
        assert (w.form, w.rpb) == (c.form, c.rpb), c
        got.add(("pool", w.form, w.rpb))
        got.add(("pool_nblk>1", w.nblk > 1))
        if pool_walk(mlen, c.D, planes=True):
            got.add(("pool_bwd", "planes"))
        got.add(("pool_bwd", pool_bwd_walk(c.D, c.D + c.pad)))
    for c in POOL_BWD_CASES:
        assert pool_bwd_walk(c.D, c.D + c.pad, c.walk == "planes") == c.walk, c
        got.add(("pool_bwd", c.walk))
    for c in GATE_SCORE_CASES:
        assert gate_score_walk(c.D) == c.walk, c
        got.add(("gate_score", c.walk))
    for c in LN_CASES:
        assert ln_walk(c.d, c.aligned, c.planes, c.dup) == LnWalk(c.kernel, c.width), c
        got.add((c.kernel, c.width))
    for c in LN_ROWS_CASES:
        got.add(("generic", ln_walk(c.d, False).width))
    for c in COLSUM_CASES:
        w = colsum_walk(c.M, c.N, c.aligned)
        assert (w.form, w.chunks) == (c.form, c.chunks), c
        got.add(("colsum", w.form)); got.add(("colsum_chunks", w.chunks)); got.add(("colsum_rpb", w.rpb))
    for c in ACT_BWD_CASES:
        got.add(("act_bwd", colsum_walk(c.M, c.N, True).form))
    return got


WALKS_WANTED = ({("pool", "online", r) for r in (32, 64, 512)} | {("pool", "stats4", r) for r in (32, 64, 512)} | {("pool", "stats8", 512)}
                | {("pool_bwd", w) for w in ("planes", "float4", "scalar")} | {("gate_score", w) for w in ("pair", "float4", "scalar")}
                | {("generic", q) for q in (2, 4, 6, 8)} | {("ln4", v) for v in (1, 2, 3, 4)}
                | {("colsum", f) for f in ("direct", "merged")} | {("act_bwd", f) for f in ("direct", "merged")}
                | {("colsum_chunks", n) for n in (1, 2, 3)} | {("colsum_rpb", 32), ("colsum_rpb", 64)})


def test_every_walk_is_reached():
    """online x rows per block {32, 64, 512}, stats4, stats8, the three backward walks, the three gate-score walks, QT {2, 4, 6, 8},
    NV {1 .. 4}, direct and merged: each is asserted by at least one case above. (stats8 needs more than 2048 blocks per segment, which
    only 512 rows per block can leave: it has no 32- or 64-row form.)"""
    missing = WALKS_WANTED - walks_reached()
    assert not missing, sorted(missing)
    if WORST:
        for fam, (r, case, k) in sorted(WORST.items()):
            print(f"worst of {fam}: {r:.3f} of its bound ({k}, {case})")
