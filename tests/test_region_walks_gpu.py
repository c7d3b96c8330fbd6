"""GPU: every walk of the discriminator's fused region network (csrc/region.hip: dx_chain_fwd_kernel, dx_chain_prep_kernel,
dx_chain_bwd_kernel, and ops.DxRegionPoolFn over them) against the float64 restatement tests/region_ref.py, which
tests/test_region_ref_cpu.py pins to float64 autograd and to the reference modules.

Direct calls of advmil_dx_chain_fwd / _prep / _bwd through _lib.lib(): free-standing weights (H.synth_params) split with
ops.split_planes, randn rows, no arena and no optimizer. Every dropout draw (dx_fc1 at row * 64 + c, the two gate branches at row * 128 + j,
rows through rng_row when given) is regenerated on the host (region_ref.keep_masks). tests/test_region_gpu.py compares the fused path with
the layer-by-layer path only, and the two share their draws, their activation code, their bf16x3 split, their pooling backward and
their h1 > 0 mask convention; here nothing is shared with the code under test but the inputs.

Forward (FWD_CASES): R = 1, 63, 64, 65, 127, 193 x {no dropout, p1 only, pg only, both, both with seed == NULL (= none)} x {no row
map, a permuted map with ids up to ~2^20} x {h1 / ab given, NULL (fc and s keep their bits)} x {bc given, NULL} -- a covering set:
every value, every (dropout, map) pair, R = 65 and 127 with both draws on. Prep: the six transposed planes bit-equal to
boundary.split_bf16 of the transposed weights. Backward (BWD_CASES): the kernel gets the FORWARD KERNEL'S OWN h1 / ab; A, ds, dpooled,
dmean, dfc_add come from the oracle, rounded to float32, pooling scores at the project's 3 * randn scale; the oracle's backward uses the
same h1 > 0 and the same a, b, so no ReLU branch is open and every entry of dG, dfc, dpre, de, of the five summed vectors, and of the three
weight gradients (dG^T fc, dfc^T h1, dpre^T e, formed here in float64 from the kernel's rows) is compared. Bags [1], [63], [64], [65],
[200], [1, 300], [30, 1, 20, 77, 64]; rowseg / seg_ptr NULL or given; dmean / dfc_add / de NULL or given; destinations zero or pre-filled
(the merge accumulates); the workspace pre-filled with NaN bytes (RC_PART's three pad columns must reach nothing); 1, 2, 3, 4 and 5 tiles.
Every output buffer carries one guard row behind row R - 1, which must keep its bits (tail rows are not written).

Wrapper (WRAP_CASES): ops.dx_region_pool through build_disc + FlatAdam in train mode, lens [130, 1, 61], the loss over pooled, mean AND
fc (so dfc_ext enters the kernel), compared end to end with the oracle: fc, A, pooled, mean, the arena's parameter gradients and e.grad.
There the ReLU branch is the kernel's own to take: the input seed WRAP_E_SEED = 48 was found on the CPU by walking torch.Generator seeds
0, 1, 2, ... for the first whose float64 Z1 = e W1^T + b1 has min abs(Z1) well clear of boundary.DEEP_DELTA = 8e-5 (seed 48: 7.9e-4;
nineteen of the first sixty seeds clear 8e-5 at all); the test asserts min abs(Z1) >= DEEP_DELTA at run time.

Bounds, relative to the largest entry of the oracle tensor, + 1e-7: fc 2e-5, A 1e-4, pooled and mean 5e-5, every gradient 5e-5
(tests/test_region_gpu.py, the last one also BOUND['grad'] of tests/test_row_walks_gpu.py), s 1e-5 (BOUND['score'] there). pool.fc2.bias /
dbc, whose true value is the cancelling sum of ds: the 5e-6 floor tests/test_region_gpu.py::_close gives it. Without a project bound:
h1 and ab are held to fc's 2e-5, dG and dpre to the gradients' 5e-5, and each of these and s to max(that, 4 e_emul), e_emul = the error of
a CPU emulation of the documented arithmetic (boundary.emulated_matmul(..., 'bf16x3') products, float32 activations and sums) against the
oracle on the same inputs; 4 for the summation order and the hardware exp2 / rcp. No figure is taken from the kernels.

Measured on an MI355X when this file was written, worst error over the bound in force per output (every case prints its figures,
`test_every_walk_is_reached` prints the worst of each output):
  forward   fc 0.49 of 2e-5 (9.9e-6 at max abs(fc) 1.5, R = 1, both draws). With the widened bound in force: h1 0.26 (2.7e-5 of 1.0e-4,
            R = 127 both), ab 0.26 (2.6e-5 of 9.8e-5, R = 64 p1), s 0.30 (1.2e-5 of 4.0e-5, R = 193 noseed).
            ab and s needed the widened bound in EVERY forward case, h1 in four (R = 1 none, R = 1 both, R = 64 noseed, R = 127 both): ab is
            1.0e-5 .. 2.8e-5 from float64 against a project bound of 2e-5, s 1.0e-6 .. 1.8e-5 against 1e-5 max abs(s) ~ 1e-5, and the CPU
            emulation of bf16x3 is as far from float64 as the kernel is (kernel error / e_emul 0.8 .. 1.2): the distance is the
            arithmetic's -- the dropped lo x lo products of three chained contractions --, not the kernel's.
  backward  dG 0.005, dfc 0.019, dpre 0.15, de 0.18, dwc 0.004, dbab 0.006, dbc 0.042 (of the 5e-6 floor), db2 0.006, db1 0.13,
            dWab 0.005, dW2 0.014, dW1 0.15 of 5e-5. No backward case needed the widened bound.
  wrapper   fc <= 0.49 of 2e-5, A 0.003 of 1e-4, pooled and mean 0.18 of 5e-5, de <= 0.18, parameter gradients 0.002 (fc1.3.bias) .. 0.34 (pool.fc1.0.weight) of 5e-5,
            pool.fc2.bias 0.08 of its floor.

Found by reading, pinned here: with seed == NULL and p1 > 0 the forward applied no dropout, while the backward still scaled dpre by
1 / (1 - p1) (the Python wrapper never passes that combination; the header offers it). dx_chain_bwd_kernel now takes the scale from
`g.seed && g.p1 > 0`, as the forward does; the `noseed` backward cases fail without that line (dpre, de, db1, dW1 off by 4/3)."""
import collections

import numpy as np
import pytest
import torch

from tests import boundary
from tests import helpers as H
from tests import region_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# csrc/region.hip (tests/test_region_walks_plan_cpu.py pins them to the source text and to the library's workspace arithmetic)
RC_ROWS, RC_D, RC_H = 64, 128, 64
RC_PART = 3 * RC_D + 4 + RC_D + RC_H
RC_PART_PAD = (3 * RC_D + 1, 3 * RC_D + 4)            # columns [385, 388): written by nobody, read by nobody

PREFIX = "D-prj:net_pair_one."
P_DROP = 0.25
SEED, SIDS = 77, (3, 5, 9)
GUARD = 12345.5

#                   p1      pg      seed given
MODES = {"none": (0.0, 0.0, True), "p1": (P_DROP, 0.0, True), "pg": (0.0, P_DROP, True), "both": (P_DROP, P_DROP, True),
         "noseed": (P_DROP, P_DROP, False)}

FLOOR = 1e-7
TOL = dict(fc=2e-5, A=1e-4, pooled=5e-5, mean=5e-5, grad=5e-5, s=1e-5)
DBC_FLOOR = 5e-6                                      # tests/test_region_gpu.py::_close, pool.fc2.bias
FWD_TOL = dict(h1=TOL["fc"], fc=TOL["fc"], ab=TOL["fc"], s=TOL["s"])
FWD_WIDEN = ("h1", "ab", "s")
BWD_OUT = ("dG", "dfc", "dpre", "de", "dwc", "dbab", "dbc", "db2", "db1", "dWab", "dW2", "dW1")
BWD_WIDEN = ("dG", "dpre")

FwdCase = collections.namedtuple("FwdCase", "R mode rmap nograd bc")
FWD_CASES = [
    FwdCase(1, "none", False, True, True),
    FwdCase(63, "none", True, False, True),
    FwdCase(64, "p1", False, False, True),
    FwdCase(65, "p1", True, True, False),
    FwdCase(127, "pg", False, False, True),
    FwdCase(193, "pg", True, False, True),
    FwdCase(65, "both", False, True, True),
    FwdCase(127, "both", True, True, True),
    FwdCase(193, "noseed", False, False, True),
    FwdCase(64, "noseed", True, False, True),
    FwdCase(193, "both", True, False, False),
    FwdCase(1, "both", True, False, True),
    FwdCase(63, "both", False, False, True),
]

BwdCase = collections.namedtuple("BwdCase", "lens seg dmean add de mode rmap prefill")
BWD_CASES = [
    BwdCase((1,), False, True, False, True, "none", False, False),
    BwdCase((63,), True, False, True, True, "p1", True, True),
    BwdCase((64,), False, True, True, False, "pg", False, False),
    BwdCase((65,), True, True, False, True, "both", True, True),
    BwdCase((200,), False, True, True, True, "both", False, False),
    BwdCase((1, 300), True, True, True, True, "noseed", False, True),
    BwdCase((30, 1, 20, 77, 64), True, True, True, True, "both", True, True),
    BwdCase((30, 1, 20, 77, 64), True, False, False, False, "none", True, False),
    BwdCase((65,), False, False, True, True, "p1", False, False),
    BwdCase((1, 300), True, True, False, True, "pg", True, False),
    BwdCase((64,), True, True, True, True, "noseed", True, False),
    BwdCase((63,), False, False, False, True, "both", False, True),
]
POISON_CASE = BWD_CASES[6]                            # tests/test_poison_kernels_gpu.py runs this one under three_runs

WrapCase = collections.namedtuple("WrapCase", "want_mean e_grad frozen rmap")
WRAP_LENS = (130, 1, 61)
WRAP_E_SEED = 48
WRAP_CASES = [WrapCase(True, True, False, False), WrapCase(False, True, False, False), WrapCase(True, False, False, False),
              WrapCase(True, True, True, False), WrapCase(True, True, False, True)]


def ceil_div(a, b):
    return -(-a // b)


def tiles(R):
    return ceil_div(R, RC_ROWS)


def cid(c):
    return "-".join(("x".join(str(x) for x in v) if isinstance(v, tuple) else f"{k}{int(v)}" if isinstance(v, bool) else str(v))
                    for k, v in c._asdict().items())


# ------------------------------------------------------------------------------------------------------------------------------
# shared inputs: computed once, never modified
# ------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}
WORST = {}                                            # output -> (error / bound, case, widened?)
WIDENED = set()                                       # (case, output) whose 4 e_emul exceeded the project bound


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _ops():
    from advmil_amd import _lib, ops
    _lib.lib()
    return ops


def host_params():
    """fp32 torch tensors keyed like region_ref.KEYS, and their float64 numpy image."""
    def make():
        P32 = H.synth_params(RR.shapes(), PREFIX)
        return P32, {k: v.double().numpy() for k, v in P32.items()}
    return cached("params", make)


def dev_params():
    """Device operands of the entry points: planes of W1, W2, [Wa; Wb], the biases, wc, bc, and the transposed planes from prep."""
    def make():
        ops = _ops()
        from advmil_amd import _lib
        P32, _ = host_params()
        d = {k: P32[k].to(DEV) for k in ("fc1.0.weight", "fc1.3.weight", "fc1.0.bias", "fc1.3.bias")}
        d["Wab"] = torch.cat([P32["pool.fc1.0.weight"], P32["pool.score.0.weight"]]).to(DEV)
        d["bab"] = torch.cat([P32["pool.fc1.0.bias"], P32["pool.score.0.bias"]]).to(DEV)
        d["wc"] = P32["pool.fc2.weight"].reshape(-1).to(DEV)
        d["bc"] = P32["pool.fc2.bias"].to(DEV)
        d["W1pl"], d["W2pl"], d["Wabpl"] = (ops.split_planes(d[k]) for k in ("fc1.0.weight", "fc1.3.weight", "Wab"))
        d["W1T"], d["W2T"], d["WabT"] = (ops.Planes.alloc(s, DEV) for s in ((RC_D, RC_H), (RC_H, RC_D), (RC_D, 2 * RC_D)))
        p = ops._p
        _lib.check(_lib.lib().advmil_dx_chain_prep(p(d["fc1.0.weight"]), p(d["fc1.3.weight"]), p(d["Wab"]), RC_D, p(d["W1T"].hi), p(d["W1T"].lo),
                                                  p(d["W2T"].hi), p(d["W2T"].lo), p(d["WabT"].hi), p(d["WabT"].lo), ops._stream()), "dx_chain_prep")
        d["seed"] = torch.tensor([SEED], dtype=torch.int64, device=DEV)
        return d
    return cached("dev_params", make)


def rows_in(R):
    """e [R, 128] and the backward's cotangents and pooling scores for R rows (fp32, host)."""
    def make():
        g = torch.Generator().manual_seed(1000 + R)
        return dict(e=torch.randn(R, RC_D, generator=g), s_pool=3.0 * torch.randn(R, generator=g), dfc_add=torch.randn(R, RC_D, generator=g),
                    dp=torch.randn(8, RC_D, generator=g), dm=torch.randn(8, RC_D, generator=g),
                    pre={k: torch.randn(n, generator=g) for k, n in (("dwc", RC_D), ("dbab", 2 * RC_D), ("dbc", 1), ("db2", RC_D), ("db1", RC_H))})
    return cached(("rows", R), make)


def row_map(R):
    """A permuted row map whose ids reach about 2^20, none of them a local row number."""
    def make():
        g = torch.Generator().manual_seed(7 + R)
        ids = torch.randperm(R, generator=g) * ((1 << 20) // R) + 4099
        assert int(ids.min()) > R and (R == 1 or int(ids.max()) > (1 << 20) - 2 * ((1 << 20) // R)) and len(set(ids.tolist())) == R
        return ids
    return cached(("rmap", R), make)


def masks_of(R, mode, rmap):
    p1, pg, seeded = MODES[mode]
    if not seeded:
        p1 = pg = 0.0
    return cached(("masks", R, mode, rmap), lambda: RR.keep_masks(SEED, SIDS, R, p1, pg, row_map(R).numpy() if rmap else None)), p1, pg


def oracle_fwd(R, mode, rmap, bc=True):
    def make():
        _, P64 = host_params()
        P = P64 if bc else {k: v for k, v in P64.items() if k != "pool.fc2.bias"}
        masks, p1, pg = masks_of(R, mode, rmap)
        h1, fc, a, b, s = RR.fwd(P, rows_in(R)["e"].numpy(), *masks, p1=p1, pg=pg)
        return dict(h1=h1, fc=fc, a=a, b=b, ab=np.concatenate([a, b], 1), s=s)
    return cached(("ofwd", R, mode, rmap, bc), make)


def _scale32(keep, p):
    return 1.0 if keep is None else torch.from_numpy(keep).float() / (1.0 - p)


def emulate_fwd(R, mode, rmap, bc=True):
    """The documented arithmetic on the CPU: bf16x3 products (hi hi + hi lo + lo hi, fp32 accumulate), fp32 activations and sums."""
    def make():
        P32, _ = host_params()
        masks, p1, pg = masks_of(R, mode, rmap)
        m1, ma, mb = (_scale32(k, p) for k, p in zip(masks, (p1, pg, pg)))
        mm = boundary.emulated_matmul
        h1 = torch.relu(mm(rows_in(R)["e"], P32["fc1.0.weight"], "bf16x3") + P32["fc1.0.bias"]) * m1
        fc = mm(h1, P32["fc1.3.weight"], "bf16x3") + P32["fc1.3.bias"]
        a = torch.tanh(mm(fc, P32["pool.fc1.0.weight"], "bf16x3") + P32["pool.fc1.0.bias"])
        b = torch.sigmoid(mm(fc, P32["pool.score.0.weight"], "bf16x3") + P32["pool.score.0.bias"])
        s = ((a * ma) * (b * mb) * P32["pool.fc2.weight"].reshape(-1)).sum(1) + (P32["pool.fc2.bias"] if bc else 0.0)
        return dict(h1=h1, fc=fc, ab=torch.cat([a, b], 1), s=s)
    return cached(("efwd", R, mode, rmap, bc), make)


def maxerr(got, want):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max())


def project_bound(tol, want, floor=FLOOR):
    return tol * float(np.abs(np.asarray(want, dtype=np.float64)).max()) + floor


def judge(case, err, bound, widened=()):
    """Print every figure, keep each output's worst ratio, then assert."""
    print(f"[region] {case}: " + " ".join(f"{k} {err[k]:.2e}/{bound[k]:.1e}{'*' if k in widened else ''}" for k in err))
    for k in err:
        r = err[k] / bound[k]
        if r > WORST.get(k, (0.0,))[0]:
            WORST[k] = (r, case, k in widened)
        if k in widened:
            WIDENED.add((case, k))
    for k in err:
        assert err[k] <= bound[k], (case, k, err[k], bound[k])


def guarded(R, width, dtype=torch.float32):
    """[R + 1, width] fresh block whose last row is the guard; -> (the block, its first R rows)."""
    buf = torch.empty(R + 1, width, dtype=dtype, device=DEV)
    buf[R].fill_(GUARD)
    return buf, buf[:R]


def guards_intact(bufs, R):
    for k, b in bufs.items():
        assert bool((b[R] == GUARD).all()), f"{k}: row {R} (behind the last row) was written"


# ------------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------------
def launch_fwd(R, mode, rmap, keep=True, bc=True, rates=None):
    """One call of advmil_dx_chain_fwd -> dict h1, fc, ab, s (device; h1 / ab None when not kept). rates: (p1, pg) instead of the mode's."""
    ops = _ops()
    from advmil_amd import _lib
    d, p = dev_params(), ops._p
    p1, pg, seeded = MODES[mode]
    if rates is not None:
        p1, pg = rates
    e = cached(("edev", R), lambda: rows_in(R)["e"].to(DEV))
    rr = cached(("rmapdev", R), lambda: row_map(R).to(DEV)) if rmap else None
    bufs = {"fc": guarded(R, RC_D), "s": guarded(R, 1)}
    if keep:
        bufs.update(h1=guarded(R, RC_H), ab=guarded(R, 2 * RC_D))
    out = {k: v[1] for k, v in bufs.items()}
    _lib.check(_lib.lib().advmil_dx_chain_fwd(
        p(e), R, RC_D, p(d["W1pl"].hi), p(d["W1pl"].lo), p(d["fc1.0.bias"]), p(d["W2pl"].hi), p(d["W2pl"].lo), p(d["fc1.3.bias"]),
        p(d["Wabpl"].hi), p(d["Wabpl"].lo), p(d["bab"]), p(d["wc"]), p(d["bc"] if bc else None), p1, pg, p(d["seed"] if seeded else None),
        SIDS[0], SIDS[1], SIDS[2], p(rr), p(out.get("h1")), p(out["fc"]), p(out.get("ab")), p(out["s"]), ops._stream()), "dx_chain_fwd")
    torch.cuda.synchronize()
    guards_intact({k: v[0] for k, v in bufs.items()}, R)
    return dict(h1=out.get("h1"), fc=out["fc"], ab=out.get("ab"), s=out["s"].reshape(-1))


def fwd_bounds(ref, emu):
    bound, widened = {}, set()
    for k, tol in FWD_TOL.items():
        bound[k] = project_bound(tol, ref[k])
        if k in FWD_WIDEN:
            e4 = 4.0 * maxerr(emu[k], ref[k])
            if e4 > bound[k]:
                bound[k] = e4
                widened.add(k)
    return bound, widened


@pytest.mark.parametrize("c", FWD_CASES, ids=cid)
def test_forward_walks(c):
    ref, emu = oracle_fwd(c.R, c.mode, c.rmap, c.bc), emulate_fwd(c.R, c.mode, c.rmap, c.bc)
    got = launch_fwd(c.R, c.mode, c.rmap, True, c.bc)
    bound, widened = fwd_bounds(ref, emu)
    judge("fwd " + cid(c), {k: maxerr(got[k], ref[k]) for k in FWD_TOL}, bound, widened)
    masks, p1, _ = masks_of(c.R, c.mode, c.rmap)
    if masks[0] is not None:                          # a dropped entry of h1 is exactly 0, a kept positive one is not
        h1 = got["h1"].cpu().numpy()
        assert not h1[~masks[0]].any() and ((h1 > 0) == (ref["h1"] > 0)).mean() > 0.999
    for k in ("h1", "fc", "ab", "s"):
        assert bool(torch.isfinite(got[k]).all()), k
    if c.nograd:                                      # the no-grad walk: h1 = ab = NULL, fc and s keep their bits
        ng = launch_fwd(c.R, c.mode, c.rmap, False, c.bc)
        assert ng["h1"] is None and ng["ab"] is None
        assert torch.equal(ng["fc"].view(torch.int32), got["fc"].view(torch.int32)) and torch.equal(ng["s"].view(torch.int32), got["s"].view(torch.int32))
    if c.mode == "noseed":                            # seed == NULL: the rates mean nothing -- the same bits as p1 = pg = 0
        z = launch_fwd(c.R, "none", c.rmap, True, c.bc)
        for k in ("h1", "fc", "ab", "s"):
            assert torch.equal(z[k].view(torch.int32), got[k].view(torch.int32)), k


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def test_prep_planes_are_the_split_of_the_transposed_weights():
    d = dev_params()
    P32, _ = host_params()
    Wab = torch.cat([P32["pool.fc1.0.weight"], P32["pool.score.0.weight"]])
    for name, W in (("W1T", P32["fc1.0.weight"]), ("W2T", P32["fc1.3.weight"]), ("WabT", Wab)):
        hi, lo = boundary.split_bf16(W.t().contiguous())
        assert tuple(d[name].hi.shape) == tuple(hi.shape)
        assert torch.equal(_bits16(d[name].hi), _bits16(hi.bfloat16())), name + ".hi"
        assert torch.equal(_bits16(d[name].lo), _bits16(lo.bfloat16())), name + ".lo"
        assert float((hi.double() + lo.double() - W.t().double()).abs().max()) <= 2.0 ** -16 * float(W.abs().max())      # (the split says something)


# ------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------
def bwd_inputs(c):
    """The oracle's side of a backward case: A, ds (from the oracle's own forward and 3 * randn pooling scores) and the cotangents, fp32."""
    def make():
        R, nb = sum(c.lens), len(c.lens)
        rin = rows_in(R)
        fwd = oracle_fwd(R, c.mode, c.rmap)
        dp, dm = rin["dp"][:nb].contiguous(), (rin["dm"][:nb].contiguous() if c.dmean else None)
        A64, _, _ = RR.pool(rin["s_pool"].numpy(), fwd["fc"], c.lens)
        ds64 = RR.pool_bwd_ds(dp.numpy(), A64, fwd["fc"], c.lens)
        return dict(A=torch.from_numpy(A64).float(), ds=torch.from_numpy(ds64).float(), dp=dp, dm=dm, add=rin["dfc_add"] if c.add else None,
                    pre=rin["pre"] if c.prefill else None)
    return cached(("bwdin",) + tuple(c), make)


def launch_bwd(c, fw, nan_ws=True):
    """One call of advmil_dx_chain_bwd on the forward launch `fw` (its h1 and ab) -> dict of device tensors."""
    ops = _ops()
    from advmil_amd import _lib
    L = _lib.lib()
    d, p = dev_params(), ops._p
    R, nb = sum(c.lens), len(c.lens)
    p1, pg, seeded = MODES[c.mode]
    inp = bwd_inputs(c)
    dv = cached(("bwddev",) + tuple(c), lambda: {k: (None if v is None or k == "pre" else v.to(DEV)) for k, v in inp.items()})
    assert c.seg or nb == 1
    seg = cached(("seg", c.lens), lambda: ops.Segments(list(c.lens), DEV)) if c.seg else None
    rr = cached(("rmapdev", R), lambda: row_map(R).to(DEV)) if c.rmap else None
    bufs = {"dG": guarded(R, 2 * RC_D), "dfc": guarded(R, RC_D), "dpre": guarded(R, RC_H)}
    if c.de:
        bufs["de"] = guarded(R, RC_D)
    out = {k: v[1] for k, v in bufs.items()}
    acc = {}
    for k, n in (("dwc", RC_D), ("dbab", 2 * RC_D), ("dbc", 1), ("db2", RC_D), ("db1", RC_H)):
        acc[k] = inp["pre"][k].to(DEV) if c.prefill else torch.zeros(n, device=DEV)
    wsb = L.advmil_dx_chain_bwd_workspace_bytes(R, RC_D)
    assert wsb == tiles(R) * RC_PART * 4
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=DEV)
    if nan_ws:
        ws.view(torch.uint8).fill_(0xFF)
    w1t = d["W1T"] if c.de else None                  # de == NULL: W1T is not needed and is not given
    _lib.check(L.advmil_dx_chain_bwd(
        R, RC_D, p(dv["ds"]), p(dv["A"]), p(dv["dp"]), p(dv["dm"]), p(None if seg is None else seg.rowseg), p(None if seg is None else seg.ptr),
        p(dv["add"]), p(fw["h1"]), p(fw["ab"]), p(d["wc"]), p1, pg, p(d["seed"] if seeded else None), SIDS[1], SIDS[2], p(rr),
        p(d["WabT"].hi), p(d["WabT"].lo), p(d["W2T"].hi), p(d["W2T"].lo), p(None if w1t is None else w1t.hi), p(None if w1t is None else w1t.lo),
        p(out["dG"]), p(out["dfc"]), p(out["dpre"]), p(out.get("de")), p(acc["dwc"]), p(acc["dbab"]), p(acc["dbc"]), p(acc["db2"]), p(acc["db1"]),
        p(ws), wsb, ops._stream()), "dx_chain_bwd")
    torch.cuda.synchronize()
    guards_intact({k: v[0] for k, v in bufs.items()}, R)
    if nan_ws:                                        # the pad columns still hold what they held: nobody writes them
        pad = ws.view(tiles(R), RC_PART)[:, RC_PART_PAD[0]:RC_PART_PAD[1]]
        assert bool(torch.isnan(pad).all()) and bool(torch.isfinite(ws.view(tiles(R), RC_PART)[:, :RC_PART_PAD[0]]).all())
    return dict(out, **acc)


def emulate_bwd(c, fw, inp, masks, p1, pg):
    """dG and dpre in the documented arithmetic on the CPU (fp32 gate backward, bf16x3 products, fp32 epilogues)."""
    P32, _ = host_params()
    mm = boundary.emulated_matmul
    R, nb = sum(c.lens), len(c.lens)
    ma, mb = _scale32(masks[1], pg), _scale32(masks[2], pg)
    ab = fw["ab"].cpu()
    a, b = ab[:, :RC_D], ab[:, RC_D:]
    ds, wc = inp["ds"][:, None], P32["pool.fc2.weight"].reshape(-1)
    ad, bd = a * ma, b * mb
    dG = torch.cat([ds * wc * bd * ma * (1 - a * a), ds * wc * ad * mb * b * (1 - b)], 1)
    Wab = torch.cat([P32["pool.fc1.0.weight"], P32["pool.score.0.weight"]])
    seg = torch.repeat_interleave(torch.arange(nb), torch.tensor(c.lens))
    dfc = mm(dG, Wab.t().contiguous(), "bf16x3") + inp["A"][:, None] * inp["dp"][seg]
    if inp["dm"] is not None:
        dfc = dfc + inp["dm"][seg] / torch.tensor(c.lens, dtype=torch.float32)[seg][:, None]
    if inp["add"] is not None:
        dfc = dfc + inp["add"]
    inv1 = 1.0 if masks[0] is None else 1.0 / (1.0 - p1)
    dpre = mm(dfc, P32["fc1.3.weight"].t().contiguous(), "bf16x3") * (fw["h1"].cpu() > 0) * inv1
    return dict(dG=dG, dpre=dpre)


def body_bwd(c, nan_ws=True):
    """Forward launch, backward launch on its h1 / ab, every output against the oracle's backward of the same saved forward."""
    R = sum(c.lens)
    _, P64 = host_params()
    inp = bwd_inputs(c)
    masks, p1, pg = masks_of(R, c.mode, c.rmap)
    fw = launch_fwd(R, c.mode, c.rmap)
    got = launch_bwd(c, fw, nan_ws)
    e64 = rows_in(R)["e"].double().numpy()
    h1k, fck, abk = (fw[k].double().cpu().numpy() for k in ("h1", "fc", "ab"))
    G = RR.bwd(P64, e64, h1k, fck, abk[:, :RC_D], abk[:, RC_D:], inp["A"].double().numpy(), inp["dp"].double().numpy(),
               None if inp["dm"] is None else inp["dm"].double().numpy(), None if inp["add"] is None else inp["add"].double().numpy(),
               c.lens, *masks, p1=p1, pg=pg, ds=inp["ds"].double().numpy())
    want = {k: G[k] for k in BWD_OUT}
    for k in ("dwc", "dbab", "dbc", "db2", "db1"):   # the merge accumulates: prefill + oracle
        if c.prefill:
            want[k] = want[k] + inp["pre"][k].double().numpy()
    g64 = {k: got[k].double().cpu().numpy() for k in ("dG", "dfc", "dpre")}
    have = dict(got, dWab=g64["dG"].T @ fck, dW2=g64["dfc"].T @ h1k, dW1=g64["dpre"].T @ e64)
    if not c.de:
        assert "de" not in got
        want.pop("de")
    emu = emulate_bwd(c, fw, inp, masks, p1, pg)
    err, bound, widened = {}, {}, set()
    for k in want:
        err[k] = maxerr(have[k], want[k])
        bound[k] = project_bound(TOL["grad"], want[k], DBC_FLOOR if k == "dbc" else FLOOR)
        if k in BWD_WIDEN:
            e4 = 4.0 * maxerr(emu[k], want[k])
            if e4 > bound[k]:
                bound[k] = e4
                widened.add(k)
    judge("bwd " + cid(c), err, bound, widened)
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), k
    if masks[0] is not None:
        assert not got["dpre"].cpu().numpy()[~masks[0]].any()
    return got


@pytest.mark.parametrize("c", BWD_CASES, ids=cid)
def test_backward_walks(c):
    body_bwd(c)


# ------------------------------------------------------------------------------------------------------------------------------
# the wrapper: ops.dx_region_pool in the discriminator, train mode, end to end
# ------------------------------------------------------------------------------------------------------------------------------
def run_wrapper(c):
    from advmil_amd import ops
    from advmil_amd.optim import FlatAdam
    from tests.test_parity_gpu import build_disc, load_synth
    prev_mode, prev_chain = ops.get_gemm_mode(), ops.DX_CHAIN
    ops.set_gemm_mode("bf16x3")
    ops.DX_CHAIN = True
    calls, real = [], ops.dx_region_pool
    ops.dx_region_pool = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        d = build_disc("prj", "instance", "x")
        d.train(True)
        load_synth(d, "D-prj:")
        opt = FlatAdam(d, lr=1e-4)
        opt.zero_grad()
        if c.frozen:
            for p in d.parameters():
                p.requires_grad_(False)
        rng = ops.DeviceRng(DEV, seed=7)
        rng.record = True
        R, nb = sum(WRAP_LENS), len(WRAP_LENS)
        rmap = row_map(R) if c.rmap else None
        if c.rmap:                                    # as the bag-parallel handler does for the length of a step's forward
            rng.rows = {"region": rmap.to(DEV)}
        for m in d.modules():
            m.rng = rng
        g = torch.Generator().manual_seed(WRAP_E_SEED)
        e_host = torch.randn(R, RC_D, generator=g)
        w = {k: torch.randn(n, RC_D, generator=g) for k, n in (("pooled", nb), ("mean", nb), ("fc", R))}
        e = e_host.to(DEV).requires_grad_(c.e_grad)
        seg = ops.Segments(list(WRAP_LENS), DEV)
        out = d.net_pair_one.pool_features_rows(e, seg, want_mean=c.want_mean)
        pooled, fc = out[0], out[1]
        mean = out[2] if c.want_mean else None
        loss = (pooled.reshape(nb, RC_D) * w["pooled"].to(DEV)).sum() + (fc * w["fc"].to(DEV)).sum()
        if mean is not None:
            loss = loss + (mean.reshape(nb, RC_D) * w["mean"].to(DEV)).sum()
        loss.backward()
        torch.cuda.synchronize()
        rng.rows = None
        assert calls == [1], "the fused region network did not run"
        pre = "net_pair_one."
        grads = {k[len(pre):]: (None if p.grad is None else p.grad.detach().clone()) for k, p in d.named_parameters() if k[len(pre):] in RR.KEYS}
        params = {k[len(pre):]: v.detach().double().cpu().numpy() for k, v in d.state_dict().items() if k[len(pre):] in RR.KEYS}
        return dict(pooled=pooled.detach().reshape(nb, RC_D), fc=fc.detach(), mean=None if mean is None else mean.detach().reshape(nb, RC_D),
                    A=d.net_pair_one.pool.last_attention.clone(), de=e.grad, grads=grads, params=params, log=list(rng.log), e=e_host, w=w,
                    rmap=rmap, p1=d.net_pair_one.fc1[2].p, pg=d.net_pair_one.pool.drop_p)
    finally:
        ops.dx_region_pool = real
        ops.DX_CHAIN = prev_chain
        ops.set_gemm_mode(prev_mode)


@pytest.mark.parametrize("c", WRAP_CASES, ids=cid)
def test_wrapper_train_mode_end_to_end(c):
    r = run_wrapper(c)
    _, P64 = host_params()
    assert set(r["params"]) == set(RR.KEYS) and all(np.array_equal(r["params"][k], P64[k]) for k in RR.KEYS)
    log = {t: (sid, shape, p) for (t, sid, shape, p) in r["log"]}
    R = sum(WRAP_LENS)
    assert [t for (t, _, _, _) in r["log"]] == list(RR.SITES) and [log[t][1] for t in RR.SITES] == [(R, RC_H), (R, RC_D), (R, RC_D)]
    p1, pg = float(r["p1"]), float(r["pg"])
    assert p1 > 0 and pg > 0 and [log[t][2] for t in RR.SITES] == [p1, pg, pg]
    masks = RR.keep_masks(7, [log[t][0] for t in RR.SITES], R, p1, pg, None if r["rmap"] is None else r["rmap"].numpy())
    e64 = r["e"].double().numpy()
    Z1 = RR.preact(P64, e64)
    assert float(np.abs(Z1).min()) >= boundary.DEEP_DELTA, float(np.abs(Z1).min())          # no ReLU branch the two sides could take apart
    h1, fc, a, b, s = RR.fwd(P64, e64, *masks, p1=p1, pg=pg)
    A, pooled, mean = RR.pool(s, fc, WRAP_LENS)
    wm = r["w"]["mean"].double().numpy() if c.want_mean else None
    G = RR.bwd(P64, e64, h1, fc, a, b, A, r["w"]["pooled"].double().numpy(), wm, r["w"]["fc"].double().numpy(), WRAP_LENS, *masks, p1=p1, pg=pg)
    err = dict(fc=maxerr(r["fc"], fc), A=maxerr(r["A"], A), pooled=maxerr(r["pooled"], pooled))
    bound = dict(fc=project_bound(TOL["fc"], fc), A=project_bound(TOL["A"], A), pooled=project_bound(TOL["pooled"], pooled))
    if c.want_mean:
        err["mean"], bound["mean"] = maxerr(r["mean"], mean), project_bound(TOL["mean"], mean)
    else:
        assert r["mean"] is None
    if c.e_grad:
        err["de"], bound["de"] = maxerr(r["de"], G["de"]), project_bound(TOL["grad"], G["de"])
    else:
        assert r["de"] is None
    for k, g in RR.param_grads(G).items():
        got = r["grads"][k]
        if c.frozen:                                  # only de leaves: the arena slots keep their zeros
            assert got is None or not bool(got.any()), k
            continue
        err["g:" + k] = maxerr(got.reshape(g.shape), g)
        bound["g:" + k] = project_bound(TOL["grad"], g, DBC_FLOOR if k == "pool.fc2.bias" else FLOOR)
    judge("wrap " + cid(c), err, bound)


# ------------------------------------------------------------------------------------------------------------------------------
# the parametrisation reaches every walk of the tables above
# ------------------------------------------------------------------------------------------------------------------------------
def walks_reached():
    """Worked out on the host from the case lists alone (tests/test_region_walks_plan_cpu.py calls this too)."""
    got = set()
    for c in FWD_CASES:
        got |= {("fwd", "R", c.R), ("fwd", "drop", c.mode), ("fwd", "pair", c.mode, c.rmap), ("fwd", "rmap", c.rmap), ("fwd", "keep", True),
                ("fwd", "bc", c.bc), ("fwd", "tiles", tiles(c.R))}
        if c.nograd:
            got.add(("fwd", "keep", False))
        if c.mode == "both":
            got.add(("fwd", "both_on", c.R))
    for c in BWD_CASES:
        assert c.seg or len(c.lens) == 1, c
        R = sum(c.lens)
        got |= {("bwd", "lens", c.lens), ("bwd", "seg", c.seg), ("bwd", "dmean", c.dmean), ("bwd", "add", c.add), ("bwd", "de", c.de),
                ("bwd", "drop", c.mode), ("bwd", "pair", c.mode, c.rmap), ("bwd", "prefill", c.prefill), ("bwd", "tiles", tiles(R))}
        if c.dmean and not c.seg:
            got.add(("bwd", "dmean_divisor_R"))
        o, ends = 0, []
        for n in c.lens:
            o += n
            ends.append(o)
        per_tile = collections.Counter((x - 1) // RC_ROWS for x in ends)
        if max(per_tile.values()) >= 2:
            got.add(("bwd", "two_ends_in_a_tile"))
        if any(n == 1 for n in c.lens) and len(c.lens) > 1:
            got.add(("bwd", "one_row_bag_inside"))
        if any(x % RC_ROWS == 0 for x in ends[:-1]) or (ends[-1] % RC_ROWS == 0 and len(c.lens) > 1):
            got.add(("bwd", "end_on_a_tile_edge"))
        if any(ceil_div(x, RC_ROWS) - (x - n) // RC_ROWS >= 3 for x, n in zip(ends, c.lens)):
            got.add(("bwd", "bag_over_three_tiles"))
    got.add(("poison", POISON_CASE.lens, POISON_CASE.mode))
    for c in WRAP_CASES:
        got |= {("wrap", "want_mean", c.want_mean), ("wrap", "e_grad", c.e_grad), ("wrap", "frozen", c.frozen), ("wrap", "rmap", c.rmap)}
    return got


WALKS_WANTED = (
    {("fwd", "R", r) for r in (1, 63, 64, 65, 127, 193)} | {("fwd", "drop", m) for m in MODES} | {("fwd", "pair", m, r) for m in MODES for r in (False, True)}
    | {("fwd", "rmap", r) for r in (False, True)} | {("fwd", "keep", k) for k in (False, True)} | {("fwd", "bc", k) for k in (False, True)}
    | {("fwd", "both_on", 65), ("fwd", "both_on", 127)} | {("fwd", "tiles", n) for n in (1, 2, 4)}
    | {("bwd", "lens", l) for l in ((1,), (63,), (64,), (65,), (200,), (1, 300), (30, 1, 20, 77, 64))}
    | {("bwd", k, v) for k in ("seg", "dmean", "add", "de", "prefill") for v in (False, True)} | {("bwd", "dmean_divisor_R")}
    | {("bwd", "drop", m) for m in MODES} | {("bwd", "pair", m, r) for m in MODES for r in (False, True)}
    | {("bwd", "tiles", n) for n in (1, 2, 5)}
    | {("bwd", w) for w in ("two_ends_in_a_tile", "one_row_bag_inside", "end_on_a_tile_edge", "bag_over_three_tiles")}
    | {("poison", (30, 1, 20, 77, 64), "both")}
    | {("wrap", k, v) for k in ("want_mean", "e_grad", "frozen", "rmap") for v in (False, True)})


def test_every_walk_is_reached():
    """Every value of the forward, backward and wrapper tables, every (dropout, row map) pair each way, R = 65 and 127 with both draws
    on, 1 / 2 / 5 workspace tiles, two segment ends in a tile, a one-row bag inside a tile, an end on a tile edge, a bag over three
    tiles or more."""
    missing = WALKS_WANTED - walks_reached()
    assert not missing, sorted(missing, key=str)
    for k, (r, case, wide) in sorted(WORST.items()):
        print(f"worst of {k}: {r:.3f} of its bound{' (widened)' if wide else ''} ({case})")
    if WIDENED:
        print("widened bound in force:", sorted(WIDENED))
