"""GPU: every walk of the attention core (csrc/attn.hip, attn_bwd1.hip, attn_core.h) against the per-block float64 oracle of
tests/attn_ref.py. Each case asserts on the host which walk it takes (attn_ref.walk_facts, pinned to the source text by
tests/test_attn_walks_plan_cpu.py) before it launches; every result -- O, the stored log-sum-exp, dQ / dK / dV, D = rowsum(dO * O) --
goes through attn_ref.block_errors: per (bag, head) block against that block's own scale, under both backward forms.

Bounds: the project's own, per block -- O, lse, D 1e-5, gradients 5e-5. Where a case misses one, the bound in force is
max(project bound, 4 e_model), e_model being the float32 host model's error against float64 on that case's inputs (the factor 4 covers
the summation order and the 1-ulp v_exp_f32 the model does not reproduce); such cases are reported by name."""
import itertools
from collections import namedtuple

import numpy as np
import pytest
import torch

from advmil_amd import synth
from tests import attn_ref as AR
from tests import helpers as H

DEV = "cuda:0"
FORMS = ("two", "one")
_C = namedtuple("Case", "name lens hd nhead p seg max_len rowoff content lse_given degenerate seed")


def C(name, lens, hd=48, nhead=8, p=0.0, seg=None, max_len=None, rowoff=None, content=None, lse_given=False, degenerate=(), seed=77):
    return _C(name, tuple(lens), hd, nhead, p, (len(lens) > 1) if seg is None else seg, max_len, rowoff, content, lse_given,
              tuple(degenerate), seed)


def cid(c):
    return f"{c.name}-{'x'.join(map(str, c.lens))}-hd{c.hd}-nh{c.nhead}-p{c.p:g}" + ("" if c.seg else "-noseg") + (f"-cap{c.max_len}" if c.max_len else "")


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import ops as _ops
    from advmil_amd import _lib
    _lib.lib()
    return _ops


@pytest.fixture(params=FORMS)
def form(request, ops):
    prev = ops.ATTN_BWD
    ops.ATTN_BWD = request.param
    yield request.param
    ops.ATTN_BWD = prev


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs, reference (computed once per case, shared by the two backward forms, never modified), launch, check
# ---------------------------------------------------------------------------------------------------------------------------------
def rnd(tag, *shape, scale=1.0):
    n = int(np.prod(shape))
    return H.T(synth.normal(synth.stream_key(29, tag), n).reshape(shape) * np.float32(scale))


def _offsets(lens):
    return [0] + list(itertools.accumulate(lens))


def content_late_maximum(c, qkv, go):
    """Per bag: one key late in the key order carries 6 x a query's direction, another -4 x: the running maximum of that query (and of
    its neighbours in direction) jumps at a late tile, after several tiles of ordinary scores."""
    d, off = c.nhead * c.hd, _offsets(c.lens)
    qkv *= np.float32(0.3 / 0.7)
    for b, L in enumerate(c.lens):
        r0 = off[b]
        qkv[r0 + L - 3, d:2 * d] = 6.0 * qkv[r0 + 17 % L, :d]
        qkv[r0 + L // 4, d:2 * d] = -4.0 * qkv[r0 + L // 2, :d]


def _rank_one_scores(c, qkv, gamma, beta_of_bag):
    """q_i = gamma_i w, k_j = beta_j w with |w|^2 / sqrt(hd) = 1 per head: the scaled score of (i, j) is gamma_i beta_j."""
    d, off = c.nhead * c.hd, _offsets(c.lens)
    w = rnd(f"w{c.name}", d)
    w = w.reshape(c.nhead, c.hd)
    w = (w / w.norm(dim=1, keepdim=True) * c.hd ** 0.25).reshape(d)
    for b, L in enumerate(c.lens):
        r0 = off[b]
        qkv[r0:r0 + L, :d] = gamma(b, L)[:, None] * w[None, :]
        qkv[r0:r0 + L, d:2 * d] = beta_of_bag(b, L)[:, None] * w[None, :]


def content_pm300(c, qkv, go):
    """Scores near +-300: for a query with gamma = +300 the key with beta = 1 has probability exactly 1 and every other underflows
    (gap >= 150 > 104 = the fp32 exponent range in nats); for gamma = -300 the key with beta = -1."""
    def beta(b, L):
        t = torch.linspace(-0.4, 0.5, L)
        t[L // 3] = 1.0
        t[L - 2] = -1.0
        return t
    _rank_one_scores(c, qkv, lambda b, L: torch.where(torch.arange(L) % 2 == 0, 300.0, -300.0), beta)


def content_underflowing_rescale(c, qkv, go):
    """The whole first key tile at -200, zeros behind it: the factor exp(m_old - m_new) that rescales o[] and l underflows to 0."""
    def beta(b, L):
        t = torch.zeros(L)
        t[:64] = -1.0
        return t
    _rank_one_scores(c, qkv, lambda b, L: torch.full((L,), 200.0), beta)


def content_constant_v(c, qkv, go):
    """V constant along the keys of a bag: the output equals that constant whatever P is (to round-off): checks 1 / l_tot."""
    d, off = c.nhead * c.hd, _offsets(c.lens)
    for b, L in enumerate(c.lens):
        qkv[off[b]:off[b] + L, 2 * d:] = rnd(f"cv{b}", d)[None, :]


def content_zero_q(c, qkv, go):
    """q = 0: all scores equal, lse = log2 L."""
    qkv[:, :c.nhead * c.hd] = 0.0


_INPUTS, _REFS = {}, {}


def inputs(c):
    if c not in _INPUTS:
        Lt, d = sum(c.lens), c.nhead * c.hd
        qkv, go = rnd(f"q{cid(c)}", Lt, 3 * d, scale=0.7), rnd(f"g{cid(c)}", Lt, d)
        if c.content is not None:
            c.content(c, qkv, go)
        _INPUTS[c] = (qkv, go)
    return _INPUTS[c]


def keeps_and_masks(c, sid=1):
    if c.p == 0:
        return None, None
    masks = AR.host_masks(c.seed, sid, c.lens, c.p, c.nhead, rowoff=c.rowoff)
    return [m > 0 for m in masks], masks


def reference(c):
    if c not in _REFS:
        qkv, go = inputs(c)
        _REFS[c] = AR.oracle(qkv, go, c.lens, c.nhead, c.hd, keeps_and_masks(c)[1])
    return _REFS[c]


def e_model(c):
    """The float32 host model's per-block error against float64 on this case's own inputs."""
    qkv, go = inputs(c)
    keeps, _ = keeps_and_masks(c)
    lse_in = None
    if c.lse_given:
        lse_in = AR.model(qkv, go, c.lens, c.nhead, c.hd, backward=False)["lse"]
    m = AR.model(qkv, go, c.lens, c.nhead, c.hd, keeps, AR.inv_keep(c.p), lse_in=lse_in)
    if c.lse_given:
        del m["lse"]
    return {k: v[0] for k, v in AR.block_errors(m, reference(c), c.lens, c.nhead, c.hd, c.degenerate).items()}


def facts(c):
    return AR.walk_facts(c.lens, c.hd, c.nhead, c.max_len)


def launch(ops, c, qkv=None, go=None, via_mha=False):
    """One forward + backward under ops.ATTN_BWD as it stands -> dict O, lse, dQ, dK, dV, D (device tensors)."""
    if qkv is None:
        qkv, go = inputs(c)
    d = c.nhead * c.hd
    Lt = sum(c.lens)
    seg = ops.Segments(c.lens, DEV) if c.seg else None
    if c.max_len is not None:
        seg.max_len = c.max_len                              # what a step graph does: the plan's cap, not this slab's longest bag
    rowoff = None if c.rowoff is None else torch.tensor(c.rowoff, dtype=torch.int64, device=DEV)
    rng = ops.DeviceRng(DEV, seed=c.seed)
    a = qkv.to(DEV).requires_grad_(True)
    g = go.to(DEV)
    ops.MhaFn.keep_dsum = True
    try:
        if c.lse_given:
            planes = ops.split_planes(a.detach())
            with torch.no_grad():
                ops.MhaFn.apply(a.detach(), c.nhead, 0.0, None, 0, seg, None, planes, None)    # the eval-mode pass leaves its log-sum-exp
            given = ops.MhaFn.last_lse
            sid = rng.site("mha_attn", (Lt, c.nhead), c.p)
            o = ops.MhaFn.apply(a, c.nhead, float(c.p), rng.seed, sid, seg, rowoff, planes, given)
            assert ops.MhaFn.last_lse is given
        elif via_mha:
            o = ops.mha(a, c.nhead, c.p, rng, seg=seg, rowoff=rowoff)
            (o * g).sum().backward()
            return {"O": o.detach(), "dQ": a.grad[:, :d], "dK": a.grad[:, d:2 * d], "dV": a.grad[:, 2 * d:], "D": ops.MhaFn.last_dsum}
        else:
            sid = rng.site("mha_attn", (Lt, c.nhead), c.p) if c.p > 0 else 0
            o = ops.MhaFn.apply(a, c.nhead, float(c.p), rng.seed if c.p > 0 else None, sid, seg, rowoff, None, None)
        lse = ops.MhaFn.last_lse
        (o * g).sum().backward()
        got = {"O": o.detach(), "lse": lse, "dQ": a.grad[:, :d], "dK": a.grad[:, d:2 * d], "dV": a.grad[:, 2 * d:], "D": ops.MhaFn.last_dsum}
        if c.lse_given:
            del got["lse"]                                   # (the eval pass's own: judged by the cases that store one)
        return got
    finally:
        ops.MhaFn.keep_dsum = False
        ops.MhaFn.last_lse = None


WIDENED = []          # (case id, form, part, error, bound in force): the cases that needed 4 e_model


def check(c, frm, got):
    ref = reference(c)
    for t in got.values():
        assert torch.isfinite(t).all()
    errs = AR.block_errors(got, ref, c.lens, c.nhead, c.hd, c.degenerate)
    assert set(errs) == set(got)
    em = None
    for part, (err, where) in errs.items():
        bound = AR.PROJECT_BOUND[part]
        if not err <= bound:
            em = em or e_model(c)
            bound = max(bound, 4.0 * em[part])
            WIDENED.append((cid(c), frm, part, err, bound))
        print(f"ATTNWALK {cid(c)} {frm} {part} err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f} at {where}"
              + (" WIDENED" if bound > AR.PROJECT_BOUND[part] else ""))
        assert err <= bound, (cid(c), frm, part, err, bound, where)
    return errs


def run(ops, c, frm):
    got = launch(ops, c)
    return got, check(c, frm, got)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
RING_SLAB = (1, 31, 32, 33, 63, 64, 65, 128, 129, 193)
RING = [C("ring", RING_SLAB, hd, p=p) for hd in AR.HEAD_DIMS for p in (0.0, 0.25)] + \
       [C("ring1", (L,), hd, p=p, seg=False) for hd in AR.HEAD_DIMS for p in (0.0, 0.25) for L in (1, 64, 65, 193)]
QTILES = [C("qtile1", (L,), hd, p=0.0, seg=False) for hd in AR.HEAD_DIMS for L in (255, 256, 257)] + \
         [C("qtile", (255, 256, 257), hd, p=0.25) for hd in AR.HEAD_DIMS]
SINGLE_PASS = [C("trips", (32, 33, 65), 48, p=0.25), C("trips", (32, 33, 65), 16, p=0.25)] + \
              [C("nkb", (L,), 48, p=0.25 if L == 1025 else 0.0, seg=False) for L in (512, 768, 1024, 1025)] + \
              [C("nkb", (L,), 16, nhead=2, p=0.25 if L == 1025 else 0.0, seg=(L == 768)) for L in (512, 768, 1024, 1025)]
# (the ABI takes a cap up to L_total -- tests/test_abi_negative_cpu.py pins the refusal beyond it --, so the 600-row cap runs on a slab
# of 622 rows and is asserted to be refused on the 322 rows of [65, 257])
RAISED = [C("cap", (65, 257, 300), 48, p=0.25, max_len=600), C("cap", (65, 257), 48, p=0.25, max_len=322)]
PREP = [C("prep", lens, hd, p=0.0) for hd in AR.HEAD_DIMS for lens in ((1,), (1, 2), (5, 32))]
NHEAD = [C("nhead", (33, 1, 70), hd, nhead=nh, p=0.25) for hd in (16, 48) for nh in (1, 3, 16)]
RATES = [C("rate", (1, 5, 67, 130), 48, p=p) for p in (1 / 256, 0.1, 0.5, 255 / 256)]
GROUPS = [C("groups", (65, 66, 67), hd, p=0.25, rowoff=(1000, 5, 70001)) for hd in (48, 32)]
LSE_GIVEN = [C("lsegiven", (1, 70, 257, 33), hd, p=0.25, lse_given=True) for hd in AR.HEAD_DIMS]
EQUAL_SCORES = [C("zeroq", (64, 256, 100, 2), hd, content=content_zero_q) for hd in (48, 16)]
CONTENT = [C("latemax", (130, 300), 48, content=content_late_maximum),
           C("latemax", (130, 300), 64, p=0.25, content=content_late_maximum),
           C("pm300", (70, 130), 48, content=content_pm300, degenerate=(0, 1)),
           C("underflow", (70, 129), 48, content=content_underflowing_rescale),
           C("underflow", (70, 129), 32, p=0.25, content=content_underflowing_rescale),
           C("constv", (5, 67, 130), 48, content=content_constant_v, degenerate=(0, 1, 2)),
           C("constv", (5, 67, 130), 16, p=0.25, content=content_constant_v)]
ISOLATION_PERMS = [(63, 65, 257, 1), (1, 257, 65, 63), (65, 1, 63, 257)]
TABLE = RING + QTILES + SINGLE_PASS + RAISED + PREP + NHEAD + RATES + GROUPS + LSE_GIVEN + EQUAL_SCORES + CONTENT
assert len(set(TABLE)) == len(TABLE)

WALKS_WANTED = set()
for _hd in AR.HEAD_DIMS:
    WALKS_WANTED |= {f"hd{_hd}:T{t}" for t in (1, 2, 3, 4)} | {f"hd{_hd}:fill{f}" for f in (1, 31, 32, 33, 63, 64)}
    WALKS_WANTED |= {f"hd{_hd}:q2:one", f"hd{_hd}:q1:255", f"hd{_hd}:q1:full", f"hd{_hd}:keyblock2:one", f"hd{_hd}:prep_partial", f"hd{_hd}:Lodd"}
for _hd in (16, 48):
    WALKS_WANTED |= {f"hd{_hd}:nkb{n}" for n in (1, 2, 3, 4, 5)} | {f"hd{_hd}:parity0", f"hd{_hd}:parity1"}
    WALKS_WANTED |= {f"hd{_hd}:nhead{n}" for n in (1, 3, 16)}
WALKS_WANTED |= {"trips1", "trips2", "trips3", "reduce_idle", "main_idle", "keys%4=1", "keys%4=2", "keys%4=3", "thr1", "thr25", "thr64",
                 "thr128", "thr255"}


def walks_reached():
    """Host side: the walks the parametrisation above reaches (every case runs under both backward forms)."""
    got = set()
    for c in TABLE + [C("iso", lens, 48, p=0.25) for lens in ISOLATION_PERMS]:
        got |= AR.walk_tags(facts(c), c.hd, c.nhead, c.p)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", RING, ids=cid)
def test_key_tile_ring(ops, form, c):
    """T = 1 (the vmcnt<0> start, no second issue), 2, 3 (first slot reuse of the forward's two slots), 4 (first reuse of the
    backward's three); a last tile of 1 / 31 / 32 / 33 / 63 / 64 keys; a slab and single bags (ptr == NULL)."""
    w = facts(c)
    if c.seg:
        assert [b.key_tiles for b in w.bags] == [1, 1, 1, 1, 1, 1, 2, 2, 3, 4]
        assert [b.last_fill for b in w.bags] == [1, 31, 32, 33, 63, 64, 1, 64, 1, 1]
        assert [b.last_half for b in w.bags][:6] == ["first", "first", "first", "second", "second", "second"]
    else:
        assert (w.bags[0].key_tiles, w.bags[0].last_fill) == {1: (1, 1), 64: (1, 64), 65: (2, 1), 193: (4, 1)}[c.lens[0]]
    assert (w.KS, w.DT, w.pad_units) == {16: (1, 1, 2), 32: (2, 1, 0), 48: (3, 2, 2), 64: (4, 2, 0)}[c.hd]
    run(ops, c, form)


@pytest.mark.parametrize("c", QTILES, ids=cid)
def test_query_tiles(ops, form, c):
    """255 / 256 / 257: a full first query tile, one query in the second (waves 1 .. 7 without a valid row), one key in the second
    key block of the keys-stationary kernels."""
    w = facts(c)
    for b in w.bags:
        assert (b.q_tiles, b.last_q_valid, b.idle_waves, b.nkb) == {255: (1, 255, 0, 1), 256: (1, 256, 0, 1), 257: (2, 1, 7, 2)}[b.L]
    run(ops, c, form)


@pytest.mark.parametrize("c", SINGLE_PASS, ids=cid)
def test_single_pass_trips_and_key_blocks(ops, form, c):
    """1, 2, 3 trips of 32 queries (parity; the flush of the last parked dQ tile); nkb = 1, 2, 3 (remainder only), 4 (one unrolled
    group), 5 (group + remainder) in the reduce."""
    w = facts(c)
    if c.name == "trips":
        assert [(b.trips, b.last_trip_parity) for b in w.bags] == [(1, 0), (2, 1), (3, 0)]
    else:
        b, = w.bags
        assert (b.nkb, b.nkb_groups, b.nkb_rem) == {512: (2, 0, 2), 768: (3, 0, 3), 1024: (4, 1, 0), 1025: (5, 1, 1)}[b.L]
        assert b.trips == AR.ceil_div(b.L, 32) and b.last_trip_parity == (b.trips - 1) % 2
    run(ops, c, form)


def body_raised_max_len(ops, c, frm):
    """A cap above the longest bag: workgroups that return in every main grid and in the reduce grid. Equal by the bit to the
    unraised launch, and inside the float64 bounds."""
    w = facts(c)
    assert c.max_len > max(c.lens) and all(b.main_wgs == AR.ceil_div(c.max_len, 256) for b in w.bags)
    assert [b.main_idle for b in w.bags] == {600: [2, 1, 1], 322: [1, 0]}[c.max_len]
    assert all(b.reduce_idle > 0 for b in w.bags) and w.bags[0].reduce_wgs == AR.ceil_div(c.max_len, 32)
    got = launch(ops, c)
    plain = launch(ops, c._replace(max_len=None), *inputs(c))
    for k in got:
        assert torch.equal(got[k], plain[k]), k
    check(c, frm, got)
    return got


@pytest.mark.parametrize("c", RAISED, ids=cid)
def test_raised_max_len(ops, form, c):
    body_raised_max_len(ops, c, form)


def test_a_cap_beyond_the_slab_is_refused_before_any_launch(ops, form):
    """max_len <= L_total is the ABI's rule (attn_args): 600 over the 322 rows of [65, 257] returns ADVMIL_EINVAL in the forward, and in
    either backward when only its cap is raised."""
    from advmil_amd._lib import AdvmilHipError
    c = RAISED[1]
    with pytest.raises(AdvmilHipError):
        launch(ops, c._replace(max_len=600))
    qkv, go = inputs(c)
    seg = ops.Segments(c.lens, DEV)
    a = qkv.to(DEV).requires_grad_(True)
    o = ops.MhaFn.apply(a, c.nhead, 0.0, None, 0, seg, None, None, None)
    seg.max_len = 600
    with pytest.raises(AdvmilHipError):
        (o * go.to(DEV)).sum().backward()
    ops.MhaFn.last_lse = None


@pytest.mark.parametrize("c", PREP, ids=cid)
def test_prep_partial_last_block_and_odd_row_counts(ops, form, c):
    w = facts(c)
    assert w.L_total in (1, 3, 37) and w.prep_partial and w.prep_blocks == AR.ceil_div(w.L_total * 8, {16: 64, 32: 32, 48: 16, 64: 16}[c.hd])
    got, errs = run(ops, c, form)
    assert "D" in errs


@pytest.mark.parametrize("c", NHEAD, ids=cid)
def test_head_counts_other_than_eight(ops, form, c):
    """head = blockIdx % nhead and the row key row * nhead + head for nhead 1, 3, 16; the masks are replayed with that nhead."""
    assert facts(c).bags[1].L == 1
    run(ops, c, form)


def _seed_with_both(c, bag):
    """A seed (host search) under which the one-row bag `bag` has its single key kept in some heads and dropped in others."""
    off = _offsets(c.lens)
    for seed in range(1, 200):
        k = [bool(synth.attn_dropout_keep(seed, 1, np.array([off[bag]]), c.nhead, h, 1, c.p)[0, 0]) for h in range(c.nhead)]
        if any(k) and not all(k):
            return seed
    raise AssertionError("no seed found")


@pytest.mark.parametrize("c", RATES, ids=cid)
def test_dropout_rates(ops, form, c):
    """1/256, 0.1 (runs at 25/256: the warning is expected), 0.5, 255/256. A row whose keys are all dropped gives an output row of exact
    zeros; at 0.5 the seed is picked so that the one-row bag's key is kept in some heads and dropped in others."""
    assert AR.drop_thr(c.p) == {1 / 256: 1, 0.1: 25, 0.5: 128, 255 / 256: 255}[c.p]
    if c.p == 0.5:
        c = c._replace(seed=_seed_with_both(c, 0))
    if c.p == 0.1:
        ops._MHA_P_WARNED.discard(c.p)
        with pytest.warns(UserWarning, match="runs at 25/256"):
            got = launch(ops, c, via_mha=True)
        check(c, form, got)
        got = launch(ops, c)
    else:
        got = launch(ops, c)
    check(c, form, got)
    keeps, _ = keeps_and_masks(c)
    o, r0, nzero = got["O"].cpu(), 0, 0
    for b, L in enumerate(c.lens):
        dead = ~keeps[b].any(dim=-1)                                   # [nhead, L]
        for h in range(c.nhead):
            rows = torch.nonzero(dead[h]).flatten() + r0
            nzero += len(rows)
            assert (o[rows, h * c.hd:(h + 1) * c.hd] == 0).all()
        r0 += L
    if c.p >= 0.5:
        assert nzero > 0
    if c.p == 0.5:
        k0 = keeps[0][:, 0, 0]
        assert k0.any() and not k0.all()


@pytest.mark.parametrize("c", GROUPS, ids=cid)
def test_dropout_key_groups_and_row_offsets(ops, form, c):
    """Key counts = 1, 2, 3 mod 4 across a tile edge (the last hash of a row covers 1, 2, 3 keys); a `rowoff` per bag of a slab."""
    assert [b.L % 4 for b in facts(c).bags] == [1, 2, 3] and all(b.key_tiles == 2 for b in facts(c).bags)
    run(ops, c, form)
    # ... and the offsets matter: without them the masks are others
    other = launch(ops, c._replace(rowoff=None), *inputs(c))
    assert not torch.equal(other["O"], launch(ops, c)["O"])


@pytest.mark.parametrize("c", LSE_GIVEN, ids=cid)
def test_forward_with_the_log_sum_exp_given_vs_float64(ops, form, c):
    """advmil_mha_fwd_lse given the eval pass's statistics: O and every gradient against float64, not against the plain forward."""
    assert facts(c).bags[0].L == 1
    got, errs = run(ops, c, form)
    assert "lse" not in errs and {"O", "dQ", "dK", "dV", "D"} <= set(errs)


@pytest.mark.parametrize("c", EQUAL_SCORES, ids=cid)
def test_all_equal_scores_store_log2_of_the_length(ops, form, c):
    got, _ = run(ops, c, form)
    lse, off = got["lse"].cpu().double(), _offsets(c.lens)
    for b, L in enumerate(c.lens):
        want = float(np.log2(L))
        assert float((lse[off[b]:off[b] + L] - want).abs().max()) <= 1e-5 * max(want, 1.0)
        if L & (L - 1) == 0:           # a power of two: log2 L is representable and the row sum of L ones is exact
            assert float((lse[off[b]:off[b] + L] - want).abs().max()) <= 2.0 ** -21 * max(want, 1.0)


@pytest.mark.parametrize("c", CONTENT, ids=cid)
def test_score_content(ops, form, c):
    qkv, go = inputs(c)
    ref = reference(c)
    d = c.nhead * c.hd
    if c.name == "latemax":
        for b in facts(c).bags:
            assert b.key_tiles >= 3
    if c.name == "pm300":
        s = ref["lse"].abs() * np.log(2.0)
        assert float(s.min()) > 250 and float(s.max()) < 350
    got, _ = run(ops, c, form)
    if c.name == "pm300":                    # one probability exactly 1: the output row is that key's v row as the planes hold it
        off = _offsets(c.lens)
        for b, L in enumerate(c.lens):
            vv = qkv[off[b]:off[b] + L, 2 * d:]
            o = got["O"][off[b]:off[b] + L].cpu()
            for rows, key in ((o[0::2], L // 3), (o[1::2], L - 2)):
                assert float((rows - vv[key]).abs().max()) <= 1e-5 * float(vv[key].abs().max())
    if c.name == "constv" and c.p == 0:
        off = _offsets(c.lens)
        for b, L in enumerate(c.lens):
            o = got["O"][off[b]:off[b] + L].cpu().double()
            want = qkv[off[b], 2 * d:].double()
            assert float((o - want).abs().max()) <= 1e-5 * float(want.abs().max())


def _clean_bag_parts(got, lo, hi):
    return {k: v[lo:hi].clone() for k, v in got.items()}


@pytest.mark.parametrize("lens", ISOLATION_PERMS, ids=lambda l: "x".join(map(str, l)))
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_bag_isolation(ops, form, lens, p):
    """Tile-edge slabs with every OTHER bag's q, k, v and dO rows set to NaN and then to 3e38: the clean bag's O, lse, gradients and D
    are equal by the bit to its values in the all-clean slab, for each bag in turn (rows past a bag's end are re-read from its own last
    row: the next bag's contents never reach a register that matters). Without dropout the slab equals per-bag launches too."""
    c = C("iso", lens, 48, p=p)
    qkv, go = inputs(c)
    clean = launch(ops, c)
    check(c, form, clean)
    off = _offsets(lens)
    for b in range(len(lens)):
        lo, hi = off[b], off[b + 1]
        for bad in (float("nan"), 3e38):
            q2, g2 = torch.full_like(qkv, bad), torch.full_like(go, bad)
            q2[lo:hi], g2[lo:hi] = qkv[lo:hi], go[lo:hi]
            got = launch(ops, c, q2, g2)
            for k in got:
                assert torch.equal(got[k][lo:hi], clean[k][lo:hi]), (b, bad, k)
        if p == 0:
            alone = launch(ops, C("iso1", (lens[b],), 48, seg=False), qkv[lo:hi].clone(), go[lo:hi].clone())
            for k in alone:
                assert torch.equal(alone[k], clean[k][lo:hi]), (b, k)


def test_the_parametrisation_reaches_every_walk():
    assert not WALKS_WANTED - walks_reached()
