"""GPU: advmil_optim_step (csrc/optim.hip::optim_kernel) and advmil_amd.optim.FlatOptim against the float64 restatement
tests/optim_ref.py (pinned to the reference's classes by tests/golden/optim_v1.npz), under allocation poisoning (tests/poison.py).

Tolerance (derived, tests/optim_ref.py::bound): max|p - p64| <= 2e-5 max|p64 - p0| + 2 steps 2^-24 max|p64| -- the suite's parity
tolerance on the displacement plus two fp32 roundings of the stored parameter per step; state arenas at 2e-5 of their own maximum."""
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests import poison as P
from tests.poison import poison  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 6                                        # lookahead_k
STEPS = 2 * K + 1                            # both RAdam branches (rectified from step 6), the creating sync at 6 and the blending one at 12
LR, WD = 1e-2, 5e-4
BIG = 2048 * 256 * 4 + 5                     # one element group more than a full grid covers in one pass: the grid-stride loop runs (+ tail)
# size -> (wd given, l1_coef, grad_scale, tick)
OPTIONS = {3: (False, 0.0, 0.5, True), 1029: (True, 1e-5, 2.0, False), BIG: (True, 1e-5, 0.5, True)}


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import _lib
    from advmil_amd import ops as _ops
    _lib.lib()
    return _ops


_INPUTS = {}


def inputs(n):
    """-> (p0, wd, base gradient) float64 with float32-exact values; step t's gradient is the base rolled by 7 t, times 1 + t / 10."""
    if n not in _INPUTS:
        rs = np.random.RandomState(n % 100003)
        f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
        p0 = f32(rs.standard_normal(n) * 0.1)
        p0[::11] = 0.0                                                  # sign(0) = 0 in the L1 fold
        wd = np.where(np.arange(n) % 3 == 0, 0.0, WD)
        _INPUTS[n] = (p0, f32(wd), f32(rs.standard_normal(n) * 1e-2 + 3e-3))
    return _INPUTS[n]


def grad_at(g, t):
    return (np.roll(g, 7 * t) * np.float32(1.0 + t / 10.0).astype(np.float64)).astype(np.float32).astype(np.float64)


_REFS = {}


def reference(kind, la, n):
    """The restatement's run, computed once per case."""
    key = (kind, la, n)
    if key not in _REFS:
        has_wd, l1, gscale, _ = OPTIONS[n]
        p0, wd, g = inputs(n)
        r = R.Ref(kind, p0, wd=wd if has_wd else 0.0, lr=LR, l1_coef=l1, lookahead=la, k=K)
        for t in range(STEPS):
            if t == K + 1:
                r.lr *= 0.5
            r.do_step(grad_at(g, t), grad_scale=gscale)
        _REFS[key] = r
    return _REFS[key]


def dev32(a):
    t = torch.empty(a.shape[0], dtype=torch.float32, device=DEV)       # (poisoned when a poisoning context is open)
    t.copy_(torch.from_numpy(a.astype(np.float32)))
    return t


def kernel_run(ops, kind, la, n):
    has_wd, l1, gscale, tick = OPTIONS[n]
    p0, wd, g = inputs(n)
    p, wdt = dev32(p0), dev32(wd) if has_wd else None
    s1, s2 = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    slow = torch.empty(n, dtype=torch.float32, device=DEV) if la else None        # never read before the sync that creates it
    la_state = torch.tensor([K, 0], dtype=torch.int32, device=DEV) if la else None
    m_sched = torch.ones(2, dtype=torch.float64, device=DEV) if kind == "nadam" else None
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    planes = ops.Planes.alloc((n,), DEV)
    nb = ops.adam_blocks(n)
    abs_sums, lr = [], LR
    for t in range(STEPS):
        if t == K + 1:
            lr *= 0.5
        grad = dev32(grad_at(g, t))
        clear = t % 2 == 1
        part = torch.empty(nb, dtype=torch.float32, device=DEV)
        before = float(p.double().abs().sum())
        ops.optim_step(kind, p, grad, s1, s2, wdt, step, lr, 0.9, 0.999, 1e-6 if kind == "adadelta" else 1e-8, gscale, l1, planes=planes,
                       tick=tick, abs_partial=part, clear_grad=clear, schedule_decay=4e-3, m_sched=m_sched, slow=slow, la_state=la_state,
                       la_alpha=0.5, la_k=K)
        if not tick:
            ops.step_seed_tick(step, None)
        abs_sums.append(part.double().sum())
        # the shares of sum |p| BEFORE the update: fp32 sums of 4 values per lane, then 6 + 2 tree levels (the shares are added in
        # float64 here): at most 12 roundings of 2^-24 each, relative to a sum of non-negative terms ((1 + u)^12 - 1 < 13 u)
        assert abs(float(abs_sums[-1]) - before) <= 13 * 2.0 ** -24 * before, (t, float(abs_sums[-1]), before)
        if clear:
            assert int(torch.count_nonzero(grad)) == 0
        else:
            assert torch.equal(grad.cpu(), torch.from_numpy(grad_at(g, t).astype(np.float32)))
        want = ops.split_planes(p)                                     # the planes the next forward reads: of the post-sync weights, bit for bit
        assert torch.equal(planes.hi.view(torch.int16), want.hi.view(torch.int16)) and torch.equal(planes.lo.view(torch.int16), want.lo.view(torch.int16))
    out = {"p": p, "s1": s1, "s2": s2, "hi": planes.hi, "lo": planes.lo, "abs": torch.stack(abs_sums), "step": int(step.item())}
    if la:
        out["slow"] = slow
    if m_sched is not None:
        out["m_schedule"] = m_sched[STEPS & 1].clone()
    return out


@pytest.mark.parametrize("n", list(OPTIONS))
@pytest.mark.parametrize("la", [False, True], ids=["plain", "lookahead"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_kernel_against_restatement(ops, kind, la, n):
    trees = P.three_runs(lambda: kernel_run(ops, kind, la, n))
    P.assert_same_bits(trees)
    for t in trees:
        P.assert_finite(t)
    got = trees[2]                                                     # the 0xFF run
    ref = reference(kind, la, n)
    p0 = inputs(n)[0]
    assert got["step"] == STEPS == ref.step
    err, bnd = R.bound(got["p"].cpu().numpy(), ref.p, p0, STEPS)
    print(f"{kind} la={la} n={n}: error {err:.3e} bound {bnd:.3e}")
    assert err <= bnd, (err, bnd)
    for k, a in (("s1", ref.s1), ("s2", ref.s2)) + ((("slow", ref.slow),) if la else ()):
        d = float(np.abs(got[k].cpu().numpy().astype(np.float64) - a).max())
        assert d <= 2e-5 * float(np.abs(a).max()), (k, d, float(np.abs(a).max()))
    if kind == "nadam":
        assert abs(float(got["m_schedule"]) - ref.m_schedule) <= 1e-13 * ref.m_schedule
    if kind == "radam":
        assert ref.rectified[0] is False and ref.rectified[-1] is True
    if la:
        assert ref.syncs == [(K, "create"), (2 * K, "blend")]


# ------------------------------------------------------------------------------------------------------------------------------
# the optimizer classes
# ------------------------------------------------------------------------------------------------------------------------------
class Net(torch.nn.Module):
    """Tensors whose sizes are no multiples of 8 (the arena pads each to one)."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(13, 7)
        self.n = torch.nn.LayerNorm(7)
        self.b = torch.nn.Linear(7, 5)
        self.c = torch.nn.Linear(5, 1, bias=False)


def NS(opt, wd=WD, lr=LR):
    return SimpleNamespace(opt=opt, weight_decay=wd, lr=lr, opt_eps=None, opt_betas=None, momentum=None)


def make(name, seed=3):
    from advmil_amd.optim import create_optimizer
    torch.manual_seed(seed)
    net = Net().to(DEV)
    return net, create_optimizer(NS(name), net)


def feed(opt, t):
    """A seeded gradient into every parameter's arena slot (the padding between them stays untouched)."""
    g = torch.Generator().manual_seed(100 + t)
    for p, o, k in opt._views:
        p.grad.copy_((torch.randn(p.shape, generator=g) * 1e-2 + 2e-3).to(DEV))


def arenas(opt):
    out = {"p": opt.flat_param, "s1": opt.flat_m, "s2": opt.flat_v, "hi": opt.planes.hi, "lo": opt.planes.lo}
    if opt.flat_slow is not None:
        out["slow"] = opt.flat_slow
    return {k: v.clone() for k, v in out.items()}


CLASS_CASES = ["adamw", "nadam", "radam", "adadelta", "lookahead_adam", "lookahead_nadam", "lookahead_radam", "lookahead_adadelta", "lookahead_adamw"]


@pytest.mark.parametrize("name", CLASS_CASES)
def test_optimizer_class_matches_restatement_and_round_trips(ops, name, poison):
    from advmil_amd.optim import FlatOptim, parse_opt_name
    kind, la = parse_opt_name(name)
    net, opt = make(name)
    assert isinstance(opt, FlatOptim) and opt.kind == kind and opt.lookahead == la
    assert len(opt.param_groups) == 2 and opt.param_groups[0]["weight_decay"] == 0.0 and opt.param_groups[1]["weight_decay"] == WD
    total = opt.flat_param.numel()
    assert any(k % 8 for _, _, k in opt._views) and total % 8 == 0
    pad = torch.ones(total, dtype=torch.bool)
    for _, o, k in opt._views:
        pad[o:o + k] = False
    assert int(pad.sum()) > 0
    opt.l1_coef = 1e-5
    p0 = opt.flat_param.cpu().numpy().astype(np.float64)
    wd = opt.flat_wd.cpu().numpy().astype(np.float64)
    assert set(np.unique(wd[~pad.numpy()])) == {0.0, float(np.float32(WD))}
    ref = R.Ref(kind, p0, wd=wd, lr=LR, l1_coef=1e-5, lookahead=la, k=K)
    n1 = K + 1
    for t in range(n1):
        opt.zero_grad(); feed(opt, t); opt.step()
        ref.do_step(opt.flat_grad.cpu().numpy())
    # ---- state_dict -> a fresh optimizer -> load_state_dict, through serialisation
    buf = io.BytesIO()
    torch.save({"model": net.state_dict(), "optimizer": opt.state_dict()}, buf)
    buf.seek(0)
    ck = torch.load(buf, map_location=DEV)
    sd = ck["optimizer"]
    s1n, s2n = R.STATE_NAMES[kind]
    want_keys = {"step", s1n, s2n} | ({"m_schedule"} if kind == "nadam" else set())
    assert set(sd["state"][0]) == want_keys, set(sd["state"][0])
    assert (type(sd["state"][0]["step"]) is int) == (kind in ("nadam", "radam")) and float(sd["state"][0]["step"]) == n1
    if la:
        assert set(sd) == {"state", "slow_state", "param_groups"} and sorted(sd["slow_state"]) == list(range(len(opt._views)))
        assert all(g["lookahead_alpha"] == 0.5 and g["lookahead_k"] == K and g["lookahead_step"] == n1 for g in sd["param_groups"])
    else:
        assert set(sd) == {"state", "param_groups"}
    net2, opt2 = make(name, seed=4)
    net2.load_state_dict(ck["model"]); opt2.load_state_dict(sd)
    opt2.l1_coef = 1e-5
    for t in range(n1, STEPS):
        for o_ in (opt, opt2):
            o_.zero_grad(); feed(o_, t); o_.step()
        ref.do_step(opt.flat_grad.cpu().numpy())
    a, b = arenas(opt), arenas(opt2)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k          # the resumed run continues bit for bit
    assert int(opt.step_t) == int(opt2.step_t) == STEPS
    # ---- against the restatement, the decay filter and the L1 fold included; the padding never moved
    err, bnd = R.bound(a["p"].cpu().numpy(), ref.p, p0, STEPS)
    assert err <= bnd, (err, bnd)
    for k, r_ in (("s1", ref.s1), ("s2", ref.s2)) + ((("slow", ref.slow),) if la else ()):
        assert float(np.abs(a[k].cpu().numpy().astype(np.float64) - r_).max()) <= 2e-5 * float(np.abs(r_).max()), k
    for k in a:
        assert int(torch.count_nonzero(a[k].cpu()[pad])) == 0, k
    if kind == "nadam":
        assert abs(opt.state_dict()["state"][0]["m_schedule"] - ref.m_schedule) <= 1e-13


@pytest.fixture(scope="module")
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_v1.npz"))


class FixNet(torch.nn.Module):
    """The fixture's two tensors: the no-decay vector, the decayed matrix."""

    def __init__(self, p):
        super().__init__()
        n0 = R.FIX_SHAPES[0][0]
        self.v = torch.nn.Parameter(torch.tensor(p[:n0].reshape(R.FIX_SHAPES[0]), dtype=torch.float32))
        self.w = torch.nn.Parameter(torch.tensor(p[n0:].reshape(R.FIX_SHAPES[1]), dtype=torch.float32))


@pytest.mark.parametrize("case", R.FIX_CASES)
def test_reference_state_loads_and_the_next_step_matches(ops, golden, case, poison):
    """A state_dict laid out as the reference's class writes it, holding the fixture's reference run, resumes here."""
    from advmil_amd.optim import create_optimizer, parse_opt_name
    kind, la = parse_opt_name(case)
    p16 = golden[f"{case}/p"].astype(np.float32).astype(np.float64)
    s1, s2 = golden[f"{case}/s1"].astype(np.float64), golden[f"{case}/s2"].astype(np.float64)
    step, m_sched, la_step = (float(v) for v in golden[f"{case}/scalars"][:3])
    net = FixNet(p16).to(DEV)
    opt = create_optimizer(NS(case, wd=R.FIX_WD, lr=R.FIX_LR), net)
    n0 = R.FIX_SHAPES[0][0]
    s1n, s2n = R.STATE_NAMES[kind]
    cut = lambda a, i: torch.tensor(a[:n0].reshape(R.FIX_SHAPES[0]) if i == 0 else a[n0:].reshape(R.FIX_SHAPES[1]), dtype=torch.float32)  # noqa: E731
    state = {}
    for i in range(2):
        st = {"step": int(step) if kind in ("nadam", "radam") else torch.tensor(step), s1n: cut(s1, i), s2n: cut(s2, i)}
        if kind == "nadam":
            st["m_schedule"] = m_sched
        state[i] = st
    hyper = {"lr": R.FIX_LR * 0.5, "eps": 1e-6 if kind == "adadelta" else 1e-8}
    hyper.update({"rho": 0.9} if kind == "adadelta" else {"betas": (0.9, 0.999)})
    if kind == "nadam":
        hyper["schedule_decay"] = 4e-3
    if la:
        hyper.update(lookahead_alpha=0.5, lookahead_k=6, lookahead_step=int(la_step))
    sd = {"state": state, "param_groups": [dict(hyper, weight_decay=0.0, params=[0]), dict(hyper, weight_decay=R.FIX_WD, params=[1])]}
    if la:
        slow = golden[f"{case}/slow"].astype(np.float64)
        sd["slow_state"] = {i: {"slow_buffer": cut(slow, i)} for i in range(2)}
    opt.load_state_dict(sd)
    assert int(opt.step_t) == R.FIX_STEPS and opt.param_groups[0]["lr"] == R.FIX_LR * 0.5
    # the arena orders vectors before matrices: here that is the fixture's own order
    assert [k for _, _, k in opt._views] == [1003, 4000] and opt.flat_param.numel() == 1008 + 4000
    ref = R.Ref(kind, p16, wd=R.fix_inputs()[1], lr=R.FIX_LR * 0.5, lookahead=la)
    ref.s1, ref.s2, ref.step, ref.m_schedule, ref.la_step = s1.copy(), s2.copy(), int(step), m_sched, int(la_step)
    if la:
        ref.slow = slow.copy()
    g = (np.random.RandomState(5).standard_normal(5003) * 1e-2).astype(np.float32).astype(np.float64)
    for s_ in range(2):                      # steps 17 and 18: the second one is a lookahead sync (blend: the slow buffer was loaded)
        opt.zero_grad()
        net.v.grad.copy_(torch.tensor(g[:n0], dtype=torch.float32)); net.w.grad.copy_(torch.tensor(g[n0:].reshape(40, 100), dtype=torch.float32))
        opt.step()
        ref.do_step(g)
    got = np.concatenate([net.v.detach().cpu().numpy().reshape(-1), net.w.detach().cpu().numpy().reshape(-1)])
    err, bnd = R.bound(got, ref.p, p16, 2)
    assert err <= bnd, (err, bnd)
    if la:
        assert ref.syncs == [(18, "blend")]
        # a checkpoint whose slow_state no process can resolve (the reference keys it by id()): no slow buffer, created at the next sync
        sd["slow_state"] = {140230000000000 + i: v for i, v in sd["slow_state"].items()}
        opt.load_state_dict(sd)
        assert opt._la_first == 18 and opt._la_off == 0 and opt.la_state.tolist() == [18, 0]
        sd.pop("slow_state")
        for g_ in sd["param_groups"]:        # ... and a checkpoint of the bare base optimizer: the wrapper starts counting at the load
            for k_ in ("lookahead_alpha", "lookahead_k", "lookahead_step"):
                g_.pop(k_)
        opt.load_state_dict(sd)
        assert opt._la_first == 6 and opt._la_off == 16 and opt.param_groups[1]["lookahead_k"] == 6


# ------------------------------------------------------------------------------------------------------------------------------
# captured replays
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lookahead_nadam", "radam"])
def test_captured_replays_equal_eager_steps(ops, name, poison):
    """2k + 1 replays of ONE captured step(tick=False) + the shared tick launch == the eager steps, bit for bit: the step-dependent
    scalars, NAdam's schedule product and the lookahead sync decision all come from the device counter."""
    _, eager = make(name)
    _, cap = make(name)
    eager.l1_coef = cap.l1_coef = 1e-5
    nb = ops.adam_blocks(cap.flat_param.numel())
    part_c, part_e = torch.zeros(nb, device=DEV), torch.zeros(nb, device=DEV)
    seed = torch.zeros(1, dtype=torch.int64, device=DEV)
    static_grad = torch.zeros_like(cap.flat_grad)

    def one():
        cap.flat_grad.copy_(static_grad)
        cap.step(tick=False, abs_partial=part_c, clear_grad=True)
        ops.step_seed_tick(cap.step_t, seed, 1)

    _, warm = make(name)                                                # (every kernel of the step has run once before the capture)
    warm.step(tick=False, abs_partial=torch.zeros(nb, device=DEV), clear_grad=True)
    ops.step_seed_tick(warm.step_t, torch.zeros(1, dtype=torch.int64, device=DEV), 1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one()
    assert int(cap.step_t) == 0                                         # capturing ran nothing
    for t in range(STEPS):
        eager.zero_grad(); feed(eager, t)
        static_grad.copy_(eager.flat_grad)
        eager.step(abs_partial=part_e)
        g.replay()
        assert torch.equal(part_c, part_e), t
    torch.cuda.synchronize()
    a, b = arenas(eager), arenas(cap)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    assert int(eager.step_t) == int(cap.step_t) == STEPS and int(seed) == STEPS
    assert int(torch.count_nonzero(cap.flat_grad)) == 0                  # cleared behind the read
    if name.endswith("nadam"):
        assert torch.equal(eager.m_sched, cap.m_sched)
