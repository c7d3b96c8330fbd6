"""CPU: the float64 restatement of the fused optimizers (tests/optim_ref.py) against the reference's own runs
(tests/golden/optim_v1.npz, tests/golden/gen_golden_optim.py), the C layout of advmil_optim_t, and create_optimizer's reading of
the optimizer name -- none of it needs a device."""
import ctypes
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "optim_v1.npz"))


@pytest.fixture(scope="module")
def inputs():
    return R.fix_inputs()


@pytest.mark.parametrize("case", R.FIX_CASES)
def test_restatement_matches_the_reference_runs(fixture, inputs, case):
    p0, wd, grads = inputs
    mine = R.fix_run(case, p0, wd, grads)
    step, m_sched, la_step, err32, bnd32, exact = fixture[f"{case}/scalars"]
    ref_p = fixture[f"{case}/p"]
    assert ref_p.shape == (5003,) and mine.step == step == R.FIX_STEPS >= 16
    if exact:                               # the stored run is the reference in float64: the restatement is the same arithmetic
        assert float(np.abs(mine.p - ref_p).max()) <= 1e-12 * float(np.abs(ref_p).max())
    else:                                   # RAdam computes in float32 whatever it is given: the stored run is held to the fp32 bound
        err, bnd = R.bound(ref_p, mine.p, p0, R.FIX_STEPS)
        assert err <= bnd, (err, bnd)
    assert err32 <= bnd32                   # the reference's own float32 run sits inside the bound the GPU tests assert
    for k, a in (("s1", mine.s1), ("s2", mine.s2)):           # (stored as float32)
        assert float(np.abs(a - fixture[f"{case}/{k}"]).max()) <= 2e-5 * float(np.abs(a).max())
    if case.endswith("nadam"):
        assert abs(mine.m_schedule - m_sched) <= 1e-14
    if case.endswith("radam"):
        cross = R.radam_first_rectified_step()
        assert 1 < cross <= R.FIX_STEPS and mine.rectified == [t >= cross for t in range(1, R.FIX_STEPS + 1)]
    if case.startswith("lookahead_"):
        assert mine.syncs == [(6, "create"), (12, "blend")] and mine.la_step == la_step
        assert float(np.abs(mine.slow - fixture[f"{case}/slow"]).max()) <= 2e-5 * float(np.abs(mine.slow).max())
        bare = R.fix_run(case.split("_")[-1], p0, wd, grads, steps=6)          # the pinned quirk: the sync at k changes nothing
        assert np.array_equal(R.fix_run(case, p0, wd, grads, steps=6).p, bare.p)


def test_fixture_run_has_a_decay_group_a_no_decay_group_and_an_lr_halving(inputs):
    p0, wd, grads = inputs
    assert set(np.unique(wd)) == {0.0, R.FIX_WD} and 0 < R.FIX_HALVE_AT < R.FIX_STEPS
    a = R.fix_run("adamw", p0, wd, grads)
    assert a.lr == R.FIX_LR * 0.5


def test_optim_struct_layout_matches_c(tmp_path):
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    fields = [n for n, _ in _lib.Optim._fields_]
    body = "".join(f'printf("%zu\\n", offsetof(advmil_optim_t, {f}));' for f in fields)
    kinds = "".join(f'printf("%d\\n", (int)ADVMIL_OPT_{k.upper()});' for k in R.KINDS)
    src = tmp_path / "layout_optim.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "advmil_hip.h"\n'
                   f'int main(void){{printf("%zu\\n", sizeof(advmil_optim_t));{body}{kinds}return 0;}}\n')
    exe = tmp_path / "layout_optim"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.Optim)
    assert out[1:1 + len(fields)] == [getattr(_lib.Optim, f).offset for f in fields]
    assert out[1 + len(fields):] == [_lib.OPT_KINDS[k] for k in R.KINDS]


def test_optim_step_validates_before_it_launches():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    lib = _lib.lib()
    A16 = 0x7F0000001000

    def args(**kw):
        a = _lib.Optim()
        a.kind, a.n, a.lr, a.beta1, a.beta2, a.eps, a.grad_scale = 1, 64, 1e-3, 0.9, 0.999, 1e-8, 1.0
        a.p, a.grad, a.s1, a.s2, a.step = A16, A16 + (1 << 20), A16 + (2 << 20), A16 + (3 << 20), A16 + (4 << 20)
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)
    assert lib.advmil_optim_step(None, None) == -1
    assert lib.advmil_optim_step(args(kind=5), None) == -1                       # unknown kind
    assert lib.advmil_optim_step(args(n=0), None) == -1
    assert lib.advmil_optim_step(args(p=A16 + 4), None) == -1                    # arenas are walked in 16-byte units
    assert lib.advmil_optim_step(args(p_hi=A16 + (5 << 20)), None) == -1         # one plane only
    assert lib.advmil_optim_step(args(kind=2), None) == -1                       # NAdam without its schedule product
    assert lib.advmil_optim_step(args(lookahead=1), None) == -1                  # lookahead without a slow arena
    assert lib.advmil_optim_step(args(lookahead=1, slow=A16 + (5 << 20), la_state=A16 + (6 << 20), la_k=0), None) == -1
    assert lib.advmil_optim_step(args(beta2=1.0), None) == -1
    assert lib.advmil_optim_step(args(step=A16 + (4 << 20) + 2), None) == -1     # the step counter is an int32
    assert lib.advmil_optim_step(args(lookahead=1, slow=A16 + (5 << 20), la_state=A16 + (6 << 20) + 2, la_k=6), None) == -1


NS = lambda opt, **kw: SimpleNamespace(opt=opt, weight_decay=5e-4, lr=1e-3, opt_eps=None, opt_betas=None, momentum=None, **kw)  # noqa: E731


def test_name_parsing_follows_the_reference():
    from advmil_amd.optim import parse_opt_name
    assert parse_opt_name("AdamW") == ("adamw", False)
    assert parse_opt_name("lookahead_radam") == ("radam", True)
    assert parse_opt_name("Lookahead_NAdam") == ("nadam", True)
    assert parse_opt_name("foo_adadelta") == ("adadelta", False)                 # only a first token `lookahead` wraps
    assert parse_opt_name("lookahead") == ("lookahead", False)


@pytest.mark.parametrize("name", ["adamp", "sgdp", "novograd", "nvnovograd", "adafactor", "adahessian", "fusedadam", "fusedadamw",
                                  "fusedsgd", "fusedmomentum", "fusedlamb", "fusednovograd", "sgd", "nesterov", "momentum", "rmsprop",
                                  "rmsproptf", "lookahead_adamp"])
def test_out_of_scope_names_say_why_before_a_device_is_needed(name):
    from advmil_amd.optim import create_optimizer
    model = torch.nn.Linear(4, 4)            # on the CPU: a name with a path here would fail on the device check instead
    with pytest.raises(NotImplementedError, match=name.split("_")[-1]):
        create_optimizer(NS(name), model)


@pytest.mark.parametrize("name", ["adamw", "nadam", "radam", "adadelta", "lookahead_adam", "lookahead_radam"])
def test_in_scope_names_reach_the_device_check(name):
    from advmil_amd.optim import create_optimizer
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        create_optimizer(NS(name), torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match="invalid optimizer"):
        create_optimizer(NS("adamx"), torch.nn.Linear(4, 4))
