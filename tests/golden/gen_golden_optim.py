#!/usr/bin/env python3
"""Golden vectors for the fused optimizers (tests/golden/optim_v1.npz): the REFERENCE's optimizer classes -- torch.optim.AdamW /
Adadelta / Adam, optim/nadam.py::Nadam, optim/radam.py::RAdam, optim/lookahead.py::Lookahead, built the way optim/optim_factory.py
builds them -- stepped on the CPU over the seeded run of tests/optim_ref.py (5 003 elements in a no-decay vector and a decayed
matrix, 16 steps, the lr halved after the 8th), and the pin of the float64 restatement tests/optim_ref.py::Ref against them.

Stored per case: the final parameters of the float64 run (float64), its two state tensors and the lookahead slow buffer (float32),
m_schedule, the error of the reference's own float32 run against the restatement with the bound the GPU tests assert, and whether the
stored run is float64-exact (RAdam's is not: its step() computes in float32 whatever the parameters are).
Only numbers. Build container only. Usage: python tests/golden/gen_golden_optim.py <path of the reference checkout>"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import optim_ref as R  # noqa: E402


def reference_run(case, dtype, classes):
    p0, wd, grads = R.fix_inputs()
    name, lookahead = case.split("_")[-1], case.startswith("lookahead_")
    n0 = int(np.prod(R.FIX_SHAPES[0]))
    vec = torch.nn.Parameter(torch.tensor(p0[:n0].reshape(R.FIX_SHAPES[0]), dtype=dtype))
    mat = torch.nn.Parameter(torch.tensor(p0[n0:].reshape(R.FIX_SHAPES[1]), dtype=dtype))
    groups = [{"params": [vec], "weight_decay": 0.0}, {"params": [mat], "weight_decay": R.FIX_WD}]      # add_weight_decay's two groups
    opt = classes[name](groups, lr=R.FIX_LR, weight_decay=0.0)
    base = opt
    if lookahead:
        opt = classes["lookahead"](opt)
    rectified = []
    for t in range(R.FIX_STEPS):
        if t == R.FIX_HALVE_AT:
            for g in opt.param_groups:
                g["lr"] *= 0.5
        vec.grad = torch.tensor(grads[t][:n0].reshape(R.FIX_SHAPES[0]), dtype=dtype)
        mat.grad = torch.tensor(grads[t][n0:].reshape(R.FIX_SHAPES[1]), dtype=dtype)
        opt.step()
        if name == "radam":                  # the branch the reference itself took: its memo holds [step, N_sma, step_size] (radam.py:54-71)
            memo = base.buffer[(t + 1) % 10]
            assert memo[0] == t + 1
            rectified.append(bool(memo[1] >= 5))
    flat = lambda a, b: np.concatenate([a.detach().double().reshape(-1).numpy(), b.detach().double().reshape(-1).numpy()])  # noqa: E731
    s1, s2 = R.STATE_NAMES[name]
    out = {"p": flat(vec, mat), "s1": flat(base.state[vec][s1], base.state[mat][s1]), "s2": flat(base.state[vec][s2], base.state[mat][s2]),
           "step": float(base.state[vec]["step"]), "m_schedule": float(base.state[vec].get("m_schedule", 1.0))}
    out["rectified"] = rectified
    if lookahead:
        out["slow"] = flat(opt.state[vec]["slow_buffer"], opt.state[mat]["slow_buffer"])
        out["la_step"] = float(opt.param_groups[0]["lookahead_step"])
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ADVMIL_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    sys.path.insert(0, ref)
    torch.set_num_threads(4)
    from optim.lookahead import Lookahead
    from optim.nadam import Nadam
    from optim.radam import RAdam
    classes = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "adadelta": torch.optim.Adadelta, "nadam": Nadam, "radam": RAdam,
               "lookahead": Lookahead}
    p0, wd, grads = R.fix_inputs()
    out = {}
    cross = R.radam_first_rectified_step()
    assert 1 < cross <= R.FIX_STEPS, cross
    for case in R.FIX_CASES:
        r64, r32 = reference_run(case, torch.float64, classes), reference_run(case, torch.float32, classes)
        mine = R.fix_run(case, p0, wd, grads)
        # the restatement IS the reference's arithmetic in float64 -- except for RAdam, whose step() casts parameters and gradients to
        # float32 whatever they are (optim/radam.py:31,35): there the "float64" run is a float32 run too, and the pin is the bound below
        exact = not case.endswith("radam")
        for k, a in (("p", mine.p), ("s1", mine.s1), ("s2", mine.s2)):
            d = float(np.abs(a - r64[k]).max())
            if exact:
                assert d <= 1e-12 * max(float(np.abs(r64[k]).max()), 1e-30) + 1e-18, (case, k, d)
            elif k != "p":
                assert d <= 2e-5 * float(np.abs(a).max()), (case, k, d)
        assert mine.step == r64["step"] == R.FIX_STEPS
        if case.endswith("nadam"):
            assert abs(mine.m_schedule - r64["m_schedule"]) <= 1e-14, (mine.m_schedule, r64["m_schedule"])
        if case.endswith("radam"):          # both branches, the crossing where the restatement says it is
            assert mine.rectified == [t >= cross for t in range(1, R.FIX_STEPS + 1)] and not mine.rectified[0] and mine.rectified[-1]
            assert r64["rectified"] == r32["rectified"] == mine.rectified            # ... and where the reference's own runs took it
        if case.startswith("lookahead_"):
            assert float(np.abs(mine.slow - r64["slow"]).max()) <= (1e-12 if exact else 2e-5) * float(np.abs(r64["slow"]).max())
            assert mine.syncs == [(6, "create"), (12, "blend")], mine.syncs
            assert mine.la_step == r64["la_step"]
            # the sync at k changes nothing: the run cut there equals the bare base optimizer's
            a, b = R.fix_run(case, p0, wd, grads, steps=6), R.fix_run(case.split("_")[-1], p0, wd, grads, steps=6)
            assert np.array_equal(a.p, b.p)
        # the reference's own float32 run sits inside the bound the GPU tests assert
        err, bnd = R.bound(r32["p"], mine.p, p0, R.FIX_STEPS)
        disp = float(np.abs(mine.p - p0).max())
        print(f"{case:20s} fp32 reference: error {err:.3e}  bound {bnd:.3e}  error/displacement {err / disp:.2e}  displacement {disp:.2e}")
        assert err <= bnd, (case, err, bnd)
        out[f"{case}/p"] = r64["p"]
        out[f"{case}/s1"], out[f"{case}/s2"] = r64["s1"].astype(np.float32), r64["s2"].astype(np.float32)
        out[f"{case}/scalars"] = np.array([r64["step"], r64["m_schedule"], r64.get("la_step", 0.0), err, bnd, float(exact)], dtype=np.float64)
        if "slow" in r64:
            out[f"{case}/slow"] = r64["slow"].astype(np.float32)
    path = os.path.join(HERE, "optim_v1.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; RAdam rectifies from step", cross)


if __name__ == "__main__":
    main()
