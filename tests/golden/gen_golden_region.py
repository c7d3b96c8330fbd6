#!/usr/bin/env python3
"""Golden vectors of the discriminator's region-level network (EmbedXLayer.fc1 + GAPool, eval mode) from the REAL reference, run in
float64 on the CPU through the import shims of gen_golden.py, and the pin of the float64 restatement (tests/region_ref.py) against the
reference modules in the same run.

Runs only in the build container (the reference never travels). Inputs and weights are regenerated from the repo's counter RNG
(advmil_amd/synth.py), so the fixture holds only outputs: tests/golden/region_v1.npz.
Usage:  python tests/golden/gen_golden_region.py

Two bags of 31 and 17 region rows (R = 48), each through the reference's fc1 and pool on its own (the reference pools one bag per call):
h1, fc, a, b, s, A, pooled, and the gradients of  L = sum(pooled * wp) + sum(fc * wf)  with respect to the ten parameters and to e
(matrices above 4096 entries as digests, region_ref.grad_digest; the pin below compares them whole)."""
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
GG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GG)

from advmil_amd import synth  # noqa: E402
from tests import region_ref as R  # noqa: E402

T, PARAM_SEED = GG.T, GG.PARAM_SEED
PREFIX = "D-prj:net_pair_one."
LENS = (31, 17)


def inputs():
    """e [48, 128], wp [2, 128], wf [48, 128]: the rows and the two fixed cotangents (tests/test_region_ref_cpu.py draws the same)."""
    n = sum(LENS)
    draw = lambda tag, r: synth.normal(synth.stream_key(1, f"region_{tag}"), r * R.D).reshape(r, R.D).astype(np.float64)   # noqa: E731
    return draw("e", n), draw("wp", len(LENS)), draw("wf", n)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    GG.install_shims()
    from model.model_utils import EmbedXLayer
    m = EmbedXLayer(SimpleNamespace(in_dim=1024, out_dim=128, ksize=1, backbone="avgpool", dropout=0.25))
    sd = m.state_dict()
    P32 = {k: synth.param(PARAM_SEED, PREFIX + k, tuple(v.shape)) for k, v in sd.items()}
    m.load_state_dict({k: T(v) for k, v in P32.items()})
    m = m.double().eval()
    P = {k: P32[k] for k in R.KEYS}
    assert {k: tuple(np.shape(v)) for k, v in P.items()} == R.shapes()
    e, wp, wf = inputs()
    cap = {}
    hooks = [mod.register_forward_hook(lambda _m, _i, o, k=k: cap.setdefault(k, []).append(o.detach().clone()))
             for k, mod in (("h1", m.fc1[2]), ("a", m.pool.fc1), ("b", m.pool.score), ("s", m.pool.fc2))]
    et = T(e).requires_grad_(True)
    fcs, pooled, loss = [], [], 0.0
    for k, (lo, hi) in enumerate(R.bounds(LENS)):
        fc = m.fc1(et[lo:hi][None])
        pb = m.pool(fc)
        assert tuple(pb.shape) == (1, R.D)
        loss = loss + (pb[0] * T(wp[k])).sum() + (fc[0] * T(wf[lo:hi])).sum()
        fcs.append(fc[0].detach()); pooled.append(pb[0].detach())
    loss.backward()
    for h in hooks:
        h.remove()
    ref = {k: torch.cat([t[0] for t in v]).numpy() for k, v in cap.items()}
    ref["s"] = ref["s"].reshape(-1)
    ref["fc"], ref["pooled"] = torch.cat(fcs).numpy(), torch.stack(pooled).numpy()
    ref["A"] = np.concatenate([torch.softmax(T(ref["s"][lo:hi]), 0).numpy() for lo, hi in R.bounds(LENS)])
    grads = {k: p.grad.numpy() for k, p in m.named_parameters() if k in R.KEYS}
    grads["e"] = et.grad.numpy()
    out = {k: ref[k] for k in ("h1", "fc", "a", "b", "s", "A", "pooled")}
    for k, g in grads.items():
        for suf, v in R.grad_digest(k, g).items():
            out[f"grad_{k}_{suf}"] = v
    out["keys"], out["lens"] = np.array(sorted(R.KEYS)), np.array(LENS)
    # the pin: the restatement on the same inputs, every tensor whole
    h1, fc, a, b, s = R.fwd(P, e)
    A, pl, _ = R.pool(s, fc, LENS)
    G = R.bwd(P, e, h1, fc, a, b, A, wp, None, wf, LENS)
    mine = dict(R.param_grads(G), e=G["de"])
    pin = {k: float(np.abs(v - ref[k]).max()) for k, v in (("h1", h1), ("fc", fc), ("a", a), ("b", b), ("s", s), ("A", A), ("pooled", pl))}
    pin.update({"grad_" + k: float(np.abs(mine[k] - grads[k]).max()) for k in grads})
    worst = max(pin.values())
    out["pin_worst"] = np.array(worst)
    print({k: f"{v:.2e}" for k, v in pin.items()})
    assert worst < 1e-12, worst
    path = os.path.join(HERE, "region_v1.npz")
    np.savez_compressed(path, **out)
    print("size", os.path.getsize(path))


if __name__ == "__main__":
    main()
