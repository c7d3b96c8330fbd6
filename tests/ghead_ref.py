"""The generator's bag-level head restated in torch on the CPU, and the comparison against it: shared by tests/test_ghead_gpu.py (width 1),
tests/test_gheadk_gpu.py (width K) and the poison runs. A result `r` is what those modules' run harnesses return: pred, dfeats, grads, the
recorded RNG sites (log), the model g, its input feats, the loss weights w, the injected noise nz, and kind / out_scale / seed."""
import numpy as np
import torch

from advmil_amd import synth

HEAD_KEYS = ("backbone.rho", "MLPs.")


def ref(r, zero_noise=False, dtype=torch.float64):
    """The head in `dtype`, with the kernel's masks and noise regenerated from the recorded sites (exact in either dtype)."""
    g, seed = r["g"], r["seed"]
    P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in g.state_dict().items()}
    x = r["feats"].detach().cpu().to(dtype).requires_grad_(True)

    def site(tag):
        ent = [e for e in r["log"] if e[0] == tag]
        return ent[0] if ent else None

    def mask(tag):
        e = site(tag)
        if e is None:
            return None
        _, sid, shape, p = e
        u = synth.kernel_uniform(seed, sid, int(np.prod(shape))).reshape(shape)
        return torch.from_numpy((u >= np.float32(p)).astype(np.float64)).to(dtype) / (1 - p)

    h = x
    if r["kind"] == "abmil":
        h = torch.relu(h @ P["backbone.rho.0.weight"].t() + P["backbone.rho.0.bias"])
        m = mask("abmil_rho")
        h = h * m if m is not None else h
    h = torch.relu(h @ P["MLPs.0.0.weight"].t() + P["MLPs.0.0.bias"])
    m = mask("gen_mlp0.2")
    h = h * m if m is not None else h
    W1 = P["MLPs.1.0.weight"]
    if W1.shape[1] == 2 * h.shape[1]:
        if zero_noise:
            nz = torch.zeros_like(h)
        elif r["nz"] is not None:
            nz = r["nz"][0].cpu().to(dtype)
        else:
            _, sid, shape, _ = site("noise")
            nz = torch.from_numpy(synth.kernel_uniform(seed, sid, int(np.prod(shape))).astype(np.float64)).reshape(h.shape).to(dtype)
        h = torch.cat([h, nz], dim=1)
    z = h @ W1.t() + P["MLPs.1.0.bias"]
    pred = torch.sigmoid(z) if r["out_scale"] == "sigmoid" else z
    (pred * r["w"].cpu().to(dtype)).sum().backward()
    return pred.detach(), x.grad, {k: v.grad for k, v in P.items()}


def rel_err(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = float(b.abs().max()) + 1e-12
    return float((a - b).abs().max()), scale


def close(a, b, tol, what, worst=None):
    """|a - b| <= tol * max|b| + 1e-7; prints the ratio error / bound (pytest -s)."""
    if b is None:
        assert a is None or float(a.abs().max()) == 0.0, what
        return
    assert a is not None, what
    d, scale = rel_err(a, b)
    bound = tol * scale + 1e-7
    print(f"  {what}: err {d:.3e} bound {bound:.3e} ratio {d / bound:.3f}")
    if worst is not None:
        worst[0] = max(worst[0], d / bound)
    assert d <= bound, (what, d, scale, tol)
