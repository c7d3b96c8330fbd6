"""Float64 restatement of the gated-attention region embedding (reference model/backbone_utils.py:171-202, GAPoolPatchEmbedding with
ksize 1) and of its 16-row pooling alone, forward and analytic backward. numpy only; pinned to the reference module run in float64 by
tests/golden/gen_golden_gapool.py (tests/golden/ORACLE_PIN_gapool.json, < 1e-12) and to tests/golden/gapool_v1.npz by
tests/test_gapool_cpu.py.

Parameters are a dict keyed like the layer's state_dict (conv.weight [d, C, 1, 1] or [d, C], conv.bias, norm.weight, norm.bias,
pool.fc1.0.*, pool.score.0.*, pool.fc2.weight [1, d], pool.fc2.bias [1])."""
import numpy as np

from advmil_amd import synth

KEYS = ("conv.weight", "conv.bias", "norm.weight", "norm.bias", "pool.fc1.0.weight", "pool.fc1.0.bias", "pool.score.0.weight",
        "pool.score.0.bias", "pool.fc2.weight", "pool.fc2.bias")
EPS = 1e-5


def shapes(c, d):
    """state_dict shapes of the layer (probed on the reference module)."""
    return {"conv.weight": (d, c, 1, 1), "conv.bias": (d,), "norm.weight": (d,), "norm.bias": (d,),
            "pool.fc1.0.weight": (d, d), "pool.fc1.0.bias": (d,), "pool.score.0.weight": (d, d), "pool.score.0.bias": (d,),
            "pool.fc2.weight": (1, d), "pool.fc2.bias": (1,)}


def f64(a):
    return np.asarray(a, dtype=np.float64)


def pool_fwd(s, z, dup=1):
    """s[N], z[N, d] -> (emb [dup N/16, d], A[N]): softmax of s over each 16 consecutive rows, weighted row sums."""
    s, z = f64(s).reshape(-1), f64(z)
    N, d = z.shape
    assert N % 16 == 0 and s.shape[0] == N
    s3 = s.reshape(-1, 16)
    e = np.exp(s3 - s3.max(axis=1, keepdims=True))
    A = e / e.sum(axis=1, keepdims=True)
    emb = np.einsum("ri,rid->rd", A, z.reshape(-1, 16, d))
    return np.concatenate([emb] * dup, axis=0), A.reshape(-1)


def pool_bwd(demb, A, z, dup=1):
    """-> (ds[N], dz[N, d]) for the upstream gradient demb [dup N/16, d] (dup = 2: its two halves summed)."""
    demb, A, z = f64(demb), f64(A).reshape(-1, 16), f64(z)
    N, d = z.shape
    R = N // 16
    g = demb[:R] + (demb[R:] if dup == 2 else 0.0)
    t = np.einsum("rid,rd->ri", z.reshape(R, 16, d), g)
    c = (A * t).sum(axis=1, keepdims=True)
    ds = A * (t - c)
    dz = A[:, :, None] * g[:, None, :]
    return ds.reshape(-1), dz.reshape(N, d)


def layer_fwd(P, x, dup=1):
    """x[N, C] -> dict of every intermediate: y, xhat, rstd, n (LayerNorm output), z, a, b, s, A, emb."""
    x = f64(x)
    W = f64(P["conv.weight"]).reshape(P["conv.weight"].shape[0], -1)
    y = x @ W.T + f64(P["conv.bias"])
    mu = y.mean(axis=1, keepdims=True)
    var = ((y - mu) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + EPS)
    xhat = (y - mu) * rstd
    n = xhat * f64(P["norm.weight"]) + f64(P["norm.bias"])
    z = np.maximum(n, 0.0)
    a = np.tanh(z @ f64(P["pool.fc1.0.weight"]).T + f64(P["pool.fc1.0.bias"]))
    b = 1.0 / (1.0 + np.exp(-(z @ f64(P["pool.score.0.weight"]).T + f64(P["pool.score.0.bias"]))))
    s = (a * b) @ f64(P["pool.fc2.weight"]).reshape(-1) + float(f64(P["pool.fc2.bias"]).reshape(-1)[0])
    emb, A = pool_fwd(s, z, dup)
    return {"x": x, "y": y, "xhat": xhat, "rstd": rstd, "n": n, "z": z, "a": a, "b": b, "s": s, "A": A, "emb": emb}


def layer_bwd(P, f, demb, dup=1):
    """Gradients of sum(emb * demb) with respect to every parameter (keyed like P, shaped like P) and to x ("x")."""
    ds, dz = pool_bwd(demb, f["A"], f["z"], dup)
    a, b, z = f["a"], f["b"], f["z"]
    mag = float(np.abs(ds).sum())                # ("ds_mag": what sum ds = the gradient of pool.fc2.bias cancels from)
    wc = f64(P["pool.fc2.weight"]).reshape(-1)
    G = {"pool.fc2.weight": (ds[:, None] * a * b).sum(axis=0).reshape(np.shape(P["pool.fc2.weight"])), "pool.fc2.bias": np.array([ds.sum()])}
    dab = ds[:, None] * wc[None, :]
    da = dab * b * (1.0 - a * a)
    db = dab * a * b * (1.0 - b)
    G["pool.fc1.0.weight"], G["pool.fc1.0.bias"] = da.T @ z, da.sum(axis=0)
    G["pool.score.0.weight"], G["pool.score.0.bias"] = db.T @ z, db.sum(axis=0)
    dz = dz + da @ f64(P["pool.fc1.0.weight"]) + db @ f64(P["pool.score.0.weight"])
    dn = dz * (f["n"] > 0.0)
    G["norm.weight"], G["norm.bias"] = (dn * f["xhat"]).sum(axis=0), dn.sum(axis=0)
    dxh = dn * f64(P["norm.weight"])
    dy = f["rstd"] * (dxh - dxh.mean(axis=1, keepdims=True) - f["xhat"] * (dxh * f["xhat"]).mean(axis=1, keepdims=True))
    G["conv.weight"] = (dy.T @ f["x"]).reshape(np.shape(P["conv.weight"]))
    G["conv.bias"] = dy.sum(axis=0)
    G["x"] = dy @ f64(P["conv.weight"]).reshape(P["conv.weight"].shape[0], -1)
    G["ds_mag"] = mag
    return G


def relu_margin(f):
    """Smallest |LayerNorm output| of the forward `f`: how far every pre-ReLU value sits from the mask's switching point."""
    return float(np.abs(f["n"]).min())


DIGEST_FULL = 4096


def grad_digest(name, G):
    """What the fixture keeps of a gradient: the tensor itself up to DIGEST_FULL entries; of a larger matrix (the conv and gate weights:
    megabytes in float64) its products with two fixed vectors, one from each side, and its Frobenius norm. -> {suffix: array}."""
    G = f64(G)
    if G.size <= DIGEST_FULL:
        return {"full": G}
    G2 = G.reshape(G.shape[0], -1)
    v = synth.normal(synth.stream_key(2, f"gapool_left:{name}"), G2.shape[0]).astype(np.float64)
    u = synth.normal(synth.stream_key(2, f"gapool_right:{name}"), G2.shape[1]).astype(np.float64)
    return {"left": v @ G2, "right": G2 @ u, "norm": np.array(np.sqrt((G2 * G2).sum()))}
