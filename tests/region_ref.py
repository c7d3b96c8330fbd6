"""Float64 restatement of the discriminator's region-level network (reference model/model_utils.py:188-210, EmbedXLayer.fc1, and
model/backbone_utils.py:31-56, GAPool), forward and analytic backward, as csrc/region.hip fuses it:

    h1 = keep1 / (1 - p1) * relu(e W1^T + b1)                 [R, 64]
    fc = h1 W2^T + b2                                        [R, 128]
    a | b = tanh | sigmoid (fc Wa^T + ba | fc Wb^T + bb)     [R, 128] each
    s = sum_j (a_j keepa_j / (1 - pg)) (b_j keepb_j / (1 - pg)) wc_j + bc
    A = softmax of s over each bag, pooled = A @ fc per bag, mean = the bag's mean of fc.

numpy only. Pinned to torch autograd in float64 over the same composition (tests/test_region_ref_cpu.py, < 1e-12) and to the reference
modules run in float64 (tests/golden/gen_golden_region.py -> tests/golden/region_v1.npz, read by the same CPU test).

Parameters are a dict keyed like EmbedXLayer's state_dict below `net_pair_one.` (KEYS); `pool.fc2.bias` may be missing or None (the
entry points accept bc == NULL). Keep masks are boolean [R, width] arrays or None (no draw: neither the mask nor the 1 / (1 - p))."""
import numpy as np

from advmil_amd import synth

D, H1 = 128, 64
KEYS = ("fc1.0.weight", "fc1.0.bias", "fc1.3.weight", "fc1.3.bias", "pool.fc1.0.weight", "pool.fc1.0.bias", "pool.score.0.weight",
        "pool.score.0.bias", "pool.fc2.weight", "pool.fc2.bias")
SITES = ("dx_fc1", "gapool_att_a", "gapool_att_b")          # the three dropout call sites, in the order they are drawn
SITE_WIDTH = {"dx_fc1": H1, "gapool_att_a": D, "gapool_att_b": D}


def shapes(d=D):
    return {"fc1.0.weight": (d // 2, d), "fc1.0.bias": (d // 2,), "fc1.3.weight": (d, d // 2), "fc1.3.bias": (d,),
            "pool.fc1.0.weight": (d, d), "pool.fc1.0.bias": (d,), "pool.score.0.weight": (d, d), "pool.score.0.bias": (d,),
            "pool.fc2.weight": (1, d), "pool.fc2.bias": (1,)}


def f64(a):
    return np.asarray(a, dtype=np.float64)


def _scale(keep, p):
    """keep / (1 - p) as float64, or 1.0 when there is no draw."""
    return 1.0 if keep is None else np.asarray(keep, dtype=bool).astype(np.float64) / (1.0 - float(p))


def _bc(P):
    v = P.get("pool.fc2.bias")
    return 0.0 if v is None else float(f64(v).reshape(-1)[0])


def preact(P, e):
    """Z1 = e W1^T + b1: the input of the network's one ReLU (its distance from 0 decides whether a branch is open)."""
    return f64(e) @ f64(P["fc1.0.weight"]).T + f64(P["fc1.0.bias"])


def fwd(P, e, keep1=None, keepa=None, keepb=None, p1=0.0, pg=0.0):
    """-> h1 [R, 64], fc [R, 128], a, b [R, 128] (before their dropout, as the kernels store them), s [R]."""
    h1 = np.maximum(preact(P, e), 0.0) * _scale(keep1, p1)
    fc = h1 @ f64(P["fc1.3.weight"]).T + f64(P["fc1.3.bias"])
    a = np.tanh(fc @ f64(P["pool.fc1.0.weight"]).T + f64(P["pool.fc1.0.bias"]))
    b = 1.0 / (1.0 + np.exp(-(fc @ f64(P["pool.score.0.weight"]).T + f64(P["pool.score.0.bias"]))))
    s = ((a * _scale(keepa, pg)) * (b * _scale(keepb, pg))) @ f64(P["pool.fc2.weight"]).reshape(-1) + _bc(P)
    return h1, fc, a, b, s


def bounds(lens):
    o = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
    return [(int(o[i]), int(o[i + 1])) for i in range(len(lens))]


def pool(s, fc, lens):
    """-> A [R] (softmax of s within each bag), pooled [B, 128], mean [B, 128]."""
    s, fc = f64(s).reshape(-1), f64(fc)
    assert sum(lens) == fc.shape[0] == s.shape[0]
    A = np.empty_like(s)
    pooled, mean = [], []
    for lo, hi in bounds(lens):
        x = np.exp(s[lo:hi] - s[lo:hi].max())
        A[lo:hi] = x / x.sum()
        pooled.append(A[lo:hi] @ fc[lo:hi])
        mean.append(fc[lo:hi].mean(axis=0))
    return A, np.stack(pooled), np.stack(mean)


def pool_bwd_ds(dpooled, A, fc, lens):
    """ds [R] of sum(pooled * dpooled): A_r (t_r - sum_bag A t), t_r = fc_r . dpooled[bag(r)]."""
    dpooled, A, fc = f64(dpooled).reshape(len(lens), -1), f64(A).reshape(-1), f64(fc)
    ds = np.empty_like(A)
    for k, (lo, hi) in enumerate(bounds(lens)):
        t = fc[lo:hi] @ dpooled[k]
        ds[lo:hi] = A[lo:hi] * (t - (A[lo:hi] * t).sum())
    return ds


def bwd(P, e, h1, fc, a, b, A, dpooled, dmean, dfc_add, lens, keep1=None, keepa=None, keepb=None, p1=0.0, pg=0.0, ds=None):
    """Gradients of L = sum(pooled * dpooled) + sum(mean * dmean) + sum(fc * dfc_add) (dmean / dfc_add may be None).

    The saved forward is (e, h1, fc, a, b, A): the ReLU mask is h1 > 0 (a dropped entry has h1 == 0 as well), the gate derivatives are
    1 - a^2 and b (1 - b) of the a, b given -- so that a kernel fed its own forward's h1 / a / b is judged on the same branches.
    `ds`: the gradient with respect to the scores, if it was worked out elsewhere (else pool_bwd_ds of the arguments).
    -> dict ds, dG [R, 256], dfc, dpre [R, 64], de, dwc [128], dbab [256], dbc [1], db2, db1, dWab [256, 128], dW2 [128, 64], dW1 [64, 128]."""
    e, h1, fc, a, b, A = f64(e), f64(h1), f64(fc), f64(a), f64(b), f64(A).reshape(-1)
    nb = len(lens)
    dpooled = f64(dpooled).reshape(nb, -1)
    ds = pool_bwd_ds(dpooled, A, fc, lens) if ds is None else f64(ds).reshape(-1)
    ma, mb = _scale(keepa, pg), _scale(keepb, pg)
    wc = f64(P["pool.fc2.weight"]).reshape(-1)
    ad, bd = a * ma, b * mb
    d1 = ds[:, None]
    ga = d1 * wc * bd * ma * (1.0 - a * a)
    gb = d1 * wc * ad * mb * b * (1.0 - b)
    dG = np.concatenate([ga, gb], axis=1)
    Wab = np.concatenate([f64(P["pool.fc1.0.weight"]), f64(P["pool.score.0.weight"])], axis=0)
    dfc = dG @ Wab
    for k, (lo, hi) in enumerate(bounds(lens)):
        dfc[lo:hi] += A[lo:hi, None] * dpooled[k][None, :]
        if dmean is not None:
            dfc[lo:hi] += f64(dmean).reshape(nb, -1)[k][None, :] / float(hi - lo)
    if dfc_add is not None:
        dfc = dfc + f64(dfc_add)
    inv1 = 1.0 if keep1 is None else 1.0 / (1.0 - float(p1))
    dpre = (dfc @ f64(P["fc1.3.weight"])) * (h1 > 0.0) * inv1
    return {"ds": ds, "dG": dG, "dfc": dfc, "dpre": dpre, "de": dpre @ f64(P["fc1.0.weight"]),
            "dwc": (d1 * ad * bd).sum(axis=0), "dbab": dG.sum(axis=0), "dbc": np.array([ds.sum()]), "db2": dfc.sum(axis=0),
            "db1": dpre.sum(axis=0), "dWab": dG.T @ fc, "dW2": dfc.T @ h1, "dW1": dpre.T @ e}


def param_grads(G):
    """The analytic backward's results keyed like the parameters (shaped like them)."""
    return {"fc1.0.weight": G["dW1"], "fc1.0.bias": G["db1"], "fc1.3.weight": G["dW2"], "fc1.3.bias": G["db2"],
            "pool.fc1.0.weight": G["dWab"][:D], "pool.fc1.0.bias": G["dbab"][:D], "pool.score.0.weight": G["dWab"][D:],
            "pool.score.0.bias": G["dbab"][D:], "pool.fc2.weight": G["dwc"].reshape(1, -1), "pool.fc2.bias": G["dbc"]}


def keep_masks(seed, sids, R, p1, pg, row_map=None):
    """The three keep masks (dx_fc1 [R, 64], gapool_att_a, gapool_att_b [R, 128]) as the kernels draw them: element [n, c] of a site is
    the draw of its stream at flat index row_map[n] * width + c (row_map None: the local row n). A site whose rate is 0 gives None."""
    rows = np.arange(R, dtype=np.int64) if row_map is None else np.asarray(row_map, dtype=np.int64).reshape(-1)
    assert rows.shape[0] == R
    out = []
    for sid, tag, p in zip(sids, SITES, (p1, pg, pg)):
        if not p > 0.0:
            out.append(None)
            continue
        w = SITE_WIDTH[tag]
        out.append(np.stack([synth.dropout_keep(seed, sid, w, p, offset=int(r) * w) for r in rows]))
    return out


DIGEST_FULL = 4096


def grad_digest(name, G):
    """What the fixture keeps of a gradient: the tensor itself up to DIGEST_FULL entries; of a larger matrix its products with two fixed
    vectors, one from each side, and its Frobenius norm (tests/gapool_ref.py::grad_digest, under this fixture's own stream names)."""
    G = f64(G)
    if G.size <= DIGEST_FULL:
        return {"full": G}
    G2 = G.reshape(G.shape[0], -1)
    v = synth.normal(synth.stream_key(2, f"region_left:{name}"), G2.shape[0]).astype(np.float64)
    u = synth.normal(synth.stream_key(2, f"region_right:{name}"), G2.shape[1]).astype(np.float64)
    return {"left": v @ G2, "right": G2 @ u, "norm": np.array(np.sqrt((G2 * G2).sum()))}
