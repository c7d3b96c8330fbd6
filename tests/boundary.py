"""The ReLU-boundary rule ("ReLU-boundary inputs"), as one helper.

A fp32-accumulating kernel and a float64 reference can disagree on which branch of a ReLU an entry takes when its pre-activation Z is
within round-off of 0, and each such entry moves the upstream parameter gradients by that row's whole contribution. The rule lets the
REFERENCE say which deviations that can produce, and nothing else:

  * a *site* is one ReLU of the network. The float64 oracle hands over its input Z and dL/d(ReLU output) (`taps` of
    oracle/advmil_oracle.py);
  * its undecided set U = {abs(Z64) < delta}; delta is a reference-side number: for a site fed by the bag itself 4 x the largest
    deviation of a CPU emulation of the documented arithmetic from float64 (`emulated_preact`), for a deeper site 4 x TOL = 8e-5, TOL
    being the absolute forward bound the suite asserts on such activations;
  * condition, asserted: len(U) <= 2e-4 x Z.numel();
  * candidate k = (i, u) in U has one direction in parameter-gradient space: the vector-Jacobian product of Z with the cotangent
    -+ dL/dReLU_out[i, u] e_iu (sign: away from the reference's branch). The residual got - want is fitted by least squares with one
    coefficient per candidate, each coefficient must be within 0.05 of 0 or 1, the 0/1 combination is subtracted, and then EVERY entry
    of EVERY parameter must be inside tol_rel x max abs(want) + tol_abs.

A kernel may therefore differ from float64 only by taking the other branch on entries the reference itself calls undecided.
What a flip does downstream of the ReLU is not modelled: it changes the forward by less than delta, i.e. by less than TOL."""
import torch
import torch.nn.functional as F

TOL = 2e-5
DEEP_DELTA = 4 * TOL
SHARE_MAX = 2e-4
S_BAND = 0.05


def split_bf16(a):
    hi = a.bfloat16().float()
    return hi, (a - hi).bfloat16().float()


def emulated_matmul(x, w, mode):
    """x[R, C] @ w[U, C]^T in the arithmetic under test, on the CPU: 'exact' = an fp32 matmul; 'bf16x3' = hi/lo bf16 split of both
    operands, hi*hi + hi*lo + lo*hi as three fp32 products, fp32 accumulation (advmil_amd/csrc/bf16split.h)."""
    x, w = x.float(), w.float()
    if mode == "exact":
        return x @ w.t()
    assert mode == "bf16x3", mode
    xh, xl = split_bf16(x)
    wh, wl = split_bf16(w)
    return xh @ wh.t() + (xh @ wl.t() + xl @ wh.t())


def emulated_preact(x, w, b, mode, ln=None):
    """Z of a bag-fed site in the arithmetic under test: Linear (-> LayerNorm in fp32 behind it, ln = (gamma, beta))."""
    y = emulated_matmul(x, w.reshape(w.shape[0], -1), mode) + b.float()
    if ln is not None:
        y = F.layer_norm(y, (y.shape[-1],), ln[0].float(), ln[1].float(), 1e-5)
    return y


class Site:
    """One ReLU of the network over all rows of the step.

    Z, gY: float64 [R, U] (the oracle's pre-activation and dL/d(ReLU output); where several forwards of one backward share the same Z
    -- D's real and fake pass over one patch embedding -- gY is their SUM: the kernel takes one branch for both).
    Bag-fed sites (`kind` 'linear' / 'conv_ln'): `rows` = the float64 input rows [R, C], `names` = parameter names by role ('weight',
    'bias', and 'gamma' / 'beta' behind a LayerNorm), `params` = those parameters in float64; directions are computed on the one-row
    subgraph. Deeper sites (`kind` 'deep', see deep_site): `vjp(i, u, sign)` -> {parameter name: direction} through the oracle's retained
    graph, `solve_on` = the site's own weight (no flip upstream of it touches that tensor)."""

    def __init__(self, name, Z, gY, delta, kind, names=None, rows=None, params=None, vjp=None, solve_on=None):
        self.name, self.Z, self.gY, self.delta, self.kind = name, Z.detach().double(), gY.detach().double(), float(delta), kind
        self.names, self.rows, self.params, self.vjp, self.solve_on = names, rows, params, vjp, solve_on
        assert self.Z.dim() == 2 and self.Z.shape == self.gY.shape, (name, self.Z.shape, self.gY.shape)


def bag_fed_site(name, rows, Z, gY, P32, names, mode):
    """A site fed by the bag itself. delta = 4 x max abs(Z_emul - Z64), Z_emul from `emulated_preact` on the fp32 parameters P32."""
    ln = (P32[names["gamma"]], P32[names["beta"]]) if "gamma" in names else None
    with torch.no_grad():
        Ze = emulated_preact(rows.float(), P32[names["weight"]], P32[names["bias"]], mode, ln)
        dev = float((Ze.double() - Z.detach().double()).abs().max())
    params = {r: P32[n].double() for r, n in names.items()}
    return Site(name, Z, gY, 4.0 * dev, "conv_ln" if ln is not None else "linear", names=names, rows=rows.double(), params=params)


def deep_site(name, groups, params, solve_on):
    """A deeper site over all bags of the step. `groups`: one list of oracle taps per block of rows; the taps of a group share one
    Z (one tap, or D's real and fake tap where the ReLU's input does not depend on the pair -- the kernel takes one branch for
    both, so their directions are ADDED). gY = sum of a group's Y.grad, direction = sum of its taps' vector-Jacobian products through the
    oracle's retained graph onto `params` ({name: the oracle's leaf tensor})."""
    names = list(params)
    plist = [params[n] for n in names]
    blocks, Zs, Gs, r0 = [], [], [], 0
    for taps in groups:
        Z0 = taps[0]["Z"].detach()
        shape = Z0.shape
        for t in taps[1:]:
            assert torch.equal(t["Z"].detach(), Z0), name
        gys = [(t["Y"].grad if t["Y"].grad is not None else torch.zeros_like(Z0)).detach().double().reshape(-1, shape[-1]) for t in taps]
        Z2 = Z0.reshape(-1, shape[-1])
        blocks.append((r0, r0 + Z2.shape[0], taps, gys, shape))
        Zs.append(Z2); Gs.append(sum(gys)); r0 += Z2.shape[0]

    def block_of(i):
        for blk in blocks:
            if blk[0] <= i < blk[1]:
                return blk
        raise IndexError(i)

    def cots(i, u):
        a, _, _, gys, _ = block_of(i)
        return [float(g[i - a, u]) for g in gys]

    def vjp(i, u, sign):
        a, b_, taps, gys, shape = block_of(i)
        out = {}
        for t, g in zip(taps, gys):
            c = sign * float(g[i - a, u])
            if c == 0.0:
                continue
            cot = torch.zeros(b_ - a, shape[-1], dtype=t["Z"].dtype)
            cot[i - a, u] = c
            gs = torch.autograd.grad(t["Z"], plist, grad_outputs=cot.reshape(shape), retain_graph=True, allow_unused=True)
            for n, gr in zip(names, gs):
                if gr is not None:
                    out[n] = out[n] + gr if n in out else gr.clone()
        return out

    s = Site(name, torch.cat(Zs), torch.cat(Gs), DEEP_DELTA, "deep", vjp=vjp, solve_on=solve_on)
    s.cots = cots
    return s


def _solve(G, rhs):
    """Least-squares coefficients from the directions' Gram matrix. The directions' norms span many orders of magnitude (they scale
    with dL/dReLU_out), so the system is solved for unit-norm directions: a rank-revealing solver would otherwise drop the small ones."""
    if G.shape[0] == 0:
        return rhs.clone()
    d = G.diagonal().clamp_min(1e-300).rsqrt()
    t = torch.linalg.lstsq(G * d[:, None] * d[None, :], (rhs * d).unsqueeze(1)).solution.squeeze(1)
    return t * d


def _check_s(site, s, mag, bound, idx):
    """Coefficients must be 0 or 1 within S_BAND. A candidate whose whole direction is smaller than the bound on every entry cannot
    show either way, and below the residual's round-off level its coefficient is not determined at all: it counts as taken only when
    the fit says 1 within S_BAND, as not taken otherwise, and is not asserted."""
    s0 = s.round()
    for k in range(s.shape[0]):
        if float(mag[k]) < bound:
            s0[k] = 1.0 if abs(float(s[k]) - 1.0) <= S_BAND else 0.0
            continue
        assert abs(float(s[k]) - float(s0[k])) <= S_BAND and float(s0[k]) in (0.0, 1.0), \
            f"site {site.name}: candidate (row {idx[k][0]}, unit {idx[k][1]}) has coefficient {float(s[k]):.4f}: neither branch of the ReLU"
    return s0


def _account(site, R, bounds):
    """Fit and subtract one site's candidates from the residuals R (in place). Returns (len(U), share, candidates solved, taken)."""
    Z, gY = site.Z, site.gY
    und = Z.abs() < site.delta
    nU = int(und.sum())
    share = nU / Z.numel()
    assert nU <= SHARE_MAX * Z.numel(), \
        f"site {site.name}: {nU} of {Z.numel()} entries ({share:.2e}) within delta = {site.delta:.3e} of the branch point: over {SHARE_MAX:g}; pick other sizes"
    idx = und.nonzero()
    if site.kind == "deep":
        nz = torch.tensor([any(c != 0.0 for c in site.cots(i, u)) for i, u in idx.tolist()], dtype=torch.bool).reshape(-1)
    else:
        nz = gY[idx[:, 0], idx[:, 1]] != 0
    idx = idx[nz]                       # (a zero direction -- the entry was dropped by the mask -- cannot show: left out)
    K = int(idx.shape[0])
    if K == 0:
        return nU, share, 0, 0
    ii, uu = idx[:, 0], idx[:, 1]
    sign = torch.where(Z[ii, uu] > 0, -1.0, 1.0).double()          # away from the reference's branch
    il = idx.tolist()
    if site.kind == "deep":
        dirs = [site.vjp(i, u, float(sg)) for (i, u), sg in zip(il, sign.tolist())]
        A = torch.stack([d[site.solve_on].reshape(-1).double() for d in dirs], dim=1)            # [numel, K]
        s = _solve(A.t() @ A, A.t() @ R[site.solve_on].reshape(-1))
        s0 = _check_s(site, s, A.abs().amax(dim=0), bounds[site.solve_on], il)
        for k, d in enumerate(dirs):
            if float(s0[k]) != 0.0:
                for n, g in d.items():
                    if n in R:
                        R[n] -= float(s0[k]) * g.double().reshape(R[n].shape)
        return nU, share, K, int(s0.sum())
    c = sign * gY[ii, uu]
    Xc = site.rows[ii]                                               # [K, C]
    U = Z.shape[1]
    nm, P = site.names, site.params
    onehot = torch.zeros(K, U, dtype=torch.float64)
    onehot[torch.arange(K), uu] = c
    xhat = None
    if site.kind == "conv_ln":
        W = P["weight"].reshape(U, -1)
        y = (Xc @ W.t() + P["bias"]).requires_grad_(True)
        z = F.layer_norm(y, (U,), P["gamma"], P["beta"], 1e-5)
        DY, = torch.autograd.grad(z, y, grad_outputs=onehot)        # rows are independent: row k = c_k dz[k, u_k] / dy[k, :]
        with torch.no_grad():
            yk = y.detach()
            xhat = ((yk - yk.mean(1, keepdim=True)) / torch.sqrt(yk.var(1, unbiased=False, keepdim=True) + 1e-5))[torch.arange(K), uu]
    else:
        DY = onehot
    RW = R[nm["weight"]].reshape(U, -1)
    G = (DY @ DY.t()) * (Xc @ Xc.t())                                # Gram matrix of the rank-one directions DY_k (x) x_k
    rhs = ((DY @ RW) * Xc).sum(dim=1)
    s = _solve(G, rhs)
    mag = DY.abs().amax(dim=1) * Xc.abs().amax(dim=1)
    s0 = _check_s(site, s, mag, bounds[nm["weight"]], il)
    SD = s0[:, None] * DY
    R[nm["weight"]] -= (SD.t() @ Xc).reshape(R[nm["weight"]].shape)
    R[nm["bias"]] -= SD.sum(dim=0)
    if xhat is not None:
        R[nm["gamma"]].index_add_(0, uu, -s0 * c * xhat)
        R[nm["beta"]].index_add_(0, uu, -s0 * c)
    return nU, share, K, int(s0.sum())


def assert_grads_match_up_to_relu_branches(got, want, sites, tol_rel, tol_abs, floor_only=(), label="", expect_no_branches=False):
    """got / want: {parameter name: gradient} of ONE network (want = the float64 oracle's; every name of `want` is compared).
    sites: the network's ReLU sites, deeper ones FIRST in the order loss -> input (each is solved on its own weight, which flips of
    sites upstream of it do not touch), the bag-fed site last. `floor_only`: name suffixes whose true gradient is exactly 0 (compared
    at tol_abs alone). Prints and returns, per site: len(U), share, candidates solved, branches taken the other way; per parameter the
    largest residual before and after accounting, relative to the bound's scale."""
    R, bounds, scales = {}, {}, {}
    for k, w in want.items():
        w = w.detach().double()
        g = got[k].detach().double().cpu().reshape(w.shape)
        R[k] = g - w
        scales[k] = float(w.abs().max())
        bounds[k] = tol_abs if any(k.endswith(sfx) for sfx in floor_only) else tol_rel * scales[k] + tol_abs
    before = {k: float(v.abs().max()) for k, v in R.items()}
    report = {"sites": {}, "params": {}}
    for site in sites:
        nU, share, K, taken = _account(site, R, bounds)
        report["sites"][site.name] = dict(undecided=nU, share=share, delta=site.delta, solved=K, taken=taken)
        print(f"[boundary] {label} site {site.name}: delta {site.delta:.3e}  undecided {nU} ({share:.2e} of {site.Z.numel()})  "
              f"solved {K}  taken the other way {taken}")
        if expect_no_branches:
            assert taken == 0, (label, site.name, taken)
    bad = []
    for k in R:
        after = float(R[k].abs().max())
        sc = scales[k] + 1e-300
        report["params"][k] = dict(before=before[k], after=after, scale=scales[k], bound=bounds[k])
        print(f"[boundary] {label} {k}: scale {scales[k]:.3e}  residual before {before[k]:.3e} ({before[k] / sc:.2e} rel)  "
              f"after {after:.3e} ({after / sc:.2e} rel)  bound {bounds[k]:.3e}")
        if not after <= bounds[k]:
            bad.append((k, after, bounds[k]))
    assert not bad, f"{label}: gradients outside the bound after branch accounting: {bad}"
    return report


# ------------------------------------------------------------------------------------------------------------------------------
# the sites of one training step from the oracle's taps (oracle.advmil_oracle.update_disc / update_gen, taps = {})
# ------------------------------------------------------------------------------------------------------------------------------
def _tap(lst, site):
    ts = [t for t in lst if t["site"] == site]
    assert len(ts) == 1, (site, [t["site"] for t in lst])
    return ts[0]


def _groups(taps, nb, passes, site):
    """Per bag: the taps of `site` in the bag's forwards, merged into one group where they hold the same Z."""
    out = []
    for i in range(nb):
        ts = [_tap(taps[(i, w)], site) for w in passes if (i, w) in taps]
        if len(ts) == 2 and torch.equal(ts[0]["Z"].detach(), ts[1]["Z"].detach()):
            out.append(ts)
        else:
            out.extend([t] for t in ts)
    return out


def cluster_first_layer(taps, ext, n, width):
    """DeepAttMISL's first layer is tapped per cluster (oracle.deep_att_misl): (Z, dL/dReLU_out) back in patch order."""
    z, g = torch.zeros(n, width, dtype=torch.float64), torch.zeros(n, width, dtype=torch.float64)
    for c in range(8):
        rows = (ext.reshape(-1) == c).nonzero().reshape(-1)
        if rows.numel():
            t_ = _tap(taps, f"phis.0/{c}")
            z[rows], g[rows] = t_["Z"].detach().double(), t_["Y"].grad.double()
    return z, g


def generator_first_layer(kind, taps_per_bag, bags, X, PG):
    """Arguments of bag_fed_site (all but the arithmetic) for the generator's first layer over the bags of a step."""
    if kind == "abmil":
        z = torch.cat([_tap(t, "attention_net.0")["Z"].detach() for t in taps_per_bag])
        g = torch.cat([_tap(t, "attention_net.0")["Y"].grad for t in taps_per_bag])
        return ("G attention_net.0", X, z, g, PG, {"weight": "backbone.attention_net.0.weight", "bias": "backbone.attention_net.0.bias"})
    if kind == "cluster":
        width = PG["backbone.phis.0.bias"].shape[0]
        zg = [cluster_first_layer(t, b[1], b[0].shape[1], width) for t, b in zip(taps_per_bag, bags)]
        return ("G phis.0", X, torch.cat([a for a, _ in zg]), torch.cat([b_ for _, b_ in zg]), PG,
                {"weight": "backbone.phis.0.weight", "bias": "backbone.phis.0.bias"})
    if kind != "patch":
        return None                               # (PatchGCN: parity unpinned, oracle/advmil_oracle.py; no site described)
    e = "backbone.patch_embedding_layer."
    z = torch.cat([_tap(t, "patch_embedding_layer")["Z"].detach()[0] for t in taps_per_bag])
    g = torch.cat([_tap(t, "patch_embedding_layer")["Y"].grad[0] for t in taps_per_bag])
    return ("G patch_embedding", X, z, g, PG, {"weight": e + "conv.weight", "bias": e + "conv.bias", "gamma": e + "norm.weight", "beta": e + "norm.bias"})


def disc_embedding(taps_per_bag, X, PD):
    """... and for the discriminator's patch embedding; taps_per_bag[i] = the tap lists of bag i's forwards (fake, real): they hold the
    same Z, so their dL/dReLU_out are added."""
    e = "net_pair_one.embedding."
    z = torch.cat([_tap(ts[0], "embedding")["Z"].detach()[0] for ts in taps_per_bag])
    g = torch.cat([sum(_tap(t, "embedding")["Y"].grad[0] for t in ts) for ts in taps_per_bag])
    return ("D embedding", X, z, g, PD, {"weight": e + "conv.weight", "bias": e + "conv.bias", "gamma": e + "norm.weight", "beta": e + "norm.bias"})


def step_sites(kind, tD, tG, bags, PG, PD, deep=True):
    """-> (D's deeper sites, D's bag-fed site as bag_fed_site arguments, G's deeper sites, G's bag-fed site arguments); the deeper
    sites in the order loss -> input. bags = [(x[1, N, C], x_ext, y)], PG / PD the fp32 parameters."""
    nb = len(bags)
    LD, LG = tD.pop("__params__"), tG.pop("__params__")
    X = torch.cat([b[0].reshape(-1, b[0].shape[-1]) for b in bags])
    sD = sG = []
    if deep:
        sD = [deep_site("D " + s, _groups(tD, nb, ("fake", "real"), s), LD, w) for s, w in
              (("net_pair_two.1.0", "net_pair_two.1.0.weight"), ("net_pair_two.0.0", "net_pair_two.0.0.weight"),
               ("fc2.0", "net_pair_one.fc2.0.weight"), ("fc1.0", "net_pair_one.fc1.0.weight"))]
        sG = [deep_site("G MLPs.0", _groups(tG, nb, ("gen",), "MLPs.0"), LG, "MLPs.0.0.weight")]
        if kind == "abmil":
            sG.append(deep_site("G rho.0", _groups(tG, nb, ("gen",), "rho.0"), LG, "backbone.rho.0.weight"))
        elif kind == "cluster":
            sG.append(deep_site("G attention_net.0", _groups(tG, nb, ("gen",), "attention_net.0"), LG, "backbone.attention_net.0.weight"))
        else:
            sG.append(deep_site("G linear1", _groups(tG, nb, ("gen",), "linear1"), LG, "backbone.patch_encoder_layer.layers.0.linear1.weight"))
    bD = disc_embedding([[tD[(i, w)] for w in ("fake", "real") if (i, w) in tD] for i in range(nb)], X, PD)
    bG = generator_first_layer(kind, [tG[(i, "gen")] for i in range(nb)], bags, X, PG)
    return sD, bD, sG, bG
