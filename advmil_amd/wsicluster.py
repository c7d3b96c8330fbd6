"""Patch cluster ids built on the device: the `ext` of `bcb_mode: cluster` (DeepAttMISL) from patch features.

The reference gets them offline from tools/deepattnmisl_cluster.py: all slides of a patient concatenated,
sklearn.cluster.KMeans(n_clusters=8, random_state=42).fit_predict on the CPU, written as <pid>.npy and loaded as torch.Tensor(cids)
(dataset/PatchWSI.py:85-94). Here the same Lloyd iteration runs on the device, for any number of patients at once: one assign launch
(ops.kmeans_assign: bf16x3 contraction of the rows' operand planes with the bag's centres) and one update launch (ops.kmeans_update:
fixed-order segmented sums) per iteration over the whole slab, pinned to a float64 oracle (tests/kmeans_ref.py) and to recorded sklearn
runs (tests/golden/kmeans_v1.npz).

    ids = cluster_patient([feats_slide0, feats_slide1])          # float32 [sum N], what PatchWSI hands DeepAttMISL
    ids_per_patient = cluster_patients([[...], [...], ...])      # all patients as one slab
    labels, info = kmeans(feats, 8, init=centres, return_info=True)

The iteration and its stopping rule are sklearn 1.7's (`KMeans(init=<array>, n_init=1, algorithm="lloyd")`): assign, update; a bag stops
when no label changed since the previous assign, else when the squared centre shift is <= tol * mean_c(var_i x_ic); after a stop of
the second kind (or max_iter) the labels are assigned once more against the returned centres. A stopped bag is masked out of the later
launches, so the batched run of several bags returns for each bag the bits it gets alone.

Seeding. init="greedy-k-means++" is sklearn's: every pick draws L = 2 + int(ln K) rows from the D^2 distribution and keeps the one that
lowers the potential most, the uniforms come from sklearn's own stream (sklearn_draws: one numpy RandomState(seed) per bag, as the
reference runs a fresh KMeans(random_state=42) per patient), and n_init > 1 keeps per bag the run sklearn keeps. One pick is two
launches over the whole slab (ops.kmeans_seed_greedy: 1 + 2 K launches for any number of bags, nothing read back). On data whose
distances are exact the rows are sklearn.cluster.kmeans_plusplus's index for index, and the labels KMeans(K, random_state=seed)'s
(tests/golden/kmeans_greedy_v1.npz). init="k-means++", the default, stays what it was: plain D^2 seeding, one trial per pick, on the
project's counter RNG -- a valid k-means partition, not sklearn's partition for random_state=42.

NOT reproduced: the relocation of an empty cluster (an empty cluster keeps its centre and shows as info["count"] == 0; the backbone
takes an empty cluster; seeds that are data points make it rare), and sklearn's float32 arithmetic on float32 input (distances here
are bf16x3 products of the raw rows, sklearn centres the rows and works in the input's type: the recorded runs are of float64 images, and
a draw or a potential closer to a tie than the distance bound may fall the other way)."""
import numpy as np
import torch

from . import ops, synth


def seeding_uniforms(seed, n_rows, n_cols, n_clusters):
    """The K uniforms that drive the D^2 seeding of a bag of n_rows x n_cols: a function of the seed and the bag's shape, not of the
    bag's position in a batch."""
    return synth.uniform01(synth.stream_key(seed, ("kmeans++", int(n_rows), int(n_cols), int(n_clusters)).__repr__()), int(n_clusters))


def _floor_row(u, n):
    return min(int(np.floor(float(u) * n)), n - 1)


def seed_rows(X, K, seed, seg=None, planes=None):
    """Plain D^2 seeding -> rows[nseg, K] int64 (bag-local, device). The first centre of a bag of n rows is row floor(u_0 n); pick p is
    the first row whose float64 inclusive prefix sum of min_j dist2 exceeds u_p * total, clamped to the last row (total == 0: row
    floor(u_p n)). The min-distance pass is ops.kmeans_assign with K = 1 against the newest centre; scan and search are torch glue."""
    N, C = int(X.shape[0]), int(X.shape[1])
    lens = [N] if seg is None else seg.lens
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nseg = len(lens)
    planes = planes if planes is not None else ops.kmeans_planes(X)
    us = [seeding_uniforms(seed, n, C, K) for n in lens]
    rows = torch.empty(nseg, K, dtype=torch.int64, device=X.device)
    rows[:, 0] = torch.tensor([_floor_row(us[b][0], lens[b]) for b in range(nseg)], dtype=torch.int64).to(X.device)
    base = torch.as_tensor(offs[:-1]).to(X.device)
    mind, norms = None, None
    for p in range(1, K):
        cent = X.index_select(0, base + rows[:, p - 1]).unsqueeze(1)                     # [nseg, 1, C]
        _, d2, norms = ops.kmeans_assign(X, cent, seg, return_dist=True, planes=planes, norms=norms)
        mind = d2 if mind is None else torch.minimum(mind, d2)
        for b in range(nseg):
            n = lens[b]
            prefix = torch.cumsum(mind[offs[b]:offs[b + 1]].double(), dim=0)
            total = prefix[-1]
            u = float(us[b][p])
            pick = torch.searchsorted(prefix, (u * total).reshape(1), right=True).clamp(max=n - 1)[0]
            rows[b, p] = torch.where(total == 0, torch.full_like(pick, _floor_row(u, n)), pick)
    return rows


GREEDY = "greedy-k-means++"


def sklearn_draws(random_state, n_rows, n_clusters, n_init=1):
    """What sklearn's KMeans(n_clusters, random_state=random_state, n_init=n_init) draws while it seeds a bag of n_rows, from ONE
    np.random.RandomState(random_state): per init, in order, choice(n_rows, p=full(1 / n_rows)) for the first centre, then K - 1 times
    uniform(size=L), L = 2 + int(ln K) (the Lloyd iteration draws nothing, so consecutive inits continue the stream).
    -> (first int64 [n_init], u float64 [n_init, K - 1, L])"""
    n_rows, K, n_init = int(n_rows), int(n_clusters), int(n_init)
    L = ops.kmeans_seed_trials(K)
    rs = np.random.RandomState(random_state)
    first, u = np.zeros(n_init, dtype=np.int64), np.zeros((n_init, K - 1, L), dtype=np.float64)
    p = np.full(n_rows, 1.0 / n_rows)
    for i in range(n_init):
        first[i] = rs.choice(n_rows, p=p)
        for k in range(K - 1):
            u[i, k] = rs.uniform(size=L)
    return first, u


def _greedy_draws(lens, K, random_state, n_init, device):
    """The draws of every bag (each from its own fresh stream) on the device -> (first int32 [n_init, nseg], u [n_init, nseg, K - 1, L])."""
    per = [sklearn_draws(random_state, n, K, n_init) for n in lens]
    first = np.stack([f for f, _ in per], axis=1).astype(np.int32)
    u = np.stack([v for _, v in per], axis=1)
    return torch.from_numpy(first).to(device), torch.from_numpy(u).to(device)


def seed_rows_greedy(X, K, random_state, seg=None, planes=None, init_index=0):
    """sklearn's greedy k-means++ -> rows[nseg, K] int64 (bag-local, device): what sklearn.cluster.kmeans_plusplus(x_b, K,
    random_state=random_state) returns as indices for every bag b, where the distances are exact (module docstring). init_index = i:
    the seeds of the (i + 1)-th init of a KMeans with n_init > i. All bags in 1 + 2 K launches (ops.kmeans_seed_greedy)."""
    N = int(X.shape[0])
    ops._kmeans_check("seed_rows_greedy", N, K, seg)
    if isinstance(init_index, bool) or not isinstance(init_index, int) or init_index < 0:
        raise ValueError(f"advmil_amd: seed_rows_greedy: init_index = {init_index!r}, must be a non-negative integer")
    ops._chk(X, "X")
    first, u = _greedy_draws([N] if seg is None else seg.lens, K, random_state, init_index + 1, X.device)
    return ops.kmeans_seed_greedy(X, K, first[init_index], u[init_index], seg, planes)


def _same_clustering(a, b, K):
    """sklearn's _is_same_clustering: every label of a maps to one label of b."""
    return all(len(np.unique(b[a == j])) <= 1 for j in range(K))


def kmeans(feats, n_clusters=8, init="k-means++", seed=42, max_iter=300, tol=1e-4, seg=None, return_info=False, n_init=1):
    """Lloyd's k-means of every bag of feats[N, C] (fp32, device; bags by `seg`, an ops.Segments, None = one bag).
    init: a [K, C] (one bag) or [nseg, K, C] tensor of starting centres, "k-means++" (plain D^2 seeding from `seed`, see seed_rows;
    not sklearn's greedy seeding, not its RNG) or "greedy-k-means++" (sklearn's seeding from sklearn's stream for random_state = seed,
    see seed_rows_greedy). n_init > 1 (greedy seeding only): the inits run one after another, and per bag a later run replaces the best
    so far when its inertia is lower and its labels are not the best's up to a relabelling, as KMeans.fit does.
    -> labels int32 [N] (bag-local cluster ids), and with return_info also
    dict(centers fp32 [nseg, K, C], n_iter [nseg], inertia float64 [nseg] = sum of dist2, count int32 [nseg, K])."""
    if feats.dim() != 2:
        raise ValueError(f"advmil_amd: kmeans: features must be [N, C], got {tuple(feats.shape)}")
    N, C = int(feats.shape[0]), int(feats.shape[1])
    K = n_clusters
    ops._kmeans_check("kmeans", N, K, seg)
    nseg = 1 if seg is None else seg.nseg
    lens = [N] if seg is None else seg.lens
    if isinstance(init, torch.Tensor):
        if tuple(init.shape) not in ((nseg, K, C),) + (((K, C),) if nseg == 1 else ()):
            raise ValueError(f"advmil_amd: kmeans: init must be [{nseg}, {K}, {C}]" + (f" or [{K}, {C}]" if nseg == 1 else "")
                             + f", got {tuple(init.shape)}")
    elif init not in ("k-means++", GREEDY):
        raise ValueError(f"advmil_amd: kmeans: init = {init!r}, must be a tensor of centres or 'k-means++'")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 1:
        raise ValueError(f"advmil_amd: kmeans: max_iter = {max_iter!r}, must be a positive integer")
    if isinstance(n_init, bool) or not isinstance(n_init, int) or n_init < 1:
        raise ValueError(f"advmil_amd: kmeans: n_init = {n_init!r}, must be a positive integer")
    if n_init > 1 and not (isinstance(init, str) and init == GREEDY):
        raise ValueError(f"advmil_amd: kmeans: n_init = {n_init} needs init = {GREEDY!r}: every other init gives the same run again")
    ops._chk(feats, "feats")
    dev = feats.device
    plain = C % 32 == 0 and feats.is_contiguous()
    X = feats.detach() if plain else ops.kmeans_pad(feats.detach()).contiguous()
    planes = ops.kmeans_planes(feats) if plain else ops.split_planes(X)
    offs = [0, N] if seg is None else seg.offsets
    # the bag constant of the shift test, once, in float64
    tol_abs = [float(tol) * float(feats[offs[b]:offs[b + 1]].double().var(dim=0, unbiased=False).mean()) for b in range(nseg)]
    base = torch.as_tensor(np.asarray(offs[:-1], dtype=np.int64)).to(dev)
    rows_to_centres = lambda rows: X.index_select(0, (base[:, None] + rows).reshape(-1)).reshape(nseg, K, X.shape[1]).contiguous()      # noqa: E731
    if isinstance(init, torch.Tensor):
        cents = [ops.kmeans_pad(ops._chk(init, "init").detach().reshape(nseg, K, C)).contiguous().clone()]
    elif init == GREEDY:
        first, u = _greedy_draws(lens, K, seed, n_init, dev)
        cents = [rows_to_centres(ops.kmeans_seed_greedy(X, K, first[i], u[i], seg, planes)) for i in range(n_init)]
    else:
        cents = [rows_to_centres(seed_rows(X, K, seed, seg, planes))]
    best = None
    for cent in cents:
        run = _lloyd(X, planes, cent, K, seg, offs, tol_abs, max_iter)
        if best is None:
            best = run
            continue
        # per bag: sklearn's rule, on the host (n_init > 1 is the rare call)
        lab_new, lab_old = run[0].cpu().numpy(), best[0].cpu().numpy()
        in_new, in_old = run[4].cpu().numpy(), best[4].cpu().numpy()
        for b in range(nseg):
            sl = slice(offs[b], offs[b + 1])
            if in_new[b] < in_old[b] and not _same_clustering(lab_new[sl], lab_old[sl], K):
                best[0][sl], best[1][b], best[2][b], best[3][b], best[4][b] = run[0][sl], run[1][b], run[2][b], run[3][b], run[4][b]
    labels, cent, n_iter, count, inertia = best
    if not return_info:
        return labels
    return labels, dict(centers=cent[:, :, :C], n_iter=torch.from_numpy(n_iter), inertia=inertia, count=count)


def _lloyd(X, planes, cent, K, seg, offs, tol_abs, max_iter):
    """The iteration from the centres cent[nseg, K, C] (updated in place) -> [labels, cent, n_iter (host), count, inertia float64 [nseg]]."""
    N, dev, nseg = int(X.shape[0]), X.device, len(offs) - 1
    labels = torch.full((N,), -1, dtype=torch.int32, device=dev)
    dist2 = torch.zeros(N, dtype=torch.float32, device=dev)
    count = torch.zeros(nseg, K, dtype=torch.int32, device=dev)
    active_h = np.ones(nseg, dtype=np.int32)
    again_h = np.zeros(nseg, dtype=np.int32)                 # bags whose stop was not "no label changed": one more assign
    n_iter = np.zeros(nseg, dtype=np.int64)
    norms = None
    for it in range(max_iter):
        active = torch.from_numpy(active_h.copy()).to(dev)
        _, _, changed, norms = ops.kmeans_assign(X, cent, seg, active, labels, return_dist=dist2, return_changed=True, planes=planes, norms=norms)
        _, _, shift2 = ops.kmeans_update(X, labels, cent, seg, active, out=cent, count=count)
        back = torch.stack([changed.double(), shift2.double()]).cpu().numpy()       # the one readback of the iteration
        for b in np.nonzero(active_h)[0]:
            n_iter[b] = it + 1
            if back[0, b] == 0:
                active_h[b] = 0
            elif back[1, b] <= tol_abs[b]:
                active_h[b], again_h[b] = 0, 1
        if not active_h.any():
            break
    again_h |= active_h                                       # max_iter reached
    if again_h.any():
        ops.kmeans_assign(X, cent, seg, torch.from_numpy(again_h).to(dev), labels, return_dist=dist2, planes=planes, norms=norms)
        count = torch.stack([torch.bincount(labels[offs[b]:offs[b + 1]].long(), minlength=K) for b in range(nseg)]).to(torch.int32)
    inertia = torch.stack([dist2[offs[b]:offs[b + 1]].double().sum() for b in range(nseg)])
    return [labels, cent, n_iter, count, inertia]


def _patient_rows(slide_feats_list, what):
    slides = list(slide_feats_list)
    if not slides:
        raise ValueError(f"advmil_amd: {what}: a patient without slides")
    return slides[0] if len(slides) == 1 else torch.cat(slides, dim=0)


def cluster_patient(slide_feats_list, n_clusters=8, seed=42, init="k-means++", n_init=1):
    """The cluster ids of one patient: the slides' patch features ([N_s, C] fp32 each, device) concatenated as the reference does,
    k-means++ seeded from `seed` -> float32 [sum N_s], ids in [0, n_clusters): the `ext` DeepAttMISL takes (PatchWSI hands floats over).
    init="greedy-k-means++" (with n_init): sklearn's seeding, the ids of the reference's KMeans(n_clusters, random_state=seed) -- see kmeans."""
    return kmeans(_patient_rows(slide_feats_list, "cluster_patient"), n_clusters, init=init, seed=seed, n_init=n_init).to(torch.float32)


def cluster_patients(list_of_slide_feats_lists, n_clusters=8, seed=42, init="k-means++", n_init=1):
    """Several patients at once: their rows form one slab, every iteration is ONE assign and ONE update launch over all of them (and
    with init="greedy-k-means++" every pick of the seeding two). -> one float32 id tensor per patient, bit-identical to cluster_patient
    of that patient with the same arguments."""
    pats = [_patient_rows(s, "cluster_patients") for s in list_of_slide_feats_lists]
    if not pats:
        raise ValueError("advmil_amd: cluster_patients: no patient")
    seg = ops.Segments([int(p.shape[0]) for p in pats], pats[0].device)
    ids = kmeans(torch.cat(pats, dim=0), n_clusters, init=init, seed=seed, seg=seg, n_init=n_init).to(torch.float32)
    return [ids[seg.offsets[b]:seg.offsets[b + 1]] for b in range(seg.nseg)]
