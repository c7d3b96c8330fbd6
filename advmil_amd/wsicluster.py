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

NOT reproduced: sklearn's greedy multi-trial k-means++ and its RNG (init="k-means++" here is plain D^2 seeding, one trial per pick, on
the project's counter RNG -- the ids are a valid k-means partition, not sklearn's partition for random_state=42), n_init > 1, and the
relocation of an empty cluster (an empty cluster keeps its centre; the backbone takes an empty cluster)."""
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


def kmeans(feats, n_clusters=8, init="k-means++", seed=42, max_iter=300, tol=1e-4, seg=None, return_info=False):
    """Lloyd's k-means of every bag of feats[N, C] (fp32, device; bags by `seg`, an ops.Segments, None = one bag).
    init: a [K, C] (one bag) or [nseg, K, C] tensor of starting centres, or "k-means++" (plain D^2 seeding from `seed`, see seed_rows;
    not sklearn's greedy seeding, not its RNG). -> labels int32 [N] (bag-local cluster ids), and with return_info also
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
    elif init != "k-means++":
        raise ValueError(f"advmil_amd: kmeans: init = {init!r}, must be a tensor of centres or 'k-means++'")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 1:
        raise ValueError(f"advmil_amd: kmeans: max_iter = {max_iter!r}, must be a positive integer")
    ops._chk(feats, "feats")
    dev = feats.device
    plain = C % 32 == 0 and feats.is_contiguous()
    X = feats.detach() if plain else ops.kmeans_pad(feats.detach()).contiguous()
    planes = ops.kmeans_planes(feats) if plain else ops.split_planes(X)
    offs = [0, N] if seg is None else seg.offsets
    # the bag constant of the shift test, once, in float64
    tol_abs = [float(tol) * float(feats[offs[b]:offs[b + 1]].double().var(dim=0, unbiased=False).mean()) for b in range(nseg)]
    if isinstance(init, torch.Tensor):
        cent = ops.kmeans_pad(ops._chk(init, "init").detach().reshape(nseg, K, C)).contiguous().clone()
    else:
        rows = seed_rows(X, K, seed, seg, planes)
        base = torch.as_tensor(np.asarray(offs[:-1], dtype=np.int64)).to(dev)
        cent = X.index_select(0, (base[:, None] + rows).reshape(-1)).reshape(nseg, K, X.shape[1]).contiguous()
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
    if not return_info:
        return labels
    inertia = torch.stack([dist2[offs[b]:offs[b + 1]].double().sum() for b in range(nseg)])
    return labels, dict(centers=cent[:, :, :C], n_iter=torch.from_numpy(n_iter), inertia=inertia, count=count)


def _patient_rows(slide_feats_list, what):
    slides = list(slide_feats_list)
    if not slides:
        raise ValueError(f"advmil_amd: {what}: a patient without slides")
    return slides[0] if len(slides) == 1 else torch.cat(slides, dim=0)


def cluster_patient(slide_feats_list, n_clusters=8, seed=42):
    """The cluster ids of one patient: the slides' patch features ([N_s, C] fp32 each, device) concatenated as the reference does,
    k-means++ seeded from `seed` -> float32 [sum N_s], ids in [0, n_clusters): the `ext` DeepAttMISL takes (PatchWSI hands floats over)."""
    return kmeans(_patient_rows(slide_feats_list, "cluster_patient"), n_clusters, seed=seed).to(torch.float32)


def cluster_patients(list_of_slide_feats_lists, n_clusters=8, seed=42):
    """Several patients at once: their rows form one slab, every iteration is ONE assign and ONE update launch over all of them.
    -> one float32 id tensor per patient, bit-identical to cluster_patient of that patient."""
    pats = [_patient_rows(s, "cluster_patients") for s in list_of_slide_feats_lists]
    if not pats:
        raise ValueError("advmil_amd: cluster_patients: no patient")
    seg = ops.Segments([int(p.shape[0]) for p in pats], pats[0].device)
    ids = kmeans(torch.cat(pats, dim=0), n_clusters, seed=seed, seg=seg).to(torch.float32)
    return [ids[seg.offsets[b]:seg.offsets[b + 1]] for b in range(seg.nseg)]
