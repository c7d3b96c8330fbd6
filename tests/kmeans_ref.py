"""The oracle of the batched k-means (advmil_amd/csrc/kmeans.hip, advmil_amd/wsicluster.py): numpy float64, one bag at a time.

Definition (the one the kernels and the Python loop implement):
  assign   label_i = the centre j with the smallest ||x_i - c_j||^2, ties to the LOWEST j; dist2_i = that distance.
  update   centre j = the mean of the rows that carry label j; a cluster WITHOUT rows keeps its previous centre and has count 0 (sklearn
           relocates it to the farthest point; the reference backbone handles an empty cluster, model/backbone.py:114-115).
  loop     per iteration assign, then update. Stop when no label changed since the previous assign (labels start as -1); otherwise stop
           when shift2 = sum_j ||new_j - old_j||^2 <= tol * mean_c(var_i x_ic). After a stop that was not "no label changed" (and after
           max_iter) the labels are assigned once more against the returned centres. This is sklearn 1.7's lloyd loop
           (_kmeans_single_lloyd) and gives its iteration counts and labels with KMeans(init=<array>, n_init=1, algorithm="lloyd").
  seeding  plain D^2 seeding, one trial per pick, driven by K given uniforms u: first centre = row floor(u_0 n); pick p = the first row
           whose inclusive prefix sum of min_j dist2 exceeds u_p * total, clamped to the last row; total == 0: row floor(u_p n).
           (sklearn's greedy multi-trial k-means++ and its RNG are NOT reproduced.)
Distances are formed as n_i + c_j - 2 <x_i, c_j> in float64: exact on small-integer data, ~1e-13 relative otherwise."""
import numpy as np


def dist2(x, cent):
    x, cent = np.asarray(x, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    return np.maximum((x * x).sum(axis=1)[:, None] + (cent * cent).sum(axis=1)[None, :] - 2.0 * (x @ cent.T), 0.0)


def assign(x, cent):
    """-> (labels int32 [n], dist2 float64 [n], D float64 [n, K]); np.argmin returns the first minimum: ties to the lowest j."""
    D = dist2(x, cent)
    lab = np.argmin(D, axis=1)
    return lab.astype(np.int32), D[np.arange(len(lab)), lab], D


def update(x, labels, cent):
    """-> (cent_new float64 [K, C], count int32 [K], shift2 float64, sums float64 [K, C])."""
    x, cent = np.asarray(x, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    K = cent.shape[0]
    new, count, sums = cent.copy(), np.zeros(K, dtype=np.int32), np.zeros_like(cent)
    for j in range(K):
        m = labels == j
        count[j] = int(m.sum())
        if count[j]:
            sums[j] = x[m].sum(axis=0)
            new[j] = sums[j] / count[j]
    return new, count, float(((new - cent) ** 2).sum()), sums


def tolerance(x, tol):
    return float(tol) * float(np.var(np.asarray(x, dtype=np.float64), axis=0).mean())


def lloyd(x, init, max_iter=300, tol=1e-4):
    """-> dict(labels, centers, n_iter, inertia, count)"""
    x = np.asarray(x, dtype=np.float64)
    cent = np.array(init, dtype=np.float64)
    tol_abs = tolerance(x, tol)
    old = np.full(x.shape[0], -1, dtype=np.int32)
    strict, n_iter = False, 0
    for it in range(max_iter):
        lab, d2, _ = assign(x, cent)
        cent, count, shift2, _ = update(x, lab, cent)
        n_iter = it + 1
        if np.array_equal(lab, old):
            strict = True
            break
        if shift2 <= tol_abs:
            break
        old = lab
    if not strict:
        lab, d2, _ = assign(x, cent)
    count = np.bincount(lab, minlength=cent.shape[0]).astype(np.int32)
    return dict(labels=lab, centers=cent, n_iter=n_iter, inertia=float(d2.sum()), count=count)


def seed_rows(x, K, u):
    """The rows D^2 seeding picks for the uniforms u[0..K-1] -> list of K row indices."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    floor_row = lambda v: min(int(np.floor(float(v) * n)), n - 1)      # noqa: E731
    rows = [floor_row(u[0])]
    mind = dist2(x, x[rows[0]][None, :])[:, 0]
    for p in range(1, K):
        prefix = np.cumsum(mind)
        total = prefix[-1]
        if total == 0.0:
            r = floor_row(u[p])
        else:
            r = min(int(np.searchsorted(prefix, float(u[p]) * total, side="right")), n - 1)      # the first prefix > u_p * total
        rows.append(r)
        mind = np.minimum(mind, dist2(x, x[r][None, :])[:, 0])
    return rows


def kmeans(x, K, lens=None, init=None, u=None, max_iter=300, tol=1e-4):
    """Per bag of `lens`: init[b] ([K, C]) or the seeding rule with the uniforms u[b] -> list of lloyd() results (plus 'rows')."""
    x = np.asarray(x)
    lens = [x.shape[0]] if lens is None else [int(v) for v in lens]
    assert sum(lens) == x.shape[0]
    out, lo = [], 0
    for b, n in enumerate(lens):
        xb = x[lo:lo + n]
        rows = None
        if init is not None:
            c0 = np.asarray(init[b] if np.asarray(init).ndim == 3 else init)
        else:
            rows = seed_rows(xb, K, u[b])
            c0 = np.asarray(xb, dtype=np.float64)[rows]
        r = lloyd(xb, c0, max_iter, tol)
        r["rows"] = rows
        out.append(r)
        lo += n
    return out
