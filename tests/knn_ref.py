"""The oracle of the k-NN graph construction (advmil_amd/csrc/knn.hip, advmil_amd/wsigraph.py): numpy only, brute force per bag.

Definition (the one the kernels implement): row i's neighbours are the k rows of its own bag, other than i itself, that come first in
ascending (squared distance, row id); ids are bag-local. Self is removed BY INDEX, so a duplicate of row i at distance 0 is a
neighbour. Spatial distances are int64 (exact for |coordinate| < 2^30), latent distances float64 of the fp32 values. The latent
matrix is formed as n_i + n_j - 2 <x_i, x_j> in float64: exact on small-integer features, and ~1e-13 relative on real-valued ones, eight
orders below the tolerance of the tests that use it (the direct form needs N^2 C doubles)."""
import numpy as np


def bag_bounds(n_rows, lens=None):
    lens = [n_rows] if lens is None else [int(v) for v in lens]
    assert sum(lens) == n_rows
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [(int(offs[b]), int(offs[b + 1])) for b in range(len(lens))]


def dist2_spatial(xy):
    xy = np.asarray(xy).astype(np.int64)
    d = xy[:, None, :] - xy[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]


def dist2_latent(x):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = (x * x).sum(axis=1)
    return n[:, None] + n[None, :] - 2.0 * (x @ x.T)


def rank_rows(D, keep):
    """-> (ids[n, keep], d2[n, keep]): per row the first `keep` other rows in ascending (D, id); -1 / the type's maximum where the bag is short."""
    n = D.shape[0]
    ids = np.broadcast_to(np.arange(n), (n, n))
    order = np.lexsort((ids, D), axis=-1)                      # last key is the primary one: D, then id
    order = order[order != np.arange(n)[:, None]].reshape(n, n - 1)
    big = np.iinfo(D.dtype).max if np.issubdtype(D.dtype, np.integer) else np.finfo(np.float32).max
    out_i = np.full((n, keep), -1, dtype=np.int64)
    out_d = np.full((n, keep), big, dtype=D.dtype)
    m = min(keep, n - 1)
    out_i[:, :m] = order[:, :m]
    out_d[:, :m] = np.take_along_axis(D, order[:, :m], axis=1)
    return out_i, out_d


def knn(points, k, lens=None, latent=False, extra=0):
    """-> dict(nbr [N, k] int32 bag-local, dist2 [N, k], more_nbr / more_dist2 [N, k + extra], D: per-bag distance matrices)."""
    points = np.asarray(points)
    N = points.shape[0]
    ids, ds, mats = [], [], []
    for lo, hi in bag_bounds(N, lens):
        D = dist2_latent(points[lo:hi]) if latent else dist2_spatial(points[lo:hi])
        i, d = rank_rows(D, k + extra)
        ids.append(i), ds.append(d), mats.append(D)
    ids, ds = np.concatenate(ids), np.concatenate(ds)
    return dict(nbr=ids[:, :k].astype(np.int32), dist2=ds[:, :k], more_nbr=ids, more_dist2=ds, D=mats)
