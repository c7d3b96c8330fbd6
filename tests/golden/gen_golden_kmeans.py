#!/usr/bin/env python3
"""Recorded sklearn runs for the k-means tests: tests/golden/kmeans_v1.npz.

For every case of tests/kmeans_cases.py::golden_cases (data regenerated from the counter RNG, so only results are stored) the labels,
centres, n_iter_ and inertia_ of

    sklearn.cluster.KMeans(n_clusters=K, init=<the stated init>, n_init=1, algorithm="lloyd", tol=1e-4, max_iter=300).fit(x)

on the float64 image of the fp32 features (the oracle tests/kmeans_ref.py is float64), plus the sklearn version. Runs where sklearn is
installed (1.7.2 when the fixture was written); the tests read the fixture and need no sklearn.
Usage:  python tests/golden/gen_golden_kmeans.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import kmeans_cases as CASES  # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import KMeans
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (x, init, K) in CASES.golden_cases().items():
        km = KMeans(n_clusters=K, init=init.astype(np.float64), n_init=1, algorithm="lloyd", tol=1e-4, max_iter=300).fit(x.astype(np.float64))
        out[name + "_labels"] = km.labels_.astype(np.int8)
        out[name + "_centers"] = km.cluster_centers_.astype(np.float64)
        out[name + "_n_iter"] = np.array(km.n_iter_, dtype=np.int64)
        out[name + "_inertia"] = np.array(km.inertia_, dtype=np.float64)
        print(name, x.shape, "n_iter", km.n_iter_, "inertia", km.inertia_, "counts", np.bincount(km.labels_, minlength=K).tolist())
    path = os.path.join(HERE, "kmeans_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
