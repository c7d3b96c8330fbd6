#!/usr/bin/env python3
"""Recorded sklearn runs for the greedy-seeding tests: tests/golden/kmeans_greedy_v1.npz.

For every case of tests/kmeans_greedy_cases.py::golden_cases (data regenerated from the counter RNG, so only results are stored), on
the float64 image of the fp32 features:

    <name>_idx                       the indices of sklearn.cluster.kmeans_plusplus(x, K, random_state=42)
    <name>_labels / _n_iter / _inertia / _centers      of KMeans(K, random_state=42).fit(x)            (cases that record a run)
    <name>_labels3 / _n_iter3 / _inertia3 / _centers3  of KMeans(K, random_state=42, n_init=3).fit(x)

plus the sklearn version. Runs where sklearn is installed (1.7.2 when the fixture was written); the tests read the fixture and need no
sklearn.
Usage:  python tests/golden/gen_golden_kmeans_greedy.py          write the fixture
        python tests/golden/gen_golden_kmeans_greedy.py --scan   print, for every real-valued case, the first random_state at which
                                                                 every draw and argmin of the seeding is decidable (REAL_STATES)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import kmeans_greedy_cases as G  # noqa: E402
from tests import kmeans_greedy_ref as GR  # noqa: E402


def scan():
    for name, (x, K, _) in G.real_cases().items():
        for state in range(1000):
            first, u = GR.draws(state, x.shape[0], K)[0]
            s = GR.seed(x, K, first, u, delta=G.deltas)
            if s["draw_ok"].all() and s["pick_ok"].all():
                print(f'"{name}": {state},')
                break
        else:
            print(name, "no decidable state below 1000")


def main():
    import sklearn
    from sklearn.cluster import KMeans, kmeans_plusplus
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (x, K, run) in G.golden_cases().items():
        x64 = x.astype(np.float64)
        _, idx = kmeans_plusplus(x64, K, random_state=G.RANDOM_STATE)
        out[name + "_idx"] = idx.astype(np.int32)
        msg = [name, x.shape, "idx", idx.tolist()[:8]]
        if run:
            for n_init, tag in ((1, ""), (3, "3")):
                km = KMeans(n_clusters=K, random_state=G.RANDOM_STATE, n_init=n_init).fit(x64)
                out[name + "_labels" + tag] = km.labels_.astype(np.int8)
                out[name + "_centers" + tag] = km.cluster_centers_.astype(np.float64)
                out[name + "_n_iter" + tag] = np.array(km.n_iter_, dtype=np.int64)
                out[name + "_inertia" + tag] = np.array(km.inertia_, dtype=np.float64)
                msg += [f"n_init={n_init}: n_iter", km.n_iter_, "inertia", km.inertia_]
        print(*msg)
    path = os.path.join(HERE, "kmeans_greedy_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    scan() if "--scan" in sys.argv[1:] else main()
