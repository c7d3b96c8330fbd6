"""The data of the greedy-seeding tests, regenerated from the counter RNG of tests/kmeans_cases.py so that the fixture
tests/golden/kmeans_greedy_v1.npz holds only results.

Integer cases: features are integers in [-7, 7] (a rounded, clipped normal), so every bf16x3 distance, every float64 potential and every
prefix sum is exact (the argument of tests/test_kmeans_gpu.py) and the device must EQUAL the oracle and sklearn.
Real-valued cases carry the random_state found by tests/golden/gen_golden_kmeans_greedy.py --scan: the first one at which every draw
and every argmin of the seeding is decidable under the per-distance bound (tests/kmeans_greedy_ref.py)."""
import numpy as np

from tests import kmeans_cases as CASES

RANDOM_STATE = 42
SLAB = [8, 200, 33, 1031]                # K = 8, C = 64: a bag of exactly K rows, a bag inside one chunk pair, a bag over nine chunks
BIG = (1 << 16) + 3                      # the scan carries across 513 workgroups


def ints(tag, n, c, lim=7):
    return np.clip(np.rint(2.5 * CASES.normal("greedy:" + tag, n, c)), -lim, lim).astype(np.float32)


def int_blobs(tag, n, c, k):
    """k integer blobs: centres in [-5, 5], noise in [-2, 2], row i in blob i % k. A Lloyd run on UNSTRUCTURED integer rows meets exact
    distance ties in its first assign (the centres are rows, every distance an integer), which the oracle gives to the lowest centre and
    sklearn, on its centred copy of the rows, to whichever rounding favours; between separated blobs no row is that close to a tie, so
    these are the integer cases whose KMeans runs are recorded."""
    centres = np.clip(np.rint(3.0 * CASES.normal("greedy:" + tag + ":centres", k, c)), -5, 5)
    noise = np.clip(np.rint(CASES.normal("greedy:" + tag + ":noise", n, c)), -2, 2)
    return (centres[np.arange(n) % k] + noise).astype(np.float32)


def slab():
    """-> (x fp32 [sum SLAB, 64], K)"""
    return int_blobs("slab", sum(SLAB), 64, 8), 8


def integer_cases():
    """name -> (x fp32, K, record a KMeans run too)."""
    xs, K = slab()
    offs = np.concatenate([[0], np.cumsum(SLAB)])
    out = {f"slab_bag{b}": (xs[offs[b]:offs[b + 1]], K, True) for b in range(len(SLAB))}
    out.update({
        "k1_c32_n127": (ints("k1", 127, 32), 1, True),
        "k2_c32_n128": (ints("k2", 128, 32), 2, False),
        "k8_c32_n129": (ints("k8", 129, 32), 8, False),
        "blobs_k8_c32_n129": (int_blobs("k8b", 129, 32, 8), 8, True),
        "k32_c32_n32": (ints("k32", 32, 32), 32, False),             # a bag of exactly K rows at L = 5
        "k32_c32_n300": (ints("k32b", 300, 32), 32, False),
        "k8_c1024_n200": (ints("c1024", 200, 1024), 8, False),
        "k32_c1024_n129": (ints("c1024b", 129, 1024), 32, False),
        "k8_c32_big": (ints("big", BIG, 32), 8, False),
    })
    return out


def separated():
    """The separated blobs of tests/kmeans_cases.py::golden_cases -> (x, K, record a KMeans run)."""
    x, _, K = CASES.golden_cases()["separated"]
    return x, K, True


def more_blobs():
    """Twelve separated blobs for eight clusters: every init ends in another local optimum (which blobs share a centre), far apart in
    inertia and with every row far from a tie -- the case in which n_init = 3 keeps a later run."""
    return CASES.blobs(600, 32, 12, tag="greedy-b12", spread=3.0)[0], 8, True


def golden_cases():
    return dict(integer_cases(), separated=separated(), more_blobs=more_blobs())


# name -> (x, K, random_state): --scan of the generator found these states
REAL_STATES = {"blobs_1031x64": 1, "half_300x1024": 5, "blobs_300x32_k32": 9}


def real_cases():
    data = {"blobs_1031x64": (CASES.blobs(1031, 64, 8, tag="greedy-real64", spread=1.0)[0], 8),
            "half_300x1024": (CASES.halfnormal(300, 1024, tag="greedy-h1024"), 8),
            "blobs_300x32_k32": (CASES.blobs(300, 32, 32, tag="greedy-k32", spread=1.0)[0], 32)}
    return {name: (x, K, REAL_STATES[name]) for name, (x, K) in data.items()}


def deltas(x, cent):
    """The per-(row, centre) distance bound the k-means tests already apply to dist2: tests/test_kmeans_gpu.py::deltas itself."""
    from tests.test_kmeans_gpu import deltas as bound
    return bound(np.asarray(x), np.asarray(cent))
