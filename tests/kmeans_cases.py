"""The data of the k-means tests, regenerated from the counter RNG (advmil_amd/synth.py) so that the fixture tests/golden/kmeans_v1.npz
holds only results: the two (G) cases whose sklearn runs are recorded (tests/golden/gen_golden_kmeans.py), and the real-valued shapes
of tests/test_kmeans_gpu.py."""
import numpy as np

from advmil_amd import synth

SEED = 7


def normal(tag, n, c):
    return synth.normal(synth.stream_key(SEED, "kmeans:" + tag), n * c).reshape(n, c)


def blobs(n, c, k, tag="blobs", spread=6.0):
    """k separated blobs: centres spread * N(0, 1), unit noise, row i in blob i % k -> (x fp32 [n, c], truth int32 [n])."""
    truth = (np.arange(n) % k).astype(np.int32)
    centres = np.float32(spread) * normal(tag + ":centres", k, c)
    return (centres[truth] + normal(tag + ":noise", n, c)).astype(np.float32), truth


def halfnormal(n, c, tag="overlap"):
    """|N(0, 1)| features: one overlapping cloud with a large common mean, the shape of post-ReLU patch embeddings."""
    return np.abs(normal(tag, n, c)).astype(np.float32)


def golden_cases():
    """name -> (x fp32, init fp32 [K, C], K). separated: init = the first row of each blob (rows 0..K-1, so the fixture's labels are the
    true partition); overlap: init = the K stated rows."""
    K = 8
    xs, _ = blobs(1031, 64, K)
    xo = halfnormal(1500, 96)
    rows = [3, 190, 377, 564, 751, 938, 1125, 1312]
    return {"separated": (xs, xs[:K].copy(), K), "overlap": (xo, xo[rows].copy(), K)}
