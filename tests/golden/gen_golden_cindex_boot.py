#!/usr/bin/env python3
"""Golden vectors for the bootstrap of the concordance index: runs the REFERENCE's eval/cindex.py::concordance_index_censored on the
EXPANDED arrays (sample i repeated as often as the resample drew it) of the seeded cases of tests/cindex_boot_ref.py -- n in
{2, 3, 17, 64, 65} at 15 % and 50 % events, ties in time and in the estimate, 16 resamples each -- and stores what it answered:
the four integer counts, the float64 C-index and a code for the exception it raised (cindex_boot_ref.OK / TOO_SMALL / ALL_CENSORED /
NO_COMPARABLE / NO_PAIR). Numbers only. Needs a checkout of the reference (and sklearn, which its module imports).
Usage: python tests/golden/gen_golden_cindex_boot.py <path to the reference>"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests import cindex_boot_ref as R  # noqa: E402

FIXTURE = os.path.join(HERE, "cindex_boot_v1.npz")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from eval import cindex as REF          # the reference's module
    K, B = len(R.GOLDEN_CASES), R.GOLDEN_B
    counts = np.full((K, B, 4), -1, dtype=np.int64)
    cindex = np.full((K, B), np.nan, dtype=np.float64)
    code = np.zeros((K, B), dtype=np.int64)
    for k in range(K):
        ev, tm, est, W = R.golden_inputs(k)
        for b in range(B):
            xe, xt, xs = R.expand(W[b], ev != 0, tm, est)
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")          # 0 / 0 where no pair is comparable
                    got = REF.concordance_index_censored(xe, xt, xs, tied_tol=1e-08)
            except REF.NoComparablePairException:
                code[k, b] = R.NO_COMPARABLE
                continue
            except ValueError as exc:
                code[k, b] = R.TOO_SMALL if "minimum" in str(exc) else R.ALL_CENSORED
                assert "minimum" in str(exc) or "censored" in str(exc), exc
                continue
            counts[k, b] = [int(v) for v in got[1:]]
            cindex[k, b] = float(got[0])
            code[k, b] = R.NO_PAIR if np.isnan(got[0]) else R.OK
        print(k, R.GOLDEN_CASES[k], "codes", np.bincount(code[k], minlength=5).tolist())
    np.savez_compressed(FIXTURE, counts=counts, cindex=cindex, code=code, n=np.array([c["n"] for c in R.GOLDEN_CASES]),
                        p_event=np.array([c["p_event"] for c in R.GOLDEN_CASES]))
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
