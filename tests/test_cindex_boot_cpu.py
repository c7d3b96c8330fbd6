"""CPU: the bootstrap of the concordance index without a device. The weighted formulas (tests/cindex_boot_ref.py) are pinned against
oracle/cindex_oracle.py on the EXPANDED arrays of each resample, the oracle on those expansions against what the reference's own
function answered (tests/golden/cindex_boot_v1.npz), and the C entry / the Python wrappers refuse what they must."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import cindex_oracle as CO
from tests import cindex_boot_ref as R

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "cindex_boot_v1.npz"))
EINVAL = -1
A16 = 0x7F0000001000          # a fake, 16-byte aligned "device address": never dereferenced when validation does its job


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib


@pytest.mark.parametrize("k", range(len(R.GOLDEN_CASES)))
def test_oracle_on_the_expansions_equals_the_reference_golden(k):
    ev, tm, est, W = R.golden_inputs(k)
    assert int(GOLD["n"][k]) == R.GOLDEN_CASES[k]["n"] and W.shape == (R.GOLDEN_B, R.GOLDEN_CASES[k]["n"])
    for b in range(R.GOLDEN_B):
        code, c, counts = R.oracle_resample(CO, ev, tm, est, W[b])
        assert code == GOLD["code"][k, b], (k, b)
        if counts is not None:
            assert list(counts) == GOLD["counts"][k, b].tolist(), (k, b)
        assert c == GOLD["cindex"][k, b] or (np.isnan(c) and np.isnan(GOLD["cindex"][k, b])), (k, b)


def test_golden_holds_every_way_the_reference_answers():
    seen = set(GOLD["code"].reshape(-1).tolist())
    assert {R.OK, R.ALL_CENSORED, R.NO_COMPARABLE, R.NO_PAIR} <= seen, seen


def _entries_by_expansion(ev, tm, w_row):
    """Slot 5 as advmil_cindex_counts defines it, on the expansion: events with another sample at or after their time."""
    xe, xt = R.expand(w_row, ev != 0, tm)
    return sum(1 for i in np.nonzero(xe)[0] if int((xt >= xt[i]).sum()) - 1 > 0)


def _sweep_weights(rs, n, B):
    """Bootstrap rows, then the rows a bootstrap rarely draws: all zero, a single copy, one sample n times, a large multiplicity."""
    W = R.multiplicities(rs.randint(0, n, size=(B, n)), n)
    extra = np.zeros((4, n), dtype=np.int32)
    extra[1, rs.randint(n)] = 1
    extra[2, rs.randint(n)] = n
    extra[3] = rs.randint(0, 3, size=n)
    extra[3, rs.randint(n)] = 2 * n
    return np.concatenate([W, extra])


@pytest.mark.parametrize("n", [2, 3, 5, 17, 64, 65])
@pytest.mark.parametrize("p_event", [0.15, 0.5])
def test_restatement_equals_oracle_on_the_expansions(n, p_event):
    rs = np.random.RandomState(1000 + n + int(100 * p_event))
    ev, tm, est = R.boot_case(50 + n, n, p_event, M=2)
    W = _sweep_weights(rs, n, 20)
    got = R.counts_weighted(ev, tm, est, W)
    code, cidx = R.classify(got), R.cindex_of(got)
    assert np.array_equal(got[0, :, 3:], got[1, :, 3:])                       # what does not depend on the estimate row
    for b in range(W.shape[0]):
        assert got[0, b, 5] == _entries_by_expansion(ev, tm, W[b]), (n, b)
        assert got[0, b, 6] == int(W[b][ev != 0].sum()) and got[0, b, 7] == int(W[b].sum())
        for m in range(2):
            wcode, wc, wcounts = R.oracle_resample(CO, ev, tm, est[m], W[b])
            assert code[m, b] == wcode, (n, m, b, code[m, b], wcode)
            if wcounts is not None:
                con, dis, tie, tt = wcounts
                assert got[m, b, :5].tolist() == [con, dis, tie, tt, con + dis + tie], (n, m, b)
            assert cidx[m, b] == wc or (np.isnan(cidx[m, b]) and np.isnan(wc)), (n, m, b)      # bit for bit


def test_host_side_of_the_product_forms_the_same_samples():
    from advmil_amd.eval import bootstrap as BS
    ev, tm, est = R.boot_case(7, 17, 0.15, M=3)
    W = _sweep_weights(np.random.RandomState(5), 17, 60)
    counts = R.counts_weighted(ev, tm, est, W)
    samples, undefined = BS.samples_from_counts(counts)
    want = R.cindex_of(counts)
    assert samples.dtype == np.float64 and np.array_equal(undefined, R.classify(counts) != R.OK)
    assert np.array_equal(np.isnan(samples), np.isnan(want)) and np.array_equal(samples[~undefined], want[~undefined])
    assert 0 < undefined.sum() < undefined.size


def test_resample_indices_is_the_documented_numpy_call():
    from advmil_amd.eval import resample_indices
    for n, B, seed in [(17, 5, 0), (64, 200, 3), (2, 1, 99)]:
        got = resample_indices(n, B, seed)
        assert got.dtype == np.int64 and got.shape == (B, n)
        assert np.array_equal(got, np.random.RandomState(seed).randint(0, n, size=(B, n)))


def test_kernel_constants_are_the_ones_python_exposes(L):
    t, r, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert L.lib().advmil_cindex_counts_weighted_plan(ctypes.byref(t), ctypes.byref(r), ctypes.byref(c)) == 0
    assert (t.value, r.value, c.value) == (L.CINDEX_BOOT_ROW_TILE, L.CINDEX_BOOT_RESAMPLE_CHUNK, L.CINDEX_BOOT_MAX_CHUNK_BLOCKS)
    from advmil_amd.eval import bootstrap as BS
    assert (BS.ROW_TILE, BS.RESAMPLE_CHUNK) == (t.value, r.value)
    assert L.lib().advmil_cindex_counts_weighted_plan(None, ctypes.byref(r), ctypes.byref(c)) == EINVAL


def test_abi_refuses_every_bad_argument_without_a_device(L):
    p = lambda k: ctypes.c_void_p(A16 + (k << 24))   # noqa: E731
    good = dict(time=p(0), event=p(1), est=p(2), lde=64, M=2, w=p(3), ldw=64, B=8, n=64, tol=1e-8, out=p(4))

    def call(**kw):
        a = dict(good, **kw)
        return L.lib().advmil_cindex_counts_weighted(a["time"], a["event"], a["est"], a["lde"], a["M"], a["w"], a["ldw"], a["B"], a["n"],
                                                     a["tol"], a["out"], None)

    for name in ("time", "event", "est", "w", "out"):
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(n=0, lde=0, ldw=0), dict(n=(1 << 20) + 1, lde=1 << 21, ldw=1 << 21), dict(B=0), dict(B=(1 << 20) + 1), dict(M=0),
               dict(M=65), dict(lde=63), dict(ldw=63), dict(tol=-1e-8), dict(tol=float("nan")),
               dict(w=ctypes.c_void_p(A16 + 2)), dict(est=ctypes.c_void_p(A16 + 1)), dict(out=ctypes.c_void_p(A16 + 4))):
        assert call(**kw) == EINVAL, kw


def test_wrappers_raise_the_stated_errors_without_a_device(monkeypatch):
    from advmil_amd.eval import (bootstrap_concordance_index, bootstrap_concordance_samples, concordance_counts_weighted, multiplicities,
                                 paired_bootstrap_concordance)
    ev, tm, est = (torch.from_numpy(a) for a in R.boot_case(3, 17, 0.5))
    W = torch.ones(4, 17, dtype=torch.int32)
    with pytest.raises(ValueError, match="inconsistent"):
        concordance_counts_weighted(ev, tm, est[:, :16], W)
    with pytest.raises(ValueError, match="inconsistent"):
        concordance_counts_weighted(ev[:5], tm, est, W)
    with pytest.raises(ValueError, match="inconsistent"):
        concordance_counts_weighted(ev, tm, est, W[:, :9])
    with pytest.raises(ValueError, match="int32"):
        concordance_counts_weighted(ev, tm, est, W.to(torch.int64))
    neg = W.clone()
    neg[2, 3] = -1
    with pytest.raises(ValueError, match="negative"):
        concordance_counts_weighted(ev, tm, est, neg)
    with pytest.raises(ValueError):
        multiplicities(np.array([[0, 17]]), 17)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    y = torch.stack([tm, ev], dim=1)
    for fn in (lambda: concordance_counts_weighted(ev, tm, est, W), lambda: multiplicities(np.zeros((2, 17), dtype=np.int64), 17),
               lambda: bootstrap_concordance_index(y, est.reshape(-1, 1)), lambda: bootstrap_concordance_samples(y, est.t().repeat(1, 3)),
               lambda: paired_bootstrap_concordance(y, est.reshape(-1, 1), -est.reshape(-1, 1))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    from advmil_amd.eval import ContSurv_Evaluator, CoxSurv_Evaluator, DiscSurv_Evaluator
    for evl in (ContSurv_Evaluator(end_time=1.0), DiscSurv_Evaluator(), CoxSurv_Evaluator()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evl.bootstrap({"y": y, "y_hat": est.reshape(-1, 1)})
