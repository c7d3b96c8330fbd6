"""numpy restatement of the weighted concordance counts (advmil_cindex_counts_weighted, include/advmil_hip.h), shared by
tests/test_cindex_boot_cpu.py and tests/test_cindex_boot_gpu.py, and the seeded inputs of both. TEST INFRASTRUCTURE ONLY.

The formulas, per event anchor i (event_i != 0) and per j:
  later = t_j > t_i; same_cens = t_j == t_i and event_j == 0; the pair is comparable iff later or same_cens;
  tied if |e_j - e_i| <= tied_tol (float32), else concordant if e_j < e_i, else discordant; every counter grows by w_i * w_j;
  events_with_entry += w_i * [sum_j w_j [t_j >= t_i] - 1 > 0], j == i included;
  slot 6 = sum_i w_i [event_i != 0], slot 7 = sum_i w_i.
test_cindex_boot_cpu.py pins them against oracle/cindex_oracle.py on the EXPANDED arrays (sample i repeated w_i times)."""
import numpy as np

from advmil_amd import synth

SLOTS = ("concordant", "discordant", "tied_risk", "tied_time", "comparable", "events_with_entry", "event_copies", "size")
OK, TOO_SMALL, ALL_CENSORED, NO_COMPARABLE, NO_PAIR = 0, 1, 2, 3, 4       # how the reference answers one resample


def counts_weighted(event, time, estimate, weights, tied_tol=1e-8):
    """event [n], time [n], estimate [n] or [M, n] (float32), weights [B, n] (integers >= 0) -> int64 [M, B, 8]."""
    ev = np.asarray(event) != 0
    t = np.asarray(time, dtype=np.float32)
    est = np.asarray(estimate, dtype=np.float32)
    est = est.reshape(1, -1) if est.ndim == 1 else est
    W = np.asarray(weights).astype(np.float64)                     # products and sums stay far below 2^53: exact
    B, n = W.shape
    M = est.shape[0]
    tol = np.float32(tied_tol)
    later = t[None, :] > t[:, None]                                # [i, j]
    same_cens = (t[None, :] == t[:, None]) & ~ev[None, :]
    cmp_ = (later | same_cens) & ev[:, None]
    at_or_after = (t[None, :] >= t[:, None]) & ev[:, None]
    Wa = W * ev[None, :]                                           # w_i of the anchors, 0 for censored samples

    def total(cls):                                                # sum_i w_i sum_j w_j cls[i, j], per resample
        s = (Wa * (W @ cls.T.astype(np.float64))).sum(axis=1)
        assert s.max(initial=0) < 2.0 ** 53
        return np.rint(s).astype(np.int64)

    out = np.zeros((M, B, 8), dtype=np.int64)
    out[:, :, 3] = total(same_cens & ev[:, None])
    out[:, :, 4] = total(cmp_)
    out[:, :, 5] = np.rint((Wa * ((W @ at_or_after.T.astype(np.float64)) - 1 > 0)).sum(axis=1)).astype(np.int64)
    out[:, :, 6] = np.rint(Wa.sum(axis=1)).astype(np.int64)
    out[:, :, 7] = np.rint(W.sum(axis=1)).astype(np.int64)
    for m in range(M):
        e = est[m]
        diff = e[None, :] - e[:, None]                             # e_j - e_i, float32 as in the kernel and in numpy on float32 inputs
        assert diff.dtype == np.float32
        tie = cmp_ & (np.absolute(diff) <= tol)
        con = cmp_ & ~tie & (e[None, :] < e[:, None])
        out[m, :, 0] = total(con)
        out[m, :, 2] = total(tie)
        out[m, :, 1] = out[m, :, 4] - out[m, :, 0] - out[m, :, 2]
    return out


def classify(counts):
    """counts [..., 8] -> the code of each resample: what the reference does on its expansion."""
    c = np.asarray(counts)
    code = np.full(c.shape[:-1], OK, dtype=np.int64)
    code[c[..., 4] == 0] = NO_PAIR                                 # entries but no comparable pair: 0 / 0
    code[c[..., 5] == 0] = NO_COMPARABLE                           # NoComparablePairException
    code[c[..., 6] == 0] = ALL_CENSORED                            # "All samples are censored"
    code[c[..., 7] < 2] = TOO_SMALL                                # "Need a minimum of two samples"
    return code


def cindex_of(counts):
    """counts [..., 8] -> float64 (con + 0.5 * tie) / comp in Python arithmetic, NaN where classify() != OK."""
    c = np.asarray(counts)
    code = classify(c)
    out = np.full(c.shape[:-1], np.nan, dtype=np.float64)
    for ix in np.ndindex(*c.shape[:-1]):
        if code[ix] == OK:
            out[ix] = (int(c[ix][0]) + 0.5 * int(c[ix][2])) / int(c[ix][4])
    return out


def expand(w_row, *arrays):
    """The arrays of one resample: sample i repeated w_row[i] times."""
    return tuple(np.repeat(np.asarray(a), np.asarray(w_row), axis=-1) for a in arrays)


def oracle_resample(CO, event, time, est, w_row, tied_tol=1e-8):
    """oracle/cindex_oracle.py::cindex_counts on the expansion -> (code, cindex or NaN, (con, dis, tie, tied_time) or None)."""
    ev, tm, e = expand(w_row, np.asarray(event) != 0, time, est)
    try:
        c, con, dis, tie, tt = CO.cindex_counts(ev, tm, e, tied_tol)
    except CO.NoComparablePairException:
        return NO_COMPARABLE, float("nan"), None
    except ValueError as exc:
        return (TOO_SMALL if "minimum" in str(exc) else ALL_CENSORED), float("nan"), None
    if con + dis + tie == 0:
        return NO_PAIR, float("nan"), (con, dis, tie, tt)
    return OK, c, (con, dis, tie, tt)


def multiplicities(indices, n):
    idx = np.asarray(indices)
    return np.stack([np.bincount(row, minlength=n) for row in idx]).astype(np.int32)


def boot_case(idx, n, p_event, time_levels=5, est_levels=4, M=1):
    """Seeded inputs (counter RNG) with ties in time and in the estimate -> (event f32 [n], time f32 [n], estimate f32 [M, n])."""
    u = synth.device_uniform(1700 + idx, 1, (2 + M) * n).astype(np.float32)
    t = np.floor(u[:n] * time_levels).astype(np.float32) / np.float32(time_levels)
    e = (u[n:2 * n] < p_event).astype(np.float32)
    est = np.floor(u[2 * n:].reshape(M, n) * est_levels).astype(np.float32) / np.float32(est_levels)
    return e, t, est


GOLDEN_B = 16
GOLDEN_CASES = [dict(n=n, p_event=p) for n in (2, 3, 17, 64, 65) for p in (0.15, 0.5)]


def golden_inputs(k):
    """Case k of tests/golden/cindex_boot_v1.npz -> (event, time, estimate [n], weights int32 [16, n])."""
    c = GOLDEN_CASES[k]
    e, t, est = boot_case(k, c["n"], c["p_event"])
    idx = np.random.RandomState(100 + k).randint(0, c["n"], size=(GOLDEN_B, c["n"]))
    return e, t, est[0], multiplicities(idx, c["n"])
