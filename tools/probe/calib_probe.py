#!/usr/bin/env python3
"""Dev probe: device time of one advmil_calib_rows call (per-row walk with and without the pseudo-observation scans, D-calibration pass:
csrc/calib.hip) at the sizes the bootstrap runs it, against a numpy float64 loop on the host, all in ONE process:

  n = 1000 and 4096, R = 1 and 1001 (the cohort and 1000 resamples), two prediction columns, ten bins;
  (i)  the C entry alone on the prepared cohort: pred with with_po = 1, pred with with_po = 0 (the difference is what the
       pseudo-observation costs), p_own alone with with_po = 0 (walk + D-calibration pass), everything together;
  (ii) the same statistics per row in numpy float64 with the SAME O(n) block recurrences (np.cumprod / np.cumsum over the tie blocks, a
       python loop only for the backward recurrence), one row per task on a pool of CPU_WORKERS processes; timed on NUMPY_ROWS rows and
       scaled to R -- it is linear in the rows.

Half the samples are events, times on 200 levels (ties). Device events around each call, REPEATS calls after WARMUP warm-up calls, the
variants interleaved PASSES times; median, min and max of every pass are recorded. The first CHECK rows are compared with the float64
restatement (tests/calib_ref.py) and the numpy loop with the kernel before anything is timed. Each section of a case runs under a time
limit of its own (SIGALRM): a section that overruns ends the process with an error. usage: calib_probe.py [out.json]"""
import ctypes
import json
import multiprocessing
import os
import signal
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import calib_ref as R  # noqa: E402

WARMUP, REPEATS, PASSES, CHECK, NUMPY_ROWS, CPU_WORKERS = 3, 20, 2, 3, 64, 16
LIMITS = dict(check=120, kernels=120, numpy=120)           # seconds per section
CASES = [dict(n=1000, rows=1), dict(n=1000, rows=1001), dict(n=4096, rows=1), dict(n=4096, rows=1001)]
P, BINS, GAMMA = 2, 10, 1.0


class Overrun(RuntimeError):
    pass


def limited(name):
    def handler(signum, frame):
        raise Overrun(f"section {name!r} ran longer than {LIMITS[name]} s")
    signal.signal(signal.SIGALRM, handler)
    signal.alarm(LIMITS[name])


def inputs(case):
    n, rows = case["n"], case["rows"]
    rs = np.random.RandomState(n + rows)
    tm = (np.ceil(rs.rand(n) * 200) / 50).astype(np.float32)
    ev = (rs.rand(n) < 0.5).astype(np.float32)
    pred = (tm[:, None] * np.exp(0.5 * rs.randn(n, P))).astype(np.float32)
    p = rs.rand(n).astype(np.float32)
    W = np.ones((1, n), dtype=np.int32)
    if rows > 1:
        W = np.concatenate([W, R.multiplicities(rs.randint(0, n, size=(rows - 1, n)), n)])
    return ev, tm, pred, p, W


def timed(fn, repeats=REPEATS):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), repeats=repeats)


def numpy_rows(task):
    """task = (the sorted cohort, rows [k, n]) -> [numpy_row(cohort, w) for every row]: what one worker of the pool is handed."""
    return [numpy_row(task[0], w) for w in task[1]]


def numpy_row(cohort, w):
    """One row in numpy float64 on the sorted cohort: the block recurrences of csrc/calib.hip. -> err [P, 3, 2], dcal [BINS]."""
    st, se, inv, first, sp, pp = (cohort[k] for k in ("st", "se", "inv", "first", "pred", "p"))
    w = w.astype(np.float64)
    N = w.sum()
    nb = first.size
    cw = np.concatenate([[0.0], np.cumsum(w)])
    at_risk = N - cw[first]
    d = np.bincount(inv, weights=w * se, minlength=nb)
    u = st[first]
    du = np.where(at_risk > 0, u - np.concatenate([[0.0], u[:-1]]), 0.0)
    with np.errstate(all="ignore"):
        f = np.where(d > 0, (at_risk - d) / at_risk, 1.0)
        g = np.where((d > 0) & (at_risk - 1 >= d), (at_risk - 1 - d) / (at_risk - 1), 1.0)
    S, Sp = np.cumprod(f), np.cumprod(g)
    theta = float((np.concatenate([[1.0], S[:-1]]) * du).sum())
    thp = np.cumsum(np.concatenate([[1.0], Sp[:-1]]) * du)
    T = np.zeros(nb)
    for b in range(nb - 2, -1, -1):
        T[b] = du[b + 1] + f[b + 1] * T[b + 1]
    Sb, Tb = S[inv], T[inv]
    cens = se == 0
    omega = np.where(cens, 1.0 - Sb, 1.0)
    m = np.where(cens & (Sb > 0), st + Tb, st)
    s = np.where(cens, N * theta - (N - 1) * (thp[inv] + Sp[inv] * Tb), st)
    err = np.zeros((P, 3, 2))
    den = float((w * omega).sum())
    for c in range(P):
        y = sp[:, c]
        h = np.where(cens, np.maximum(0.0, st + GAMMA - y), np.abs(st - y))
        err[c] = [[(w * h).sum(), N], [(w * omega * np.abs(m - y)).sum(), den], [(w * omega * np.abs(s - y)).sum(), den]]
    kb = np.minimum(BINS - 1, (pp.astype(np.float32) * np.float32(BINS)).astype(np.int64))
    pos = cens & (pp > 0)
    safe = np.where(pos, pp, 1.0)
    own = np.where(pos, w * (pp - kb / BINS) / safe, w)
    own_bin = np.where(cens & ~pos, 0, kb)
    below = np.bincount(kb, weights=np.where(pos, w / (BINS * safe), 0.0), minlength=BINS)
    dcal = np.bincount(own_bin, weights=own, minlength=BINS) + np.concatenate([np.cumsum(below[::-1])[::-1][1:], [0.0]])
    return err, dcal


def main():
    # the host baseline's workers are started BEFORE the device is opened: they never hold it, and the process count with the GPU open stays 1
    pool = multiprocessing.get_context("fork").Pool(CPU_WORKERS)
    from advmil_amd import _lib
    from advmil_amd.eval import calib_rows
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    plan = [ctypes.c_int(0) for _ in range(3)]
    L.advmil_calib_rows_plan(*(ctypes.byref(x) for x in plan))
    results = []
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None    # noqa: E731
    for case in CASES:
        n, rows = case["n"], case["rows"]
        ev, tm, pred, p, W = inputs(case)
        # ---- section 1: the kernel's rows against the restatement ----
        limited("check")
        d = dict(ev=torch.from_numpy(ev).to(dev), tm=torch.from_numpy(tm).to(dev), pred=torch.from_numpy(pred).to(dev),
                 p=torch.from_numpy(p).to(dev), W=torch.from_numpy(W).to(dev))
        r = calib_rows(d["ev"], d["tm"], d["pred"], d["p"], BINS, GAMMA, True, d["W"])
        k = min(CHECK, rows)
        want = R.rows(ev, tm, pred, p, BINS, GAMMA, W[:k])
        got = {a: getattr(r, a)[:k].cpu().numpy() for a in ("rowcnt", "km", "err", "dcal")}
        mine = {a: getattr(r, a)[:NUMPY_ROWS].cpu().numpy() for a in ("err", "dcal")}     # (the timed calls below write into r's arrays)
        same = bool(np.array_equal(got["rowcnt"], want["rowcnt"]) and (np.abs(got["km"] - want["km"]) <= 2 * want["b_km"]).all()
                    and (np.abs(got["err"] - want["err"]) <= 2 * want["b_err"]).all()
                    and (np.abs(got["dcal"] - want["dcal"]) <= 2 * want["b_dcal"][:, None]).all())
        # ---- section 2: the C entry alone, the sorted cohort prepared once ----
        limited("kernels")
        stime, order = torch.sort(d["tm"], stable=True)
        sevent, order32 = d["ev"][order].contiguous(), order.to(torch.int32)
        wsb = L.advmil_calib_rows_workspace_bytes(n, rows, 1)
        ws = torch.empty(wsb // 8 + 1, dtype=torch.float64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def calib(y, q, po):
            def go():
                _lib.check(L.advmil_calib_rows(ptr(stime), ptr(sevent), ptr(order32), n, ptr(d["W"]), n, rows, ptr(y), P, P, ptr(q), BINS,
                                               GAMMA, po, ptr(r.rowcnt), ptr(r.km), ptr(r.err), ptr(r.dcal), ptr(ws), wsb, stream), "calib_rows")
            return go
        fns = dict(pred_po=calib(d["pred"], None, 1), pred_no_po=calib(d["pred"], None, 0), p_own_only=calib(None, d["p"], 0),
                   everything=calib(d["pred"], d["p"], 1))
        times = {a: [] for a in fns}
        for _ in range(PASSES):
            for a, fn in fns.items():
                times[a].append(timed(fn))
        # ---- section 3: numpy float64 on the host, one row per task ----
        limited("numpy")
        st, se = stime.cpu().numpy().astype(np.float64), sevent.cpu().numpy().astype(np.float64)
        o = order.cpu().numpy()
        _, first, inv = np.unique(st, return_index=True, return_inverse=True)
        cohort = dict(st=st, se=se, inv=inv, first=first, pred=pred[o].astype(np.float64), p=p[o].astype(np.float64))
        Ws = W[:NUMPY_ROWS][:, o]
        ref = [numpy_row(cohort, w) for w in Ws[:k]]
        numpy_agrees = bool(all(np.allclose(e, mine["err"][i], rtol=1e-9, atol=0) and np.allclose(c, mine["dcal"][i], rtol=1e-9, atol=1e-9)
                                for i, (e, c) in enumerate(ref)))
        full = np.stack([Ws[i % len(Ws)] for i in range(NUMPY_ROWS)])
        tasks = [(cohort, chunk) for chunk in np.array_split(full, CPU_WORKERS)]  # one chunk of rows per worker
        pool.map(numpy_rows, tasks)
        t0 = time.perf_counter()
        pool.map(numpy_rows, tasks)
        t_pool = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for w in full[:8]:
            numpy_row(cohort, w)
        t_one = (time.perf_counter() - t0) * 1e3 / 8
        signal.alarm(0)
        slow = lambda ps: max(x["median_ms"] for x in ps)      # noqa: E731
        allms = slow(times["everything"])
        row = dict(case, P=P, bins=BINS, plan=dict(walk_rows=plan[0].value, walk_trip=plan[1].value, dcal_rows=plan[2].value),
                   rows_equal_restatement=same, rows_checked=k, numpy_agrees=numpy_agrees, times=times,
                   pred_po_ms=slow(times["pred_po"]), pred_no_po_ms=slow(times["pred_no_po"]), p_own_only_ms=slow(times["p_own_only"]),
                   everything_ms=allms, ns_per_row_sample_everything=1e6 * allms / (rows * n),
                   numpy_rows_timed=NUMPY_ROWS, cpu_workers=CPU_WORKERS, numpy_ms_per_row_one_process=t_one,
                   numpy_pool_ms_for_timed_rows=t_pool, numpy_ms_scaled_to_all_rows=t_pool * rows / NUMPY_ROWS if rows > 1 else t_one,
                   ratio_numpy_vs_everything=(t_pool * rows / NUMPY_ROWS if rows > 1 else t_one) / allms)
        results.append(row)
        print(json.dumps(row), flush=True)
    pool.close()
    pool.join()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
