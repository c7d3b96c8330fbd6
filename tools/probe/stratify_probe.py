#!/usr/bin/env python3
"""Dev probe: device time of one eval.logrank_rows call (the sort of the cohort, the query prologue and the row kernel, csrc/strat.hip)
beside the float64 numpy restatement of the same rows (tests/logrank_ref.py) on the box's CPUs, in one run:

  n = 1000, R = 1000, Q = 100   bootstrap rows (integer weights, one shared split) with the curves at 100 query times;
  n = 1000, R = 32000, Q = 0    permutation rows (group bits, no weights), the log-rank sums only.

Half the samples are events, times on 200 levels (ties). Device events around each call, REPEATS calls after WARMUP warm-up calls of
the same shape (operands resident on the device), and the whole timing PASSES times over, call and entry in turn; median, min and max
of every pass are recorded, for the whole call and for the C entry alone, and the ratios are taken from the SLOWER pass's median. The
restatement runs FIRST, in a pool of CPUS forked processes that is closed before the device is touched, and the kernel's rows are
checked against its rows before anything is timed. usage: stratify_probe.py [out.json]"""
import ctypes
import json
import multiprocessing
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import logrank_ref as R  # noqa: E402

WARMUP, REPEATS, PASSES, CPUS = 10, 200, 2, 16
CASES = [dict(n=1000, rows=1000, Q=100, weighted=True), dict(n=1000, rows=32000, Q=0, weighted=False)]
_JOB = {}


def inputs(case):
    n, rows = case["n"], case["rows"]
    rs = np.random.RandomState(n + rows)
    tm = (np.floor(rs.rand(n) * 200) / 200).astype(np.float32)
    ev = (rs.rand(n) < 0.5).astype(np.float32)
    g = (rs.rand(n) < 0.5).astype(np.uint8)
    at = np.linspace(0.0, 1.0, case["Q"]).astype(np.float32) if case["Q"] else None
    if case["weighted"]:
        return ev, tm, g, R.multiplicities(rs.randint(0, n, size=(rows, n)), n), at
    return ev, tm, np.stack([rs.permutation(g) for _ in range(rows)]), None, at


def _chunk(span):
    ev, tm, G, W, at = _JOB["in"]
    co = R.Cohort(ev, tm)
    out = [co.row(G if G.ndim == 1 else G[r], None if W is None else W[r], at) for r in range(*span)]
    return (np.stack([o["counts"] for o in out]), np.array([[o["E1"], o["V"], o["bE1"], o["bV"]] for o in out]),
            np.stack([o["km"] for o in out]), np.array([o["bkm"] for o in out]))


def restatement(case):
    """-> (seconds on CPUS processes, counts, sums + bounds, km, its bound)."""
    _JOB["in"] = inputs(case)
    rows = case["rows"]
    step = (rows + 4 * CPUS - 1) // (4 * CPUS)
    spans = [(a, min(a + step, rows)) for a in range(0, rows, step)]
    with multiprocessing.get_context("fork").Pool(CPUS) as pool:
        pool.map(_chunk, [(0, 1)] * CPUS)                 # the workers are up before the clock starts
        t0 = time.perf_counter()
        parts = pool.map(_chunk, spans)
        dt = time.perf_counter() - t0
    return (dt,) + tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), repeats=REPEATS)


def main():
    cpu = [restatement(c) for c in CASES]                 # every forked process is gone before the device is opened
    from advmil_amd import _lib
    from advmil_amd.eval import logrank_rows
    dev = torch.device("cuda", 0)
    rows = []
    for case, (cpu_s, counts, sums, km, bkm) in zip(CASES, cpu):
        ev, tm, G, W, at = (None if a is None else torch.from_numpy(a).to(dev) for a in inputs(case))
        call = lambda: logrank_rows(ev, tm, G, W, at)      # noqa: E731
        r = call()
        got_c, got_s, got_k = r.counts.cpu().numpy(), r.sums.cpu().numpy(), r.km.cpu().numpy()
        same = bool(np.array_equal(got_c, counts) and (np.abs(got_s - sums[:, :2]) <= sums[:, 2:]).all()
                    and (np.abs(got_k - km) <= bkm[:, None, None] * km).all())
        # the C entry alone: the preparation done once, as a caller that keeps the sorted cohort would
        n, Q, nrows = case["n"], case["Q"], case["rows"]
        stime, order = torch.sort(tm, stable=True)
        sevent, order = ev[order].contiguous(), order.to(torch.int32)
        L = _lib.lib()
        wsb = L.advmil_logrank_rows_workspace_bytes(n, Q)
        ws = torch.empty(max(wsb // 4, 1), dtype=torch.int32, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def entry():
            _lib.check(L.advmil_logrank_rows(p(stime), p(sevent), p(order), n, p(G), 0 if G.dim() == 1 else n, p(W), n if W is not None else 0,
                                             nrows, p(at), Q, p(r.counts), p(r.sums), p(r.km) if Q else None, p(r.median), p(ws) if Q else None,
                                             wsb, stream), "logrank_rows")

        a, b = [], []
        for _ in range(PASSES):
            a.append(timed(call))
            b.append(timed(entry))
        slow = lambda ps: max(p["median_ms"] for p in ps)      # noqa: E731
        row = dict(case, rows_equal_restatement=same, logrank_rows_call=a, c_entry_alone=b, restatement_s=cpu_s, restatement_cpus=CPUS,
                   restatement_ms_per_row_per_cpu=1e3 * cpu_s * CPUS / nrows, speedup_call_median=1e3 * cpu_s / slow(a),
                   speedup_entry_median=1e3 * cpu_s / slow(b))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
