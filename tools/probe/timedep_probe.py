#!/usr/bin/env python3
"""Dev probe: device time of one eval.ipcw_rows call (the sort of the cohort, the prologue, the per-row walk and the pair pass,
csrc/timedep.hip) and of the C entry alone, at the size the bootstrap runs it:

  n = 1000, Q = 16, R = 1      the point estimate: Brier score and AUC(t) at 16 query times;
  n = 1000, Q = 16, R = 1000   ... of a thousand resamples (integer weights), one risk column per query time.

Half the samples are events, times on 200 levels (ties), risks on 64 levels (ties). Device events around each call, REPEATS calls after
WARMUP warm-up calls of the same shape (operands resident on the device), the whole timing PASSES times over; median, min and max of
every pass are recorded. The first CHECK rows are compared with the float64 restatement (tests/timedep_ref.py) before anything is
timed, and the restatement's time per row on one CPU is recorded beside the kernel's. usage: timedep_probe.py [out.json]"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import timedep_ref as R  # noqa: E402

WARMUP, REPEATS, PASSES, CHECK = 5, 50, 2, 8
CASES = [dict(n=1000, rows=1, Q=16), dict(n=1000, rows=1000, Q=16)]


def inputs(case):
    n, rows, Q = case["n"], case["rows"], case["Q"]
    rs = np.random.RandomState(n + rows)
    tm = (np.floor(rs.rand(n) * 200) / 200).astype(np.float32)
    ev = (rs.rand(n) < 0.5).astype(np.float32)
    at = np.quantile(tm, np.linspace(0.1, 0.9, Q), method="lower").astype(np.float32)
    surv = np.sort(rs.rand(n, Q), axis=1)[:, ::-1].astype(np.float32).copy()
    risk = (np.round((1 - surv) * 64) / 64).astype(np.float32)
    W = R.multiplicities(rs.randint(0, n, size=(rows, n)), n) if rows > 1 else None
    return ev, tm, at, surv, risk, W


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
    from advmil_amd import _lib
    from advmil_amd.eval import ipcw_rows
    dev = torch.device("cuda", 0)
    rows = []
    for case in CASES:
        ev, tm, at, surv, risk, W = inputs(case)
        k = min(CHECK, case["rows"])
        t0 = time.perf_counter()
        want = R.rows(ev, tm, at, surv, risk, None if W is None else W[:k])
        cpu_s = (time.perf_counter() - t0) / k
        d = [None if a is None else torch.from_numpy(a).to(dev) for a in (ev, tm, at, surv, risk, W)]
        call = lambda: ipcw_rows(*d)                       # noqa: E731
        r = call()
        got_c, got_s = r.counts[:k].cpu().numpy(), r.sums[:k].cpu().numpy()
        same = bool(np.array_equal(got_c, want["counts"]) and (np.abs(got_s - want["sums"]) <= want["bound"] * np.abs(want["sums"])).all())
        # the C entry alone: the preparation done once, as a caller that keeps the sorted cohort would
        n, Q, nrows = case["n"], case["Q"], case["rows"]
        stime, order = torch.sort(d[1], stable=True)
        sevent, order = d[0][order].contiguous(), order.to(torch.int32)
        L = _lib.lib()
        wsb = L.advmil_ipcw_rows_workspace_bytes(n, nrows, Q)
        ws = torch.empty(wsb // 8 + 1, dtype=torch.float64, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def entry():
            _lib.check(L.advmil_ipcw_rows(p(stime), p(sevent), p(order), n, p(d[5]), n if W is not None else 0, nrows, p(d[2]), Q, p(d[3]), Q,
                                          p(d[4]), Q, Q, p(r.counts), p(r.rowcnt), p(r.sums), p(ws), wsb, stream), "ipcw_rows")

        a, b = [], []
        for _ in range(PASSES):
            a.append(timed(call))
            b.append(timed(entry))
        slow = lambda ps: max(x["median_ms"] for x in ps)      # noqa: E731
        row = dict(case, rows_equal_restatement=same, rows_checked=k, ipcw_rows_call=a, c_entry_alone=b, restatement_ms_per_row_one_cpu=1e3 * cpu_s,
                   entry_us_per_row=1e3 * slow(b) / nrows)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
