#!/usr/bin/env python3
"""Dev probe: device time of one advmil_concord_rows call (prologue, per-row walk, pair pass, reduce: csrc/concord.hip) at the size the
bootstrap runs it -- the cohort and 1000 resamples, both sources, one tau -- against two baselines, all in ONE process:

  n = 1000, R = 1001, T = 1     and the same at n = 4000;
  (i)  advmil_ipcw_rows at the same n and R with Q = 1 (the median time) and one risk column: the parent's kernel of the same structure.
       Its pair pass visits cases x controls of ONE query time, this one every case with everything at or behind its tie block, so the
       probe counts the pairs each kernel visits and reports time per (row, visited pair);
  (ii) the same statistic in plain torch on the device, per row with n x n broadcasts (the masks are built once, outside the timing);
       timed on TORCH_ROWS rows and scaled to R -- it is linear in the rows.

Half the samples are events, times on 200 levels (ties), risks on 64 levels (ties), the survival matrix at the distinct event times.
Device events around each call, REPEATS calls after WARMUP warm-up calls, the two kernels interleaved PASSES times; median, min and max
of every pass are recorded. The first CHECK rows are compared with the float64 restatement (tests/concord_ref.py) before anything is
timed. Each of the three sections (check, kernels, torch) of a case runs under a time limit of its own (SIGALRM): a section that overruns
ends the process with an error. usage: concord_probe.py [out.json]"""
import ctypes
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import concord_ref as R  # noqa: E402

WARMUP, REPEATS, PASSES, CHECK, TORCH_ROWS = 3, 20, 2, 4, 8
LIMITS = dict(check=120, kernels=120, torch=120)           # seconds per section
CASES = [dict(n=1000, rows=1001), dict(n=4000, rows=1001)]


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
    tm = (np.floor(rs.rand(n) * 200) / 200).astype(np.float32)
    ev = (rs.rand(n) < 0.5).astype(np.float32)
    at = np.unique(tm[ev != 0])
    col = R.own_columns(tm, at).astype(np.int32)
    base = rs.rand(n, 1)
    surv = np.clip(np.round((1 - at[None, :]) * base * 64) / 64, 0, 1).astype(np.float32)
    risk = (np.round((1 - base[:, 0]) * 64) / 64).astype(np.float32)
    W = np.concatenate([np.ones((1, n), dtype=np.int32), R.multiplicities(rs.randint(0, n, size=(rows - 1, n)), n)])
    return ev, tm, risk, surv, col, W


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


def torch_rows(stime, sevent, masks, W_sorted, tau):
    """The statistic of every row of W_sorted [r, n] (in sorted order) in plain torch: per row the censoring Kaplan-Meier estimate at every
    sample's own time from cumulative sums over the tie blocks, then five n x n broadcasts (mask * w_j, summed over j)."""
    first, last, inv = masks["first"], masks["last"], masks["inv"]
    ev = sevent != 0
    out = []
    for w in W_sorted.to(torch.float64):
        cw = torch.cumsum(w, 0)
        before = torch.cat([cw.new_zeros(1), cw])[first]                       # weight before each tie block
        d = torch.zeros_like(before).index_add_(0, inv, w * ev)
        c = torch.zeros_like(before).index_add_(0, inv, w * ~ev)
        at_risk = cw[-1] - before
        f = torch.where(c > 0, (at_risk - d - c) / (at_risk - d), torch.ones_like(c))
        G = torch.cumprod(f, 0)[inv]
        use = ev & (stime < tau) & (G > 0) & (w > 0)
        ig2 = torch.where(use, w / (G * G), torch.zeros_like(G))
        K = [(m * w[None, :]).sum(dim=1) for m in masks["pairs"]]
        out.append(torch.stack([(ig2 * k).sum() for k in K] + [(w * k * ev).sum() for k in K]))
    return torch.stack(out)


def main():
    from advmil_amd import _lib
    from advmil_amd.eval import concord_rows
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    plan = [ctypes.c_int(0) for _ in range(4)]
    L.advmil_concord_rows_plan(*(ctypes.byref(x) for x in plan))
    results = []
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    for case in CASES:
        n, rows = case["n"], case["rows"]
        ev, tm, risk, surv, col, W = inputs(case)
        Q, T = surv.shape[1], 1
        # ---- section 1: the kernel's rows against the restatement ----
        limited("check")
        d = dict(ev=torch.from_numpy(ev).to(dev), tm=torch.from_numpy(tm).to(dev), risk=torch.from_numpy(risk).to(dev),
                 surv=torch.from_numpy(surv).to(dev), col=torch.from_numpy(col).to(dev), W=torch.from_numpy(W).to(dev))
        r = concord_rows(d["ev"], d["tm"], d["risk"], d["surv"], d["col"], None, d["W"])
        want = R.rows(ev, tm, risk, surv, col, None, W[:CHECK], literal=False)
        got_s = r.sums[:CHECK].cpu().numpy()
        mine_k = r.sums[:TORCH_ROWS].cpu().numpy()                              # (the timed calls below write into r's arrays)
        same = bool(np.array_equal(r.counts[:CHECK].cpu().numpy(), want["counts"]) and np.array_equal(r.rowcnt[:CHECK].cpu().numpy(), want["rowcnt"])
                    and (np.abs(got_s - want["sums"]) <= 2 * want["bound"] * want["sums"]).all())
        # ---- section 2: the two kernels, C entries alone, the sorted cohort prepared once ----
        limited("kernels")
        stime, order = torch.sort(d["tm"], stable=True)
        sevent, order32 = d["ev"][order].contiguous(), order.to(torch.int32)
        tau = torch.tensor([float("inf")], dtype=torch.float32, device=dev)
        wsb = L.advmil_concord_rows_workspace_bytes(n, rows, T)
        ws = torch.empty(wsb // 8 + 1, dtype=torch.float64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def concord(rk, sv):
            def go():
                _lib.check(L.advmil_concord_rows(p(stime), p(sevent), p(order32), n, p(d["W"]), n, rows, p(rk), p(sv), Q, Q,
                                                 p(d["col"]) if sv is not None else None, p(tau), T, p(r.counts), p(r.rowcnt), p(r.sums),
                                                 p(ws), wsb, stream), "concord_rows")
            return go
        at1 = torch.tensor([float(np.median(tm))], dtype=torch.float32, device=dev)
        wsb_i = L.advmil_ipcw_rows_workspace_bytes(n, rows, 1)
        ws_i = torch.empty(wsb_i // 8 + 1, dtype=torch.float64, device=dev)
        oc, orc, osum = (torch.empty((rows, 1, 2), dtype=torch.int64, device=dev), torch.empty((rows, 2), dtype=torch.int64, device=dev),
                         torch.empty((rows, 1, 6), dtype=torch.float64, device=dev))

        def ipcw():
            _lib.check(L.advmil_ipcw_rows(p(stime), p(sevent), p(order32), n, p(d["W"]), n, rows, p(at1), 1, None, 0, p(d["risk"]), 1, 1,
                                          p(oc), p(orc), p(osum), p(ws_i), wsb_i, stream), "ipcw_rows")
        fns = dict(concord_both=concord(d["risk"], d["surv"]), concord_risk=concord(d["risk"], None), concord_surv=concord(None, d["surv"]),
                   ipcw_q1_risk=ipcw)
        times = {k: [] for k in fns}
        for _ in range(PASSES):
            for k, fn in fns.items():
                times[k].append(timed(fn))
        # the pairs each pair pass visits, per row (cases are the event samples; a thread per sorted sample either way)
        st, se = stime.cpu().numpy(), sevent.cpu().numpy() != 0
        tile = plan[2].value
        jstart = np.searchsorted(st, st[(np.arange(n) // tile) * tile], side="left")
        pairs_concord = int((n - jstart)[se].sum())
        k0 = int(np.searchsorted(st, float(at1[0]), side="right"))
        pairs_ipcw = int(se[:k0].sum()) * (n - k0)
        # ---- section 3: plain torch on the device ----
        limited("torch")
        ss = d["surv"][order]
        sc = d["col"][order].to(torch.int64)
        sr = d["risk"][order]
        uniq, inv = torch.unique_consecutive(stime, return_inverse=True)
        cnt = torch.bincount(inv)
        last = torch.cumsum(cnt, 0) - 1
        first = last - cnt + 1
        evb = sevent != 0
        comp = ((stime[None, :] > stime[:, None]) | ((stime[None, :] == stime[:, None]) & ~evb[None, :])) & evb[:, None]
        mine, theirs = ss[torch.arange(n, device=dev), sc], ss[:, sc].t()          # theirs[i, j] = surv[j, col[i]]
        masks = dict(first=first, last=last, inv=inv,
                     pairs=[comp, comp & (sr[:, None] > sr[None, :]), comp & (sr[:, None] == sr[None, :]),
                            comp & (mine[:, None] < theirs), comp & (mine[:, None] == theirs)])
        Ws = d["W"][:TORCH_ROWS][:, order]
        ref_t = torch_rows(stime, sevent, masks, Ws, tau[0]).cpu().numpy()
        torch_agrees = bool(np.allclose(ref_t[:, :5], np.stack([mine_k[:, 0, 0, 2], mine_k[:, 0, 0, 0], mine_k[:, 0, 0, 1], mine_k[:, 1, 0, 0],
                                                                mine_k[:, 1, 0, 1]], axis=1), rtol=1e-10, atol=0))
        t_torch = timed(lambda: torch_rows(stime, sevent, masks, Ws, tau[0]), repeats=5)
        signal.alarm(0)
        slow = lambda ps: max(x["median_ms"] for x in ps)      # noqa: E731
        both, rk, ip = slow(times["concord_both"]), slow(times["concord_risk"]), slow(times["ipcw_q1_risk"])
        row = dict(case, Q=int(Q), T=T, plan=dict(walk_rows=plan[0].value, walk_trip=plan[1].value, pair_tile=plan[2].value, pair_rows=plan[3].value),
                   rows_equal_restatement=same, rows_checked=CHECK, torch_agrees=torch_agrees, times=times, torch_rows_timed=TORCH_ROWS,
                   torch=t_torch, pairs_per_row_concord=pairs_concord, pairs_per_row_ipcw=pairs_ipcw,
                   concord_both_ms=both, concord_risk_ms=rk, ipcw_ms=ip, torch_ms_scaled_to_all_rows=t_torch["median_ms"] * rows / TORCH_ROWS,
                   ps_per_row_pair_concord_both=1e9 * both / (rows * pairs_concord), ps_per_row_pair_concord_risk=1e9 * rk / (rows * pairs_concord),
                   ps_per_row_pair_ipcw=1e9 * ip / (rows * pairs_ipcw),
                   ratio_risk_vs_ipcw_per_row_pair=(rk / pairs_concord) / (ip / pairs_ipcw),
                   ratio_both_vs_ipcw_per_row_pair=(both / pairs_concord) / (ip / pairs_ipcw),
                   ratio_torch_vs_concord_both=t_torch["median_ms"] * rows / TORCH_ROWS / both)
        results.append(row)
        print(json.dumps(row), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
