"""The oracle of the greedy k-means++ seeding (advmil_amd/csrc/kmeans.hip kmeans_seed_*, advmil_amd/wsicluster.py seed_rows_greedy) and
of the n_init selection: numpy float64, one bag at a time, a restatement of sklearn 1.7's _kmeans_plusplus and KMeans.fit.

  draws      ONE np.random.RandomState(random_state) per bag; per init, in order: choice(n, p=full(1 / n)) for the first centre, then
             K - 1 times uniform(size=L), L = 2 + int(ln K). Consecutive inits continue the stream.
  seed       closest = dist2 to the first centre. Per pick: cum = cumsum(closest); the L trial rows are
             min(searchsorted(cum, u * cum[-1], side="left"), n - 1); m_l = minimum(closest, dist2 to trial l); pot_l = sum(m_l);
             best = argmin(pot) (first minimum); the pick is trial `best`, closest = m_best.
             (sklearn multiplies u by closest @ weight where this takes cum[-1]: the same number on data whose sums are exact.)
  select     run i replaces the best so far when its inertia is lower AND its labels are not the best's up to a relabelling
             (_is_same_clustering).
NOT restated: the relocation of an empty cluster, the float32 arithmetic of float32 input, and X -= X.mean(0) -- on the recorded cases
the float64 distances of the raw rows give sklearn's picks (tests/test_kmeans_greedy_cpu.py asserts it).

Decidability (real-valued data, `delta`): the device forms every distance within delta_il of the float64 one (the bound of
tests/test_kmeans_gpu.py::deltas). As long as the picks agree, the device's closest_i lies within e_i = the largest delta of row i
against the centres picked so far of the oracle's, and m_il within max(e_i, delta_il). A draw is decidable when cum_k >= u * total
(written as (1 - u) cum_k - u (total - cum_k) >= 0, two sums over disjoint rows) holds for its row k, and fails for row k - 1, under
EVERY such perturbation, by more than the rounding of the float64 additions in any order; an argmin is decidable when the best
trial's largest potential is below the smallest potential of every trial that is a different row."""
import numpy as np

from tests import kmeans_ref as R


def trials(K):
    return 2 + int(np.log(K))


def draws(random_state, n_rows, K, n_init=1):
    """-> [(first, u float64 [K - 1, L])] per init, from one RandomState."""
    rs = np.random.RandomState(random_state)
    out = []
    for _ in range(n_init):
        first = int(rs.choice(n_rows, p=np.full(n_rows, 1.0 / n_rows)))
        out.append((first, np.array([rs.uniform(size=trials(K)) for _ in range(K - 1)], dtype=np.float64).reshape(K - 1, trials(K))))
    return out


def seed(x, K, first, u, delta=None):
    """-> dict(rows [K], closest [n], pot0, pot [K - 1, L], cand [K - 1, L], best [K - 1]; with delta(x, cent) -> [n, k] also
    draw_ok bool [K - 1, L], pick_ok bool [K - 1], err [n] = e_i after the last pick)."""
    x = np.asarray(x, dtype=np.float64)
    n, L = x.shape[0], trials(K)
    closest = R.dist2(x, x[[first]])[:, 0]
    err = delta(x, x[[first]])[:, 0] if delta is not None else np.zeros(n)
    rows, pot0 = [int(first)], float(closest.sum())
    pots, cands, bests = np.zeros((K - 1, L)), np.zeros((K - 1, L), dtype=np.int64), np.zeros(K - 1, dtype=np.int64)
    draw_ok, pick_ok = np.ones((K - 1, L), dtype=bool), np.ones(K - 1, dtype=bool)
    for p in range(1, K):
        cum = np.cumsum(closest)
        total = cum[-1]
        target = np.asarray(u[p - 1], dtype=np.float64) * total
        cand = np.minimum(np.searchsorted(cum, target, side="left"), n - 1)
        if delta is not None:
            slack = n * 2.0 ** -52
            lo, hi = np.cumsum(np.maximum(closest - err, 0.0)), np.cumsum(closest + err)
            margin = 4 * slack * hi[-1]                                     # the roundings of cum_k, of total and of u * total
            for l, k in enumerate(cand):
                v = float(u[p - 1][l])
                # cum_k >= v total  <=>  (1 - v) cum_k - v (total - cum_k) >= 0: head and tail are sums over disjoint rows
                reaches = k == n - 1 or (1 - v) * lo[k] - v * (hi[-1] - hi[k]) > margin          # (the last row is taken whatever its prefix)
                draw_ok[p - 1, l] = reaches and (k == 0 or (1 - v) * hi[k - 1] - v * (lo[-1] - lo[k - 1]) < -margin)
        M = np.minimum(closest[:, None], R.dist2(x, x[cand]))
        pot = M.sum(axis=0)
        best = int(np.argmin(pot))
        if delta is not None:
            e = np.maximum(err[:, None], delta(x, x[cand]))
            p_lo, p_hi = np.maximum(M - e, 0.0).sum(axis=0) * (1 - slack), (M + e).sum(axis=0) * (1 + slack)
            pick_ok[p - 1] = all(p_hi[best] < p_lo[l] for l in range(L) if cand[l] != cand[best])
            err = e[:, best]
        pots[p - 1], cands[p - 1], bests[p - 1] = pot, cand, best
        rows.append(int(cand[best]))
        closest = M[:, best]
    out = dict(rows=rows, closest=closest, pot0=pot0, pot=pots, cand=cands, best=bests)
    if delta is not None:
        out.update(draw_ok=draw_ok, pick_ok=pick_ok, err=err)
    return out


def same_clustering(a, b, K):
    """sklearn's _is_same_clustering: every label of a maps to ONE label of b."""
    a, b = np.asarray(a), np.asarray(b)
    return all(len(np.unique(b[a == j])) <= 1 for j in range(K))


def select(runs, K):
    """The index of the run KMeans.fit keeps: runs = [dict(labels, inertia, ...)] in init order."""
    best = 0
    for i in range(1, len(runs)):
        if runs[i]["inertia"] < runs[best]["inertia"] and not same_clustering(runs[i]["labels"], runs[best]["labels"], K):
            best = i
    return best


def kmeans(x, K, random_state=42, n_init=1, max_iter=300, tol=1e-4):
    """KMeans(K, random_state=random_state, n_init=n_init) on one bag -> the kept run of kmeans_ref.lloyd, plus rows (its seed rows),
    init_index, and all_rows (the seed rows of every init)."""
    runs = []
    for first, u in draws(random_state, x.shape[0], K, n_init):
        rows = seed(x, K, first, u)["rows"]
        r = R.lloyd(x, np.asarray(x, dtype=np.float64)[rows], max_iter, tol)
        r["rows"] = rows
        runs.append(r)
    i = select(runs, K)
    return dict(runs[i], init_index=i, all_rows=[r["rows"] for r in runs])
