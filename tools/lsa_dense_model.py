#!/usr/bin/env python
"""CPU model of the dense assignment solver (gd4d_lsa_dense_fwd): counts the SEQUENTIAL scan steps each scheme needs.

One scan step = one pass over a row's remaining columns followed by a workgroup-wide arg-min - the unit whose latency (a row
read from L2, a reduction, a barrier) bounds a one-workgroup-per-problem solver.  Schemes:

  sap      scipy's shortest augmenting path from zero duals, one Dijkstra per row (what gd4d_hungarian_assign_fwd runs);
  dense    the new kernel: a parallel warm start (square: column reduction - v_j = min_i c_ij, every column offers itself to its
           arg-min row, the row keeps the lowest such column; rectangular: row reduction - u_i = min_j c_ij, v = 0, the row
           takes its arg-min column if no lower row took it), then one Dijkstra per row left free, from those duals.

The warm start costs no sequential steps in this count (one parallel pass over the matrix).  Both schemes are exact; the model
also checks that every scheme reaches scipy's optimum.

    python tools/lsa_dense_model.py [--n 900] [--seeds 3]
"""
import argparse

import numpy as np


def families(n, seed):
    """The two seeded families of tools/bench_distill_match.py: 'independent' (student query order unrelated to the teacher's)
    and 'noise' (student = teacher + small noise)."""
    g = np.random.default_rng(seed)
    t = g.standard_normal((n, 8)).astype(np.float32)
    s_ind = g.standard_normal((n, 8)).astype(np.float32)
    s_noise = (t + 0.05 * g.standard_normal((n, 8))).astype(np.float32)
    cost = lambda s: np.abs(s[:, None, :] - t[None, :, :]).sum(-1).astype(np.float32)  # noqa: E731
    return {'independent': cost(s_ind), 'noise': cost(s_noise)}


def dijkstra(c, u, v, col4row, row4col, cur):
    """One shortest augmenting path from free row `cur` (scipy's inner loop, vectorised per scan step).  Returns the steps."""
    nr, nc = c.shape
    shortest = np.full(nc, np.inf)
    path = np.full(nc, -1)
    sc = np.zeros(nc, bool)
    sr = np.zeros(nr, bool)
    min_val, i, sink, steps = 0.0, cur, -1, 0
    while sink < 0:
        steps += 1
        sr[i] = True
        r = min_val + c[i] - u[i] - v
        upd = (~sc) & (r < shortest)
        shortest[upd] = r[upd]
        path[upd] = i
        cand = np.where(sc, np.inf, shortest)
        low = cand.min()
        if low == np.inf:
            raise RuntimeError('infeasible')
        ties = np.flatnonzero(cand == low)
        free = ties[row4col[ties] < 0]
        j = int(free[0]) if free.size else int(ties[0])
        min_val = low
        sc[j] = True
        if row4col[j] < 0:
            sink = j
        else:
            i = row4col[j]
    u[cur] += min_val
    rows = np.flatnonzero(sr)
    rows = rows[rows != cur]
    u[rows] += min_val - shortest[col4row[rows]]
    v[sc] -= min_val - shortest[sc]
    j = sink
    while True:
        r = path[j]
        row4col[j] = r
        col4row[r], j = j, col4row[r]
        if r == cur:
            break
    return steps


def solve(c, scheme):
    c = c.astype(np.float64)
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    if scheme == 'dense':
        if nr == nc:
            v = c.min(0)
            arg = c.argmin(0)
            for j in range(nc):                                   # the lowest offering column wins the row
                if col4row[arg[j]] < 0:
                    col4row[arg[j]], row4col[j] = j, arg[j]
        else:
            u = c.min(1)
            arg = c.argmin(1)
            for i in range(nr):                                   # the lowest claiming row wins the column
                if row4col[arg[i]] < 0:
                    row4col[arg[i]], col4row[i] = i, arg[i]
    free = np.flatnonzero(col4row < 0)
    steps = sum(dijkstra(c, u, v, col4row, row4col, int(i)) for i in free)
    return col4row, steps, int(free.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=900)
    ap.add_argument('--seeds', type=int, default=3)
    a = ap.parse_args()
    from scipy.optimize import linear_sum_assignment
    for seed in range(a.seeds):
        for fam, c in families(a.n, seed).items():
            _, ref = linear_sum_assignment(c)
            out = []
            for scheme in ('sap', 'dense'):
                col, steps, free = solve(c, scheme)
                assert np.array_equal(col, ref), (fam, scheme)
                out.append(f'{scheme}: {steps:6d} steps ({free} free rows)')
            print(f'seed {seed} {fam:12s} ' + '   '.join(out))


if __name__ == '__main__':
    main()
