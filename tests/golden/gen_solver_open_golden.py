#!/usr/bin/env python3
"""Generate tests/golden/solver_open.npz: positions with 25..32 empty squares and their children, answered table-free by
this project's host mirror of the solver (connect4_amd.solver.solve_host(deep=True), i.e. solver._Search).  CPU only.

    PYTHONPATH=<repo> python tests/golden/gen_solver_open_golden.py

Per empty-square count e = 25..32: candidates come from ``random_playout(RandomState(SEED + e), 42 - e)``; one is kept if it
and every one of its legal children are answered within CAP = 2^18 nodes each (a finished child answers for itself); the
first N_PER_E = 8 kept of at most MAX_CANDIDATES drawn make the depth's rows, and a depth must yield at least MIN_PER_E = 4.
The depths are independent (a seed each), so they run in parallel and the file does not depend on the worker count.

Arrays, n rows: c0, c1 uint64; outcome float64 (0.0 / 0.5 / 1.0); final_age int8; value float64; nodes int64; and for the
children in column order [n, 7]: child_legal int8, child_c0 / child_c1 uint64, child_status int8 (SOLVED or TERMINAL),
child_outcome, child_final_age, child_value, child_nodes (NaN / -1 / 0 in the slots of full columns)."""
import os
import sys
from multiprocessing import Pool

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 4300
N_PER_E = 8
MIN_PER_E = 4
MAX_CANDIDATES = 96
CAP = 1 << 18
EMPTIES = list(range(25, 33))


def depth_rows(e):
    from connect4_amd import _lib as L
    from connect4_amd.solver import random_playout, solve_host
    rng = np.random.RandomState(SEED + e)
    rows, drawn = [], 0
    while len(rows) < N_PER_E and drawn < MAX_CANDIDATES:
        drawn += 1
        b = random_playout(rng, 42 - e)
        a = solve_host(b, node_budget=CAP, deep=True)
        if a.status != L.SOLVE_SOLVED:
            continue
        kids, ok = [None] * 7, True
        for m in sorted(b.valid_moves):
            cb = b.__copy__()
            cb.make_move(m)
            k = solve_host(cb, node_budget=CAP, deep=True)
            if k.status not in (L.SOLVE_SOLVED, L.SOLVE_TERMINAL):
                ok = False
                break
            kids[m] = (cb.color[0], cb.color[1], k)
        if ok:
            rows.append((b.color[0], b.color[1], a, kids))
    return e, drawn, rows


def main():
    with Pool(min(len(EMPTIES), os.cpu_count() or 1)) as pool:
        per_e = pool.map(depth_rows, EMPTIES)
    rows = []
    for e, drawn, got in per_e:
        print("%d empty squares: %d kept of %d drawn; max nodes %d" % (e, len(got), drawn, max([r[2].nodes for r in got] + [0])))
        if len(got) < MIN_PER_E:
            sys.exit("fewer than %d positions at %d empty squares" % (MIN_PER_E, e))
        rows += got
    n = len(rows)
    z = {"c0": np.array([r[0] for r in rows], dtype=np.uint64), "c1": np.array([r[1] for r in rows], dtype=np.uint64),
         "outcome": np.array([r[2].outcome for r in rows], dtype=np.float64),
         "final_age": np.array([r[2].final_age for r in rows], dtype=np.int8),
         "value": np.array([r[2].value for r in rows], dtype=np.float64), "nodes": np.array([r[2].nodes for r in rows], dtype=np.int64),
         "child_legal": np.zeros((n, 7), dtype=np.int8), "child_c0": np.zeros((n, 7), dtype=np.uint64),
         "child_c1": np.zeros((n, 7), dtype=np.uint64), "child_status": np.full((n, 7), -1, dtype=np.int8),
         "child_outcome": np.full((n, 7), np.nan), "child_final_age": np.full((n, 7), -1, dtype=np.int8),
         "child_value": np.full((n, 7), np.nan), "child_nodes": np.zeros((n, 7), dtype=np.int64)}
    for i, r in enumerate(rows):
        for m, kid in enumerate(r[3]):
            if kid is None:
                continue
            k = kid[2]
            z["child_legal"][i, m] = 1
            z["child_c0"][i, m], z["child_c1"][i, m] = kid[0], kid[1]
            z["child_status"][i, m], z["child_outcome"][i, m], z["child_final_age"][i, m] = k.status, k.outcome, k.final_age
            z["child_value"][i, m], z["child_nodes"][i, m] = k.value, k.nodes
    if sorted(set(z["outcome"].tolist())) != [0.0, 0.5, 1.0]:
        sys.exit("not all three outcomes occur: %s" % sorted(set(z["outcome"].tolist())))
    np.savez_compressed(os.path.join(OUT, "solver_open.npz"), **z)
    print("solver_open.npz: %d positions, outcomes %s" % (n, np.unique(z["outcome"], return_counts=True)))


if __name__ == "__main__":
    main()
