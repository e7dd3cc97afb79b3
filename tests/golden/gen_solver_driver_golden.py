#!/usr/bin/env python3
"""Writes tests/golden/solver_driver.npz from ``solver.drive_host``, table-free: for every case of
tests/solver_driver_cases.py -- the chosen roots, the windows, driver_plies, the quota and the budget -- the per-row answers
and the per-node report.  The open roots of tests/golden/solver_open.npz come last, with the window (-1, 1) and
driver_plies = 2: the first OPEN_ROOTS of them, hardest first among those one lane solves in 2^20 nodes, every leaf of which
``solve_host`` answers within 2^16 nodes (found by running it here), at the quota 256 and at the default one.

    python tests/golden/gen_solver_driver_golden.py          # a few minutes of plain Python, no GPU
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import solver_driver_cases as D  # noqa: E402
from connect4_amd import solver as S  # noqa: E402


def memoised(leaf_solver):
    memo = {}

    def solve(*key):
        if key not in memo:
            memo[key] = leaf_solver(*key)
        return memo[key]
    return solve


LEAF = memoised(S._host_leaf)


def run(case):
    res, rep = S.drive_host(case.rows, case.alpha, case.beta, case.plies, node_budget=case.budget, nodes_per_launch=case.quota, leaf_solver=LEAF)
    return res, rep


def main():
    z = D.exact_rows()
    cases = D.fixed_cases(z)
    o = np.load(os.path.join(HERE, "solver_open.npz"))
    found = 0
    for i in np.argsort(-o["nodes"], kind="stable"):
        if found == D.OPEN_ROOTS:
            break
        if o["nodes"][i] > 1 << 20:
            continue
        rows = np.array([[o["c0"][i], o["c1"][i]]], dtype=np.uint64)
        probe = D.Case("probe", rows, np.array([-1], dtype=np.int8), np.array([1], dtype=np.int8), 2, D.DEFAULT_QUOTA, D.OPEN_LEAF_BUDGET)
        t0 = time.time()
        g = S._build_graph(rows, probe.alpha, probe.beta, 2, S._children_host)
        wa, wb = S._graph_windows(g)
        first = int(g.level_start[-2])
        ok = all(LEAF(int(g.color0[j]), int(g.color1[j]), int(wa[j]), int(wb[j]), D.OPEN_LEAF_BUDGET)[0] != S.L.SOLVE_UNKNOWN
                 for j in range(first, len(g.child)))
        print("open root %d (%d nodes alone): %s, %.0f s" % (i, o["nodes"][i], "taken" if ok else "a leaf passes 2^16 nodes", time.time() - t0), flush=True)
        if ok:
            found += 1
            for quota in (256, D.DEFAULT_QUOTA):
                cases.append(D.Case("open%d_q%d" % (i, quota), rows, probe.alpha, probe.beta, 2, quota, D.AMPLE))
    out = {"names": np.array([c.name for c in cases])}
    for n, case in enumerate(cases):
        t0 = time.time()
        res, rep = run(case)
        p = "c%02d__" % n
        out.update({p + "rows": case.rows, p + "alpha": case.alpha, p + "beta": case.beta, p + "plies": np.int64(case.plies),
                    p + "quota": np.int64(case.quota), p + "budget": np.int64(case.budget)})
        out.update({p + f: getattr(res, f) for f in D.ROW_FIELDS})
        out.update({p + "lo": rep["lo"], p + "hi": rep["hi"], p + "state": rep["state"], p + "node_nodes": rep["nodes"]})
        print("%-22s %4d rows %6d nodes of the graph, %d launches, states %s, %.1f s" % (
            case.name, len(case.rows), len(rep["state"]), rep["launches"], np.bincount(rep["state"], minlength=5).tolist(), time.time() - t0), flush=True)
    path = os.path.join(HERE, "solver_driver.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
