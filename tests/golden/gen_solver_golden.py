#!/usr/bin/env python3
"""Generate the solver's fixtures under tests/golden/.

    python gen_solver_golden.py          solver.npz, from the UNMODIFIED reference (import path as for gen_golden.py:
                                         PYTHONPATH=<repo>/oracle/refshim:<reference>)
    python gen_solver_golden.py deep     solver_deep.npz, from this project's solve_host (PYTHONPATH=<repo>)

solver.npz -- the reference's exact answers.  GridSearch(plies=e, Evaluator(lambda b: 0.5)).make_move on seeded random
legal undecided positions with e = 3..10 empty squares (with plies = e no evaluator is reached, grid_search.py:38-71), N_PER_E
per e.  Per position: c0, c1 (the colours), move, value (the returned pair), root_search (the root's search_value),
child_names int8 [7] (the root's children in order, -1 padded) and child_abs float64 [7] (their absolute_value, NaN padded).
Only data: inputs and the reference's outputs.

solver_deep.npz -- 256 seeded random positions with 12..20 empty squares, answered by connect4_amd.solver.solve_host: c0, c1,
outcome, final_age, value, nodes (solve_host's node counts).  Only positions that solve_host answers in at most 2^17 nodes
are kept.  Of the 256 candidates drawn (seed 20, empties cycling 12..20) none was discarded: the hardest took 114,980.
"""
import os
import sys
from copy import copy

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
N_PER_E = 8
DEEP_N = 256
DEEP_MAX_NODES = 1 << 17


def reference_fixture():
    from oinkoink.board import Board
    from oinkoink.evaluators import Evaluator
    from oinkoink.grid_search import GridSearch

    def random_position(rng, plies):
        while True:
            b = Board()
            ok = True
            for _ in range(plies):
                moves = sorted(b.valid_moves)
                if not moves:
                    ok = False
                    break
                b.make_move(int(rng.choice(moves)))
            if ok and b.result is None:
                return b

    rng = np.random.RandomState(4242)
    rows = []
    for e in range(3, 11):
        player = GridSearch("exact", e, Evaluator(lambda b: 0.5))
        for _ in range(N_PER_E):
            b = random_position(rng, 42 - e)
            move, value, tree = player.make_move(copy(b))
            names = [int(c.name) for c in tree.root.children]
            vals = [float(c.data.absolute_value) for c in tree.root.children]
            rows.append((int(b.color[0]), int(b.color[1]), int(move), float(value), float(tree.root.data.search_value),
                         names + [-1] * (7 - len(names)), vals + [np.nan] * (7 - len(vals))))
    np.savez_compressed(os.path.join(OUT, "solver.npz"),
                        c0=np.array([r[0] for r in rows], dtype=np.uint64), c1=np.array([r[1] for r in rows], dtype=np.uint64),
                        move=np.array([r[2] for r in rows], dtype=np.int32), value=np.array([r[3] for r in rows], dtype=np.float64),
                        root_search=np.array([r[4] for r in rows], dtype=np.float64),
                        child_names=np.array([r[5] for r in rows], dtype=np.int8),
                        child_abs=np.array([r[6] for r in rows], dtype=np.float64))
    print("solver.npz: %d positions" % len(rows))


def deep_fixture():
    from connect4_amd.solver import random_playout, solve_host
    from connect4_amd import _lib as L
    rng = np.random.RandomState(20)
    rows, drawn = [], 0
    while len(rows) < DEEP_N:
        e = 12 + drawn % 9
        drawn += 1
        b = random_playout(rng, 42 - e)
        a = solve_host(b, node_budget=DEEP_MAX_NODES)
        if a.status != L.SOLVE_SOLVED:
            continue
        rows.append((b.color[0], b.color[1], a.outcome, a.final_age, a.value, a.nodes))
    np.savez_compressed(os.path.join(OUT, "solver_deep.npz"),
                        c0=np.array([r[0] for r in rows], dtype=np.uint64), c1=np.array([r[1] for r in rows], dtype=np.uint64),
                        outcome=np.array([r[2] for r in rows], dtype=np.float64), final_age=np.array([r[3] for r in rows], dtype=np.int8),
                        value=np.array([r[4] for r in rows], dtype=np.float64), nodes=np.array([r[5] for r in rows], dtype=np.int64))
    print("solver_deep.npz: %d positions kept, %d of %d candidates discarded (more than %d nodes); max nodes %d" % (
        len(rows), drawn - len(rows), drawn, DEEP_MAX_NODES, max(r[5] for r in rows)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "deep":
        deep_fixture()
    else:
        reference_fixture()
