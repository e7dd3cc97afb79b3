#!/usr/bin/env python3
"""Generate tests/golden/grid_search.json by running the UNMODIFIED reference's GridSearch
(oinkoink/grid_search.py:10-35) on fixed and seeded positions.  Same set-up as gen_golden.py, from the
repository root, with REF a checkout of the reference:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=oracle/refshim:$REF python tests/golden/gen_grid_golden.py

Every case records the root position, depth and evaluator, and what the reference returned: the move, the
returned value (the chosen child's absolute_value), the 7 root children's get_node_value (None for an
illegal column) and the root's search_value.  Floats are float64 and round-trip exactly through JSON.
Cases: the 7 positions of the reference's test_grid_next_move (tests/player_test.py:126-148, with their
accepted moves), seeded random positions at depths 1-4 and 5, near-full positions searched 8-20 plies deep
and a few with Evaluator(lambda b: 0.5) (scripts/generate_7ply.py's return_half).
"""
import json
import os
import time
from copy import copy

import numpy as np

from oinkoink.board import Board
from oinkoink.evaluators import Evaluator, evaluate_centre
from oinkoink.grid_search import GridSearch

OUT = os.path.dirname(os.path.abspath(__file__))


def return_half(board):
    return 0.5


EVALS = {"centre": evaluate_centre, "half": return_half}


def run_case(b, plies, ev, **extra):
    g = GridSearch("golden", plies, Evaluator(EVALS[ev]))
    bc = copy(b)
    move, value, tree = g.make_move(bc)
    child = [None] * 7
    for c in tree.root.children:
        child[int(c.name)] = float(tree.get_node_value(c))
    d = dict(c0=int(b.color[0]), c1=int(b.color[1]), plies=int(plies), eval=ev, move=int(move),
             value=float(value), child_values=child, root_value=float(tree.root.data.search_value))
    d.update(extra)
    return d


def random_position(rng, n_moves):
    while True:
        b = Board()
        for _ in range(n_moves):
            mv = sorted(b.valid_moves)
            b.make_move(int(rng.choice(mv)))
            if b.result is not None:
                break
        if b.result is None:
            return b


def tree_size(b, plies, cap):
    """Number of nodes the reference will create (gives up past cap)."""
    n = 1
    stack = [(b, plies)]
    while stack:
        x, p = stack.pop()
        if p == 0 or x.result is not None:
            continue
        for m in x.valid_moves:
            y = copy(x)
            y.make_move(m)
            n += 1
            if n > cap:
                return n
            stack.append((y, p - 1))
    return n


def main():
    with open(os.path.join(OUT, "ref_tests.json")) as f:
        player = json.load(f)["player"]
    cases = []
    t0 = time.time()
    for i, p in enumerate(player):
        b = Board.from_pieces(np.array(p["o"], dtype=bool), np.array(p["x"], dtype=bool))
        cases.append(run_case(b, p["plies"], "centre", kind="player", ans=p["ans"]))
    print("player", time.time() - t0, flush=True)

    rng = np.random.RandomState(20261016)
    for i in range(200):
        plies = 1 + i % 4
        cases.append(run_case(random_position(rng, int(rng.randint(0, 30))), plies, "centre", kind="random"))
    print("random 1-4", time.time() - t0, flush=True)
    for i in range(16):
        cases.append(run_case(random_position(rng, int(rng.randint(0, 24))), 5, "centre", kind="random5"))
    print("random 5", time.time() - t0, flush=True)
    n_deep = 0
    while n_deep < 20:
        b = random_position(rng, int(rng.randint(28, 37)))
        plies = int(rng.randint(8, 21))
        if tree_size(b, plies, 60000) > 60000:
            continue
        cases.append(run_case(b, plies, "centre", kind="deep"))
        n_deep += 1
    print("deep", time.time() - t0, flush=True)
    for i in range(12):
        cases.append(run_case(random_position(rng, int(rng.randint(0, 36))), 1 + i % 3, "half", kind="half"))
    with open(os.path.join(OUT, "grid_search.json"), "w") as f:
        json.dump(dict(source="oinkoink.grid_search.GridSearch (unmodified)", cases=cases), f)
    print("%d cases, %.1f s" % (len(cases), time.time() - t0))


if __name__ == "__main__":
    main()
