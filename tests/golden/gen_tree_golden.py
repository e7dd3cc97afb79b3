#!/usr/bin/env python3
"""Generate tests/golden/search_trees.npz: WHOLE search trees of the unmodified reference.

Run where the reference is importable (it never travels to the GPU box), as gen_grid_golden.py:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=oracle/refshim:$REF python tests/golden/gen_tree_golden.py

It re-runs the searches that search_centre.json (simulations <= 3200) and search_net.json already pin -- same
board, config and recorded noise; net cases answer from search_net_tables.npz, no checkpoint needed -- and asserts
that each re-run reproduces the pinned root before anything is written.  A few positions 30 or more plies deep are
added (terminal children, full columns, trees that reach the end of the game, a root with a winning move).
Only numbers are written, and only search_trees.npz; every other fixture stays as it is.

Per case NAME, the tree as a table in breadth-first order (within a level by parent, within a parent by ascending
column, i.e. the order of node.children):
  NAME__board     uint64 [2]   color0, color1 of the root
  NAME__config    float64 [6]  simulations, pb_c_base, pb_c_init, root_dirichlet_alpha, root_exploration_fraction,
                               num_sampling_moves
  NAME__noise     float64 [7]  the Gamma draws of the root noise (noisy cases only)
  NAME__parent    int32 [n]    row of the parent, -1 for the root
  NAME__move      int8 [n]     node.name (-1 for the root)
  NAME__visits    int32 [n]    search_value.visit_count (0: search_value is None)
  NAME__value_sum float64 [n]  search_value.value_sum
  NAME__status    int8 [n]     -1 undecided, else board.result.value * 2
  NAME__prior_kind int8 [n]    0 position_value is None, 1 its prior is float32, 2 float64
  NAME__prior32   float32 [k1][7]  the priors of the kind-1 nodes, in table order
  NAME__prior64   float64 [k2][7]  the priors of the kind-2 nodes, in table order
and `names` / `kinds` ("centre", "net", "deep") listing the cases.  Boards are not stored: replay the moves.
"""
import json
import os
from collections import deque

import numpy as np

from oinkoink.board import Board
from oinkoink.evaluators import Evaluator, evaluate_centre_with_prior
from oinkoink.mcts import MCTSConfig, search

OUT = os.path.dirname(os.path.abspath(__file__))
MAX_SIMS = 3200


def board_from_bits(c0, c1):
    o = np.zeros((6, 7), dtype=np.bool_)
    x = np.zeros((6, 7), dtype=np.bool_)
    for c in range(7):
        for r in range(6):       # row 0 = top
            bit = 1 << (c * 7 + (5 - r))
            o[r, c] = bool(c0 & bit)
            x[r, c] = bool(c1 & bit)
    b = Board.from_pieces(o, x)
    assert int(b.color[0]) == c0 and int(b.color[1]) == c1 and b.result is None
    return b


def config_of(d):
    return MCTSConfig(d["simulations"], d["pb_c_base"], d["pb_c_init"], d["root_dirichlet_alpha"],
                      d["root_exploration_fraction"], d["num_sampling_moves"])


def config_row(c):
    return np.array([c.simulations, c.pb_c_base, c.pb_c_init, c.root_dirichlet_alpha, c.root_exploration_fraction,
                     c.num_sampling_moves], dtype=np.float64)


class RecordedGamma:
    """np.random.gamma answers the case's recorded draws for the duration of one search."""

    def __init__(self, noise):
        self.noise = noise

    def __enter__(self):
        self._g = np.random.gamma
        if self.noise is not None:
            draws = [np.array(self.noise, dtype=np.float64)]
            np.random.gamma = lambda *a, **k: draws.pop(0)
        return self

    def __exit__(self, *exc):
        np.random.gamma = self._g


def raising_fn(board):
    raise AssertionError("position missing from the recorded table")


def table_evaluator(npz, name):
    # the value as a Python float, as evaluate_nn hands it over (evaluators.py:41-44): a numpy.float32 would make
    # the reference sum in float32 under NumPy >= 2
    table = {(int(a), int(b)): (float(v), p.copy())
             for a, b, v, p in zip(npz[name + "__c0"], npz[name + "__c1"], npz[name + "__v"], npz[name + "__p"])}
    return Evaluator(raising_fn, position_table=table)


def tree_table(tree):
    rows, order = [], deque([(tree.root, -1)])
    while order:
        node, parent = order.popleft()
        me = len(rows)
        rows.append((node, parent))
        for c in sorted(node.children, key=lambda c: c.name):
            order.append((c, me))
    n = len(rows)
    t = dict(parent=np.full(n, -1, dtype=np.int32), move=np.full(n, -1, dtype=np.int8), visits=np.zeros(n, dtype=np.int32),
             value_sum=np.zeros(n, dtype=np.float64), status=np.full(n, -1, dtype=np.int8),
             prior_kind=np.zeros(n, dtype=np.int8))
    p32, p64 = [], []
    for i, (node, parent) in enumerate(rows):
        d = node.data
        if not node.is_root:
            assert rows[parent][0] is node.parent
            t["parent"][i] = parent
            t["move"][i] = node.name
        if d.search_value is not None:
            t["visits"][i] = d.search_value.visit_count
            t["value_sum"][i] = d.search_value.value_sum
            assert isinstance(d.search_value.value_sum, float) or d.search_value.value_sum.dtype == np.float64
        if d.board.result is not None:
            t["status"][i] = int(d.board.result.value * 2)
        if d.position_value is not None:
            pr = np.asarray(d.position_value.prior)
            assert pr.shape == (7,) and pr.dtype in (np.float32, np.float64)
            if pr.dtype == np.float32:
                t["prior_kind"][i] = 1
                p32.append(pr.copy())
            else:
                t["prior_kind"][i] = 2
                p64.append(pr.copy())
    t["prior32"] = np.array(p32, dtype=np.float32).reshape(-1, 7)
    t["prior64"] = np.array(p64, dtype=np.float64).reshape(-1, 7)
    return t


def assert_matches_json(tree, t, case):
    """The re-run is the pinned search: root row, root children, policies' inputs, node and expansion counts."""
    root = tree.root
    assert int(t["visits"][0]) == case["root_N"] and float(t["value_sum"][0]) == case["root_W"], case["name"]
    N, W, status = [0] * 7, [0.0] * 7, [-2] * 7
    for i in np.nonzero(t["parent"] == 0)[0]:
        m = int(t["move"][i])
        N[m], W[m], status[m] = int(t["visits"][i]), float(t["value_sum"][i]), int(t["status"][i])
    assert N == case["N"] and W == case["W"] and status == case["status"], case["name"]
    assert [float(x) for x in root.data.position_value.prior] == case["root_prior"], case["name"]
    assert len(t["parent"]) == case["n_nodes"], case["name"]
    has_children = np.zeros(len(t["parent"]), dtype=bool)
    has_children[t["parent"][1:]] = True
    assert int(has_children.sum()) == case["n_expansions"], case["name"]


def run_case(name, board, cfg, evaluator, noise):
    with RecordedGamma(noise):
        tree = search(cfg, board, evaluator)
    t = tree_table(tree)
    t["board"] = np.array([int(board.color[0]), int(board.color[1])], dtype=np.uint64)
    t["config"] = config_row(cfg)
    if noise is not None:
        t["noise"] = np.array(noise, dtype=np.float64)
    return tree, t


def deep_position(rng, plies):
    while True:
        b = Board()
        for _ in range(plies):
            moves = sorted(b.valid_moves)
            if not moves:
                break
            b.make_move(int(rng.choice(moves)))
        if b.result is None and b.age == plies:
            return b


def main():
    blobs, names, kinds = {}, [], []

    def keep(name, kind, t):
        names.append(name)
        kinds.append(kind)
        for k, a in t.items():
            blobs["%s__%s" % (name, k)] = a

    with open(os.path.join(OUT, "search_centre.json")) as f:
        centre = [c for c in json.load(f) if c["config"]["simulations"] <= MAX_SIMS]
    for case in centre:
        b = board_from_bits(case["board"]["c0"], case["board"]["c1"])
        tree, t = run_case(case["name"], b, config_of(case["config"]), Evaluator(evaluate_centre_with_prior), case["noise"])
        assert_matches_json(tree, t, case)
        keep(case["name"], "centre", t)

    npz = np.load(os.path.join(OUT, "search_net_tables.npz"), allow_pickle=False)
    with open(os.path.join(OUT, "search_net.json")) as f:
        net = json.load(f)
    for case in net:
        b = board_from_bits(case["board"]["c0"], case["board"]["c1"])
        tree, t = run_case(case["name"], b, config_of(case["config"]), table_evaluator(npz, case["name"]), case["noise"])
        assert_matches_json(tree, t, case)
        keep(case["name"], "net", t)

    # late positions: terminal children, full columns, trees that run into the end of the game
    rng = np.random.RandomState(2024)
    wins = full = draws = 0
    for i, plies in enumerate((30, 32, 34, 36, 38, 39, 33, 31)):
        b = deep_position(rng, plies)
        sims = 800 if i % 2 else 200
        tree, t = run_case("deep%d_p%d_s%d" % (i, plies, sims), b, MCTSConfig(sims), Evaluator(evaluate_centre_with_prior), None)
        mover_wins = 2 if b.age % 2 == 0 else 0
        wins += any(int(t["status"][j]) == mover_wins for j in np.nonzero(t["parent"] == 0)[0])
        full += len(b.valid_moves) < 7
        draws += bool((t["status"] == 1).any())
        keep("deep%d_p%d_s%d" % (i, plies, sims), "deep", t)
    assert wins >= 1 and full >= 1 and draws >= 1, (wins, full, draws)

    blobs["names"] = np.array(names)
    blobs["kinds"] = np.array(kinds)
    out = os.path.join(OUT, "search_trees.npz")
    np.savez_compressed(out, **blobs)
    total = sum(len(blobs[n + "__parent"]) for n in names)
    print("%d trees, %d nodes, %d bytes -> %s" % (len(names), total, os.path.getsize(out), out))
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
