#!/usr/bin/env python3
"""Writes tests/golden/solver_split_fold.npz: the host half of ``solve(split_plies=k)`` pinned on drawn answers, no GPU.

The cases (rows and k): the empty board at k = 1 and 3, 6 four-stone positions at k = 2, 12 nine-stone positions at k = 3, 40
positions of 30 stones at k = 3 and 20 of 38 stones at k = 8 (most descendants end the game before level k: the lower levels
thin out, the last ones are empty), each with two mirror images and three duplicates appended.  The answers of the last
level are drawn from a fixed seed -- SOLVED with probability 0.9 else UNKNOWN, any outcome code, any final age from the
node's own to 42, nodes and hits in 1..999 -- and the nodes without a child above it answer with ``solve_host(deep=True)``.

Per case the file holds rows, k, the answers per node of the graph (levels concatenated; -1, and 0 nodes and hits, where a
node is not searched) and the five arrays the fold returns, one entry a row.

The file was written at commit 4398d61 by this script with that commit's fold over per-level arrays in place of the one
below (``_split_levels`` gave the graph's nodes in the graph's order, ``_fold_split`` took each level's slice of the
answers): it pins ``_graph_fold_exact`` to that fold.  Run now, the script says whether it reproduces the file.

    python tests/golden/gen_solver_split_fold_golden.py          # seconds of plain Python
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from connect4_amd import _lib as L  # noqa: E402
from connect4_amd import solver as S  # noqa: E402
from connect4_amd.board import Board  # noqa: E402

SEED = 20261021
FIELDS = ("status", "outcome", "final_age", "nodes", "hits")


def cases():
    rng = np.random.RandomState(SEED)
    for name, stones, count, k in (("empty_k1", 0, 1, 1), ("empty_k3", 0, 1, 3), ("four_k2", 4, 6, 2), ("nine_k3", 9, 12, 3),
                                   ("thirty_k3", 30, 40, 3), ("thirtyeight_k8", 38, 20, 8)):
        boards = [S.random_playout(rng, stones) for _ in range(count)] if stones else [Board()]
        rows = np.array([b.color for b in boards], dtype=np.uint64).reshape(-1, 2)
        yield name, np.concatenate([rows, S._mirror_bits(rows[np.arange(2) % count]), rows[np.arange(3) % count]]), k, rng


def drawn_answers(g, rng):
    """(status, outcome code, final_age int8, nodes, hits int64) per node of `g`, filled where a split call searches."""
    n_nodes, first_leaf = len(g.child), int(g.level_start[-2])
    nodes = np.stack([g.color0, g.color1], axis=1)
    status, outcome, age = (np.full(n_nodes, -1, dtype=np.int8) for _ in range(3))
    count, hits = (np.zeros(n_nodes, dtype=np.int64) for _ in range(2))
    own_age = S._ages(nodes)
    for i in range(first_leaf, n_nodes):
        status[i] = L.SOLVE_SOLVED if rng.random_sample() < 0.9 else L.SOLVE_UNKNOWN
        outcome[i] = rng.randint(0, 3)
        age[i] = rng.randint(int(own_age[i]), 43)
        count[i], hits[i] = rng.randint(1, 1000), rng.randint(1, 1000)
    inner = (g.child >= 0).any(axis=1)
    for i in np.nonzero(~inner[:first_leaf])[0]:
        h = S.solve_host((int(g.color0[i]), int(g.color1[i])), deep=True)
        status[i], outcome[i], age[i] = h.status, -1 if h.outcome is None else int(h.outcome * 2), h.final_age
    return status, outcome, age, count, hits


def main():
    every = list(cases())       # all the playouts are drawn before the first answer
    out = {"names": np.array([name for name, _, _, _ in every])}
    for name, rows, k, rng in every:
        g = S._build_graph(rows, None, None, k, S._children_host)
        answers = drawn_answers(g, rng)
        folded = [a[g.inverse] for a in S._graph_fold_exact(g, *answers)]
        out.update({name + "__rows": rows, name + "__k": np.int64(k)})
        out.update({name + "__node_" + f: a for f, a in zip(FIELDS, answers)})
        out.update({name + "__" + f: a for f, a in zip(FIELDS, folded)})
        print("%-15s %3d rows, levels %s, statuses %s" % (name, len(rows), np.diff(g.level_start).tolist(),
                                                       np.bincount(folded[0], minlength=5).tolist()), flush=True)
    path = os.path.join(HERE, "solver_split_fold.npz")
    if os.path.exists(path):
        old = np.load(path, allow_pickle=False)
        same = sorted(old.files) == sorted(out) and all(old[f].dtype == np.asarray(out[f]).dtype and np.array_equal(old[f], out[f]) for f in old.files)
        print("%s: %s" % (path, "reproduced, array for array" if same else "DIFFERS from what this run computed"))
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(out["names"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
