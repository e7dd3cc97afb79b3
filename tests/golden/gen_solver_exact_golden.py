#!/usr/bin/env python3
"""Generate tests/golden/solver_exact.npz: positions with 1..22 empty squares and the answers of the exhaustive oracle
(oracle/c4_oracle.c c4o_exact_scores: every legal move of every position, a memo of exact values, nothing else).

    PYTHONPATH=<repo> python tests/golden/gen_solver_exact_golden.py

Rows: seeded ``solver.random_playout`` positions, distinct over the file, ``ROWS_PER_EMPTIES[e]`` per number e of empty
squares (512 at 1..12, 256 at 13..16, 96 at 17..18, 32 at 19..20, 16 at 21..22: 7,456 rows).  At each e the first half are
the draws as they come.  The other half are positions whose mover cannot win at once, so that the search has a tree; they
are picked from a pool of POOL_FACTOR times as many such draws, in turn one from each of the strata of
tests/solver_exact_cases.py that still has an unused pool row (the rare ones first), so that the rules enter_node adds to
minimax -- the forced block, two threats, the squares under an opposing win, the empty non-losing list -- each meet at
least STRATUM_MIN rows.  The strata are decided from the stones alone (solver_exact_cases.root_facts); the generator exits
with an error if one has fewer rows.

At e >= 19 a row is kept only if ``solver.solve_host`` answers it table-free within 2^20 nodes (the GPU test runs the
table-free kernel under that budget and allows no UNKNOWN; the node counts are the mirror's).  That selects rows only: every
value in the file is the oracle's.  Of the 96 rows picked at e >= 19, 0 were discarded on this account; over the whole file
the mirror's dearest row takes 74,256 nodes.

Columns: c0, c1 uint64; score int8, the mover's score (43 - final age for a win, final age - 43 for a loss, 0 for a draw);
child_score int8 [n, 7], the score after each move from the same side (-128: the column is full); empties int8; one bool
column per stratum, and tree (the mover cannot win at once).

Measured on an 8-core machine: this generator 1,148 s -- drawing 1,120 s (a random playout seldom reaches the last few
empty squares undecided, and each pool is POOL_FACTOR times the rows taken from it), the oracle 27 s for all 7,456 rows
through memos of 2^26 words, the mirror's filter 2 s.  tests/test_exact_oracle.py takes about 60 s: the oracle re-solves the
7,168 rows with e <= 16 in 5 s and its self-checks take 7 s; the host mirror answers all rows in 5.5 s table-free, 5.7 s with
deep=True, 3.2 s with HostTable(10), and under the six windows in 13..19 s table-free and 8..9 s with HostTable(14).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import solver_exact_cases as X  # noqa: E402

SEED = 2206
POOL_FACTOR = 8
FILTER_FROM_EMPTIES = 19
FILTER_NODES = 1 << 20
# the order of the turns: rarest first (measured root frequencies: all_under 0.7 %, block_under 3.6 %)
TURNS = ("all_under", "block_under", "two_threats", "one_nonlosing", "one_threat", "some_under", "quiet")


def main():
    from connect4_amd import _lib as L
    from connect4_amd.solver import random_playout, solve_host
    from oracle import c4oracle as O
    t_start = time.perf_counter()
    rng = np.random.RandomState(SEED)
    seen = set()
    picked = []                     # (c0, c1)
    discarded = filtered = 0
    t_filter = 0.0

    def affordable(c0, c1, e):
        nonlocal discarded, filtered, t_filter
        if e < FILTER_FROM_EMPTIES:
            return True
        t0 = time.perf_counter()
        ok = solve_host((c0, c1), node_budget=FILTER_NODES).status == L.SOLVE_SOLVED
        t_filter += time.perf_counter() - t0
        filtered += 1
        discarded += 0 if ok else 1
        return ok

    def draw(e, want, tree_only):
        out = []
        for _ in range(400 * want + 4000):
            if len(out) == want:
                return out
            b = random_playout(rng, X.SIZE - e)
            at = (int(b.color[0]), int(b.color[1]))
            if at in seen:
                continue
            if tree_only and not X.strata([at[0]], [at[1]], [0])["tree"][0]:
                continue
            seen.add(at)
            out.append(at)
        raise SystemExit("no %d distinct rows with %d empty squares" % (want, e))

    for e in sorted(X.ROWS_PER_EMPTIES):
        half = X.ROWS_PER_EMPTIES[e] // 2
        plain = []
        while len(plain) < half:
            plain += [at for at in draw(e, half - len(plain), False) if affordable(at[0], at[1], e)]
        pool = draw(e, POOL_FACTOR * half, True)
        s = X.strata([p[0] for p in pool], [p[1] for p in pool], np.zeros(len(pool)))
        s["quiet"] = s["tree"] & ~(s["one_threat"] | s["two_threats"] | s["all_under"] | s["one_nonlosing"] | s["some_under"])
        queues = {name: list(np.nonzero(s[name])[0]) for name in TURNS}
        used, treed = set(), []
        while len(treed) < half:
            progress = False
            for name in TURNS:
                while queues[name] and queues[name][0] in used:
                    queues[name].pop(0)
                if queues[name] and len(treed) < half:
                    i = queues[name].pop(0)
                    used.add(i)
                    progress = True
                    if affordable(pool[i][0], pool[i][1], e):
                        treed.append(pool[i])
            if not progress:
                raise SystemExit("the pool at %d empty squares is used up" % e)
        picked += plain + treed
        print("e = %2d: %d rows" % (e, len(plain) + len(treed)), flush=True)
    t_draw = time.perf_counter() - t_start - t_filter

    c0 = np.array([p[0] for p in picked], dtype=np.uint64)
    c1 = np.array([p[1] for p in picked], dtype=np.uint64)
    t0 = time.perf_counter()
    score, child, status = X.solve_all(O, c0, c1, log2_entries=26)
    t_oracle = time.perf_counter() - t0
    assert (status == O.EXACT_SEARCHED).all() and len(c0) == sum(X.ROWS_PER_EMPTIES.values()) == 7456
    empties = (X.SIZE - X.ages(c0, c1)).astype(np.int8)
    s = X.strata(c0, c1, score)
    counts = {name: int(s[name].sum()) for name in X.STRATA}
    print("strata: " + ", ".join("%s %d" % kv for kv in counts.items()))
    short = [name for name in X.STRATA if counts[name] < X.STRATUM_MIN]
    if short:
        raise SystemExit("fewer than %d rows in: %s" % (X.STRATUM_MIN, ", ".join(short)))
    path = os.path.join(HERE, "solver_exact.npz")
    np.savez_compressed(path, c0=c0, c1=c1, score=score, child_score=child, empties=empties, tree=s["tree"],
                        **{name: s[name] for name in X.STRATA})
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != "solver_exact.npz")
    assert os.path.getsize(path) < largest, "the fixture must stay smaller than the largest one committed"
    print("solver_exact.npz: %d rows, %d bytes; %d of %d rows at e >= %d discarded (more than %d nodes in solve_host)" % (
        len(c0), os.path.getsize(path), discarded, filtered, FILTER_FROM_EMPTIES, FILTER_NODES))
    print("seconds: drawing %.0f, the oracle %.0f, the filter %.0f, in all %.0f" % (
        t_draw, t_oracle, t_filter, time.perf_counter() - t_start))


if __name__ == "__main__":
    main()
