"""What the windowed-solver tests share (tests/test_solver_window_host.py, tests/test_gpu_solver_window.py): the six windows,
the rows of the three solver fixtures with their exact scores, and tests/golden/solver_window.npz -- the host mirror's
(``solver.solve_host(window=...)``) score, bound kind and node count of every fixture row under every window, written by
tests/golden/gen_solver_window_golden.py.  The host test holds that file to the live host mirror on the rows that are
cheap in Python; the GPU test holds the kernel to the file on all of them."""
from collections import namedtuple

import numpy as np

from conftest import load_npz

# the full window, the outcome window, the two null windows of the staged labelling, a wide off-centre one, a far one
WINDOWS = [(-42, 42), (-1, 1), (-1, 0), (0, 1), (-3, 10), (5, 6)]
FIXTURES = ("solver.npz", "solver_deep.npz", "solver_open.npz")
HOST_NODE_CAP = 20000       # open roots above this are left to the golden file on the host (the existing split test's bound)

Rows = namedtuple("Rows", "name c0 c1 age exact outcome final_age nodes")


def mover_score(outcome, final_age, age):
    """43 - final_age for a win by o, final_age - 43 for one by x, 0 for a draw; from the mover's side (x moves at odd ages)."""
    outcome = np.asarray(outcome, dtype=np.float64)
    final_age = np.asarray(final_age, dtype=np.int64)
    s = np.where(outcome == 1.0, 43 - final_age, np.where(outcome == 0.0, final_age - 43, 0))
    return np.where(np.asarray(age) & 1, -s, s).astype(np.int64)


def fixture_rows(name):
    """A fixture's rows with the mover's exact score of each.  solver.npz has the reference's float only (1 - a/10000 for o,
    a/10000 for x, 0.5 + 42/10000 for a draw) and no node counts: outcome and age are read off the float."""
    z = load_npz(name)
    c0, c1 = z["c0"].astype(np.uint64), z["c1"].astype(np.uint64)
    age = np.array([bin(int(a) | int(b)).count("1") for a, b in zip(c0, c1)], dtype=np.int64)
    if "outcome" in z.files:
        outcome, final_age, nodes = z["outcome"], z["final_age"].astype(np.int64), z["nodes"].astype(np.int64)
    else:
        v = z["root_search"]
        outcome = np.where(v > 0.9, 1.0, np.where(v < 0.1, 0.0, 0.5))
        final_age = np.where(v > 0.9, np.rint((1.0 - v) * 10000), np.where(v < 0.1, np.rint(v * 10000), 42)).astype(np.int64)
        nodes = None
    return Rows(name, c0, c1, age, mover_score(outcome, final_age, age), outcome, final_age, nodes)


def golden():
    """{fixture name: (score, bound, nodes) int64 [rows, windows]} of tests/golden/solver_window.npz."""
    z = load_npz("solver_window.npz")
    assert [tuple(w) for w in z["windows"].tolist()] == WINDOWS
    return {name: tuple(z["%s__%s" % (name[:-4], f)].astype(np.int64) for f in ("score", "bound", "nodes")) for name in FIXTURES}


def consistent(score, bound, alpha, beta, exact):
    """The issue's rule: an exact bound is the exact score, a lower bound has exact >= score >= beta, an upper bound
    exact <= score <= alpha.  Arrays or scalars; bool of the same shape."""
    from connect4_amd import _lib as L
    score, bound, exact = np.asarray(score), np.asarray(bound), np.asarray(exact)
    return np.where(bound == L.SOLVE_BOUND_EXACT, (score == exact) & (alpha < score) & (score < beta),
                    np.where(bound == L.SOLVE_BOUND_LOWER, (exact >= score) & (score >= beta),
                             np.where(bound == L.SOLVE_BOUND_UPPER, (exact <= score) & (score <= alpha), False)))
