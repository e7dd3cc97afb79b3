"""The transposition table and the split of the exact solver on the host (connect4_amd/solver.py), no GPU: solve_host with a
dict is the plain-Python statement of the kernel's probe / store / bound logic, and it must answer what the table-free
search answers (tests/golden/solver_deep.npz, and tests/golden/solver_open.npz written by
tests/golden/gen_solver_open_golden.py) whatever the dict holds; the host fold of split_plies against the fixture's
children; the new symbols and constants."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_npz


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def rows():
    """(c0, c1, outcome, final_age, value, nodes) of every row of the two fixtures, the table-free answers."""
    out = []
    for name in ("solver_deep.npz", "solver_open.npz"):
        z = load_npz(name)
        out += [(int(z["c0"][i]), int(z["c1"][i]), float(z["outcome"][i]), int(z["final_age"][i]), float(z["value"][i]),
                 int(z["nodes"][i])) for i in range(len(z["c0"]))]
    return out


@pytest.fixture(scope="module")
def open_set():
    return load_npz("solver_open.npz")


def check(answer, row):
    from connect4_amd import _lib as L
    assert answer.status == L.SOLVE_SOLVED
    assert (answer.outcome, answer.final_age) == (row[2], row[3]) and same_bits(answer.value, row[4]), (row, answer)


def test_open_fixture_is_what_it_should_be(open_set):
    from connect4_amd import _lib as L
    z = open_set
    empties = 42 - np.array([bin(int(a | b)).count("1") for a, b in zip(z["c0"], z["c1"])])
    counts = np.bincount(empties, minlength=33)
    assert sorted(set(empties.tolist())) == list(range(25, 33)) and counts[25:].min() >= 4 and counts[25:].max() == 8
    assert sorted(set(z["outcome"].tolist())) == [0.0, 0.5, 1.0]
    legal = z["child_legal"] != 0
    assert z["nodes"].max() <= 1 << 18 and z["child_nodes"].max() <= 1 << 18 and legal.sum(axis=1).min() >= 1
    assert np.isin(z["child_status"][legal], (L.SOLVE_SOLVED, L.SOLVE_TERMINAL)).all()
    # the fixture is consistent with itself: a position's value is the best of its children's for its mover
    for i in range(len(empties)):
        vals = z["child_value"][i][legal[i]]
        assert same_bits(z["value"][i], vals.max() if empties[i] % 2 == 0 else vals.min())


def test_fresh_table_per_row(rows):
    from connect4_amd.solver import solve_host
    for row in rows:
        check(solve_host(row[:2], table={}), row)


def test_shared_table_in_both_orders_and_warm(rows):
    from connect4_amd.solver import solve_host
    for order in (rows, rows[::-1]):
        table = {}
        cold = 0
        for row in order:
            a = solve_host(row[:2], table=table)
            check(a, row)
            cold += a.nodes
        warm = 0
        for row in order:
            a = solve_host(row[:2], table=table)
            check(a, row)
            warm += a.nodes
        print("nodes: table-free %d, shared table %d, second pass %d, entries %d" % (sum(r[5] for r in rows), cold, warm, len(table)))
        assert warm < cold
        # an entry is (kind, score) under the 49-bit key, the score within 7 bits
        assert all(0 < k < 1 << 49 and kind in (1, 2, 3) and -64 <= s < 64 for k, (kind, s) in table.items())


def test_deep_and_table_statuses_on_the_host():
    from connect4_amd import _lib as L
    from connect4_amd.solver import random_playout, solve_host
    rng = np.random.RandomState(5)
    b = random_playout(rng, 17)                                    # 25 empty squares
    assert solve_host(b).status == L.SOLVE_TOO_DEEP                # the default search is what it was
    for kw in ({"deep": True}, {"table": {}}):
        a = solve_host(b, node_budget=64, **kw)
        assert a.status in (L.SOLVE_SOLVED, L.SOLVE_UNKNOWN) and (a.status == L.SOLVE_SOLVED or a.nodes == 64)
    # table-free, the deep search walks the tree of the default search
    z = load_npz("solver_deep.npz")
    for i in range(0, 256, 32):
        a = solve_host((int(z["c0"][i]), int(z["c1"][i])), deep=True)
        assert a.nodes == z["nodes"][i] and a.final_age == z["final_age"][i]


def test_grid_triple_host_with_a_table(open_set):
    """grid_triple(host=True, table=dict) on positions the default search calls too deep: GridTree's children from the
    fixture's children, Tree.best_move's tie to the higher column."""
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    from connect4_amd.solver import grid_triple
    z = open_set
    legal = z["child_legal"] != 0
    pick = [i for i in range(len(z["c0"])) if z["nodes"][i] + z["child_nodes"][i].sum() <= 20000]
    assert len(pick) >= 20
    boards = [Board.from_bits(int(z["c0"][i]), int(z["c1"][i])) for i in pick]
    with pytest.raises(ValueError):
        grid_triple(boards[:1], host=True)
    for i, b, (move, value, tree) in zip(pick, boards, grid_triple(boards, host=True, table={})):
        cols = np.nonzero(legal[i])[0]
        # a finished child's absolute_value is its result (tree.py:27-38), any other child's its exact value
        vals = np.where(z["child_status"][i][cols] == L.SOLVE_TERMINAL, z["child_outcome"][i][cols], z["child_value"][i][cols])
        assert [c.name for c in tree.root.children] == cols.tolist()
        assert same_bits([c.data.absolute_value for c in tree.root.children], vals)
        assert same_bits(tree.root.data.search_value, z["value"][i])
        best = vals.max() if b.age % 2 == 0 else vals.min()
        assert move == int(cols[vals == best].max()) and same_bits(value, best)


def test_symbols_and_constants():
    from connect4_amd import _lib as L
    from connect4_amd import solver
    import __graft_entry__ as g
    g.build_engine()
    text = open(os.path.join(ROOT, "include", "c4_engine.h")).read()
    assert re.search(r"#define\s+C4_SOLVE_DEEP_MAX_EMPTIES\s+42\b", text) and re.search(r"#define\s+C4_SOLVE_MAX_EMPTIES\s+24\b", text)
    assert L.SOLVE_DEEP_MAX_EMPTIES == solver.DEEP_MAX_EMPTIES == 42 and L.SOLVE_MAX_EMPTIES == solver.MAX_EMPTIES == 24
    assert re.search(r"#define\s+C4_ABI_VERSION\s+4\b", text) and L.ABI_VERSION == 4 and L.load().c4_abi_version() == 4
    src = open(os.path.join(ROOT, "connect4_amd", "csrc", "c4_solve.hip")).read()
    assert int(re.search(r"TT_MIN_EMPTIES = (\d+);", src).group(1)) == solver._TT_MIN_EMPTIES
    lo, hi = re.search(r"TT_MIN_LOG2 = (\d+), TT_MAX_LOG2 = (\d+);", src).groups()
    assert (int(lo), int(hi)) == (L.SOLVE_TABLE_MIN_LOG2, L.SOLVE_TABLE_MAX_LOG2) == (10, 30)
    assert [int(x) for x in re.search(r"TT_LOWER = (\d), TT_UPPER = (\d), TT_EXACT = (\d);", src).groups()] == [
        solver._LOWER, solver._UPPER, solver._EXACT]
    # the entry word and the slot function HostTable and entry_fields restate
    assert "key * 0x%XULL) >> t.shift" % solver._TT_HASH in src and "TT_KEY_MASK = (1ULL << %d) - 1;" % solver._TT_KEY_BITS in src
    assert "(uint64_t)(score + 64) << %d) | ((uint64_t)kind << %d)" % (solver._TT_SCORE_SHIFT, solver._TT_KIND_SHIFT) in src
    lib = L.load()
    for name in ("c4_solve_table_create", "c4_solve_table_destroy", "c4_solve_table_clear", "c4_solve_table_read", "c4_solve_deep_dev",
                 "c4_solve_deep"):
        assert name in L.SIGNATURES and hasattr(lib, name) and re.search(r"\bint %s\(" % name, text)
    assert len(L.SIGNATURES["c4_solve_deep_dev"][1]) == 12 and len(L.SIGNATURES["c4_solve_deep"][1]) == 12


# -- the split's host half ---------------------------------------------------------------------------------------------------
def fixture_answers(z):
    """{(c0, c1): (status, outcome code, final age, nodes)} of the fixture's children, under both orientations."""
    from connect4_amd.solver import _mirror_bits
    known = {}
    legal = z["child_legal"] != 0
    for i, c in zip(*np.nonzero(legal)):
        ans = (int(z["child_status"][i, c]), int(round(z["child_outcome"][i, c] * 2)), int(z["child_final_age"][i, c]),
               int(z["child_nodes"][i, c]))
        pair = np.array([z["child_c0"][i, c], z["child_c1"][i, c]], dtype=np.uint64)
        known[tuple(int(x) for x in pair)] = ans
        known[tuple(int(x) for x in _mirror_bits(pair))] = ans
    return known


def fold(g, answer_of):
    """_graph_fold_exact with the last level answered by `answer_of(c0, c1)` and the childless nodes above it by solve_host."""
    from connect4_amd.solver import _graph_fold_exact, solve_host
    first_leaf = int(g.level_start[-2])
    cols = [np.full(len(g.child), -1, dtype=np.int64) for _ in range(5)]
    for i in range(first_leaf, len(g.child)):
        cols[0][i], cols[1][i], cols[2][i], cols[3][i], cols[4][i] = answer_of(int(g.color0[i]), int(g.color1[i])) + (0,)
    for i in np.nonzero(~(g.child[:first_leaf] >= 0).any(axis=1))[0]:
        h = solve_host((int(g.color0[i]), int(g.color1[i])), deep=True)
        cols[0][i], cols[1][i], cols[2][i] = h.status, -1 if h.outcome is None else int(h.outcome * 2), h.final_age
    return _graph_fold_exact(g, *cols)


def test_split_one_ply_folds_the_fixture_children(open_set):
    from connect4_amd import _lib as L
    from connect4_amd.solver import _build_graph, _children_host, _mirror_bits, value_from_answer
    z = open_set
    known = fixture_answers(z)
    roots = np.stack([z["c0"], z["c1"]], axis=1)
    both = np.concatenate([roots, roots[:5]])                     # duplicates fold like their originals
    g = _build_graph(both, None, None, 1, _children_host)
    sizes, inverse = np.diff(g.level_start), g.inverse
    assert sizes[0] == len(roots) and sizes[1] <= int((z["child_legal"] != 0).sum()) and (g.child[:sizes[0]] >= 0).any(axis=1).all()
    status, outcome, age, nodes, hits = fold(g, lambda a, b: known[(a, b)])
    status, outcome, age, nodes = status[inverse], outcome[inverse], age[inverse], nodes[inverse]
    want = np.concatenate([np.arange(len(roots)), np.arange(5)])
    assert (status == L.SOLVE_SOLVED).all() and np.array_equal(age, z["final_age"][want])
    assert same_bits(outcome * 0.5, z["outcome"][want]) and same_bits(value_from_answer(outcome * 0.5, age), z["value"][want])
    # nodes: the sum over the distinct children (two children that mirror each other are one)
    for i in range(len(roots)):
        kids = {}
        for a, b, n, ok in zip(z["child_c0"][i], z["child_c1"][i], z["child_nodes"][i], z["child_legal"][i]):
            if ok:
                m = _mirror_bits(np.array([a, b], dtype=np.uint64))
                kids[min((int(a), int(b)), (int(m[0]), int(m[1])))] = int(n)
        assert nodes[i] == sum(kids.values())
    # a child without an answer leaves its parents UNKNOWN and nobody else
    leaf0 = int(g.level_start[1])
    victim = (int(g.color0[leaf0]), int(g.color1[leaf0]))
    status2 = fold(g, lambda a, b: (L.SOLVE_UNKNOWN, -1, -1, 64) if (a, b) == victim else known[(a, b)])[0]
    parents = (g.child[:leaf0] == leaf0).any(axis=1)
    assert parents.any() and (status2[parents] == L.SOLVE_UNKNOWN).all() and (status2[~parents] == L.SOLVE_SOLVED).all()


def test_split_two_plies_on_the_host(open_set):
    """Two plies below the fixture's cheapest rows, the grandchildren answered by solve_host: finished descendants (a child
    that ends the game) answer for themselves, and the fold gives the fixture's answers."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import _build_graph, _children_host, solve_host
    z = open_set
    cost = z["nodes"] + z["child_nodes"].sum(axis=1)
    pick = np.argsort(cost, kind="stable")[:12]
    assert cost[pick].max() <= 4096
    roots = np.stack([z["c0"], z["c1"]], axis=1)[pick]
    g = _build_graph(roots, None, None, 2, _children_host)
    assert not (g.child[g.level_start[1]:g.level_start[2]] >= 0).any(axis=1).all()     # some child has already won the game

    shared = {}

    def answer(a, b):
        h = solve_host((a, b), table=shared)
        return (h.status, int(h.outcome * 2), h.final_age, h.nodes)

    status, outcome, age, _, _ = (a[g.inverse] for a in fold(g, answer))
    assert (status == L.SOLVE_SOLVED).all() and np.array_equal(age, z["final_age"][pick]) and same_bits(outcome * 0.5, z["outcome"][pick])


def test_split_fold_is_the_pinned_fold():
    """_graph_fold_exact on drawn answers (tests/golden/solver_split_fold.npz, written by the fold over per-level arrays that
    it replaced: tests/golden/gen_solver_split_fold_golden.py) -- the five arrays bit for bit, rows that share a node,
    UNKNOWN leaves, levels that thin out to nothing."""
    from connect4_amd.solver import _build_graph, _children_host, _graph_fold_exact
    z = load_npz("solver_split_fold.npz")
    fields = ("status", "outcome", "final_age", "nodes", "hits")
    assert len(z["names"]) == 6
    for name in z["names"]:
        g = _build_graph(z[name + "__rows"], None, None, int(z[name + "__k"]), _children_host)
        answers = [z["%s__node_%s" % (name, f)] for f in fields]
        assert all(len(a) == len(g.child) for a in answers), name
        for f, got in zip(fields, _graph_fold_exact(g, *answers)):
            want = z["%s__%s" % (name, f)]
            assert got.dtype == want.dtype and np.array_equal(got[g.inverse], want), (name, f)
