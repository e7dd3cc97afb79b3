"""The root driver without a device (solver.drive_host / drive_graph_host): alpha-beta over the split.
The yardstick is tests/golden/solver_exact.npz -- the exhaustive oracle's exact scores -- and, for the nodes of the graphs,
the same oracle run here.  No GPU: the device is held to tests/golden/solver_driver.npz by tests/test_gpu_solver_driver.py, and
this file holds that file to the live host mirror."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import solver_driver_cases as D
import solver_exact_cases as E
from conftest import ROOT
from solver_window_cases import WINDOWS


@pytest.fixture(scope="module")
def z():
    return D.exact_rows()


@pytest.fixture(scope="module")
def sample(z):
    idx = D.stratified_sample(z)
    return idx, np.stack([z["c0"][idx], z["c1"][idx]], axis=1).astype(np.uint64), z["score"][idx].astype(np.int64)


@pytest.fixture(scope="module")
def leaf():
    """The host mirror's leaf search, memoised for the module: the same leaves come back under many windows and budgets."""
    from connect4_amd.solver import _host_leaf
    memo = {}

    def solve(*key):
        if key not in memo:
            memo[key] = _host_leaf(*key)
        return memo[key]
    return solve


def node_exact(oracle, g):
    """The oracle's exact score for the mover of every node of a graph; finished positions score for themselves."""
    score, _, status = E.solve_all(oracle, g.color0, g.color1, log2_entries=22)
    score = score.astype(np.int64)
    for i in np.nonzero(status == oracle.EXACT_FINISHED)[0]:
        score[i] = D.mover_score_of_finished(g.color0[i], g.color1[i])
    return score, status


def test_the_sample_covers_every_stratum_and_immediate_wins(z, sample):
    idx = sample[0]
    for name in E.STRATA:
        assert z[name][idx].sum() >= 3, name
    assert (~z["tree"][idx]).sum() >= 3
    assert z["empties"][idx].max() >= 16 and z["empties"][idx].min() <= 3


# -- 1. an ample budget: every row is decided, and as the oracle says -----------------------------------------------------
@pytest.mark.parametrize("plies", D.PLIES)
@pytest.mark.parametrize("window", WINDOWS)
def test_an_ample_budget_decides_every_row(sample, leaf, plies, window):
    from connect4_amd import _lib as L
    from connect4_amd.solver import drive_host
    _, rows, exact = sample
    a, b = window
    res, rep = drive_host(rows, a, b, plies, leaf_solver=leaf)
    assert (res.status == L.SOLVE_SOLVED).all()
    assert len(E.window_violations(res.score, res.bound, a, b, exact)) == 0
    if window == (-42, 42):
        assert (res.bound == L.SOLVE_BOUND_EXACT).all() and np.array_equal(res.score, exact)
    ex = res.bound == L.SOLVE_BOUND_EXACT
    out, age = E.answer_of_score(exact, 42 - D.exact_rows()["empties"][sample[0]].astype(np.int64))
    assert np.array_equal(res.final_age, np.where(ex, age, -1)) and np.array_equal(np.nan_to_num(res.outcome, nan=-1.0), np.where(ex, out, -1.0))
    assert not np.isin(rep["state"], (L.SOLVE_NODE_OVER_BUDGET, L.SOLVE_NODE_PENDING)).any()


# -- 2. small budgets: what is said is true, what is not said is not known ------------------------------------------------
@pytest.mark.parametrize("budget", [1, 64, 1024])
@pytest.mark.parametrize("plies", D.PLIES)
def test_under_a_budget_every_answer_and_every_interval_is_true(oracle, sample, leaf, budget, plies):
    from connect4_amd import _lib as L
    from connect4_amd.solver import drive_host
    _, rows, exact = sample
    a, b = D.cycled_windows(len(rows), plies)
    res, rep = drive_host(rows, a, b, plies, node_budget=budget, nodes_per_launch=16, leaf_solver=leaf)
    g = rep["graph"]
    truth, status = node_exact(oracle, g)
    valid = status != oracle.EXACT_INVALID
    assert valid.all()
    lo, hi = rep["lo"].astype(np.int64), rep["hi"].astype(np.int64)
    assert ((lo <= truth) & (truth <= hi)).all()
    given = res.status == L.SOLVE_SOLVED
    assert np.isin(res.status, (L.SOLVE_SOLVED, L.SOLVE_UNKNOWN)).all()
    from solver_window_cases import consistent
    assert consistent(res.score[given], res.bound[given], a[given].astype(np.int64), b[given].astype(np.int64), exact[given]).all()
    r_lo, r_hi = lo[g.inverse], hi[g.inverse]
    decides = (r_lo == r_hi) | (r_lo >= b) | (r_hi <= a)
    assert np.array_equal(given, decides)
    print("budget %d, k = %d: %d of %d rows decided; states %s" % (budget, plies, given.sum(), len(rows), np.bincount(rep["state"], minlength=5).tolist()))
    assert budget > 64 or (~given).any()        # the budget bites
    assert (rep["nodes"] <= budget).all()


# -- 3. dropping -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plies", D.PLIES)
def test_needed_only_ever_shrinks_and_dropped_leaves_were_not_needed(sample, leaf, plies):
    from connect4_amd import _lib as L
    from connect4_amd.solver import drive_graph_host, drive_host
    _, rows, exact = sample
    a, b = D.cycled_windows(len(rows), plies + 1)
    res, rep = drive_host(rows, a, b, plies, nodes_per_launch=16, leaf_solver=leaf)
    marks = rep["needed"]
    assert len(marks) == rep["launches"] + 1 and rep["launches"] > 3
    for before, after in zip(marks, marks[1:]):
        assert not (after & ~before).any()
    dropped = np.nonzero(rep["state"] == L.SOLVE_NODE_DROPPED)[0]
    assert len(dropped) > 10 and (rep["nodes"][dropped] % 16 == 1).all()
    # the dropped leaves' true answers, handed in from the start, change no decided row
    g = rep["graph"]
    truth = {int(i): leaf(int(g.color0[i]), int(g.color1[i]), int(rep["alpha"][i]), int(rep["beta"][i]), 1 << 26)[1:3] for i in dropped}
    again, rep2 = drive_graph_host(g, nodes_per_launch=16, leaf_solver=leaf, given=truth)
    first = (res.status, res.score, res.bound)
    status2, score2, bound2 = (np.asarray(x)[g.inverse] for x in again[:3])
    assert (res.status == L.SOLVE_SOLVED).all() and np.array_equal(status2, res.status) and np.array_equal(bound2, res.bound)
    ex = res.bound == L.SOLVE_BOUND_EXACT
    assert np.array_equal(score2[ex], res.score[ex])
    assert len(E.window_violations(score2, bound2, a.astype(np.int64), b.astype(np.int64), exact)) == 0
    assert first[0] is res.status


def test_the_siblings_of_an_early_refutation_are_dropped_in_its_launch(sample, leaf):
    """Found in the sample, not constructed: a row, alone and one ply deep, one of whose replies fails low for the opponent
    (the row's lower bound reaches beta) in launch t while other replies are still being searched.  They end dropped with the
    1 + t * quota nodes they had entered."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import drive_host
    _, rows, _ = sample
    quota, found = 16, []
    for i, row in enumerate(rows):
        for a, b in ((-1, 0), (0, 1), (-1, 1)):
            res, rep = drive_host(row[None, :], a, b, 1, nodes_per_launch=quota, leaf_solver=leaf)
            state, nodes = rep["state"][1:], rep["nodes"][1:]
            late = (state == L.SOLVE_NODE_DROPPED) & (nodes > 1)
            if not late.any():
                continue
            found.append(i)
            t = (int(nodes[late][0]) - 1) // quota
            assert t >= 1 and (nodes[late] == 1 + t * quota).all()
            assert res.status[0] == L.SOLVE_SOLVED and res.bound[0] == L.SOLVE_BOUND_LOWER and res.score[0] >= b
            # the refutation: an answered reply whose upper bound, negated, reaches beta -- and it landed in launch t
            refuters = (state == L.SOLVE_NODE_ANSWERED) & (-rep["hi"][1:].astype(np.int64) >= b)
            assert refuters.any()
            landed = np.where(nodes[refuters] <= 1, 0, -(-(nodes[refuters] - 1) // quota))
            assert landed.min() in (t, t - 1) and (landed >= t - 1).all()
            # (t - 1: the reply entered its last node with the last of a launch's quota and closed in the next, run_lane's rule)
            assert rep["launches"] == t
    print("rows with an early refutation: %s" % sorted(set(found)))
    assert found


# -- 4. the graph and the fold --------------------------------------------------------------------------------------------
def _asymmetric_root():
    from connect4_amd.board import Board
    b = Board()
    for m in (0, 1, 0, 2, 5, 1):
        b.make_move(m)
    return b


def test_two_parents_with_different_windows_give_their_child_the_union_and_mirror_images_are_merged():
    from connect4_amd.solver import _build_graph, _children_host, _graph_windows, _mirror_bits
    b = _asymmetric_root()
    row = np.array([b.color], dtype=np.uint64)
    rows = np.concatenate([row, row, _mirror_bits(row)])
    a, bb = np.array([-3, 5, -1], dtype=np.int8), np.array([2, 9, 1], dtype=np.int8)
    g = _build_graph(rows, a, bb, 1, _children_host)
    assert g.level_start.tolist() == [0, 3, 10]                         # three roots, seven children between them
    assert sorted(g.inverse.tolist()) == [0, 1, 2]
    wa, wb = _graph_windows(g)
    kids = g.child[:3]
    assert (kids >= 3).all() and len(np.unique(kids)) == 7
    assert np.array_equal(np.sort(kids[g.inverse[0]]), np.sort(kids[g.inverse[2]]))         # the mirror image's children are the row's
    assert np.array_equal(kids[g.inverse[0]], kids[g.inverse[2]][::-1])
    # every child has the three parents (-3, 2), (5, 9), (-1, 1): the union of (-2, 3), (-9, -5), (-1, 1)
    assert (wa[3:] == -9).all() and (wb[3:] == 3).all()
    # one parent alone: the plain negamax window
    g1 = _build_graph(row, a[:1], bb[:1], 2, _children_host)
    wa1, wb1 = _graph_windows(g1)
    assert (wa1[1:8] == -2).all() and (wb1[1:8] == 3).all() and (wa1[8:] == -3).all() and (wb1[8:] == 2).all()
    assert g1.level_start[3] - g1.level_start[2] == 49                  # two plies of an asymmetric position: nothing meets
    g3 = _build_graph(row, a[:1], bb[:1], 3, _children_host)
    assert g3.level_start[4] - g3.level_start[3] < 343                  # three plies: o's two moves in either order are one node
    assert len(np.unique(np.stack([g3.color0, g3.color1], axis=1)[int(g3.level_start[3]):], axis=0)) == g3.level_start[4] - g3.level_start[3]


def test_a_finished_child_answers_for_itself():
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    from connect4_amd.solver import drive_host
    b = Board()
    for m in (3, 0, 3, 0, 3, 1):
        b.make_move(m)                      # o wins by 3 at age 7
    res, rep = drive_host([b], -1, 1, 2, node_budget=1)
    g = rep["graph"]
    won = [i for i in range(1, int(g.level_start[2])) if (g.child[i] < 0).all()]
    assert len(won) == 1 and rep["state"][won[0]] == L.SOLVE_NODE_SELF and rep["lo"][won[0]] == rep["hi"][won[0]] == 7 - 43
    assert rep["nodes"][won[0]] == 0
    # the row is decided by that child alone, whatever the budget leaves of the others
    assert res.status[0] == L.SOLVE_SOLVED and res.bound[0] == L.SOLVE_BOUND_LOWER and res.score[0] == 36
    finished = Board()
    for m in (3, 0, 3, 0, 3, 1, 3):
        finished.make_move(m)
    res, rep = drive_host([finished, b], -1, 1, 1, node_budget=1)
    assert res.status.tolist() == [L.SOLVE_TERMINAL, L.SOLVE_SOLVED] and res.final_age.tolist() == [7, -1] and res.outcome[0] == 1.0
    assert res.score.tolist() == [0, 36] and res.bound.tolist() == [L.SOLVE_BOUND_NONE, L.SOLVE_BOUND_LOWER] and res.nodes[0] == 0


def test_the_nodes_of_a_row_are_the_sum_over_its_distinct_leaves():
    from connect4_amd import _lib as L
    from connect4_amd.solver import drive_host
    b = _asymmetric_root()

    def scripted(c0, c1, alpha, beta, budget):      # every leaf costs as many nodes as its color0 has low bits set, plus two
        n = 2 + bin(c0 & 0xffff).count("1")
        return (L.SOLVE_UNKNOWN, 0, L.SOLVE_BOUND_NONE, min(n, budget), False) if n > budget else (L.SOLVE_SOLVED, 0, L.SOLVE_BOUND_EXACT, n, True)

    other = b.__copy__()
    other.make_move(4)
    res, rep = drive_host([b, other], None, None, 2, leaf_solver=scripted)
    g = rep["graph"]
    first = int(g.level_start[-2])
    for i, r in enumerate(g.inverse):
        reach, todo = set(), [int(r)]
        while todo:
            j = todo.pop()
            kids = [int(c) for c in g.child[j] if c >= 0]
            if j >= first:
                reach.add(j)
            todo += kids
        assert len(reach) > 20
        assert res.nodes[i] == sum(int(rep["nodes"][j]) for j in reach) == sum(2 + bin(int(g.color0[j]) & 0xffff).count("1") for j in reach)
    assert (rep["nodes"][:first] == 0).all()


# -- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_bad_driver_plies_are_refused():
    from connect4_amd.solver import drive_host, label, label_values, outcomes, solve_window
    b = [_asymmetric_root()]
    for bad in (9, -1, 1.5):
        with pytest.raises(ValueError, match="driver_plies"):
            drive_host(b, -1, 1, bad)
        for call in (lambda: solve_window(b, -1, 1, driver_plies=bad, host=True), lambda: outcomes(b, driver_plies=bad, host=True),
                     lambda: label_values(b, driver_plies=bad, host=True), lambda: label(b, exact=False, driver_plies=bad, host=True)):
            with pytest.raises(ValueError, match="driver_plies"):
                call()
    with pytest.raises(ValueError, match="driver_plies"):
        drive_host(b, -1, 1, 0)
    with pytest.raises(ValueError, match="split_plies"):
        label(b, exact=False, driver_plies=2, split_plies=1, host=True)
    with pytest.raises(ValueError, match="split_plies"):
        label(b, driver_plies=2, split_plies=1)
    with pytest.raises(ValueError, match="exact=False"):
        label(b, driver_plies=2)
    with pytest.raises(ValueError, match="exact=False"):
        label(b, driver_plies=2, exact=True, host=True)
    with pytest.raises(ValueError):                                 # what was refused before still is
        label(b, exact=False, split_plies=1, host=True)
    with pytest.raises(ValueError, match="window"):
        drive_host(b, 3, 3, 2)


def _bad_graphs():
    from connect4_amd.solver import _build_graph, _children_host
    b = _asymmetric_root()
    g = _build_graph(np.array([b.color], dtype=np.uint64), np.array([-1], dtype=np.int8), np.array([1], dtype=np.int8), 2, _children_host)
    n = len(g.child)

    def with_child(at, col, value):
        child = g.child.copy()
        child[at, col] = value
        return g._replace(child=child)

    start = g.level_start
    # one node above 2^20 + 1 of them: more than a graph's last level takes (the size is refused before the links are read)
    big = (1 << 20) + 1
    wide = g._replace(color0=np.zeros(big + 1, dtype=np.uint64), color1=np.zeros(big + 1, dtype=np.uint64),
                      level_start=np.array([0, 1, big + 1], dtype=np.int64), child=np.full((big + 1, 7), -1, dtype=np.int32))
    return {"a child in its own level": with_child(1, 0, 2), "a child two levels down": with_child(0, 0, int(start[2])),
            "a child beyond the graph": with_child(1, 0, n), "a child below -1": with_child(1, 0, -2),
            "a child of the last level": with_child(n - 1, 0, n - 1), "levels that overlap": g._replace(level_start=np.array([0, 8, 1, n])),
            "levels that do not start at 0": g._replace(level_start=start + 1), "one level": g._replace(level_start=start[[0, 3]]),
            "ten levels": g._replace(level_start=np.concatenate([start[:2], np.repeat(start[2:3], 8), start[3:]])),
            "a last level beyond 2^20 nodes": wide,
            "a bad window": g._replace(alpha=np.array([1], dtype=np.int8)), "half a window": g._replace(alpha=None),
            "an orphan": with_child(0, int(np.nonzero(g.child[0] >= 0)[0][0]), -1)}, g


def test_a_bad_graph_is_refused_by_the_binding_and_by_the_library():
    """Every malformed graph raises in the binding's own checks; handed to the library past them it comes back C4_EINVAL with a
    message, before a device is looked for (this machine has none: C4_EDEVICE would say that it was)."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_graph
    bad, good = _bad_graphs()
    lib = L.load()
    i8p, i64 = C.POINTER(C.c_int8), L._i64p
    for name, g in bad.items():
        with pytest.raises(ValueError):
            solve_graph(g)
        start = np.ascontiguousarray(g.level_start, dtype=np.int64)
        n0, n_nodes = 1, len(g.child)
        c0, c1 = (np.ascontiguousarray(x, dtype=np.uint64) for x in (g.color0, g.color1))
        child = np.ascontiguousarray(g.child, dtype=np.int32)
        outs8 = [np.zeros(max(n0, 16), dtype=np.int8) for _ in range(5)]
        outs64 = [np.zeros(max(n0, 16), dtype=np.int64) for _ in range(2)]
        ptr8 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int8).ctypes.data_as(i8p)  # noqa: E731
        alpha, beta = (None if x is None else np.ascontiguousarray(x, dtype=np.int8) for x in (g.alpha, g.beta))
        rc = lib.c4_solve_graph(0, None, c0.ctypes.data_as(L._u64p), c1.ctypes.data_as(L._u64p), start.ctypes.data_as(i64), len(start) - 1,
                                child.ctypes.data_as(C.POINTER(C.c_int32)), None if alpha is None else alpha.ctypes.data_as(i8p),
                                None if beta is None else beta.ctypes.data_as(i8p), 0, 0, *[x.ctypes.data_as(i8p) for x in outs8],
                                *[x.ctypes.data_as(i64) for x in outs64], None, None, None, None, None)
        msg = lib.c4_solve_last_error().decode()
        print("%-32s %d %s" % (name, rc, msg))
        assert rc == L.EINVAL and msg, name
    assert len(good.child) == int(good.level_start[-1])


def test_the_binding_and_the_header_agree():
    from connect4_amd import _lib as L
    from connect4_amd import solver
    text = open(os.path.join(ROOT, "include", "c4_engine.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+C4_SOLVE_NODE_([A-Z_]+)\s+(\d+)", text)}
    assert header == {"INTERIOR": L.SOLVE_NODE_INTERIOR, "SELF": L.SOLVE_NODE_SELF, "ANSWERED": L.SOLVE_NODE_ANSWERED,
                      "OVER_BUDGET": L.SOLVE_NODE_OVER_BUDGET, "DROPPED": L.SOLVE_NODE_DROPPED, "PENDING": L.SOLVE_NODE_PENDING}
    assert sorted(solver.NODE_STATE_NAMES) == [0, 1, 2, 3, 4]
    assert int(re.search(r"#define\s+C4_SOLVE_GRAPH_MAX_PLIES\s+(\d+)", text).group(1)) == L.SOLVE_GRAPH_MAX_PLIES == 8
    res, args = L.SIGNATURES["c4_solve_graph"]
    proto = re.search(r"\bint c4_solve_graph\(([^;]*)\);", text).group(1)
    assert res is C.c_int and len(args) == len(proto.split(",")) == 23
    src = open(os.path.join(ROOT, "connect4_amd", "csrc", "c4_solve.hip")).read()
    assert "int c4_solve_graph(" in src
    assert int(re.search(r"DEFAULT_PER_LAUNCH = \(int64_t\)1 << (\d+)", src).group(1)) == 14 and L.SOLVE_DEFAULT_NODES_PER_LAUNCH == 1 << 14
    assert int(re.search(r"CHUNK_ROWS = \(int64_t\)1 << (\d+)", src).group(1)) == 20 and solver.GRAPH_MAX_LEAVES == 1 << 20
    assert re.search(r"#define\s+C4_ABI_VERSION\s+4\b", text) and L.ABI_VERSION == 4       # an addition only
    assert L.load().c4_abi_version() == 4


# -- 6. the golden file, the public calls, the tool -----------------------------------------------------------------------
def test_the_golden_file_is_the_live_host_mirror(z, leaf):
    from connect4_amd.solver import drive_host
    cases = D.golden_cases()
    fixed = D.fixed_cases(z)
    assert [c.name for c, _ in cases][:len(fixed)] == [c.name for c in fixed]
    names = [c.name for c, _ in cases]
    assert sum(n.startswith("open") for n in names) == 2 * D.OPEN_ROOTS
    for (case, want), mine in zip(cases, fixed):
        for f in ("rows", "alpha", "beta"):
            assert np.array_equal(getattr(case, f), getattr(mine, f)), (case.name, f)
        assert (case.plies, case.quota, case.budget) == (mine.plies, mine.quota, mine.budget)
        res, rep = drive_host(case.rows, case.alpha, case.beta, case.plies, node_budget=case.budget, nodes_per_launch=case.quota, leaf_solver=leaf)
        for f in D.ROW_FIELDS:
            assert np.array_equal(getattr(res, f), want[f], equal_nan=f == "outcome"), (case.name, f)
        for f, mine_f in zip(D.NODE_FIELDS, ("lo", "hi", "state", "nodes")):
            assert np.array_equal(rep[mine_f], want[f]), (case.name, f)
    # the cases do what they are there for: rows park under the quota of 256, leaves are dropped between launches, budgets bite
    by_name = {c.name: w for c, w in cases}
    from connect4_amd import _lib as L
    n_late = 0
    for k in D.PLIES:
        w = by_name["sample_k%d_q256" % k]
        late = (w["state"] == L.SOLVE_NODE_DROPPED) & (w["node_nodes"] > 1)
        n_late = n_late + int(late.sum())
        assert (w["node_nodes"] > 2 * 256).any() and (w["node_nodes"][late] % 256 == 1).all()
    assert n_late >= 3
    assert any((w["state"] == L.SOLVE_NODE_OVER_BUDGET).any() and (w["status"] == L.SOLVE_UNKNOWN).any() for n, w in by_name.items() if n.endswith("b64"))
    for n, w in by_name.items():
        if n.startswith("open"):
            assert w["status"].tolist() == [L.SOLVE_SOLVED] and w["node_nodes"].max() > 256 and w["node_nodes"].max() <= D.OPEN_LEAF_BUDGET


def test_driven_labels_are_the_undriven_ones_on_the_host(z):
    """label(exact=False, driver_plies=k, host=True), label_values and outcomes against the same calls without a driver, on
    late rows the host mirror labels in seconds."""
    from connect4_amd.solver import label, label_values, outcomes
    idx = np.nonzero((z["empties"] >= 5) & (z["empties"] <= 9))[0][::37][:12]
    rows = np.stack([z["c0"][idx], z["c1"][idx]], axis=1).astype(np.uint64)
    want, w_rep = label(rows, exact=False, host=True)
    for k in (1, 2):
        got, rep = label(rows, exact=False, host=True, driver_plies=k)
        assert rep["driver_plies"] == k and rep["labelled"] == w_rep["labelled"] == len(rows) and rep["unknown"] == 0
        assert got.boards.equal(want.boards) and got.values.equal(want.values) and got.priors.equal(want.priors)
    got, _ = label_values(rows, host=True, driver_plies=2)
    assert got.values.equal(label_values(rows, host=True)[0].values) and got.priors is None
    boards = [(int(a), int(b)) for a, b in rows]
    sign = np.sign(z["score"][idx].astype(np.int64))
    absolute = np.where((42 - z["empties"][idx]) & 1, -sign, sign)
    assert np.array_equal(outcomes(boards, driver_plies=2, host=True), (absolute + 1) * 0.5)


def test_make_test_set_knows_driver_plies(capsys):
    spec = importlib.util.spec_from_file_location("make_test_set", os.path.join(ROOT, "tools", "make_test_set.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for argv, why in ((["--openings", "4", "--driver-plies", "2", "--table-log2", "20", "-o", "x.pth"], "--driver-plies belongs to"),
                      (["--openings", "4", "--outcome-only", "--driver-plies", "9", "-o", "x.pth"], "--driver-plies takes 1..8"),
                      (["--openings", "4", "--values-only", "--driver-plies", "-1", "-o", "x.pth"], "--driver-plies takes 1..8"),
                      (["--openings", "4", "--outcome-only", "--driver-plies", "2", "--split-plies", "1", "-o", "x.pth"], "--split-plies belongs to")):
        with pytest.raises(SystemExit):
            mod.main(argv)
        err = capsys.readouterr().err
        assert why in err and "unrecognized" not in err, err          # refused for its value, not as an unknown flag


def test_every_golden_answer_is_a_true_bound_against_the_oracle(z):
    """The file's own rows -- the batches with finished and invalid rows mixed in, under budgets of 64 and ample, and the
    sample -- against solver_exact.npz: the device is held to the file bit for bit, the file to the oracle here."""
    from connect4_amd import _lib as L
    from solver_window_cases import consistent
    lookup = {(int(a), int(b)): int(s) for a, b, s in zip(z["c0"], z["c1"], z["score"])}
    special = D.specials()
    for case, want in D.golden_cases():
        if case.name.startswith("open"):
            continue
        keys = [(int(a), int(b)) for a, b in case.rows]
        plain = np.array([k not in special for k in keys])
        exact = np.array([lookup.get(k, 0) for k in keys], dtype=np.int64)
        given = want["status"] == L.SOLVE_SOLVED
        assert all(k in lookup for k, p in zip(keys, plain) if p)
        assert np.isin(want["status"][plain], (L.SOLVE_SOLVED, L.SOLVE_UNKNOWN)).all()
        assert [int(st) for k, st in zip(keys, want["status"]) if k in special] == \
            [(L.SOLVE_TERMINAL, L.SOLVE_INVALID, L.SOLVE_INVALID, L.SOLVE_INVALID)[special.index(k)] for k in keys if k in special]
        assert consistent(want["score"][given], want["bound"][given], case.alpha[given].astype(np.int64), case.beta[given].astype(np.int64),
                          exact[given]).all()
        if case.budget == D.AMPLE:
            assert given[plain].all()
            assert len(E.window_violations(want["score"][plain], want["bound"][plain], case.alpha[plain].astype(np.int64),
                                           case.beta[plain].astype(np.int64), exact[plain])) == 0


def test_a_graph_may_end_in_an_empty_level():
    """Rows that all answer for themselves, and rows with fewer empty squares than driver_plies: the graph is accepted, the last
    level is empty, nothing is searched and every row is answered by the fold alone."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import _check_graph
    by_name = {c.name: (c, w) for c, w in D.golden_cases()}
    case, want = by_name["all_self_k2"]
    assert want["status"].tolist() == [L.SOLVE_TERMINAL, L.SOLVE_INVALID, L.SOLVE_INVALID, L.SOLVE_INVALID] and not want["nodes"].any()
    case, want = by_name["short_k3"]
    assert (want["status"] == L.SOLVE_SOLVED).all() and not want["nodes"].any() and (want["lo"] == want["hi"]).all()
    from connect4_amd.solver import _build_graph, _children_host
    g = _build_graph(case.rows, case.alpha, case.beta, case.plies, _children_host)
    assert g.level_start[-1] == g.level_start[-2] and g.level_start[-2] > g.level_start[1]
    _check_graph(g)
