"""The windowed search on the host (connect4_amd/solver.py: solve_host(window=...), staged_labels, label(exact=False,
host=True)), no GPU: the CPU-checkable statement of c4_solve_window.  Against the exact scores of the three solver fixtures
under six windows, against tests/golden/solver_window.npz (which the GPU test holds the kernel to), with dict and HostTable
tables, and the staged labelling against prior_from_children fed with the fixtures' exact child outcomes.

With a table the *score* of a row whose bound is not exact may differ from the table-free one -- a stored bound that closes
the window is returned as it is -- so "the same answer" means: the same status, the same kind, the same score where the
kind is exact, and a true bound of that kind otherwise.  The kind cannot differ: it is exact iff the exact score lies inside
the window, and a sound search returns a value on the exact score's side of the window."""
import os
import re

import numpy as np
import pytest

import solver_window_cases as cases
from conftest import ROOT, load_npz
from solver_window_cases import FIXTURES, HOST_NODE_CAP, WINDOWS

CONTAINS = [(i, j) for i, a in enumerate(WINDOWS) for j, b in enumerate(WINDOWS) if i != j and b[0] <= a[0] and a[1] <= b[1]]


def cheap(rows):
    """The rows the host mirror answers quickly: all but the open roots above HOST_NODE_CAP nodes."""
    return np.nonzero(rows.nodes <= HOST_NODE_CAP)[0] if rows.name == "solver_open.npz" else np.arange(len(rows.c0))


@pytest.fixture(scope="module")
def live():
    """{fixture: (rows, picked row indices, answers [picked][window])}: every cheap row under every window, table-free, once."""
    from connect4_amd.solver import solve_host
    out = {}
    for name in FIXTURES:
        rows = cases.fixture_rows(name)
        pick = cheap(rows)
        out[name] = (rows, pick, [[solve_host((int(rows.c0[i]), int(rows.c1[i])), window=w) for w in WINDOWS] for i in pick])
    return out


def test_the_cases_cover_what_they_should(live):
    assert (0, 1) not in CONTAINS and {(1, 0), (2, 1), (3, 1), (2, 4), (5, 4), (5, 0)} <= set(CONTAINS)
    assert len(live["solver.npz"][1]) == 64 and len(live["solver_deep.npz"][1]) == 256 and len(live["solver_open.npz"][1]) >= 40
    kinds = {(wi, a.bound) for _, _, ans in live.values() for row in ans for wi, a in enumerate(row)}
    from connect4_amd import _lib as L
    for wi in range(1, len(WINDOWS)):       # every narrow window meets all three kinds ((5, 6): no exact score fits inside)
        want = {L.SOLVE_BOUND_LOWER, L.SOLVE_BOUND_UPPER} | ({L.SOLVE_BOUND_EXACT} if WINDOWS[wi][1] - WINDOWS[wi][0] > 1 else set())
        assert {k for w, k in kinds if w == wi} == want, WINDOWS[wi]


def test_the_full_window_is_the_fixture(live):
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_host
    for name, (rows, pick, ans) in live.items():
        for i, row in zip(pick, ans):
            a = row[0]
            assert (a.status, a.bound, a.score) == (L.SOLVE_SOLVED, L.SOLVE_BOUND_EXACT, rows.exact[i]), (name, i, a)
            assert (a.outcome, a.final_age) == (rows.outcome[i], rows.final_age[i])
            if rows.nodes is not None:
                assert a.nodes == rows.nodes[i]
        # and it is the search without a window, field for field
        for i in pick[::16]:
            a, b = solve_host((int(rows.c0[i]), int(rows.c1[i])), window=(-42, 42)), solve_host((int(rows.c0[i]), int(rows.c1[i])), deep=True)
            assert (a.status, a.outcome, a.final_age, a.value, a.nodes) == tuple(b)


def test_every_window_gives_a_true_bound_of_its_kind(live):
    from connect4_amd import _lib as L
    for name, (rows, pick, ans) in live.items():
        for i, row in zip(pick, ans):
            for (alpha, beta), a in zip(WINDOWS, row):
                assert a.status == L.SOLVE_SOLVED
                assert cases.consistent(a.score, a.bound, alpha, beta, rows.exact[i]), (name, i, (alpha, beta), a, rows.exact[i])
                if a.bound == L.SOLVE_BOUND_EXACT:
                    assert (a.outcome, a.final_age) == (rows.outcome[i], rows.final_age[i]) and a.value is not None
                else:
                    assert (a.outcome, a.final_age, a.value) == (None, -1, None)


def test_a_narrower_window_never_enters_more_nodes(live):
    """Fail-hard alpha-beta with an ordering that does not depend on the window: the tree under (a, b) is a subtree of the
    tree under any window that contains it.  On the live rows, and on every row of the golden file."""
    for name, (rows, pick, ans) in live.items():
        nodes = np.array([[a.nodes for a in row] for row in ans])
        for inner, outer in CONTAINS:
            assert (nodes[:, inner] <= nodes[:, outer]).all(), (name, WINDOWS[inner], WINDOWS[outer])
    for name, (_, _, nodes) in cases.golden().items():
        for inner, outer in CONTAINS:
            assert (nodes[:, inner] <= nodes[:, outer]).all(), (name, WINDOWS[inner], WINDOWS[outer])


def test_the_golden_file_is_the_live_host_mirror(live):
    """tests/golden/solver_window.npz row for row on the cheap rows; on all rows it is consistent with the exact scores and
    its full-window column is the fixtures' node counts (the issue's host-mirror totals among them)."""
    gold = cases.golden()
    for name, (rows, pick, ans) in live.items():
        score, bound, nodes = gold[name]
        assert score.shape == (len(rows.c0), len(WINDOWS))
        got = np.array([[(a.score, a.bound, a.nodes) for a in row] for row in ans])
        assert np.array_equal(got[:, :, 0], score[pick]) and np.array_equal(got[:, :, 1], bound[pick]) and np.array_equal(got[:, :, 2], nodes[pick])
        for wi, (alpha, beta) in enumerate(WINDOWS):
            assert cases.consistent(score[:, wi], bound[:, wi], alpha, beta, rows.exact).all(), (name, alpha, beta)
        if rows.nodes is not None:
            assert np.array_equal(nodes[:, 0], rows.nodes)
    assert gold["solver_open.npz"][2][:, 0].sum() == 551788 and gold["solver_open.npz"][2][:, 1].sum() == 259422


def same_answer(a, b, alpha, beta, exact):
    from connect4_amd import _lib as L
    return (a.status == b.status and a.bound == b.bound and cases.consistent(a.score, a.bound, alpha, beta, exact)
            and (a.bound != L.SOLVE_BOUND_EXACT or (a.score, a.outcome, a.final_age) == (b.score, b.outcome, b.final_age)))


@pytest.mark.parametrize("order", ["windows forward", "windows backward", "exact first", "exact last"])
def test_a_shared_dict_table_changes_no_answer(live, order):
    from connect4_amd.solver import solve_host
    table = {}
    windows = list(enumerate(WINDOWS))
    windows = {"windows forward": windows, "windows backward": windows[::-1], "exact first": windows,
               "exact last": windows[1:] + windows[:1]}[order]
    used = 0
    for name in ("solver_deep.npz", "solver_open.npz"):
        rows, pick, ans = live[name]
        for k in range(0, len(pick), 5):
            i = pick[k]
            if rows.nodes[i] > 4000:
                continue
            for wi, w in windows:
                a = solve_host((int(rows.c0[i]), int(rows.c1[i])), table=table, window=w)
                assert same_answer(a, ans[k][wi], w[0], w[1], rows.exact[i]), (name, i, w, a, ans[k][wi])
                assert a.nodes <= ans[k][wi].nodes or len(table)      # a table never needs to help, and never changes the answer
                used += 1
    assert used >= 200 and len(table) > 1000


def test_a_host_table_filled_by_windowed_searches_audits_clean(live):
    """Entries written under narrow windows are true bounds of their positions: 2^10 entries, always-replace, every entry
    left at the end checked against the position's exact score."""
    import solver_audit
    from connect4_amd.solver import HostTable, solve_host
    table = HostTable(10)
    rows, pick, ans = live["solver_deep.npz"]
    for k in range(0, len(pick), 3):
        i = pick[k]
        if not 64 <= rows.nodes[i] <= 3000:
            continue
        for wi in (1, 2, 3, 4, 5, 0, 3, 1):
            w = WINDOWS[wi]
            a = solve_host((int(rows.c0[i]), int(rows.c1[i])), table=table, window=w)
            assert same_answer(a, ans[k][wi], w[0], w[1], rows.exact[i]), (i, w, a)
    report = {}
    bad = solver_audit.audit(table.words, 10, solver_audit.host_oracle(), report)
    print(solver_audit.summary(report), "; stores %d, replaced %d, hits %d" % (table.stores, table.replaced, table.hits))
    assert not bad, bad[:5]
    assert report["entries"] >= 512 and report["left_out"] == 0 and table.replaced > 0 and table.hits > 0
    assert min(report["lower"], report["upper"], report["exact"]) > 0


# -- the staged labelling --------------------------------------------------------------------------------------------------
def labelled_fixture():
    """(rows uint64 [n, 2], outcome code int [n], child outcome code int [n, 7] (-1: none), legal [n, 7]) from the fixtures
    that hold their children's exact answers: the open roots that are cheap with their children, and solver.npz."""
    z = load_npz("solver_open.npz")
    pick = [i for i in range(len(z["c0"])) if z["nodes"][i] + z["child_nodes"][i].sum() <= HOST_NODE_CAP]
    rows = [np.stack([z["c0"][pick], z["c1"][pick]], axis=1).astype(np.uint64)]
    outcome = [np.rint(z["outcome"][pick] * 2).astype(np.int64)]
    legal = [z["child_legal"][pick].astype(np.int64)]
    kids = [np.where(legal[0] != 0, np.rint(np.nan_to_num(z["child_outcome"][pick]) * 2), -1).astype(np.int64)]
    s = load_npz("solver.npz")
    code = lambda v: np.where(v > 0.9, 2, np.where(v < 0.1, 0, 1))  # noqa: E731
    rows.append(np.stack([s["c0"], s["c1"]], axis=1).astype(np.uint64))
    outcome.append(code(s["root_search"]))
    lg = np.zeros((len(s["c0"]), 7), dtype=np.int64)
    ko = np.full((len(s["c0"]), 7), -1, dtype=np.int64)
    for i in range(len(s["c0"])):
        for m, v in zip(s["child_names"][i], s["child_abs"][i]):
            if m >= 0:
                lg[i, m], ko[i, m] = 1, code(v)
    legal.append(lg)
    kids.append(ko)
    return np.concatenate(rows), np.concatenate(outcome), np.concatenate(kids), np.concatenate(legal)


@pytest.mark.parametrize("table", ["none", "dict", "HostTable"])
def test_staged_labels_are_prior_from_children_on_exact_outcomes(table):
    from connect4_amd import _lib as L
    from connect4_amd.solver import HostTable, label, label_values, prior_from_children
    rows, outcome, kids, legal = labelled_fixture()
    assert len(rows) >= 90 and sorted(set(outcome.tolist())) == [0, 1, 2]
    want_priors = prior_from_children(outcome, kids, legal).astype(np.float32)
    assert (want_priors.sum(axis=1) > 0.99).all()
    t = {"none": None, "dict": {}, "HostTable": HostTable(12)}[table]
    doubled = np.concatenate([rows, rows[::-1]])        # duplicates: each distinct position once, in the order of first occurrence
    ls, report = label(doubled, exact=False, host=True, table=t)
    assert np.array_equal(ls.boards.numpy().view(np.uint64), rows)
    assert np.array_equal(ls.values.numpy(), outcome.astype(np.float32) * np.float32(0.5))
    assert ls.priors.dtype == ls.values.dtype and np.array_equal(ls.priors.numpy(), want_priors)
    assert report["positions"] == 2 * len(rows) and report["distinct"] == report["labelled"] == report["solved"] == len(rows)
    assert report["exact"] is False and report["unknown"] == report["stage1_unknown"] == report["stage2_unknown"] == 0
    assert report["nodes"] == report["stage1_nodes"] + report["stage2_nodes"] and report["stage1_rows"] == len(rows)
    assert 0 < report["stage2_rows"] <= int(((legal != 0) & (outcome >= 0)[:, None]).sum())
    if table == "none":
        vs, vreport = label_values(doubled, host=True)
        assert vs.priors is None and np.array_equal(vs.boards.numpy(), ls.boards.numpy()) and np.array_equal(vs.values.numpy(), ls.values.numpy())
        assert vreport["nodes"] == vreport["stage1_nodes"] == report["stage1_nodes"] and vreport["stage2_rows"] == 0
        # a tight budget: what is labelled is labelled the same, the rest is counted as unknown, stage by stage
        few, r = label(rows, exact=False, host=True, node_budget=300)
        at = {tuple(b): k for k, b in enumerate(rows.tolist())}
        idx = [at[tuple(b)] for b in few.boards.numpy().view(np.uint64).tolist()]
        assert 0 < len(few) < len(rows) and idx == sorted(idx)
        assert np.array_equal(few.values.numpy(), ls.values.numpy()[idx]) and np.array_equal(few.priors.numpy(), want_priors[idx])
        assert r["unknown"] == len(rows) - len(few) and r["stage1_unknown"] > 0 and r["unknown"] >= r["stage1_unknown"]


def test_mirror_images_are_searched_once_in_stage_two():
    """Parents and their mirror images: the children are each other's images and make one stage-2 row, and the image met
    first is the one that is searched -- so the originals' stage 2 is entered node for node."""
    from connect4_amd.board import Board
    from connect4_amd.solver import label
    rows = labelled_fixture()[0][-32:]
    images = np.array([Board.from_bits(int(a), int(b)).create_fliplr().color for a, b in rows], dtype=np.uint64)
    assert not (images == rows).all(axis=1).any()
    alone, r1 = label(rows, exact=False, host=True)
    both, r2 = label(np.concatenate([rows, images]), exact=False, host=True)
    assert r2["stage1_rows"] == 2 * r1["stage1_rows"] == 64 and r1["stage2_rows"] > 0
    assert (r2["stage2_rows"], r2["stage2_nodes"]) == (r1["stage2_rows"], r1["stage2_nodes"])
    assert np.array_equal(both.values.numpy(), np.tile(alone.values.numpy(), 2))
    assert np.array_equal(both.priors.numpy()[32:], alone.priors.numpy()[:, ::-1])


def test_staged_labels_rule_on_a_scripted_solver():
    """staged_labels around a window_solver that answers from a script: the windows it asks for, what it skips, how unknown
    rows propagate, and the invariant."""
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    from connect4_amd.solver import _canonical, _children_host, staged_labels
    b = Board()
    for m in (3, 3, 2, 4):
        b.make_move(m)
    lost = Board()
    for m in (0, 6, 0, 6, 1):
        lost.make_move(m)
    rows = np.array([b.color, lost.color], dtype=np.uint64)
    kids, legal = _children_host(rows)
    asked = []

    def script(v, keeping, unknown=()):
        def solver(r, alpha, beta):
            asked.append((r.copy(), alpha.copy(), beta.copy()))
            if len(asked) % 2 == 1:     # stage 1
                return np.zeros(len(r), dtype=np.int8), np.array(v, dtype=np.int8), np.full(len(r), 10), np.zeros(len(r), dtype=np.int64)
            canon = [tuple(x) for x in _canonical(kids[0]).tolist()]
            cols = [canon.index(tuple(x)) for x in _canonical(r).tolist()]
            score = np.array([alpha[k] if c in keeping else beta[k] for k, c in enumerate(cols)], dtype=np.int8)
            status = np.array([L.SOLVE_UNKNOWN if c in unknown else L.SOLVE_SOLVED for c in cols], dtype=np.int8)
            return status, score, np.full(len(r), 7), np.zeros(len(r), dtype=np.int64)
        return solver

    st = staged_labels(rows, script([1, -1], {3, 4}))
    assert [a.tolist() for a in asked[0][1:]] == [[-1, -1], [1, 1]]
    assert set(asked[1][1].tolist()) == {-1} and set(asked[1][2].tolist()) == {0}        # V = +1: the null window (-1, 0)
    assert len(asked[1][0]) == st["stage2_rows"] <= 7 and st["stage2_nodes"] == 7 * st["stage2_rows"] and st["stage1_nodes"] == 20
    assert st["keep"][0].tolist() == [c in (3, 4) for c in range(7)]
    assert st["keep"][1].tolist() == legal[1].tolist() and st["outcome"].tolist() == [L.RESULT_OWIN, L.RESULT_OWIN]   # x to move and lost
    del asked[:]
    st = staged_labels(rows, script([0, -1], {1}))
    assert set(asked[1][1].tolist()) == {0} and set(asked[1][2].tolist()) == {1}         # V = 0: the null window (0, 1)
    assert st["keep"][0].tolist() == [c == 1 for c in range(7)] and st["outcome"][0] == L.RESULT_DRAW
    del asked[:]
    st = staged_labels(rows, script([1, -1], {3}, unknown={6}))
    assert st["status"].tolist() == [L.SOLVE_UNKNOWN, L.SOLVE_SOLVED] and st["stage1_unknown"] == 0 and st["stage2_unknown"] == 1
    assert st["outcome"][0] == -1 and not st["keep"][0].any()
    with pytest.raises(RuntimeError, match="no move that keeps it"):
        staged_labels(rows, script([1, -1], set()))
    del asked[:]
    st = staged_labels(rows, script([1, -1], set()), stage2=False)
    assert len(asked) == 1 and st["stage2_rows"] == 0 and st["outcome"].tolist() == [L.RESULT_OWIN, L.RESULT_OWIN]


# -- refusals and the binding -----------------------------------------------------------------------------------------------
def test_bad_windows_are_refused():
    from connect4_amd.board import Board
    from connect4_amd.solver import _window_arrays, label, solve_host
    for w in ((0, 0), (1, 0), (-43, 0), (0, 43), (0.5, 1), (-42, 42.5)):
        with pytest.raises(ValueError):
            solve_host(Board(), node_budget=4, window=w)
    assert solve_host(Board(), node_budget=4, window=(-42, 42)).nodes == 4
    for a, b in ((np.array([0, 1, 2]), np.array([1, 2, 2])), (0, np.array([1, 1, 0])), (np.zeros(2), np.ones(2)), (None, 1), (-43, 0), (0, 43)):
        with pytest.raises(ValueError):
            _window_arrays(a, b, 3)
    with pytest.raises(ValueError, match="row 2"):
        _window_arrays(np.array([0, 1, 2]), np.array([1, 2, 2]), 3)
    assert _window_arrays(None, None, 3) == (None, None)
    a, b = _window_arrays(-1, np.array([0, 1, 42]), 3)
    assert a.dtype == b.dtype == np.int8 and a.tolist() == [-1, -1, -1] and b.tolist() == [0, 1, 42]
    with pytest.raises(ValueError):
        label([Board()], exact=False, split_plies=1, host=True)
    with pytest.raises(ValueError):
        label([Board()], host=True)


def test_the_binding_and_the_header_agree():
    import ctypes as C
    from connect4_amd import _lib as L
    from connect4_amd import solver
    text = open(os.path.join(ROOT, "include", "c4_engine.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define\s+C4_SOLVE_BOUND_([A-Z]+)\s+(\d+)", text)}
    assert header == {"NONE": L.SOLVE_BOUND_NONE, "LOWER": L.SOLVE_BOUND_LOWER, "UPPER": L.SOLVE_BOUND_UPPER, "EXACT": L.SOLVE_BOUND_EXACT}
    assert (L.SOLVE_BOUND_LOWER, L.SOLVE_BOUND_UPPER, L.SOLVE_BOUND_EXACT) == (solver._LOWER, solver._UPPER, solver._EXACT)
    assert sorted(solver.BOUND_NAMES) == [0, 1, 2, 3]
    for name in ("c4_solve_window_dev", "c4_solve_window"):
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and len(args) == 16 and re.search(r"\bint %s\(" % name, text)
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, text).group(1)
        assert len(proto.split(",")) == 16
    src = open(os.path.join(ROOT, "connect4_amd", "csrc", "c4_solve.hip")).read()
    assert "int c4_solve_window_dev(" in src and "int c4_solve_window(" in src
    assert re.search(r"#define\s+C4_ABI_VERSION\s+4\b", text) and L.ABI_VERSION == 4       # additions only


def test_make_test_set_knows_the_new_modes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_test_set", os.path.join(ROOT, "tools", "make_test_set.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for argv in (["--openings", "4", "--outcome-only", "--values-only", "-o", "x.pth"],
                 ["--openings", "4", "--outcome-only", "--split-plies", "1", "-o", "x.pth"]):
        with pytest.raises(SystemExit):
            mod.main(argv)
