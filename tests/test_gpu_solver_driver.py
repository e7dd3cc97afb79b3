"""The root driver on the GPU (c4_solve_graph of connect4_amd/csrc/c4_solve.hip behind solver.solve_graph and the driver_plies
keyword): bit for bit against the host mirror's answers and per-node reports in tests/golden/solver_driver.npz
(tests/test_solver_driver_host.py holds that file to solver.drive_host), against tests/golden/solver_exact.npz with tables, and
against the undriven calls."""
import importlib.util
import os

import numpy as np
import pytest

import solver_audit as A
import solver_driver_cases as D
import solver_exact_cases as E
from conftest import ROOT
from solver_helpers import gpu_oracle, packed

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def golden():
    return D.golden_cases()


@pytest.fixture(scope="module")
def z():
    return D.exact_rows()


def device_children(level):
    from connect4_amd.solver import _children_of
    return _children_of(0)(level)


def graph_of(case):
    from connect4_amd.solver import _build_graph
    return _build_graph(case.rows, case.alpha, case.beta, case.plies, device_children)


def is_golden(case, want, answers, report, g):
    status, score, bound, outcome, final_age, nodes, hits = (np.asarray(x)[g.inverse] for x in answers)
    out = np.where(outcome < 0, np.nan, outcome * 0.5)
    ok = {"status": np.array_equal(status, want["status"]), "score": np.array_equal(score, want["score"]),
          "bound": np.array_equal(bound, want["bound"]), "outcome": np.array_equal(out, want["outcome"], equal_nan=True),
          "final_age": np.array_equal(final_age, want["final_age"]), "nodes": np.array_equal(nodes, want["nodes"]),
          "lo": np.array_equal(report["lo"], want["lo"]), "hi": np.array_equal(report["hi"], want["hi"]),
          "state": np.array_equal(report["state"], want["state"]), "node_nodes": np.array_equal(report["nodes"], want["node_nodes"]),
          "hits": not hits.any() and not report["table_hits"].any()}
    bad = [k for k, v in ok.items() if not v]
    assert not bad, (case.name, bad)


def test_every_golden_case_is_the_host_mirror_bit_for_bit(golden):
    """Rows, intervals, states and node counts, at the quota the case was written with: 256 and 16 make rows park, so that
    fold, mark-down and filter run between launches; the budget of 64 leaves rows unknown."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_graph
    parked = dropped_late = 0
    for case, want in golden:
        g = graph_of(case)
        answers, report = solve_graph(g, node_budget=case.budget, nodes_per_launch=case.quota)
        is_golden(case, want, answers, report, g)
        parked += int((want["node_nodes"] > 1 + case.quota).sum())
        dropped_late += int(((want["state"] == L.SOLVE_NODE_DROPPED) & (want["node_nodes"] > 1)).sum())
    print("%d cases; %d leaves parked at least once, %d were dropped after a launch" % (len(golden), parked, dropped_late))
    assert parked > 100 and dropped_late > 10


def test_the_public_call_is_the_golden_case_from_packed_rows_and_from_boards(golden):
    from connect4_amd.solver import solve_window
    for case, want in golden:
        if not case.name.startswith(("batch", "open")):
            continue
        for boards in (packed(case.rows), [(int(a), int(b)) for a, b in case.rows]):
            res = solve_window(boards, case.alpha, case.beta, node_budget=case.budget, nodes_per_launch=case.quota, driver_plies=case.plies)
            for f in D.ROW_FIELDS:
                assert np.array_equal(getattr(res, f), want[f], equal_nan=f == "outcome"), (case.name, f)


@pytest.mark.parametrize("log2_entries", [10, 20])
def test_a_table_changes_no_status_kind_or_exact_score(golden, z, log2_entries):
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table, solve_graph
    lookup = {(int(a), int(b)): int(s) for a, b, s in zip(z["c0"], z["c1"], z["score"])}
    with Table(log2_entries) as table:
        for case, want in golden:
            if case.budget != D.AMPLE or case.quota != 256 or case.name.startswith("open"):
                continue
            g = graph_of(case)
            answers, report = solve_graph(g, nodes_per_launch=case.quota, table=table)
            status, score, bound = (np.asarray(x)[g.inverse] for x in answers[:3])
            assert np.array_equal(status, want["status"]) and np.array_equal(bound, want["bound"]), case.name
            ex = bound == L.SOLVE_BOUND_EXACT
            assert np.array_equal(score[ex], want["score"][ex])
            keys = [(int(a), int(b)) for a, b in case.rows]
            searched = status == L.SOLVE_SOLVED
            exact = np.array([lookup.get(k, 0) for k in keys], dtype=np.int64)
            assert len(E.window_violations(score[searched], bound[searched], case.alpha[searched].astype(np.int64),
                                           case.beta[searched].astype(np.int64), exact[searched])) == 0
            assert not np.isin(report["state"], (L.SOLVE_NODE_PENDING, L.SOLVE_NODE_OVER_BUDGET)).any()
        report = {}
        bad = A.audit(table.read(), log2_entries, gpu_oracle(20, 1 << 16), report)
        print("2^%d entries: %s; %d violations" % (log2_entries, A.summary(report), len(bad)))
        assert report["entries"] > 0 and not bad, bad[:5]


def test_the_driver_agrees_with_the_undriven_search(golden):
    """Wherever solve_window without a driver answers a row, the driven call's kind equals it, and so does the score where the
    kind is EXACT; rows that answer for themselves answer the same.  Both sides are device calls."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_window
    for case, _ in golden:
        if not case.name.endswith(("ample", "k2", "k3")):
            continue
        t = packed(case.rows)
        plain = solve_window(t, case.alpha, case.beta)
        driven = solve_window(t, case.alpha, case.beta, driver_plies=case.plies, nodes_per_launch=case.quota)
        both = (plain.status == L.SOLVE_SOLVED) & (driven.status == L.SOLVE_SOLVED)
        assert np.array_equal(plain.status, driven.status), case.name
        assert np.array_equal(plain.bound[both], driven.bound[both])
        ex = both & (plain.bound == L.SOLVE_BOUND_EXACT)
        assert np.array_equal(plain.score[ex], driven.score[ex]) and np.array_equal(plain.final_age, driven.final_age)
        assert np.array_equal(plain.outcome, driven.outcome, equal_nan=True)


def test_a_graph_that_ends_in_an_empty_level_is_folded_without_a_search(golden):
    """An all-finished-or-invalid batch and rows with fewer empty squares than driver_plies: the last level is empty, the fold
    reads no child that is not there, and the answers are the host mirror's."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_graph
    for case, want in golden:
        if case.name not in ("all_self_k2", "short_k3"):
            continue
        g = graph_of(case)
        assert g.level_start[-1] == g.level_start[-2]
        for quota in (case.quota, None):
            answers, report = solve_graph(g, nodes_per_launch=quota)
            is_golden(case, want, answers, report, g)
        assert not np.isin(report["state"], (L.SOLVE_NODE_ANSWERED, L.SOLVE_NODE_DROPPED, L.SOLVE_NODE_OVER_BUDGET)).any()


@pytest.mark.parametrize("log2_entries", [None, 20])
def test_driven_labels_are_the_undriven_ones(z, log2_entries):
    from connect4_amd.solver import Table, label, label_values, outcomes
    idx = np.nonzero((z["empties"] >= 6) & (z["empties"] <= 16))[0][::23][:96]
    t = packed(np.stack([z["c0"][idx], z["c1"][idx]], axis=1).astype(np.uint64))
    table = Table(log2_entries) if log2_entries else None
    want, w_rep = label(t, exact=False, table=table)
    got, rep = label(t, exact=False, table=table, driver_plies=2)
    assert rep["driver_plies"] == 2 and rep["labelled"] == w_rep["labelled"] == len(idx) and rep["unknown"] == 0
    assert got.boards.equal(want.boards) and got.values.equal(want.values) and got.priors.equal(want.priors)
    v_want, _ = label_values(t, table=table)
    v_got, _ = label_values(t, table=table, driver_plies=2)
    assert v_got.boards.equal(v_want.boards) and v_got.values.equal(v_want.values) and v_got.priors is None
    assert np.array_equal(outcomes(t, table=table, driver_plies=2), outcomes(t, table=table))
    if table is not None:
        table.close()


def test_make_test_set_writes_the_same_file_with_the_driver(tmp_path, z):
    spec = importlib.util.spec_from_file_location("make_test_set", os.path.join(ROOT, "tools", "make_test_set.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    idx = np.nonzero((z["empties"] >= 8) & (z["empties"] <= 14))[0][::41][:24]
    rows = np.stack([z["c0"][idx], z["c1"][idx]], axis=1).astype(np.uint64)
    from connect4_amd import engine
    planes = torch.from_numpy(engine.board_planes(rows[:, 0], rows[:, 1]))
    src = tmp_path / "data.pth"
    torch.save({"boards": torch.cat([planes, planes.flip(3)])}, str(src))
    a, b = tmp_path / "plain.pth", tmp_path / "driven.pth"
    r1 = mod.main([str(src), "--min-age", "0", "--outcome-only", "-o", str(a)])
    r2 = mod.main([str(src), "--min-age", "0", "--outcome-only", "--driver-plies", "2", "-o", str(b)])
    assert r1["labelled"] == r2["labelled"] == len(idx) and r2["driver_plies"] == 2
    one, two = torch.load(str(a), weights_only=True), torch.load(str(b), weights_only=True)
    assert sorted(one) == sorted(two)
    for k in one:
        assert torch.equal(one[k], two[k]) if torch.is_tensor(one[k]) else one[k] == two[k], k
