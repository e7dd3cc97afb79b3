"""The windowed deep search on the GPU (k_solve_init / k_solve_search<DEEP_MAX_PLY, TableRef> of connect4_amd/csrc/c4_solve.hip
behind c4_solve_window / c4_solve_window_dev and solver.solve_window / outcomes / label(exact=False) / label_values): row for
row against the host mirror's answers in tests/golden/solver_window.npz (tests/test_solver_window_host.py holds that file to
solve_host), against c4_solve_deep with null windows, with tables of three sizes shared between windowed and exact calls and
audited afterwards, and the staged labelling against today's exact one.

With a table, "the same answer" is what tests/test_solver_window_host.py says: status, kind, the score where the kind is
exact, and a true bound of that kind otherwise (a stored bound that closes the window is returned as it is)."""
import importlib.util
import json
import os

import numpy as np
import pytest

import solver_audit as A
import solver_window_cases as cases
from conftest import ROOT, load_npz
from solver_helpers import boards_of, gpu_oracle, packed
from solver_window_cases import FIXTURES, WINDOWS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def pool():
    """Every fixture row under every window as one batch of (64 + 256 + 62) * 6 rows: rows uint64 [m, 2], alpha, beta int8
    [m], the exact score, and the host mirror's score, kind and node count of each (none is modified)."""
    gold = cases.golden()
    rows, alpha, beta, exact, score, bound, nodes, age, outcome, final_age = ([] for _ in range(10))
    for name in FIXTURES:
        f = cases.fixture_rows(name)
        for wi, (a, b) in enumerate(WINDOWS):
            rows.append(np.stack([f.c0, f.c1], axis=1))
            alpha.append(np.full(len(f.c0), a, dtype=np.int8))
            beta.append(np.full(len(f.c0), b, dtype=np.int8))
            exact.append(f.exact)
            age.append(f.age)
            outcome.append(f.outcome)
            final_age.append(f.final_age)
            for out, g in zip((score, bound, nodes), gold[name]):
                out.append(g[:, wi])
    p = {k: np.concatenate(v) for k, v in dict(rows=rows, alpha=alpha, beta=beta, exact=exact, score=score, bound=bound, nodes=nodes,
                                               age=age, outcome=outcome, final_age=final_age).items()}
    order = np.random.RandomState(11).permutation(len(p["alpha"]))       # neighbouring lanes get different windows and depths
    p = {k: v[order] for k, v in p.items()}
    p["t"] = packed(p["rows"])
    return p


def is_table_free_answer(res, p, at=slice(None)):
    """Row for row the host mirror's: status, score, kind, node count; outcome and final age exactly where the kind is exact."""
    from connect4_amd import _lib as L
    ex = p["bound"][at] == L.SOLVE_BOUND_EXACT
    return ((res.status == L.SOLVE_SOLVED).all() and np.array_equal(res.score, p["score"][at]) and np.array_equal(res.bound, p["bound"][at])
            and np.array_equal(res.nodes, p["nodes"][at]) and (res.table_hits == 0).all()
            and np.array_equal(res.final_age, np.where(ex, p["final_age"][at], -1))
            and np.array_equal(np.nan_to_num(res.outcome, nan=-1.0), np.where(ex, p["outcome"][at], -1.0)))


def is_the_same_answer(res, p, at=slice(None)):
    from connect4_amd import _lib as L
    ex = p["bound"][at] == L.SOLVE_BOUND_EXACT
    return ((res.status == L.SOLVE_SOLVED).all() and np.array_equal(res.bound, p["bound"][at])
            and cases.consistent(res.score, res.bound, p["alpha"][at], p["beta"][at], p["exact"][at]).all()
            and np.array_equal(res.score[ex], p["score"][at][ex]) and np.array_equal(res.final_age, np.where(ex, p["final_age"][at], -1))
            and np.array_equal(np.nan_to_num(res.outcome, nan=-1.0), np.where(ex, p["outcome"][at], -1.0)))


# -- 1. table-free: the host mirror row for row ----------------------------------------------------------------------------
@pytest.mark.parametrize("per_launch", [None, 256])
def test_every_fixture_row_under_every_window_is_the_host_mirror(pool, per_launch):
    from connect4_amd.solver import solve_window
    res = solve_window(pool["t"], pool["alpha"], pool["beta"], nodes_per_launch=per_launch)
    print("quota %s: %d rows, %d nodes (host mirror %d); hardest row %d nodes" % (per_launch, len(res.nodes), res.nodes.sum(), pool["nodes"].sum(),
                                                                            res.nodes.max()))
    assert is_table_free_answer(res, pool)
    assert per_launch is None or (pool["nodes"] > 100 * per_launch).any()           # rows that park and resume hundreds of times


def specials():
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    won = Board()
    for m in (3, 2, 3, 2, 3, 2, 3):
        won.make_move(m)
    c0, c1 = 0b0111, 0b0111 << 7
    return [(won.color[0], won.color[1], L.SOLVE_TERMINAL, L.RESULT_OWIN * 0.5, 7), (c0, c1 | 1, L.SOLVE_INVALID, np.nan, -1),
            (0b1111 | 1 << 14, 0b1111 << 7, L.SOLVE_INVALID, np.nan, -1), (c0 | 1 << 48, c1, L.SOLVE_INVALID, np.nan, -1)]


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_batches_mixing_windows_and_statuses(pool, n):
    """n rows drawn across fixtures and windows, finished and invalid rows among them, from device and from host memory, with
    the default quota and with 256; then under a budget of 64 nodes, which leaves exactly the rows that need more UNKNOWN."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_window
    at = np.random.RandomState(n).choice(np.nonzero(pool["nodes"] <= 1 << 14)[0], size=n, replace=False)
    if n > 1:
        at[0] = int(np.argmax(pool["nodes"] * (pool["nodes"] <= 1 << 16)))           # one row that parks under the quota of 256
    rows, alpha, beta = pool["rows"][at].copy(), pool["alpha"][at], pool["beta"][at]
    where = {}
    for k, sp in enumerate(specials()):
        if 1 + 5 * k < n:
            rows[1 + 5 * k] = sp[:2]
            where[1 + 5 * k] = sp
    plain = np.array([i not in where for i in range(n)])
    boards = [(int(a), int(b)) for a, b in rows]
    sub = {k: v[at][plain] for k, v in pool.items() if k != "t"}

    def part(res, mask):
        return type(res)(*(f[mask] for f in res))

    for res in (solve_window(packed(rows), alpha, beta), solve_window(packed(rows), alpha, beta, nodes_per_launch=256),
                solve_window(boards, alpha, beta)):
        assert is_table_free_answer(part(res, plain), sub)
        for i, sp in where.items():
            assert (res.status[i], res.score[i], res.bound[i], res.nodes[i], res.final_age[i]) == (sp[2], 0, L.SOLVE_BOUND_NONE, 0, sp[4])
            assert np.isnan(res.outcome[i]) if np.isnan(sp[3]) else res.outcome[i] == sp[3]
    for res in (solve_window(packed(rows), alpha, beta, node_budget=64), solve_window(boards, alpha, beta, node_budget=64, nodes_per_launch=16)):
        over = sub["nodes"] > 64
        got = part(res, plain)
        assert np.array_equal(got.status, np.where(over, L.SOLVE_UNKNOWN, L.SOLVE_SOLVED)) and (got.nodes[over] == 64).all()
        assert (got.score[over] == 0).all() and (got.bound[over] == L.SOLVE_BOUND_NONE).all()
        assert np.isnan(got.outcome[over]).all() and (got.final_age[over] == -1).all()
        assert is_table_free_answer(part(got, ~over), {k: v[~over] for k, v in sub.items()})
        assert n < 63 or (over.any() and (~over).any())
        for i, sp in where.items():
            assert (res.status[i], res.nodes[i]) == (sp[2], 0)


# -- 2. null windows are c4_solve_deep --------------------------------------------------------------------------------------
def test_null_windows_are_the_deep_search_bit_for_bit():
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table, solve, solve_window
    f = [cases.fixture_rows(name) for name in FIXTURES]
    rows = np.concatenate([np.stack([x.c0, x.c1], axis=1) for x in f])
    exact = np.concatenate([x.exact for x in f])
    t, boards = packed(rows), [(int(a), int(b)) for a, b in rows]
    want = solve(t, deep=True)
    for res in (solve_window(t, None, None), solve_window(boards, None, None), solve_window(t, None, None, nodes_per_launch=256),
                solve_window(t, -42, 42)):
        assert np.array_equal(res.status, want.status) and np.array_equal(res.nodes, want.nodes) and np.array_equal(res.final_age, want.final_age)
        assert res.outcome.tobytes() == want.outcome.tobytes() and (res.table_hits == 0).all()
        assert np.array_equal(res.score, exact) and (res.bound == L.SOLVE_BOUND_EXACT).all()
    for budget in (64, 1000):
        a, b = solve_window(t, None, None, node_budget=budget), solve(t, deep=True, node_budget=budget)
        assert np.array_equal(a.status, b.status) and np.array_equal(a.nodes, b.nodes) and np.array_equal(a.final_age, b.final_age)
        assert (a.status == L.SOLVE_UNKNOWN).any() and (a.nodes[a.status == L.SOLVE_UNKNOWN] == budget).all()
    with Table(12) as one, Table(12) as two:        # one lane: the stores are in program order, so the two images are one
        for i in (5, 100, 200, 330):
            a, b = solve_window(t[i:i + 1], None, None, table=one), solve(t[i:i + 1], table=two)
            assert (a.nodes[0], a.table_hits[0], a.final_age[0]) == (b.nodes[0], b.table_hits[0], b.final_age[0])
            assert np.array_equal(one.read(), two.read())


# -- 3. tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2_entries", [10, 14, 24])
def test_tables_shared_between_windowed_and_exact_searches_change_no_answer(pool, log2_entries):
    from connect4_amd.solver import Table, solve, solve_window
    z = load_npz("solver_open.npz")
    open_t = packed(np.stack([z["c0"], z["c1"]], axis=1))

    def exact_is_fixture(res):
        return (res.status == 0).all() and np.array_equal(res.final_age, z["final_age"]) and res.outcome.tobytes() == z["outcome"].tobytes()

    with Table(log2_entries) as table:
        first = solve_window(pool["t"], pool["alpha"], pool["beta"], table=table)       # filled by windowed searches
        assert is_the_same_answer(first, pool)
        exact = solve(open_t, table=table)                                              # then used by exact ones
        assert exact_is_fixture(exact)
        again = solve_window(pool["t"], pool["alpha"], pool["beta"], table=table, nodes_per_launch=256)
        assert is_the_same_answer(again, pool)
        table.clear()
        cold = solve(open_t, table=table)                                               # the reverse: exact first
        assert exact_is_fixture(cold)
        after = solve_window(pool["t"], pool["alpha"], pool["beta"], table=table)
        assert is_the_same_answer(after, pool)
    print("2^%d entries: nodes table-free %d; windowed on a cold table %d (hits %d), again %d, after the exact searches %d; exact after windowed %d, "
          "exact cold %d" % (log2_entries, pool["nodes"].sum(), first.nodes.sum(), first.table_hits.sum(), again.nodes.sum(), after.nodes.sum(),
                             exact.nodes.sum(), cold.nodes.sum()))
    assert first.table_hits.sum() > 0 and (first.nodes >= 1).all()
    assert log2_entries < 24 or (first.nodes.sum() < pool["nodes"].sum() and again.nodes.sum() < first.nodes.sum())


ORACLE_MAX_EMPTIES = 20         # as tests/test_gpu_solver_table_audit.py: k_solve_search<MAX_PLY, NoTable> answers these, deeper entries get a budget
DEEP_ORACLE_BUDGET = 1 << 16


@pytest.mark.parametrize("log2_entries", [10, 14, 24])
def test_tables_written_by_windowed_searches_audit_clean(log2_entries):
    """Every row of solver_deep.npz and -- in the two small tables, which keep few entries -- the six open roots that search
    most cheaply, under the six windows, one batch, quota 256: every entry left in the table is a true bound of its
    position.  Entries with more than 20 empty squares that the table-free search does not answer within its budget are
    left out of the value check: at most 15 % may be.  (2^24 entries keep every store: checking the opening rows' would ask
    the oracle for hundreds of thousands of deep searches, so that table gets the late rows, whose entries are all
    checked.)"""
    from connect4_amd.solver import Table, solve_window
    z = load_npz("solver_open.npz")
    f = cases.fixture_rows("solver_deep.npz")
    pick = [61, 37, 0, 57, 3, 36] if log2_entries <= 14 else []
    base = np.concatenate([np.stack([f.c0, f.c1], axis=1), np.stack([z["c0"][pick], z["c1"][pick]], axis=1).astype(np.uint64)])
    rows = np.concatenate([base] * len(WINDOWS))
    alpha = np.repeat(np.array([w[0] for w in WINDOWS], dtype=np.int8), len(base))
    beta = np.repeat(np.array([w[1] for w in WINDOWS], dtype=np.int8), len(base))
    age = np.array([bin(int(a) | int(b)).count("1") for a, b in base])
    exact = np.tile(np.concatenate([f.exact, cases.mover_score(z["outcome"][pick], z["final_age"][pick], age[len(f.c0):])]), len(WINDOWS))
    with Table(log2_entries) as table:
        res = solve_window(packed(rows), alpha, beta, table=table, nodes_per_launch=256)
        assert (res.status == 0).all() and cases.consistent(res.score, res.bound, alpha, beta, exact).all()
        report = {}
        bad = A.audit(table.read(), log2_entries, gpu_oracle(ORACLE_MAX_EMPTIES, DEEP_ORACLE_BUDGET), report)
    share = report["left_out"] / report["entries"]
    print("2^%d entries: %s; %d violations; %.2f %% left out; nodes %d, hits %d" % (log2_entries, A.summary(report), len(bad), 100.0 * share,
                                                                               res.nodes.sum(), res.table_hits.sum()))
    for v in bad[:10]:
        print("   slot %d, word %#x: %s" % v)
    assert bad == [] and share <= 0.15
    assert min(report["lower"], report["upper"], report["exact"]) > 0 and res.table_hits.sum() > 0


# -- 4. the staged labelling ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def open_fx():
    z = load_npz("solver_open.npz")
    rows = np.stack([z["c0"], z["c1"]], axis=1).astype(np.uint64)
    return z, rows, packed(rows)


def same_set(a, b):
    return (torch.equal(a.boards, b.boards) and a.values.dtype == b.values.dtype and torch.equal(a.values, b.values)
            and a.priors.dtype == b.priors.dtype and torch.equal(a.priors, b.priors))


@pytest.mark.parametrize("table_log2", [None, 20])
def test_staged_labels_are_the_exact_labels_bit_for_bit(open_fx, table_log2):
    from connect4_amd.solver import Table, label
    z, rows, t = open_fx
    doubled = torch.cat([t, t.flip(0)])
    if table_log2 is None:
        exact_set, exact_report = label(doubled, deep=True)
        staged_set, report = label(doubled, exact=False)
    else:
        with Table(table_log2) as one, Table(table_log2) as two:
            exact_set, exact_report = label(doubled, table=one)
            staged_set, report = label(doubled, exact=False, table=two)
            again, warm = label(doubled, exact=False, table=one)      # on the table the exact searches filled
        assert same_set(again, exact_set) and warm["unknown"] == 0
        assert report["table_log2_entries"] == table_log2 and report["table_hits"] > 0
    print("table %s: exact %d nodes %.2f s; staged %d nodes (%d + %d over %d + %d rows) %.2f s" % (
        table_log2, exact_report["nodes"], exact_report["seconds"], report["nodes"], report["stage1_nodes"], report["stage2_nodes"],
        report["stage1_rows"], report["stage2_rows"], report["seconds"]))
    assert len(exact_set) == len(rows) and same_set(staged_set, exact_set)
    assert np.array_equal(staged_set.boards.cpu().numpy().view(np.uint64), rows)
    assert np.array_equal(staged_set.values.cpu().numpy(), z["outcome"].astype(np.float32))
    keep = (z["child_legal"] != 0) & (z["child_outcome"] == z["outcome"][:, None])
    assert np.array_equal(staged_set.priors.cpu().numpy(), (keep / keep.sum(axis=1, keepdims=True)).astype(np.float32))
    # the report, stage by stage
    assert report["exact"] is False and report["positions"] == 2 * len(rows) and report["distinct"] == report["labelled"] == report["solved"] == len(rows)
    assert report["nodes"] == report["stage1_nodes"] + report["stage2_nodes"] and report["stage1_rows"] == len(rows)
    assert report["unknown"] == report["stage1_unknown"] == report["stage2_unknown"] == 0
    assert 0 < report["stage2_rows"] <= int((z["child_legal"] != 0).sum())
    assert report["solved"] + report["unknown"] + report["terminal"] + report["too_deep"] + report["invalid"] == report["distinct"]
    if table_log2 is None:
        # the host mirror's counts: the outcome window on the roots, and the whole staged scheme (tests/test_solver_window_host.py
        # holds the first to solve_host)
        assert report["stage1_nodes"] == cases.golden()["solver_open.npz"][2][:, 1].sum() == 259422
        assert report["nodes"] < exact_report["nodes"]
        print("   table-free: staged %d nodes against %d" % (report["nodes"], exact_report["nodes"]))


def test_outcomes_and_label_values_agree_with_the_fixture(open_fx):
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table, label, label_values, outcomes
    z, rows, t = open_fx
    sp = specials()
    mixed = np.concatenate([rows, np.array([s[:2] for s in sp], dtype=np.uint64)])
    want = np.concatenate([z["outcome"], [s[3] for s in sp]])
    for got in (outcomes(packed(mixed)), outcomes([(int(a), int(b)) for a, b in mixed]), outcomes(packed(mixed), nodes_per_launch=256)):
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    tight = outcomes(t, node_budget=64)
    over = cases.golden()["solver_open.npz"][2][:, 1] > 64
    assert np.isnan(tight[over]).all() and np.array_equal(tight[~over], z["outcome"][~over]) and over.any() and (~over).any()
    with Table(20) as table:
        assert outcomes(t, table=table).tobytes() == z["outcome"].tobytes()
        vs, report = label_values(packed(mixed), table=table)
    assert vs.priors is None and np.array_equal(vs.boards.cpu().numpy().view(np.uint64), rows)
    assert np.array_equal(vs.values.cpu().numpy(), z["outcome"].astype(np.float32))
    assert (report["solved"], report["terminal"], report["invalid"], report["unknown"]) == (len(rows), 1, 3, 0)
    assert report["stage2_rows"] == report["stage2_nodes"] == 0 and report["nodes"] == report["stage1_nodes"] > 0
    few, r = label(t, exact=False, node_budget=2048)
    full, _ = label(t, exact=False)
    at = {tuple(b): k for k, b in enumerate(rows.tolist())}
    idx = [at[tuple(b)] for b in few.boards.cpu().numpy().view(np.uint64).tolist()]
    assert 0 < len(few) < len(rows) and idx == sorted(idx) and r["unknown"] == len(rows) - len(few) >= r["stage1_unknown"] > 0
    assert torch.equal(few.values, full.values[idx]) and torch.equal(few.priors, full.priors[idx])
    assert r["labelled"] == r["solved"] == len(few)
    # mirror images among the parents: their children are the images of the originals' and are searched once
    some = rows[:16]
    both = np.concatenate([some, np.array([(b.create_fliplr().color) for b in boards_of(some[:, 0], some[:, 1])], dtype=np.uint64)])
    _, r1 = label(packed(some), exact=False)
    _, r2 = label(packed(both), exact=False)
    assert r2["stage1_rows"] == 2 * r1["stage1_rows"] and r2["stage2_rows"] == r1["stage2_rows"] and r2["stage2_nodes"] == r1["stage2_nodes"]


# -- 5. refusals at the C interface -------------------------------------------------------------------------------------------
def test_bad_windows_are_refused_before_anything_runs(open_fx):
    import ctypes as C
    from connect4_amd import _lib as L
    from connect4_amd.solver import _solve_window_dev, solve_window
    _, rows, t = open_fx
    lib = L.load()
    n = 8
    bad_rows = [(np.r_[[0] * 5, 3, 0, 0], np.r_[[1] * 5, 3, 1, 1], 5), (np.r_[-43, [0] * 7], np.ones(8), 0), (np.zeros(8), np.r_[[1] * 7, 43], 7)]
    for a, b, first in bad_rows:
        a, b = a.astype(np.int8), b.astype(np.int8)
        with pytest.raises(L.EngineError) as e:
            _solve_window_dev(t[:n].contiguous(), a, b)
        assert e.value.code == L.EINVAL and "row %d" % first in str(e.value)
        c0, c1 = np.ascontiguousarray(rows[:n, 0]), np.ascontiguousarray(rows[:n, 1])
        i8 = C.POINTER(C.c_int8)
        outs = [np.full(n, 99, dtype=np.int8) for _ in range(5)]
        nodes, hits = np.full(n, -7, dtype=np.int64), np.zeros(n, dtype=np.int64)
        rc = lib.c4_solve_window(0, None, c0.ctypes.data_as(L._u64p), c1.ctypes.data_as(L._u64p), a.ctypes.data_as(i8), b.ctypes.data_as(i8), n, 0, 0,
                                 *(o.ctypes.data_as(i8) for o in outs), nodes.ctypes.data_as(L._i64p), hits.ctypes.data_as(L._i64p))
        assert rc == L.EINVAL and ("row %d" % first).encode() in lib.c4_solve_last_error()
        assert all((o == 99).all() for o in outs) and (nodes == -7).all()          # nothing was written
        one = lib.c4_solve_window(0, None, c0.ctypes.data_as(L._u64p), c1.ctypes.data_as(L._u64p), a.ctypes.data_as(i8), None, n, 0, 0,
                                  *(o.ctypes.data_as(i8) for o in outs), nodes.ctypes.data_as(L._i64p), hits.ctypes.data_as(L._i64p))
        assert one == L.EINVAL
    with pytest.raises(ValueError):
        solve_window(t, 0, 0)
    empty = solve_window(torch.zeros((0, 2), dtype=torch.int64).cuda(), -1, 1)
    assert len(empty.status) == 0 and len(solve_window([], -1, 1).score) == 0


# -- 6. end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["--outcome-only", "--values-only"])
def test_make_test_set_staged_end_to_end(tmp_path, capsys, mode):
    """The issue's command line (4-ply openings, 8 positions, a table of 2^20) under a node budget that ends it in seconds --
    at the default 2^26 nodes a row it would run for minutes -- so these rows stay unknown and the file is empty but
    loadable; the same line on 30-ply openings writes labelled rows."""
    from connect4_amd.stats import LabelledSet
    spec = importlib.util.spec_from_file_location("make_test_set", os.path.join(ROOT, "tools", "make_test_set.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for plies, count in ((4, 8), (30, 64)):
        out = os.path.join(str(tmp_path), "set%d.pth" % plies)
        tool.main(["--openings", str(plies), "--count", str(count), mode, "--table-log2", "20", "--node-budget", "2048", "-o", out])
        printed = capsys.readouterr().out
        report = json.loads([line for line in printed.splitlines() if line.startswith("{")][0])
        ls = LabelledSet.load(out, device="cuda")
        print("%d plies: %d labelled, %d unknown" % (plies, len(ls), report["unknown"]))
        assert report["mode"] == mode[2:] and report["exact"] is False and report["positions"] == report["distinct"] == count
        assert report["labelled"] == len(ls) == report["solved"] and report["solved"] + report["unknown"] == count
        assert report["nodes"] == report["stage1_nodes"] + report["stage2_nodes"] and (mode == "--outcome-only" or report["stage2_rows"] == 0)
        bits = ls.boards.cpu().numpy().view(np.uint64)
        assert all(bin(int(a | b)).count("1") == plies for a, b in bits)
        if plies == 30:
            assert len(ls) > 0 and set(ls.values.cpu().numpy().tolist()) <= {0.0, 0.5, 1.0}
            if mode == "--outcome-only":
                assert np.allclose(ls.priors.sum(dim=1).cpu().numpy(), 1.0, rtol=0, atol=2e-7)
            else:
                assert ls.priors is None
