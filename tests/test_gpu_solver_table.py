"""The deep search and its transposition table on the GPU (k_solve_search<DEEP_MAX_PLY, TableRef> of connect4_amd/csrc/c4_solve.hip behind
solver.solve(deep= / table= / split_plies=)): against tests/golden/solver_open.npz (25..32 empty squares, answered table-free
by the host mirror), against today's table-free search on late positions with mirror images and duplicates in the batch,
and end to end through grid_triple, label and tools/make_test_set.py --openings."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import ROOT, load_npz
from solver_helpers import boards_of, packed, same_answers, same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def fx():
    """The fixture, its boards, a packed device tensor of them (none is modified)."""
    z = load_npz("solver_open.npz")
    boards = boards_of(z["c0"], z["c1"])
    return z, boards, packed(boards)


def is_fixture(res, z):
    from connect4_amd import _lib as L
    return ((res.status == L.SOLVE_SOLVED).all() and same_bits(res.outcome, z["outcome"]) and np.array_equal(res.final_age, z["final_age"])
            and same_bits(res.value, z["value"]))


# -- 1. the 42-ply stack, table-free ---------------------------------------------------------------------------------------
def test_deep_table_free_is_the_fixture_bit_for_bit(fx):
    from connect4_amd.solver import solve
    z, boards, t = fx
    for res in (solve(t, deep=True), solve(boards, deep=True), solve(t, deep=True, nodes_per_launch=256)):   # _dev, host, parked often
        assert is_fixture(res, z)
        assert np.array_equal(res.nodes, z["nodes"]) and (res.table_hits == 0).all()


# -- 2. with a table: size, replacement and launch quota do not matter -------------------------------------------------------
@pytest.mark.parametrize("log2_entries, per_launch", [(24, None), (10, None), (20, 256), (20, 1 << 20)])
def test_table_answers_are_the_fixture(fx, log2_entries, per_launch):
    from connect4_amd.solver import Table, solve
    z, boards, t = fx
    with Table(log2_entries) as table:
        assert table.entries == 1 << log2_entries
        res = solve(t, table=table, nodes_per_launch=per_launch)
        print("2^%d entries, quota %s: nodes %d (table-free %d), hits %d" % (log2_entries, per_launch, res.nodes.sum(), z["nodes"].sum(),
                                                                        res.table_hits.sum()))
        assert is_fixture(res, z) and (res.nodes >= 1).all() and (res.table_hits >= 0).all()
        if log2_entries == 24 and per_launch is None:
            assert is_fixture(solve(boards, table=table), z)            # c4_solve_deep, from host memory


# -- 3. against today's search, mirror images and duplicates in the batch ----------------------------------------------------
def test_table_is_todays_search_on_late_positions():
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table, random_playout, solve
    rng = np.random.RandomState(33)
    roots = [random_playout(rng, 42 - (20 + i % 3)) for i in range(512)]
    rows = roots + [b.create_fliplr() for b in roots] + roots
    t = packed(rows)
    want = solve(t)
    with Table(24) as table:
        got = solve(t, table=table)
    print("nodes: table-free %d, table %d, hits %d" % (want.nodes.sum(), got.nodes.sum(), got.table_hits.sum()))
    assert not (want.status == L.SOLVE_UNKNOWN).any() and not (got.status == L.SOLVE_UNKNOWN).any()
    assert same_answers(got, want) and (got.status == L.SOLVE_SOLVED).all()
    assert got.table_hits.sum() > 0 and (got.nodes >= 1).all()


# -- 4. a warm table ---------------------------------------------------------------------------------------------------------
def test_a_warm_table_answers_the_same_with_fewer_nodes(fx):
    from connect4_amd.solver import Table, solve
    z, _, t = fx
    with Table(24) as table:
        first = solve(t, table=table)
        second = solve(t, table=table)
        table.clear()
        third = solve(t, table=table)
    print("nodes: first %d, second %d, after clear %d" % (first.nodes.sum(), second.nodes.sum(), third.nodes.sum()))
    assert is_fixture(first, z) and is_fixture(second, z) and is_fixture(third, z)
    assert second.nodes.sum() < first.nodes.sum() and third.nodes.sum() > second.nodes.sum()


# -- 5. the split ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split_plies", [1, 2])
def test_split_gives_the_answers_of_no_split(fx, split_plies):
    from connect4_amd.solver import Table, solve
    z, boards, t = fx
    with Table(22) as table:
        res = solve(t, table=table, split_plies=split_plies)
        assert is_fixture(res, z) and (res.nodes >= 0).all()
        if split_plies == 1:
            assert is_fixture(solve(boards, split_plies=1), z)              # table-free, from Boards


def test_split_nodes_are_the_sums_over_the_graphs_last_level(fx):
    """Table-free node counts are deterministic: two plies below the fixture's 12 cheapest rows a row's nodes are the nodes of
    solve(deep=True) summed over its distinct last-level nodes of the graph -- the batch and the way back are the graph's."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import _build_graph, _children_of, solve
    z = fx[0]
    cost = z["nodes"] + z["child_nodes"].sum(axis=1)
    pick = np.argsort(cost, kind="stable")[:12]
    assert cost[pick].max() <= 4096
    rows = np.stack([z["c0"], z["c1"]], axis=1)[pick]
    res = solve(packed(rows), split_plies=2)
    g = _build_graph(rows, None, None, 2, _children_of(0))
    first_leaf = int(g.level_start[-2])
    per_node = np.zeros(len(g.child), dtype=np.int64)
    per_node[first_leaf:] = solve(packed(np.stack([g.color0[first_leaf:], g.color1[first_leaf:]], axis=1)), deep=True).nodes

    def leaves_below(node):
        if node >= first_leaf:
            return {node}
        return set().union(*[leaves_below(int(c)) for c in g.child[node] if c >= 0])

    want = [int(per_node[sorted(leaves_below(int(i)))].sum()) for i in g.inverse]
    assert min(want) > 0 and res.nodes.tolist() == want
    assert (res.status == L.SOLVE_SOLVED).all() and (res.table_hits == 0).all()
    assert same_bits(res.outcome, z["outcome"][pick]) and np.array_equal(res.final_age, z["final_age"][pick])


# -- 6. grid_triple and label -------------------------------------------------------------------------------------------------
def test_grid_triple_and_label_with_a_table(fx):
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table, grid_triple, label
    z, boards, t = fx
    legal = z["child_legal"] != 0
    with Table(22) as table:
        triples = grid_triple(boards, table=table)
        ls, report = label(t, table=table)
        split = grid_triple(boards[:16], table=table, split_plies=1)
    for i, (move, value, tree) in enumerate(triples):
        cols = np.nonzero(legal[i])[0]
        # a finished child's absolute_value is its result (tree.py:27-38), any other child's its exact value
        vals = np.where(z["child_status"][i][cols] == L.SOLVE_TERMINAL, z["child_outcome"][i][cols], z["child_value"][i][cols])
        assert [c.name for c in tree.root.children] == cols.tolist()
        assert same_bits([c.data.absolute_value for c in tree.root.children], vals)
        assert same_bits(tree.root.data.search_value, z["value"][i])
        best = vals.max() if boards[i].age % 2 == 0 else vals.min()
        assert move == int(cols[vals == best].max()) and same_bits(value, best)       # Tree.best_move: ties go to the higher column
        if i < 16:
            assert (split[i][0], np.float64(split[i][1]).tobytes()) == (move, np.float64(value).tobytes())
    n = len(boards)
    assert len(ls) == n == report["labelled"] == report["solved"] and report["unknown"] == report["too_deep"] == 0
    assert report["table_log2_entries"] == 22 and report["table_hits"] > 0 and report["nodes"] > 0
    assert np.array_equal(ls.boards.cpu().numpy().view(np.uint64), np.stack([z["c0"], z["c1"]], axis=1))
    assert np.array_equal(ls.values.cpu().numpy(), z["outcome"].astype(np.float32))
    keep = legal & (z["child_outcome"] == z["outcome"][:, None])
    want = (keep / keep.sum(axis=1, keepdims=True)).astype(np.float32)
    assert np.array_equal(ls.priors.cpu().numpy(), want)


# -- 7. the statuses -----------------------------------------------------------------------------------------------------------
def test_the_budget_never_lies_with_a_table(fx):
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table, solve
    z, _, t = fx
    for table in (None, Table(20)):
        got = solve(t, node_budget=64, table=table, deep=True)
        unknown = got.status == L.SOLVE_UNKNOWN
        assert unknown.any() and (~unknown).any() and np.isin(got.status, (L.SOLVE_SOLVED, L.SOLVE_UNKNOWN)).all()
        assert (got.nodes[unknown] == 64).all() and np.isnan(got.value[unknown]).all() and (got.final_age[unknown] == -1).all()
        assert same_bits(got.value[~unknown], z["value"][~unknown]) and np.array_equal(got.final_age[~unknown], z["final_age"][~unknown])
        assert (got.nodes[~unknown] <= 64).all()
        if table is None:
            assert np.array_equal(unknown, z["nodes"] > 64)
        else:
            table.close()


def test_finished_and_invalid_rows_among_deep_neighbours(fx):
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    from connect4_amd.solver import Table, solve, solve_host
    z, boards, _ = fx
    cheap = [i for i in np.argsort(z["nodes"], kind="stable")[:24]]
    won = Board()
    for m in (3, 2, 3, 2, 3, 2, 3):
        won.make_move(m)
    c0, c1 = boards[cheap[0]].color
    specials = [(won.color[0], won.color[1], L.SOLVE_TERMINAL), (c0, c1 | (c0 & -c0), L.SOLVE_INVALID),
                (0b1111 | 1 << 14, 0b1111 << 7, L.SOLVE_INVALID), (c0 | 1 << 48, c1, L.SOLVE_INVALID)]
    with Table(16) as table:
        for n in (1, 63, 65, 257):
            src = [cheap[i % len(cheap)] for i in range(n)]
            rows = [tuple(boards[i].color) for i in src]
            where = {}
            for k, sp in enumerate(specials):
                if 1 + 5 * k < n:
                    rows[1 + 5 * k] = sp[:2]
                    where[1 + 5 * k] = sp
            t = torch.from_numpy(np.array(rows, dtype=np.uint64).view(np.int64)).cuda()
            for got in (solve(t, table=table), solve(t, deep=True), solve(rows, table=table)):
                for at in range(n):
                    if at in where:
                        h = solve_host(where[at][:2])
                        assert got.status[at] == where[at][2] == h.status and got.nodes[at] == 0 and got.final_age[at] == h.final_age
                        if h.status == L.SOLVE_TERMINAL:
                            assert got.outcome[at] == h.outcome and same_bits(got.value[at], h.value)
                        else:
                            assert np.isnan(got.outcome[at]) and np.isnan(got.value[at])
                    else:
                        i = src[at]
                        assert got.status[at] == L.SOLVE_SOLVED and got.final_age[at] == z["final_age"][i]
                        assert same_bits(got.value[at], z["value"][i])
    empty = solve(torch.zeros((0, 2), dtype=torch.int64).cuda(), deep=True)
    assert len(empty.status) == 0 and len(solve([], deep=True).table_hits) == 0


def test_table_sizes_out_of_range_are_refused():
    import ctypes as C
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table
    lib = L.load()
    for bad in (9, 31):
        h = C.c_void_p()
        assert lib.c4_solve_table_create(0, bad, C.byref(h)) == L.EINVAL and not h.value
        with pytest.raises(L.EngineError) as e:
            Table(bad)
        assert e.value.code == L.EINVAL
    t = Table(10)
    t.close()
    t.close()
    with pytest.raises(ValueError):
        t.clear()


# -- 8. end to end -------------------------------------------------------------------------------------------------------------
def test_make_test_set_openings_end_to_end(tmp_path, capsys):
    from connect4_amd.stats import LabelledSet
    out = os.path.join(str(tmp_path), "open.pth")
    spec = importlib.util.spec_from_file_location("make_test_set", os.path.join(ROOT, "tools", "make_test_set.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(["--openings", "30", "--count", "64", "--seed", "3", "--table-log2", "20", "--node-budget", "2048", "-o", out])
    printed = capsys.readouterr().out
    report = json.loads(printed.splitlines()[0])
    print("unknown: %d of %d" % (report["unknown"], report["distinct"]))
    ls = LabelledSet.load(out, device="cuda")
    assert report["positions"] == report["distinct"] == 64 and report["openings"] == 30 and report["table_log2_entries"] == 20
    assert report["solved"] + report["unknown"] + report["terminal"] + report["too_deep"] + report["invalid"] == 64
    assert report["terminal"] == report["too_deep"] == report["invalid"] == 0
    assert report["labelled"] == len(ls) == report["solved"] and "positions labelled" in printed
    bits = ls.boards.cpu().numpy().view(np.uint64)
    assert len(ls) == 0 or all(bin(int(a | b)).count("1") == 30 for a, b in bits)
    if len(ls):
        sums = ls.priors.sum(dim=1).cpu().numpy()
        assert np.allclose(sums, 1.0, rtol=0, atol=2e-7) and set(ls.values.cpu().numpy().tolist()) <= {0.0, 0.5, 1.0}
