"""The exact solver on the GPU (connect4_amd/csrc/c4_solve.hip behind connect4_amd/solver.py): against the unmodified
reference's exhaustive search (tests/golden/solver.npz, 3..10 empty squares), against the device grid search that is pinned
to it, against the host mirror's answers on deeper positions (tests/golden/solver_deep.npz, 12..20 empty squares, node counts
included), and against itself: mirror symmetry and the fold over the children.  Then the labeller and tools/make_test_set.py
end to end.

The yardsticks: up to 22 empty squares the kernel and the host mirror are both held to the oracle's exhaustive search --
tests/test_gpu_solver_exact.py and tests/test_exact_oracle.py on tests/golden/solver_exact.npz -- which shares no rule with
either and reproduces the reference's values bit for bit.  The host mirror's fixtures here add what that search does not
have, the node counts; deeper than 22 empty squares the mirror, itself held to the oracle, and the self-checks below are what
there is."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import ROOT, load_npz
from solver_helpers import boards_of, one_lane_is_the_host_model, packed, same_answers, same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ref():
    return load_npz("solver.npz")


@pytest.fixture(scope="module")
def deep():
    """The deep fixture and its answers at the default budget (computed once, shared, not modified)."""
    from connect4_amd.solver import solve
    z = load_npz("solver_deep.npz")
    boards = boards_of(z["c0"], z["c1"])
    return z, boards, solve(packed(boards))


# -- 1. the reference ------------------------------------------------------------------------------------------------------
def test_reference_fixture_bit_for_bit(ref):
    from connect4_amd import _lib as L
    from connect4_amd.solver import grid_triple, solve
    boards = boards_of(ref["c0"], ref["c1"])
    want_outcome = np.where(ref["root_search"] > 0.9, 1.0, np.where(ref["root_search"] < 0.1, 0.0, 0.5))
    for res in (solve(boards), solve(packed(boards)), solve(packed(boards, cuda=False))):       # c4_solve, c4_solve_dev (twice)
        assert (res.status == L.SOLVE_SOLVED).all() and (res.nodes >= 1).all()
        assert same_bits(res.value, ref["root_search"]) and np.array_equal(res.outcome, want_outcome)
    for i, (move, value, tree) in enumerate(grid_triple(boards)):
        assert move == int(ref["move"][i]) and same_bits(value, ref["value"][i])
        assert same_bits(tree.root.data.search_value, ref["root_search"][i])
        assert [c.name for c in tree.root.children] == [int(x) for x in ref["child_names"][i] if x >= 0]
        for c, want in zip(tree.root.children, ref["child_abs"][i]):
            assert same_bits(c.data.absolute_value, want)


# -- 2. the device grid search ---------------------------------------------------------------------------------------------
def test_grid_triple_is_the_device_grid_search():
    from connect4_amd.evaluators import evaluate_centre
    from connect4_amd.grid_search import grid_search
    from connect4_amd.solver import grid_triple, random_playout
    rng = np.random.RandomState(512)
    boards = [random_playout(rng, 42 - (3 + i % 6)) for i in range(512)]
    got = grid_triple(boards)
    for e in range(3, 9):
        idx = [i for i, b in enumerate(boards) if 42 - b.age == e]
        assert len(idx) >= 85
        for i, (m, v, t) in zip(idx, grid_search([boards[i] for i in idx], e, evaluate_centre)):
            move, value, tree = got[i]
            assert (move, np.float64(value).tobytes()) == (m, np.float64(v).tobytes())
            assert same_bits(tree.root.data.search_value, t.root.data.search_value)
            assert [c.name for c in tree.root.children] == [c.name for c in t.root.children]
            assert same_bits([c.data.absolute_value for c in tree.root.children], [c.data.absolute_value for c in t.root.children])
            assert [c.data.position_value for c in tree.root.children] == [c.data.position_value for c in t.root.children]


# -- 3. the deep fixture ---------------------------------------------------------------------------------------------------
def test_deep_fixture_at_the_default_budget(deep):
    from connect4_amd import _lib as L
    from connect4_amd import solver
    z, _, res = deep
    assert solver.DEFAULT_NODE_BUDGET >= 1 << 26 and z["nodes"].max() * 512 <= solver.DEFAULT_NODE_BUDGET
    assert not (res.status == L.SOLVE_UNKNOWN).any() and (res.status == L.SOLVE_SOLVED).all()
    assert same_bits(res.outcome, z["outcome"]) and np.array_equal(res.final_age, z["final_age"]) and same_bits(res.value, z["value"])
    assert np.array_equal(res.nodes, z["nodes"])        # the host mirror walks the same tree


# -- 4. launch boundaries --------------------------------------------------------------------------------------------------
def test_launch_boundaries_do_not_matter(deep):
    from connect4_amd.solver import solve
    _, boards, res = deep
    t = packed(boards)
    for per_launch in (256, 1 << 20):
        other = solve(t, nodes_per_launch=per_launch)
        assert same_answers(other, res) and np.array_equal(other.nodes, res.nodes)


def test_every_parked_state_crosses_a_launch_boundary():
    """With a quota of 1 node a launch a lane parks after every node it enters -- pending or not, at every depth, through
    k_solve_init's parked word and k_solve_search's -- and with 3 at every third; either way the answers and node counts are
    the default quota's and the host mirror's, on the late search, the deep search and the deep search from three windows.
    64 seeded playouts with 6..12 empty squares, with special_rows() among them -- finished and invalid rows, which are never
    searched, and a row with 25 empty squares, which is TOO_DEEP for the late search and searched by the others: 71 rows, two
    workgroups.  A run relaunches once per node of its dearest row: on every path the host mirror's dearest takes at most 512.
    Then the dearest rows one at a time against a table of 2^10 entries: one lane's table image is the host model's word for
    word at both quotas."""
    from connect4_amd.solver import HostTable, Table, random_playout, solve, solve_host, solve_window
    rng = np.random.RandomState(9)
    boards = [random_playout(rng, 42 - (6 + i % 7)) for i in range(64)]
    host_nodes = np.array([solve_host(b).nodes for b in boards])
    assert host_nodes.max() <= 512 and (host_nodes > 3).sum() >= 8         # the launches of a run; rows that park at both quotas
    rows = [tuple(b.color) for b in boards]
    for k, (c0, c1, _) in enumerate(special_rows()):
        rows.insert(1 + 9 * k, (c0, c1))
    t = packed(rows)

    def unknown_is_nan(values):
        return [np.nan if v is None else v for v in values]

    def is_host_mirror(res, **how):
        want = [solve_host(r, **how) for r in rows]
        assert max(a.nodes for a in want) <= 512, how          # the launches of this path's runs at a quota of 1
        fields = ["status", "outcome", "final_age", "nodes"] + (["score", "bound"] if "window" in how else ["value"])
        return all(same_bits(getattr(res, f), unknown_is_nan([getattr(a, f) for a in want])) for f in fields)

    def same_fields(a, b):
        return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))

    paths = [(lambda **kw: solve(t, **kw), {}), (lambda **kw: solve(t, deep=True, **kw), {"deep": True})]
    paths += [(lambda a=a, b=b, **kw: solve_window(t, a, b, **kw), {"window": (a, b)}) for a, b in ((-42, 42), (-1, 1), (0, 1))]
    for run, how in paths:
        res = run()
        assert is_host_mirror(res, **how), how
        for per_launch in (1, 3):
            assert same_fields(run(nodes_per_launch=per_launch), res), (how, per_launch)
    for per_launch in (1, 3):
        for i in np.argsort(host_nodes, kind="stable")[-3:]:
            with Table(10) as table:
                host = HostTable(10)
                nodes = one_lane_is_the_host_model(table, host, boards[i], "quota %d, %d empty squares" % (per_launch, 42 - boards[i].age), per_launch)
                assert nodes > per_launch and host.stores > 0         # the lane has parked, and the table was written


# -- 5. the budget ---------------------------------------------------------------------------------------------------------
def test_the_budget_never_lies(deep):
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve
    z, boards, res = deep
    order = np.argsort(z["nodes"], kind="stable")
    rows = np.concatenate([order[:24], order[-24:]])          # the cheapest and the dearest rows: both kinds are in the set
    assert z["nodes"][rows].min() <= 64 < z["nodes"][rows].max()
    got = solve(packed([boards[i] for i in rows]), node_budget=64)
    unknown = got.status == L.SOLVE_UNKNOWN
    assert unknown.any() and (~unknown).any()
    assert np.array_equal(unknown, z["nodes"][rows] > 64)
    assert (got.nodes[unknown] == 64).all() and np.isnan(got.value[unknown]).all() and (got.final_age[unknown] == -1).all()
    full = type(res)(*(a[rows] for a in res))
    assert same_answers(got, full, ~unknown) and np.array_equal(got.nodes[~unknown], full.nodes[~unknown])


# -- 6. statuses, partial waves and blocks ----------------------------------------------------------------------------------
def special_rows():
    """(color0, color1, status) of one row of every kind that is not searched."""
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    from connect4_amd.solver import random_playout
    rng = np.random.RandomState(6)
    won = Board()
    for m in (3, 2, 3, 2, 3, 2, 3):
        won.make_move(m)
    b = random_playout(rng, 17)                               # 25 empty squares
    c0, c1 = b.color
    h = b.height
    low = [c for c in range(7) if h[c] - 7 * c <= 3]
    return [(won.color[0], won.color[1], L.SOLVE_TERMINAL),
            (c0, c1, L.SOLVE_TOO_DEEP),
            (c0, c1 | (c0 & -c0), L.SOLVE_INVALID),                                    # the colours overlap
            (c0, c1 | 1 << (h[low[0]] + 1), L.SOLVE_INVALID),                          # a stone floats (x moves after 17: counts stay legal)
            (c0 | 1 << h[low[0]] | 1 << h[low[1]], c1, L.SOLVE_INVALID),               # o two stones ahead
            (c0, c1 | 1 << h[low[0]] | 1 << h[low[1]], L.SOLVE_INVALID),               # x ahead
            (0b1111 | 1 << 14, 0b1111 << 7, L.SOLVE_INVALID)]                          # both sides have four in a row


def test_statuses_and_neighbours(deep):
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve, solve_host
    z, boards, res = deep
    specials = special_rows()
    for c0, c1, st in specials:
        assert solve_host((c0, c1)).status == st
    for n in (1, 63, 65, 257):
        src = [i % len(boards) for i in range(n)]
        rows = [(boards[i].color[0], boards[i].color[1]) for i in src]
        where = {}
        for k, (c0, c1, st) in enumerate(specials):
            at = 1 + 7 * k
            if at < n:
                rows[at] = (c0, c1)
                where[at] = (c0, c1, st)
        t = torch.from_numpy(np.array(rows, dtype=np.uint64).view(np.int64)).cuda()
        for got in (solve(t), solve(rows)):
            valid = np.array([i not in where for i in range(n)])
            want = type(res)(*(a[src] for a in res))
            assert same_answers(got, want, valid) and np.array_equal(got.nodes[valid], want.nodes[valid])
            for at, (c0, c1, st) in where.items():
                h = solve_host((c0, c1))
                assert got.status[at] == st and got.nodes[at] == 0 and got.final_age[at] == h.final_age
                if st == L.SOLVE_TERMINAL:
                    assert got.outcome[at] == h.outcome and same_bits(got.value[at], h.value)
                else:
                    assert np.isnan(got.outcome[at]) and np.isnan(got.value[at])
    empty = solve(torch.zeros((0, 2), dtype=torch.int64).cuda())
    assert len(empty.status) == 0 and len(solve([]).nodes) == 0


# -- 7. where no yardstick exists ------------------------------------------------------------------------------------------
def test_symmetry_and_consistency_at_21_to_24_empty_squares():
    """200 seeded random playouts with 21..24 empty squares, their mirror images and their children in one batch.  The
    budget here is 2^20 nodes a row, which bounds the test's run time by the quota, not by the hardest position; rows it
    leaves UNKNOWN are excluded and may be at most 5 % of the batch."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve, random_playout, value_from_answer
    rng = np.random.RandomState(7)
    roots = [random_playout(rng, 42 - (21 + i % 4)) for i in range(200)]
    rows, kids_of = [], []
    for b in roots:
        rows.append(b)
        rows.append(b.create_fliplr())
    for b in roots:
        ks = []
        for m in sorted(b.valid_moves):
            cb = b.__copy__()
            cb.make_move(m)
            ks.append(len(rows))
            rows.append(cb)
        kids_of.append(ks)
    res = solve(packed(rows), node_budget=1 << 20)
    unknown = res.status == L.SOLVE_UNKNOWN
    print("rows %d, unknown %d, nodes: total %d, max %d" % (len(rows), unknown.sum(), res.nodes.sum(), res.nodes.max()))
    assert unknown.mean() <= 0.05
    assert np.isin(res.status, (L.SOLVE_SOLVED, L.SOLVE_TERMINAL, L.SOLVE_UNKNOWN)).all()
    checked_flip = checked_fold = 0
    for i, (b, ks) in enumerate(zip(roots, kids_of)):
        a, f = 2 * i, 2 * i + 1
        if not unknown[a] and not unknown[f]:
            assert (res.outcome[a], res.final_age[a]) == (res.outcome[f], res.final_age[f])
            checked_flip += 1
        if not unknown[a] and not unknown[ks].any():
            # a finished child's value is its terminal value: outcome and age are its own
            vals = [float(value_from_answer(res.outcome[k], res.final_age[k])) for k in ks]
            fold = max(vals) if b.age % 2 == 0 else min(vals)
            assert same_bits(res.value[a], fold)
            checked_fold += 1
    assert checked_flip >= 190 and checked_fold >= 180


# -- 8. end to end ----------------------------------------------------------------------------------------------------------
def test_make_test_set_end_to_end(tmp_path, capsys):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.data import save_generation
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import random_init_state_dict
    from connect4_amd.selfplay import SelfPlay
    from connect4_amd.stats import LabelledSet, score
    from connect4_amd.training import ModelConfig, Trainer
    d = str(tmp_path)
    sd = random_init_state_dict(seed=0)
    net = FusedNet(sd)
    sp = SelfPlay(net, 24, MCTSConfig.self_play(16), seed=1, games_target=24, record_capacity_games=24, use_graph=False,
                  fused_loop=True, steps_per_launch=16)
    for _ in range(2000):
        sp.run_steps(64)
        if sp.stats()["active_slots"] == 0:
            break
    games = sp.engine.export_games()
    sp.close()
    assert games.n_games == 24
    save_generation(games, os.path.join(d, "1"))
    out = os.path.join(d, "endgame.pth")
    # the tool's own main(), in this process: a second interpreter would spend its seconds importing torch
    spec = importlib.util.spec_from_file_location("make_test_set", os.path.join(ROOT, "tools", "make_test_set.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main([d, "--min-age", "18", "-o", out])
    printed = capsys.readouterr().out
    report = json.loads(printed.splitlines()[0])
    assert os.path.exists(out) and "positions labelled" in printed
    ls = LabelledSet.load(out, device="cuda")
    n = len(ls)
    played = games.boards.cpu().numpy().view(np.uint64)
    ages = np.array([bin(int(a | b)).count("1") for a, b in played])
    late = np.unique(played[ages >= 18], axis=0)
    assert report["distinct"] == int(late.shape[0]) and report["labelled"] == n and n > 0
    assert report["solved"] + report["unknown"] + report["terminal"] + report["too_deep"] + report["invalid"] == report["distinct"]
    assert report["terminal"] == report["too_deep"] == report["invalid"] == 0 and report["solved"] == n
    hist = {k: int((ls.values == k).sum().item()) for k in (0.0, 0.5, 1.0)}
    assert sum(hist.values()) == n
    sums = ls.priors.sum(dim=1).cpu().numpy()
    assert np.allclose(sums, 1.0, rtol=0, atol=2e-7) and (ls.priors >= 0).all()
    st = score(net, ls)
    assert st.value_stats.n == n == st.prior_stats.n and st.value_stats.total == hist
    net.close()
    tr = Trainer(ModelConfig(), device="cuda")
    ev = tr.evaluate(ls)
    assert ev.value_stats.n == n and ev.value_stats.total == hist
    # the labels are the solver's: every kept row's value is its outcome, its prior the moves that keep it
    from connect4_amd.solver import solve_host
    bits = ls.boards.cpu().numpy().view(np.uint64)
    cheap = [i for i in range(n) if bin(int(bits[i, 0] | bits[i, 1])).count("1") >= 30][:20]
    assert cheap
    for i in cheap:
        from connect4_amd.board import Board
        b = Board.from_bits(int(bits[i, 0]), int(bits[i, 1]))
        a = solve_host(b)
        assert float(ls.values[i]) == a.outcome
        keep = []
        for m in sorted(b.valid_moves):
            cb = b.__copy__()
            cb.make_move(m)
            keep.append(m) if solve_host(cb).outcome == a.outcome else None
        want = np.zeros(7, dtype=np.float32)
        want[keep] = np.float32(1.0 / len(keep))
        assert np.array_equal(ls.priors[i].cpu().numpy(), want)
