"""The exhaustive exact search of the oracle (oracle/c4_oracle.c c4o_exact_*) and what rests on it.

1. The oracle against the unmodified reference: tests/golden/solver.npz, 64 positions at 3..10 empty squares.
2. The oracle against itself: a fresh memo against a warm one, a memo that runs full against a large one, a position against
   its mirror image.
3. tests/golden/solver_exact.npz (7,456 positions at 1..22 empty squares, tests/golden/gen_solver_exact_golden.py) against
   the live oracle, and its strata.
4. The host mirror ``solver.solve_host`` -- the yardstick of every deeper fixture -- against that file: table-free,
   ``deep=True``, with a ``HostTable(10)`` shared by all rows, and windowed under the six windows of
   ``solver_exact_cases.windows``, table-free and against a ``HostTable(14)``.

In Python the mirror answers the whole file in 3..6 s per exact mode and in 8..19 s for the six windows of a windowed mode
(tests/golden/gen_solver_exact_golden.py has the figures), so no mode exceeds about 20 s and every mode takes all rows: none
is cut down to the rows with at most 18 empty squares.  With a HostTable(10) the table's image is audited on the way
(solver_audit.audit against the oracle), after the rows with at most 16 empty squares.

Broken one rule at a time (in a scratch copy), the mirror fails section 4: ``age - 41`` -> ``age - 40`` on 2,408 rows in
every mode; without ``& ~(opp_win >> 1)`` on 2,436 in every mode; EXACT stored where UPPER belongs on 5 rows with
HostTable(10) and 4 under the full window with HostTable(14), table-free on none; ``lo = age - 38`` on 1,437 and
``hi = 39 - age`` on 256.  ``lo = age - 40`` and ``hi = 41 - age`` loosen a true bound and change no answer (each is implied
by the other side's clip one ply on), so no comparison of answers can see them; the node counts pinned in
tests/test_solver_host.py and tests/test_solver_window_host.py do."""
import time

import numpy as np
import pytest

import solver_audit as A
import solver_exact_cases as X
from conftest import load_npz


@pytest.fixture(scope="module")
def fixture():
    z = load_npz("solver_exact.npz")
    return {k: z[k] for k in z.files}


def rows_of(z, pick):
    return [(int(a), int(b)) for a, b in zip(z["c0"][pick], z["c1"][pick])]


# -- 1. the reference ------------------------------------------------------------------------------------------------------
def test_oracle_is_the_reference_bit_for_bit(oracle):
    from connect4_amd.solver import value_from_answer
    ref = load_npz("solver.npz")
    with oracle.Exact(20) as memo:
        score, child, status = memo.scores(ref["c0"], ref["c1"])
    assert len(score) == 64 and (status == oracle.EXACT_SEARCHED).all()
    age = X.ages(ref["c0"], ref["c1"])
    assert value_from_answer(*X.answer_of_score(score, age)).tobytes() == ref["root_search"].tobytes()
    assert (score == np.where(child == X.NO_MOVE, -99, child).max(axis=1)).all()
    for i in range(64):
        names = [int(c) for c in ref["child_names"][i] if c >= 0]
        assert names == [c for c in range(7) if child[i, c] != X.NO_MOVE]
        # a child's score is held from the root's mover's side: back to the child's own mover, at the child's age
        outcome, final_age = X.answer_of_score(-child[i, names].astype(np.int64), age[i] + 1)
        # the reference's absolute_value of a finished child is the bare result, without the age term (tree.py:27-38)
        got = np.where(final_age == age[i] + 1, outcome, value_from_answer(outcome, final_age))
        assert got.tobytes() == ref["child_abs"][i][:len(names)].tobytes()


def test_oracle_statuses(oracle):
    from connect4_amd.board import Board
    won = Board()
    for m in (3, 2, 3, 2, 3, 2, 3):
        won.make_move(m)
    rows = [won.color, (0, 0), (1, 1), (2, 0), (1 << 6, 0), (0, 1), (3, 0)]        # o has won; empty; overlap; floating; off board; x first; 2-0
    with oracle.Exact(4) as memo:
        score, child, status = memo.scores_raw([r[0] for r in rows], [r[1] for r in rows])
    assert status.tolist() == [oracle.EXACT_FINISHED, oracle.EXACT_CAPACITY] + [oracle.EXACT_INVALID] * 5
    assert score.tolist() == [7 - 43, 0, 0, 0, 0, 0, 0] and (child == X.NO_MOVE).all()      # x is to move and has lost at age 7
    with pytest.raises(ValueError):
        oracle.Exact(3)


# -- 2. the oracle against itself -------------------------------------------------------------------------------------------
def test_oracle_against_itself(oracle, fixture):
    from connect4_amd.board import Board
    rng = np.random.RandomState(2)
    pick = np.sort(np.concatenate([rng.choice(np.nonzero(fixture["empties"] == e)[0], 10, replace=False) for e in range(1, 21)]))
    assert len(pick) == 200
    c0, c1 = fixture["c0"][pick], fixture["c1"][pick]
    with oracle.Exact(25) as memo:
        cold = memo.scores(c0, c1)
        entries = memo.stats()["entries"]
        warm = memo.scores(c0, c1)
        assert memo.stats()["entries"] == entries and memo.stats()["visited"] == entries          # the second pass searched nothing
        mirrored = [Board.from_bits(int(a), int(b)).create_fliplr().color for a, b in zip(c0, c1)]
        flipped = memo.scores([m[0] for m in mirrored], [m[1] for m in mirrored])
    alone = X.solve_all(oracle, c0[-40:-20], c1[-40:-20], log2_entries=20)   # 17 and 18 empty squares through other, fresh memos
    for got in (warm, (flipped[0], flipped[1][:, ::-1], flipped[2])):
        assert all(np.array_equal(a, b) for a, b in zip(got, cold))
    assert all(np.array_equal(a, b[-40:-20]) for a, b in zip(alone, cold))
    assert np.array_equal(cold[0], fixture["score"][pick]) and np.array_equal(cold[1], fixture["child_score"][pick])
    # a memo that runs full: some rows end with EXACT_CAPACITY, none loops, and every answer it does give is the large memo's
    with oracle.Exact(10) as small:
        score, child, status = small.scores_raw(c0, c1)
        assert small.stats()["entries"] <= 1024 - 128
        with pytest.raises(oracle.ExactCapacityError):
            small.scores(c0, c1)
    full = status == oracle.EXACT_CAPACITY
    assert full.any() and (~full).sum() >= 50 and (status[~full] == oracle.EXACT_SEARCHED).all()
    assert np.array_equal(score[~full], cold[0][~full]) and np.array_equal(child[~full], cold[1][~full])
    assert (score[full] == 0).all() and (child[full] == X.NO_MOVE).all()


# -- 3. the fixture ------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_live_oracle_and_has_its_strata(oracle, fixture):
    z = fixture
    n = len(z["c0"])
    assert n == 7456 and len(set(zip(z["c0"].tolist(), z["c1"].tolist()))) == n
    assert np.array_equal(z["empties"], X.SIZE - X.ages(z["c0"], z["c1"]))
    assert {int(e): int((z["empties"] == e).sum()) for e in np.unique(z["empties"])} == X.ROWS_PER_EMPTIES
    assert z["score"].dtype == np.int8 and z["child_score"].dtype == np.int8 and z["child_score"].shape == (n, 7)
    late = z["empties"] <= 16
    t0 = time.perf_counter()
    score, child, status = X.solve_all(oracle, z["c0"][late], z["c1"][late], log2_entries=24)
    print("the oracle re-solves %d rows with at most 16 empty squares in %.1f s" % (late.sum(), time.perf_counter() - t0))
    assert (status == oracle.EXACT_SEARCHED).all()
    assert np.array_equal(score, z["score"][late]) and np.array_equal(child, z["child_score"][late])
    # every row: the score is the best child's, a legal move is a column with room, an immediate win is 42 - age
    legal, wins, _, _ = X.root_facts(z["c0"], z["c1"])
    kids = z["child_score"].astype(np.int64)
    assert np.array_equal(kids != X.NO_MOVE, legal)
    assert np.array_equal(z["score"], np.where(legal, kids, -99).max(axis=1))
    assert (kids[wins] == np.broadcast_to((z["empties"].astype(np.int64))[:, None], kids.shape)[wins]).all()
    strata = X.strata(z["c0"], z["c1"], z["score"])
    for name in X.STRATA + ("tree",):
        assert np.array_equal(z[name], strata[name]), name
    counts = {name: int(z[name].sum()) for name in X.STRATA}
    print(counts)
    assert min(counts.values()) >= X.STRATUM_MIN, counts
    for e in X.ROWS_PER_EMPTIES:                          # at least half of every depth cannot win at once
        assert z["tree"][z["empties"] == e].sum() * 2 >= X.ROWS_PER_EMPTIES[e]


# -- 4. the host mirror ----------------------------------------------------------------------------------------------------------
def first_stratum(z, i):
    return [name for name in X.STRATA if z[name][i]] or ["none"]


def check_exact(z, pick, answers, label):
    from connect4_amd import _lib as L
    from connect4_amd.solver import value_from_answer
    age = 42 - z["empties"][pick].astype(np.int64)
    outcome, final_age = X.answer_of_score(z["score"][pick], age)
    bad = [k for k, a in enumerate(answers) if a.status != L.SOLVE_SOLVED or a.outcome != outcome[k] or a.final_age != final_age[k]]
    for k in bad[:5]:
        i = int(pick[k])
        print("%s: row %d (%#x, %#x), strata %s: the oracle's score %d = outcome %.1f at age %d; the mirror says %r" % (
            label, i, int(z["c0"][i]), int(z["c1"][i]), first_stratum(z, i), z["score"][i], outcome[k], final_age[k], answers[k]))
    assert not bad, "%s: %d of %d rows differ from the oracle" % (label, len(bad), len(answers))
    want = value_from_answer(outcome, final_age)
    assert np.array([a.value for a in answers], dtype=np.float64).tobytes() == want.tobytes()


@pytest.mark.parametrize("mode", ["table_free", "deep", "host_table_10"])
def test_host_mirror_exact_scores_are_the_oracles(oracle, fixture, mode):
    from connect4_amd.solver import HostTable, solve_host
    pick = np.arange(len(fixture["c0"]))
    table = HostTable(10) if mode == "host_table_10" else None
    kw = {"table_free": {"node_budget": 1 << 20}, "deep": {"deep": True, "node_budget": 1 << 20}, "host_table_10": {"table": table}}[mode]
    t0 = time.perf_counter()
    shallow = int((fixture["empties"] <= 16).sum())
    assert (np.diff(fixture["empties"].astype(np.int64)) >= 0).all()          # the rows come by rising depth
    answers = [solve_host(r, **kw) for r in rows_of(fixture, pick[:shallow])]
    if table is not None:
        # the table as the rows with at most 16 empty squares leave it: every entry a true bound of its position by the
        # oracle, and no score that the rules exclude at its age (solver_audit.audit)
        report = {}
        bad = A.audit(table.words.copy(), table.log2_entries, A.exact_oracle(oracle, 22), report)
        print(A.summary(report), bad[:5])
        assert bad == [] and report["left_out"] == 0 and min(report["lower"], report["upper"], report["exact"]) > 0
    answers += [solve_host(r, **kw) for r in rows_of(fixture, pick[shallow:])]
    print("%s: %d rows in %.1f s, %d nodes, the dearest row %d" % (mode, len(pick), time.perf_counter() - t0,
                                                                  sum(a.nodes for a in answers), max(a.nodes for a in answers)))
    check_exact(fixture, pick, answers, mode)
    if table is not None:
        assert table.hits > 0 and table.replaced > 0


@pytest.mark.parametrize("mode", ["table_free", "host_table_14"])
def test_host_mirror_windowed_searches_obey_the_oracle(fixture, mode):
    from connect4_amd import _lib as L
    from connect4_amd.solver import HostTable, solve_host
    assert (L.SOLVE_BOUND_LOWER, L.SOLVE_BOUND_UPPER, L.SOLVE_BOUND_EXACT) == (1, 2, 3)
    pick = np.arange(len(fixture["c0"]))
    rows = rows_of(fixture, pick)
    exact = fixture["score"][pick].astype(np.int64)
    table = HostTable(14) if mode == "host_table_14" else None
    t0 = time.perf_counter()
    kinds = set()
    for name, alpha, beta in X.windows(fixture["score"])[:]:
        alpha, beta = alpha[pick], beta[pick]
        ans = [solve_host(r, table=table, window=(int(a), int(b))) for r, a, b in zip(rows, alpha, beta)]
        assert all(a.status == L.SOLVE_SOLVED for a in ans)
        score, bound = np.array([a.score for a in ans]), np.array([a.bound for a in ans])
        bad = X.window_violations(score, bound, alpha, beta, exact)
        for k in bad[:5]:
            i = int(pick[k])
            print("%s, window %s (%d, %d): row %d (%#x, %#x), strata %s: the oracle's score %d; the mirror returns %d as kind %d" % (
                mode, name, alpha[k], beta[k], i, int(fixture["c0"][i]), int(fixture["c1"][i]), first_stratum(fixture, i), exact[k],
                score[k], bound[k]))
        assert len(bad) == 0, "%s, window %s: %d of %d rows break the rule" % (mode, name, len(bad), len(rows))
        solved = bound == L.SOLVE_BOUND_EXACT
        outcome, final_age = X.answer_of_score(exact, 42 - fixture["empties"][pick].astype(np.int64))
        assert all((a.outcome, a.final_age) == ((outcome[k], final_age[k]) if solved[k] else (None, -1)) for k, a in enumerate(ans))
        kinds |= {(name, int(b)) for b in np.unique(bound)}
    print("%s: %d rows x 6 windows in %.1f s" % (mode, len(rows), time.perf_counter() - t0))
    assert {("full", 3), ("outcome", 1), ("outcome", 2), ("outcome", 3), ("null_below", 1), ("null_above", 2)} <= kinds
    assert {k for n, k in kinds if n == "full"} == {3} and {k for n, k in kinds if n.startswith("random")} == {1, 2, 3}
