"""The review of finished games against exact play, on the host: ``review.review_host`` against tests/golden/review.npz, whose
labels come from the exhaustive oracle alone (tests/golden/gen_review_golden.py), and the rule's edges.  No GPU."""
import numpy as np
import pytest

import review_cases as RC
from conftest import load_npz


@pytest.fixture(scope="module")
def z():
    f = load_npz("review.npz")
    return {k: f[k] for k in f.files}


def _L():
    from connect4_amd import _lib as L
    return L


@pytest.mark.parametrize("empties", RC.EMPTIES)
def test_host_review_equals_the_oracle(z, empties):
    from connect4_amd.review import review_host
    for n_games in (1, 3, 65):
        games = RC.games_of(z, n_games)
        r = review_host(games, max_empties=empties)
        RC.assert_review_equals(r, RC.expected(z, empties, n_games))
        RC.assert_identities(r)
        assert r.report["contradictions"] == 0 and r.report["unknown"] == 0 and r.report["late"] == int(r.by_ply[:, 0].sum())
        assert r.report["positions"] == RC.positions_of(z, n_games) and (r.report["nodes"], r.report["distinct"]) == _distinct_nodes(games, r)


def _distinct_nodes(games, r):
    """The nodes of the distinct late positions, each counted once."""
    late = (r.status != _L().SOLVE_TOO_DEEP).numpy()
    _, first = np.unique(games.boards.numpy()[late], axis=0, return_index=True)
    return int(r.nodes.numpy()[late][first].sum()), len(first)


def test_whole_file_at_twelve(z):
    """All 257 games at the default cut-off; the games of kind (c) -- every late move chosen by the oracle to keep the outcome
    -- show no blunder in their tails."""
    from connect4_amd.review import DEFAULT_MAX_EMPTIES, review_games
    r = review_games(RC.games_of(z, 257), max_empties=12, host=True)
    assert r.max_empties == 12 and review_games(RC.games_of(z, 1), host=True, node_budget=64).max_empties == DEFAULT_MAX_EMPTIES
    RC.assert_review_equals(r, RC.expected(z, 12, 257))
    assert int(r.per_game[:, 2][z["kinds"] == 2].sum()) == 0 and int(r.per_game[:, 2].sum()) > 0
    assert sorted(set(z["results"].tolist())) == [0, 1, 2] and (z["lengths"] == 42).any() and (r.per_game[:, 0] == 0).any()


def test_no_row_and_every_row(z):
    from connect4_amd.review import review_host
    L = _L()
    games = RC.games_of(z, 65)
    none = review_host(games, max_empties=0)
    assert (none.status == L.SOLVE_TOO_DEEP).all() and (none.kept == -1).all() and not none.by_ply.any() and none.report["distinct"] == 0
    assert (none.per_game.numpy() == [0, 0, 0, -1]).all() and none.exact_targets.equal(games.targets)
    every = review_host(games, max_empties=42, node_budget=64)
    status = every.status.numpy()
    assert set(status.tolist()) == {L.SOLVE_SOLVED, L.SOLVE_UNKNOWN} and int(every.by_ply[:, 0].sum()) == games.n_positions
    RC.assert_identities(every)
    known = every.outcome.numpy() >= 0
    same_game = np.zeros(len(known), dtype=bool)
    same_game[:-1] = games.game_index.numpy()[1:] == games.game_index.numpy()[:-1]
    nxt_known = np.where(same_game, np.roll(known, -1), True)
    assert ((every.kept.numpy() >= 0) == (known & nxt_known)).all()
    assert (every.nodes.numpy()[status == L.SOLVE_UNKNOWN] == 64).all()


def test_tight_budget_statuses(z):
    from connect4_amd.review import review_host
    e, budget, n_games = (int(v) for v in z["tight"])
    r = review_host(RC.games_of(z, n_games), max_empties=e, node_budget=budget)
    assert r.status.numpy().tobytes() == z["status_e20_b64"].tobytes()
    assert r.report["unknown"] == int((z["status_e20_b64"] == _L().SOLVE_UNKNOWN).sum()) > 0
    RC.assert_identities(r)


def _broken(z, n_games, fn):
    games = RC.games_of(z, n_games)
    fields = {k: getattr(games, k).clone() for k in ("boards", "moves", "values", "policy", "targets", "game_index", "lengths", "results", "ids")}
    fn(fields)
    from connect4_amd.packed import PackedGames
    return PackedGames(**fields)


def broken_batches(z):
    """(name, games, the first row that breaks the chain): a corrupted move, two swapped rows, a wrong result."""
    start = np.concatenate([[0], np.cumsum(z["lengths"])])
    row = int(start[1]) + 3       # game 1, ply 3

    def move(f):
        f["moves"][row] = (int(f["moves"][row]) + 1) % 7

    def swap(f):
        f["boards"][[row, row + 1]] = f["boards"][[row + 1, row]]

    def result(f):
        f["results"][2] = (int(f["results"][2]) + 1) % 3

    return [("move", _broken(z, 3, move), row), ("swap", _broken(z, 3, swap), row - 1), ("result", _broken(z, 3, result), int(start[3]) - 1)]


def test_broken_chains_are_refused(z):
    from connect4_amd.review import review_host
    for name, games, row in broken_batches(z):
        with pytest.raises(ValueError, match=r"row %d breaks" % row):
            review_host(games, max_empties=8)


def test_game_without_result(z):
    from connect4_amd.review import review_host
    def no_result(f):
        f["results"][0] = -1
    games = _broken(z, 3, no_result)
    r, ref = review_host(games, max_empties=12), review_host(RC.games_of(z, 3), max_empties=12)
    last = int(z["lengths"][0]) - 1
    differs = np.nonzero(r.kept.numpy() != ref.kept.numpy())[0]
    assert differs.tolist() == [last] and int(r.kept[last]) == -1 and int(ref.kept[last]) >= 0
    assert not r.target_agrees[:last + 1].any() and r.outcome.equal(ref.outcome)


def test_duplicated_games_are_searched_once(z):
    from connect4_amd.packed import PackedGames
    from connect4_amd.review import review_host
    one = RC.games_of(z, 3)
    two = PackedGames.cat([one, RC.games_of(z, 3)])
    a, b = review_host(one, max_empties=12), review_host(two, max_empties=12)
    n = one.n_positions
    for k in ("status", "outcome", "kept", "target_agrees", "nodes"):
        assert getattr(b, k)[:n].equal(getattr(a, k)) and getattr(b, k)[n:].equal(getattr(a, k)), k
    assert b.per_game[:3].equal(a.per_game) and b.per_game[3:].equal(a.per_game) and b.by_ply.equal(2 * a.by_ply)
    assert b.report["distinct"] == a.report["distinct"] and b.report["nodes"] == a.report["nodes"] and b.report["late"] == 2 * a.report["late"]
    assert b.distinct_boards.equal(a.distinct_boards)


def test_exact_targets_change_the_solved_late_rows_only(z):
    from connect4_amd.packed import PackedGames
    from connect4_amd.review import review_host
    L = _L()
    games = RC.games_of(z, 65)
    r = review_host(games, max_empties=20, node_budget=64)
    new = games.with_exact_targets(r)
    solved = (r.status == L.SOLVE_SOLVED).numpy()
    want = np.where(solved, z["outcome_e16"][:games.n_positions].astype(np.float32) * np.float32(0.5), games.targets.numpy())
    deep = solved & (z["outcome_e16"][:games.n_positions] < 0)      # 17..20 empty squares: no oracle label in the file
    assert new.targets.numpy()[~deep].tobytes() == want[~deep].tobytes()
    assert (new.targets.numpy()[~solved] == games.targets.numpy()[~solved]).all() and (new.targets != games.targets).any()
    assert (new.targets.numpy()[solved] == r.outcome.numpy()[solved] * np.float32(0.5)).all()
    for k in ("boards", "moves", "values", "policy", "game_index", "lengths", "results", "ids"):
        assert getattr(new, k) is getattr(games, k), k
    with pytest.raises(ValueError, match="keep mask"):
        games.with_exact_targets(r, priors=True)
    # the object form keeps the games' own results
    small = RC.games_of(z, 3)
    back = PackedGames.from_game_data(small.with_exact_targets(review_host(small, max_empties=12)).to_game_data())
    assert back.results.equal(small.results) and back.boards.equal(small.boards) and back.moves.equal(small.moves)


@pytest.mark.parametrize("empties", [8, 16])
def test_keep_masks_equal_the_oracle(z, empties):
    from connect4_amd.review import review_host
    games = RC.games_of(z, 65)
    plain, r = review_host(games, max_empties=empties), review_host(games, max_empties=empties, moves=True)
    want, late = RC.expected_keep(z, empties, 65)
    assert r.keep.numpy().tobytes() == want.tobytes() and r.keep_known.numpy().tobytes() == late.tobytes()
    assert want[late].any(axis=1).all()         # a solved position has a move that keeps its outcome
    for k in ("status", "outcome", "kept", "target_agrees", "nodes", "by_ply", "per_game", "exact_targets"):
        assert getattr(r, k).equal(getattr(plain, k)), k        # stage 1 is the search already made: nothing is searched twice
    assert r.report["nodes"] == plain.report["nodes"] and r.report["stage2_rows"] > 0 and r.report["stage2_unknown"] == 0
    policy = games.policy.numpy()
    share = RC.policy_on_kept(policy, want, late)
    assert r.policy_on_kept.numpy().tobytes() == share.tobytes()
    count = want.sum(axis=1)
    priors = np.where(late[:, None], want / np.maximum(count, 1)[:, None].astype(np.float32), policy).astype(np.float32)
    assert r.exact_priors.numpy().tobytes() == priors.tobytes()
    new = games.with_exact_targets(r, priors=True)
    assert new.policy.equal(r.exact_priors) and new.targets.equal(r.exact_targets) and new.moves is games.moves
    assert games.with_exact_targets(r).policy is games.policy
    s = r.summary()
    assert s["policy_on_kept_rows"] == int(late.sum()) and s["policy_on_kept"] == float(share[late].astype(np.float64).sum() / late.sum())
    ages = np.array([bin(int(a) | int(b)).count("1") for a, b in z["boards"][:len(late)]])
    for age, mean in enumerate(s["policy_on_kept_by_ply"]):
        pick = late & (ages == age)
        assert (mean is None) == (not pick.any()) and (mean is None or abs(mean - share[pick].astype(np.float64).mean()) < 1e-12)
    assert "policy_on_kept" not in plain.summary() and plain.keep is None


def test_keep_is_unknown_where_a_child_is(z):
    """Under a tight budget a stage-2 row stays unknown: the position's keep mask is unknown, its outcome is not."""
    from connect4_amd.review import review_host
    games = RC.games_of(z, 65)
    plain, r = review_host(games, max_empties=20, node_budget=64), review_host(games, max_empties=20, node_budget=64, moves=True)
    assert r.outcome.equal(plain.outcome) and r.status.equal(plain.status) and r.kept.equal(plain.kept)
    known, solved = r.keep_known.numpy(), (r.outcome >= 0).numpy()
    assert not known[~solved].any() and (solved & ~known).any() and r.report["stage2_unknown"] > 0
    assert not r.keep.numpy()[~known].any() and np.isnan(r.policy_on_kept.numpy()[~known]).all()
    assert r.exact_priors.numpy()[~known].tobytes() == games.policy.numpy()[~known].tobytes()


def test_summary_and_labelled_set(z):
    from connect4_amd.review import review_host
    r = review_host(RC.games_of(z, 65), max_empties=12)
    s = r.summary()
    t = z["by_ply_e12_g65"]
    assert s["games"] == 65 and s["late"] == int(t[:, 0].sum()) and s["blunders"] == int(t[:, 4].sum()) and s["contradictions"] == 0
    assert s["blunders_per_game"] == int(t[:, 4].sum()) / 65 and s["target_agreement"] == int(t[:, 5].sum()) / int(t[:, 0].sum())
    assert s["by_side"]["o"]["late"] == int(t[0::2, 0].sum()) and s["by_side"]["x"]["blunders"] == int(t[1::2, 4].sum())
    assert s["by_ply"] == t.tolist() and all(type(v) is int for row in s["by_ply"] for v in row)
    ls = r.labelled_set()
    assert len(ls) == r.report["distinct"] == r.report["solved"] and ls.priors is None
    assert set(ls.values.tolist()) <= {0.0, 0.5, 1.0}


def test_refusals(z):
    from connect4_amd.generation import run_generation, run_generations
    from connect4_amd.review import review_games
    games = RC.games_of(z, 3)
    for bad in (-1, 43, 1.5):
        with pytest.raises(ValueError, match="max_empties"):
            review_games(games, max_empties=bad, host=True)
    with pytest.raises(ValueError, match="host=True"):
        review_games(games)
    with pytest.raises(ValueError, match="review_empties"):
        run_generation(None, None, 1, exact_targets=True)
    with pytest.raises(ValueError, match="review_empties"):
        run_generations(None, None, 1, None, 1, exact_targets=True)
