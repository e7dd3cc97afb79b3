"""GridSearch on the MI355X (connect4_amd/csrc/c4_grid.hip): the reference's answers
(tests/golden/grid_search.json) bit for bit, batches of every shape against the host mirror, edge positions,
caller evaluators through the frontier / finish round trip, and lock-step Match play."""
import copy

import numpy as np
import pytest

from conftest import load_json

from connect4_amd.board import Board
from connect4_amd.config import MCTSConfig
from connect4_amd.evaluators import Evaluator, evaluate_centre, evaluate_centre_with_prior
from connect4_amd.grid_search import GridSearch, grid_search, nega_max_host
from connect4_amd.match import Match
from connect4_amd.mcts import MCTS
from connect4_amd.player import BasePlayer

pytestmark = pytest.mark.gpu

CASES = load_json("grid_search.json")["cases"]


def return_half(board):
    return 0.5


EVALS = {"centre": evaluate_centre, "half": return_half}


def bits(x):
    return None if x is None else float(x).hex()


def summary(move, value, tree):
    child = [None] * 7
    for c in tree.root.children:
        child[c.name] = tree.get_node_value(c)
    return (move, bits(value), tuple(bits(v) for v in child), bits(tree.root.data.search_value))


def expected(c):
    return (c["move"], bits(c["value"]), tuple(bits(v) for v in c["child_values"]), bits(c["root_value"]))


def random_positions(rng, n, lo=0, hi=30):
    out = []
    while len(out) < n:
        b = Board()
        for _ in range(int(rng.randint(lo, hi + 1))):
            b.make_move(int(rng.choice(sorted(b.valid_moves))))
            if b.result is not None:
                break
        if b.result is None:
            out.append(b)
    return out


def test_fixture_make_move():
    for c in CASES:
        b = Board.from_bits(c["c0"], c["c1"])
        got = GridSearch("g", c["plies"], Evaluator(EVALS[c["eval"]])).make_move(b)
        assert summary(*got) == expected(c), c
        after = Board.from_bits(c["c0"], c["c1"])
        after.make_move(c["move"])
        assert b == after and b.age == after.age and b.result == after.result
        if c["kind"] == "player":
            assert got[0] in c["ans"]


def test_fixture_make_moves_batches():
    groups = {}
    for c in CASES:
        groups.setdefault((c["plies"], c["eval"]), []).append(c)
    for (plies, ev), cs in groups.items():
        boards = [Board.from_bits(c["c0"], c["c1"]) for c in cs]
        res = GridSearch("g", plies, Evaluator(EVALS[ev])).make_moves(boards)
        assert [summary(*r) for r in res] == [expected(c) for c in cs], (plies, ev)


@pytest.mark.parametrize("plies", [1, 2, 3, 4, 5, 6])
def test_batch_shapes_against_host(plies):
    rng = np.random.RandomState(100 + plies)
    pool = random_positions(rng, 4099)
    results = {}
    for n in (1, 7, 64, 4099):
        res = grid_search(pool[:n], plies, Evaluator(evaluate_centre))
        results[n] = [summary(*r) for r in res]
    for n in (1, 7, 64):                    # every batch size splits the work differently: same answers
        assert results[n] == results[4099][:n]
    if plies <= 4:
        check = range(64) if plies >= 3 else range(4099)
        for i in check:
            assert summary(*nega_max_host(pool[i], plies, Evaluator(evaluate_centre))) == results[4099][i], i


def test_edge_positions():
    boards = []
    b = Board()                       # o to move can win now in column 3, x threatens too
    for m in (3, 0, 3, 0, 3, 0):
        b.make_move(m)
    boards.append(b)
    b = Board()                       # x to move must block / can win
    for m in (1, 0, 1, 0, 1, 0, 6):
        b.make_move(m)
    boards.append(b)
    rng = np.random.RandomState(7)
    full = []                         # one empty cell left: the only child is a win or a draw
    while len(full) < 6:
        x = random_positions(rng, 1, 41, 41)[0]
        if x.age == 41:
            full.append(x)
    boards += full
    boards += random_positions(rng, 20, 34, 40)        # near the end of the game ...
    boards += random_positions(rng, 20, 0, 6)          # ... and near the start, in one call
    for plies in (1, 2, 3):
        res = grid_search(boards, plies, Evaluator(evaluate_centre))
        for b, r in zip(boards, res):
            assert summary(*r) == summary(*nega_max_host(b, plies, Evaluator(evaluate_centre)))
    assert grid_search(boards[:1], 1, Evaluator(evaluate_centre))[0][0] == 3
    assert grid_search(boards[1:2], 2, Evaluator(evaluate_centre))[0][0] == 0


def test_external_evaluator_counts_and_values():
    calls = []

    def counting(board):
        calls.append(board.to_int_tuple())
        return evaluate_centre(board) * 0.75 + 0.125

    rng = np.random.RandomState(3)
    boards = random_positions(rng, 40, 0, 30)
    for plies in (1, 2, 3):
        calls.clear()
        ev = Evaluator(counting)
        res = grid_search(boards, plies, ev)
        assert len(calls) == len(set(calls))              # each distinct frontier position once
        host_ev = Evaluator(counting)
        host = []
        for b in boards:
            host.append(summary(*nega_max_host(b, plies, host_ev)))
        assert [summary(*r) for r in res] == host
        assert list(ev.position_table) == list(host_ev.position_table)   # same positions, same order
        n_first = len(ev.position_table)
        calls.clear()
        again = grid_search(boards, plies, ev)                 # repeat: every leaf is in the table
        assert calls == [] and len(ev.position_table) == n_first
        assert [summary(*r) for r in again] == host


def test_external_evaluator_distinct_count_with_empty_table():
    calls = []

    def counting(board):
        calls.append(board.to_int_tuple())
        return 0.5

    b = Board()
    GridSearch("g", 3, Evaluator(counting)).make_move(b)
    frontier = set()

    def walk(x, p):
        if x.result is not None:
            return
        if p == 0:
            frontier.add(x.to_int_tuple())
            return
        for m in sorted(x.valid_moves):
            y = x.__copy__()
            y.make_move(m)
            walk(y, p - 1)
    walk(Board(), 3)
    assert len(calls) == len(frontier) and set(calls) == frontier


def test_tuple_valued_evaluator_raises_type_error():
    with pytest.raises(TypeError):
        GridSearch("g", 2, Evaluator(evaluate_centre_with_prior)).make_move(Board())


class HostGrid(BasePlayer):
    def __init__(self, name, plies, evaluator):
        super().__init__(name)
        self.plies = plies
        self.evaluator = evaluator

    def make_move(self, board):
        move, value, tree = nega_max_host(board, self.plies, self.evaluator)
        board.make_move(move)
        return move, value, tree


def test_match_against_mcts_equals_host_mirror():
    cfg = MCTSConfig(simulations=40)
    np.random.seed(11)
    dev = Match(False, GridSearch("g", 2, Evaluator(evaluate_centre)),
                MCTS("m", cfg, Evaluator(evaluate_centre_with_prior)), plies=1, switch=True)
    r_dev = dev.play()
    np.random.seed(11)
    host = Match(False, HostGrid("g", 2, Evaluator(evaluate_centre)),
                 MCTS("m", cfg, Evaluator(evaluate_centre_with_prior)), plies=1, switch=True)
    r_host = host.play()
    assert r_dev == r_host
    assert [g[0].to_int_tuple() for g in dev.games] == [g[0].to_int_tuple() for g in host.games]
    assert copy.copy(dev._player_1).plies == 2
