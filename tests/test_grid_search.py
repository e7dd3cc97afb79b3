"""GridSearch on the host: the plain-Python mirror (connect4_amd.grid_search.nega_max_host) against what the
reference's own GridSearch returned (tests/golden/grid_search.json, written by gen_grid_golden.py), and the
argument checks of the device player, which fail before any device call."""
import copy
import pickle

import numpy as np
import pytest

from conftest import load_json

from connect4_amd.board import Board
from connect4_amd.evaluators import Evaluator, evaluate_centre, evaluate_centre_with_prior
from connect4_amd.grid_search import GridSearch, nega_max_host


def return_half(board):
    return 0.5


EVALS = {"centre": evaluate_centre, "half": return_half}


def bits(x):
    return None if x is None else float(x).hex()


def case_board(c):
    return Board.from_bits(c["c0"], c["c1"])


def result_of(move, value, tree):
    child = [None] * 7
    for c in tree.root.children:
        child[c.name] = tree.get_node_value(c)
    return dict(move=move, value=bits(value), child_values=[bits(v) for v in child],
                root_value=bits(tree.root.data.search_value))


def expected(c):
    return dict(move=c["move"], value=bits(c["value"]), child_values=[bits(v) for v in c["child_values"]],
                root_value=bits(c["root_value"]))


CASES = load_json("grid_search.json")["cases"]


def test_fixture_covers_the_issue():
    kinds = {}
    for c in CASES:
        kinds[c["kind"]] = kinds.get(c["kind"], 0) + 1
    assert kinds["player"] == 7 and kinds["random"] >= 200 and kinds["random5"] >= 16 and kinds["deep"] >= 20
    assert kinds["half"] >= 8
    assert max(c["plies"] for c in CASES if c["kind"] == "deep") >= 15


@pytest.mark.parametrize("i", range(len(CASES)))
def test_host_matches_reference(i):
    c = CASES[i]
    b = case_board(c)
    before = b.to_int_tuple()
    got = result_of(*nega_max_host(b, c["plies"], Evaluator(EVALS[c["eval"]])))
    assert got == expected(c)
    assert b.to_int_tuple() == before


def test_player_positions_play_an_accepted_move():
    for p in load_json("ref_tests.json")["player"]:
        b = Board.from_pieces(np.array(p["o"], dtype=bool), np.array(p["x"], dtype=bool))
        move, _, _ = nega_max_host(b, p["plies"], Evaluator(evaluate_centre))
        assert move in p["ans"]


def test_empty_board_tie_goes_to_the_higher_column():
    move, value, tree = nega_max_host(Board(), 2, Evaluator(evaluate_centre))
    vals = {c.name: tree.get_node_value(c) for c in tree.root.children}
    assert vals[2] == vals[3] == vals[4] == max(vals.values())
    assert move == 4 and value == vals[4]
    p = tree.get_values_policy()
    assert abs(p.sum() - 1.0) < 1e-12 and np.argmax(p) == 2


def test_bad_plies_and_finished_board_raise():
    b = Board()
    with pytest.raises(ValueError):
        nega_max_host(b, 0, Evaluator(evaluate_centre))
    with pytest.raises(ValueError):
        GridSearch("g", 0, Evaluator(evaluate_centre)).make_move(b)
    done = Board()
    for m in (0, 1, 0, 1, 0, 1, 0):
        done.make_move(m)
    assert done.result is not None
    with pytest.raises(ValueError):
        nega_max_host(done, 2, Evaluator(evaluate_centre))
    with pytest.raises(ValueError):
        GridSearch("g", 2, Evaluator(evaluate_centre)).make_moves([Board(), done])
    assert b.to_int_tuple() == (0, 0)


def test_tuple_valued_evaluator_raises_type_error():
    for plies in (1, 2):
        with pytest.raises(TypeError):
            nega_max_host(Board(), plies, Evaluator(evaluate_centre_with_prior))


def test_player_copies_and_pickles():
    g = GridSearch("g", 3, Evaluator(evaluate_centre), device=0)
    for h in (copy.copy(g), pickle.loads(pickle.dumps(g))):
        assert (h.name, h.plies, h.device) == ("g", 3, 0)
    assert "Computer" in str(g)
