"""GridSearch on the MI355X: every way c4_grid.hip can split a search gives the same answers.

The depth-first tail of 5 and 6 plies (k_grid_dfs<5>, <6>) is reached by deep batches and, through the
C4_GRID_FILL_NODES test aid, by the reference's own deep answers (tests/golden/grid_search.json).  A tiny
C4_GRID_LEVEL_CAP runs the halving of oversized levels and the chunking of the roots, for the in-kernel
evaluator and for the frontier / finish round trip; c4_grid_finish refuses a wrong number of leaf values."""
import numpy as np
import pytest

from conftest import load_json

from connect4_amd import _lib as L
from connect4_amd.board import Board, boards_to_bits
from connect4_amd.evaluators import Evaluator, evaluate_centre
from connect4_amd.grid_search import grid_search, nega_max_host

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


def random_positions(rng, n, lo, hi):
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


def fixture_by_group():
    groups = {}
    for c in CASES:
        groups.setdefault((c["plies"], c["eval"]), []).append(c)
    return groups


@pytest.mark.parametrize("fill", ["1", "50"])
def test_fixture_through_the_deep_depth_first_tail(monkeypatch, fill):
    # fill=1: the first level with at most 6 plies left goes depth-first, so the near-full cases searched
    # 9-20 plies deep run k_grid_dfs<6> (and <5>, <4> ... for the shallower ones) against the reference
    monkeypatch.setenv("C4_GRID_FILL_NODES", fill)
    for (plies, ev), cs in fixture_by_group().items():
        boards = [Board.from_bits(c["c0"], c["c1"]) for c in cs]
        got = [summary(*r) for r in grid_search(boards, plies, Evaluator(EVALS[ev]))]
        assert got == [expected(c) for c in cs], (plies, ev)


@pytest.mark.parametrize("plies", [7, 8])
def test_deep_batches_equal_single_root_searches(plies):
    # 4099 roots: the second level (~2e5 nodes) goes depth-first with plies-2 = 5 or 6 plies left; a single
    # root expands level by level instead
    rng = np.random.RandomState(700 + plies)
    pool = random_positions(rng, 4099, 6, 30)
    batch = [summary(*r) for r in grid_search(pool, plies, Evaluator(evaluate_centre))]
    for i in range(0, 4099, 683):
        assert summary(*grid_search([pool[i]], plies, Evaluator(evaluate_centre))[0]) == batch[i], i


def test_forced_depth_first_tail_equals_host_mirror(monkeypatch):
    monkeypatch.setenv("C4_GRID_FILL_NODES", "1")
    rng = np.random.RandomState(5)
    boards = random_positions(rng, 24, 26, 34)
    for plies in (6, 7):
        got = grid_search(boards, plies, Evaluator(evaluate_centre))
        for b, r in zip(boards, got):
            assert summary(*r) == summary(*nega_max_host(b, plies, Evaluator(evaluate_centre)))


@pytest.mark.parametrize("cap", ["7", "64"])
def test_level_cap_halving_and_root_chunks(monkeypatch, cap):
    rng = np.random.RandomState(11)
    boards = random_positions(rng, 40, 0, 30)
    ref = {p: [summary(*r) for r in grid_search(boards, p, Evaluator(evaluate_centre))] for p in (1, 3, 4)}
    monkeypatch.setenv("C4_GRID_LEVEL_CAP", cap)
    for p in (1, 3, 4):
        assert [summary(*r) for r in grid_search(boards, p, Evaluator(evaluate_centre))] == ref[p], p


@pytest.mark.parametrize("cap", ["7", "64"])
def test_level_cap_with_external_evaluator(monkeypatch, cap):
    monkeypatch.setenv("C4_GRID_LEVEL_CAP", cap)

    def shifted(board):
        return evaluate_centre(board) * 0.5 + 0.25

    rng = np.random.RandomState(12)
    boards = random_positions(rng, 30, 0, 30)
    for plies in (1, 2, 3):
        ev, host_ev = Evaluator(shifted), Evaluator(shifted)
        got = [summary(*r) for r in grid_search(boards, plies, ev)]
        host = [summary(*nega_max_host(b, plies, host_ev)) for b in boards]
        assert got == host
        assert list(ev.position_table) == list(host_ev.position_table)


def test_finish_refuses_a_wrong_leaf_count():
    lib = L.load()
    boards = [Board(), Board()]
    c0, c1 = boards_to_bits(boards)
    got = np.zeros(1, dtype=np.int64)
    rc = lib.c4_grid_frontier(0, c0.ctypes.data_as(L._u64p), c1.ctypes.data_as(L._u64p), 2, 2, None, None, 0,
                              got.ctypes.data_as(L._i64p))
    assert rc == L.ECAPACITY and got[0] == 98
    child = np.zeros((2, 7))
    root = np.zeros(2)
    move = np.zeros(2, dtype=np.int32)
    for k in (97, 99):
        vals = np.full(k, 0.5)
        rc = lib.c4_grid_finish(0, c0.ctypes.data_as(L._u64p), c1.ctypes.data_as(L._u64p), 2, 2,
                                vals.ctypes.data_as(L._f64p), k, child.ctypes.data_as(L._f64p),
                                root.ctypes.data_as(L._f64p), move.ctypes.data_as(L._i32p))
        assert rc == L.EINVAL, k
        assert b"leaf values" in lib.c4_grid_last_error()
    vals = np.full(98, 0.5)
    rc = lib.c4_grid_finish(0, c0.ctypes.data_as(L._u64p), c1.ctypes.data_as(L._u64p), 2, 2,
                            vals.ctypes.data_as(L._f64p), 98, child.ctypes.data_as(L._f64p),
                            root.ctypes.data_as(L._f64p), move.ctypes.data_as(L._i32p))
    assert rc == L.OK and list(move) == [6, 6]
