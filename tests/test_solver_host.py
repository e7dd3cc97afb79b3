"""The exact solver's host side (connect4_amd/solver.py), no GPU: solve_host and the host half of grid_triple against the
unmodified reference's exhaustive GridSearch(plies = empty squares) (tests/golden/solver.npz, written by
tests/golden/gen_solver_golden.py) and against nega_max_host; the labeller's prior rule; LabelledSet.save; the constants."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_npz


@pytest.fixture(scope="module")
def ref():
    return load_npz("solver.npz")


def boards_of(z):
    from connect4_amd.board import Board
    return [Board.from_bits(int(a), int(b)) for a, b in zip(z["c0"], z["c1"])]


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def test_fixture_covers_what_it_should(ref):
    empties = 42 - np.array([b.age for b in boards_of(ref)])
    assert sorted(set(empties.tolist())) == list(range(3, 11))
    assert min(np.bincount(empties)[3:]) >= 6
    deep = load_npz("solver_deep.npz")
    e = 42 - np.array([b.age for b in boards_of(deep)])
    assert len(e) == 256 and e.min() == 12 and e.max() == 20 and deep["nodes"].max() <= 1 << 17


def test_solve_host_is_the_reference_bit_for_bit(ref):
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_host
    for b, want in zip(boards_of(ref), ref["root_search"]):
        a = solve_host(b)
        assert a.status == L.SOLVE_SOLVED and a.nodes >= 1
        assert same_bits(a.value, want), (b.color, a, want)
        assert a.outcome == (1.0 if want > 0.9 else 0.0 if want < 0.1 else 0.5)


def test_grid_triple_host_is_the_reference_bit_for_bit(ref):
    from connect4_amd.solver import grid_triple
    boards = boards_of(ref)
    before = [tuple(b.color) for b in boards]
    out = grid_triple(boards, host=True)
    assert before == [tuple(b.color) for b in boards]
    for i, (move, value, tree) in enumerate(out):
        assert move == int(ref["move"][i]) and same_bits(value, ref["value"][i])
        assert same_bits(tree.root.data.search_value, ref["root_search"][i])
        names = [int(x) for x in ref["child_names"][i] if x >= 0]
        assert [c.name for c in tree.root.children] == names
        for c, want in zip(tree.root.children, ref["child_abs"][i]):
            assert same_bits(c.data.absolute_value, want)


def test_solve_host_is_nega_max_host_on_other_positions():
    from connect4_amd.evaluators import evaluate_centre
    from connect4_amd.grid_search import nega_max_host
    from connect4_amd.solver import grid_triple, random_playout, solve_host
    rng = np.random.RandomState(77)
    boards = [random_playout(rng, 42 - int(rng.randint(1, 8))) for _ in range(50)]
    triples = grid_triple(boards, host=True)
    for b, (move, value, tree) in zip(boards, triples):
        m, v, t = nega_max_host(b, 42 - b.age, evaluate_centre)
        assert same_bits(solve_host(b).value, t.root.data.search_value)
        assert (move, value) == (m, v)
        assert [c.data.absolute_value for c in tree.root.children] == [c.data.absolute_value for c in t.root.children]
        assert [c.data.position_value for c in tree.root.children] == [c.data.position_value for c in t.root.children]


def test_statuses_and_budget_on_the_host():
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    from connect4_amd.solver import random_playout, solve_host, value_from_answer
    rng = np.random.RandomState(5)
    b = random_playout(rng, 17)
    assert solve_host(b).status == L.SOLVE_TOO_DEEP
    assert solve_host(random_playout(rng, 18), node_budget=256).status in (L.SOLVE_SOLVED, L.SOLVE_UNKNOWN)
    won = Board()
    for m in (0, 1, 0, 1, 0, 1, 0):
        won.make_move(m)
    a = solve_host(won)
    assert (a.status, a.outcome, a.final_age, a.nodes) == (L.SOLVE_TERMINAL, 1.0, 7, 0) and a.value == 1.0 - 7 / 10000.0
    c0, c1 = b.color
    floating = c0 | 1 << (b.height[0] + 1)
    for bad in ((c0, c1 | (c0 & -c0)), (floating, c1), (c0 | 1 << b.height[0] | 1 << b.height[1], c1), (c0, c1 | 1 << b.height[2] | 1 << b.height[3]),
                (0b1111, 0b1111 << 7), (c0 | 1 << 6, c1)):
        assert solve_host(bad).status == L.SOLVE_INVALID, bad
    assert float(value_from_answer(0.5, 42)) == 0.5 + 42 / 10000.0 and float(value_from_answer(0.0, 30)) == 30 / 10000.0
    # the budget never lies
    deep = load_npz("solver_deep.npz")
    seen = set()
    for i in np.argsort(deep["nodes"])[::16]:
        a = solve_host((int(deep["c0"][i]), int(deep["c1"][i])), node_budget=64)
        seen.add(a.status)
        if a.status == L.SOLVE_UNKNOWN:
            assert a.nodes == 64 and deep["nodes"][i] > 64 and a.value is None
        else:
            assert (a.status, a.outcome, a.final_age, a.nodes) == (L.SOLVE_SOLVED, deep["outcome"][i], deep["final_age"][i], deep["nodes"][i])
            assert same_bits(a.value, deep["value"][i])
    assert seen == {L.SOLVE_SOLVED, L.SOLVE_UNKNOWN}


def test_prior_rule():
    """generate_7ply.py:83-91: 1.0 for every legal move whose child has the position's value, normalised; zeros if none."""
    from connect4_amd.solver import prior_from_children
    outcome = np.array([2, 2, 0, 1, 2])
    kids = np.array([[0, 0, 2, 0, 1, 0, 0],        # one winning move for o
                     [2, 0, 2, 1, 2, 2, 0],        # several; column 5 wins too but is full
                     [2, 2, 2, 0, 0, 2, 2],        # x to move: two moves keep the x win
                     [2, 1, 1, 1, 1, 1, 1],        # no winning move (x to move, drawn): every drawing move
                     [0, 0, 1, 1, 0, 0, 0]])       # no move has the position's value
    legal = np.array([[1] * 7, [1, 1, 1, 1, 1, 0, 1], [1] * 7, [1, 1, 0, 1, 1, 1, 1], [1] * 7])
    want = np.zeros((5, 7))
    want[0, 2] = 1.0
    want[1, [0, 2, 4]] = 1.0 / 3.0
    want[2, [3, 4]] = 0.5
    want[3, [1, 3, 4, 5, 6]] = 0.2
    p = prior_from_children(outcome, kids, legal)
    assert p.dtype == np.float64 and np.array_equal(p, want)
    import torch
    t = prior_from_children(torch.from_numpy(outcome), torch.from_numpy(kids), torch.from_numpy(legal))
    assert np.array_equal(t.numpy(), want)


def test_prior_rule_on_solved_positions():
    """The rule fed with solve_host's outcomes equals the rule fed with the exhaustive search's children."""
    from connect4_amd.evaluators import evaluate_centre
    from connect4_amd.grid_search import nega_max_host
    from connect4_amd.solver import prior_from_children, random_playout, solve_host
    rng = np.random.RandomState(9)
    for _ in range(30):
        b = random_playout(rng, 42 - int(rng.randint(2, 8)))
        _, _, tree = nega_max_host(b, 42 - b.age, evaluate_centre)
        root = round(tree.root.data.search_value * 2) / 2
        want = np.zeros(7)
        for c in tree.root.children:
            v = c.data.board.result.value if c.data.board.result is not None else round(c.data.search_value * 2) / 2
            want[c.name] = 1.0 if v == root else 0.0
        want /= want.sum()
        kids, legal = np.full((1, 7), -1.0), np.zeros((1, 7))
        for c in tree.root.children:
            kids[0, c.name] = solve_host(c.data.board).outcome
            legal[0, c.name] = 1
        got = prior_from_children(np.array([solve_host(b).outcome]), kids, legal)[0]
        assert np.array_equal(got, want) and got.sum() == pytest.approx(1.0)


def labelled_rows():
    import torch
    from connect4_amd.solver import random_playout
    rng = np.random.RandomState(3)
    boards = [random_playout(rng, int(rng.randint(0, 40))) for _ in range(40)]
    bits = np.array([b.color for b in boards], dtype=np.uint64).view(np.int64)
    values = torch.from_numpy(rng.choice([0.0, 0.5, 1.0], size=40).astype(np.float32))
    priors = torch.from_numpy(rng.dirichlet(np.ones(7), size=40).astype(np.float32))
    return boards, torch.from_numpy(bits), values, priors


def test_labelled_set_save_writes_the_reference_file(tmp_path):
    """data.py:22-33: a dict of float32 boards [n, 3, 6, 7], values [n], priors [n, 7]."""
    import torch
    from connect4_amd.stats import LabelledSet
    boards, bits, values, priors = labelled_rows()
    path = os.path.join(str(tmp_path), "set.pth")
    LabelledSet(bits, values, priors).save(path)
    d = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(d) == ["boards", "priors", "values"]
    assert d["boards"].dtype == torch.float32 and tuple(d["boards"].shape) == (40, 3, 6, 7)
    assert np.array_equal(d["boards"].numpy(), np.stack([b.to_array() for b in boards]).astype(np.float32))
    assert torch.equal(d["values"], values) and torch.equal(d["priors"], priors)
    LabelledSet(bits, values).save(path)
    assert torch.load(path, map_location="cpu", weights_only=True)["priors"] is None


def test_labelled_set_save_then_load_round_trips(tmp_path):
    import torch
    from connect4_amd.stats import LabelledSet
    if not torch.cuda.is_available():
        pytest.skip("LabelledSet.load turns the planes back into boards on the GPU")
    _, bits, values, priors = labelled_rows()
    path = os.path.join(str(tmp_path), "set.pth")
    for src in (LabelledSet(bits, values, priors), LabelledSet(bits.cuda(), values, priors)):
        src.save(path)
        ls = LabelledSet.load(path, device="cuda")
        assert torch.equal(ls.boards.cpu(), bits) and torch.equal(ls.values.cpu(), values) and torch.equal(ls.priors.cpu(), priors)


def test_constants_agree():
    from connect4_amd import _lib as L
    from connect4_amd import solver
    text = open(os.path.join(ROOT, "include", "c4_engine.h")).read()
    header = {k: int(v) for k, v in re.findall(r"#define C4_SOLVE_([A-Z_]+) (\d+)", text)}
    assert header == {"MAX_EMPTIES": 24, "SOLVED": L.SOLVE_SOLVED, "TERMINAL": L.SOLVE_TERMINAL, "UNKNOWN": L.SOLVE_UNKNOWN,
                      "TOO_DEEP": L.SOLVE_TOO_DEEP, "INVALID": L.SOLVE_INVALID}
    assert L.SOLVE_MAX_EMPTIES == solver.MAX_EMPTIES == 24 and solver.DEFAULT_NODE_BUDGET >= 1 << 26
    assert sorted(solver.STATUS_NAMES) == [0, 1, 2, 3, 4] and len(set(solver.STATUS_NAMES.values())) == 5
    src = open(os.path.join(ROOT, "connect4_amd", "csrc", "c4_solve.hip")).read()
    assert re.search(r"DEFAULT_BUDGET = \(int64_t\)1 << (\d+)", src).group(1) == "26"
    for name in ("c4_solve", "c4_solve_dev", "c4_solve_children_dev", "c4_solve_last_error"):
        assert name in L.SIGNATURES
