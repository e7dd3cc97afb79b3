"""What the exact-leaf tests share (tests/test_exact_leaves_host.py, tests/test_gpu_exact_leaves*.py): the rows of
tests/golden/solver_exact.npz with a few rows that are no searchable position, the evaluator's value of an exact score, and
an evaluator for the oracle's replay whose late values come from the oracle's exhaustive search.

Nothing here is code of the search under test: lateness is the fixture's own count of empty squares (every fixture row is an
undecided position), the outcomes are ``oracle.c4oracle.Exact``'s scores."""
import numpy as np

from conftest import load_npz

SENTINEL = np.float32(0.25)         # no exact value (0, 0.5, 1) and no bit pattern the overlay writes


def value_of_score(score, age):
    """float32 1.0 / 0.5 / 0.0 from o's side of the mover's exact score (c4_oracle.h: 43 - final age for a win of the mover,
    final age - 43 for a loss, 0 for a draw); o moves at even ages."""
    s = np.sign(np.asarray(score, dtype=np.int64))
    s = np.where(np.asarray(age, dtype=np.int64) & 1, -s, s)
    return ((s + 1) * 0.5).astype(np.float32)


def ages(c0, c1):
    occ = np.asarray(c0, dtype=np.uint64) | np.asarray(c1, dtype=np.uint64)
    return np.array([bin(int(x)).count("1") for x in occ], dtype=np.int64)


def extra_rows():
    """(c0, c1) of rows no overlay may touch: the zero row (the empty board: 42 empty squares), two finished positions (o has
    four in column 3 after seven stones; a seeded random game that ended with at most ten empty squares), and three rows that
    are no position (overlapping stones, a floating stone, x having moved first)."""
    from connect4_amd.board import Board
    won = Board()
    for m in (3, 2, 3, 2, 3, 2, 3):
        won.make_move(m)
    assert won.result is not None
    rng = np.random.RandomState(5)
    while True:
        late_end = Board()
        while late_end.result is None:
            late_end.make_move(int(rng.choice(sorted(late_end.valid_moves))))
        if late_end.age >= 32:
            break
    rows = [(0, 0), tuple(int(x) for x in won.color), tuple(int(x) for x in late_end.color), (1, 1), (2, 0), (0, 1)]
    return np.array([r[0] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.uint64)


def fixture_rows(pick=None):
    """dict(c0, c1, empties, score, late_ok): the fixture's rows (those of `pick`) followed by extra_rows(); late_ok is False
    for the extras, whose empties / score are -1 / 0."""
    z = load_npz("solver_exact.npz")
    pick = slice(None) if pick is None else pick
    c0, c1, empties, score = z["c0"][pick], z["c1"][pick], z["empties"][pick].astype(np.int64), z["score"][pick].astype(np.int64)
    x0, x1 = extra_rows()
    k = len(x0)
    return dict(c0=np.concatenate([c0, x0]).astype(np.uint64), c1=np.concatenate([c1, x1]).astype(np.uint64),
                empties=np.concatenate([empties, np.full(k, -1)]), score=np.concatenate([score, np.zeros(k, dtype=np.int64)]),
                late_ok=np.concatenate([np.ones(len(c0), dtype=bool), np.zeros(k, dtype=bool)]))


class OracleOverlay:
    """``evaluate_bits`` for oracle.replay.replay_games_bulk: the net's answers with the exhaustive oracle's outcome laid over
    every undecided position with at most `max_empties` empty squares.  The replay only asks for undecided positions of
    games, so lateness is the count of empty squares; `laid_over` counts the positions answered exactly."""

    def __init__(self, oracle, net, max_empties, log2_entries=24):
        self.net, self.max_empties = net, max_empties
        self.memo = oracle.Exact(log2_entries)
        self.oracle = oracle
        self.laid_over = 0

    def evaluate_bits(self, c0, c1, wave=False):
        v, p = self.net.evaluate_bits(c0, c1, wave=wave)
        c0, c1 = np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
        age = ages(c0, c1)
        late = np.nonzero(42 - age <= self.max_empties)[0]
        if len(late):
            score, _, status = self.memo.scores(c0[late], c1[late])
            assert (status == self.oracle.EXACT_SEARCHED).all()
            v = v.copy()
            v[late] = value_of_score(score, age[late])
            self.laid_over += len(late)
        return v, p

    def close(self):
        self.memo.close()
