"""What the exact-oracle tests share (tests/test_exact_oracle.py, tests/test_gpu_solver_exact.py) with the generator of
tests/golden/solver_exact.npz: the strata of the fixture, the oracle's scores turned into the solver's answers, the labels
that follow from the children's scores, and the windows of the windowed checks.

Nothing here is code of the search under test.  The strata are decided by trying stones with a four-in-a-row test written
out below -- not with solver._winning_squares, solver._Search or tests/solver_audit.py."""
import numpy as np

WIDTH, HEIGHT, H1, SIZE = 7, 6, 7, 42
BOTTOM = sum(1 << (H1 * c) for c in range(WIDTH))
NO_MOVE = -128                      # child_score of a full column (oracle/c4_oracle.h C4O_EXACT_NO_MOVE)
ROWS_PER_EMPTIES = {**{e: 512 for e in range(1, 13)}, **{e: 256 for e in range(13, 17)}, 17: 96, 18: 96, 19: 32, 20: 32, 21: 16, 22: 16}
STRATA = ("one_threat", "two_threats", "block_under", "all_under", "one_nonlosing", "some_under", "late", "quiet_win",
          "quiet_loss", "quiet_draw")
STRATUM_MIN = 64
_u = np.uint64


def four(p):
    """bool [m]: the stones `p` (uint64 [m]) hold four in a row."""
    out = np.zeros(p.shape, dtype=bool)
    for s in (1, HEIGHT, H1, H1 + 1):
        y = p & (p >> _u(s))
        out |= (y & (y >> _u(2 * s))) != 0
    return out


def ages(c0, c1):
    occ = np.asarray(c0, dtype=np.uint64) | np.asarray(c1, dtype=np.uint64)
    return np.array([bin(int(x)).count("1") for x in occ], dtype=np.int64)


def root_facts(c0, c1):
    """Per row and column, by putting a stone there and testing for four in a row: legal (the column has room), wins (the
    mover wins by playing it), threat (the opponent would win on the square the move takes), under (the opponent wins on the
    square above it, the one the move makes playable).  bool [n, 7] each."""
    c0, c1 = np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    odd = (ages(c0, c1) & 1) == 1
    mine, theirs = np.where(odd, c1, c0), np.where(odd, c0, c1)
    occ = c0 | c1
    legal, wins, threat, under = (np.zeros((len(c0), WIDTH), dtype=bool) for _ in range(4))
    for c in range(WIDTH):
        col = _u(((1 << HEIGHT) - 1) << (H1 * c))
        low = (occ + _u(BOTTOM)) & col
        above = (low << _u(1)) & col
        legal[:, c] = low != 0
        wins[:, c] = legal[:, c] & four(mine | low)
        threat[:, c] = legal[:, c] & four(theirs | low)
        under[:, c] = (above != 0) & four(theirs | above)
    return legal, wins, threat, under


def strata(c0, c1, score):
    """{name: bool [n]} of STRATA.  Every stratum but `late` is of rows whose mover cannot win at once (`tree`, also in the
    dict), the positions enter_node reasons about:

    one_threat     the opponent threatens on exactly one playable square: the forced block
    two_threats    on two or more
    block_under    one threat, and the opponent also wins on the square above the block
    all_under      no threat, and every legal move lies under a square the opponent wins on
    one_nonlosing  no threat, and exactly one legal move does not lie under such a square
    some_under     no threat; some legal moves lie under such a square, but not all
    late           at most three empty squares (with or without an immediate win)
    quiet_win / quiet_loss / quiet_draw   no threat and no move under such a square; by the sign of `score`"""
    legal, wins, threat, under = root_facts(c0, c1)
    score = np.asarray(score, dtype=np.int64)
    tree = ~wins.any(axis=1)
    n_threat = threat.sum(axis=1)
    calm = tree & (n_threat == 0)
    n_under = (legal & under).sum(axis=1)
    n_free = (legal & ~under).sum(axis=1)
    quiet = calm & (n_under == 0)
    return {"tree": tree,
            "one_threat": tree & (n_threat == 1),
            "two_threats": tree & (n_threat >= 2),
            "block_under": tree & (n_threat == 1) & (threat & under).any(axis=1),
            "all_under": calm & (n_free == 0),
            "one_nonlosing": calm & (n_free == 1),
            "some_under": calm & (n_under > 0) & (n_free > 0),
            "late": SIZE - ages(c0, c1) <= 3,
            "quiet_win": quiet & (score > 0), "quiet_loss": quiet & (score < 0), "quiet_draw": quiet & (score == 0)}


def answer_of_score(score, age):
    """(outcome float64 0.0 / 0.5 / 1.0, final_age int64) of the mover's score at a position of age `age`: the mover is x at
    odd ages, a win ends at age 43 - |score|, a draw at 42."""
    s = np.asarray(score, dtype=np.int64)
    s = np.where(np.asarray(age) & 1, -s, s)
    return np.where(s > 0, 1.0, np.where(s < 0, 0.0, 0.5)), np.where(s != 0, 43 - np.abs(s), SIZE)


def labels_of_children(score, child_score):
    """The labelling rule of the reference's generate_7ply.py:83-91 from the oracle's scores alone: the mover's outcome is
    the sign of its score; a legal move keeps it iff the child's score (already from the mover's side) has the same sign;
    the prior is uniform over the keeping moves, formed in float64 and rounded to float32 once.
    Returns (v int64 [n] in -1 / 0 / +1, keep bool [n, 7], prior float32 [n, 7])."""
    child = np.asarray(child_score, dtype=np.int64)
    legal = child != NO_MOVE
    v = np.sign(np.asarray(score, dtype=np.int64))
    keep = legal & (np.sign(child) == v[:, None])
    p = keep.astype(np.float64)
    return v, keep, (p / p.sum(axis=1, keepdims=True)).astype(np.float32)


def windows(score, seed=22):
    """The six windows per row of the windowed checks, [(name, alpha int64 [n], beta int64 [n])]: the full window, (-1, +1),
    the two null windows at S = the oracle's score -- (S - 1, S) and (S, S + 1); |S| <= 41 keeps them inside -42..42 -- and two random ones
    from ``RandomState(seed)``: alpha uniform in -42..41, beta uniform in alpha + 1..42."""
    s = np.asarray(score, dtype=np.int64)
    n = len(s)
    rng = np.random.RandomState(seed)
    out = [("full", np.full(n, -42), np.full(n, 42)), ("outcome", np.full(n, -1), np.full(n, 1)),
           ("null_below", s - 1, s), ("null_above", s, s + 1)]
    for k in range(2):
        a = rng.randint(-42, 42, size=n)
        b = a + 1 + (rng.random_sample(n) * (42 - a)).astype(np.int64)
        out.append(("random%d" % k, a, np.minimum(b, 42)))
    return [(name, np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for name, a, b in out]


def expected_kind(score, alpha, beta):
    """The bound kind a search from (alpha, beta) must report at the exact score S: 1 LOWER iff S >= beta, 2 UPPER iff
    S <= alpha, else 3 EXACT (_lib.SOLVE_BOUND_*)."""
    s = np.asarray(score, dtype=np.int64)
    return np.where(s >= beta, 1, np.where(s <= alpha, 2, 3))


def window_violations(score, bound, alpha, beta, exact):
    """The rows that break the rule: the kind is ``expected_kind``; EXACT means score == S, LOWER beta <= score <= S, UPPER
    S <= score <= alpha."""
    score, bound, exact = (np.asarray(a, dtype=np.int64) for a in (score, bound, exact))
    kind = expected_kind(exact, alpha, beta)
    ok = (bound == kind) & np.where(kind == 3, score == exact,
                                    np.where(kind == 1, (beta <= score) & (score <= exact), (exact <= score) & (score <= alpha)))
    return np.nonzero(~ok)[0]


def solve_all(oracle, c0, c1, log2_entries=24):
    """(score, child_score, status) of every row from the exhaustive oracle with memos of 2^log2_entries words: rows a full
    memo leaves without an answer go to a fresh one.  A row that a fresh memo cannot hold raises ExactCapacityError."""
    c0, c1 = np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    memo = oracle.Exact(log2_entries)
    score, child, status = memo.scores_raw(c0, c1)
    while (status == oracle.EXACT_CAPACITY).any():
        todo = np.nonzero(status == oracle.EXACT_CAPACITY)[0]
        memo.close()
        memo = oracle.Exact(log2_entries)
        s, c, st = memo.scores_raw(c0[todo], c1[todo])
        if st[0] == oracle.EXACT_CAPACITY:
            raise oracle.ExactCapacityError("a row exceeds a fresh memo of 2^%d entries" % log2_entries)
        score[todo], child[todo], status[todo] = s, c, st
    memo.close()
    return score, child, status
