"""The audit of a transposition-table image of the exact solver (connect4_amd/csrc/c4_solve.hip), for the tests.

DESIGN's argument that answers do not depend on the table rests on one premise: every entry ever written is a true bound of
its position.  ``audit`` checks that premise on an image -- ``solver.Table.read()`` from the device, ``solver.HostTable.words``
on the host -- entry by entry, after the searches have finished:

* structure: the unused bits are zero, the kind is one of the three, the word sits in the slot its key hashes to, the key
  is a position (it decodes and encodes back), that position is one the search would have entered as an interior node
  (searchable, at least TT_MIN_EMPTIES empty squares, the mover cannot win at once), and the score is one enter_node's
  window allows at that age;
* value: with S the mover's exact score of the position from a table-free search, EXACT needs S == score, LOWER
  S >= score, UPPER S <= score.

Everything is NumPy over the whole image; the oracle is handed all positions at once.  Nothing here is code of the search:
the position tests below are written out again, on arrays, and tests/test_solver_table_audit_host.py holds them to
solver._classify and solver._winning_squares.
"""
import numpy as np

from connect4_amd import _lib as L
from connect4_amd.board import BOTTOM, H1, HEIGHT, SIZE, WIDTH
from connect4_amd.solver import _EXACT, _LOWER, _TT_HASH, _TT_KEY_MASK, _TT_MIN_EMPTIES, _UPPER, _popcount64, entry_fields

UNSOLVED = -128         # an oracle's answer for a row it could not solve: the entry is left out of the value check
KIND_NAMES = {_LOWER: "lower", _UPPER: "upper", _EXACT: "exact"}

_BOARD = np.uint64(BOTTOM * ((1 << HEIGHT) - 1))
_BOTTOM = np.uint64(BOTTOM)
_u = np.uint64


def wins(p):
    """bool [m]: the stones `p` (uint64 [m]) hold four in a row."""
    out = np.zeros(p.shape, dtype=bool)
    for s in (HEIGHT, H1, H1 + 1, 1):
        y = p & (p >> _u(s))
        out |= (y & (y >> _u(2 * s))) != 0
    return out


def winning_squares(p, occ):
    """uint64 [m]: the empty squares on which `p` completes four in a row, `occ` the occupied squares."""
    r = (p << _u(1)) & (p << _u(2)) & (p << _u(3))
    for s in (H1, HEIGHT, H1 + 1):
        q = (p << _u(s)) & (p << _u(2 * s))
        r |= q & (p << _u(3 * s))
        r |= q & (p >> _u(s))
        q = (p >> _u(s)) & (p >> _u(2 * s))
        r |= q & (p << _u(s))
        r |= q & (p >> _u(3 * s))
    return r & (_BOARD ^ occ)


def searchable(c0, c1):
    """bool [m]: a legal, unfinished position (what solver._classify calls SOLVED when every depth is allowed)."""
    occ = c0 | c1
    diff = _popcount64(c0) - _popcount64(c1)
    invalid = ((c0 & c1) != 0) | ((occ & ~_BOARD) != 0) | ((occ & (occ + _BOTTOM)) != 0) | (diff < 0) | (diff > 1)
    finished = wins(c0) | wins(c1) | (_popcount64(occ) == SIZE)
    return ~invalid & ~finished


def mover_score(outcome, final_age, age):
    """S: 43 - final_age for a win by o, final_age - 43 for a win by x, 0 for a draw; negated at odd ages.  outcome: 0.0 /
    0.5 / 1.0 as ``solve`` and ``solve_host`` give it."""
    outcome = np.asarray(outcome, dtype=np.float64)
    final_age = np.asarray(final_age, dtype=np.int64)
    s = np.where(outcome == 1.0, 43 - final_age, np.where(outcome == 0.0, final_age - 43, 0))
    return np.where(np.asarray(age) & 1, -s, s).astype(np.int64)


def score_range(age):
    """(lo, hi) of enter_node's window at `age`: no loss before age + 4, no win before age + 3."""
    age = np.asarray(age, dtype=np.int64)
    return np.where(age + 4 <= SIZE, age - 39, 0), np.where(age + 3 <= SIZE, 40 - age, 0)


def audit(words, log2_entries, exact_score_of_rows, report=None):
    """The violations of a table image: a list of ``(slot, word, what)``, empty for a sound table.

    words: uint64 [2^log2_entries].  exact_score_of_rows(rows): uint64 [m, 2] = (color0, color1) per row -> int64 [m], the
    mover's exact score S of each (``mover_score`` of a table-free answer), or UNSOLVED.  It is called once, with the
    entries that pass the structural checks.  report: a dict that receives entries, the count per kind, left_out (entries
    without a value check) and empties (the histogram of empty squares over the entries that decode)."""
    words = np.asarray(words, dtype=np.uint64)
    assert words.shape == (1 << log2_entries,)
    e = entry_fields(words)
    word = words[e.index]
    n = len(word)
    bad = []

    def flag(mask, what):
        for i in np.nonzero(mask)[0]:
            bad.append((int(e.index[i]), int(word[i]), what))
        return mask

    broken = flag((word >> _u(58)) != 0, "bits 58..63 are not zero")
    broken |= flag(~np.isin(e.kind, (_LOWER, _UPPER, _EXACT)), "the kind is none of lower, upper, exact")
    slot = (e.key * _u(_TT_HASH)) >> _u(64 - log2_entries)
    broken |= flag(slot != e.index.astype(np.uint64), "the word is not in the slot its key hashes to")
    is_position = ((e.mine + e.occ + _BOTTOM) & _u(_TT_KEY_MASK)) == e.key
    is_position &= ((e.mine & ~e.occ) == 0) & ((e.occ & ~_BOARD) == 0)
    broken |= flag(~is_position, "the key is no position")
    ok = is_position & searchable(e.color0, e.color1)
    broken |= flag(is_position & ~ok, "the position is invalid or finished")
    empties = SIZE - e.age
    broken |= flag(ok & (empties < _TT_MIN_EMPTIES), "fewer than TT_MIN_EMPTIES empty squares")
    at_once = (winning_squares(e.mine, e.occ) & (e.occ + _BOTTOM)) != 0
    broken |= flag(ok & at_once, "the mover wins at once: no interior node")
    lo, hi = score_range(e.age)
    broken |= flag(ok & ((e.score < lo) | (e.score > hi)), "the score is outside the window enter_node allows at this age")

    sound = ~broken
    rows = np.stack([e.color0[sound], e.color1[sound]], axis=1) if n else np.zeros((0, 2), dtype=np.uint64)
    exact = np.full(n, UNSOLVED, dtype=np.int64)
    if len(rows):
        answer = np.asarray(exact_score_of_rows(np.ascontiguousarray(rows)), dtype=np.int64)
        assert answer.shape == (len(rows),)
        exact[sound] = answer
    solved = sound & (exact != UNSOLVED)
    false_entry = solved & (((e.kind == _EXACT) & (exact != e.score)) | ((e.kind == _LOWER) & (exact < e.score))
                            | ((e.kind == _UPPER) & (exact > e.score)))
    for i in np.nonzero(false_entry)[0]:
        bad.append((int(e.index[i]), int(word[i]), "false entry: %s %d at age %d, the exact score is %d (color0 %#x, color1 %#x)" % (
            KIND_NAMES[int(e.kind[i])], e.score[i], e.age[i], exact[i], int(e.color0[i]), int(e.color1[i]))))
    if report is not None:
        report.update(entries=n, left_out=int(n - solved.sum()), empties=np.bincount(empties[is_position], minlength=SIZE + 1),
                      **{name: int((e.kind == k).sum()) for k, name in KIND_NAMES.items()})
    return bad


def summary(report):
    return "%d entries (%d lower, %d upper, %d exact), %d without a value check" % (
        report["entries"], report["lower"], report["upper"], report["exact"], report["left_out"])


def pick_roots(empties, count, seed, min_stores=16, max_nodes=4096):
    """`count` distinct positions with `empties` empty squares that are worth auditing, drawn by ``random_playout`` from
    ``RandomState(seed)``: the mover cannot win at once, and the host model, searching the position alone against a fresh
    ``HostTable(14)``, answers within `max_nodes` nodes and stores at least `min_stores` entries (most random playouts
    are decided in a node or two and would write nothing).  Returns ``[(board, HostAnswer)]``."""
    from connect4_amd.solver import HostTable, _winning_squares, random_playout, solve_host
    rng = np.random.RandomState(seed)
    seen, out = set(), []
    for _ in range(20000):
        if len(out) == count:
            return out
        b = random_playout(rng, SIZE - empties)
        c0, c1 = b.color
        occ = c0 | c1
        if tuple(b.color) in seen or _winning_squares(c1 if b.age & 1 else c0, occ) & (occ + BOTTOM):
            continue
        seen.add(tuple(b.color))
        table = HostTable(14)
        a = solve_host(b, node_budget=max_nodes, table=table)
        if a.status == L.SOLVE_SOLVED and table.stores >= min_stores:
            out.append((b, a))
    raise AssertionError("no %d roots with %d empty squares" % (count, empties))


def host_oracle(cache=None):
    """exact_score_of_rows from ``solve_host(deep=True)``, the table-free search in Python; `cache`: a dict shared between
    audits (a position's score is its own)."""
    from connect4_amd.solver import solve_host
    cache = {} if cache is None else cache

    def exact_score_of_rows(rows):
        out = np.empty(len(rows), dtype=np.int64)
        for i, (c0, c1) in enumerate(rows):
            at = (int(c0), int(c1))
            if at not in cache:
                a = solve_host(at, deep=True)
                age = bin(at[0] | at[1]).count("1")
                cache[at] = int(mover_score(a.outcome, a.final_age, age)) if a.status == L.SOLVE_SOLVED else UNSOLVED
            out[i] = cache[at]
        return out

    return exact_score_of_rows


def exact_oracle(oracle, log2_entries=26, warm_rows=None):
    """exact_score_of_rows from the oracle's exhaustive search (oracle/c4_oracle.c c4o_exact_scores: every legal move of every
    position, a memo of exact values, nothing of the solver's reasoning) -- a yardstick that shares no rule with the search
    that wrote the table.  `oracle`: the module oracle.c4oracle.  One memo of 2^log2_entries words serves every call of the
    returned function; warm_rows (uint64 [m, 2]), searched first, put the positions below them into it, so that the
    entries of a table those rows filled are memo hits.  Rows a full memo cannot answer go to a fresh one; a position that
    is finished or invalid is UNSOLVED."""
    state = {"memo": oracle.Exact(log2_entries)}

    def exact_score_of_rows(rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
        score, _, status = state["memo"].scores_raw(rows[:, 0], rows[:, 1])
        full = np.nonzero(status == oracle.EXACT_CAPACITY)[0]
        if len(full):
            state["memo"].close()
            state["memo"] = oracle.Exact(log2_entries)
            score[full], _, status[full] = state["memo"].scores_raw(rows[full, 0], rows[full, 1])
        return np.where(status == oracle.EXACT_SEARCHED, score.astype(np.int64), UNSOLVED)

    if warm_rows is not None:
        exact_score_of_rows(warm_rows)
    return exact_score_of_rows
