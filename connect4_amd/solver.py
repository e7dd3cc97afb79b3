"""Exact values of late-game positions, and test sets labelled with them.

The reference defines a position's exact value through ``GridSearch(plies >= empty squares)``: no evaluator is reached
(oinkoink/grid_search.py:38-71), so the search returns the game-theoretic result with its terminal scoring -- an o win that
ends at age ``a`` is ``1 - a/10000``, an x win ``a/10000``, a draw ``0.5 + 42/10000``.  That search is exhaustive; the kernel
behind this module (connect4_amd/csrc/c4_solve.hip) finds the same number by alpha-beta, for positions with at most
``MAX_EMPTIES`` = 24 empty squares -- and, asked for with ``deep=True``, a ``Table`` or ``split_plies``, for every position
(``DEEP_MAX_EMPTIES`` = 42): the same search with 42 plies of stack, a transposition table in device memory that all rows of
all calls share, and a split that spreads one hard position over many lanes.  Neither changes an answer.

``solve``       status, outcome, final age, the reference's float64 value, the node count and the table hits of every row
``Table``       the owner of a device transposition table
``grid_triple`` ``(move, value, tree)`` per board, what ``grid_search(boards, plies=empties, evaluate_centre)`` returns
``label``       a ``LabelledSet`` (value = outcome, prior = uniform over the moves that keep it: the rule of
                oinkoink/scripts/generate_7ply.py:83-91) and a report
``solve_window`` the deep search from a root window per row: the score the root returns and whether it is exact, a lower or an
                upper bound against that window; ``outcomes`` is the window (-1, +1), the cheapest search that tells who wins
``label(exact=False)`` / ``label_values``  the same labels from outcome windows and null windows instead of exact scores
``solve_host``  a plain-Python mirror of the kernel's search -- same integer score, same pruning and move order, same node
                counts -- for tests and for machines without a GPU; with ``table={}`` also of its probe / store logic
``HostTable``   the kernel's table (layout, slot function, always-replace) behind ``solve_host(table=...)``;
                ``entry_fields`` takes a table image (``Table.read()``, ``HostTable.words``) apart

The integer score: a game o wins at age ``a`` scores ``43 - a``, one x wins ``a - 43``, a draw 0, taken from the side to
move inside the search.  It is strictly monotone in the reference's float, so max / min over it pick what the reference's
max / min pick; the float itself is formed once, from outcome and age, by the division the reference performs.
"""
import contextlib
import ctypes as C
import functools
import time
from collections import namedtuple
from typing import Sequence

import numpy as np

from . import _lib as L
from .board import BOTTOM, H1, HEIGHT, SIZE, WIDTH, Board, _wins
from .grid_search import GridTree, _terminal_value
from .utils import Side

__all__ = ["Book", "HostBook", "enumerate_ply", "MAX_EMPTIES", "DEEP_MAX_EMPTIES", "DEFAULT_NODE_BUDGET", "STATUS_NAMES", "Solved", "HostAnswer", "Table", "HostTable",
           "EntryFields", "entry_fields", "solve", "solve_host", "HostWindowAnswer", "Windowed", "BOUND_NAMES", "solve_window", "outcomes",
           "label_values", "staged_labels", "drive_host", "drive_graph_host", "solve_graph", "Graph", "NODE_STATE_NAMES", "grid_triple", "label", "prior_from_children", "value_from_answer", "random_playout", "random_openings"]

MAX_EMPTIES = L.SOLVE_MAX_EMPTIES
DEEP_MAX_EMPTIES = L.SOLVE_DEEP_MAX_EMPTIES     # every position: c4_solve_deep and solve(deep=True / table=)
DEFAULT_NODE_BUDGET = 1 << 26          # the kernel's default (c4_engine.h)
STATUS_NAMES = {L.SOLVE_SOLVED: "solved", L.SOLVE_TERMINAL: "terminal", L.SOLVE_UNKNOWN: "unknown",
                L.SOLVE_TOO_DEEP: "too_deep", L.SOLVE_INVALID: "invalid"}

Solved = namedtuple("Solved", "status outcome final_age value nodes table_hits")
class HostAnswer(namedtuple("HostAnswer", "status outcome final_age value nodes")):
    """``solve_host``'s answer.  Beside the tuple's fields -- they alone take part in comparisons -- it carries hits, what the
    kernel counts into table_hits (table and book probes that returned or narrowed), and book_probes, the nodes at which
    the book was looked up.  The two are plain attributes set on the answer ``solve_host`` returns: they are in neither the
    repr nor a comparison, and a copy made by a tuple operation (``_replace``, slicing, pickling) has the class defaults, 0."""
    hits = 0
    book_probes = 0


class HostWindowAnswer(namedtuple("HostWindowAnswer", "status score bound outcome final_age value nodes")):
    """``solve_host(window=)``'s answer; hits and book_probes as ``HostAnswer`` has them."""
    hits = 0
    book_probes = 0


Windowed = namedtuple("Windowed", "status score bound outcome final_age nodes table_hits")
BOUND_NAMES = {L.SOLVE_BOUND_NONE: "none", L.SOLVE_BOUND_LOWER: "lower", L.SOLVE_BOUND_UPPER: "upper", L.SOLVE_BOUND_EXACT: "exact"}
SCORE_MAX = 42      # beyond every score: (-SCORE_MAX, SCORE_MAX) is the full window

_BOARD = BOTTOM * ((1 << HEIGHT) - 1)
_COL = (1 << HEIGHT) - 1
_PRIO = {3: 6, 2: 5, 4: 4, 1: 3, 5: 2, 0: 1, 6: 0}     # ties: centre first


def value_from_answer(outcome, final_age):
    """The reference's float64 (grid_search.py:46-49) of a game with result `outcome` (0.0 / 0.5 / 1.0) that ends at age
    `final_age`; scalars or arrays."""
    outcome = np.asarray(outcome, dtype=np.float64)
    age = np.asarray(final_age, dtype=np.float64)
    return np.where(outcome == 1.0, outcome - age / 10000.0, outcome + age / 10000.0)


def random_playout(rng, n_stones):
    """An undecided position after `n_stones` uniformly random legal moves (np.random.RandomState `rng`)."""
    while True:
        b = Board()
        for _ in range(n_stones):
            b.make_move(int(rng.choice(sorted(b.valid_moves))))
            if b.result is not None:
                break
        if b.result is None and b.age == n_stones:
            return b


def random_openings(plies, count, seed=0, max_draws=None):
    """`count` distinct undecided positions after `plies` uniformly random legal moves (``random_playout`` from
    ``RandomState(seed)``), in the order drawn: a sample of the set the reference's ``make_random_ips(plies)`` enumerates
    (oinkoink/board.py:225-243).  Fewer than `count` if `max_draws` (default 64 * count + 64) playouts do not yield them."""
    rng = np.random.RandomState(seed)
    seen, out = set(), []
    for _ in range(64 * count + 64 if max_draws is None else max_draws):
        if len(out) >= count:
            break
        b = random_playout(rng, plies)
        if tuple(b.color) not in seen:
            seen.add(tuple(b.color))
            out.append(b)
    return out


# -- the host mirror ------------------------------------------------------------------------------------------------------
def _winning_squares(p, occ):
    r = (p << 1) & (p << 2) & (p << 3)
    for s in (H1, HEIGHT, H1 + 1):
        q = (p << s) & (p << 2 * s)
        r |= q & (p << 3 * s)
        r |= q & (p >> s)
        q = (p >> s) & (p >> 2 * s)
        r |= q & (p << s)
        r |= q & (p >> 3 * s)
    return r & (_BOARD ^ occ)


class _OverBudget(Exception):
    pass


_LOWER, _UPPER, _EXACT = 1, 2, 3        # the bound kinds of a table entry (c4_solve.hip TT_*)
_TT_MIN_EMPTIES = 6                     # nodes with fewer empty squares neither probe nor store (c4_solve.hip)


_TT_KEY_BITS, _TT_SCORE_SHIFT, _TT_KIND_SHIFT = 49, 49, 56      # the entry word (c4_solve.hip tt_store)
_TT_KEY_MASK = (1 << _TT_KEY_BITS) - 1
_TT_HASH = 0x9E3779B97F4A7C15                                   # tt_slot

EntryFields = namedtuple("EntryFields", "index key score kind mine occ color0 color1 age")


class HostTable:
    """The kernel's table on the host: ``2 ** log2_entries`` words of its layout (key in bits 0..48, score + 64 in bits
    49..55, kind in bits 56..57), its slot function (the top `log2_entries` bits of ``key * 0x9E3779B97F4A7C15 mod 2^64``),
    always-replace, and a hit only on the whole key.  It is what ``solve_host(table=...)`` takes in place of a dict;
    ``words`` is the image ``Table.read()`` returns for the same stores in the same order.  ``stores`` counts the stores,
    ``replaced`` those that overwrote an entry of another key, ``hits`` what ``table_hits`` counts, summed over the
    ``solve_host`` calls the table was given to."""

    def __init__(self, log2_entries):
        if not L.SOLVE_TABLE_MIN_LOG2 <= int(log2_entries) <= L.SOLVE_TABLE_MAX_LOG2:
            raise ValueError("log2_entries %r outside %d..%d" % (log2_entries, L.SOLVE_TABLE_MIN_LOG2, L.SOLVE_TABLE_MAX_LOG2))
        self.log2_entries = int(log2_entries)
        self.words = np.zeros(1 << self.log2_entries, dtype=np.uint64)
        self.stores = 0
        self.replaced = 0
        self.hits = 0

    def slot(self, key):
        return ((key * _TT_HASH) & 0xFFFFFFFFFFFFFFFF) >> (64 - self.log2_entries)

    def get(self, key, default=None):
        w = int(self.words[self.slot(key)])
        if w & _TT_KEY_MASK != key:
            return default
        return (w >> _TT_KIND_SHIFT) & 3, ((w >> _TT_SCORE_SHIFT) & 0x7f) - 64

    def __setitem__(self, key, entry):
        kind, score = entry
        at = self.slot(key)
        old = int(self.words[at])
        self.stores += 1
        self.replaced += 1 if old and old & _TT_KEY_MASK != key else 0
        self.words[at] = np.uint64(key | ((score + 64) << _TT_SCORE_SHIFT) | (kind << _TT_KIND_SHIFT))


def _popcount64(x):
    x = np.asarray(x, dtype=np.uint64)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).astype(np.int64)
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((x * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.int64)


def entry_fields(words):
    """Every non-zero word of a table image (``Table.read()``, ``HostTable.words``) taken apart, as ``EntryFields`` of
    arrays: index (the word's slot), key, score, kind, the mover's stones, the occupied squares, color0, color1 and age.

    The key is mover's stones + occupied squares + bottom row, so the 7-bit field of a column of height h is
    ``f = 2^h + (the mover's stones in it)``: h = floor(log2 f), the mover's stones are f - 2^h, the occupied cells 2^h - 1.
    The mover is x (color1) at odd ages.  A field of 0 belongs to no position: it decodes as an empty column, and
    ``mine + occ + BOTTOM`` then differs from the key."""
    words = np.asarray(words, dtype=np.uint64)
    index = np.nonzero(words)[0]
    w = words[index]
    key = w & np.uint64(_TT_KEY_MASK)
    score = ((w >> np.uint64(_TT_SCORE_SHIFT)) & np.uint64(0x7f)).astype(np.int64) - 64
    kind = ((w >> np.uint64(_TT_KIND_SHIFT)) & np.uint64(3)).astype(np.int64)
    top = np.array([0] + [1 << (f.bit_length() - 1) for f in range(1, 1 << H1)], dtype=np.uint64)    # 2^floor(log2 f)
    mine = np.zeros_like(key)
    occ = np.zeros_like(key)
    for c in range(WIDTH):
        f = (key >> np.uint64(H1 * c)) & np.uint64((1 << H1) - 1)
        t = top[f.astype(np.int64)]
        mine |= (f - t) << np.uint64(H1 * c)
        occ |= (np.maximum(t, np.uint64(1)) - np.uint64(1)) << np.uint64(H1 * c)
    age = _popcount64(occ)
    odd = (age & 1) == 1
    theirs = occ ^ (mine & occ)
    return EntryFields(index, key, score, kind, mine, occ, np.where(odd, theirs, mine), np.where(odd, mine, theirs), age)


def _mirror_key(key):
    """The key of the mirror image: no 7-bit column field of ``mine + occ + BOTTOM`` carries into the next, so it is the
    key with its seven fields reversed (c4_solve.hip tt_mirror_key).  An int or a uint64 array."""
    if isinstance(key, np.ndarray):
        out = np.zeros_like(key)
        for c in range(WIDTH):
            out |= ((key >> np.uint64(H1 * c)) & np.uint64((1 << H1) - 1)) << np.uint64(H1 * (WIDTH - 1 - c))
        return out
    return sum(((key >> (H1 * c)) & ((1 << H1) - 1)) << (H1 * (WIDTH - 1 - c)) for c in range(WIDTH))


def _probe_entry(hit, alpha, beta):
    """c4_solve.hip probe_word on a ``(kind, score)`` entry: (0 nothing / 1 narrowed / 2 closes, alpha, beta, score)."""
    kind, s = hit
    if kind == _EXACT or (kind == _LOWER and s >= beta) or (kind == _UPPER and s <= alpha):
        return 2, alpha, beta, s
    if kind == _LOWER and s > alpha:
        return 1, s, beta, s
    if kind == _UPPER and s < beta:
        return 1, alpha, s, s
    return 0, alpha, beta, s


class _Search:
    """`table`: None, a dict ``key -> (kind, score)`` -- the kernel's transposition table without its replacement -- or a
    ``HostTable``, the kernel's table with it.  `book`: None or a ``Book``, probed before the table at nodes of its age."""

    def __init__(self, budget, table=None, book=None):
        self.nodes = 0
        self.budget = budget
        self.table = table
        self.book = book
        self.hits = 0
        self.book_probes = 0
        self.hit_at = []        # the node count at every hit: the hits of a search stopped after c nodes are those <= c
        self.clean = True

    def _hit(self):
        self.hits += 1
        self.hit_at.append(self.nodes)

    def enter(self):
        if self.nodes >= self.budget:
            raise _OverBudget()
        self.nodes += 1
        self.clean = True       # every return since the last node entered was a cut-off (drive_host's launch model)

    def node(self, mine, theirs, age, alpha, beta):
        """Score for the mover of a position whose mover cannot win at once (c4_solve.hip enter_node + run_lane)."""
        self.enter()
        if age == SIZE - 1:
            return 0
        occ = mine | theirs
        possible = (occ + BOTTOM) & _BOARD
        opp_win = _winning_squares(theirs, occ)
        forced = possible & opp_win
        if forced:
            if forced & (forced - 1):
                return age - 41
            possible = forced
        possible &= ~(opp_win >> 1)
        if not possible:
            return age - 41
        lo = age - 39 if age + 4 <= SIZE else 0
        hi = 40 - age if age + 3 <= SIZE else 0
        if beta > hi:
            beta = hi
            if alpha >= beta:
                return beta
        if alpha < lo:
            alpha = lo
            if alpha >= beta:
                return alpha
        if self.book is not None and age == self.book.age:
            # the book first (c4_solve.hip book_probe), whatever _TT_MIN_EMPTIES and the table are: an entry that closes
            # the node returns, one that narrows hands the narrowed window on
            self.book_probes += 1
            hit = self.book.get(mine + occ + BOTTOM)
            if hit is not None:
                how, alpha, beta, s = _probe_entry(hit, alpha, beta)
                if how:
                    self._hit()
                if how == 2:
                    return s
        if self.table is not None and SIZE - age >= _TT_MIN_EMPTIES:
            # probe (c4_solve.hip tt_probe): the key is the position, the score its mover's, so an entry is a true bound
            # wherever and whenever it was written
            key = mine + occ + BOTTOM
            hit = self.table.get(key)
            if hit is not None:
                how, alpha, beta, s = _probe_entry(hit, alpha, beta)
                if how:
                    self._hit()
                if how == 2:
                    return s
            ret = self._moves(mine, theirs, occ, possible, age, alpha, beta)
            # store (tt_store): against the window the moves were searched with
            self.table[key] = (_UPPER if ret <= alpha else _LOWER if ret >= beta else _EXACT, ret)
            return ret
        return self._moves(mine, theirs, occ, possible, age, alpha, beta)

    def _moves(self, mine, theirs, occ, possible, age, alpha, beta):
        keyed = []
        for c in range(WIDTH):
            bit = possible & (_COL << (H1 * c))
            if bit:
                keyed.append((bin(_winning_squares(mine | bit, occ | bit)).count("1") * 8 + _PRIO[c], bit))
        keyed.sort(reverse=True)
        for _, bit in keyed:
            v = -self.node(theirs, mine | bit, age + 1, -beta, -alpha)
            if v >= beta:
                return v
            self.clean = False
            if v > alpha:
                alpha = v
        return alpha


def _classify(c0, c1, max_empties=None):
    max_empties = MAX_EMPTIES if max_empties is None else max_empties
    occ = c0 | c1
    n0, n1 = bin(c0).count("1"), bin(c1).count("1")
    if (c0 & c1) or (occ & ~_BOARD) or (occ & (occ + BOTTOM)) or not 0 <= n0 - n1 <= 1 or (_wins(c0) and _wins(c1)):
        return L.SOLVE_INVALID
    if _wins(c0) or _wins(c1) or n0 + n1 == SIZE:
        return L.SOLVE_TERMINAL
    if SIZE - (n0 + n1) > max_empties:
        return L.SOLVE_TOO_DEEP
    return L.SOLVE_SOLVED


def _check_window(alpha, beta):
    if not (float(alpha).is_integer() and float(beta).is_integer() and -SCORE_MAX <= alpha < beta <= SCORE_MAX):
        raise ValueError("the window (%r, %r) is not -%d <= alpha < beta <= %d in whole numbers" % (alpha, beta, SCORE_MAX, SCORE_MAX))
    return int(alpha), int(beta)


def _bound_kind(score, alpha, beta):
    return L.SOLVE_BOUND_LOWER if score >= beta else L.SOLVE_BOUND_UPPER if score <= alpha else L.SOLVE_BOUND_EXACT


def solve_host(board, node_budget=None, table=None, deep=False, window=None, book=None):
    """The kernel's answer for one position, computed in plain Python: ``HostAnswer(status, outcome, final_age, value,
    nodes)``.  `board`: a Board or a ``(color0, color1)`` pair.  outcome / value are None where the status has none.

    deep=True is c4_solve_deep's table-free search (any number of empty squares, never TOO_DEEP).  table: a ``dict``, which
    implies deep -- the kernel's probe / store / bound logic on ``key -> (kind, score)`` entries; the dict may be shared by
    any number of calls, the answer does not depend on what it holds, the node count does.  A ``HostTable`` in its place
    adds the kernel's slots and replacement: one row at a time it holds, word for word, what one lane leaves in a ``Table``.

    window=(alpha, beta), -42 <= alpha < beta <= 42 on the mover's score, implies deep and is c4_solve_window's row: the
    root is entered with that window instead of (-42, 42), and the answer is a ``HostWindowAnswer`` that also has the score
    the root returns and its kind against the window (_lib.SOLVE_BOUND_*): exact inside it, a lower bound at or above beta,
    an upper bound at or below alpha.  outcome, final_age and value are None / -1 unless the bound is exact; rows that are
    not searched have score 0 and bound SOLVE_BOUND_NONE.

    book: a ``Book`` (implies deep), probed like the kernel probes it: before the table, at every node of the book's age,
    the root included.  Table-free the node count is the kernel's, and the answer's ``hits`` are its table_hits."""
    c0, c1 = (board.color if isinstance(board, Board) else board)
    c0, c1 = int(c0), int(c1)
    budget = DEFAULT_NODE_BUDGET if node_budget is None else int(node_budget)
    if window is not None:
        w_alpha, w_beta = _check_window(*window)
    else:
        w_alpha, w_beta = -SCORE_MAX, SCORE_MAX
    st = _classify(c0, c1, DEEP_MAX_EMPTIES if deep or table is not None or window is not None or book is not None else MAX_EMPTIES)
    s = None

    def answer(status, outcome, final_age, value, nodes, score=0, bound=L.SOLVE_BOUND_NONE):
        ans = HostAnswer(status, outcome, final_age, value, nodes) if window is None else \
            HostWindowAnswer(status, score, bound, outcome, final_age, value, nodes)
        if s is not None:
            ans.hits, ans.book_probes = s.hits, s.book_probes
        return ans

    if st == L.SOLVE_TERMINAL:
        outcome = 1.0 if _wins(c0) else 0.0 if _wins(c1) else 0.5
        age = bin(c0 | c1).count("1")
        return answer(st, outcome, age, float(value_from_answer(outcome, age)), 0)
    if st != L.SOLVE_SOLVED:
        return answer(st, None, -1, None, 0)
    occ = c0 | c1
    age = bin(occ).count("1")
    mine, theirs = (c1, c0) if age & 1 else (c0, c1)
    s = _Search(budget, table, book)
    if _winning_squares(mine, occ) & (occ + BOTTOM):
        score, nodes = 42 - age, 1
    else:
        try:
            score = s.node(mine, theirs, age, w_alpha, w_beta)
        except _OverBudget:
            return answer(L.SOLVE_UNKNOWN, None, -1, None, s.nodes)
        finally:
            if isinstance(table, HostTable):
                table.hits += s.hits
        nodes = s.nodes
    bound = _bound_kind(score, w_alpha, w_beta)
    if bound != L.SOLVE_BOUND_EXACT:        # only a windowed search gets here: no score leaves (-42, 42)
        return answer(L.SOLVE_SOLVED, None, -1, None, nodes, score, bound)
    abs_score = -score if age & 1 else score
    outcome = 1.0 if abs_score > 0 else 0.0 if abs_score < 0 else 0.5
    final_age = 43 - abs(abs_score) if abs_score else SIZE
    return answer(L.SOLVE_SOLVED, outcome, final_age, float(value_from_answer(outcome, final_age)), nodes, score, bound)


# -- the device ------------------------------------------------------------------------------------------------------------
def _check(rc):
    if rc != L.OK:
        msg = L.load().c4_solve_last_error()
        raise L.EngineError(rc, msg.decode("utf-8", "replace") if msg else "")


def _bits(boards):
    """(color0, color1) uint64 arrays of a sequence of Boards or (color0, color1) pairs."""
    pairs = [(b.color[0], b.color[1]) if isinstance(b, Board) else (int(b[0]), int(b[1])) for b in boards]
    a = np.array(pairs, dtype=np.uint64).reshape(len(pairs), 2)
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])


def _is_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _rows_u64(boards):
    """uint64 [n, 2] of a packed tensor, a uint64 / int64 [n, 2] array or a sequence of Boards or pairs."""
    if _is_tensor(boards):
        return boards.cpu().numpy().view(np.uint64).reshape(-1, 2)
    if isinstance(boards, np.ndarray):
        return np.ascontiguousarray(boards).view(np.uint64).reshape(-1, 2)
    return np.stack(_bits(boards), axis=1) if len(boards) else np.zeros((0, 2), dtype=np.uint64)


def _ptr(x):
    """What the C entry points take: the address of a device tensor, or of a NumPy array typed by its dtype; None (an optional
    argument left out) stays None."""
    if x is None:
        return None
    return C.c_void_p(x.data_ptr()) if _is_tensor(x) else x.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(x.dtype)))


def _packed_on_device(boards, device):
    """A contiguous int64 [n, 2] cuda tensor of `boards` (a packed tensor on any device, or a sequence of Boards)."""
    import torch
    if _is_tensor(boards):
        if boards.dtype != torch.int64 or boards.dim() != 2 or boards.shape[1] != 2:
            raise ValueError("packed boards are a torch int64 tensor [n, 2] = {color0, color1} per row; got %s %s" % (
                boards.dtype, tuple(boards.shape)))
        t = boards
    else:
        c0, c1 = _bits(boards)
        t = torch.from_numpy(np.stack([c0, c1], axis=1).view(np.int64))
    if t.device.type != "cuda":
        if not torch.cuda.is_available():
            raise L.EngineError(L.EDEVICE, "the solver runs on the GPU (c4_solve_dev) and there is no CPU fallback; "
                                           "solve_host answers single positions in Python")
        t = t.to(torch.device("cuda", device))
    return t.contiguous()


class Table:
    """A transposition table in device memory (c4_solve_table_create): ``2 ** log2_entries`` entries of 8 bytes, zero-filled.
    Pass it to ``solve`` / ``grid_triple`` / ``label`` as ``table=``; any number of calls may share it, and what it holds
    never changes an answer, only how many nodes the answer costs.  ``clear()`` empties it (for measurements); ``close()``
    frees it (also on garbage collection and at the end of a ``with`` block)."""

    def __init__(self, log2_entries=24, device=0):
        self._h = None
        h = C.c_void_p()
        if log2_entries is None:        # Table.entryless
            _check(L.load().c4_solve_table_create_entryless(int(device), C.byref(h)))
        else:
            _check(L.load().c4_solve_table_create(int(device), int(log2_entries), C.byref(h)))
        self._h = h
        self.log2_entries = None if log2_entries is None else int(log2_entries)
        self.device = int(device)
        self.book = None        # attach_book

    @classmethod
    def entryless(cls, device=0):
        """A handle without entries (c4_solve_table_create_entryless): the table-free search, there to carry a book."""
        return cls(None, device)

    def attach_book(self, book):
        """Every later call given this table probes `book` (a ``Book``, or None: no book) at the book's ply.  The book must
        stay open for as long as it is attached; ``book=`` of the solving calls attaches and detaches for one call."""
        _check(L.load().c4_solve_table_attach_book(self.handle, None if book is None else book.handle(self.device)))
        self.book = book        # keeps the device image alive

    @property
    def entries(self):
        return 0 if self.log2_entries is None else 1 << self.log2_entries

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("the table is closed")
        return self._h

    def clear(self):
        _check(L.load().c4_solve_table_clear(self.handle, None))

    def read(self):
        """The table's ``2 ** log2_entries`` words as a ``numpy.uint64`` array (c4_solve_table_read): every store of every
        call that has returned is in it.  ``entry_fields`` takes it apart; ``HostTable.words`` has the same layout."""
        out = np.empty(self.entries, dtype=np.uint64)
        _check(L.load().c4_solve_table_read(self.handle, _ptr(out), out.size))
        return out

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            L.load().c4_solve_table_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _solve_dev(packed, node_budget=None, nodes_per_launch=None, table=None, deep=False, window=None):
    """A packed cuda tensor through the _dev entry point the arguments select: c4_solve_dev; with `deep` or a `table`
    c4_solve_deep_dev; with `window` = (alpha, beta), int8 NumPy arrays or both None, c4_solve_window_dev.  Returns device
    tensors (status int8, outcome int8, final_age int8, nodes int64, table_hits int64) and, with a window, (score int8, bound
    int8) after them."""
    import torch
    n = int(packed.shape[0])
    dev = packed.device
    status, outcome, age = (torch.empty(n, dtype=torch.int8, device=dev) for _ in range(3))
    extra = tuple(torch.empty(n, dtype=torch.int8, device=dev) for _ in range(2)) if window is not None else ()      # score, bound
    nodes = torch.empty(n, dtype=torch.int64, device=dev)
    hits = torch.zeros(n, dtype=torch.int64, device=dev)
    if n:
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            a_dev, b_dev = (torch.from_numpy(x).to(dev) if x is not None else None for x in (window or (None, None)))
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            handle = table.handle if table is not None else None
            size = (n, int(node_budget or 0), int(nodes_per_launch or 0))
            lib = L.load()
            if window is not None:
                rc = lib.c4_solve_window_dev(idx, stream, handle, _ptr(packed), _ptr(a_dev), _ptr(b_dev), *size, _ptr(status), _ptr(extra[0]),
                                             _ptr(extra[1]), _ptr(outcome), _ptr(age), _ptr(nodes), _ptr(hits))
            elif deep or table is not None:
                rc = lib.c4_solve_deep_dev(idx, stream, handle, _ptr(packed), *size, _ptr(status), _ptr(outcome), _ptr(age), _ptr(nodes),
                                           _ptr(hits))
            else:
                rc = lib.c4_solve_dev(idx, stream, _ptr(packed), *size, _ptr(status), _ptr(outcome), _ptr(age), _ptr(nodes))
            _check(rc)
    return (status, outcome, age, nodes, hits) + extra


def _solve_arrays(boards, node_budget, nodes_per_launch, device, table, deep, window=None):
    """``_solve_dev`` for a sequence of Boards or pairs, through the entry points that take host arrays (c4_solve, c4_solve_deep,
    c4_solve_window): the same tuple, of NumPy arrays."""
    n = len(boards)
    status, outcome, age = (np.zeros(n, dtype=np.int8) for _ in range(3))
    extra = tuple(np.zeros(n, dtype=np.int8) for _ in range(2)) if window is not None else ()     # score, bound
    nodes = np.zeros(n, dtype=np.int64)
    hits = np.zeros(n, dtype=np.int64)
    if n:
        bits = _bits(boards)
        c0, c1 = (_ptr(x) for x in bits)
        handle = table.handle if table is not None else None
        size = (n, int(node_budget or 0), int(nodes_per_launch or 0))
        lib = L.load()
        if window is not None:
            rc = lib.c4_solve_window(device, handle, c0, c1, _ptr(window[0]), _ptr(window[1]), *size, _ptr(status), _ptr(extra[0]), _ptr(extra[1]),
                                     _ptr(outcome), _ptr(age), _ptr(nodes), _ptr(hits))
        elif deep:
            rc = lib.c4_solve_deep(device, handle, c0, c1, *size, _ptr(status), _ptr(outcome), _ptr(age), _ptr(nodes), _ptr(hits))
        else:
            rc = lib.c4_solve(device, c0, c1, *size, _ptr(status), _ptr(outcome), _ptr(age), _ptr(nodes))
        _check(rc)
    return (status, outcome, age, nodes, hits) + extra


def _solve_any(boards, node_budget, nodes_per_launch, device, table, deep, window=None):
    """``_solve_dev`` for a packed tensor on any device, ``_solve_arrays`` for anything else; NumPy arrays either way."""
    if _is_tensor(boards):
        return tuple(t.cpu().numpy() for t in _solve_dev(_packed_on_device(boards, device), node_budget, nodes_per_launch, table, deep, window))
    return _solve_arrays(boards, node_budget, nodes_per_launch, device, table, deep, window)


def _children_dev(packed):
    """c4_solve_children_dev: (children int64 [n, 7, 2], legal int8 [n, 7]) device tensors."""
    import torch
    n = int(packed.shape[0])
    dev = packed.device
    children = torch.zeros((n, WIDTH, 2), dtype=torch.int64, device=dev)
    legal = torch.zeros((n, WIDTH), dtype=torch.int8, device=dev)
    if n:
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(L.load().c4_solve_children_dev(idx, C.c_void_p(stream), _ptr(packed), n, _ptr(children), _ptr(legal)))
    return children, legal


def _outcome(outcome):
    """(known bool, float64 0.0 / 0.5 / 1.0 or NaN) of C4_RESULT_* codes, -1 where a row has none."""
    known = np.asarray(outcome) >= 0
    return known, np.where(known, np.asarray(outcome, dtype=np.float64) * 0.5, np.nan)


def _finish(status, outcome, age, nodes, hits=None):
    status = np.asarray(status, dtype=np.int8)
    age = np.asarray(age, dtype=np.int8)
    known, out = _outcome(outcome)
    value = np.where(known, value_from_answer(np.where(known, out, 0.0), np.where(known, age, 0)), np.nan)
    nodes = np.asarray(nodes, dtype=np.int64)
    return Solved(status, out, age, value, nodes, np.zeros_like(nodes) if hits is None else np.asarray(hits, dtype=np.int64))


def _solve_window_dev(packed, alpha, beta, node_budget=None, nodes_per_launch=None, table=None):
    """``_solve_dev(window=(alpha, beta))`` in c4_solve_window_dev's order of outputs: (status, score, bound, outcome, final_age,
    nodes, table_hits)."""
    status, outcome, age, nodes, hits, score, bound = _solve_dev(packed, node_budget, nodes_per_launch, table, window=(alpha, beta))
    return status, score, bound, outcome, age, nodes, hits


def _finish_window(status, outcome, age, nodes, hits, score, bound):
    return Windowed(np.asarray(status, dtype=np.int8), np.asarray(score, dtype=np.int8), np.asarray(bound, dtype=np.int8),
                    _outcome(outcome)[1], np.asarray(age, dtype=np.int8), np.asarray(nodes, dtype=np.int64),
                    np.asarray(hits, dtype=np.int64))


# -- the graph: one hard position over many lanes -------------------------------------------------------------------------
# Level 0 holds the distinct (row, window) pairs of a call, level j + 1 the distinct children of level j with mirror images
# merged; child[node][col] is the child's index among all nodes, levels concatenated, or -1.  ``split_plies`` and
# ``driver_plies`` both build it, search its last level and the nodes without a child as one batch, and sum nodes and hits
# over each row's distinct last-level nodes.  The folds back to level 0 are two: the split's exact scores by max / min
# (``_graph_fold_exact``), the driver's bounds as intervals (``_graph_fold``), which answer a row, and drop descendants,
# before every descendant is known -- so the two differ, by design, in what an UNKNOWN descendant does to a row.
def _mirror_bits(x):
    """The left-right mirror image of uint64 bitboards (any shape)."""
    out = np.zeros_like(x)
    for c in range(WIDTH):
        out |= ((x >> np.uint64(H1 * c)) & np.uint64((1 << H1) - 1)) << np.uint64(H1 * (WIDTH - 1 - c))
    return out


def _canonical(rows):
    """uint64 [m, 2] rows, each replaced by the smaller of itself and its mirror image (by color0, then color1): the value
    of a position is its mirror image's, so the two are solved once."""
    m = _mirror_bits(rows)
    swap = (m[:, 0] < rows[:, 0]) | ((m[:, 0] == rows[:, 0]) & (m[:, 1] < rows[:, 1]))
    return np.where(swap[:, None], m, rows)


def _unique_rows(rows):
    """(unique uint64 [u, 2], inverse int64 [m]) of uint64 [m, 2]."""
    if len(rows) == 0:
        return rows.reshape(0, 2), np.zeros(0, dtype=np.int64)
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    return uniq, np.asarray(inv, dtype=np.int64).reshape(-1)


def _ages(rows):
    return _popcount64(rows[:, 0] | rows[:, 1]) if len(rows) else np.zeros(0, dtype=np.int64)


def _children_host(rows):
    """c4_solve_children_dev in Python: (children uint64 [m, 7, 2], legal bool [m, 7]) of uint64 [m, 2] rows."""
    children = np.zeros((len(rows), WIDTH, 2), dtype=np.uint64)
    legal = np.zeros((len(rows), WIDTH), dtype=bool)
    for i, (c0, c1) in enumerate(rows):
        c0, c1 = int(c0), int(c1)
        if _classify(c0, c1, DEEP_MAX_EMPTIES) != L.SOLVE_SOLVED:
            continue
        occ = c0 | c1
        o_moves = bin(occ).count("1") % 2 == 0
        for c in range(WIDTH):
            bit = (occ + BOTTOM) & (_COL << (H1 * c))
            if bit:
                children[i, c] = (c0 | bit, c1) if o_moves else (c0, c1 | bit)
                legal[i, c] = True
    return children, legal


def _children_of(device):
    """``_children_host`` on cuda:`device`: c4_solve_children_dev around uint64 [m, 2] rows."""
    def children_of(rows):
        import torch
        children, legal = _children_dev(_packed_on_device(torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)), device))
        return children.cpu().numpy().view(np.uint64).reshape(-1, WIDTH, 2), legal.cpu().numpy() != 0
    return children_of


# -- a whole ply, and the book that keeps it solved -----------------------------------------------------------------------
def _winning_squares_np(p, occ):
    """``_winning_squares`` on uint64 arrays."""
    u = np.uint64
    r = (p << u(1)) & (p << u(2)) & (p << u(3))
    for s in (H1, HEIGHT, H1 + 1):
        q = (p << u(s)) & (p << u(2 * s))
        r |= q & (p << u(3 * s))
        r |= q & (p >> u(s))
        q = (p >> u(s)) & (p >> u(2 * s))
        r |= q & (p << u(s))
        r |= q & (p >> u(3 * s))
    return r & (u(_BOARD) ^ occ)


def _next_ply_host(rows):
    """The undecided children of undecided uint64 [m, 2] rows of one age: ``_children_host``'s, vectorised, without the
    positions the move just won and without the full board."""
    occ = rows[:, 0] | rows[:, 1]
    age = int(_popcount64(occ[:1])[0])
    if age + 1 >= SIZE:
        return np.zeros((0, 2), dtype=np.uint64)
    side = age & 1
    out = []
    for c in range(WIDTH):
        bit = (occ + np.uint64(BOTTOM)) & np.uint64(_COL << (H1 * c))
        ch = rows[bit != 0].copy()
        ch[:, side] |= bit[bit != 0]
        out.append(ch[~_wins_bits(ch[:, side])])
    return np.concatenate(out)


def _next_ply_dev(packed):
    """``_next_ply_host`` on the device: c4_solve_children_dev lists the children, torch drops the won ones, mirrors and
    takes the unique rows.  int64 [m, 2] cuda tensor in and out."""
    import torch
    children, legal = _children_dev(packed)
    ch = children[legal != 0]
    if ch.shape[0] == 0:
        return ch.reshape(0, 2)
    occ = ch[:, 0] | ch[:, 1]
    age = int(_popcount64(np.array([int(occ[0].item())], dtype=np.uint64))[0])
    if age >= SIZE:
        return ch[:0]
    moved = ch[:, (age - 1) & 1]
    won = torch.zeros_like(moved, dtype=torch.bool)
    for s in (1, HEIGHT, H1, H1 + 1):
        y = moved & (moved >> s)
        won |= (y & (y >> (2 * s))) != 0
    ch = ch[~won]
    m = torch.zeros_like(ch)
    for c in range(WIDTH):
        m |= ((ch >> (H1 * c)) & ((1 << H1) - 1)) << (H1 * (WIDTH - 1 - c))
    swap = (m[:, 0] < ch[:, 0]) | ((m[:, 0] == ch[:, 0]) & (m[:, 1] < ch[:, 1]))
    return torch.unique(torch.where(swap[:, None], m, ch), dim=0).contiguous()


def enumerate_ply(plies, unforced=False, device=None):
    """Every undecided position with exactly `plies` stones that legal play reaches from the empty board -- no game goes on
    past a win -- one row per mirror pair (``_canonical``'s choice), uint64 [n, 2] sorted as ``np.unique(axis=0)`` sorts.
    unforced=True keeps the rows where neither the mover nor the opponent has a playable square that completes four: at 8
    plies the 67,557 positions of the UCI connect-4 dataset ("neither player has won yet, and the next move is not forced").
    device=None enumerates in NumPy; a device index lists the children with c4_solve_children_dev and merges on the
    device.  Both give the same rows, bit for bit."""
    if not (float(plies).is_integer() and 0 <= int(plies) <= SIZE):
        raise ValueError("plies must be 0..%d; got %r" % (SIZE, plies))
    rows = np.zeros((1, 2), dtype=np.uint64)
    if device is None:
        for _ in range(int(plies)):
            if len(rows) == 0:
                break
            rows = _unique_rows(_canonical(_next_ply_host(rows)))[0]
    else:
        import torch
        t = _packed_on_device(torch.from_numpy(rows.view(np.int64)), device)
        with torch.cuda.device(t.device):
            for _ in range(int(plies)):
                if t.shape[0] == 0:
                    break
                t = _next_ply_dev(t)
        rows = np.ascontiguousarray(t.cpu().numpy().view(np.uint64).reshape(-1, 2))
    if int(plies) == SIZE:
        rows = rows[:0]
    if unforced and len(rows):
        occ = rows[:, 0] | rows[:, 1]
        playable = (occ + np.uint64(BOTTOM)) & np.uint64(_BOARD)
        rows = rows[((_winning_squares_np(rows[:, 0], occ) | _winning_squares_np(rows[:, 1], occ)) & playable) == 0]
    return np.ascontiguousarray(rows)


def _book_keys(rows):
    """The book's key of uint64 [n, 2] rows: the smaller of ``mine + occ + BOTTOM`` and its mirror image's."""
    occ = rows[:, 0] | rows[:, 1]
    mine = np.where((_popcount64(occ) & 1) == 1, rows[:, 1], rows[:, 0])
    key = mine + occ + np.uint64(BOTTOM)
    return np.minimum(key, _mirror_key(key))


def _interior_rows(rows):
    """bool [n]: the undecided uint64 [n, 2] rows the search enters as interior nodes under the full window -- the mover
    cannot win at once, and enter_node finds a move that does not lose at once.  Only these are ever probed: every other
    position is answered by the node that meets it."""
    occ = rows[:, 0] | rows[:, 1]
    odd = (_popcount64(occ) & 1) == 1
    mine, theirs = np.where(odd, rows[:, 1], rows[:, 0]), np.where(odd, rows[:, 0], rows[:, 1])
    possible = (occ + np.uint64(BOTTOM)) & np.uint64(_BOARD)
    at_once = (_winning_squares_np(mine, occ) & possible) != 0
    opp_win = _winning_squares_np(theirs, occ)
    forced = possible & opp_win
    two = (forced & (forced - np.uint64(1))) != 0
    left = np.where(forced != 0, forced, possible) & ~(opp_win >> np.uint64(1))
    return ~at_once & ~two & (left != 0) & (_popcount64(occ) < SIZE - 1)


def _merge_words(words):
    """Sorted entry words with one entry a key: an exact entry before a lower bound before an upper bound, the tighter of
    two bounds of a kind."""
    words = np.asarray(words, dtype=np.uint64).reshape(-1)
    if len(words) == 0:
        return words
    key = words & np.uint64(_TT_KEY_MASK)
    score = ((words >> np.uint64(_TT_SCORE_SHIFT)) & np.uint64(0x7f)).astype(np.int64) - 64
    kind = ((words >> np.uint64(_TT_KIND_SHIFT)) & np.uint64(3)).astype(np.int64)
    prio = np.where(kind == _EXACT, 3 << 8, np.where(kind == _LOWER, (2 << 8) + score + 64, (1 << 8) + 64 - score))
    order = np.lexsort((-prio, key))
    first = np.ones(len(order), dtype=bool)
    first[1:] = key[order][1:] != key[order][:-1]
    return np.ascontiguousarray(words[order][first])


class Book:
    """One ply solved once: a sorted ``uint64`` array of table-format entries (``entry_fields``' layout: key in bits 0..48,
    score + 64 in bits 49..55, kind 1..3 in bits 56..57), every key of a position with `age` stones.  The key is the
    canonical one of a mirror pair, the smaller of ``mine + occ + BOTTOM`` and that key with its seven column fields
    reversed, so one entry serves both images and no board is mirrored.  Every entry is a true bound of its position's
    value -- the invariant a ``Table``'s entries obey -- so a book never changes an answer, whatever windows found its
    entries and however many positions it lacks: a missing entry means the search goes on.

    ``book=`` of ``solve`` / ``solve_window`` / ``outcomes`` / ``grid_triple`` / ``label`` / ``label_values`` probes it on
    the device wherever a search reaches the book's ply (c4_solve_book_create; the image is built on first use and freed
    by ``close()``); ``solve_host`` / ``drive_host`` probe the same object in Python (``get``).  `unknown`: uint64 [k, 2]
    rows still to be solved, kept with the entries by ``save`` so that a later sitting goes on with them.

    Raises ValueError unless the keys are sorted, unique, canonical and well formed for `age`, every kind is 1..3 and
    every score within +-42."""

    def __init__(self, age, words, unknown=None):
        if not (float(age).is_integer() and 0 <= int(age) <= SIZE - 1):
            raise ValueError("age %r outside 0..%d" % (age, SIZE - 1))
        self.age = int(age)
        self.words = np.ascontiguousarray(np.asarray(words, dtype=np.uint64).reshape(-1))
        self.unknown = np.zeros((0, 2), dtype=np.uint64) if unknown is None else np.ascontiguousarray(unknown, dtype=np.uint64).reshape(-1, 2)
        self._entries = None
        self._dev = {}
        w = self.words
        if (w >> np.uint64(_TT_KIND_SHIFT + 2)).any():
            raise ValueError("an entry has bits above the kind")
        f = entry_fields(w)
        if len(f.key) != len(w) or (f.kind == 0).any():
            raise ValueError("every entry has a kind in 1..3")
        if (np.abs(f.score) > SCORE_MAX).any():
            raise ValueError("a score lies outside +-%d" % SCORE_MAX)
        if (f.key[1:] <= f.key[:-1]).any():
            raise ValueError("the keys are not sorted and unique")
        if (f.mine + f.occ + np.uint64(BOTTOM) != f.key).any() or (f.mine & ~f.occ).any() or (f.occ & ~np.uint64(_BOARD)).any() or (f.age != self.age).any():
            raise ValueError("a key is not the key of a position with %d stones" % self.age)
        if (_mirror_key(f.key) < f.key).any():
            raise ValueError("a key is not the canonical one of its mirror pair")

    def __len__(self):
        return len(self.words)

    @property
    def keys(self):
        return self.words & np.uint64(_TT_KEY_MASK)

    @classmethod
    def empty(cls, age):
        return cls(age, np.zeros(0, dtype=np.uint64))

    @classmethod
    def from_answers(cls, rows, answers, age=None):
        """The book of uint64 [n, 2] `rows` (Boards or pairs) of one age and their `answers`: a ``Windowed``
        (``solve_window``: an exact score becomes an exact entry, a fail-high a lower bound, a fail-low an upper bound) or
        a ``Solved`` (``solve``: exact entries).  Only SOLVED rows give entries; UNKNOWN rows go to ``unknown``; rows of
        any other status are left out, and so are the rows the search never looks up (``_interior_rows``: the node that
        meets them answers them).  Mirror images give one entry.  age: needed only where there are no rows."""
        rows = _rows_u64(rows)
        ages = _ages(rows)
        if len(rows) == 0 and age is None:
            raise ValueError("no rows: give the age")
        age = int(ages[0]) if age is None else int(age)
        if (ages != age).any():
            raise ValueError("a book holds one ply: the rows have %s stones" % sorted(set(ages.tolist())))
        status = np.asarray(answers.status)
        if hasattr(answers, "bound"):
            score, kind = np.asarray(answers.score, dtype=np.int64), np.asarray(answers.bound, dtype=np.int64)
        else:
            out = np.nan_to_num(np.asarray(answers.outcome, dtype=np.float64), nan=0.5)
            s = np.where(out == 0.5, 0, np.where(out == 1.0, 1, -1) * (43 - np.asarray(answers.final_age, dtype=np.int64)))
            score, kind = np.where(ages & 1, -s, s), np.full(len(rows), _EXACT, dtype=np.int64)
        ok = (status == L.SOLVE_SOLVED) & (kind != L.SOLVE_BOUND_NONE) & _interior_rows(rows)
        words = _book_keys(rows[ok]) | ((score[ok] + 64).astype(np.uint64) << np.uint64(_TT_SCORE_SHIFT)) | (kind[ok].astype(np.uint64) << np.uint64(_TT_KIND_SHIFT))
        return cls(age, _merge_words(words), rows[status == L.SOLVE_UNKNOWN])._without_known()

    def _without_known(self):
        """The unknown rows that have no entry yet, one a mirror pair."""
        u = _unique_rows(_canonical(self.unknown))[0] if len(self.unknown) else self.unknown
        self.unknown = np.ascontiguousarray(u[~np.isin(_book_keys(u), self.keys)]) if len(u) else u
        return self

    def merge(self, other):
        """A book with the entries of both (``_merge_words`` where both have a key) and the rows neither has solved."""
        if other.age != self.age:
            raise ValueError("books of %d and %d stones do not merge" % (self.age, other.age))
        return Book(self.age, _merge_words(np.concatenate([self.words, other.words])), np.concatenate([self.unknown, other.unknown]))._without_known()

    def save(self, path):
        """One ``.npz``: age, words, unknown."""
        with open(path, "wb") as f:
            np.savez_compressed(f, age=np.int64(self.age), words=self.words, unknown=self.unknown)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(int(z["age"]), z["words"], z["unknown"])

    # probed in Python
    def get(self, key, default=None):
        """``(kind, score)`` of the position with the key ``mine + occ + BOTTOM``, or of its mirror image."""
        if self._entries is None:
            f = entry_fields(self.words)
            self._entries = dict(zip(f.key.tolist(), zip(f.kind.tolist(), f.score.tolist())))
        return self._entries.get(min(key, _mirror_key(key)), default)

    # probed on the device
    def handle(self, device=0):
        """The c4_solve_book of this book on cuda:`device`, created on first use."""
        if int(device) not in self._dev:
            h = C.c_void_p()
            _check(L.load().c4_solve_book_create(int(device), _ptr(self.words), len(self.words), self.age, C.byref(h)))
            self._dev[int(device)] = h
        return self._dev[int(device)]

    def close(self):
        """Free the device images.  No ``Table`` may still have the book attached."""
        while self._dev:
            L.load().c4_solve_book_destroy(self._dev.popitem()[1])

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


HostBook = Book     # probed in Python it is the same object: solve_host(book=), drive_host(book=)


@contextlib.contextmanager
def _carrying(table, book, device):
    """The ``Table`` a device call passes so that it probes `book`: `table` with the book attached for the duration, or
    without a table an entryless handle (the table-free search) that lives as long.  The attachment is a property of the
    handle: calls that pass different books through one ``Table`` must not overlap (give each thread its own ``Table`` or
    attach once with ``Table.attach_book``)."""
    own = table is None
    t = Table.entryless(device) if own else table
    before = t.book
    t.attach_book(book)
    try:
        yield t
    finally:
        if own:
            t.close()
        else:
            t.attach_book(before)       # what the caller had attached stays attached


Graph = namedtuple("Graph", "color0 color1 level_start child alpha beta inverse")


def _build_graph(rows, alpha, beta, plies, children_of):
    """The graph `plies` deep below uint64 [n, 2] `rows` with windows int8 [n] (or both None: the full window): ``Graph`` of
    color0, color1 uint64 [n_nodes], level_start int64 [plies + 2], child int32 [n_nodes, 7], alpha, beta int8 [n_0] (level
    0's windows) and inverse int64 [n]: level-0 node ``inverse[i]`` is row i with its window.  children_of: ``_children_host``
    or ``_children_of(device)``."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
    n = len(rows)
    a = np.full(n, -SCORE_MAX, dtype=np.int64) if alpha is None else np.asarray(alpha, dtype=np.int64)
    b = np.full(n, SCORE_MAX, dtype=np.int64) if beta is None else np.asarray(beta, dtype=np.int64)
    keyed = np.concatenate([rows, (a + 64).astype(np.uint64)[:, None], (b + 64).astype(np.uint64)[:, None]], axis=1)
    if n:
        uniq, inverse = np.unique(keyed, axis=0, return_inverse=True)
        inverse = np.asarray(inverse, dtype=np.int64).reshape(-1)
    else:
        uniq, inverse = keyed, np.zeros(0, dtype=np.int64)
    levels, links = [np.ascontiguousarray(uniq[:, :2])], []
    for _ in range(plies):
        ch, lg = children_of(levels[-1])
        ch, lg = np.asarray(ch, dtype=np.uint64), np.asarray(lg).astype(bool)
        nxt, inv = _unique_rows(_canonical(ch[lg]))
        link = np.full(lg.shape, -1, dtype=np.int64)
        link[lg] = inv
        levels.append(nxt)
        links.append(link)
    start = np.concatenate([[0], np.cumsum([len(lv) for lv in levels])]).astype(np.int64)
    child = np.full((int(start[-1]), WIDTH), -1, dtype=np.int32)
    for j, link in enumerate(links):
        child[start[j]:start[j + 1]] = np.where(link >= 0, link + start[j + 1], -1)
    nodes = np.concatenate(levels)
    return Graph(np.ascontiguousarray(nodes[:, 0]), np.ascontiguousarray(nodes[:, 1]), start, child,
                 (uniq[:, 2].astype(np.int64) - 64).astype(np.int8), (uniq[:, 3].astype(np.int64) - 64).astype(np.int8), inverse)


def _graph_root_sums(g, *per_node):
    """int64 [n_0] for each of `per_node` (int64 [n_nodes], read on the last level): its sum over each level-0 row's distinct
    last-level nodes.  The walk keeps (row, leaf) pairs sorted by row and lifts them one level at a time: a row's leaves are
    its children's, each once."""
    first_leaf = int(g.level_start[-2])
    p_row = p_leaf = np.arange(len(g.child) - first_leaf)
    for j in range(len(g.level_start) - 3, -1, -1):
        s, e, n_next = int(g.level_start[j]), int(g.level_start[j + 1]), int(g.level_start[j + 2] - g.level_start[j + 1])
        r, c = np.nonzero(g.child[s:e] >= 0)
        ch = g.child[s:e][r, c].astype(np.int64) - e
        start = np.searchsorted(p_row, np.arange(n_next))
        reps = np.bincount(p_row, minlength=n_next)[ch]
        offs = np.arange(int(reps.sum())) - np.repeat(np.cumsum(reps) - reps, reps)
        pairs = np.stack([np.repeat(r, reps), p_leaf[np.repeat(start[ch], reps) + offs]], axis=1)
        pairs = np.unique(pairs, axis=0) if len(pairs) else pairs.reshape(0, 2)
        p_row, p_leaf = pairs[:, 0], pairs[:, 1]
    weights = (np.asarray(a, dtype=np.int64)[first_leaf:][p_leaf] for a in per_node)
    return tuple(np.bincount(p_row, weights=w, minlength=int(g.level_start[1])).astype(np.int64) for w in weights)


# -- the split: exact answers folded by max / min -------------------------------------------------------------------------
def _abs_score(outcome_code, age):
    """The integer score from o's side (43 - age, age - 43, 0) of answers given as C4_RESULT_* and final age."""
    outcome_code = np.asarray(outcome_code, dtype=np.int64)
    age = np.asarray(age, dtype=np.int64)
    return np.where(outcome_code == L.RESULT_OWIN, 43 - age, np.where(outcome_code == L.RESULT_XWIN, age - 43, 0))


def _graph_fold_exact(g, status, outcome, final_age, nodes, hits):
    """The host half of ``split_plies``: level 0's (status, outcome code, final_age int8, nodes, hits int64) from the exact
    answers of the searched nodes -- those without a child, and the last level -- as arrays of one entry a node, read nowhere
    else.  The rule of grid_search.py:21-32 on the integer score, the level above the last one first: a node with children is
    SOLVED with the max (o to move) or min (x to move) of its children's scores if every child has an answer (is SOLVED or
    TERMINAL), else UNKNOWN; a node without children answers for itself.  Unlike ``_graph_fold`` no node is answered by a
    bound: one UNKNOWN descendant leaves a row UNKNOWN.  nodes and hits are ``_graph_root_sums``."""
    status = np.array(status, dtype=np.int8)
    score = _abs_score(outcome, final_age)
    known = (status == L.SOLVE_SOLVED) | (status == L.SOLVE_TERMINAL)
    o_moves = (_popcount64(g.color0 | g.color1) & 1) == 0
    for j in range(len(g.level_start) - 3, -1, -1):
        s, e = int(g.level_start[j]), int(g.level_start[j + 1])
        has = g.child[s:e] >= 0
        inner = has.any(axis=1)
        at = np.where(has, g.child[s:e], 0)
        best = np.where(o_moves[s:e], np.where(has, score[at], -99).max(axis=1), np.where(has, score[at], 99).min(axis=1))
        all_known = (known[at] | ~has).all(axis=1)
        score[s:e] = np.where(inner, best, score[s:e])
        known[s:e] = np.where(inner, all_known, known[s:e])
        status[s:e] = np.where(inner, np.where(all_known, L.SOLVE_SOLVED, L.SOLVE_UNKNOWN), status[s:e])
    n0 = int(g.level_start[1])
    status, score, known = status[:n0], score[:n0], known[:n0]
    out_code = np.where(known, np.where(score > 0, L.RESULT_OWIN, np.where(score < 0, L.RESULT_XWIN, L.RESULT_DRAW)), -1).astype(np.int8)
    out_age = np.where(known, np.where(score != 0, 43 - np.abs(score), SIZE), -1).astype(np.int8)
    return (status, out_code, out_age) + _graph_root_sums(g, nodes, hits)


def _solve_split(packed, split_plies, node_budget, nodes_per_launch, table):
    import torch
    g = _build_graph(_rows_u64(packed), None, None, split_plies, _children_of(packed.device.index))
    # one batch, in the order of the nodes: the last level, and above it the nodes without a child (they answer for
    # themselves and cost no node)
    searched = ~(g.child >= 0).any(axis=1)
    searched[int(g.level_start[-2]):] = True
    batch = torch.from_numpy(np.stack([g.color0[searched], g.color1[searched]], axis=1).view(np.int64)).to(packed.device).contiguous()
    answers = []
    for t in _solve_dev(batch, node_budget, nodes_per_launch, table, deep=True):
        a = t.cpu().numpy()
        answers.append(np.full(len(searched), -1, dtype=a.dtype))
        answers[-1][searched] = a
    return _finish(*(a[g.inverse] for a in _graph_fold_exact(g, *answers)))


def solve(boards, node_budget=None, nodes_per_launch=None, device=0, table=None, deep=False, split_plies=0, book=None):
    """Solve every row on the GPU.  `boards`: a sequence of Boards (host arrays through c4_solve) or a packed int64 [n, 2]
    tensor (c4_solve_dev; a CPU tensor is moved to cuda:`device`).  Returns ``Solved`` of NumPy arrays:

      status     int8, _lib.SOLVE_* (STATUS_NAMES)
      outcome    float64 0.0 / 0.5 / 1.0, absolute like ``Result``; NaN where the status has no answer
      final_age  int8, the age at which best play ends the game; -1 where unknown
      value      float64, what ``GridSearch(plies=empties)`` computes for the node (grid_search.py:43-71); NaN where unknown
      nodes      int64, positions the search entered
      table_hits int64, table probes that returned a stored score or narrowed the window (zeros without a table)

    node_budget: most nodes of one row, beyond it the row is UNKNOWN (default 2^26); nodes_per_launch: the quota of one
    kernel launch (default 2^14) -- it changes neither answers nor, without a table, node counts.

    deep=True: c4_solve_deep's search, which reaches every position (no TOO_DEEP); table-free it enters the nodes the
    default search enters.  table: a ``Table`` (implies deep, and the table's device) shared by all rows and by every other
    call it is passed to; the answers stay exact and the same, the node counts fall and are no longer deterministic.
    split_plies=k (implies deep): every row is expanded k plies (c4_solve_children_dev), the distinct descendants -- mirror
    images merged -- are solved as rows of one batch, so one hard position occupies many lanes and they share the table,
    and the answers are folded back by max / min over the integer score; a row is UNKNOWN if any of its descendants is, and
    its nodes and table_hits are the sums over its distinct descendants (so node_budget bounds each descendant).
    book: a ``Book`` (implies deep): the search probes it wherever it reaches the book's ply, with or without a table; the
    answers stay the same, the node counts fall -- table-free they stay deterministic -- and a book hit counts into
    table_hits.  With a `table` the book is attached to that handle for the duration of the call (what
    ``Table.attach_book`` had attached comes back afterwards), so calls that pass different books through one ``Table``
    must not overlap: give each thread its own ``Table``."""
    if book is not None:
        with _carrying(table, book, device) as carrier:
            return solve(boards, node_budget, nodes_per_launch, device, carrier, True, split_plies)
    deep = bool(deep or table is not None or split_plies)
    if table is not None:
        device = table.device
    if split_plies:
        if not 0 < int(split_plies) <= 8:
            raise ValueError("split_plies must be 0..8")
        if not _is_tensor(boards) and len(boards) == 0:
            return _finish(*(np.zeros(0, dtype=np.int8),) * 3, np.zeros(0, dtype=np.int64))
        return _solve_split(_packed_on_device(boards, device), int(split_plies), node_budget, nodes_per_launch, table)
    return _finish(*_solve_any(boards, node_budget, nodes_per_launch, device, table, deep))


# -- the deep search from a root window per row --------------------------------------------------------------------------
def _window_arrays(alpha, beta, n):
    """int8 [n] arrays of a scalar or per-row window, checked row by row; (None, None) for the full window."""
    if alpha is None and beta is None:
        return None, None
    if alpha is None or beta is None:
        raise ValueError("alpha and beta are given together, or both are None")
    a = np.broadcast_to(np.asarray(alpha), (n,)) if np.ndim(alpha) == 0 else np.asarray(alpha)
    b = np.broadcast_to(np.asarray(beta), (n,)) if np.ndim(beta) == 0 else np.asarray(beta)
    if a.shape != (n,) or b.shape != (n,):
        raise ValueError("alpha and beta are scalars or arrays of one entry per row (%d); got %s and %s" % (n, a.shape, b.shape))
    bad = np.nonzero(~((a == np.floor(a)) & (b == np.floor(b)) & (a >= -SCORE_MAX) & (a < b) & (b <= SCORE_MAX)))[0]
    if len(bad):
        raise ValueError("row %d: the window (%r, %r) is not -%d <= alpha < beta <= %d in whole numbers" % (
            bad[0], a[bad[0]].item(), b[bad[0]].item(), SCORE_MAX, SCORE_MAX))
    return np.ascontiguousarray(a, dtype=np.int8), np.ascontiguousarray(b, dtype=np.int8)


def solve_window(boards, alpha, beta, node_budget=None, nodes_per_launch=None, device=0, table=None, driver_plies=0, host=False, book=None):
    """The deep search (``solve(deep=True)``: every position, optionally a ``Table``) from a root window per row.  alpha, beta:
    scalars or per-row arrays on the mover's score (43 - final age for a win, final age - 43 for a loss, 0 for a draw),
    -42 <= alpha < beta <= 42; both None: the full window.  `boards` as ``solve`` takes them.  Returns ``Windowed`` of arrays:

      status     int8, _lib.SOLVE_* -- ``solve``'s, never TOO_DEEP
      score      int8, the mover's score as the root returns it (0 where the row has no answer)
      bound      int8, _lib.SOLVE_BOUND_* (BOUND_NAMES): EXACT where alpha < score < beta -- the score is the position's;
                 LOWER where score >= beta, UPPER where score <= alpha -- a true bound of that kind, possibly beyond the
                 window (an immediate win answers 42 - age whatever was asked); NONE where the row was not searched to the end
      outcome    float64 0.0 / 0.5 / 1.0 where the bound is exact and for finished positions, else NaN
      final_age  int8, likewise, else -1
      nodes, table_hits  as ``solve``

    A narrower window never costs a table-free search more nodes than one that contains it; (-1, 1) answers who wins,
    (v - 1, v) whether the mover's score reaches v.

    driver_plies=k (1..8): the root driver.  Every row is expanded k plies, the distinct descendants -- mirror images merged
    -- are searched as rows of one batch from windows derived from the row's, and their bounds are folded back as intervals
    (c4_solve_graph): a row is answered as soon as the interval decides its window, an unfinished descendant leaves it
    UNKNOWN only where the proof needs it, and descendants no open row can still use are dropped between launches.  The kind
    is the undriven call's wherever both answer, and so is the score where it is EXACT; a bound's score may differ, and nodes
    and table_hits are the sums over the row's distinct descendants (node_budget bounds each).  A call is cut into graphs
    whose last level has at most 2^20 positions; a single row with more distinct descendants than that -- an early position
    with driver_plies of 7 or 8 -- raises ValueError: give fewer plies.  host=True (with driver_plies)
    computes the same with ``drive_host``: no GPU, no table.  book: ``solve``'s, on the device and with host=True."""
    if book is not None and not host:
        with _carrying(table, book, device) as carrier:
            return solve_window(boards, alpha, beta, node_budget, nodes_per_launch, device, carrier, driver_plies)
    if table is not None and not host:
        device = table.device
    n = int(boards.shape[0]) if _is_tensor(boards) else len(boards)
    a, b = _window_arrays(alpha, beta, n)
    if driver_plies:
        if host and table is not None:
            raise ValueError("host=True drives table-free")
        return _drive(_rows_u64(boards), a, b, driver_plies, node_budget, nodes_per_launch, device, table, host, book=book)
    if host:
        raise ValueError("host=True belongs to driver_plies; solve_host answers single positions")
    return _finish_window(*_solve_any(boards, node_budget, nodes_per_launch, device, table, True, (a, b)))


def outcomes(boards, node_budget=None, nodes_per_launch=None, device=0, table=None, driver_plies=0, host=False, book=None):
    """Who wins each position: float64 0.0 (x) / 0.5 (draw) / 1.0 (o), NaN where the budget leaves a row unknown or the row is
    invalid; a finished position answers with its own result.  One search per row with the window (-1, +1), the narrowest
    that separates win, draw and loss -- how fast is not asked, and not paid for.  driver_plies, host: ``solve_window``'s."""
    res = solve_window(boards, -1, 1, node_budget, nodes_per_launch, device, table, driver_plies, host, book)
    sign = np.sign(res.score.astype(np.int64))
    absolute = np.where(_ages(_rows_u64(boards)) & 1, -sign, sign)
    return np.where(res.status == L.SOLVE_SOLVED, (absolute + 1) * 0.5, np.where(res.status == L.SOLVE_TERMINAL, res.outcome, np.nan))


# -- the root driver: intervals folded by alpha-beta over the same graph ----------------------------------------------------
# DESIGN.md section 3.13 has the rules (static windows, leaf intervals, fold up, answer, mark down) and why they are sound;
# the functions below are those rules on the ``Graph``'s flat NumPy arrays, c4_solve_graph's kernels are the same rules one
# lane per node.
NODE_INTERIOR, NODE_SELF, NODE_ANSWERED, NODE_OVER_BUDGET, NODE_DROPPED = (L.SOLVE_NODE_INTERIOR, L.SOLVE_NODE_SELF, L.SOLVE_NODE_ANSWERED,
                                                                           L.SOLVE_NODE_OVER_BUDGET, L.SOLVE_NODE_DROPPED)
_NODE_PENDING = L.SOLVE_NODE_PENDING        # a leaf between launches; no report that is returned holds it
NODE_STATE_NAMES = {NODE_INTERIOR: "interior", NODE_SELF: "self_answering", NODE_ANSWERED: "answered", NODE_OVER_BUDGET: "over_budget",
                    NODE_DROPPED: "dropped"}
GRAPH_MAX_LEAVES = 1 << 20      # the last level of one graph (c4_solve.hip CHUNK_ROWS)


def _graph_windows(g):
    """The static windows of every node, int64 [n_nodes] each: level 0 has the caller's, a child of (a, b) gets (-b, -a), a
    node with several parents the union."""
    n0 = int(g.level_start[1])
    wa = np.full(len(g.child), SCORE_MAX, dtype=np.int64)
    wb = np.full(len(g.child), -SCORE_MAX, dtype=np.int64)
    wa[:n0], wb[:n0] = g.alpha, g.beta
    for j in range(len(g.level_start) - 2):
        lo, hi = int(g.level_start[j]), int(g.level_start[j + 1])
        r, c = np.nonzero(g.child[lo:hi] >= 0)
        at = g.child[lo:hi][r, c]
        np.minimum.at(wa, at, -wb[lo + r])
        np.maximum.at(wb, at, -wa[lo + r])
    return wa, wb


def _graph_fold(g, lo, hi):
    """Fold up in place, the level above the last one first: lo = max over children of -hi_c, hi = max of -lo_c."""
    for j in range(len(g.level_start) - 3, -1, -1):
        s, e = int(g.level_start[j]), int(g.level_start[j + 1])
        ch = g.child[s:e]
        has = ch >= 0
        at = np.where(has, ch, 0)
        f_lo = np.where(has, -hi[at], -99).max(axis=1) if e > s else np.zeros(0, dtype=np.int64)
        f_hi = np.where(has, -lo[at], -99).max(axis=1) if e > s else np.zeros(0, dtype=np.int64)
        inner = has.any(axis=1)
        lo[s:e] = np.where(inner, f_lo, lo[s:e])
        hi[s:e] = np.where(inner, f_hi, hi[s:e])


def _graph_decided(lo, hi, a, b):
    return (lo == hi) | (lo >= b) | (hi <= a)


def _graph_mark(g, lo, hi, wa, wb):
    """Mark down: bool [n_nodes], the nodes some undecided level-0 row still needs."""
    inner = (g.child >= 0).any(axis=1)
    needed = np.zeros(len(g.child), dtype=bool)
    n0 = int(g.level_start[1])
    needed[:n0] = inner[:n0] & ~_graph_decided(lo[:n0], hi[:n0], wa[:n0], wb[:n0])
    for j in range(len(g.level_start) - 2):
        s, e = int(g.level_start[j]), int(g.level_start[j + 1])
        is_open = needed[s:e] & inner[s:e] & ~_graph_decided(lo[s:e], hi[s:e], wa[s:e], wb[s:e])
        raised = np.maximum(wa[s:e], lo[s:e])
        ch = g.child[s:e]
        at = np.where(ch >= 0, ch, 0)
        want = (ch >= 0) & is_open[:, None] & (lo[at] < hi[at]) & (-lo[at] > raised[:, None])
        needed[at[want]] = True
    return needed


def _mover_score_of_finished(c0, c1):
    """The score for the side to move of a finished position: it has lost, or the board is full."""
    age = bin(c0 | c1).count("1")
    return age - 43 if (_wins(c0) or _wins(c1)) else 0


def _graph_root_answers(g, lo, hi, wa, wb):
    """The answers of level 0 from its intervals: (status, score, bound, outcome code, final_age) int8 [n_0]."""
    n0 = int(g.level_start[1])
    status, score, bound = (np.zeros(n0, dtype=np.int8) for _ in range(3))
    outcome, final_age = (np.full(n0, -1, dtype=np.int8) for _ in range(2))
    for i in range(n0):
        c0, c1 = int(g.color0[i]), int(g.color1[i])
        st = _classify(c0, c1, DEEP_MAX_EMPTIES)
        status[i] = st
        if st == L.SOLVE_TERMINAL:
            outcome[i] = L.RESULT_OWIN if _wins(c0) else L.RESULT_XWIN if _wins(c1) else L.RESULT_DRAW
            final_age[i] = bin(c0 | c1).count("1")
        if st != L.SOLVE_SOLVED:
            continue
        l, h, a, b = int(lo[i]), int(hi[i]), int(wa[i]), int(wb[i])
        if l == h:
            score[i], bound[i] = l, _bound_kind(l, a, b)
        elif l >= b:
            score[i], bound[i] = l, L.SOLVE_BOUND_LOWER
        elif h <= a:
            score[i], bound[i] = h, L.SOLVE_BOUND_UPPER
        else:
            status[i] = L.SOLVE_UNKNOWN
            continue
        if bound[i] == L.SOLVE_BOUND_EXACT:
            s = -int(score[i]) if bin(c0 | c1).count("1") & 1 else int(score[i])
            outcome[i] = L.RESULT_OWIN if s > 0 else L.RESULT_XWIN if s < 0 else L.RESULT_DRAW
            final_age[i] = 43 - abs(s) if s else SIZE
    return status, score, bound, outcome, final_age


def _host_leaf(c0, c1, alpha, beta, node_budget, book=None):
    """drive_host's default leaf_solver, ``solve_host(window=)`` table-free: (status, score, bound, nodes, clean) and, with a
    sixth entry, the node counts at which the search hit the `book` (``_Search.hit_at``; empty without one).  clean: no
    node of the search returned without a cut-off after the last one was entered -- the lane is done in the launch that
    enters its last node even where that node uses up the launch's quota (run_lane closes a node whose moves are used up
    only while quota is left)."""
    st = _classify(c0, c1, DEEP_MAX_EMPTIES)
    if st != L.SOLVE_SOLVED:
        return st, 0, L.SOLVE_BOUND_NONE, 0, True, []
    occ = c0 | c1
    age = bin(occ).count("1")
    mine, theirs = (c1, c0) if age & 1 else (c0, c1)
    if _winning_squares(mine, occ) & (occ + BOTTOM):
        return st, 42 - age, _bound_kind(42 - age, alpha, beta), 1, True, []
    s = _Search(node_budget, None, book)
    try:
        score = s.node(mine, theirs, age, alpha, beta)
    except _OverBudget:
        return L.SOLVE_UNKNOWN, 0, L.SOLVE_BOUND_NONE, s.nodes, False, s.hit_at
    return st, score, _bound_kind(score, alpha, beta), s.nodes, s.clean, s.hit_at


def _interval(score, bound):
    return {L.SOLVE_BOUND_EXACT: (score, score), L.SOLVE_BOUND_LOWER: (score, SCORE_MAX),
            L.SOLVE_BOUND_UPPER: (-SCORE_MAX, score)}.get(bound, (-SCORE_MAX, SCORE_MAX))


def _check_driver_plies(driver_plies):
    if not (float(driver_plies).is_integer() and 1 <= int(driver_plies) <= 8):
        raise ValueError("driver_plies must be 1..8; got %r" % (driver_plies,))
    return int(driver_plies)


def _budgets(node_budget, nodes_per_launch):
    budget = DEFAULT_NODE_BUDGET if not node_budget else int(node_budget)
    quota = L.SOLVE_DEFAULT_NODES_PER_LAUNCH if not nodes_per_launch else int(nodes_per_launch)
    if budget < 0 or quota < 0:
        raise ValueError("node_budget and nodes_per_launch must not be negative")
    return budget, quota


def drive_graph_host(g, node_budget=None, nodes_per_launch=None, leaf_solver=_host_leaf, given=None):
    """``drive_host`` on a ``Graph``: (status, score, bound, outcome code, final_age, nodes, table_hits) of level 0 and the
    per-node report.  given: {node: (score, bound)} -- leaves answered from the start whatever the budget (a test's way to
    hand dropped leaves their true answers)."""
    budget, quota = _budgets(node_budget, nodes_per_launch)
    n_nodes = len(g.child)
    first_leaf = int(g.level_start[-2])
    wa, wb = _graph_windows(g)
    inner = (g.child >= 0).any(axis=1)
    lo = np.full(n_nodes, -SCORE_MAX, dtype=np.int64)
    hi = np.full(n_nodes, SCORE_MAX, dtype=np.int64)
    state = np.where(inner, NODE_INTERIOR, _NODE_PENDING).astype(np.int8)
    count = np.zeros(n_nodes, dtype=np.int64)
    full = {}       # node -> the leaf's whole search under the budget, computed when the leaf first takes part in a launch

    def leaf(i, cap):       # (status, score, bound, nodes, clean, hit_at); a leaf_solver may leave the last one out
        ans = tuple(leaf_solver(int(g.color0[i]), int(g.color1[i]), int(wa[i]), int(wb[i]), cap))
        return ans if len(ans) > 5 else ans + ((),)

    def answer(i, score, bound):
        lo[i], hi[i] = _interval(score, bound)
        state[i] = NODE_ANSWERED

    # before launch 1: what k_solve_init answers
    for i in np.nonzero(~inner)[0]:
        c0, c1 = int(g.color0[i]), int(g.color1[i])
        st = _classify(c0, c1, DEEP_MAX_EMPTIES)
        if st != L.SOLVE_SOLVED or i < first_leaf:
            state[i] = NODE_SELF
            if st == L.SOLVE_TERMINAL:
                lo[i] = hi[i] = _mover_score_of_finished(c0, c1)
            continue
        count[i] = 1
        if given is not None and int(i) in given:
            answer(i, *given[int(i)])
            continue
        st, score, bound, nodes, _, _ = leaf(i, 1)
        if st == L.SOLVE_SOLVED:
            answer(i, score, bound)
        elif budget <= 1:
            state[i] = NODE_OVER_BUDGET
    history = []

    def fold_mark_filter():
        _graph_fold(g, lo, hi)
        needed = _graph_mark(g, lo, hi, wa, wb)
        history.append(needed)
        state[(state == _NODE_PENDING) & ~needed] = NODE_DROPPED

    fold_mark_filter()
    launches = 0
    while (state == _NODE_PENDING).any():
        launches += 1
        for i in np.nonzero(state == _NODE_PENDING)[0]:
            if int(i) not in full:
                full[int(i)] = leaf(i, budget)
            st, score, bound, nodes, clean, _ = full[int(i)]
            step = min(budget - int(count[i]), quota)
            reach = int(count[i]) + step
            if st == L.SOLVE_SOLVED and nodes <= reach:
                count[i] = nodes
                if nodes < reach or clean:
                    answer(i, score, bound)
                    continue
            else:
                count[i] = reach
            if count[i] >= budget:
                state[i] = NODE_OVER_BUDGET
        fold_mark_filter()
    status, score, bound, outcome, final_age = _graph_root_answers(g, lo, hi, wa, wb)
    # the hits among the nodes a leaf entered: those its search made up to that node count
    hits = np.zeros(n_nodes, dtype=np.int64)
    for i in np.nonzero(count > 0)[0]:
        if given is not None and int(i) in given:
            continue
        hit_at = (full[int(i)] if int(i) in full else leaf(i, 1))[5]
        hits[i] = int((np.asarray(hit_at, dtype=np.int64) <= count[i]).sum())
    report = {"lo": lo.astype(np.int8), "hi": hi.astype(np.int8), "state": state, "nodes": count, "table_hits": hits,
              "alpha": wa.astype(np.int8), "beta": wb.astype(np.int8), "launches": launches, "needed": history, "graph": g}
    return (status, score, bound, outcome, final_age) + _graph_root_sums(g, count, hits), report


def _finish_graph(parts):
    """``Windowed`` of a call's rows from [(Graph, level 0's answers)], one pair for each run of rows in turn: a row's answer
    is its level-0 node's."""
    status, score, bound, outcome, final_age, nodes, hits = (
        np.concatenate(col) for col in zip(*([np.asarray(x)[g.inverse] for x in answers] for g, answers in parts)))
    return _finish_window(status, outcome, final_age, nodes, hits, score, bound)


def drive_host(rows, alpha, beta, driver_plies, node_budget=None, nodes_per_launch=None, leaf_solver=_host_leaf, book=None):
    """The root driver without a device: ``(Windowed, report)`` for `rows` (Boards, pairs or uint64 [n, 2]) with the window
    `alpha`, `beta` (scalars, per-row arrays, or both None), each row spread over the leaves `driver_plies` (1..8) below it.

    The leaves are searched with ``solve_host(window=)`` from their static windows, table-free, and the launches of the
    device are modelled: a leaf that needs N nodes has entered min(N, 1 + t * nodes_per_launch, node_budget) after launch
    t; it is answered in the launch that enters its last node if quota is left then or nothing but cut-offs follows that
    node, else in the next; it is over budget when the count reaches node_budget unanswered.  After k_solve_init's answers
    and after every launch the intervals are folded up, the needed nodes marked down, and the leaves no undecided row needs
    dropped -- so states, intervals and node counts are what c4_solve_graph reports table-free, bit for bit.

    report: per node, levels concatenated, lo, hi int8, state int8 (NODE_*), nodes, table_hits int64, the static windows
    alpha, beta, and launches, needed (the marks after k_solve_init and after each launch) and graph (the ``Graph``).
    leaf_solver(c0, c1, alpha, beta, node_budget) -> (status, score, bound, nodes, clean) replaces the search.  book: a
    ``Book`` the default leaf search probes as the kernel does; table_hits then counts its hits, as c4_solve_graph does."""
    plies = _check_driver_plies(driver_plies)
    if book is not None:
        leaf_solver = functools.partial(leaf_solver, book=book)
    rows = _rows_u64(rows)
    a, b = _window_arrays(alpha, beta, len(rows))
    g = _build_graph(rows, a, b, plies, _children_host)
    answers, report = drive_graph_host(g, node_budget, nodes_per_launch, leaf_solver)
    return _finish_graph([(g, answers)]), report


def _check_graph(g):
    """The binding's own checks of a ``Graph``, before any device call: what c4_solve_graph checks again."""
    start = np.asarray(g.level_start, dtype=np.int64)
    if start.ndim != 1 or not 1 <= len(start) - 2 <= 8:
        raise ValueError("a graph has 2..9 levels; level_start has %d entries" % start.size)
    if start[0] != 0 or (np.diff(start) < 0).any():
        raise ValueError("level_start must begin at 0 and not decrease")
    n_nodes = int(start[-1])
    child = np.asarray(g.child)
    if child.shape != (n_nodes, WIDTH) or len(g.color0) != n_nodes or len(g.color1) != n_nodes:
        raise ValueError("color0, color1 and child have one entry a node (%d)" % n_nodes)
    if start[-1] - start[-2] > GRAPH_MAX_LEAVES:
        raise ValueError("the last level has %d nodes, a graph takes %d" % (start[-1] - start[-2], GRAPH_MAX_LEAVES))
    level = np.searchsorted(start, np.arange(n_nodes), side="right") - 1
    nxt_lo = np.append(start, n_nodes)[level + 1][:, None]
    nxt_hi = np.append(start, n_nodes)[level + 2][:, None]
    bad = np.nonzero((child != -1) & ((child < nxt_lo) | (child >= nxt_hi)))
    if len(bad[0]):
        raise ValueError("node %d, column %d: child %d is not in the next level" % (bad[0][0], bad[1][0], child[bad[0][0], bad[1][0]]))
    orphan = np.ones(n_nodes, dtype=bool)
    orphan[:int(start[1])] = False
    orphan[child[child >= 0]] = False
    if orphan.any():
        raise ValueError("node %d has no parent" % np.nonzero(orphan)[0][0])
    if (g.alpha is None) != (g.beta is None):
        raise ValueError("alpha and beta are given together, or both are None")
    if g.alpha is not None:
        _window_arrays(g.alpha, g.beta, int(start[1]))


def solve_graph(g, node_budget=None, nodes_per_launch=None, device=0, table=None):
    """c4_solve_graph on a ``Graph`` (``_build_graph``): the answers of level 0, (status, score, bound, outcome code,
    final_age, nodes, table_hits), and the per-node report {lo, hi, state, nodes, table_hits} -- ``drive_graph_host``'s,
    from the device.  For tests and tools; the public calls take ``driver_plies``."""
    _check_graph(g)
    if table is not None:
        device = table.device
    n_nodes, n0 = len(g.child), int(g.level_start[1])
    status, score, bound, outcome, age = (np.zeros(n0, dtype=np.int8) for _ in range(5))
    nodes, hits = (np.zeros(n0, dtype=np.int64) for _ in range(2))
    report = {"lo": np.zeros(n_nodes, dtype=np.int8), "hi": np.zeros(n_nodes, dtype=np.int8), "state": np.zeros(n_nodes, dtype=np.int8),
              "nodes": np.zeros(n_nodes, dtype=np.int64), "table_hits": np.zeros(n_nodes, dtype=np.int64)}
    c0, c1 = (np.ascontiguousarray(x, dtype=np.uint64) for x in (g.color0, g.color1))
    start = np.ascontiguousarray(g.level_start, dtype=np.int64)
    child = np.ascontiguousarray(g.child, dtype=np.int32)
    a = None if g.alpha is None else np.ascontiguousarray(g.alpha, dtype=np.int8)
    b = None if g.beta is None else np.ascontiguousarray(g.beta, dtype=np.int8)
    _check(L.load().c4_solve_graph(int(device), table.handle if table is not None else None, _ptr(c0), _ptr(c1), _ptr(start),
                                   len(start) - 1, _ptr(child), _ptr(a), _ptr(b), int(node_budget or 0),
                                   int(nodes_per_launch or 0), _ptr(status), _ptr(score), _ptr(bound), _ptr(outcome), _ptr(age), _ptr(nodes),
                                   _ptr(hits), _ptr(report["lo"]), _ptr(report["hi"]), _ptr(report["state"]), _ptr(report["nodes"]),
                                   _ptr(report["table_hits"])))
    report["graph"] = g
    return (status, score, bound, outcome, age, nodes, hits), report


def _split_for_graphs(n, build):
    """``build(lo, hi)`` -> Graph for the rows [lo, hi), halved until no graph's last level passes GRAPH_MAX_LEAVES."""
    todo, out = [(0, n)], []
    while todo:
        lo, hi = todo.pop()
        g = build(lo, hi)
        leaves = int(g.level_start[-1] - g.level_start[-2])
        if leaves > GRAPH_MAX_LEAVES and hi - lo > 1:
            mid = (lo + hi) // 2
            todo += [(mid, hi), (lo, mid)]
        elif leaves > GRAPH_MAX_LEAVES:
            raise ValueError("row %d alone has %d distinct descendants %d plies down, a graph takes %d: give fewer driver_plies" % (
                lo, leaves, len(g.level_start) - 2, GRAPH_MAX_LEAVES))
        else:
            out.append((lo, hi, g))
    return out


def _drive(rows, alpha, beta, driver_plies, node_budget, nodes_per_launch, device, table, host, tally=None, book=None):
    """``Windowed`` of uint64 [n, 2] `rows` with windows int8 [n] (or None, None) through the root driver: on the device
    (c4_solve_graph, the children listed by c4_solve_children_dev) or, host=True, ``drive_graph_host``.  tally: a dict that
    gets the count of nodes per state name (NODE_STATE_NAMES) added."""
    plies = _check_driver_plies(driver_plies)
    n = len(rows)
    if table is not None and not host:
        device = table.device
    children_of = _children_host if host else _children_of(device)
    parts = _split_for_graphs(n, lambda lo, hi: _build_graph(rows[lo:hi], None if alpha is None else alpha[lo:hi],
                                                             None if beta is None else beta[lo:hi], plies, children_of))
    answered = []
    for lo, hi, g in sorted(parts, key=lambda p: p[0]):
        if host:
            answers, report = drive_graph_host(g, node_budget, nodes_per_launch, functools.partial(_host_leaf, book=book) if book is not None else _host_leaf)
        else:
            answers, report = solve_graph(g, node_budget, nodes_per_launch, device, table)
        if tally is not None:
            for code, name in NODE_STATE_NAMES.items():
                tally[name] = tally.get(name, 0) + int((report["state"] == code).sum())
        answered.append((g, answers))
    return _finish_graph(answered)


# -- grid_search's triple --------------------------------------------------------------------------------------------------
def _check_root(board, deep=False):
    if board.result is not None:
        raise ValueError("cannot search a finished position")
    if not deep and SIZE - board.age > MAX_EMPTIES:
        raise ValueError("grid_triple solves positions with at most %d empty squares; this one has %d" % (
            MAX_EMPTIES, SIZE - board.age))


def _triple(board, child_boards, child_values):
    """grid_search.py:21-32 with plies = the board's empty squares: the tree's root and children from the children's exact
    values, Tree.best_move and the returned triple."""
    side = board.player_to_move
    value = -2 if side == Side.o else 2
    kids = []
    for (m, cb), v in zip(child_boards, child_values):
        value = max(value, v) if side == Side.o else min(value, v)
        if cb.result is not None:
            kids.append((m, cb, v, None))
        else:
            kids.append((m, cb, None, v))
    tree = GridTree(board, value, kids)
    child = tree.best_move()
    return child.name, child.data.absolute_value, tree


def _child_boards(board):
    out = []
    for m in sorted(board.valid_moves):
        cb = board.__copy__()
        cb.make_move(m)
        out.append((m, cb))
    return out


def grid_triple(boards: Sequence[Board], device=0, node_budget=None, nodes_per_launch=None, host=False, table=None, split_plies=0, book=None):
    """``[(move, value, tree)]``, what ``grid_search.grid_search(boards, plies=empties, evaluate_centre)`` returns for
    undecided boards with at most MAX_EMPTIES empty squares: GridTree's root and children with their ``absolute_value``s,
    Tree.best_move's tie to the higher column.  Every child of every root is solved as a row of its own in one batch;
    host=True solves them with ``solve_host`` instead (no GPU).  A child the budget leaves UNKNOWN raises RuntimeError.
    table (a ``Table``; with host=True a dict), split_plies and book are ``solve``'s: with any, boards of any depth are taken."""
    deep = table is not None or bool(split_plies) or book is not None
    for b in boards:
        _check_root(b, deep)
    kids = [_child_boards(b) for b in boards]
    flat = [cb for ks in kids for _, cb in ks if cb.result is None]
    if host:
        answers = [solve_host(cb, node_budget, table=table, deep=deep, book=book) for cb in flat]
        status = [a.status for a in answers]
        values = [a.value for a in answers]
    elif flat:
        res = solve(flat, node_budget, nodes_per_launch, device, table=table, split_plies=split_plies, book=book)
        status, values = res.status.tolist(), res.value.tolist()
    else:
        status, values = [], []
    if any(s != L.SOLVE_SOLVED for s in status):
        raise RuntimeError("%d child positions were not solved within the node budget" % sum(s != L.SOLVE_SOLVED for s in status))
    it = iter(values)
    out = []
    for b, ks in zip(boards, kids):
        vals = [_terminal_value(cb) if cb.result is not None else float(next(it)) for _, cb in ks]
        out.append(_triple(b, ks, vals))
    return out


# -- labelling ---------------------------------------------------------------------------------------------------------------
def prior_from_children(outcome, child_outcomes, legal):
    """generate_7ply.py:83-91 with exact outcomes: uniform over the legal moves whose child has the position's outcome,
    zeros if there is none.  outcome [n], child_outcomes [n, 7], legal [n, 7] (NumPy or torch, any numeric type)."""
    if _is_tensor(outcome):
        import torch
        keep = (legal != 0) & (child_outcomes == outcome[:, None])
        p = keep.to(torch.float64)
        s = p.sum(dim=1, keepdim=True)
        return torch.where(s > 0, p / torch.clamp(s, min=1.0), torch.zeros_like(p))
    keep = (np.asarray(legal) != 0) & (np.asarray(child_outcomes) == np.asarray(outcome)[:, None])
    p = keep.astype(np.float64)
    s = p.sum(axis=1, keepdims=True)
    return np.where(s > 0, p / np.maximum(s, 1.0), 0.0)


def _wins_bits(p):
    """bool [m]: the stones `p` (uint64 [m]) hold four in a row."""
    out = np.zeros(p.shape, dtype=bool)
    for s in (1, HEIGHT, H1, H1 + 1):
        y = p & (p >> np.uint64(s))
        out |= (y & (y >> np.uint64(2 * s))) != 0
    return out


def staged_labels(rows, window_solver, children_of=None, stage2=True):
    """The labelling rule from outcomes alone, in two stages of windowed searches; plain NumPy around two callables, so the
    device and the host mirror label by the same lines.

    rows: uint64 [n, 2] distinct positions.  window_solver(rows uint64 [m, 2], alpha int8 [m], beta int8 [m]) -> (status,
    score, nodes, table_hits) arrays of m: c4_solve_window's answers.  children_of(rows) -> (children uint64 [n, 7, 2], legal
    bool [n, 7]), default ``_children_host``.

    Stage 1: every row with the window (-1, +1); the sign of the score is V, the outcome for the mover.
    Stage 2: for rows with V >= 0, each legal child that is not finished, with a null window on the child's mover's score:
    (-1, 0) under V = +1, (0, 1) under V = 0.  The child keeps V iff it fails low (score <= alpha): it is lost for its mover,
    or no better than drawn.  A finished child answers with its own result; under V = -1 every legal move keeps V and nothing
    is searched.  The stage-2 rows are the distinct (position, window) pairs, mirror images merged (``_canonical`` is the
    key, the image met first is the one searched), one batch.

    Returns a dict: status int8 [n] (stage 1's, UNKNOWN also where a stage-2 row the position needs is), v int64 [n],
    outcome int8 [n] (C4_RESULT_*, -1 where there is none), keep bool [n, 7] (the moves that keep the outcome), legal, and
    stage1_rows / _nodes / _unknown / _hits and stage2_rows / _nodes / _unknown / _hits.  Raises RuntimeError if a fully
    known position with V >= 0 has no keeping move: the searches would contradict each other.  stage2=False stops after
    stage 1: keep and legal are all False and the stage-2 counts zero."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
    n = len(rows)
    ones = np.ones(n, dtype=np.int8)
    status, score, nodes1, hits1 = (np.asarray(a) for a in window_solver(rows, -ones, ones))
    status = status.astype(np.int8)
    solved = status == L.SOLVE_SOLVED
    v = np.where(solved, np.sign(score.astype(np.int64)), 0)
    odd = (_ages(rows) & 1) == 1
    outcome = np.where(solved, np.where(odd, -v, v) + 1, -1).astype(np.int8)
    if not stage2:
        none = np.zeros((n, WIDTH), dtype=bool)
        return {"status": status, "v": v, "outcome": outcome, "keep": none, "legal": none, "stage1_rows": n,
                "stage1_nodes": int(nodes1.sum()), "stage1_unknown": int((status == L.SOLVE_UNKNOWN).sum()), "stage1_hits": int(hits1.sum()),
                "stage2_rows": 0, "stage2_nodes": 0, "stage2_unknown": 0, "stage2_hits": 0}
    children, legal = (children_of or _children_host)(rows)
    children = np.asarray(children, dtype=np.uint64)
    legal = np.asarray(legal).astype(bool) & solved[:, None]
    moved = np.where(odd[:, None], children[:, :, 1], children[:, :, 0])        # the stones of the side that just moved
    won = legal & _wins_bits(moved)
    full = legal & ~won & ((_popcount64(children[:, :, 0] | children[:, :, 1]) == SIZE))
    need = legal & ~won & ~full & (v >= 0)[:, None]
    parent_v = np.broadcast_to(v[:, None], need.shape)[need]
    # a stage-2 row is a (position, window) pair; mirror images are one pair, searched as the one met first (the move order
    # breaks ties by column, so an image can cost other nodes than its original: none is the cheaper by rule)
    asked = children[need]
    triples = np.concatenate([_canonical(asked), parent_v.astype(np.uint64)[:, None]], axis=1) if need.any() else np.zeros((0, 3), dtype=np.uint64)
    if len(triples):
        _, first, inv = np.unique(triples, axis=0, return_index=True, return_inverse=True)
        inv = np.asarray(inv, dtype=np.int64).reshape(-1)
        uniq = np.concatenate([asked[first], triples[first, 2:]], axis=1)
    else:
        uniq, inv = triples, np.zeros(0, dtype=np.int64)
    alpha2 = np.where(uniq[:, 2] == 1, -1, 0).astype(np.int8)
    if len(uniq):
        status2, score2, nodes2, hits2 = (np.asarray(a) for a in window_solver(np.ascontiguousarray(uniq[:, :2]), alpha2, (alpha2 + 1).astype(np.int8)))
    else:
        status2, score2, nodes2, hits2 = (np.zeros(0, dtype=np.int64) for _ in range(4))
    known2 = status2 == L.SOLVE_SOLVED
    keep = np.where((v < 0)[:, None], legal, (won & (v == 1)[:, None]) | (full & (v == 0)[:, None]))
    keep[need] = (known2 & (score2 <= alpha2))[inv]
    missing = np.zeros(need.shape, dtype=bool)
    missing[need] = ~known2[inv]
    unknown = solved & missing.any(axis=1)
    broken = np.nonzero(solved & ~unknown & (v >= 0) & ~keep.any(axis=1))[0]
    if len(broken):
        i = int(broken[0])
        raise RuntimeError("the position (%#x, %#x) has the outcome %+d for its mover and no move that keeps it" % (
            int(rows[i, 0]), int(rows[i, 1]), int(v[i])))
    status = np.where(unknown, L.SOLVE_UNKNOWN, status).astype(np.int8)
    return {"status": status, "v": v, "outcome": np.where(unknown, -1, outcome).astype(np.int8), "keep": keep & ~unknown[:, None],
            "legal": legal,
            "stage1_rows": n, "stage1_nodes": int(nodes1.sum()), "stage1_unknown": int((status == L.SOLVE_UNKNOWN).sum() - unknown.sum()),
            "stage1_hits": int(hits1.sum()),
            "stage2_rows": len(uniq), "stage2_nodes": int(nodes2.sum()), "stage2_unknown": int((status2 == L.SOLVE_UNKNOWN).sum()),
            "stage2_hits": int(hits2.sum())}


def _first_occurrences(rows):
    """The distinct rows of uint64 [n, 2] in the order of their first occurrence."""
    if len(rows) == 0:
        return rows
    _, first = np.unique(rows, axis=0, return_index=True)
    return np.ascontiguousarray(rows[np.sort(first)])


def _window_solver(node_budget, nodes_per_launch, device, table, host, driver_plies=0, tally=None, book=None):
    """staged_labels' window_solver on the device (c4_solve_window_dev) or, host=True, on ``solve_host`` (table: a dict or a
    ``HostTable``); with driver_plies the root driver on either, each stage one driven batch."""
    if driver_plies:
        if host and table is not None:
            raise ValueError("host=True drives table-free")

        def driven(rows, alpha, beta):
            res = _drive(np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2), np.ascontiguousarray(alpha, dtype=np.int8),
                         np.ascontiguousarray(beta, dtype=np.int8), driver_plies, node_budget, nodes_per_launch, device, table, host, tally, book if host else None)
            return res.status, res.score, res.nodes, res.table_hits
        return driven
    if host:
        def on_host(rows, alpha, beta):
            ans, hits = [], []
            for (c0, c1), a, b in zip(rows, alpha, beta):
                ans.append(solve_host((int(c0), int(c1)), node_budget, table=table, window=(int(a), int(b)), book=book))
                hits.append(ans[-1].hits if book is not None else 0)
            return (np.array([a.status for a in ans], dtype=np.int8), np.array([a.score for a in ans], dtype=np.int8),
                    np.array([a.nodes for a in ans], dtype=np.int64), np.array(hits, dtype=np.int64))
        return on_host

    def on_device(rows, alpha, beta):
        import torch
        packed = _packed_on_device(torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)), device)
        window = (np.ascontiguousarray(alpha, dtype=np.int8), np.ascontiguousarray(beta, dtype=np.int8))
        status, _, _, nodes, hits, score, _ = (t.cpu().numpy() for t in _solve_dev(packed, node_budget, nodes_per_launch, table, window=window))
        return status, score, nodes, hits
    return on_device


def _label_staged(boards, node_budget, nodes_per_launch, device, table, host, with_priors, driver_plies=0, book=None):
    import torch
    from .stats import LabelledSet
    if book is not None and not host:
        with _carrying(table, book, device) as carrier:
            ls, report = _label_staged(boards, node_budget, nodes_per_launch, device, carrier, host, with_priors, driver_plies)
        report["book_age"], report["book_entries"] = book.age, len(book)
        return ls, report
    t0 = time.perf_counter()
    if table is not None and not host:
        device = table.device
    if host:
        rows_in, out_dev = _rows_u64(boards), torch.device("cpu")
    else:
        packed = _packed_on_device(boards, device)
        rows_in, out_dev = _rows_u64(packed), packed.device
    rows = _first_occurrences(rows_in)
    tally = {}
    solver_fn = _window_solver(node_budget, nodes_per_launch, device, table, host, driver_plies, tally, book)
    st = staged_labels(rows, solver_fn, stage2=with_priors)
    keep = st["status"] == L.SOLVE_SOLVED
    values = torch.from_numpy((st["outcome"][keep].astype(np.float32) * np.float32(0.5)))
    bits = torch.from_numpy(np.ascontiguousarray(rows[keep]).view(np.int64)).to(out_dev).contiguous()
    priors = None
    if with_priors:
        p = st["keep"][keep].astype(np.float64)
        tot = p.sum(axis=1, keepdims=True)
        priors = torch.from_numpy(np.where(tot > 0, p / np.maximum(tot, 1.0), 0.0).astype(np.float32)).to(out_dev).contiguous()
    ls = LabelledSet(bits, values.to(out_dev).contiguous(), priors)
    counts = np.bincount(st["status"].astype(np.int64), minlength=len(STATUS_NAMES))
    report = {"positions": len(rows_in), "distinct": len(rows), "labelled": len(ls), "nodes": st["stage1_nodes"] + st["stage2_nodes"],
              "exact": False, "table_log2_entries": getattr(table, "log2_entries", None),
              "table_hits": st["stage1_hits"] + st["stage2_hits"]}
    if driver_plies:
        report["driver_plies"] = int(driver_plies)
        report["driver_nodes"] = tally      # the graphs' nodes by state: interior, self_answering, answered, over_budget, dropped
    report.update({k: st[k] for k in ("stage1_rows", "stage1_nodes", "stage1_unknown", "stage2_rows", "stage2_nodes", "stage2_unknown")})
    report.update({name: int(counts[code]) for code, name in STATUS_NAMES.items()})
    report["seconds"] = time.perf_counter() - t0
    return ls, report


def label_values(boards, node_budget=None, nodes_per_launch=None, device=0, table=None, host=False, driver_plies=0, book=None):
    """Label positions with their outcome alone: ``(LabelledSet without priors, report)``, the kind of set the reference
    scores by value only.  This is stage 1 of ``label(exact=False)`` -- one search per distinct position with the window
    (-1, +1), at any depth -- and nothing else; rows, order and report as there.  driver_plies: ``solve_window``'s; book:
    ``solve``'s (the report then says book_age and book_entries)."""
    if driver_plies:
        _check_driver_plies(driver_plies)
    return _label_staged(boards, node_budget, nodes_per_launch, device, table, host, with_priors=False, driver_plies=driver_plies, book=book)


def label(boards, node_budget=None, nodes_per_launch=None, device=0, table=None, split_plies=0, exact=True, host=False, deep=False,
          driver_plies=0, book=None):
    """Label positions with their exact outcome: returns ``(LabelledSet, report)``.

    Each distinct position is solved once, together with its up-to-seven children (c4_solve_children_dev lists them) in one
    batch.  value = the outcome (0.0 / 0.5 / 1.0); prior = ``prior_from_children``.  Rows that are unknown, too deep,
    terminal or invalid are dropped, as is a row one of whose children stayed unknown (counted as unknown); the kept rows
    stay in the order of their first occurrence.  report: positions, distinct, labelled, the count per status
    (STATUS_NAMES), nodes (parents and children) and seconds.

    table (a ``Table``) and split_plies are ``solve``'s; with either, positions of any depth are labelled (none is too deep)
    and only the children that exist are solved.  The report then also says table_log2_entries and table_hits.  deep=True
    is the same without either: the table-free deep search.

    exact=False labels by outcome alone (``staged_labels``): the rule never asks how fast a game is won, so each distinct
    position gets one search with the window (-1, +1), and only the unfinished children of positions that are not lost get
    one null-window search each ("does this move keep the outcome?"), as one batch against the same `table`.  Positions of
    any depth are taken, with or without a table.  Wherever both label a row the set equals exact=True's bit for bit; the
    report says exact: False and, per stage, stage1_rows / stage1_nodes / stage1_unknown and stage2_rows / stage2_nodes /
    stage2_unknown (nodes = stage1_nodes + stage2_nodes; unknown = stage1_unknown + the positions a stage-2 row leaves
    open).  host=True (with exact=False) runs the same staging on ``solve_host`` -- no GPU; `table` is then a dict or a
    ``HostTable``.  driver_plies=k (with exact=False, not with split_plies) runs each stage through the root driver
    (``solve_window``): the same labels wherever both label a row, and a row stays unknown only where a descendant the proof
    needs does; with host=True no table is taken.  book: ``solve``'s, on every path (the report then says book_age and
    book_entries): with a book of the children's ply a position is labelled by lookups alone."""
    if book is not None and exact:
        if host:
            raise ValueError("host=True labels with exact=False only")
        with _carrying(table, book, device) as carrier:
            ls, report = label(boards, node_budget, nodes_per_launch, device, carrier, split_plies, True, False, True, driver_plies)
        report["book_age"], report["book_entries"] = book.age, len(book)
        return ls, report
    if driver_plies:
        _check_driver_plies(driver_plies)
        if split_plies:
            raise ValueError("driver_plies and split_plies are two ways to spread a position: give one")
        if exact:
            raise ValueError("driver_plies belongs to exact=False: the driver folds bounds, not exact scores")
    if not exact:
        if split_plies:
            raise ValueError("split_plies belongs to exact=True: the staged labelling does not split")
        return _label_staged(boards, node_budget, nodes_per_launch, device, table, host, with_priors=True, driver_plies=driver_plies, book=book)
    if host:
        raise ValueError("host=True labels with exact=False only")
    import torch
    from .stats import LabelledSet
    t0 = time.perf_counter()
    packed = _packed_on_device(boards, device)
    n_in = int(packed.shape[0])
    with torch.cuda.device(packed.device):
        uniq, inverse = torch.unique(packed, dim=0, return_inverse=True)
        first = torch.full((uniq.shape[0],), n_in, dtype=torch.int64, device=packed.device)
        first.scatter_reduce_(0, inverse, torch.arange(n_in, device=packed.device), reduce="amin")
        uniq = uniq[torch.argsort(first)].contiguous()
        n = int(uniq.shape[0])
        children, legal = _children_dev(uniq)
        is_legal = legal != 0
        total_hits = 0
        if table is None and not split_plies and not deep:
            batch = torch.cat([uniq, children.reshape(n * WIDTH, 2)]).contiguous()
            status, outcome, _, nodes, _ = _solve_dev(batch, node_budget, nodes_per_launch)
            p_status, p_out = status[:n], outcome[:n]
            c_status, c_out = status[n:].reshape(n, WIDTH), outcome[n:].reshape(n, WIDTH)
        else:
            # the deep search reaches the empty board, so the zero rows of the illegal slots stay out of the batch
            res = solve(torch.cat([uniq, children[is_legal]]).contiguous(), node_budget, nodes_per_launch, device, table=table,
                        deep=True, split_plies=split_plies)
            status = torch.from_numpy(res.status).to(packed.device)
            outcome = torch.from_numpy(np.where(np.isnan(res.outcome), -1, res.outcome * 2).astype(np.int8)).to(packed.device)
            nodes = torch.from_numpy(res.nodes)
            total_hits = int(res.table_hits.sum())
            p_status, p_out = status[:n], outcome[:n]
            c_status = torch.full((n, WIDTH), L.SOLVE_INVALID, dtype=torch.int8, device=packed.device)
            c_out = torch.full((n, WIDTH), -1, dtype=torch.int8, device=packed.device)
            c_status[is_legal] = status[n:]
            c_out[is_legal] = outcome[n:]
        child_known = (~is_legal | (c_status == L.SOLVE_SOLVED) | (c_status == L.SOLVE_TERMINAL)).all(dim=1)
        keep = (p_status == L.SOLVE_SOLVED) & child_known
        p_status = torch.where((p_status == L.SOLVE_SOLVED) & ~child_known, torch.full_like(p_status, L.SOLVE_UNKNOWN), p_status)
        priors = prior_from_children(p_out, c_out, legal).to(torch.float32)
        values = p_out.to(torch.float32) * 0.5
        ls = LabelledSet(uniq[keep].contiguous(), values[keep].contiguous(), priors[keep].contiguous())
        counts = torch.bincount(p_status.long(), minlength=len(STATUS_NAMES)).cpu().tolist()
        # illegal child slots are zero rows (the empty board: too deep, never searched, 0 nodes)
        total_nodes = int(nodes.sum().item())
    report = {"positions": n_in, "distinct": n, "labelled": len(ls), "nodes": total_nodes}
    if table is not None or split_plies or deep:
        report.update(table_log2_entries=table.log2_entries if table is not None else None, table_hits=total_hits,
                      split_plies=int(split_plies))
    report.update({name: int(counts[code]) for code, name in STATUS_NAMES.items()})
    report["seconds"] = time.perf_counter() - t0
    return ls, report
