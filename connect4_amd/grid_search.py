"""Fixed-depth negamax player with the reference's interface (oinkoink/grid_search.py:10-71), searched on
the GPU by connect4_amd/csrc/c4_grid.hip.

``GridSearch(name, plies, evaluator).make_move(board)`` expands every position ``plies`` deep, folds the
values back with max (o to move) / min (x to move), plays the best root child on the caller's board and
returns ``(move, value, tree)``; ``make_moves(boards)`` does a whole batch in one device call (``Match``
plays grid-search players in lock-step through it).  Leaves:

  * ``evaluate_centre`` is computed inside the kernel;
  * any other scalar evaluator: the device lists the undecided positions ``plies`` deep in the order the
    reference evaluates them, each distinct one goes through the caller's ``Evaluator`` once (so its
    ``position_table`` fills as in the reference), and the device finishes the search with those values;
  * an evaluator returning anything but a real number (``evaluate_centre_with_prior``, ``evaluate_nn``)
    raises the ``TypeError`` the reference raises when it compares such a value.

Two deviations from the reference:
  * the returned tree holds only the root and its children (the reference's anytree holds every node; its
    callers read the root's children only);
  * with ``evaluate_centre`` the leaves are scored in the kernel, so the ``Evaluator``'s ``position_table`` is
    not filled (the reference fills it with every leaf); other evaluators fill it as the reference does.

``nega_max_host`` is a plain-Python mirror of the reference's search for tests and tools.
"""
import numbers
from typing import List, Sequence

import numpy as np

from . import _lib as L
from .board import Board, boards_to_bits
from .evaluators import evaluate_centre, unwrap
from .player import BasePlayer
from .utils import Connect4Stats as info
from .utils import Side, same_side, value_to_side

__all__ = ["GridSearch", "GridTree", "grid_search", "nega_max_host"]


class GridNodeData:
    """tree.py:18-44 NodeData: board, position_value (leaf or terminal value), search_value (interior)."""

    def __init__(self, board: Board, position_value=None, search_value=None):
        self.board = board
        self.valid_moves = board.valid_moves
        self.position_value = position_value
        self.search_value = search_value

    @property
    def absolute_value(self):          # tree.py:27-38
        if self.board.result is not None:
            return self.board.result.value
        if self.search_value is not None:
            return float(self.search_value)
        if self.position_value is not None:
            return float(self.position_value)
        return None

    def value(self, side: Side):       # tree.py:40-44
        v = self.absolute_value
        return 0.0 if v is None else value_to_side(v, side)

    def __str__(self):
        return "board_result: {},  position_value: ({}),  search_value: ({})".format(
            self.board.result, self.position_value, self.search_value)


class GridNode:
    def __init__(self, name, data, parent=None):
        self.name = name
        self.data = data
        self.parent = parent
        self.children = ()

    @property
    def is_root(self):
        return self.parent is None

    def __gt__(self, other):           # tree.py:11-15 node_gt
        return self.name > other.name


class GridTree:
    """The root and its children of the reference's Tree (tree.py:61-147) after a grid search."""

    def __init__(self, board: Board, root_value, children):
        self.side = board.player_to_move
        self.root = GridNode("root", GridNodeData(board.__copy__(), search_value=root_value))
        kids = []
        for move, cb, pv, sv in children:
            kids.append(GridNode(move, GridNodeData(cb, pv, sv), self.root))
        self.root.children = tuple(kids)

    def get_node_value(self, node):
        return node.data.value(self.side)

    def best_move(self):               # tree.py:68-72
        return max(((self.get_node_value(c), c) for c in self.root.children))[1]

    def get_values_policy(self):       # tree.py:104-109,139-147
        policy = np.zeros((info.width,))
        for c in self.root.children:
            policy[c.name] = self.get_node_value(c)
        s = np.sum(policy)
        if s == 0.0:
            for c in self.root.children:
                policy[c.name] = 1.0
            policy /= len(self.root.children)
        else:
            policy /= s
        return policy


def _terminal_value(board: Board):
    """grid_search.py:43-50: prefer faster wins and slower losses."""
    if same_side(board.result, Side.o):
        return board.result.value - board.age / 10000.0
    return board.result.value + board.age / 10000.0


def _check(board: Board, plies: int):
    if plies < 1:
        raise ValueError("GridSearch needs plies >= 1, got %r" % (plies,))
    if board.result is not None:
        raise ValueError("cannot search a finished position")


def _nega_max(board: Board, plies: int, evaluator):
    if board.result is not None:
        return _terminal_value(board)
    if plies == 0:
        return evaluator(board)
    if board.player_to_move == Side.o:
        value = -2
        for m in sorted(board.valid_moves):
            b = board.__copy__()
            b.make_move(m)
            value = max(value, _nega_max(b, plies - 1, evaluator))
    else:
        value = 2
        for m in sorted(board.valid_moves):
            b = board.__copy__()
            b.make_move(m)
            value = min(value, _nega_max(b, plies - 1, evaluator))
    return value


def nega_max_host(board: Board, plies: int, evaluator):
    """Plain-Python grid search (grid_search.py:21-71): returns ``(move, value, tree)`` and leaves the
    board unchanged.  Any evaluator the reference accepts works here, non-scalar ones fail as they do
    there."""
    _check(board, plies)
    children = []
    side = board.player_to_move
    value = -2 if side == Side.o else 2
    for m in sorted(board.valid_moves):
        cb = board.__copy__()
        cb.make_move(m)
        v = _nega_max(cb, plies - 1, evaluator)
        value = max(value, v) if side == Side.o else min(value, v)
        if cb.result is not None or plies == 1:
            children.append((m, cb, v, None))
        else:
            children.append((m, cb, None, v))
    tree = GridTree(board, value, children)
    child = tree.best_move()
    return child.name, child.data.absolute_value, tree


def _scalar(v):
    if isinstance(v, (numbers.Real, np.floating, np.integer)) or (isinstance(v, np.ndarray) and v.ndim == 0):
        return float(v)
    # grid_search.py:62-70 compares the value with a number: the reference fails there
    raise TypeError("GridSearch needs a scalar evaluator; got a value of type %s" % type(v).__name__)


def _external_values(c0, c1, n, plies, evaluator, device):
    lib = L.load()
    cap = max(1024, 8 * n)
    while True:
        l0 = np.zeros(cap, dtype=np.uint64)
        l1 = np.zeros(cap, dtype=np.uint64)
        got = np.zeros(1, dtype=np.int64)
        rc = lib.c4_grid_frontier(device, _p(c0, L._u64p), _p(c1, L._u64p), n, plies, _p(l0, L._u64p),
                                  _p(l1, L._u64p), cap, _p(got, L._i64p))
        if rc == L.ECAPACITY:
            cap = int(got[0])
            continue
        _check_rc(rc)
        break
    k = int(got[0])
    values = np.empty(k, dtype=np.float64)
    seen = {}
    for i in range(k):                       # the reference's evaluation order; each distinct position once
        key = (int(l0[i]), int(l1[i]))
        v = seen.get(key)
        if v is None:
            v = seen[key] = _scalar(evaluator(Board.from_bits(*key)))
        values[i] = v
    return values


def _p(a, t):
    return a.ctypes.data_as(t)


def _check_rc(rc):
    if rc != L.OK:
        msg = L.load().c4_grid_last_error()
        raise L.EngineError(rc, msg.decode("utf-8", "replace") if msg else "")


def grid_search(boards: Sequence[Board], plies: int, evaluator, device: int = 0):
    """Search every board on the GPU; returns ``[(move, value, tree)]`` without touching the boards."""
    for b in boards:
        _check(b, plies)
    n = len(boards)
    if n == 0:
        return []
    c0, c1 = boards_to_bits(boards)
    c0 = np.ascontiguousarray(c0)
    c1 = np.ascontiguousarray(c1)
    child = np.zeros((n, 7), dtype=np.float64)
    root = np.zeros(n, dtype=np.float64)
    move = np.zeros(n, dtype=np.int32)
    lib = L.load()
    outs = (_p(child, L._f64p), _p(root, L._f64p), _p(move, L._i32p))
    if unwrap(evaluator) is evaluate_centre:
        rc = lib.c4_grid_search(device, _p(c0, L._u64p), _p(c1, L._u64p), n, plies, *outs)
    else:
        values = _external_values(c0, c1, n, plies, evaluator, device)
        rc = lib.c4_grid_finish(device, _p(c0, L._u64p), _p(c1, L._u64p), n, plies, _p(values, L._f64p),
                                len(values), *outs)
    _check_rc(rc)
    out = []
    for i, b in enumerate(boards):
        kids = []
        for m in sorted(b.valid_moves):
            cb = b.__copy__()
            cb.make_move(m)
            a = float(child[i, m])
            if cb.result is not None:
                kids.append((m, cb, _terminal_value(cb), None))
            elif plies == 1:
                kids.append((m, cb, a, None))
            else:
                kids.append((m, cb, None, a))
        tree = GridTree(b, float(root[i]), kids)
        mv = int(move[i])
        out.append((mv, tree.root.children[[c.name for c in tree.root.children].index(mv)].data.absolute_value, tree))
    return out


class GridSearch(BasePlayer):
    """grid_search.py:10-35: ``GridSearch(name, plies, evaluator)``, searched on device ``device``."""

    def __init__(self, name: str, plies: int, evaluator, device: int = 0):
        super().__init__(name)
        self.plies = plies
        self.evaluator = evaluator
        self.device = device

    def make_moves(self, boards: List[Board]):
        """Batch form: every board searched in one device call, then each plays its move."""
        res = grid_search(boards, self.plies, self.evaluator, self.device)
        for b, (mv, _, _) in zip(boards, res):
            b.make_move(mv)
        return res

    def make_move(self, board: Board):
        return self.make_moves([board])[0]

    def __copy__(self):                 # match.py:26-40 copies players per game
        return GridSearch(self.name, self.plies, self.evaluator, self.device)

    def __str__(self):
        return super().__str__() + ", type: Computer"
