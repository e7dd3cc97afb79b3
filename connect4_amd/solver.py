"""Exact values of late-game positions, and test sets labelled with them.

The reference defines a position's exact value through ``GridSearch(plies >= empty squares)``: no evaluator is reached
(oinkoink/grid_search.py:38-71), so the search returns the game-theoretic result with its terminal scoring -- an o win that
ends at age ``a`` is ``1 - a/10000``, an x win ``a/10000``, a draw ``0.5 + 42/10000``.  That search is exhaustive; the kernel
behind this module (connect4_amd/csrc/c4_solve.hip) finds the same number by alpha-beta, for positions with at most
``MAX_EMPTIES`` = 24 empty squares.

``solve``       status, outcome, final age, the reference's float64 value and the node count of every row
``grid_triple`` ``(move, value, tree)`` per board, what ``grid_search(boards, plies=empties, evaluate_centre)`` returns
``label``       a ``LabelledSet`` (value = outcome, prior = uniform over the moves that keep it: the rule of
                oinkoink/scripts/generate_7ply.py:83-91) and a report
``solve_host``  a plain-Python mirror of the kernel's search -- same integer score, same pruning and move order, same node
                counts -- for tests and for machines without a GPU

The integer score: a game o wins at age ``a`` scores ``43 - a``, one x wins ``a - 43``, a draw 0, taken from the side to
move inside the search.  It is strictly monotone in the reference's float, so max / min over it pick what the reference's
max / min pick; the float itself is formed once, from outcome and age, by the division the reference performs.
"""
import time
from collections import namedtuple
from typing import Sequence

import numpy as np

from . import _lib as L
from .board import BOTTOM, H1, HEIGHT, SIZE, WIDTH, Board, _wins
from .grid_search import GridTree, _terminal_value
from .utils import Side

__all__ = ["MAX_EMPTIES", "DEFAULT_NODE_BUDGET", "STATUS_NAMES", "Solved", "HostAnswer", "solve", "solve_host", "grid_triple",
           "label", "prior_from_children", "value_from_answer", "random_playout"]

MAX_EMPTIES = L.SOLVE_MAX_EMPTIES
DEFAULT_NODE_BUDGET = 1 << 26          # the kernel's default (c4_engine.h)
STATUS_NAMES = {L.SOLVE_SOLVED: "solved", L.SOLVE_TERMINAL: "terminal", L.SOLVE_UNKNOWN: "unknown",
                L.SOLVE_TOO_DEEP: "too_deep", L.SOLVE_INVALID: "invalid"}

Solved = namedtuple("Solved", "status outcome final_age value nodes")
HostAnswer = namedtuple("HostAnswer", "status outcome final_age value nodes")

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


class _Search:
    def __init__(self, budget):
        self.nodes = 0
        self.budget = budget

    def enter(self):
        if self.nodes >= self.budget:
            raise _OverBudget()
        self.nodes += 1

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
            if v > alpha:
                alpha = v
        return alpha


def _classify(c0, c1):
    occ = c0 | c1
    n0, n1 = bin(c0).count("1"), bin(c1).count("1")
    if (c0 & c1) or (occ & ~_BOARD) or (occ & (occ + BOTTOM)) or not 0 <= n0 - n1 <= 1 or (_wins(c0) and _wins(c1)):
        return L.SOLVE_INVALID
    if _wins(c0) or _wins(c1) or n0 + n1 == SIZE:
        return L.SOLVE_TERMINAL
    if SIZE - (n0 + n1) > MAX_EMPTIES:
        return L.SOLVE_TOO_DEEP
    return L.SOLVE_SOLVED


def solve_host(board, node_budget=None):
    """The kernel's answer for one position, computed in plain Python: ``HostAnswer(status, outcome, final_age, value,
    nodes)``.  `board`: a Board or a ``(color0, color1)`` pair.  outcome / value are None where the status has none."""
    c0, c1 = (board.color if isinstance(board, Board) else board)
    c0, c1 = int(c0), int(c1)
    budget = DEFAULT_NODE_BUDGET if node_budget is None else int(node_budget)
    st = _classify(c0, c1)
    if st == L.SOLVE_TERMINAL:
        outcome = 1.0 if _wins(c0) else 0.0 if _wins(c1) else 0.5
        age = bin(c0 | c1).count("1")
        return HostAnswer(st, outcome, age, float(value_from_answer(outcome, age)), 0)
    if st != L.SOLVE_SOLVED:
        return HostAnswer(st, None, -1, None, 0)
    occ = c0 | c1
    age = bin(occ).count("1")
    mine, theirs = (c1, c0) if age & 1 else (c0, c1)
    s = _Search(budget)
    if _winning_squares(mine, occ) & (occ + BOTTOM):
        score, nodes = 42 - age, 1
    else:
        try:
            score = s.node(mine, theirs, age, -42, 42)
        except _OverBudget:
            return HostAnswer(L.SOLVE_UNKNOWN, None, -1, None, s.nodes)
        nodes = s.nodes
    abs_score = -score if age & 1 else score
    outcome = 1.0 if abs_score > 0 else 0.0 if abs_score < 0 else 0.5
    final_age = 43 - abs(abs_score) if abs_score else SIZE
    return HostAnswer(L.SOLVE_SOLVED, outcome, final_age, float(value_from_answer(outcome, final_age)), nodes)


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


def _solve_dev(packed, node_budget=None, nodes_per_launch=None):
    """c4_solve_dev on a packed cuda tensor: (status int8, outcome int8, final_age int8, nodes int64) device tensors."""
    import ctypes as C
    import torch
    n = int(packed.shape[0])
    dev = packed.device
    status = torch.empty(n, dtype=torch.int8, device=dev)
    outcome = torch.empty(n, dtype=torch.int8, device=dev)
    age = torch.empty(n, dtype=torch.int8, device=dev)
    nodes = torch.empty(n, dtype=torch.int64, device=dev)
    if n:
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            _check(L.load().c4_solve_dev(idx, C.c_void_p(stream), ptr(packed), n, int(node_budget or 0), int(nodes_per_launch or 0),
                                         ptr(status), ptr(outcome), ptr(age), ptr(nodes)))
    return status, outcome, age, nodes


def _children_dev(packed):
    """c4_solve_children_dev: (children int64 [n, 7, 2], legal int8 [n, 7]) device tensors."""
    import ctypes as C
    import torch
    n = int(packed.shape[0])
    dev = packed.device
    children = torch.zeros((n, WIDTH, 2), dtype=torch.int64, device=dev)
    legal = torch.zeros((n, WIDTH), dtype=torch.int8, device=dev)
    if n:
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _check(L.load().c4_solve_children_dev(idx, C.c_void_p(stream), C.c_void_p(packed.data_ptr()), n,
                                                  C.c_void_p(children.data_ptr()), C.c_void_p(legal.data_ptr())))
    return children, legal


def _finish(status, outcome, age, nodes):
    status = np.asarray(status, dtype=np.int8)
    age = np.asarray(age, dtype=np.int8)
    known = np.asarray(outcome) >= 0
    out = np.where(known, np.asarray(outcome, dtype=np.float64) * 0.5, np.nan)
    value = np.where(known, value_from_answer(np.where(known, out, 0.0), np.where(known, age, 0)), np.nan)
    return Solved(status, out, age, value, np.asarray(nodes, dtype=np.int64))


def solve(boards, node_budget=None, nodes_per_launch=None, device=0):
    """Solve every row on the GPU.  `boards`: a sequence of Boards (host arrays through c4_solve) or a packed int64 [n, 2]
    tensor (c4_solve_dev; a CPU tensor is moved to cuda:`device`).  Returns ``Solved`` of NumPy arrays:

      status     int8, _lib.SOLVE_* (STATUS_NAMES)
      outcome    float64 0.0 / 0.5 / 1.0, absolute like ``Result``; NaN where the status has no answer
      final_age  int8, the age at which best play ends the game; -1 where unknown
      value      float64, what ``GridSearch(plies=empties)`` computes for the node (grid_search.py:43-71); NaN where unknown
      nodes      int64, positions the search entered

    node_budget: most nodes of one row, beyond it the row is UNKNOWN (default 2^26); nodes_per_launch: the quota of one
    kernel launch (default 2^14) -- it changes neither answers nor node counts."""
    if _is_tensor(boards):
        st, out, age, nodes = _solve_dev(_packed_on_device(boards, device), node_budget, nodes_per_launch)
        return _finish(st.cpu().numpy(), out.cpu().numpy(), age.cpu().numpy(), nodes.cpu().numpy())
    import ctypes as C
    n = len(boards)
    status = np.zeros(n, dtype=np.int8)
    outcome = np.zeros(n, dtype=np.int8)
    age = np.zeros(n, dtype=np.int8)
    nodes = np.zeros(n, dtype=np.int64)
    if n:
        c0, c1 = _bits(boards)
        i8 = C.POINTER(C.c_int8)
        _check(L.load().c4_solve(device, c0.ctypes.data_as(L._u64p), c1.ctypes.data_as(L._u64p), n, int(node_budget or 0),
                                 int(nodes_per_launch or 0), status.ctypes.data_as(i8), outcome.ctypes.data_as(i8),
                                 age.ctypes.data_as(i8), nodes.ctypes.data_as(L._i64p)))
    return _finish(status, outcome, age, nodes)


# -- grid_search's triple --------------------------------------------------------------------------------------------------
def _check_root(board):
    if board.result is not None:
        raise ValueError("cannot search a finished position")
    if SIZE - board.age > MAX_EMPTIES:
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


def grid_triple(boards: Sequence[Board], device=0, node_budget=None, nodes_per_launch=None, host=False):
    """``[(move, value, tree)]``, what ``grid_search.grid_search(boards, plies=empties, evaluate_centre)`` returns for
    undecided boards with at most MAX_EMPTIES empty squares: GridTree's root and children with their ``absolute_value``s,
    Tree.best_move's tie to the higher column.  Every child of every root is solved as a row of its own in one batch;
    host=True solves them with ``solve_host`` instead (no GPU).  A child the budget leaves UNKNOWN raises RuntimeError."""
    for b in boards:
        _check_root(b)
    kids = [_child_boards(b) for b in boards]
    flat = [cb for ks in kids for _, cb in ks if cb.result is None]
    if host:
        answers = [solve_host(cb, node_budget) for cb in flat]
        status = [a.status for a in answers]
        values = [a.value for a in answers]
    elif flat:
        res = solve(flat, node_budget, nodes_per_launch, device)
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


def label(boards, node_budget=None, nodes_per_launch=None, device=0):
    """Label positions with their exact outcome: returns ``(LabelledSet, report)``.

    Each distinct position is solved once, together with its up-to-seven children (c4_solve_children_dev lists them) in one
    batch.  value = the outcome (0.0 / 0.5 / 1.0); prior = ``prior_from_children``.  Rows that are unknown, too deep,
    terminal or invalid are dropped, as is a row one of whose children stayed unknown (counted as unknown); the kept rows
    stay in the order of their first occurrence.  report: positions, distinct, labelled, the count per status
    (STATUS_NAMES), nodes (parents and children) and seconds."""
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
        batch = torch.cat([uniq, children.reshape(n * WIDTH, 2)]).contiguous()
        status, outcome, _, nodes = _solve_dev(batch, node_budget, nodes_per_launch)
        p_status, p_out = status[:n], outcome[:n]
        c_status, c_out = status[n:].reshape(n, WIDTH), outcome[n:].reshape(n, WIDTH)
        is_legal = legal != 0
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
    report.update({name: int(counts[code]) for code, name in STATUS_NAMES.items()})
    report["seconds"] = time.perf_counter() - t0
    return ls, report
