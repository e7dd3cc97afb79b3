"""Finished self-play games reviewed against exact play.

A generation of self-play ends as ``PackedGames``; the last plies of every game are positions the exact solver
(connect4_amd/solver.py, csrc/c4_solve.hip) answers in a few hundred nodes.  ``review_games`` searches the distinct late
positions of a batch once each -- ``c4_solve_window_dev`` with the window (-1, +1), the search ``solver.outcomes`` makes --
and folds the answers along the games on the device (c4_review_select_dev / _outcomes_dev / _fold_dev): nothing per
position goes through Python or NumPy on that path.

The rule.  A game is a run of consecutive rows with one ``game_index``, plies ascending; row i + 1 is the position after
``moves[i]`` on row i, and after the last row's move the game is over with ``results[g]``.  With ``max_empties`` = E a
position is late when it has at most E empty squares; the late positions of a game are a suffix of it.  For a late row i:

  outcome[i]        the exact outcome under best play as C4_RESULT_* (0 x win, 1 draw, 2 o win), absolute; -1 where the
                    node budget leaves the row UNKNOWN
  next[i]           outcome[i + 1] if row i + 1 belongs to the same game, else results[g] (-1: the game carries none)
  kept[i]           1 if outcome[i] and next[i] are both known and equal, 0 if both are known and differ -- a blunder of the
                    side to move at i: best play cannot change the outcome in the mover's favour --, -1 otherwise
  target_agrees[i]  1 if outcome[i] is known and equals results[g]: the value target the position is trained on agrees
                    with its game-theoretic value

A blunder that changes the outcome in the mover's FAVOUR is a contradiction: it is counted separately (and as a blunder,
so that kept + blunders = kept_known), it must be zero, and it is a tripwire for the solver, not a statistic.

The chain is checked, not trusted: the position after ``moves[i]`` (csrc/c4_board.h make_move) must equal row i + 1
exactly, and behind a game's last row it must be finished, with the result ``results[g]`` where that is not -1.  A batch
with a row that fails raises ``ValueError`` naming the first such row; no answer is returned for it.

``review_games``   the review on the device; ``host=True`` / ``review_host``: the same rule in NumPy over ``solve_host``
``GameReview``     the answers: per position, ``by_ply`` int64 [42, 7] (``BY_PLY_COLUMNS``), ``per_game`` int32 [n_games, 4]
                   (``PER_GAME_COLUMNS``), ``report``; ``summary()``, ``labelled_set()``
``PackedGames.with_exact_targets(review)``  the games with the solved late rows' targets replaced by their exact value

``moves=True`` also answers which legal moves keep the outcome (``keep`` bool [n, 7]): ``staged_labels`` as it stands on
the distinct late rows, its stage 1 the search already made, its stage 2 one batch of null-window searches of the children.
From the mask: ``policy_on_kept``, how much of the policy target lies on moves that lose nothing, and the exact priors,
uniform over the keeping moves, that ``with_exact_targets(priors=True)`` trains on.
"""
import ctypes as C
import time

import numpy as np

from . import _lib as L
from . import solver as S
from .board import H1, HEIGHT, SIZE, WIDTH, _wins

__all__ = ["BY_PLY_COLUMNS", "PER_GAME_COLUMNS", "DEFAULT_MAX_EMPTIES", "GameReview", "review_games", "review_host"]

BY_PLY_COLUMNS = L.REVIEW_COLUMNS
PER_GAME_COLUMNS = L.REVIEW_GAME_COLUMNS
# The largest measured E whose table-free review costs under a tenth of its batch's self-play (profiles/review.json, 8,192
# games at 800 simulations on one MI355X: 1.3 % at E = 12, 33 % at E = 16 -- 5.8 % there with a Table(24)).
DEFAULT_MAX_EMPTIES = 12
_COL = {name: i for i, name in enumerate(BY_PLY_COLUMNS)}


class GameReview:
    """What ``review_games`` answers.  Tensors on the games' device (CPU tensors from the host mirror):

      status, outcome, kept, target_agrees   int8 [n_positions]; status is SOLVE_SOLVED, SOLVE_UNKNOWN or, for a position that
                                             is not late, SOLVE_TOO_DEEP: more empty squares than asked for
      nodes            int64 [n_positions]: the node count of the position's distinct row, 0 if it is not late
      by_ply           int64 [42, 7] by the position's age, columns ``BY_PLY_COLUMNS``
      per_game         int32 [n_games, 4], columns ``PER_GAME_COLUMNS``; from last_blunder_age + 1 on the game was played
                       outcome-perfectly as far as the review knows (-1: no blunder)
      exact_targets    float32 [n_positions]: 0.5 * outcome for a late row with a known outcome, the games' target elsewhere
      distinct_boards  int64 [m, 2], the distinct late positions in the order of their first occurrence -- each searched
                       once --, with distinct_status int8 [m] and distinct_outcome int8 [m]
      report           positions, late, distinct, nodes, table_hits, the count per status over the positions (solved,
                       unknown, too_deep), chain_errors, contradictions, max_empties, table_log2_entries, seconds
    and, from a review with moves=True (else None):
      keep             bool [n_positions, 7]: the legal moves that keep the outcome; all False where keep_known is
      keep_known       bool [n_positions]: late, solved, and every child the rule had to search was searched to the end
      policy_on_kept   float32 [n_positions]: the sum, in column order, of the games' policy over keep; NaN where unknown
      exact_priors     float32 [n_positions, 7]: uniform over keep where it is known, the games' policy elsewhere"""

    def __init__(self, max_empties, status, outcome, kept, target_agrees, nodes, by_ply, per_game, exact_targets, distinct_boards,
                 distinct_status, distinct_outcome, report, keep=None, keep_known=None, policy_on_kept=None, exact_priors=None, boards=None):
        self.max_empties = int(max_empties)
        self.status, self.outcome, self.kept, self.target_agrees, self.nodes = status, outcome, kept, target_agrees, nodes
        self.by_ply, self.per_game, self.exact_targets = by_ply, per_game, exact_targets
        self.distinct_boards, self.distinct_status, self.distinct_outcome = distinct_boards, distinct_status, distinct_outcome
        self.report = report
        self.keep, self.keep_known, self.policy_on_kept, self.exact_priors = keep, keep_known, policy_on_kept, exact_priors
        self._boards = boards       # with moves=True: the games' boards, for the ages of summary()'s by-ply means

    @property
    def n_games(self):
        return int(self.per_game.shape[0])

    def summary(self):
        """Plain Python numbers: games, positions, late, max_empties, unknown (late rows without an outcome), blunders,
        contradictions, blunders_per_game, target_agreement (the share of late positions whose target agrees; None without
        late positions), by_side {"o", "x"} with the same two figures and late / blunders / target_agrees for the side to move
        (o moves at even ages), and the by-ply table: by_ply_columns and by_ply, 42 lists of 7.  From a review with moves=True
        also policy_on_kept (the mean over the rows where it is known, None without one), policy_on_kept_rows and
        policy_on_kept_by_ply (42 means, None where an age has no such row): float64 means of the per-position array, formed on
        the host in row order."""
        table = self.by_ply.cpu().numpy().astype(np.int64)
        games = self.n_games

        def part(rows):
            late, blunders, agrees = (int(rows[:, _COL[k]].sum()) for k in ("late", "blunders", "target_agrees"))
            return {"late": late, "blunders": blunders, "target_agrees": agrees,
                    "blunders_per_game": blunders / games if games else None, "target_agreement": agrees / late if late else None}

        out = {"games": games, "positions": int(self.status.shape[0]), "max_empties": self.max_empties}
        out.update(part(table))
        out["unknown"] = int(table[:, _COL["late"]].sum() - table[:, _COL["outcome_known"]].sum())
        out["contradictions"] = int(table[:, _COL["contradictions"]].sum())
        out["by_side"] = {"o": part(table[0::2]), "x": part(table[1::2])}
        out["by_ply_columns"] = list(BY_PLY_COLUMNS)
        out["by_ply"] = [[int(v) for v in row] for row in table]
        if self.policy_on_kept is not None:
            share = self.policy_on_kept.cpu().numpy().astype(np.float64)
            known = ~np.isnan(share)
            ages = S._ages(np.ascontiguousarray(self._boards.cpu().numpy()).view(np.uint64).reshape(-1, 2))
            rows = np.bincount(ages[known], minlength=SIZE)[:SIZE]
            sums = np.bincount(ages[known], weights=share[known], minlength=SIZE)[:SIZE]
            out["policy_on_kept"] = float(share[known].sum() / known.sum()) if known.any() else None
            out["policy_on_kept_rows"] = int(known.sum())
            out["policy_on_kept_by_ply"] = [float(s / r) if r else None for s, r in zip(sums, rows)]
        return out

    def labelled_set(self):
        """The distinct solved late positions as a value-only ``stats.LabelledSet`` (values 0.0 / 0.5 / 1.0), in the order of
        their first occurrence: ``stats.score(net, review.labelled_set())`` says how the value head does on its own endgames."""
        import torch
        from .stats import LabelledSet
        solved = self.distinct_status == L.SOLVE_SOLVED
        return LabelledSet(self.distinct_boards[solved].contiguous(), (self.distinct_outcome[solved].to(torch.float32) * 0.5).contiguous())


def _check_empties(max_empties):
    if isinstance(max_empties, bool) or not float(max_empties).is_integer() or not 0 <= int(max_empties) <= SIZE:
        raise ValueError("max_empties must be a whole number in 0..%d; got %r" % (SIZE, max_empties))
    return int(max_empties)


def _chain_error(row):
    return ValueError("row %d breaks its game's chain: it is no undecided position of a game of the batch, its move is not "
                      "playable, or the position after its move is neither the game's next row nor finished with the game's "
                      "result" % row)


def _report(n, late, distinct, nodes, hits, counts, contradictions, max_empties, table, t0, stage2=None):
    """counts: the positions per status code; stage2: staged_labels' dict of a review with moves=True."""
    report = {"positions": int(n), "late": int(late), "distinct": int(distinct), "nodes": int(nodes), "table_hits": int(hits),
              "chain_errors": 0, "contradictions": int(contradictions), "max_empties": int(max_empties),
              "table_log2_entries": getattr(table, "log2_entries", None)}
    report.update({S.STATUS_NAMES[code]: int(counts[code]) for code in (L.SOLVE_SOLVED, L.SOLVE_UNKNOWN, L.SOLVE_TOO_DEEP)})
    if stage2 is not None:
        report.update({k: stage2[k] for k in ("stage2_rows", "stage2_nodes", "stage2_unknown", "stage2_hits")})
    report["seconds"] = time.perf_counter() - t0
    return report


def _keep_masks(distinct, stage1, solver_fn, children_of=None):
    """``staged_labels`` as it stands on the distinct late rows (uint64 [m, 2]) with its stage 1 answered by the search
    already made -- `stage1` = (status, score, nodes, table_hits) of those rows -- and its stage 2 by `solver_fn`.  Returns
    (keep bool [m, 7], known bool [m], staged_labels' dict)."""
    calls = []

    def solve(rows, alpha, beta):
        calls.append(len(rows))
        return stage1 if len(calls) == 1 else solver_fn(rows, alpha, beta)

    st = S.staged_labels(distinct, solve, children_of)
    known = st["status"] == L.SOLVE_SOLVED
    return st["keep"] & known[:, None], known, st


def _policy_on_kept(policy, keep, known):
    """The float32 sum, in column order, of `policy` [n, 7] over `keep`; NaN where not `known`.  NumPy arrays or tensors."""
    acc = policy[:, 0] * 0
    for c in range(WIDTH):
        acc = acc + policy[:, c] * keep[:, c]       # adding 0.0 changes nothing: the sum runs over the kept columns in order
    acc[~known] = float("nan")
    return acc


# -- the host mirror -------------------------------------------------------------------------------------------------------
def _after_move(c0, c1, col):
    """csrc/c4_board.h make_move on Python ints: (color0, color1, result code or -1) after the mover plays `col`."""
    occ = c0 | c1
    age = bin(occ).count("1")
    bit = 1 << (H1 * col + bin((occ >> (H1 * col)) & 0x7f).count("1"))
    if age & 1:
        c1 ^= bit
        won = _wins(c1)
    else:
        c0 ^= bit
        won = _wins(c0)
    if won:
        return c0, c1, L.RESULT_XWIN if age & 1 else L.RESULT_OWIN
    return c0, c1, L.RESULT_DRAW if age + 1 == SIZE else -1


def review_host(games, max_empties=DEFAULT_MAX_EMPTIES, node_budget=None, table=None, book=None, moves=False):
    """``review_games`` in NumPy over ``solve_host(window=(-1, 1))``: the same rule, no GPU.  Table-free the node counts are
    the kernel's.  table: None, a dict or a ``HostTable`` (``solve_host``'s); book: a ``Book``; moves: ``review_games``'.
    Returns a ``GameReview`` of CPU tensors."""
    import torch
    t0 = time.perf_counter()
    max_empties = _check_empties(max_empties)
    p = games.cpu()
    rows = np.ascontiguousarray(p.boards.numpy()).view(np.uint64).reshape(-1, 2)
    played, gidx, results = p.moves.numpy(), p.game_index.numpy(), p.results.numpy()
    targets = p.targets.numpy()
    n, n_games = len(rows), len(results)
    ages = S._ages(rows)
    kind = np.array([S._classify(int(a), int(b), max_empties) for a, b in rows], dtype=np.int8).reshape(n)
    late = kind == L.SOLVE_SOLVED
    # the chain
    for i in range(n):
        g, mv, c0, c1 = int(gidx[i]), int(played[i]), int(rows[i, 0]), int(rows[i, 1])
        ok = kind[i] in (L.SOLVE_SOLVED, L.SOLVE_TOO_DEEP) and 0 <= g < n_games and mv < WIDTH
        ok = ok and -1 <= int(results[g]) <= L.RESULT_OWIN and bin(((c0 | c1) >> (H1 * mv)) & 0x7f).count("1") < HEIGHT
        if ok:
            n0, n1, after = _after_move(c0, c1, mv)
            if i + 1 < n and int(gidx[i + 1]) == g:
                ok = after < 0 and (int(rows[i + 1, 0]), int(rows[i + 1, 1])) == (n0, n1)
            else:
                ok = after >= 0 and int(results[g]) in (-1, after)
        if not ok:
            raise _chain_error(i)
    # every distinct late position once
    distinct = S._first_occurrences(rows[late])
    index = {(int(a), int(b)): k for k, (a, b) in enumerate(distinct)}
    answers = [S.solve_host((int(a), int(b)), node_budget, table=table, window=(-1, 1), book=book) for a, b in distinct]
    d_status = np.array([a.status for a in answers], dtype=np.int8).reshape(len(distinct))
    d_score = np.array([a.score for a in answers], dtype=np.int64).reshape(len(distinct))
    d_nodes = np.array([a.nodes for a in answers], dtype=np.int64).reshape(len(distinct))
    d_hits = sum(int(a.hits) for a in answers)
    sign = np.sign(d_score)
    d_outcome = np.where(d_status == L.SOLVE_SOLVED, np.where(S._ages(distinct) & 1, -sign, sign) + 1, -1).astype(np.int8)
    row_of = np.array([index[(int(a), int(b))] for a, b in rows[late]], dtype=np.int64)
    status = np.full(n, L.SOLVE_TOO_DEEP, dtype=np.int8)
    outcome = np.full(n, -1, dtype=np.int8)
    nodes = np.zeros(n, dtype=np.int64)
    status[late], outcome[late], nodes[late] = d_status[row_of], d_outcome[row_of], d_nodes[row_of]
    # the fold
    result = results[gidx].astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    has_next = np.zeros(n, dtype=bool)
    has_next[:-1] = gidx[1:] == gidx[:-1]
    nxt = np.where(has_next, np.roll(outcome, -1), result).astype(np.int64) if n else result
    o = outcome.astype(np.int64)
    both = late & (o >= 0) & (nxt >= 0)
    kept = np.where(both, (o == nxt).astype(np.int8), -1).astype(np.int8)
    agrees = (late & (o >= 0) & (o == result)).astype(np.int8)
    contradiction = (kept == 0) & np.where(ages & 1, nxt < o, nxt > o)
    by_ply = np.zeros((SIZE, len(BY_PLY_COLUMNS)), dtype=np.int64)
    for name, mask in (("late", late), ("outcome_known", late & (o >= 0)), ("kept_known", kept >= 0), ("kept", kept == 1),
                       ("blunders", kept == 0), ("target_agrees", agrees == 1), ("contradictions", contradiction)):
        by_ply[:, _COL[name]] = np.bincount(ages[mask], minlength=SIZE)[:SIZE]
    per_game = np.zeros((n_games, len(PER_GAME_COLUMNS)), dtype=np.int32)
    per_game[:, 3] = -1
    for col, mask in enumerate((late, kept >= 0, kept == 0)):
        per_game[:, col] = np.bincount(gidx[mask], minlength=n_games)
    if (kept == 0).any():
        np.maximum.at(per_game[:, 3], gidx[kept == 0], ages[kept == 0].astype(np.int32))
    exact = np.where(late & (o >= 0), o.astype(np.float32) * np.float32(0.5), targets).astype(np.float32)
    t = torch.from_numpy
    extra, stage2 = {}, None
    if moves:
        d_keep, d_known, stage2 = _keep_masks(distinct, (d_status, d_score.astype(np.int8), d_nodes, np.zeros_like(d_nodes)),
                                              S._window_solver(node_budget, None, 0, table, True, book=book))
        keep = np.zeros((n, WIDTH), dtype=bool)
        known = np.zeros(n, dtype=bool)
        keep[late], known[late] = d_keep[row_of], d_known[row_of]
        policy = p.policy.numpy()
        count = keep.sum(axis=1)
        priors = np.where((count > 0)[:, None], keep / np.maximum(count, 1).astype(np.float32)[:, None], policy).astype(np.float32)
        extra = dict(keep=t(keep), keep_known=t(known), policy_on_kept=t(_policy_on_kept(policy, keep.astype(np.float32), known)),
                     exact_priors=t(priors), boards=p.boards)
    counts = np.bincount(status.astype(np.int64), minlength=len(S.STATUS_NAMES))
    report = _report(n, late.sum(), len(distinct), d_nodes.sum(), d_hits, counts, contradiction.sum(), max_empties, table, t0, stage2)
    return GameReview(max_empties, t(status), t(outcome), t(kept), t(agrees), t(nodes), t(by_ply), t(per_game), t(exact),
                      t(np.ascontiguousarray(distinct).view(np.int64).reshape(-1, 2)), t(d_status), t(d_outcome), report, **extra)


# -- the device --------------------------------------------------------------------------------------------------------------
def _review_dev(games, max_empties, node_budget, nodes_per_launch, table, moves):
    import torch
    t0 = time.perf_counter()
    dev = games.boards.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    n, n_games = games.n_positions, games.n_games
    lib = L.load()
    ptr = S._ptr
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        boards = games.boards.contiguous()
        played, gidx, results, targets = (x.contiguous() for x in (games.moves, games.game_index, games.results, games.targets))
        late = torch.zeros(n, dtype=torch.uint8, device=dev)
        S._check(lib.c4_review_select_dev(idx, stream, ptr(boards), n, max_empties, ptr(late)))
        # the distinct late rows in the order of their first occurrence, as solver.label orders them
        at = torch.nonzero(late).reshape(-1)
        n_late = int(at.numel())
        row_of = torch.full((n,), -1, dtype=torch.int64, device=dev)
        if n_late:
            uniq, inverse = torch.unique(boards[at], dim=0, return_inverse=True)
            first = torch.full((uniq.shape[0],), n_late, dtype=torch.int64, device=dev)
            first.scatter_reduce_(0, inverse, torch.arange(n_late, device=dev), reduce="amin")
            order = torch.argsort(first)
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.numel(), device=dev)
            uniq = uniq[order].contiguous()
            row_of[at] = rank[inverse]
        else:
            uniq = boards[:0].contiguous()
        m = int(uniq.shape[0])
        # one search a distinct row, the window (-1, +1)
        d_status, _, _, d_nodes, d_hits, d_score, _ = S._solve_dev(uniq, node_budget, nodes_per_launch, table,
                                                                   window=(np.full(m, -1, dtype=np.int8), np.full(m, 1, dtype=np.int8)))
        status, outcome, kept, agrees = (torch.empty(n, dtype=torch.int8, device=dev) for _ in range(4))
        nodes = torch.empty(n, dtype=torch.int64, device=dev)
        S._check(lib.c4_review_outcomes_dev(idx, stream, ptr(boards), ptr(late), ptr(row_of), n, ptr(d_status), ptr(d_score), ptr(d_nodes), m,
                                            ptr(status), ptr(outcome), ptr(nodes)))
        extra, stage2, keep8, known8, policy, priors = {}, None, None, None, None, None
        if moves:       # stage 2 of the labelling rule: host book-keeping around one more batch of searches on the device
            stage1 = tuple(x.cpu().numpy() for x in (d_status, d_score, d_nodes, d_hits))
            d_keep, d_known, stage2 = _keep_masks(np.ascontiguousarray(uniq.cpu().numpy()).view(np.uint64).reshape(-1, 2), stage1,
                                                  S._window_solver(node_budget, nodes_per_launch, idx, table, False), S._children_of(idx))
            keep8 = torch.zeros((n, WIDTH), dtype=torch.uint8, device=dev)
            known8 = torch.zeros(n, dtype=torch.uint8, device=dev)
            if n_late:
                keep8[at] = torch.from_numpy(d_keep.astype(np.uint8)).to(dev)[row_of[at]]
                known8[at] = torch.from_numpy(d_known.astype(np.uint8)).to(dev)[row_of[at]]
            policy = games.policy.contiguous()
            priors = torch.empty((n, WIDTH), dtype=torch.float32, device=dev)
        by_ply = torch.empty((SIZE, len(BY_PLY_COLUMNS)), dtype=torch.int64, device=dev)
        per_game = torch.empty((n_games, len(PER_GAME_COLUMNS)), dtype=torch.int32, device=dev)
        errors = torch.empty(2, dtype=torch.int32, device=dev)      # the count, the first row
        exact = torch.empty(n, dtype=torch.float32, device=dev)
        S._check(lib.c4_review_fold_dev(idx, stream, ptr(boards), ptr(played), ptr(gidx), ptr(results), n, n_games, ptr(outcome), ptr(late),
                                        ptr(targets), ptr(kept), ptr(agrees), ptr(by_ply), ptr(per_game), ptr(errors[:1]), ptr(errors[1:]),
                                        ptr(exact), ptr(keep8), ptr(known8), ptr(policy), ptr(priors)))
        n_errors, first_error = (int(x) for x in errors.cpu().tolist())
        if n_errors:
            raise _chain_error(first_error)
        d_outcome = torch.full((m,), -1, dtype=torch.int8, device=dev)
        if n_late:
            d_outcome[row_of[at]] = outcome[at]     # rows of one position carry one outcome
        counts = torch.bincount(status.long(), minlength=len(S.STATUS_NAMES)).cpu().tolist()
        report = _report(n, n_late, m, d_nodes.sum().item() if m else 0, d_hits.sum().item() if m else 0, counts,
                         by_ply[:, _COL["contradictions"]].sum().item(), max_empties, table, t0, stage2)
        if moves:
            extra = dict(keep=keep8 != 0, keep_known=known8 != 0, policy_on_kept=_policy_on_kept(policy, keep8.to(torch.float32), known8 != 0),
                         exact_priors=priors, boards=boards)
    return GameReview(max_empties, status, outcome, kept, agrees, nodes, by_ply, per_game, exact, uniq, d_status, d_outcome, report, **extra)


def review_games(games, max_empties=DEFAULT_MAX_EMPTIES, node_budget=None, nodes_per_launch=None, table=None, book=None, moves=False,
                 host=False):
    """Review a batch of finished games (``PackedGames``) against exact play: a ``GameReview``.

    max_empties: 0..42, the positions with at most that many empty squares are reviewed (0: none, 42: every row).
    node_budget / nodes_per_launch: ``solve_window``'s -- a row over the budget stays UNKNOWN, and kept is -1 wherever either
    side of it is unknown; the launch quota changes no answer and, table-free, no node count.  table: a ``Table`` on the
    games' device, shared as everywhere: no answer depends on it, node counts do.  book: a ``Book``, probed where the search
    reaches its ply.  moves=True: also ``keep``, ``policy_on_kept`` and ``exact_priors`` (``GameReview``): ``staged_labels`` on the
    distinct late rows, stage 1 the search already made, stage 2 one more batch on the device with NumPy book-keeping on the
    host.  host=True: ``review_host`` (table: None, a dict or a ``HostTable``; no GPU; CPU tensors).

    On the device the games must live on a cuda device: there is no CPU fallback.  Each distinct late position is searched
    once (mirror images are not merged).  Raises ValueError for max_empties outside 0..42, games on the CPU without
    host=True, a table on another device, and a batch whose chain is broken (the message names the first such row)."""
    max_empties = _check_empties(max_empties)
    if host:
        return review_host(games, max_empties, node_budget, table, book, moves)
    dev = games.boards.device
    if dev.type != "cuda":
        raise ValueError("the review runs on the GPU (c4_review_*_dev) and the games are on %s: move them to a cuda device, or "
                         "ask for host=True" % dev)
    import torch
    n, n_games = games.n_positions, games.n_games
    layout = (("boards", torch.int64, (n, 2)), ("moves", torch.uint8, (n,)), ("targets", torch.float32, (n,)), ("policy", torch.float32, (n, 7)),
              ("game_index", torch.int32, (n,)),
              ("results", torch.int8, (n_games,)))
    for name, dtype, shape in layout:      # the kernels index by these shapes
        t = getattr(games, name)
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev:
            raise ValueError("games.%s must be %s %s on %s; got %s %s on %s" % (name, dtype, list(shape), dev, t.dtype, list(t.shape), t.device))
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    if table is not None and table.device != index:
        raise ValueError("the table lives on device %d, the games on device %d" % (table.device, index))
    if book is not None:
        with S._carrying(table, book, index) as carrier:
            return _review_dev(games, max_empties, node_budget, nodes_per_launch, carrier, moves)
    return _review_dev(games, max_empties, node_budget, nodes_per_launch, table, moves)
