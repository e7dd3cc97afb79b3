#!/usr/bin/env python3
"""Generate tests/golden/review.npz: seeded games as move lists and their review against exact play, labelled from the
exhaustive oracle alone (oracle/c4_oracle.c c4o_exact_scores through ``oracle.c4oracle.Exact.scores``), which shares no
rule with the solver.

    PYTHONPATH=<repo> python tests/golden/gen_review_golden.py

Games.  N_GAMES = 257 games played on the oracle's board, three kinds interleaved (game k is of kind k % 3):
  (a) uniformly random legal moves;
  (b) "win-averse": uniformly among the legal moves that do not end the game at once, when there is one (stone 42 is
      allowed): these run long and end in draws and late wins;
  (c) as (b) until 16 empty squares are left, then every move chosen by the oracle to keep the outcome, the highest column
      on ties: their reviewed tail must show no blunder.
Three games are then moved to the front -- the first 42-ply draw, the first o win of at most MIN_SHORT plies (shorter than
every cut-off below: no late row at 16 empty squares) and the first x win -- so that the batches of 3, 65 and 257 games (the
first so many; BATCHES) each hold every result, a game shorter than the cut-off and a game of 42 plies.  The batch of one game
is the 42-ply draw alone.

Labels.  For every position with at most 16 empty squares the oracle's score and child scores; from the sign of the score and
the parity of the age the absolute outcome (C4_RESULT_*: 0 x win, 1 draw, 2 o win).  For every E in EMPTIES the rule of
connect4_amd/review.py, written out here a second time and fed by the oracle alone: outcome_eE, kept_eE, target_agrees_eE
(per position of the 257 games; a batch's are the first so many), per_game_eE [257, 4] and, per batch, by_ply_eE_gB [42, 7].
keep bool [n, 7]: the legal moves whose child score has the sign of the position's (all False above 16 empty squares).

From the host mirror (``review.review_host``, table-free) and pinned by nothing else, as elsewhere in this project: nodes_e16,
the per-position node counts at E = 16 (a position's count at a smaller E is the same, or 0 where it is not late), and
status_e20_b64, the statuses of the first 65 games at E = 20 under a node budget of 64.  The generator also asserts that the
mirror's every other array, its keep masks (moves=True) included, equals the oracle's labels, for every E and batch.

The figures the generator prints are copied into tests/review_cases.py.  It takes about 20 s: 2 s of oracle, the rest mirror.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED = 3113
N_GAMES = 257
BATCHES = (1, 3, 65, 257)
EMPTIES = (1, 8, 12, 16)
ORACLE_EMPTIES = 16
MIN_SHORT = 26          # plies of a game without a position of at most 16 empty squares
TIGHT = (20, 64, 65)    # max_empties, node budget, games of status_e20_b64
NO_MOVE = -128


def play(kind, rng, oc, memo):
    b = oc.Board.empty()
    rows, moves = [], []
    while b.result == oc.NONE:
        mask = b.valid_mask()
        legal = [c for c in range(7) if (mask >> c) & 1]
        if kind == 0:
            mv = int(rng.choice(legal))
        elif kind == 2 and 42 - b.age <= ORACLE_EMPTIES:
            score, child, _ = memo.scores([b.key()[0]], [b.key()[1]])
            keeping = [c for c in legal if np.sign(int(child[0, c])) == np.sign(int(score[0]))]
            mv = max(keeping)
        else:
            safe = []
            for c in legal:
                nb = b.copy()
                nb.make_move(c)
                if nb.result == oc.NONE:
                    safe.append(c)
            mv = int(rng.choice(safe or legal))
        rows.append(b.key())
        moves.append(mv)
        b.make_move(mv)
    return rows, moves, int(b.result)


def popcount(x):
    return np.array([bin(int(v)).count("1") for v in x], dtype=np.int64)


def review_by_oracle(ages, game_index, results, outcome16, max_empties, n_games):
    """The rule on the oracle's outcomes: (outcome, kept, target_agrees, by_ply, per_game) of the first n_games games."""
    pick = game_index < n_games
    ages, gi, out16 = ages[pick], game_index[pick], outcome16[pick]
    n = len(ages)
    late = 42 - ages <= max_empties
    outcome = np.where(late, out16, -1).astype(np.int8)
    kept = np.full(n, -1, dtype=np.int8)
    agrees = np.zeros(n, dtype=np.int8)
    by_ply = np.zeros((42, 7), dtype=np.int64)
    per_game = np.zeros((n_games, 4), dtype=np.int32)
    per_game[:, 3] = -1
    for i in range(n):
        if not late[i]:
            continue
        g, a, o = int(gi[i]), int(ages[i]), int(outcome[i])
        nxt = int(outcome[i + 1]) if i + 1 < n and gi[i + 1] == g else int(results[g])
        by_ply[a, 0] += 1
        per_game[g, 0] += 1
        if o >= 0:
            by_ply[a, 1] += 1
            if o == results[g]:
                agrees[i] = 1
                by_ply[a, 5] += 1
        if o >= 0 and nxt >= 0:
            kept[i] = 1 if o == nxt else 0
            by_ply[a, 2] += 1
            per_game[g, 1] += 1
            if o == nxt:
                by_ply[a, 3] += 1
            else:
                by_ply[a, 4] += 1
                per_game[g, 2] += 1
                per_game[g, 3] = max(per_game[g, 3], a)
                # o moves at even ages and gains by a larger code
                if (nxt < o) if a & 1 else (nxt > o):
                    by_ply[a, 6] += 1
    return outcome, kept, agrees, by_ply, per_game


def main():
    from oracle import c4oracle as oc
    import review_cases as RC
    from connect4_amd.review import review_host
    oc.build()
    t0 = time.perf_counter()
    rng = np.random.RandomState(SEED)
    with oc.Exact(26) as memo:
        games = [play(k % 3, rng, oc, memo) + (k % 3,) for k in range(N_GAMES)]
        front = [next(k for k, g in enumerate(games) if len(g[1]) == 42 and g[2] == oc.DRAW),
                 next(k for k, g in enumerate(games) if len(g[1]) <= MIN_SHORT and g[2] == oc.OWIN),
                 next(k for k, g in enumerate(games) if g[2] == oc.XWIN)]
        games = [games[k] for k in front] + [g for k, g in enumerate(games) if k not in front]
        boards = np.array([r for g in games for r in g[0]], dtype=np.uint64).reshape(-1, 2)
        moves = np.array([m for g in games for m in g[1]], dtype=np.uint8)
        lengths = np.array([len(g[1]) for g in games], dtype=np.int32)
        results = np.array([g[2] for g in games], dtype=np.int8)
        kinds = np.array([g[3] for g in games], dtype=np.int8)
        game_index = np.repeat(np.arange(N_GAMES, dtype=np.int32), lengths)
        ages = popcount(boards[:, 0] | boards[:, 1])
        deep = 42 - ages <= ORACLE_EMPTIES
        score, child, status = memo.scores(boards[deep, 0], boards[deep, 1])
        assert (status == oc.EXACT_SEARCHED).all()
    t_oracle = time.perf_counter() - t0
    n = len(boards)
    sign = np.sign(score.astype(np.int64))
    outcome16 = np.full(n, -1, dtype=np.int8)
    outcome16[deep] = np.where(ages[deep] & 1, -sign, sign) + 1
    keep = np.zeros((n, 7), dtype=bool)
    keep[deep] = (child != NO_MOVE) & (np.sign(child.astype(np.int64)) == sign[:, None])

    out = {"boards": boards, "moves": moves, "lengths": lengths, "results": results, "kinds": kinds, "game_index": game_index, "keep": keep,
           "batches": np.array(BATCHES, dtype=np.int64), "empties": np.array(EMPTIES, dtype=np.int64), "tight": np.array(TIGHT, dtype=np.int64)}
    for e in EMPTIES:
        for b in BATCHES:
            outcome, kept, agrees, by_ply, per_game = review_by_oracle(ages, game_index, results, outcome16, e, b)
            out["by_ply_e%d_g%d" % (e, b)] = by_ply
        out["outcome_e%d" % e], out["kept_e%d" % e], out["target_agrees_e%d" % e], out["per_game_e%d" % e] = outcome, kept, agrees, per_game

    # the mirror: node counts and the statuses under a tight budget; everything else must be what the oracle says
    t1 = time.perf_counter()
    z = {k: np.asarray(v) for k, v in out.items()}
    max_nodes = 0
    for e in EMPTIES:
        for b in BATCHES:
            r = review_host(RC.games_of(z, b), max_empties=e, moves=True)
            m = int(lengths[:b].sum())
            want_keep, late = RC.expected_keep(z, e, b)
            assert (r.keep.numpy() == want_keep).all() and (r.keep_known.numpy() == late).all(), ("keep", e, b)
            for name, got in (("outcome", r.outcome), ("kept", r.kept), ("target_agrees", r.target_agrees)):
                assert (got.numpy() == out["%s_e%d" % (name, e)][:m]).all(), (name, e, b)
            assert (r.by_ply.numpy() == out["by_ply_e%d_g%d" % (e, b)]).all(), (e, b)
            assert (r.per_game.numpy() == out["per_game_e%d" % e][:b]).all(), (e, b)
            if e == ORACLE_EMPTIES and b == N_GAMES:
                out["nodes_e16"] = r.nodes.numpy().astype(np.int64)
                max_nodes = int(r.nodes.max())
    tight = review_host(RC.games_of(z, TIGHT[2]), max_empties=TIGHT[0], node_budget=TIGHT[1])
    out["status_e20_b64"] = tight.status.numpy().astype(np.int8)
    t_mirror = time.perf_counter() - t1
    np.savez_compressed(os.path.join(HERE, "review.npz"), **out)

    print("games %d positions %d; results x/draw/o %s; kinds %s; 42-ply games %d" % (
        N_GAMES, n, np.bincount(results, minlength=3).tolist(), np.bincount(kinds).tolist(), int((lengths == 42).sum())))
    for e in EMPTIES:
        for b in BATCHES:
            t = out["by_ply_e%d_g%d" % (e, b)].sum(axis=0)
            with_late = int((out["per_game_e%d" % e][:b, 0] > 0).sum())
            print("E=%2d games=%3d: late %4d kept %4d blunders %4d agrees %4d contradictions %d; games with late rows %d" % (
                e, b, t[0], t[3], t[4], t[5], t[6], with_late))
    c_tail = out["per_game_e16"][kinds == 2]
    print("kind (c): %d games, blunders in their reviewed tails at E=16: %d" % (len(c_tail), int(c_tail[:, 2].sum())))
    print("mirror: most nodes of a row at E=16: %d; E=%d budget %d over %d games: %d of %d late rows UNKNOWN" % (
        max_nodes, TIGHT[0], TIGHT[1], TIGHT[2], int((out["status_e20_b64"] == 2).sum()), int((out["status_e20_b64"] != 3).sum())))
    print("oracle %.1f s, mirror %.1f s; review.npz %d bytes" % (t_oracle, t_mirror, os.path.getsize(os.path.join(HERE, "review.npz"))))


if __name__ == "__main__":
    main()
