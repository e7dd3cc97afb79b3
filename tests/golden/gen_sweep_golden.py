#!/usr/bin/env python3
"""Generate tests/golden/search_sweep.json by importing the UNMODIFIED reference (conventions of gen_golden.py).

Runs where the reference is available only:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 \
      PYTHONPATH=<repo>/oracle/refshim:<reference> python <repo>/tests/golden/gen_sweep_golden.py

What is written (data only: inputs + expected outputs, no reference source text):
  evaluator_outputs  raw answers of tests/sweep_evaluators.py as bit patterns (a later change to that file is noticed)
  configs            the 16 (pb_c_base, pb_c_init) pairs; simulations and the noise fraction cycle over their value sets
  searches           mcts.search per (config, evaluator kind, position): what gen_golden.py's tree_summary records, the
                     chosen child's value, the two principal variations of the reference's tree (Tree.best_move /
                     Tree.most_visited followed from the root: moves and visit counts), and how many select_child calls
                     met an exact tie of the best score (`tie_steps` of `descent_steps`)
  games              training_game() with recorded RNG tapes

Root noise rows are not NumPy's draws: np.random.gamma is replaced by designed rows (exact zeros on legal columns, one
entry of 1e300 or 1e-300, a row that is zero except on one legal column), never all zero on the legal columns.
"""
import json
import os
import sys
from copy import copy

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))

import sweep_evaluators as SE  # noqa: E402

import oinkoink.mcts as ref_mcts  # noqa: E402
from oinkoink.board import Board  # noqa: E402
from oinkoink.evaluators import Evaluator  # noqa: E402
from oinkoink.mcts import MCTS, MCTSConfig, search  # noqa: E402
from oinkoink.neural.training_game import training_game  # noqa: E402
from oinkoink.utils import Side  # noqa: E402

SIMS = (1, 2, 3, 7, 8, 9, 64, 65, 200)
BASES = (1, 50, 19652, 10 ** 9)
INITS = (-0.5, 0.0, 1.25, 4.0)
FRACS = (0.0, 0.25, 0.5, 1.0)          # 0.0: noise off
ALPHA = 0.3
POSITIONS_PER_CONFIG = 3


def res_code(r):
    return None if r is None else float(r.value)


def board_dict(b):
    return dict(c0=int(b.color[0]), c1=int(b.color[1]), age=int(b.age))


def ref_evaluator(kind):
    fn = SE.make(kind)
    return Evaluator(lambda board: fn(int(board.color[0]), int(board.color[1])))


# ---------------------------------------------------------------- positions
def playout(rng, plies):
    """A random legal playout of `plies` moves, or None when the game ended on the way."""
    b = Board()
    for _ in range(plies):
        if b.result is not None:
            return None
        b.make_move(int(rng.choice(sorted(b.valid_moves))))
    return b if b.result is None else None


def mover_wins_with(b, m):
    c = copy(b)
    c.make_move(m)
    return c.result is not None and c.result.value == (1.0 if b.player_to_move == Side.o else 0.0)


def has_win(b):
    return any(mover_wins_with(b, m) for m in b.valid_moves)


def forced_loss(b):
    """The mover cannot win at once, and whatever they play the opponent wins at once."""
    if has_win(b):
        return False
    for m in b.valid_moves:
        c = copy(b)
        c.make_move(m)
        if c.result is not None or not has_win(c):
            return False
    return True


def make_positions():
    rng = np.random.RandomState(20260)
    pool = []
    while len(pool) < 24:
        b = playout(rng, int(rng.randint(0, 39)))
        if b is not None:
            pool.append(("random%d" % len(pool), b))
    pool[0] = ("empty", Board())
    wanted = dict(one_legal=lambda b: len(b.valid_moves) == 1 and b.age < 41, winning_move=has_win,
                  forced_loss=forced_loss, last_move=lambda b: b.age == 41)
    found = {k: [] for k in wanted}
    while any(len(v) < 4 for v in found.values()):
        b = playout(rng, int(rng.randint(6, 42)))
        if b is None:
            continue
        for k, pred in wanted.items():
            if len(found[k]) < 4 and pred(b) and all(board_dict(b) != board_dict(o) for _, o in found[k]):
                found[k].append(("%s%d" % (k, len(found[k])), b))
                break
    for k in wanted:
        pool.extend(found[k])
    return pool


# ---------------------------------------------------------------- noise rows
def noise_row(rng, board, pattern):
    legal = sorted(board.valid_moves)
    row = rng.gamma(ALPHA, 1, 7)
    pick = legal[int(rng.randint(len(legal)))]
    if pattern == 1 and len(legal) > 1:          # exact zeros on some legal columns, never on all of them
        for c in legal:
            if c != pick and rng.randint(2):
                row[c] = 0.0
        row[legal[0] if legal[0] != pick else legal[1]] = 0.0
    elif pattern == 2:
        row[pick] = 1e300
    elif pattern == 3:
        row[pick] = 1e-300
    elif pattern == 4:                           # zero everywhere except one legal column
        row[:] = 0.0
        row[pick] = 2.5
    assert sum(row[c] for c in legal) > 0.0
    return row


# ---------------------------------------------------------------- recording
class Recorder:
    """Feeds np.random.gamma from `rows` (or lets NumPy draw when rows is None), records what it returned, which uniform
    np.random.choice consumed, and the exact score ties that select_child met."""

    def __init__(self, rows=None):
        self.rows = rows

    def __enter__(self):
        self.noise, self.uniforms, self.tie_steps, self.descent_steps = [], [], 0, 0
        self._g, self._c, self._s = np.random.gamma, np.random.choice, ref_mcts.select_child

        def gamma(*a, **k):
            r = self._g(*a, **k) if self.rows is None else np.array(self.rows.pop(0), dtype=np.float64)
            self.noise.append([float(x) for x in np.asarray(r).reshape(-1)])
            return r

        def choice(*a, **k):
            replica = np.random.RandomState()
            replica.set_state(np.random.get_state())
            self.uniforms.append(float(replica.random_sample()))
            return self._c(*a, **k)

        def select_child(config, tree, node):
            scores = [float(ref_mcts.ucb_score(config, node, c)) for c in node.children]
            self.descent_steps += 1
            self.tie_steps += scores.count(max(scores)) > 1
            return self._s(config, tree, node)
        np.random.gamma, np.random.choice, ref_mcts.select_child = gamma, choice, select_child
        return self

    def __exit__(self, *exc):
        np.random.gamma, np.random.choice, ref_mcts.select_child = self._g, self._c, self._s


def cfg_dict(c):
    return dict(simulations=c.simulations, pb_c_base=c.pb_c_base, pb_c_init=c.pb_c_init,
                root_dirichlet_alpha=c.root_dirichlet_alpha, root_exploration_fraction=c.root_exploration_fraction,
                num_sampling_moves=c.num_sampling_moves)


def line(tree, rule):
    """Tree.best_move (for the side to move at every node) or Tree.most_visited, followed from the root."""
    moves, visits = [], []
    node = tree.root
    while node.children:
        side = node.data.board.player_to_move
        if rule == "value":
            _, node = max((c.data.value(side), c) for c in node.children)
        else:
            _, node = max((c.data.search_value.visit_count if c.data.search_value is not None else 0, c) for c in node.children)
        moves.append(int(node.name))
        visits.append(0 if node.data.search_value is None else int(node.data.search_value.visit_count))
    return dict(moves=moves, visits=visits)


def tree_summary(tree):
    root = tree.root
    N, W, status, val = [0] * 7, [0.0] * 7, [-2] * 7, [0.0] * 7
    for c in root.children:
        sv = c.data.search_value
        N[c.name] = 0 if sv is None else int(sv.visit_count)
        W[c.name] = 0.0 if sv is None else float(sv.value_sum)
        status[c.name] = -1 if c.data.board.result is None else int(c.data.board.result.value * 2)
        val[c.name] = float(tree.get_node_value(c))
    n_nodes = n_exp = 0
    stack = [root]
    while stack:
        n = stack.pop()
        n_nodes += 1
        if n.children:
            n_exp += 1
            stack.extend(n.children)
    best = tree.best_move()
    return dict(root_N=int(root.data.search_value.visit_count), root_W=float(root.data.search_value.value_sum),
                N=N, W=W, status=status, child_value=val,
                values_policy=[float(x) for x in tree.get_values_policy()],
                visit_policy=[float(x) for x in tree.get_visit_count_policy()],
                root_prior=[float(x) for x in root.data.position_value.prior],
                best_move=int(best.name), value=best.data.absolute_value, n_nodes=n_nodes, n_expansions=n_exp,
                pv_value=line(tree, "value"), pv_visits=line(tree, "visits"))


# ---------------------------------------------------------------- searches
def make_configs():
    """All 16 (base, init) pairs; simulations and the fraction cycle so that each of their values occurs."""
    out = []
    for i, (base, init) in enumerate((b, a) for b in BASES for a in INITS):
        frac = FRACS[(i + i // 4) % 4]
        out.append(MCTSConfig(SIMS[i % len(SIMS)], pb_c_base=base, pb_c_init=init,
                              root_dirichlet_alpha=ALPHA if frac else 0.0, root_exploration_fraction=frac))
    assert {c.simulations for c in out} == set(SIMS) and {c.root_exploration_fraction for c in out} == set(FRACS)
    return out


def dump_searches(configs, positions):
    rng = np.random.RandomState(777)
    cases = []
    nxt = n_noisy = 0
    for k, kind in enumerate(SE.KINDS):
        for ci, cfg in enumerate(configs):
            for j in range(POSITIONS_PER_CONFIG):
                pname, board = positions[nxt % len(positions)]
                nxt += 7                                    # 7 and the pool's size are coprime: every position is used
                noisy = cfg.root_exploration_fraction != 0.0
                rows = [noise_row(rng, board, n_noisy % 5)] if noisy else None
                n_noisy += noisy
                with Recorder(rows) as rec:
                    tree = search(cfg, copy(board), ref_evaluator(kind))
                d = dict(name="%s_c%d_%s" % (kind, ci, pname), kind=kind, cfg=ci, board=board_dict(board),
                         noise=rec.noise[0] if noisy else None, tie_steps=int(rec.tie_steps), descent_steps=int(rec.descent_steps))
                d.update(tree_summary(tree))
                cases.append(d)
    return cases


# ---------------------------------------------------------------- games
GAMES = (("const32", 42, 1.0, 9), ("const32", 0, 0.25, 60), ("quant32", 42, 0.25, 60), ("quant32", 0, 1.0, 9),
         ("sparse32", 42, 1.0, 60), ("sparse32", 0, 0.25, 9))


def dump_games():
    games = []
    for seed, (kind, nsm, frac, sims) in enumerate(GAMES):
        cfg = MCTSConfig(sims, root_dirichlet_alpha=ALPHA, root_exploration_fraction=frac, num_sampling_moves=nsm)
        np.random.seed(4200 + seed)
        with Recorder() as rec:
            gd = training_game(MCTS("ref", cfg, ref_evaluator(kind)))
        games.append(dict(name="game%d_%s" % (seed, kind), kind=kind, seed=4200 + seed, config=cfg_dict(cfg),
                          moves=[int(m) for m in gd.moves],
                          boards=[[int(b.color[0]), int(b.color[1])] for b in gd.boards],
                          values=[None if v is None else float(v) for v in gd.values],
                          policies=[[float(x) for x in p] for p in gd.priors],
                          result=float(gd.result.value), noise_tape=rec.noise, uniforms=rec.uniforms))
    return games


def dump_evaluator_outputs(positions):
    out = []
    for kind in SE.KINDS:
        for _, b in positions[::5]:
            c0, c1 = int(b.color[0]), int(b.color[1])
            vb, pb = SE.output_bits(kind, c0, c1)
            out.append(dict(kind=kind, c0=c0, c1=c1, value_bits=vb, prior_bits=pb))
    return out


def main():
    positions = make_positions()
    assert len(positions) % 7 != 0
    configs = make_configs()
    data = dict(evaluator_outputs=dump_evaluator_outputs(positions), configs=[cfg_dict(c) for c in configs],
                searches=dump_searches(configs, positions), games=dump_games())
    path = os.path.join(OUT, "search_sweep.json")
    with open(path, "w") as f:
        json.dump(data, f, separators=(",", ":"))
    n = len(data["searches"])
    print("search_sweep.json: %d searches, %d games, %d bytes" % (n, len(data["games"]), os.path.getsize(path)))
    for kind in SE.KINDS:
        cs = [c for c in data["searches"] if c["kind"] == kind]
        print("  %-8s %3d searches, %3d with a tied descent step (%.0f%%)" % (
            kind, len(cs), sum(c["tie_steps"] > 0 for c in cs), 100.0 * sum(c["tie_steps"] > 0 for c in cs) / len(cs)))


if __name__ == "__main__":
    main()
