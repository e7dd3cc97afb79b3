#!/usr/bin/env python3
"""Generate tests/golden/net_parity.json and net_parity_tables.npz: the reference's own searches with
data/example_net.pth at the production simulation count, and for each of them whether the reference DECIDES it by a
margin or whether it is a near-tie that rounding in the last bits of the net's answers may turn.

Like gen_golden.py this imports the UNMODIFIED reference over oracle/refshim and runs in the build container only:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 \
      PYTHONPATH=<repo>/oracle/refshim:<reference> python <repo>/tests/golden/gen_net_parity_golden.py

Everything written is data (inputs + expected outputs, no reference source text).  A re-run reproduces both files byte
for byte (torch on one thread; the npz is written with fixed zip timestamps).

Cases (each recorded with tree_summary / cfg_dict / board_dict exactly as search_net.json is):
  family A  48 seeded random undecided positions, ages spread over 0..33, mcts.search with 800 simulations, no noise;
            four of them (A_S3200) also with 3200 simulations.
  family B  every ply of three training_game()s (800 simulations, alpha 0.3, fraction 0.25, 6 sampling moves;
            np.random.seed 0, 1, 2).  The reference searches every ply from scratch (mcts.py:78-88), so a ply is one
            independent search: the board before the move, that ply's gamma draws, the uniform np.random.choice consumed
            (plies 0..5), the move the reference made, its GameData.priors row and value.

`decided`, per case, from the reference's answers alone: the case is searched again K times on the CPU oracle
(oracle/c4_oracle.c -- asserted here to reproduce every case's visit counts, and bit-exact to the reference on every
fixture of tests/test_oracle_golden.py), with the same noise tape, while every evaluator answer -- the value and each
of the 7 priors, float32 -- is moved by uniform(-EPS, EPS), EPS = 16 x 9 x 2^-22 = tests/net_models.tol_f32x3(3), the
tolerance the f32x3 forward of this 3-block net is held to against float64.  The amounts are a hash of (position key,
draw), so a position is moved by the same amount wherever a search meets it.  (A moved value is kept inside [0, 1] and a
moved prior at or above 0: what every evaluator guarantees.)  decided = all K child-visit vectors equal the unperturbed
one; self_tv = the largest total-variation distance of the K visit distributions from it.  K = 6.

Cap (a condition, not a tolerance): at least half of family A and at least half of family B must be decided, else the
fixture separates nothing; asserted below, both shares recorded in the JSON.

Tables: the evaluator's position_table (c0, c1, float32 value, float32 priors, as gen_golden.table_arrays) of the first
eight cases of family A and of every fourth ply of each game -- asserted to hold decided and undecided cases.
"""
import io
import json
import os
import sys
import zipfile
from copy import copy
from functools import partial

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, REPO)
sys.path.insert(0, OUT)

import torch  # noqa: E402

from gen_golden import GammaRecorder, board_dict, cfg_dict, random_position, table_arrays, tree_summary  # noqa: E402
from oinkoink.board import Board  # noqa: E402
from oinkoink.evaluators import Evaluator, evaluate_nn  # noqa: E402
from oinkoink.mcts import MCTS, MCTSConfig, search  # noqa: E402
from oinkoink.neural.config import ModelConfig  # noqa: E402
from oinkoink.neural.pytorch.model import ModelWrapper  # noqa: E402
from oinkoink.neural.training_game import training_game  # noqa: E402
from oracle import c4oracle as oc  # noqa: E402

REF = os.path.dirname(os.path.dirname(os.path.abspath(sys.modules["oinkoink"].__file__)))

EPS = 16 * 9 * 2.0 ** -22       # tests/net_models.tol_f32x3(3); test_net_parity_fixture.py checks the two agree
K = 6
N_A, AGE_MAX = 48, 33
A_S3200 = (5, 17, 29, 41)
GAME_SEEDS = (0, 1, 2)
SIMS = 800
M64 = (1 << 64) - 1


class MemoModel:
    """model(board) of the reference's ModelWrapper, each position evaluated once (one position per forward, as
    evaluate_nn asks: a batched forward may round differently)."""

    def __init__(self, model):
        self.model = model
        self.memo = {}

    def __call__(self, board):
        k = (int(board.color[0]), int(board.color[1]))
        if k not in self.memo:
            v, p = self.model(board)
            assert v.dtype == np.float32 and p.dtype == np.float32
            self.memo[k] = (v.copy(), p.copy())
        v, p = self.memo[k]
        return v.copy(), p.copy()

    def bits(self, c0, c1):
        k = (int(c0), int(c1))
        if k not in self.memo:
            self(ref_board(c0, c1))
        v, p = self.memo[k]
        return np.float32(v.reshape(-1)[0]), p


def ref_board(c0, c1):
    """The reference's Board of an undecided position given as bitboards (bit = 7 col + row from the bottom)."""
    b = Board()
    b.color[0], b.color[1] = int(c0), int(c1)
    occ = int(c0) | int(c1)
    b.age = bin(occ).count("1")
    for c in range(7):
        b.height[c] = 7 * c + bin((occ >> (7 * c)) & 0x3F).count("1")
    return b


def perturbation(c0, c1, draw):
    """8 float32 amounts in (-EPS, EPS) for (position key, draw): splitmix64 on a mix of the three."""
    x = ((int(c0) * 0x9E3779B97F4A7C15) ^ (int(c1) * 0xC2B2AE3D27D4EB4F) ^ ((draw + 1) * 0x165667B19E3779F9)) & M64
    out = np.empty(8)
    for i in range(8):
        x = (x + 0x9E3779B97F4A7C15) & M64
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        out[i] = (z >> 11) * 2.0 ** -53
    return ((2.0 * out - 1.0) * EPS).astype(np.float32)


def oracle_visits(case, memo, draw):
    """Child visits of the case searched on the oracle; draw < 0: the reference's answers, else perturbed ones."""
    def fn(c0, c1):
        v, p = memo.bits(c0, c1)
        if draw >= 0:
            d = perturbation(c0, c1, draw)
            v = np.float32(min(max(np.float32(v + d[0]), np.float32(0.0)), np.float32(1.0)))
            p = np.maximum(p + d[1:], np.float32(0.0)).astype(np.float32)
        return float(v), p, True
    cfg = oc.make_config(**case["config"])
    b = oc.Board.from_bits(case["board"]["c0"], case["board"]["c1"])
    info = oc.search(cfg, b, oc.CallbackEvaluator(fn), case["noise"])
    return np.array(list(info.child_visits), dtype=np.float64)


def total_variation(a, b):
    return float(0.5 * np.abs(a / a.sum() - b / b.sum()).sum())


def judge(case, memo):
    base = oracle_visits(case, memo, -1)
    assert base.tolist() == [float(n) for n in case["N"]], "the oracle does not reproduce %s" % case["name"]
    runs = [oracle_visits(case, memo, k) for k in range(K)]
    case["decided"] = bool(all(np.array_equal(r, base) for r in runs))
    case["self_tv"] = max(total_variation(r, base) for r in runs)


def searched(name, family, board, cfg, memo, tables, keep_table):
    """One mcts.search of the unmodified reference, recorded like gen_golden.run_search_case."""
    evaluator = Evaluator(partial(evaluate_nn, model=memo))
    with GammaRecorder() as rec:
        tree = search(cfg, board, evaluator)
    d = dict(name=name, family=family, board=board_dict(board), config=cfg_dict(cfg),
             noise=rec.noise[0] if rec.noise else None, uniform=None)
    d.update(tree_summary(tree, board))
    d["move"] = d["best_move"]
    if keep_table:
        tables[name] = table_arrays(evaluator.position_table)
    return d


class RecordingMCTS(MCTS):
    """The reference's player, unchanged but for what it writes down: make_move runs the reference's make_move with a
    fresh Evaluator (the memo table changes no answer; a fresh one makes position_table this ply's positions)."""

    def __init__(self, name, config, memo, rec, game, tables):
        super().__init__(name, config, None)
        self.memo, self.rec, self.game, self.tables, self.cases = memo, rec, game, tables, []

    def make_move(self, board):
        before = copy(board)
        ply = len(self.cases)
        self.evaluator = Evaluator(partial(evaluate_nn, model=self.memo))
        n_noise, n_u = len(self.rec.noise), len(self.rec.uniforms)
        move, value, tree = super().make_move(board)
        assert len(self.rec.noise) == n_noise + 1 and len(self.rec.uniforms) - n_u == (1 if before.age < 6 else 0)
        name = "B%d_ply%02d" % (self.game, ply)
        d = dict(name=name, family="B", game=self.game, ply=ply, board=board_dict(before), config=cfg_dict(self.config),
                 noise=self.rec.noise[n_noise], uniform=self.rec.uniforms[n_u] if before.age < 6 else None)
        d.update(tree_summary(tree, before))
        d["move"] = int(move)
        d["value"] = None if value is None else float(value)
        if ply % 4 == 0:
            self.tables[name] = table_arrays(self.evaluator.position_table)
        self.cases.append(d)
        return move, value, tree


def write_npz(path, blobs):
    """np.savez_compressed with fixed member timestamps, so that a re-run writes the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(blobs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(blobs[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)  # deterministic accumulation order for the recorded net outputs
    oc.build()
    memo = MemoModel(ModelWrapper(ModelConfig(use_gpu=False), os.path.join(REF, "oinkoink", "data", "example_net.pth")))
    cases, tables, games = [], {}, []

    rng = np.random.RandomState(2024)
    seen, boards = set(), []
    for i in range(N_A):
        age = int(round(i * AGE_MAX / (N_A - 1.0)))
        while True:
            b = random_position(rng, age)
            if (int(b.color[0]), int(b.color[1])) not in seen:
                break
        seen.add((int(b.color[0]), int(b.color[1])))
        boards.append(b)
        cases.append(searched("A%02d_s%d" % (i, SIMS), "A", b, MCTSConfig(SIMS), memo, tables, i < 8))
        print(cases[-1]["name"], "age", age, cases[-1]["N"], flush=True)
    for i in A_S3200:
        cases.append(searched("A%02d_s3200" % i, "A", boards[i], MCTSConfig(3200), memo, tables, False))
        print(cases[-1]["name"], cases[-1]["N"], flush=True)

    for seed in GAME_SEEDS:
        cfg = MCTSConfig(SIMS, root_dirichlet_alpha=0.3, root_exploration_fraction=0.25, num_sampling_moves=6)
        np.random.seed(seed)
        with GammaRecorder() as rec:
            player = RecordingMCTS("ref", cfg, memo, rec, seed, tables)
            gd = training_game(player)
        assert len(player.cases) == len(gd.moves)
        for d, mv, pol, v in zip(player.cases, gd.moves, gd.priors, gd.values):
            assert d["move"] == int(mv) and d["value"] == (None if v is None else float(v))
            d["policy"] = [float(x) for x in pol]
            assert d["policy"] == d["values_policy"]
        cases.extend(player.cases)
        games.append(dict(seed=seed, moves=[int(m) for m in gd.moves], result=float(gd.result.value)))
        print("game", seed, games[-1]["moves"], flush=True)

    for c in cases:
        judge(c, memo)
        print(c["name"], "decided" if c["decided"] else "near-tie", "self_tv %.4f" % c["self_tv"], flush=True)

    share = {f: float(np.mean([c["decided"] for c in cases if c["family"] == f])) for f in ("A", "B")}
    print("decided shares:", share)
    assert share["A"] >= 0.5 and share["B"] >= 0.5, share
    with_table = [c for c in cases if c["name"] in tables]
    assert any(c["decided"] for c in with_table) and any(not c["decided"] for c in with_table)

    blobs = {}
    for name, (c0, c1, v, p) in tables.items():
        for k, a in (("c0", c0), ("c1", c1), ("v", v), ("p", p)):
            blobs["%s__%s" % (name, k)] = a
    write_npz(os.path.join(OUT, "net_parity_tables.npz"), blobs)
    with open(os.path.join(OUT, "net_parity.json"), "w") as f:
        json.dump(dict(eps=EPS, K=K, decided_share=share, table_cases=[c["name"] for c in with_table], games=games,
                       cases=cases), f)
    print("%d cases, %d tables, %d table positions written to %s" %
          (len(cases), len(tables), sum(len(t[0]) for t in tables.values()), OUT))


if __name__ == "__main__":
    main()
