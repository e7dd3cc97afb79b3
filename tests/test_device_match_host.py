"""Host side of the device match (connect4_amd.match.DeviceMatch / play_match / tournament, generation.append_history):
the bookkeeping, the eligibility rules, the fallback and the C prototypes.  No GPU: nets are FusedNet objects that were
never handed to the device, the games are synthetic records."""
import os
import pickle
import re

import numpy as np
import pytest

from connect4_amd import _lib as L
from connect4_amd import match as M
from connect4_amd.board import Board
from connect4_amd.evaluators import DeviceNetEvaluator, Evaluator, evaluate_centre_with_prior
from connect4_amd.fused_net import FusedNet
from connect4_amd.mcts import MCTS, MCTSConfig
from connect4_amd.net import NetConfig
from connect4_amd.player import BasePlayer
from connect4_amd.training_game import GameData
from connect4_amd.utils import Result


def fake_net(filters=32, n_residuals=1, precision="f32x3", device=0):
    """A FusedNet as the eligibility rules see it (shape, precision, device), without the device object behind it."""
    net = object.__new__(FusedNet)
    net.config = NetConfig(filters=filters, n_residuals=n_residuals)
    net.precision = precision
    net.device = device
    net._h = None
    return net


def net_player(name="p", config=None, **net_kwargs):
    return MCTS(name, config or MCTSConfig(32), DeviceNetEvaluator(fake_net(**net_kwargs)))


# ---------------------------------------------------------------- bookkeeping (oinkoink/match.py:51-60)
def reference_bookkeeping(results, n, switch):
    results = np.array(results, dtype="f")
    if switch:
        results[n:] *= -1.0
        results[n:] += 1.0
    wins = np.sum(results == 1)
    draws = np.sum(results == 0.5)
    losses = np.sum(results == 0)
    return {"wins": wins, "draws": draws, "losses": losses, "return": (1.0 * wins + 0.5 * draws) / (wins + draws + losses)}


@pytest.mark.parametrize("switch", [False, True])
def test_score_results_is_the_references_bookkeeping(switch):
    rng = np.random.RandomState(3)
    for n in (1, 7, 49):
        res = rng.choice([0.0, 0.5, 1.0], size=2 * n if switch else n).tolist()
        got, want = M.score_results(res, n, switch), reference_bookkeeping(res, n, switch)
        assert got == {k: (float(v) if k == "return" else int(v)) for k, v in want.items()}
        assert all(type(got[k]) is int for k in ("wins", "draws", "losses"))
    # a switched game that x wins is a win of player_1, who moved x there
    assert M.score_results([1.0, 0.0], 1, True) == {"wins": 2, "draws": 0, "losses": 0, "return": 1.0}
    assert M.score_results([0.0, 1.0], 1, True) == {"wins": 0, "draws": 0, "losses": 2, "return": 0.0}
    assert M.score_results([1.0, 0.0], 2, False) == {"wins": 1, "draws": 0, "losses": 1, "return": 0.5}


def test_device_match_scores_synthetic_records(monkeypatch, capsys):
    """DeviceMatch.play on records handed in by a stand-in for the engine: Match.games order, the switch flip, the
    reference's dict and line of output."""
    p1, p2 = net_player("one"), net_player("two")
    seen = {}

    def fake_play(players, games, n_steps, cache_bits, order):
        seen.update(players=players, games=games, n_steps=n_steps, cache_bits=cache_bits, order=order)
        out = []
        for i, (board, o, x) in enumerate(games):
            gd = GameData()
            gd.game_id = i
            gd.result = Result.o_win if i % 3 == 0 else (Result.draw if i % 3 == 1 else Result.x_win)
            out.append(gd)
        return out, {"eval_cache_hits": 5}
    monkeypatch.setattr(M, "play_device_games", fake_play)
    m = M.DeviceMatch(True, p1, p2, plies=1, switch=True, n_steps=9, eval_cache_log2_entries=-1, net_order=(1, 0))
    ref = M.Match(False, p1, p2, plies=1, switch=True)
    assert m.n == ref.n == 7 and len(m.games) == len(ref.games) == 14
    for (b, o, x), (rb, ro, rx) in zip(m.games, ref.games):
        assert b.to_int_tuple() == rb.to_int_tuple() and (p1, p2)[o] is ro and (p1, p2)[x] is rx
    out = m.play()
    assert seen["players"] == [p1, p2] and (seen["n_steps"], seen["cache_bits"], seen["order"]) == (9, -1, (1, 0))
    results = [1.0 if i % 3 == 0 else (0.5 if i % 3 == 1 else 0.0) for i in range(14)]
    want = reference_bookkeeping(results, 7, True)
    assert out == {"wins": int(want["wins"]), "draws": int(want["draws"]), "losses": int(want["losses"]), "return": float(want["return"])}
    assert len(m.records) == 14 and m.stats == {"eval_cache_hits": 5}
    assert capsys.readouterr().out == "The results for one vs two are: {} wins, {} draws, {} losses, {:.3f} return\n".format(
        out["wins"], out["draws"], out["losses"], out["return"])


# ---------------------------------------------------------------- eligibility
class FirstColumn(BasePlayer):
    def make_move(self, board):
        move = min(board.valid_moves)
        board.make_move(move)
        return move, None, None


CASES = [
    ("not an MCTS", lambda: (net_player("a"), FirstColumn("b")), "is not an MCTS player"),
    ("centre evaluator", lambda: (net_player("a"), MCTS("c", MCTSConfig(32), Evaluator(evaluate_centre_with_prior))), "centre evaluator"),
    ("bare centre evaluator", lambda: (MCTS("c", MCTSConfig(32), evaluate_centre_with_prior), net_player("a")), "centre evaluator"),
    ("host callable", lambda: (net_player("a"), MCTS("h", MCTSConfig(32), Evaluator(lambda b: (0.5, np.ones(7) / 7)))), "not a DeviceNetEvaluator"),
    ("not a FusedNet", lambda: (net_player("a"), MCTS("t", MCTSConfig(32), DeviceNetEvaluator(lambda planes: None))), "not a FusedNet"),
    ("filters", lambda: (net_player("a"), net_player("b", filters=64, precision="f16")), "differ in shape"),
    ("residual blocks", lambda: (net_player("a"), net_player("b", n_residuals=2)), "differ in shape"),
    ("precision", lambda: (net_player("a"), net_player("b", precision="f16")), "differ in precision"),
    ("f32x3w", lambda: (net_player("a", filters=64, precision="f32x3w"), net_player("b", filters=64, precision="f32x3w")), "f32x3w"),
    ("devices", lambda: (net_player("a"), net_player("b", device=1)), "different devices"),
    ("simulations", lambda: (net_player("a"), net_player("b", MCTSConfig(48))), "simulations, pb_c_base or pb_c_init"),
    ("pb_c_base", lambda: (net_player("a"), net_player("b", MCTSConfig(32, pb_c_base=100))), "simulations, pb_c_base or pb_c_init"),
    ("pb_c_init", lambda: (net_player("a"), net_player("b", MCTSConfig(32, pb_c_init=2.0))), "simulations, pb_c_base or pb_c_init"),
    ("root noise", lambda: (net_player("a", MCTSConfig(32, root_dirichlet_alpha=0.3, root_exploration_fraction=0.25)),) * 2, "root noise"),
    ("sampling", lambda: (net_player("a", MCTSConfig(32, num_sampling_moves=6)),) * 2, "samples its first 6 moves"),
]


@pytest.mark.parametrize("name, make, reason", CASES, ids=[c[0] for c in CASES])
def test_ineligible_players_raise_with_the_reason(name, make, reason):
    p1, p2 = make()
    assert reason in M.device_match_reason([p1, p2])
    with pytest.raises(ValueError, match=re.escape(reason)):
        M.DeviceMatch(False, p1, p2, plies=1, switch=True)
    with pytest.raises(ValueError, match=re.escape(reason)):
        M.tournament([p1, p2], plies=1, switch=True)
    with pytest.raises(ValueError, match=re.escape(reason)):
        M.play_device_games([p1, p2], [(Board(), 0, 1)])


def test_eligible_players_and_player_count():
    a, b = net_player("a"), net_player("b")
    assert M.device_match_reason([a, b]) is None
    assert M.device_match_reason([a, b, net_player("c")]) is None
    assert M.device_match_reason([net_player("a", filters=64, precision="f16"), net_player("b", filters=64, precision="f16")]) is None
    assert M.device_match_reason([MCTS("w", MCTSConfig(32), Evaluator(DeviceNetEvaluator(fake_net()))), b]) is None
    # noise needs both parameters, as in the engine (mcts.py:174)
    assert M.device_match_reason([net_player("a", MCTSConfig(32, root_dirichlet_alpha=0.3)), b]) is None
    assert "2 to %d players" % L.MATCH_MAX_NETS in M.device_match_reason([a])
    assert "2 to %d players" % L.MATCH_MAX_NETS in M.device_match_reason([a] * (L.MATCH_MAX_NETS + 1))
    with pytest.raises(ValueError, match="permutation"):
        M.play_device_games([a, b], [(Board(), 0, 1)], net_order=(0, 0))


# ---------------------------------------------------------------- play_match
def test_play_match_falls_back_to_the_host_match(monkeypatch):
    p1, p2 = FirstColumn("left"), FirstColumn("also left")
    out, path = M.play_match(False, p1, p2, plies=1, switch=True)
    assert path == "host" and out == M.Match(False, p1, p2, plies=1, switch=True).play()
    assert out["wins"] + out["draws"] + out["losses"] == 14
    # eligible players take the device path -- unless the caller prefers the host
    a, b = net_player("a"), net_player("b")
    calls = []

    class Stub:
        def __init__(self, *args, **kwargs):
            calls.append((args, kwargs))

        def play(self, agents=1):
            return {"wins": 1, "draws": 0, "losses": 0, "return": 1.0}
    monkeypatch.setattr(M, "DeviceMatch", Stub)
    assert M.play_match(False, a, b, plies=2, switch=True, n_steps=7) == ({"wins": 1, "draws": 0, "losses": 0, "return": 1.0}, "device")
    assert calls == [((False, a, b, 2, True), {"n_steps": 7})]
    monkeypatch.setattr(M, "Match", Stub)
    assert M.play_match(False, a, b, plies=2, switch=True, prefer_device=False)[1] == "host"
    assert M.play_match(False, a, FirstColumn("x"), plies=2, switch=True)[1] == "host"


# ---------------------------------------------------------------- match_results.pkl
def test_append_history_replaces_and_truncates(tmp_path):
    from connect4_amd.generation import append_history
    path = os.path.join(str(tmp_path), "match_results.pkl")

    def read():
        with open(path, "rb") as f:
            return pickle.load(f)
    row = lambda w: {"wins": w, "draws": 1, "losses": 2, "return": 0.5}  # noqa: E731
    append_history(path, 1, row(1))
    append_history(path, 2, row(2))
    append_history(path, 4, row(4))
    assert [(e["generation"], e["wins"]) for e in read()] == [(1, 1), (2, 2), (4, 4)]
    assert set(read()[0]) == {"generation", "wins", "draws", "losses", "return"}
    append_history(path, 4, row(40))            # this generation again: replaced
    assert [(e["generation"], e["wins"]) for e in read()] == [(1, 1), (2, 2), (4, 40)]
    append_history(path, 2, row(20))            # redone from a lower generation: later entries are dropped
    assert [(e["generation"], e["wins"]) for e in read()] == [(1, 1), (2, 20)]
    assert not os.path.exists(path + ".tmp")


# ---------------------------------------------------------------- the C prototypes
C_TYPES = {"c4_engine *": "c_void_p", "c4_net *": "c_void_p", "void *": "c_void_p", "float *": "c_void_p",
           "const int32_t *": "LP_c_int", "int32_t": "c_int"}


def test_ctypes_prototypes_match_the_header():
    with open(L.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("c4_match_assign", "c4_match_steps"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in c4_engine.h" % name
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
        want = []
        for p in params:
            ctype = re.sub(r"\b\w+$", "", p).strip()          # drop the parameter's name
            want.append(C_TYPES[ctype])
        res, args = L.SIGNATURES[name]
        assert res.__name__ == "c_int" and [a.__name__ for a in args] == want, (name, params)
    assert re.search(r"#define\s+C4_MATCH_MAX_NETS\s+(\d+)", text).group(1) == str(L.MATCH_MAX_NETS)
    assert L.Config.reserved.size == 16 and "reserved[0] = n_match_nets" in open(L.HEADER_PATH).read()
