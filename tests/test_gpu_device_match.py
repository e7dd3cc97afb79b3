"""Net-vs-net matches inside the fused kernel (connect4_amd.match.DeviceMatch / tournament, c4_match_steps): the games
must be those of the host lock-step path (one MCTS.make_moves search per ply, the path test_gpu_api.py pins to the
oracle), move for move and bit for bit, whatever the launch length, the order the nets are served in, the workgroup
shape or the evaluation caches do.  Every configuration here is deterministic (no root noise, no sampled moves)."""
import pytest

from gpu_helpers import game_key as key_of
from gpu_helpers import host_lockstep_games as host_games
from net_models import stressed_state_dict

pytestmark = pytest.mark.gpu

SIMS = 32
NET_SEEDS = {"A": 101, "B": 102, "C": 103}


def _state(name):
    from connect4_amd.net import NetConfig
    return stressed_state_dict(NetConfig(filters=32, n_residuals=1, n_fc_layers=1), seed=NET_SEEDS[name])


_PLAYERS = {}


def player(name, precision="f32x3", sims=SIMS):
    """One MCTS player per (net, precision, simulations) for the whole module."""
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.mcts import MCTS, MCTSConfig
    key = (name, precision, sims)
    if key not in _PLAYERS:
        _PLAYERS[key] = MCTS(name, MCTSConfig(sims), DeviceNetEvaluator(FusedNet(_state(name), precision=precision)))
    return _PLAYERS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_players():
    yield
    for p in _PLAYERS.values():
        if p._searcher is not None:
            p._searcher.close()
        p.evaluator.net.close()
    _PLAYERS.clear()
    _HOST.clear()


_HOST = {}


def host_reference(precision, plies):
    """Host lock-step games of A vs B with switch=True, computed once per (precision, plies) and never modified."""
    from connect4_amd.match import DeviceMatch
    if (precision, plies) not in _HOST:
        a, b = player("A", precision), player("B", precision)
        games = DeviceMatch(False, a, b, plies=plies, switch=True).games
        _HOST[(precision, plies)] = [key_of(g) for g in host_games([a, b], games)]
    return _HOST[(precision, plies)]


def counts(keys, n):
    from connect4_amd.match import score_results
    return score_results([k[4] for k in keys], n, True)


@pytest.mark.parametrize("precision", ["f32x3", "f16"])
def test_equals_host_lockstep_game_for_game(precision):
    from connect4_amd.match import DeviceMatch
    m = DeviceMatch(False, player("A", precision), player("B", precision), plies=1, switch=True)
    assert m.n == 7 and len(m.games) == 14
    out = m.play()
    ref = host_reference(precision, 1)
    got = [key_of(r) for r in m.records]
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0], "game %d: moves differ" % i
        assert g == r, "game %d: values, policies, boards or result differ" % i
    assert out == counts(ref, 7)
    assert out["wins"] + out["draws"] + out["losses"] == 14


def test_one_net_on_both_sides_equals_selfplay_kernel():
    """DeviceMatch(A, A) against an independent partner that never runs the match kernel: a noise-free continuous engine
    reset to the same 7 openings and driven by c4_selfplay_steps."""
    from connect4_amd.match import DeviceMatch
    from connect4_amd.mcts import MCTS
    from connect4_amd.selfplay import SelfPlay
    from connect4_amd.training_game import game_data_from_record
    a = player("A")
    m = DeviceMatch(False, a, MCTS("A again", a.config, a.evaluator), plies=1)
    m.play()
    sp = SelfPlay(a.evaluator.net, 7, a.config, games_target=7, record_capacity_games=7, use_graph=False, fused_loop=True,
                  steps_per_launch=16)
    try:
        sp.engine.reset([g[0].color[0] for g in m.games], [g[0].color[1] for g in m.games])
        for _ in range(4000):
            sp.run_steps(64)
            if sp.stats()["active_slots"] == 0:
                break
        recs = sorted(sp.engine.drain_games(), key=lambda r: r.game_id)
    finally:
        sp.close()
    assert len(recs) == 7
    assert [key_of(r) for r in m.records] == [key_of(game_data_from_record(r)) for r in recs]


def test_partial_workgroup_98_games():
    """plies=2, switch: 98 games in 16-slot workgroups -- the last one holds 2 -- with both nets' slots interleaved in
    every wave.  All 98 games move for move, and the counts."""
    from connect4_amd.match import DeviceMatch
    m = DeviceMatch(False, player("A"), player("B"), plies=2, switch=True)
    assert m.n == 49 and len(m.games) == 98
    out = m.play()
    ref = host_reference("f32x3", 2)
    got = [key_of(r) for r in m.records]
    assert [g[4] for g in got] == [r[4] for r in ref]
    for i in list(range(16)) + list(range(82, 98)):
        assert got[i] == ref[i], "game %d differs" % i
    assert got == ref
    assert out == counts(ref, 49)


@pytest.mark.parametrize("n_steps, order", [(1, (0, 1)), (64, (0, 1)), (64, (1, 0)), (1, (1, 0))])
def test_launch_boundaries_and_net_order_do_not_matter(n_steps, order):
    from connect4_amd.match import DeviceMatch
    m = DeviceMatch(False, player("A"), player("B"), plies=1, switch=True, n_steps=n_steps, net_order=order)
    m.play()
    assert [key_of(r) for r in m.records] == host_reference("f32x3", 1)


def test_caches_are_separate_and_transparent():
    """The same records with one evaluation cache per net and with none; the caches do answer.  (With ONE table for both
    nets a search is answered with the opponent's evaluations and this comparison fails.)"""
    from connect4_amd.match import DeviceMatch
    on = DeviceMatch(False, player("A"), player("B"), plies=1, switch=True)
    on.play()
    off = DeviceMatch(False, player("A"), player("B"), plies=1, switch=True, eval_cache_log2_entries=-1)
    off.play()
    assert on.stats["eval_cache_hits"] > 0
    assert off.stats["eval_cache_hits"] == 0 and off.stats["eval_cache_probes"] == 0
    assert [key_of(r) for r in on.records] == [key_of(r) for r in off.records]
    assert [key_of(r) for r in on.records] == host_reference("f32x3", 1)


def test_tournament_equals_single_matches():
    from connect4_amd.match import DeviceMatch, tournament
    ps = [player("A"), player("B"), player("C")]
    table = tournament(ps, plies=1, switch=True)
    assert [row["name"] for row in table] == ["A vs B", "A vs C", "B vs C"]
    singles = [DeviceMatch(False, ps[i], ps[j], plies=1, switch=True).play() for i, j in ((0, 1), (0, 2), (1, 2))]
    assert [{k: row[k] for k in ("wins", "draws", "losses", "return")} for row in table] == singles


def test_run_generations_plays_the_generation_match(tmp_path):
    """TrainingLoop._match inside run_generation(s): one row of match_results.pkl per generation; the centre opponent of
    gen <= 10 goes through the host Match, the net of ten generations ago through the device match; a resumed run
    extends the file."""
    import os
    import pickle

    import torch

    from connect4_amd.config import MCTSConfig
    from connect4_amd.generation import run_generation, run_generations
    from connect4_amd.training import ModelConfig, Trainer
    d = str(tmp_path)
    cfg = MCTSConfig.self_play(16)
    torch.manual_seed(0)
    tr = Trainer(ModelConfig(batch_size=256, n_training_epochs=1, use_gpu=True))
    timings = []
    run_generations(tr, cfg, 24, d, 2, first_gen=1, n_slots=24, timings=timings, match_every=1)

    def history():
        with open(os.path.join(d, "match_results.pkl"), "rb") as f:
            return pickle.load(f)
    hist = history()
    assert [e["generation"] for e in hist] == [1, 2]
    for e, t in zip(hist, timings):
        assert set(e) == {"generation", "wins", "draws", "losses", "return"}
        assert e["wins"] + e["draws"] + e["losses"] == 14
        assert e["return"] == (e["wins"] + 0.5 * e["draws"]) / 14
        assert t["match"]["path"] == "host" and t["match"]["opponent"] == "Evaluate_centre_with_prior"
        assert {k: t["match"][k] for k in ("wins", "draws", "losses", "return")} == {k: e[k] for k in ("wins", "draws", "losses", "return")}
    # resumed (the directory says generation 3 is next): the file is extended
    tr2 = Trainer(ModelConfig(batch_size=256, n_training_epochs=1, use_gpu=True))
    t2 = []
    run_generations(tr2, cfg, 24, d, 1, n_slots=24, timings=t2, match_every=1)
    assert [e["generation"] for e in history()] == [1, 2, 3] and history()[:2] == hist
    # match_every=2: generation 3 would have been skipped
    t3 = {}
    run_generation(tr2, cfg, 24, d, gen=5, n_slots=24, timings=t3, match_every=2)
    assert "match" not in t3 and [e["generation"] for e in history()] == [1, 2, 3]
    # generation 11 meets the net of generation 1 (planted by the run above): two nets, the device path
    t11 = {}
    run_generation(tr2, cfg, 24, d, gen=11, n_slots=24, timings=t11, match_every=1, match_plies=1)
    assert t11["match"]["path"] == "device" and t11["match"]["opponent"] == "Older net"
    h = history()
    assert [e["generation"] for e in h] == [1, 2, 3, 11] and h[3]["wins"] + h[3]["draws"] + h[3]["losses"] == 14
