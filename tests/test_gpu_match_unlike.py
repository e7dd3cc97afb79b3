"""Device matches between unlike players: c4_match_split_kernel (every net mode, the 64-filter "f32x3w" among them), the
per-net player description (c4_match_configure: simulations, pb_c_base, pb_c_init, kernel) and the host path that uses
them (connect4_amd.match with unlike=True / kernel=...).  The yardstick throughout is the host lock-step path --
gpu_helpers.host_lockstep_games, one MCTS.make_moves search per ply with each player's own net and config, the path
test_gpu_api.py pins to the oracle: device games equal it bit for bit (moves, boards, float64 values, policies, result).
Every configuration is deterministic (no root noise, no sampled moves); there is no tolerance anywhere."""
import pytest

from gpu_helpers import game_key as key_of
from gpu_helpers import host_lockstep_games as host_games
from net_models import stressed_state_dict

pytestmark = pytest.mark.gpu

SIMS = 32
# name -> (filters, residual blocks, seed)
NETS = {"A": (32, 1, 101), "B": (32, 1, 102), "R": (32, 2, 104), "W": (64, 1, 105), "X": (64, 1, 106)}
MODE = {"f16": 0, "f32x3": 1, "f16_64": 2, "f32x3w": 3}          # the kernels' MODE template argument
SPLIT_TW = {0: 4, 1: 4, 2: 2, 3: 4}                               # tree waves at 16 slots (launch_split)

_PLAYERS = {}
_HOST = {}


def player(name, precision, sims=SIMS, **config):
    """One MCTS player per (net, precision, search config) for the whole module."""
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.mcts import MCTS, MCTSConfig
    from connect4_amd.net import NetConfig
    key = (name, precision, sims, tuple(sorted(config.items())))
    if key not in _PLAYERS:
        filters, blocks, seed = NETS[name]
        sd = stressed_state_dict(NetConfig(filters=filters, n_residuals=blocks, n_fc_layers=1), seed=seed)
        _PLAYERS[key] = MCTS("%s/%s/%d" % (name, precision, sims), MCTSConfig(sims, **config), DeviceNetEvaluator(FusedNet(sd, precision=precision)))
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


def match_games(plies, switch=True):
    from connect4_amd.match import DeviceMatch
    return DeviceMatch(False, player("A", "f32x3"), player("B", "f32x3"), plies=plies, switch=switch).games


def host_reference(players, plies):
    """Host lock-step games of players[0] vs players[1] (Match.games order, switch=True): computed once per pairing and
    never modified."""
    key = (tuple(p.name for p in players), plies)
    if key not in _HOST:
        _HOST[key] = [key_of(g) for g in host_games(list(players), match_games(plies))]
    return _HOST[key]


def pair(mode):
    """The two players of the module for a net mode: (filters, precision) of MODE's names."""
    names, precision = {"f16": ("AB", "f16"), "f32x3": ("AB", "f32x3"), "f16_64": ("WX", "f16"), "f32x3w": ("WX", "f32x3w")}[mode]
    return player(names[0], precision), player(names[1], precision)


def kernel_log():
    seen = []
    return seen, (lambda eng: seen.append(eng.last_fused_kernel()))


def same_games(got, ref, what=""):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0], "%s game %d: moves differ: %r != %r" % (what, i, g[0], r[0])
        assert g == r, "%s game %d: values, policies, boards or result differ" % (what, i)


# ---------------------------------------------------------------- 1. f32x3w on the device
def test_wide_reference_precision_net_plays_on_the_device():
    from connect4_amd.match import DeviceMatch, score_results
    w, x = pair("f32x3w")
    seen, log = kernel_log()
    m = DeviceMatch(False, w, x, plies=1, switch=True, unlike=True, on_launch=log)
    assert len(m.games) == 14
    out = m.play()
    ref = host_reference((w, x), 1)
    same_games([key_of(r) for r in m.records], ref)
    assert out == score_results([k[4] for k in ref], 7, True)
    assert seen and all(s.startswith("c4_match_split_kernel<16,3,") for s in seen), seen
    assert set(seen) == {"c4_match_split_kernel<16,3,4> spread=0 grid=1"}


# ---------------------------------------------------------------- 2. the split kernel in every mode
@pytest.mark.parametrize("mode", ["f16", "f32x3", "f16_64", "f32x3w"])
def test_split_kernel_in_every_mode(mode):
    from connect4_amd.match import DeviceMatch
    a, b = pair(mode)
    seen, log = kernel_log()
    m = DeviceMatch(False, a, b, plies=1, switch=True, kernel="split", unlike=(mode == "f32x3w"), on_launch=log)
    m.play()
    got = [key_of(r) for r in m.records]
    same_games(got, host_reference((a, b), 1), "split")
    assert set(seen) == {"c4_match_split_kernel<16,%d,%d> spread=0 grid=1" % (MODE[mode], SPLIT_TW[MODE[mode]])}
    if mode != "f32x3w":   # the same match on the default kernel
        seen_w, log_w = kernel_log()
        w = DeviceMatch(False, a, b, plies=1, switch=True, on_launch=log_w)
        w.play()
        assert set(seen_w) == {"c4_match_wave_kernel<16,%d> spread=0 grid=1" % MODE[mode]}
        assert [key_of(r) for r in w.records] == got


# ---------------------------------------------------------------- 3. ragged and interleaved
def test_split_kernel_ragged_last_workgroup_98_games():
    """plies=2, switch: 98 games in seven workgroups of 16 slots, the last with 2, both nets' slots in every tree wave."""
    from connect4_amd.match import DeviceMatch, score_results
    a, b = pair("f32x3")
    seen, log = kernel_log()
    m = DeviceMatch(False, a, b, plies=2, switch=True, kernel="split", on_launch=log)
    assert m.n == 49 and len(m.games) == 98
    out = m.play()
    ref = host_reference((a, b), 2)
    got = [key_of(r) for r in m.records]
    for i in list(range(16)) + list(range(82, 98)):
        assert got[i] == ref[i], "game %d differs" % i
    same_games(got, ref)
    assert out == score_results([k[4] for k in ref], 49, True)
    assert set(seen) == {"c4_match_split_kernel<16,1,4> spread=0 grid=7"}


# ---------------------------------------------------------------- 4. launch boundaries and order
@pytest.mark.parametrize("mode, n_steps, order", [("f32x3", 1, (0, 1)), ("f32x3", 64, (1, 0)), ("f32x3w", 1, (0, 1))])
def test_split_kernel_launch_boundaries_and_net_order(mode, n_steps, order):
    """One quantum per launch: every launch ends at its deadline with leaves pending (posted, claimed or answered), and
    the slowest forward still makes progress."""
    from connect4_amd.match import DeviceMatch
    a, b = pair(mode)
    m = DeviceMatch(False, a, b, plies=1, switch=True, kernel="split", unlike=(mode == "f32x3w"), n_steps=n_steps, net_order=order)
    m.play()
    same_games([key_of(r) for r in m.records], host_reference((a, b), 1))


# ---------------------------------------------------------------- 5. caches
def test_split_kernel_caches_are_separate_and_transparent():
    from connect4_amd.match import DeviceMatch
    a, b = pair("f32x3")
    on = DeviceMatch(False, a, b, plies=1, switch=True, kernel="split")
    on.play()
    off = DeviceMatch(False, a, b, plies=1, switch=True, kernel="split", eval_cache_log2_entries=-1)
    off.play()
    assert on.stats["eval_cache_hits"] > 0
    assert off.stats["eval_cache_hits"] == 0 and off.stats["eval_cache_probes"] == 0
    assert [key_of(r) for r in on.records] == [key_of(r) for r in off.records]
    same_games([key_of(r) for r in on.records], host_reference((a, b), 1))


def test_speculating_split_kernel_with_and_without_caches():
    """The fp16 mode's network waves evaluate speculatively into the launch's own table: the games do not change."""
    from connect4_amd.match import DeviceMatch
    a, b = pair("f16")
    on = DeviceMatch(False, a, b, plies=1, switch=True, kernel="split")
    on.play()
    off = DeviceMatch(False, a, b, plies=1, switch=True, kernel="split", eval_cache_log2_entries=-1)
    off.play()
    assert off.stats["speculative_evals"] == 0
    assert [key_of(r) for r in on.records] == [key_of(r) for r in off.records]
    same_games([key_of(r) for r in on.records], host_reference((a, b), 1))


# ---------------------------------------------------------------- 6. unlike shapes and precisions
def test_tournament_of_unlike_nets():
    """32 filters f32x3, 32 filters fp16, two residual blocks f32x3 and 64 filters f32x3w: six pairings, 84 games in one
    engine, two match kernels."""
    from connect4_amd.match import DeviceMatch, tournament
    ps = [player("A", "f32x3"), player("B", "f16"), player("R", "f32x3"), player("W", "f32x3w")]
    seen, log = kernel_log()
    records = []
    import connect4_amd.match as M
    real = M.play_device_games

    def keep(*args, **kwargs):
        recs, st = real(*args, **kwargs)
        records.extend(recs)
        return recs, st
    M.play_device_games = keep
    try:
        table = tournament(ps, plies=1, switch=True, unlike=True, on_launch=log)
    finally:
        M.play_device_games = real
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert [row["name"] for row in table] == ["%s vs %s" % (ps[i].name, ps[j].name) for i, j in pairs]
    assert len(records) == 84
    openings = [g[0] for g in match_games(1, switch=False)]
    games = []
    for i, j in pairs:
        games += [(b, i, j) for b in openings] + [(b, j, i) for b in openings]
    same_games([key_of(r) for r in records], [key_of(g) for g in host_games(ps, games)])
    singles = [DeviceMatch(False, ps[i], ps[j], plies=1, switch=True, unlike=True).play() for i, j in pairs]
    assert [{k: row[k] for k in ("wins", "draws", "losses", "return")} for row in table] == singles
    names = {s.split(" ")[0] for s in seen}
    assert names == {"c4_match_wave_kernel<16,1>", "c4_match_wave_kernel<16,0>", "c4_match_split_kernel<16,3,4>"}
    assert all(s.endswith(" spread=0 grid=6") for s in seen)


# ---------------------------------------------------------------- 7. unlike searches
@pytest.mark.parametrize("big_first", [False, True], ids=["largest is index 1", "largest is index 0"])
def test_unlike_searches(big_first):
    """One net at 32 simulations against the same net at 48 with other PUCT constants.  Every move takes exactly its
    mover's simulations (tree_step counts a simulation when it is issued, the root's evaluation is none, and a move is
    chosen when the count reaches the launch's S), so the engine's total says which S each side searched with.  (A game
    record holds the values policy -- normalised child values, tree.py:104-109 -- not visit counts: there is nothing in
    it that is a multiple of 1/S.)"""
    from connect4_amd.match import DeviceMatch
    small, big = player("A", "f32x3", 32), player("A", "f32x3", 48, pb_c_init=2.0, pb_c_base=100)
    ps = (big, small) if big_first else (small, big)
    m = DeviceMatch(False, ps[0], ps[1], plies=1, switch=True, unlike=True)
    m.play()
    same_games([key_of(r) for r in m.records], host_reference(ps, 1))
    own = 0
    moves = {32: 0, 48: 0}
    for r, (board, o, x) in zip(m.records, m.games):
        for b in r.boards:
            s = ps[(o, x)[b.age % 2]].config.simulations
            moves[s] += 1
            own += s
    assert moves[32] > 0 and moves[48] > 0 and m.stats["moves"] == moves[32] + moves[48]
    print("simulations: engine %d, 32 x %d + 48 x %d = %d" % (m.stats["simulations"], moves[32], moves[48], own))
    assert m.stats["simulations"] == own
    # the host path of the same two players differs from a match of two 32-simulation players: the configs do matter
    assert host_reference(ps, 1) != host_reference((small, player("B", "f32x3", 32)), 1)


# ---------------------------------------------------------------- 8. c4_match_configure's refusals
def _engine(n_slots=14, sims=SIMS, **kwargs):
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    return Engine(n_slots, sims, eval_mode=L.EVAL_EXTERNAL_F32, games_target=n_slots, record_capacity_games=n_slots, max_inner_iters=32,
                  time_budget_cycles=80000, **kwargs)


def _buffers(n):
    import torch
    return torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros(n, 7, dtype=torch.float32, device="cuda")


def test_configure_needs_an_idle_match_engine():
    from connect4_amd import _lib as L
    games = match_games(1)
    with _engine() as eng:                                  # not a match engine
        with pytest.raises(L.EngineError) as e:
            eng.match_configure(0, kernel="split")
        assert e.value.code == L.ESTATE
    with _engine(n_match_nets=2) as eng:
        eng.match_configure(0, kernel="split")              # idle after create
        eng.reset([g[0].color[0] for g in games], [g[0].color[1] for g in games])
        eng.match_configure(1, 16, 100, 2.0, "wave")
        eng.match_assign([g[1] for g in games], [g[2] for g in games])
        with pytest.raises(L.EngineError) as e:             # a match is in progress
            eng.match_configure(0, kernel="split")
        assert e.value.code == L.ESTATE
        with pytest.raises(L.EngineError) as e:             # ... and index 1 is on the wave kernel, which cannot hold the wide net
            eng.match_steps(player("W", "f32x3w").evaluator.net, 1, *_buffers(14), 1)
        assert e.value.code == L.ESTATE and "cannot hold the 64-filter reference-precision net" in str(e.value)
        assert eng.last_fused_kernel() == ""
        eng.reset([g[0].color[0] for g in games], [g[0].color[1] for g in games])
        eng.match_configure(1, kernel="split")              # idle again
        for index in (-1, 2):                               # the engine has nets 0 and 1
            with pytest.raises(L.EngineError) as e:
                eng.match_configure(index, kernel="split")
            assert e.value.code == L.EINVAL


def test_unconfigured_engine_refuses_the_wide_net_as_ever():
    from connect4_amd import _lib as L
    games = match_games(1)
    with _engine(n_match_nets=2) as eng:
        eng.reset([g[0].color[0] for g in games], [g[0].color[1] for g in games])
        eng.match_assign([g[1] for g in games], [g[2] for g in games])
        with pytest.raises(L.EngineError) as e:
            eng.match_steps(player("W", "f32x3w").evaluator.net, 0, *_buffers(14), 1)
        assert e.value.code == L.ESTATE
        assert "c4_match_steps cannot hold the 64-filter reference-precision net (eight waves' planes exceed a CU's LDS)" in str(e.value)


def test_refused_values_leave_the_engine_as_it_was(monkeypatch):
    """C4_EINVAL for simulations above the engine's, a negative pb_c_base and a pb_c_init that is not finite -- tried on
    the engine of test 1's match between its configuration and its assignment: the match is the host's all the same."""
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    from connect4_amd.match import DeviceMatch
    w, x = pair("f32x3w")
    refused = []
    assign = Engine.match_assign

    def refuse_then_assign(eng, net_o, net_x):
        for index, kwargs in ((0, dict(simulations=SIMS + 1)), (1, dict(pb_c_base=-1)), (0, dict(pb_c_init=float("nan"))),
                              (1, dict(pb_c_init=float("inf"))), (0, dict(simulations=-3))):
            with pytest.raises(L.EngineError) as e:
                eng.match_configure(index, kernel="wave", **kwargs)
            assert e.value.code == L.EINVAL, kwargs
            refused.append(str(e.value))
        return assign(eng, net_o, net_x)
    monkeypatch.setattr(Engine, "match_assign", refuse_then_assign)
    seen, log = kernel_log()
    m = DeviceMatch(False, w, x, plies=1, switch=True, unlike=True, on_launch=log)
    m.play()
    assert len(refused) == 5 and "simulations" in refused[0] and "pb_c_base" in refused[1] and "pb_c_init" in refused[2]
    same_games([key_of(r) for r in m.records], host_reference((w, x), 1))
    assert set(seen) == {"c4_match_split_kernel<16,3,4> spread=0 grid=1"}     # (kernel="wave" of the refused calls did not stick)


# ---------------------------------------------------------------- 9. generation
def test_generation_match_of_a_wide_reference_precision_run(tmp_path):
    """Generation 11 of a 64-filter run in f32x3w meets the net of generation 1: on the device with match_unlike, on the
    host without."""
    import os

    import torch

    from connect4_amd.config import MCTSConfig
    from connect4_amd.generation import run_generation
    from connect4_amd.net import NetConfig
    from connect4_amd.training import ModelConfig, Trainer
    d = str(tmp_path)
    cfg = MCTSConfig.self_play(16)
    torch.manual_seed(0)
    tr = Trainer(ModelConfig(net_config=NetConfig(filters=64, n_residuals=1, n_fc_layers=1), batch_size=256, n_training_epochs=1, use_gpu=True))
    tr.save(os.path.join(d, "1"))
    t = {}
    run_generation(tr, cfg, 16, d, gen=11, n_slots=16, timings=t, precision="f32x3w", match_every=1, match_plies=1, match_unlike=True)
    assert t["match"]["path"] == "device" and t["match"]["opponent"] == "Older net"
    assert t["match"]["wins"] + t["match"]["draws"] + t["match"]["losses"] == 14
    t2 = {}
    run_generation(tr, cfg, 16, d, gen=11, n_slots=16, timings=t2, precision="f32x3w", match_every=1, match_plies=1)
    assert t2["match"]["path"] == "host" and t2["match"]["opponent"] == "Older net"
