"""The fused self-play kernels (split, wave, block: each has a descent of its own) where ties decide the games, and off the
default configuration.  Short runs shaped like test_gpu_net_float64.py::test_selfplay_caches_the_stressed_nets_answers -- 64
slots, at most 64 simulations, 48 games, a 2^22-entry evaluation cache -- with RNG tapes; every game is replayed on the oracle
(oracle.replay.replay_games_bulk), whose evaluator answers with what the device's cache holds.

Degenerate nets: net_models.grid_net with every convolution weight zeroed, so no activation depends on the position and the
net answers every position alike; the policy head's Linear weight is zeroed as well, so its bias alone is the logits: equal
biases give the uniform prior (every PUCT score ties in the float32 form, at every node of every search), distinct biases a
fixed non-uniform one (ties wherever visit counts agree, since the value is one constant).

Modes: the block kernel serves the 32-filter fp16 net only (c4_selfplay_steps: C4_ESTATE otherwise), so the
reference-precision runs compare split and wave, the fp16 runs all three."""
import numpy as np
import pytest

import net_models as M

pytestmark = pytest.mark.gpu

GAMES, SLOTS = 48, 64
KERNEL = {"split": "c4_selfplay_split_kernel<", "wave": "c4_selfplay_wave_kernel<", "block": "c4_selfplay_kernel<"}
LOST_SHARE = 0.10      # share of replayed positions the table has lost and the net re-answers: the existing replays' bound


def degenerate_net(filters, n_res, biases):
    import torch
    sd = {k: v.clone() for k, v in M.grid_net(filters, n_res).items()}
    for k, v in sd.items():
        if v.dim() == 4:                        # every convolution: stem, tower, both heads' 1x1
            sd[k] = torch.zeros_like(v)
    sd["policy_head.fc1.weight"] = torch.zeros_like(sd["policy_head.fc1.weight"])
    sd["policy_head.fc1.bias"] = torch.tensor(biases, dtype=torch.float32)
    return sd


BIASES = {"uniform": [0.25] * 7, "fixed": [0.0, 0.5, -0.5, 1.0, 0.25, -1.0, 0.75]}


def assert_degenerate(net, uniform):
    """The answers are finite and bit-identical across positions (and across columns for the uniform prior)."""
    c0, c1 = M.position_set(84, seed=9)
    for wave in (False, True):
        v, p = net.evaluate_bits(c0, c1, wave=wave)
        assert np.isfinite(v).all() and np.isfinite(p).all() and 0.0 <= v[0] <= 1.0
        assert len(set(v.view(np.uint32).tolist())) == 1
        assert len({row.tobytes() for row in p}) == 1
        assert (len(set(p[0].view(np.uint32).tolist())) == 1) == uniform
    return float(v[0]), p[0].copy()


def play(net, cfg, mode, monkeypatch, noise, u, seed=4):
    from connect4_amd import _lib as L
    from connect4_amd.selfplay import SelfPlay
    monkeypatch.setenv("C4_FUSED_MODE", mode)
    sp = SelfPlay(net, SLOTS, cfg, seed=seed, games_target=GAMES, record_capacity_games=64, use_graph=False, fused_loop=True,
                  steps_per_launch=16, eval_cache_log2_entries=22, rng_mode=L.RNG_TAPE)
    sp.engine.set_tapes(noise, u)
    sp.engine.reset()
    for _ in range(1000):
        sp.run_steps(64)
        if sp.stats()["active_slots"] == 0:
            break
    st = sp.stats()
    recs = sorted(sp.engine.drain_games(), key=lambda r: r.game_id)
    assert len(recs) == GAMES and st["bad_evals"] == 0 and st["dropped_games"] == 0 and st["active_slots"] == 0
    assert sp.engine.last_fused_kernel().startswith(KERNEL[mode]), sp.engine.last_fused_kernel()    # the mode asked for is what ran
    return sp, recs


def key(recs):
    return [(r.game_id, r.length, r.result, list(r.move[:r.length]), list(r.color0[:r.length]), list(r.color1[:r.length]),
             np.array(r.value[:r.length]).tobytes(), np.array([list(r.policy[i]) for i in range(r.length)]).tobytes()) for r in recs]


def replay(sp, net, cfg, recs, noise, u, what):
    from oracle.replay import oracle_config, replay_games_bulk
    out = replay_games_bulk(oracle_config(cfg), sp.engine, net, recs, noise, u)
    share = out["lost_by_the_table"] / max(out["positions_asked"], 1)
    print("%s: %d games replayed, %d positions asked, %d lost by the table (%.2f%%)" % (
        what, out["games"], out["positions_asked"], out["lost_by_the_table"], 100.0 * share))
    assert out["games"] == GAMES and share <= LOST_SHARE


def run_modes(net, cfg, modes, monkeypatch, what, tape_seed=8):
    from oracle.replay import random_tapes
    noise, u = random_tapes(GAMES, cfg.root_dirichlet_alpha, seed=tape_seed)
    first = None
    for mode in modes:
        sp, recs = play(net, cfg, mode, monkeypatch, noise, u)
        try:
            if first is None:
                first = key(recs)
                replay(sp, net, cfg, recs, noise, u, "%s, %s kernel" % (what, mode))
            else:
                assert key(recs) == first, "%s: the %s kernel plays other games than the %s kernel" % (what, mode, modes[0])
        finally:
            sp.close()
    return first


@pytest.mark.parametrize("precision", ["f32x3", "f16"])
@pytest.mark.parametrize("prior", ["uniform", "fixed"])
def test_degenerate_nets_play_the_oracles_games_in_every_kernel(oracle, monkeypatch, prior, precision):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import FusedNet
    net = FusedNet(degenerate_net(32, 1, BIASES[prior]), precision=precision)
    try:
        assert_degenerate(net, prior == "uniform")
        modes = ("split", "wave", "block") if precision == "f16" else ("split", "wave")
        games = run_modes(net, MCTSConfig.self_play(48), modes, monkeypatch, "%s prior, %s" % (prior, precision))
        assert len({tuple(g[3]) for g in games}) > GAMES // 2        # the tapes, not the net, tell the games apart
    finally:
        net.close()


def test_degenerate_64_filter_net_in_the_split_kernel(oracle, monkeypatch):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import FusedNet
    net = FusedNet(degenerate_net(64, 1, BIASES["uniform"]), precision="f16")
    try:
        assert_degenerate(net, True)
        run_modes(net, MCTSConfig.self_play(32), ("split",), monkeypatch, "uniform prior, 64 filters")
    finally:
        net.close()


OFF_DEFAULT = {"base50": dict(simulations=64, pb_c_base=50, pb_c_init=0.0, root_dirichlet_alpha=0.3, root_exploration_fraction=1.0,
                              num_sampling_moves=42),
               "base1e9": dict(simulations=64, pb_c_base=10 ** 9, pb_c_init=4.0, root_dirichlet_alpha=0.3,
                               root_exploration_fraction=0.5, num_sampling_moves=0)}


@pytest.mark.parametrize("name", sorted(OFF_DEFAULT))
def test_off_default_configurations_in_the_fused_kernels(oracle, monkeypatch, name):
    """The ordinary random-init net in reference precision: the A = log((N + base + 1) / base) + init table at base 50 and
    10^9, root priors that are all noise (fraction 1.0) or half noise, every move sampled or none."""
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import random_init_state_dict
    net = FusedNet(random_init_state_dict(seed=0), precision="f32x3")
    try:
        run_modes(net, MCTSConfig(**OFF_DEFAULT[name]), ("split", "wave"), monkeypatch, name, tape_seed=15)
    finally:
        net.close()
