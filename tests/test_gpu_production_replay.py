"""Self-play on the PRODUCTION random streams (C4_RNG_PHILOX, SelfPlay's default and what bench.py, run_generation and
generate_games* run) replayed move for move on the CPU oracle.  No tapes go into the engine: the oracle's tapes are what
the engine's streams drew for each recorded game -- the opening-move uniforms from the host model oracle/philox_ref.py
(bit-exact against the device, tests/test_gpu_rng.py) and the root noise from c4_debug_root_noise, the device function
the kernel calls (exact by construction; test_gpu_rng.py ties it to the model).  A stream keyed by the wrong seed, game
id or ply, in any slot or generation, changes an opening and the replay fails.

(a) configs[1]: 4096 games x 800 simulations, games_target = G, with the f32x3 and the fp16 net;
(b) continuous mode as the bench runs it (games_target = -1): at least half the replayed games were played on reused
    slots (game id >= n_slots), where a slot that kept its old ply or game id would show;
(c) configs[4] at size through run_generation (8192 games with the default slots, and the reference's 1200 games on 1200
    slots) at gen 1 and seed s != 0, so that the engine's key s + 1000*gen + rank is the one replayed; the engine is
    gone by then, so the oracle is answered by the net the generation played with (its cache held exactly the net's
    answers, test_gpu_records.py::test_eval_cache_lookup_returns_the_nets_answers), and the exported PackedGames hold
    float32 values / policies: compared as np.float32(oracle) == packed.

Moves, boards, results and (a, b) float64 values and policies must be IDENTICAL, with the bounds of test_gpu_fullsize.py
on the share of positions the evaluation cache has lost.
"""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = (1 << 33) + 2024          # the key's high word is set
N_REPLAY = 128


def philox_tapes(seed, alpha, gids):
    """(noise[n][42][7], u[n][42]) for game ids `gids` of a C4_RNG_PHILOX engine keyed by `seed`; prints how many noise
    draws the host model gives bit for bit."""
    from connect4_amd.engine import debug_root_noise
    from oracle import philox_ref as R
    g = np.asarray(gids, dtype=np.int64)
    n = len(g)
    plies = np.arange(42)
    u, _ = R.uniform2(seed, g[:, None], plies[None, :], R.MOVE_STREAM, 0)
    raw, _ = debug_root_noise(seed, alpha, np.repeat(g, 42), np.tile(plies, n).astype(np.int32), np.full(n * 42, 0x7f, dtype=np.int32))
    noise = raw.reshape(n, 42, 7)
    model, _ = R.production_tapes(seed, alpha, g)
    print("tapes for %d games: %d of %d noise draws bit-equal to the host model" %
          (n, int(np.count_nonzero(model.view(np.uint64) == noise.view(np.uint64))), noise.size))
    return noise, u


def pick(lengths, ids, n, seed, pool=None):
    """n record indices: the longest and the shortest game, the rest at random (from `pool` if given)."""
    lengths = np.asarray(lengths)
    pool = np.arange(len(lengths)) if pool is None else np.asarray(pool)
    out = {int(pool[np.argmax(lengths[pool])]), int(pool[np.argmin(lengths[pool])])}
    rng = np.random.RandomState(seed)
    for k in rng.permutation(pool):
        if len(out) >= n:
            break
        out.add(int(k))
    return sorted(out, key=lambda k: ids[k])


def report(tag, res, lost_share_max):
    print("%s: %d games replayed on the oracle, %d positions asked in %d rounds, %d lost by the table (re-evaluated by the net)"
          % (tag, res["games"], res["positions_asked"], res["rounds"], res["lost_by_the_table"]))
    assert res["positions_asked"] > 1000
    assert res["lost_by_the_table"] <= lost_share_max * res["positions_asked"]


def _selfplay(G, S, precision, seed, games_target, rec_cap):
    import inspect
    from connect4_amd import _lib as L
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import random_init_state_dict
    from connect4_amd.selfplay import SelfPlay
    assert inspect.signature(SelfPlay).parameters["rng_mode"].default == L.RNG_PHILOX      # production = the default
    cfg = MCTSConfig.self_play(S)
    net = FusedNet(random_init_state_dict(seed=0), precision=precision)
    sp = SelfPlay(net, G, cfg, seed=seed, games_target=games_target, record_capacity_games=rec_cap, use_graph=False,
                  fused_loop=True, steps_per_launch=128, max_inner_iters=32)
    return sp, net, cfg


@pytest.mark.parametrize("precision", [None, "f16"])
def test_config1_philox_selfplay_replays_on_the_oracle(oracle, precision):
    from oracle.replay import oracle_config, replay_games_bulk
    G, S = 4096, 800
    sp, net, cfg = _selfplay(G, S, precision, SEED, G, G)
    try:
        for _ in range(4000):
            sp.run_steps(256)
            st = sp.stats()
            if st["active_slots"] == 0:
                break
        assert st["active_slots"] == 0 and st["games_finished"] == G and st["dropped_games"] == 0 and st["bad_evals"] == 0
        recs = sp.engine.drain_games()
        assert len(recs) == G and sorted(r.game_id for r in recs) == list(range(G))
        ids = [r.game_id for r in recs]
        chosen = [recs[k] for k in pick([r.length for r in recs], ids, N_REPLAY, 5)]
        noise, u = philox_tapes(SEED, cfg.root_dirichlet_alpha, [r.game_id for r in chosen])
        res = replay_games_bulk(oracle_config(cfg), sp.engine, net, chosen, noise, u, threads=16, aligned=True)
        assert res["games"] == N_REPLAY
        report("philox %d x %d %s" % (G, S, net.precision), res, 0.10)
    finally:
        sp.close()
        net.close()


def test_continuous_philox_selfplay_reused_slots_replay_on_the_oracle(oracle):
    from oracle.replay import oracle_config, replay_games_bulk
    G, S = 4096, 800
    sp, net, cfg = _selfplay(G, S, None, SEED + 1, -1, 4 * G)
    try:
        for _ in range(8000):
            sp.run_steps(256)
            st = sp.stats()
            if st["games_finished"] >= 2 * G:
                break
        assert st["games_finished"] >= 2 * G and st["dropped_games"] == 0 and st["bad_evals"] == 0
        recs = sp.engine.drain_games()
        ids = [r.game_id for r in recs]
        assert len(recs) == st["games_finished"] and len(set(ids)) == len(ids)
        reused = [k for k, g in enumerate(ids) if g >= G]
        assert len(reused) >= G
        lengths = [r.length for r in recs]
        first = pick(lengths, ids, N_REPLAY // 2, 6, pool=[k for k, g in enumerate(ids) if g < G])
        later = pick(lengths, ids, N_REPLAY // 2, 7, pool=reused)
        chosen = [recs[k] for k in first + later]
        noise, u = philox_tapes(SEED + 1, cfg.root_dirichlet_alpha, [r.game_id for r in chosen])
        res = replay_games_bulk(oracle_config(cfg), sp.engine, net, chosen, noise, u, threads=16, aligned=True)
        assert res["games"] == N_REPLAY and sum(r.game_id >= G for r in chosen) >= N_REPLAY // 2
        report("philox continuous %d slots x %d, %d games finished, max replayed id %d"
               % (G, S, st["games_finished"], max(r.game_id for r in chosen)), res, 0.10)
    finally:
        sp.close()
        net.close()


@pytest.mark.parametrize("n_games,n_slots", [(8192, None), (1200, 1200)])
def test_config4_generation_at_size_replays_on_the_oracle(oracle, tmp_path, n_games, n_slots):
    import torch
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import make_selfplay_net
    from connect4_amd.generation import run_generation
    from connect4_amd.training import Trainer
    from oracle.replay import oracle_config, packed_records, replay_games_bulk
    seed, gen = 4321, 1
    torch.manual_seed(0)
    tr = Trainer(device="cuda")
    played_by = {k: v.detach().cpu().clone() for k, v in tr.net.state_dict().items()}    # before run_generation trains
    cfg = MCTSConfig.self_play(800)
    games, loss = run_generation(tr, cfg, n_games, save_dir=str(tmp_path), gen=gen, seed=seed, n_slots=n_slots)
    assert games.n_games == n_games and games.ids.cpu().tolist() == list(range(n_games))
    data = torch.load(os.path.join(str(tmp_path), str(gen), "data.pth"), weights_only=True)
    rows = 2 * games.n_positions                                   # flip augmentation
    assert data["boards"].shape == (rows, 3, 6, 7) and data["values"].shape == (rows,) and data["priors"].shape == (rows, 7)
    assert loss is not None and math.isfinite(loss)
    again = Trainer(file_name=os.path.join(str(tmp_path), str(gen), "net.pth"), device="cuda")
    trained = tr.net.state_dict()
    assert all(torch.equal(v.cpu(), trained[k].cpu()) for k, v in again.net.state_dict().items())
    assert any(not torch.equal(v, trained[k].cpu()) for k, v in played_by.items())   # training did change the net
    engine_seed = seed + 1000 * gen + 0                            # rank 0 of one: its local game ids are the global ones
    lengths = games.lengths.cpu().numpy()
    ids = games.ids.cpu().tolist()
    recs = packed_records(games, pick(lengths, ids, N_REPLAY, 8))
    net = make_selfplay_net(played_by)
    try:
        noise, u = philox_tapes(engine_seed, cfg.root_dirichlet_alpha, [r.game_id for r in recs])
        res = replay_games_bulk(oracle_config(cfg), None, net, recs, noise, u, threads=16, aligned=True)
    finally:
        if hasattr(net, "close"):
            net.close()
    assert res["games"] == N_REPLAY and res["lost_by_the_table"] == 0
    report("generation %d games on %s slots (engine seed %d)" % (n_games, n_slots or "default", engine_seed), res, 0.0)
