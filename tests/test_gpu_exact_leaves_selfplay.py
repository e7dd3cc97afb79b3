"""Self-play and generations with an ExactLeafNet: the step path (c4_step, forward, overlay), eager and as a captured graph.

The shapes are tests/test_gpu_step_paths.py's: 32 and 19 slots, 24 simulations, 48 games, the production random streams.

1. ExactLeafNet(net, 0) plays the plain net's games bit for bit, and _play_to_completion takes the step path for it.
2. With max_empties = 14 the eager path and the captured graph (32 and 19 slots) play the same games id by id; eight of them
   -- the longest, the shortest, six at random -- are replayed move for move on the CPU oracle, whose evaluator is the net's
   answer with the exhaustive oracle's outcome laid over every position with at most 14 empty squares
   (exact_leaf_cases.OracleOverlay): the yardstick is the oracle plus the exhaustive search, not the solver.  14 and this
   seed were chosen so that the replay lays over at least 64 positions (asserted, and printed).  No device row is over budget.
3. run_generation(exact_leaves=E): E = 0 writes the rows of a run without the option bit for bit; E = 14 finishes, writes rows
   and a checkpoint of the same form, and reports the counters."""
import os

import numpy as np
import pytest

import exact_leaf_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_SLOTS = 19
SEED = (1 << 33) + 7
SIMS, GAMES, RING = 24, 48, 64
MAX_EMPTIES = 14
BUDGET = 1 << 20


@pytest.fixture(scope="module")
def net():
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import random_init_state_dict
    n = FusedNet(random_init_state_dict(seed=0))
    yield n
    n.close()


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def _play(evaluator, n_slots, **kw):
    """One run to the end on the step path: (records sorted by id, comparable form of them, SelfPlay's _graph is set)."""
    from connect4_amd.config import MCTSConfig
    from connect4_amd.selfplay import SelfPlay
    sp = SelfPlay(evaluator, n_slots, MCTSConfig.self_play(SIMS), seed=SEED, games_target=GAMES, record_capacity_games=RING,
                  fused_loop=False, pipeline=1, **kw)
    try:
        for _ in range(400):
            sp.run_steps(64)
            st = sp.stats()
            if st["active_slots"] == 0:
                break
        assert st["active_slots"] == 0 and st["games_finished"] == GAMES
        assert st["bad_evals"] == 0 and st["dropped_games"] == 0
        recs = sorted(sp.engine.drain_games(), key=lambda r: r.game_id)
        assert len(recs) == GAMES
        games = [(r.game_id, r.length, r.result, list(r.move[:r.length]), list(r.color0[:r.length]), list(r.color1[:r.length]),
                  _bits(list(r.value[:r.length])), _bits([list(p) for p in r.policy[:r.length]])) for r in recs]
        return recs, games, sp._graph is not None
    finally:
        sp.close()


@pytest.fixture(scope="module")
def plain(net):
    _, games, graph = _play(net, 32, use_graph=False)
    assert not graph
    return games


@pytest.fixture(scope="module")
def eager(net):
    """The eager step path with the overlay, 32 slots: (records, games, counters)."""
    from connect4_amd.exact_leaves import ExactLeafNet
    exact = ExactLeafNet(net, MAX_EMPTIES, node_budget=BUDGET)
    recs, games, graph = _play(exact, 32, use_graph=False)
    assert not graph
    return recs, games, exact.counters()


def test_max_empties_zero_plays_the_plain_nets_games(net, plain):
    from connect4_amd.exact_leaves import ExactLeafNet
    exact = ExactLeafNet(net, 0)
    _, games, graph = _play(exact, N_SLOTS, use_graph=True, steps_per_graph=8)
    assert graph and games == plain
    assert exact.counters() == dict(overridden=0, over_budget=0, nodes=0, late=0)


def test_overlay_changes_the_games_and_is_never_over_budget(plain, eager):
    _, games, counters = eager
    print("device counters over the run: %r" % (counters,))
    assert games != plain
    assert counters["over_budget"] == 0 and counters["overridden"] == counters["late"] > 0 and counters["nodes"] >= counters["late"]


@pytest.mark.parametrize("n_slots", [32, N_SLOTS])
def test_captured_graph_plays_the_eager_games(net, eager, n_slots):
    from connect4_amd.exact_leaves import ExactLeafNet
    exact = ExactLeafNet(net, MAX_EMPTIES, node_budget=BUDGET)
    _, games, graph = _play(exact, n_slots, use_graph=True, steps_per_graph=8)
    assert graph
    for mine, want in zip(games, eager[1]):
        assert mine == want, "game %d differs from the eager path's" % want[0]
    assert exact.counters()["over_budget"] == 0


def test_games_replay_on_the_oracle_with_exhaustive_late_values(oracle, net, eager):
    from connect4_amd.config import MCTSConfig
    from oracle.replay import oracle_config, replay_games_bulk
    from test_gpu_production_replay import philox_tapes, pick
    recs = eager[0]
    cfg = MCTSConfig.self_play(SIMS)
    chosen = [recs[k] for k in pick([r.length for r in recs], [r.game_id for r in recs], 8, 3)]
    noise, u = philox_tapes(SEED, cfg.root_dirichlet_alpha, [r.game_id for r in chosen])
    overlay = K.OracleOverlay(oracle, net, MAX_EMPTIES)
    try:
        res = replay_games_bulk(oracle_config(cfg), None, overlay, chosen, noise, u, threads=16, aligned=True)
    finally:
        overlay.close()
    print("replayed %d games (lengths %r): %d positions asked, %d of them laid over by the exhaustive oracle"
          % (res["games"], [r.length for r in chosen], res["positions_asked"], overlay.laid_over))
    assert res["games"] == 8
    assert overlay.laid_over >= 64


def test_play_to_completion_takes_the_step_path(net):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.exact_leaves import ExactLeafNet
    from connect4_amd.selfplay import _play_to_completion, generate_games_packed, has_net_handle
    exact = ExactLeafNet(net, MAX_EMPTIES, node_budget=BUDGET)
    assert has_net_handle(net) and not has_net_handle(exact)
    cfg = MCTSConfig.self_play(SIMS)
    sp = _play_to_completion(cfg, exact, 16, 16, 5, 0, torch.float32, 64, True, 600.0)
    try:
        assert not sp._fused_loop and sp._graph is not None and sp.stats()["games_finished"] == 16
    finally:
        sp.close()
    packed = generate_games_packed(cfg, exact, 16, n_slots=16, seed=5)
    assert packed.n_games == 16 and exact.counters()["late"] > 0


def _trainer():
    from connect4_amd.training import ModelConfig, Trainer
    torch.manual_seed(0)
    return Trainer(ModelConfig(batch_size=256, n_training_epochs=2, use_gpu=True))


def test_run_generation_with_exact_leaves(tmp_path):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.exact_leaves import DEFAULT_NODE_BUDGET
    from connect4_amd.generation import run_generation
    cfg = MCTSConfig.self_play(16)
    dirs = {k: str(tmp_path / k) for k in ("plain", "zero", "exact")}
    t = {k: {} for k in dirs}
    g0, _ = run_generation(_trainer(), cfg, GAMES, dirs["plain"], gen=1, n_slots=GAMES, timings=t["plain"])
    g1, _ = run_generation(_trainer(), cfg, GAMES, dirs["zero"], gen=1, n_slots=GAMES, timings=t["zero"], exact_leaves=0)
    g2, loss = run_generation(_trainer(), cfg, GAMES, dirs["exact"], gen=1, n_slots=GAMES, timings=t["exact"], exact_leaves=MAX_EMPTIES,
                              exact_leaf_budget=BUDGET)
    assert "exact_leaves" not in t["plain"]
    assert t["zero"]["exact_leaves"] == dict(max_empties=0, node_budget=DEFAULT_NODE_BUDGET, overridden=0, over_budget=0, nodes=0, late=0)
    c = t["exact"]["exact_leaves"]
    print("run_generation(exact_leaves=%d): %r" % (MAX_EMPTIES, c))
    assert c["max_empties"] == MAX_EMPTIES and c["node_budget"] == BUDGET and c["over_budget"] == 0 and c["overridden"] == c["late"] > 0
    assert loss is not None and np.isfinite(loss)
    d0, d1, d2 = (torch.load(os.path.join(dirs[k], "1", "data.pth"), weights_only=True) for k in ("plain", "zero", "exact"))
    # max_empties = 0: the plain run's games and rows, bit for bit
    assert all(getattr(g0, k).equal(getattr(g1, k)) for k in ("boards", "moves", "targets", "results"))
    assert all(d0[k].equal(d1[k]) for k in ("boards", "values", "priors"))
    # max_empties = 14: rows and a checkpoint of the same form
    assert g2.n_games == GAMES and t["exact"]["training_rows"] == int(d2["boards"].shape[0]) >= int(g2.n_positions) > GAMES
    for k in ("boards", "values", "priors"):
        assert d2[k].dtype == d0[k].dtype and d2[k].shape[1:] == d0[k].shape[1:] and d2[k].shape[0] == d2["boards"].shape[0]
    n0, n2 = (torch.load(os.path.join(dirs[k], "1", "net.pth"), map_location="cpu", weights_only=True) for k in ("plain", "exact"))
    assert n0.keys() == n2.keys()
    assert {k: v.shape for k, v in n0["net_state_dict"].items()} == {k: v.shape for k, v in n2["net_state_dict"].items()}
    with pytest.raises(ValueError):
        run_generation(_trainer(), cfg, GAMES, None, exact_leaf_budget=64)
