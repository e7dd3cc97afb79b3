"""Every fused kernel libc4engine.so holds is launched here, one case per `verified` row of tests/fused_matrix.py, and
must compute what the host-driven path (c4_step + c4_net_forward, the reference side: pinned to the oracle elsewhere)
computes -- bit for bit, no tolerance anywhere.  Each case asks the engine which kernel it launched
(Engine.last_fused_kernel, c4_debug_last_fused_kernel) after the first launch and after the last: a recipe that the
dispatcher ignores would otherwise pass on the default kernel.

Nets: one stressed net per mode (answers vary strongly between positions), two residual blocks (the run-time-depth tower
loop) and, at 64 filters, six value-head Linear layers (the large MLP table).
Self-play rows: 35 slots under C4_FUSED_PACK=dense -- two full 16-slot workgroups and one of 3, or one of 32 and one of 3;
three tree waves carry 6, 6 and 4 slots --, 24 simulations, Philox noise and sampled moves, 40 games to the end, so five
slots re-root into a second game and all park while others still play.  Each row twice: 16 steps per launch, and 1 step
per launch (every launch ends with leaves in flight that prologue and epilogue carry over).
Queue rows: the 50 positions of the search-queue tests on 35 slots, 1 step per launch, against run_queue(fused=False).
Match rows: DeviceMatch(A, B, plies=1, switch=True) against the host lock-step games."""
import numpy as np
import pytest

import fused_matrix as fm
from gpu_helpers import game_key, host_lockstep_games, positions_50, same_rows
from net_models import stressed_state_dict

pytestmark = pytest.mark.gpu

N_SLOTS, SIMS, GAMES, RING = 35, 24, 40, 64
SEED = (1 << 33) + 11                  # the key's high word is set
QUEUE_SIMS = 32
COUNTERS = ("simulations", "expansions", "moves", "games_finished", "terminal_sims", "leaf_evals")
# mode -> (filters, residual blocks, value-head Linear layers, FusedNet precision)
NETS = {"f16": (32, 2, 0, "f16"), "f32x3": (32, 2, 0, "f32x3"), "f16_64": (64, 2, 6, "f16"), "f32x3w": (64, 2, 6, "f32x3w")}

VERIFIED = [r for r in fm.ROWS if r.status == "verified"]
_CACHE = {}


def once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _close_nets():
    yield
    for k, v in _CACHE.items():
        if k[0] == "net":
            v.close()
    _CACHE.clear()


def fused_net(mode, which="A"):
    """The net of a mode; "A" is net_models.grid_net's seed for two blocks, "B" the opponent of the match rows."""
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import NetConfig
    filters, n_res, n_fc, precision = NETS[mode]

    def make():
        sd = stressed_state_dict(NetConfig(filters=filters, n_residuals=n_res, n_fc_layers=n_fc), seed=20 + n_res + (which == "B"))
        net = FusedNet(sd, precision=precision)
        assert net.precision == precision
        return net
    return once(("net", mode, which), make)


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def set_env(monkeypatch, env, pack="dense"):
    for k in fm.ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("C4_FUSED_PACK", pack)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def games_of(recs):
    return [(r.game_id, r.length, r.result, list(r.move[:r.length]), list(r.color0[:r.length]), list(r.color1[:r.length]),
             _bits(list(r.value[:r.length])), np.asarray([list(p) for p in r.policy[:r.length]], dtype=np.float64).tobytes()) for r in recs]


# ---------------------------------------------------------------- self-play
def play(net, fused, steps_per_launch=16, expect=None, n_slots=N_SLOTS, games=GAMES, ring=RING):
    """One SelfPlay run to the end: (games sorted by id in comparable form, counters, all statistics).  `expect`: what
    Engine.last_fused_kernel() must say after the first launch and after the last."""
    from connect4_amd.config import MCTSConfig
    from connect4_amd.selfplay import SelfPlay
    sp = SelfPlay(net, n_slots, MCTSConfig.self_play(SIMS), seed=SEED, games_target=games, record_capacity_games=ring,
                  use_graph=False, fused_loop=fused, steps_per_launch=steps_per_launch)
    try:
        assert sp.engine.last_fused_kernel() == ""
        if fused:
            sp.run_steps(steps_per_launch)
            assert sp.engine.last_fused_kernel() == expect, "after the first launch"
        for _ in range(4000):
            sp.run_steps(64)
            st = sp.stats()
            if st["active_slots"] == 0:
                break
        assert st["active_slots"] == 0 and st["games_finished"] == games
        assert sp.engine.last_fused_kernel() == (expect if fused else ""), "after the last launch"
        recs = sorted(sp.engine.drain_games(), key=lambda r: r.game_id)
        assert [r.game_id for r in recs] == list(range(games))
        return games_of(recs), {k: st[k] for k in COUNTERS}, st
    finally:
        sp.close()


def selfplay_reference(mode):
    """The host-driven path (fused_loop=False: c4_step + c4_net_forward, eager, one stream), once per net; checked here,
    and only here, for being a reference worth comparing with: games differ from each other and end as games do."""
    def make():
        games, counters, st = play(fused_net(mode), fused=False)
        assert st["bad_evals"] == 0 and st["dropped_games"] == 0 and st["leaf_evals"] > 0
        assert len({tuple(g[3]) for g in games}) >= 30, "the reference's games are too much alike"
        assert all(7 <= g[1] <= 42 for g in games)
        return games, counters
    return once(("selfplay", mode), make)


SELFPLAY_ROWS = [r for r in VERIFIED if r.kind == "selfplay"]


@pytest.mark.parametrize("steps_per_launch", [16, 1])
@pytest.mark.parametrize("row", SELFPLAY_ROWS, ids=[r.kernel for r in SELFPLAY_ROWS])
def test_selfplay_row_plays_the_host_driven_games(monkeypatch, row, steps_per_launch):
    want_games, want_counters = selfplay_reference(row.net)
    set_env(monkeypatch, row.env)
    expect = fm.reported("selfplay", row.net, N_SLOTS, row.env, cus(), pack_dense=True)
    assert expect.startswith(row.kernel + " spread=0 grid=")
    games, counters, st = play(fused_net(row.net), True, steps_per_launch, expect)
    print("%s, %d step(s) per launch: %d leaf evaluations, %d cache hits, %d speculative" % (
        expect, steps_per_launch, st["leaf_evals"], st["eval_cache_hits"], st["speculative_evals"]))
    for mine, want in zip(games, want_games):
        assert mine[3] == want[3], "game %d: moves differ from the host-driven path's" % want[0]
        assert mine == want, "game %d: values, policies, boards or result differ from the host-driven path's" % want[0]
    assert counters == want_counters
    assert st["bad_evals"] == 0 and st["dropped_games"] == 0 and st["leaf_evals"] > 0
    # (every run here has an evaluation cache: eval_cache_log2_entries = 0 is the engine's automatic size, on for a net;
    # only a negative value turns the cache off, and without one nothing is evaluated ahead)
    if row.kernel.startswith("c4_selfplay_split_kernel") and row.net == "f16":
        assert st["eval_cache_probes"] > 0 and st["speculative_evals"] > 0


# ---------------------------------------------------------------- position queue
def evaluator(mode):
    from connect4_amd.evaluators import DeviceNetEvaluator
    return DeviceNetEvaluator(fused_net(mode))


def queue_rows(mode, **kw):
    """(rows, statistics, what Engine.last_fused_kernel() said after every launch, and at the end)"""
    from connect4_amd.analysis import run_queue
    from connect4_amd.mcts import MCTSConfig
    launched = []
    eng = run_queue(MCTSConfig(QUEUE_SIMS), positions_50(), evaluator(mode), n_slots=N_SLOTS,
                    on_launch=lambda e: launched.append(e.last_fused_kernel()), **kw)
    try:
        return eng.queue_results(), eng.stats(), launched, eng.last_fused_kernel()
    finally:
        eng.close()


def queue_reference(mode):
    def make():
        rows, st, launched, last = queue_rows(mode, fused=False)
        assert launched == [] and last == ""
        assert st["moves"] == 50 and st["bad_evals"] == 0 and len(set(rows.move.tolist())) > 1
        return rows
    return once(("queue", mode), make)


QUEUE_ROWS = [r for r in VERIFIED if r.kind == "queue"]


@pytest.mark.parametrize("row", QUEUE_ROWS, ids=[r.kernel for r in QUEUE_ROWS])
def test_queue_row_equals_the_host_driven_rows(monkeypatch, row):
    want = queue_reference(row.net)
    set_env(monkeypatch, row.env)
    expect = fm.reported("queue", row.net, N_SLOTS, row.env, cus(), pack_dense=True)
    assert expect.startswith(row.kernel + " spread=0 grid=")
    rows, st, launched, last = queue_rows(row.net, steps_per_launch=1)
    print("%s: %d leaf evaluations, %d cache hits, %d speculative" % (expect, st["leaf_evals"], st["eval_cache_hits"], st["speculative_evals"]))
    assert launched[0] == expect, "after the first launch"
    assert len(launched) > 4 and set(launched) == {expect} and last == expect, "after every launch and after the last"
    same_rows(rows, want, row.kernel)
    assert st["moves"] == 50 and st["simulations"] == 50 * QUEUE_SIMS
    assert st["bad_evals"] == 0 and st["dropped_games"] == 0 and st["leaf_evals"] > 0
    if row.kernel.startswith("c4_selfplay_split_kernel") and row.net == "f16":      # (a cache: see the self-play rows)
        assert st["eval_cache_probes"] > 0 and st["speculative_evals"] > 0


# ---------------------------------------------------------------- net-vs-net matches
def player(mode, which):
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.mcts import MCTS, MCTSConfig
    return MCTS(which, MCTSConfig(QUEUE_SIMS), DeviceNetEvaluator(fused_net(mode, which)))


MATCH_ROWS = [r for r in VERIFIED if r.kind == "match"]


@pytest.mark.parametrize("row", MATCH_ROWS, ids=[r.kernel for r in MATCH_ROWS])
def test_match_row_equals_host_lockstep(monkeypatch, row):
    from connect4_amd.match import DeviceMatch, score_results
    set_env(monkeypatch, row.env, pack="spread")
    a, b = player(row.net, "A"), player(row.net, "B")
    try:
        launched = []
        m = DeviceMatch(False, a, b, plies=1, switch=True, on_launch=lambda e: launched.append(e.last_fused_kernel()))
        assert m.n == 7 and len(m.games) == 14
        out = m.play()
        ref = [game_key(g) for g in host_lockstep_games([a, b], m.games)]
    finally:
        for p in (a, b):
            if p._searcher is not None:
                p._searcher.close()
    expect = fm.reported("match", row.net, 14, row.env, cus())
    assert expect == row.kernel + " spread=0 grid=1"
    assert launched[0] == expect, "after the first launch"
    assert len(launched) > 2 and set(launched) == {expect}, "after every launch, the last included"
    got = [game_key(r) for r in m.records]
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0], "game %d: moves differ from the host lock-step path's" % i
        assert g == r, "game %d: values, policies, boards or result differ" % i
    # the reference is worth comparing with: were A and B one function, swapping the colours would not change a game
    assert any(ref[i][0] != ref[i + 7][0] for i in range(7))
    assert out == score_results([r[4] for r in ref], 7, True)
    st = m.stats
    assert st["bad_evals"] == 0 and st["dropped_games"] == 0 and st["leaf_evals"] > 0
