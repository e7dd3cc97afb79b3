"""The host-driven step paths, pinned to the games the eager single-stream path plays.

Nearly every self-play test drives c4_selfplay_steps, the persistent fused kernel.  What serves everything that kernel
does not -- a PyTorch InferenceNet fed through the planes buffer, bench.py --pipeline 2 and --fused-loop 0 -- alternates
c4_step / c4_step_range launches with a network call, optionally captured in a HIP graph, optionally split into two halves
on two streams.  The eager single-stream bitboard path (c4_step + c4_net_forward) is already pinned to the fused kernels id
by id (test_gpu_api.py::test_fused_selfplay_kernel_equals_separate_kernels) and to the CPU oracle move for move
(test_gpu_production_replay.py); it is the reference here.  A game is a pure function of (seed, game id) and a
deterministic evaluator, so every comparison is exact:

1. the planes c4_step emits (float32, fp16, bf16) equal c4_board_planes of the emitted leaf, in the leaf's own row, and no
   other row is touched -- c4_step_range included;
2. a search advanced only through c4_step_range (ranges that end inside an 8-slot block, slots outside the range untouched,
   buffers indexed by absolute slot) ends with the roots of whole steps and of the oracle;
3. SelfPlay through a captured graph, through two phase-shifted streams (eager and captured; no cache, a 256-entry cache, the
   default cache shared by both streams), and through the planes buffer in all three dtypes (eager and captured, via
   gpu_helpers.PlanesAdapter) plays the eager single-stream path's games id by id, for several slot counts; games of the
   captured two-stream run are replayed on the oracle as well;
4. c4_clear_eval_cache leaves no entry behind: a search with another net after it equals that of a fresh engine.
"""
import numpy as np
import pytest

from gpu_helpers import PlanesAdapter, random_undecided_positions, root_fields

pytestmark = pytest.mark.gpu

N_SLOTS = 19                     # three 8-slot blocks, the last ragged
SEED = (1 << 33) + 7             # the key's high word is set
SIMS, GAMES, RING = 24, 48, 64


def _torch_dtypes():
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _planes_code(name):
    from connect4_amd import _lib as L
    return {"f32": L.PLANES_F32, "f16": L.PLANES_F16, "bf16": L.PLANES_BF16}[name]


def _keys(boards):
    return [b.key()[0] for b in boards], [b.key()[1] for b in boards]


# ---------------------------------------------------------------------------------------------- 1. planes emission
def _planes_engine(dtype_name, c0, c1):
    import torch
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    eng = Engine(N_SLOTS, 40, eval_mode=L.EVAL_EXTERNAL_F32, stop_after_move=True, planes_dtype=_planes_code(dtype_name))
    eng.reset(c0, c1)
    planes = torch.full((N_SLOTS, 3, 6, 7), 7.0, dtype=_torch_dtypes()[dtype_name], device="cuda")
    values = torch.full((N_SLOTS,), 0.5, dtype=torch.float32, device="cuda")
    priors = torch.full((N_SLOTS, 7), 1.0 / 7.0, dtype=torch.float32, device="cuda")
    return eng, values, priors, planes


@pytest.mark.parametrize("dtype_name", ["f32", "f16", "bf16"])
def test_step_emits_the_leaf_planes_in_the_leaf_row_only(oracle, dtype_name):
    """After every c4_step: a slot with a leaf holds c4_board_planes(leaf) (pinned to the reference's to_array by
    tests/golden/board.json) cast to the planes dtype in ITS row; every other row is what it was before the step -- the
    sentinel, or the slot's last leaf."""
    import torch
    from connect4_amd.engine import board_planes
    c0, c1 = _keys(random_undecided_positions(oracle, N_SLOTS, seed=21))
    eng, values, priors, planes = _planes_engine(dtype_name, c0, c1)
    dtype = planes.dtype
    with eng:
        before = planes.cpu()
        n_leaf = n_kept = n_sentinel = 0
        for _ in range(1000):
            eng.step(values, priors, planes)
            l0, l1, has = eng.read_leaves()            # (synchronises the device)
            now = planes.cpu()
            want = torch.from_numpy(board_planes(l0, l1)).to(dtype)
            for g in range(N_SLOTS):
                if has[g]:
                    assert torch.equal(now[g], want[g]), "slot %d: planes are not those of its leaf" % g
                    n_leaf += 1
                else:
                    assert torch.equal(now[g], before[g]), "slot %d emitted no leaf but its row changed" % g
                    n_kept += 1
                    n_sentinel += bool((now[g] == 7.0).all())
            before = now
            if eng.stats()["active_slots"] == 0:
                break
        st = eng.stats()
        assert st["active_slots"] == 0 and st["simulations"] == 40 * N_SLOTS
        assert n_leaf > N_SLOTS and n_kept > 0
        print("%s: %d leaf rows, %d untouched rows (%d still the sentinel)" % (dtype_name, n_leaf, n_kept, n_sentinel))


def test_step_range_emits_planes_for_its_slots_only(oracle):
    """c4_step_range [8,+5): the range ends inside the second block.  Rows and has_leaf of slots 0..7 and 13..18 stay
    untouched; slots 8..12 emit their root into rows 8..12 (the buffers are indexed by absolute slot)."""
    import torch
    from connect4_amd.engine import board_planes
    c0, c1 = _keys(random_undecided_positions(oracle, N_SLOTS, seed=22))
    eng, values, priors, planes = _planes_engine("f32", c0, c1)
    with eng:
        assert not eng.read_leaves()[2].any()
        eng.step_range(values, priors, planes, 8, 5)
        l0, l1, has = eng.read_leaves()
        now = planes.cpu()
        inside = np.arange(8, 13)
        outside = np.r_[0:8, 13:N_SLOTS]
        assert (now[torch.from_numpy(outside)] == 7.0).all()
        assert not has[outside].any()
        assert has[inside].all()
        # the first leaf of a search is its root
        assert l0[inside].tolist() == c0[8:13] and l1[inside].tolist() == c1[8:13]
        assert torch.equal(now[8:13], torch.from_numpy(board_planes(c0[8:13], c1[8:13])))


# ---------------------------------------------------------------------------------------------- 2. c4_step_range
def test_step_range_searches_equal_whole_steps_and_the_oracle(oracle):
    """Engine A: c4_run_centre (whole steps).  Engine B: only c4_step_range -- [0,8) to the end, then [8,+5) to the end
    (slots 13..18 must not have moved), then [8,+11).  40 simulations per launch, so every search spans several launches.
    B == A field by field, and both == the oracle.  Bad ranges are refused with C4_EINVAL and change nothing."""
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    boards = random_undecided_positions(oracle, N_SLOTS, seed=23)
    c0, c1 = _keys(boards)
    c = dict(simulations=150, pb_c_base=19652, pb_c_init=1.25, root_dirichlet_alpha=0.0, root_exploration_fraction=0.0,
             num_sampling_moves=0)

    def engine():
        e = Engine(N_SLOTS, eval_mode=L.EVAL_CENTRE, stop_after_move=True, max_inner_iters=40, **c)
        e.reset(c0, c1)
        return e

    def states(e, lo, hi):
        return [r.state for r in e.read_roots()[lo:hi]]

    def run_range(e, lo, cnt, done_lo, done_hi):
        for launches in range(1, 65):
            e.step_range(None, None, None, lo, cnt)
            if all(s == L.SLOT_MOVE_DONE for s in states(e, done_lo, done_hi)):
                return launches
        raise AssertionError("slots [%d,%d) did not finish" % (done_lo, done_hi))

    with engine() as a, engine() as b:
        a.run_centre()
        fresh = [root_fields(r) for r in b.read_roots()]
        assert all(f["state"] == L.SLOT_ACTIVE for f in fresh)
        # a slot that has not been stepped has no tree, whatever its pool's memory held before
        assert all(f["root_visits"] == 0 and f["child_status"] == [-2] * 7 and f["child_visits"] == [0] * 7 for f in fresh)
        for lo, cnt in ((4, 4), (8, 12), (16, 4), (8, 0), (-8, 8)):
            with pytest.raises(L.EngineError) as err:
                b.step_range(None, None, None, lo, cnt)
            assert err.value.code == L.EINVAL
        assert [root_fields(r) for r in b.read_roots()] == fresh
        assert run_range(b, 0, 8, 0, 8) >= 4
        assert [root_fields(r) for r in b.read_roots()[8:]] == fresh[8:]
        with pytest.raises(L.EngineError) as err:       # ... and in the middle of a run
            b.step_range(None, None, None, 4, 4)
        assert err.value.code == L.EINVAL
        assert run_range(b, 8, 5, 8, 13) >= 4
        assert [root_fields(r) for r in b.read_roots()[13:]] == fresh[13:]       # state 0, root_visits as after reset
        run_range(b, 8, 11, 8, N_SLOTS)
        ra, rb = a.read_roots(), b.read_roots()
        sa, sb = a.stats(), b.stats()
    cfg = oracle.make_config(**c)
    for g, board in enumerate(boards):
        assert root_fields(rb[g]) == root_fields(ra[g]), "slot %d" % g
        info, mv, av = oracle.search_and_pick(cfg, board, oracle.CentreEvaluator())
        for r in (ra[g], rb[g]):
            assert r.state == L.SLOT_MOVE_DONE
            assert r.root_visits == info.root_visits == 151
            assert list(r.child_visits) == list(info.child_visits)
            assert list(r.child_value_sum) == list(info.child_value_sum)
            assert list(r.child_status) == list(info.child_status)
            assert list(r.values_policy) == list(info.values_policy)
            assert r.move == mv
            assert (np.isnan(r.value) and np.isnan(av)) or r.value == av
            assert r.expansions == info.n_expansions
    for k in ("simulations", "expansions", "children_created", "terminal_sims", "moves"):
        assert sa[k] == sb[k], k
    assert sb["simulations"] == 150 * N_SLOTS and sb["moves"] == N_SLOTS


# ---------------------------------------------------------------------------------------------- 3. SelfPlay paths
@pytest.fixture(scope="module")
def net():
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import random_init_state_dict
    n = FusedNet(random_init_state_dict(seed=0))
    assert n.precision == "f32x3"
    yield n
    n.close()


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def _play(evaluator, n_slots, **kw):
    """One run to the end: (records sorted by id, comparable form of them, counters, SelfPlay's _graph is set, _pipeline)."""
    from connect4_amd.config import MCTSConfig
    from connect4_amd.selfplay import SelfPlay
    sp = SelfPlay(evaluator, n_slots, MCTSConfig.self_play(SIMS), seed=SEED, games_target=GAMES, record_capacity_games=RING,
                  fused_loop=False, **kw)
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
        counters = {k: st[k] for k in ("simulations", "moves", "games_finished")}
        return recs, games, counters, sp._graph is not None, sp._pipeline
    finally:
        sp.close()


@pytest.fixture(scope="module")
def baseline(net):
    """The eager single-stream bitboard path without an evaluation cache: c4_step + c4_net_forward, 32 slots."""
    _, games, counters, graph, pipeline = _play(net, 32, use_graph=False, pipeline=1, eval_cache_log2_entries=-1)
    assert not graph and pipeline == 1
    assert [g[0] for g in games] == list(range(GAMES))
    return games, counters


def _assert_same_games(got, baseline):
    games, counters = got
    for mine, want in zip(games, baseline[0]):
        assert mine == want, "game %d differs from the eager single-stream path's" % want[0]
    assert counters == baseline[1]


@pytest.mark.parametrize("n_slots", [32, N_SLOTS])
def test_captured_graph_plays_the_eager_games(net, baseline, n_slots):
    _, games, counters, graph, pipeline = _play(net, n_slots, use_graph=True, steps_per_graph=8, pipeline=1)
    assert graph and pipeline == 1
    _assert_same_games((games, counters), baseline)


@pytest.mark.parametrize("cache_bits", [-1, 8, 0])
@pytest.mark.parametrize("n_slots", [32, 48])
def test_two_streams_play_the_eager_games(net, baseline, n_slots, cache_bits):
    """pipeline=2, eager: two halves (16, or 24 slots = three blocks each) on two streams, phase-shifted, sharing the
    evaluation cache (none / 256 entries under constant eviction / the default), the record ring and the id counter."""
    _, games, counters, graph, pipeline = _play(net, n_slots, use_graph=False, pipeline=2, eval_cache_log2_entries=cache_bits)
    assert pipeline == 2 and not graph
    _assert_same_games((games, counters), baseline)


@pytest.mark.parametrize("dtype_name", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("n_slots", [32, N_SLOTS])
@pytest.mark.parametrize("use_graph", [False, True])
def test_planes_fed_evaluator_plays_the_eager_games(net, baseline, use_graph, n_slots, dtype_name):
    """The path every PyTorch net takes (c4_step writes planes, the net reads them), with an evaluator that answers with
    the fused net's bits for whatever board the planes encode: the cells are 0.0 and 1.0, so every dtype is exact."""
    _, games, counters, graph, pipeline = _play(PlanesAdapter(net), n_slots, use_graph=use_graph, steps_per_graph=8, pipeline=1,
                                                planes_dtype=_torch_dtypes()[dtype_name])
    assert graph == use_graph and pipeline == 1
    _assert_same_games((games, counters), baseline)


def test_captured_two_streams_play_the_eager_games_and_replay_on_the_oracle(oracle, net, baseline):
    """pipeline=2 captured: one graph with two parallel branches.  Its games equal the baseline's, and eight of them
    (the longest, the shortest, six at random) are replayed move for move on the CPU oracle, answered by the net."""
    from connect4_amd.config import MCTSConfig
    from oracle.replay import oracle_config, replay_games_bulk
    from test_gpu_production_replay import philox_tapes, pick
    recs, games, counters, graph, pipeline = _play(net, 32, use_graph=True, steps_per_graph=8, pipeline=2)
    assert pipeline == 2 and graph
    _assert_same_games((games, counters), baseline)
    cfg = MCTSConfig.self_play(SIMS)
    chosen = [recs[k] for k in pick([r.length for r in recs], [r.game_id for r in recs], 8, 3)]
    noise, u = philox_tapes(SEED, cfg.root_dirichlet_alpha, [r.game_id for r in chosen])
    res = replay_games_bulk(oracle_config(cfg), None, net, chosen, noise, u, threads=16, aligned=True)
    assert res["games"] == 8 and res["lost_by_the_table"] == 0


# ---------------------------------------------------------------------------------------------- 4. c4_clear_eval_cache
def _drive_bits(eng, evaluator):
    """The bitboard loop of connect4_amd.mcts._Searcher._drive_device."""
    import torch
    n = eng.n_slots
    values = torch.zeros(n, dtype=torch.float32, device="cuda")
    priors = torch.zeros(n, 7, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    eng.set_stream(stream)
    c0p, c1p, _ = eng.leaf_buffers()
    eng.step(None, None, None)
    for _ in range(10000):
        evaluator.forward_bitboards(c0p, c1p, n, values, priors, stream)
        eng.step(values, priors, None)
        if eng.stats()["active_slots"] == 0:
            return
    raise AssertionError("the searches did not finish")


def test_clear_eval_cache_leaves_nothing_of_the_old_net(oracle, net):
    """Search with net A, clear, search the same positions with net B: the cache answers for none of A's positions after
    the clear, and B's roots are those of an engine that never saw A."""
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import random_init_state_dict
    boards = random_undecided_positions(oracle, 8, seed=24)
    c0, c1 = _keys(boards)

    def engine(cache_bits=16):
        return Engine(8, 60, eval_mode=L.EVAL_EXTERNAL_F32, stop_after_move=True, eval_cache_log2_entries=cache_bits)

    net_b = FusedNet(random_init_state_dict(seed=1))
    try:
        with engine() as eng, engine() as fresh:
            eng.reset(c0, c1)
            _drive_bits(eng, net)
            roots_a = eng.read_roots()
            # the roots, and every child a simulation went through that is not decided, were evaluated and inserted
            k0, k1, evaluated = list(c0), list(c1), [True] * 8
            for r, b in zip(roots_a, boards):
                m = b.valid_mask()
                for col in range(7):
                    if (m >> col) & 1:
                        k = b.copy()
                        k.make_move(col)
                        k0.append(k.key()[0])
                        k1.append(k.key()[1])
                        evaluated.append(k.result == -1 and r.child_visits[col] > 0)
            evaluated = np.array(evaluated)
            v, p, found = eng.cache_lookup(k0, k1)
            # at most 8 x 61 insertions into 2^16 direct-mapped entries: a probed position was overwritten by a later
            # one with probability < 1 %, so far fewer than a tenth of them are gone
            assert evaluated.sum() >= 24 and found[evaluated].sum() >= 0.9 * evaluated.sum()
            va, pa = net.evaluate_bits(np.array(k0, dtype=np.uint64), np.array(k1, dtype=np.uint64), wave=True)
            assert np.array_equal(v[found], va[found]) and np.array_equal(p[found], pa[found])
            eng.clear_eval_cache()
            assert not eng.cache_lookup(k0, k1)[2].any()
            eng.reset(c0, c1)
            _drive_bits(eng, net_b)
            fresh.reset(c0, c1)
            _drive_bits(fresh, net_b)
            got, want = eng.read_roots(), fresh.read_roots()
            for g in range(8):
                assert root_fields(got[g]) == root_fields(want[g]), "slot %d was served another net's answers" % g
            assert any(root_fields(got[g]) != root_fields(roots_a[g]) for g in range(8))     # the nets do differ
        with engine(cache_bits=-1) as nocache:
            nocache.clear_eval_cache()
    finally:
        net_b.close()
