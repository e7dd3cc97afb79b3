"""The position queue (c4_queue_positions ..., connect4_amd.analysis.search_positions, stats.score_search): N positions
searched by G slots inside the stepping kernels.  A row must be what ONE search of that position gives -- the oracle's for
the centre evaluator, the one-slot-per-position path's (`_Searcher.run`, itself pinned to the oracle) for a net, bit for
bit -- whatever the number of slots, the kernel, the launch length or the evaluation cache do."""
import numpy as np
import pytest

from gpu_helpers import positions_50, random_undecided_positions, same_rows
from net_models import stressed_state_dict

pytestmark = pytest.mark.gpu

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
            v.net.close()
    _CACHE.clear()


# ---------------------------------------------------------------- centre evaluator against the oracle
def centre_cfg(sims):
    return dict(simulations=sims, pb_c_base=19652, pb_c_init=1.25, root_dirichlet_alpha=0.0, root_exploration_fraction=0.0,
                num_sampling_moves=0)


def oracle_200(oracle):
    def make():
        rng = np.random.RandomState(23)
        boards = []
        while len(boards) < 200:        # as test_gpu_search.py generates its 2,048
            b = oracle.Board.empty()
            for _ in range(int(rng.randint(0, 41))):
                m = b.valid_mask()
                if not m:
                    break
                b.make_move(int(rng.choice([c for c in range(7) if (m >> c) & 1])))
            if b.result == -1:
                boards.append(b)
        cfg = oracle.make_config(**centre_cfg(64))
        return boards, [oracle.search_and_pick(cfg, b, oracle.CentreEvaluator()) for b in boards]
    return once(("oracle", 200), make)


def assert_row_is_oracle(r, b, ref, sims):
    info, mv, av = ref
    assert r.state == 2
    assert (int(r.color0), int(r.color1)) == tuple(int(x) for x in b.key())
    assert r.root_visits == info.root_visits == sims + 1
    assert r.root_value_sum == info.root_value_sum
    assert list(r.child_visits) == list(info.child_visits)
    assert list(r.child_value_sum) == list(info.child_value_sum)
    assert list(r.child_status) == list(info.child_status)
    assert list(r.values_policy) == list(info.values_policy)
    assert list(r.root_prior) == list(info.root_prior)
    assert r.move == mv
    assert (np.isnan(r.value) and np.isnan(av)) or r.value == av
    assert r.expansions == info.n_expansions
    assert r.simulations == sims


@pytest.mark.parametrize("n_slots", [1, 7, 16, 200])
def test_centre_rows_equal_the_oracle(oracle, n_slots):
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    boards, refs = oracle_200(oracle)
    with Engine(n_slots, eval_mode=L.EVAL_CENTRE, stop_after_move=True, position_queue=True, **centre_cfg(64)) as eng:
        eng.queue_positions([b.key()[0] for b in boards], [b.key()[1] for b in boards])
        eng.run_centre(max_launches=1 << 16)
        assert eng.queue_progress() == (200, 200)
        rows = eng.queue_results()
        st = eng.stats()
    for r, b, ref in zip(rows, boards, refs):
        assert_row_is_oracle(r, b, ref, 64)
    assert st["moves"] == 200 and st["simulations"] == 200 * 64 and st["active_slots"] == 0
    assert st["expansions"] == sum(ref[0].n_expansions for ref in refs) and st["games_started"] == 200


def test_many_pulls_per_slot(oracle):
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    boards = random_undecided_positions(oracle, 5000, seed=29, max_plies=36)
    c0, c1 = [b.key()[0] for b in boards], [b.key()[1] for b in boards]
    with Engine(64, eval_mode=L.EVAL_CENTRE, stop_after_move=True, position_queue=True, **centre_cfg(8)) as eng:
        eng.queue_positions(c0, c1)
        eng.run_centre(max_launches=1 << 16)
        assert eng.queue_progress() == (5000, 5000)
        rows = eng.queue_results()
        st = eng.stats()
        assert [r.state for r in eng.read_roots()] == [L.SLOT_PARKED] * 64
    assert (rows.state == 2).all() and (rows.root_visits == 9).all() and (rows.simulations == 8).all()
    assert rows.color0.tolist() == [int(x) for x in c0] and rows.color1.tolist() == [int(x) for x in c1]
    assert st["moves"] == 5000 and st["simulations"] == 5000 * 8 and st["active_slots"] == 0
    cfg = oracle.make_config(**centre_cfg(8))
    for i in np.random.RandomState(1).choice(5000, 64, replace=False).tolist():
        assert_row_is_oracle(rows[i], boards[i], oracle.search_and_pick(cfg, boards[i], oracle.CentreEvaluator()), 8)


# ---------------------------------------------------------------- a net: the fused kernels against the one-slot path
SIMS = 32


def evaluator(precision="f32x3", filters=32):
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import NetConfig
    return once(("net", precision, filters), lambda: DeviceNetEvaluator(FusedNet(
        stressed_state_dict(NetConfig(filters=filters, n_residuals=1, n_fc_layers=1), seed=131), precision=precision)))


def one_slot_path(cfg, ev, boards, seed=None):
    """`_Searcher.run`: one slot per position, host-driven c4_step + forward (what MCTS.make_moves runs)."""
    from connect4_amd.mcts import _Searcher
    s = _Searcher(cfg, ev)
    try:
        if seed is not None:
            np.random.seed(seed)
        return s.run(boards)
    finally:
        s.close()


def reference_50(precision):
    from connect4_amd.mcts import MCTSConfig
    return once(("ref50", precision), lambda: one_slot_path(MCTSConfig(SIMS), evaluator(precision), positions_50()))


@pytest.mark.parametrize("precision", ["f32x3", "f16"])
@pytest.mark.parametrize("n_slots", [18, 50])
def test_fused_rows_equal_the_one_slot_path(precision, n_slots):
    """18 slots: the second workgroup of 16 holds 2; 50: spread over the CUs, every slot searches one position."""
    from connect4_amd.analysis import search_positions
    from connect4_amd.mcts import MCTSConfig
    rows = search_positions(MCTSConfig(SIMS), positions_50(), evaluator(precision), n_slots=n_slots)
    same_rows(rows, reference_50(precision), "%s, %d slots" % (precision, n_slots))


def test_rows_do_not_depend_on_launches_cache_or_driver():
    from connect4_amd.analysis import run_queue
    from connect4_amd.mcts import MCTSConfig
    cfg, ev, boards, want = MCTSConfig(SIMS), evaluator("f32x3"), positions_50(), reference_50("f32x3")
    for what, kw, hits in (("1 step per launch", dict(steps_per_launch=1), True), ("64 steps per launch", dict(steps_per_launch=64), True),
                           ("cache off", dict(eval_cache_log2_entries=-1), False), ("cache 2^12", dict(eval_cache_log2_entries=12), True),
                           ("host-driven c4_step + forward", dict(fused=False), True),
                           ("host-driven, cache off", dict(fused=False, eval_cache_log2_entries=-1), False)):
        eng = run_queue(cfg, boards, ev, n_slots=18, **kw)
        try:
            rows, st = eng.queue_results(), eng.stats()
        finally:
            eng.close()
        same_rows(rows, want, what)
        assert st["moves"] == 50 and st["simulations"] == 50 * SIMS
        assert (st["eval_cache_hits"] > 0) == hits, (what, st)


@pytest.mark.parametrize("mode,slots,precision", [("wave", 16, "f16"), ("wave", 32, "f16"), ("wave", 16, "f32x3"),
                                                  ("block", 16, "f16"), ("block", 32, "f16")])
def test_older_fused_kernels_serve_a_queue(monkeypatch, mode, slots, precision):
    """The position-queue twins of the wave-autonomous and the workgroup-synchronous kernel.  18 slots: the last workgroup is
    ragged (2 of 16 slots, 18 of 32); one step per launch: every launch ends with leaves in flight, so the rows pass through
    the kernels' launch prologue and epilogue all the time."""
    from connect4_amd.analysis import run_queue
    from connect4_amd.mcts import MCTSConfig
    monkeypatch.setenv("C4_FUSED_MODE", mode)
    monkeypatch.setenv("C4_FUSED_SLOTS", str(slots))
    monkeypatch.setenv("C4_FUSED_PACK", "dense")
    eng = run_queue(MCTSConfig(SIMS), positions_50(), evaluator(precision), n_slots=18, steps_per_launch=1)
    try:
        rows, st = eng.queue_results(), eng.stats()
    finally:
        eng.close()
    same_rows(rows, reference_50(precision), "%s kernel, %d slots per workgroup, %s" % (mode, slots, precision))
    assert st["moves"] == 50 and st["simulations"] == 50 * SIMS


def test_tapes_are_indexed_by_position():
    """Root noise and sampled moves: drawn from np.random position by position as MCTS.make_moves draws them, row i and
    ply 0 of the tapes serve position i whichever slot searches it."""
    from connect4_amd.analysis import search_positions
    from connect4_amd.mcts import MCTSConfig
    cfg = MCTSConfig(SIMS, root_dirichlet_alpha=0.3, root_exploration_fraction=0.25, num_sampling_moves=6)
    ev, boards = evaluator("f32x3"), positions_50()
    want = one_slot_path(cfg, ev, boards, seed=77)
    assert len({r.move for r in want}) > 1 and want[0].root_prior[0] != want[1].root_prior[0]
    np.random.seed(77)
    same_rows(search_positions(cfg, boards, ev, n_slots=18), want, "tape, fused")
    np.random.seed(77)
    same_rows(search_positions(cfg, boards, ev, n_slots=7, fused=False), want, "tape, host-driven")


def test_philox_streams_are_keyed_by_position(oracle):
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    boards = random_undecided_positions(oracle, 40, seed=31, max_plies=12)
    c0, c1 = [b.key()[0] for b in boards], [b.key()[1] for b in boards]
    kw = dict(centre_cfg(24), root_dirichlet_alpha=0.3, root_exploration_fraction=0.25, num_sampling_moves=8,
              eval_mode=L.EVAL_CENTRE, rng_mode=L.RNG_PHILOX, seed=5, stop_after_move=True)
    with Engine(40, **kw) as eng:       # game id = slot = index, ply 0
        eng.reset(c0, c1)
        eng.run_centre()
        want = list(eng.read_roots())
    assert len({tuple(r.root_prior) for r in want}) == 40
    with Engine(7, position_queue=True, **kw) as eng:
        eng.queue_positions(c0, c1)
        eng.run_centre(max_launches=1 << 16)
        same_rows(eng.queue_results(), want, "philox")


def test_64_filter_net_in_the_split_kernel():
    from connect4_amd.analysis import search_positions
    from connect4_amd.mcts import MCTSConfig
    cfg, ev, boards = MCTSConfig(16), evaluator("f32x3w", 64), positions_50()[15:35]
    same_rows(search_positions(cfg, boards, ev, n_slots=16), one_slot_path(cfg, ev, boards), "f32x3w")


# ---------------------------------------------------------------- device in, device out
def host_export(rows):
    n = len(rows)
    pol = np.zeros((n, 7), dtype=np.float32)
    vis = np.zeros((n, 7), dtype=np.float32)
    for i, r in enumerate(rows):
        pol[i] = np.asarray(r.values_policy, dtype=np.float64).astype(np.float32)
        p = np.zeros(7)
        kids = [m for m in range(7) if r.child_status[m] != -2]
        for m in kids:
            p[m] = r.child_visits[m]
        s = np.sum(p)
        if s == 0.0:
            p[kids] = 1.0
            p /= len(kids)
        else:
            p /= s
        vis[i] = p.astype(np.float32)
    root = (rows.root_value_sum / rows.root_visits.astype(np.float64)).astype(np.float32)
    return dict(policy=pol, visit_policy=vis, root_values=root, move_values=rows.value.astype(np.float32),
                moves=rows.move.astype(np.uint8))


def test_device_in_device_out(oracle):
    import torch

    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    boards = random_undecided_positions(oracle, 300, seed=37, max_plies=40)
    c0 = np.array([b.key()[0] for b in boards], dtype=np.uint64)
    c1 = np.array([b.key()[1] for b in boards], dtype=np.uint64)
    packed = torch.from_numpy(np.stack([c0, c1], axis=1).view(np.int64)).cuda()
    with Engine(24, eval_mode=L.EVAL_CENTRE, stop_after_move=True, position_queue=True, **centre_cfg(16)) as eng:
        eng.queue_positions(c0, c1)
        eng.run_centre(max_launches=1 << 16)
        host_rows = eng.queue_results()
        eng.queue_positions_dev(packed)
        assert eng.queue_progress() == (0, 300) and (eng.queue_results().state == 0).all()
        eng.run_centre(max_launches=1 << 16)
        rows = eng.queue_results()
        out = {k: v.cpu().numpy() for k, v in eng.queue_export().items()}
        only = eng.queue_export(("moves",))
        assert list(only) == ["moves"] and only["moves"].cpu().numpy().tolist() == out["moves"].tolist()
        assert eng.queue_results(290, 10).tobytes() == rows[290:].tobytes()
    assert rows.tobytes() == host_rows.tobytes() and (rows.state == 2).all()
    assert np.isnan(rows.value).any() or (rows.child_status >= 0).any()      # the set reaches the edge cases
    want = host_export(rows)
    for k in ("policy", "visit_policy", "root_values", "move_values"):
        assert out[k].dtype == np.float32 and out[k].view(np.uint32).tolist() == want[k].view(np.uint32).tolist(), k
    assert out["moves"].dtype == np.uint8 and out["moves"].tolist() == want["moves"].tolist()


# ---------------------------------------------------------------- refusals
def test_refusals():
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    from connect4_amd.engine import Engine
    done = Board()
    for m in (0, 1, 0, 1, 0, 1, 0):
        done.make_move(m)
    assert done.result is not None
    good = positions_50()[:9]
    bad = good[:4] + [done] + good[4:]
    kw = dict(eval_mode=L.EVAL_CENTRE, stop_after_move=True, **centre_cfg(16))
    with Engine(4, position_queue=True, **kw) as eng:
        for call in (eng.queue_progress, eng.queue_results, eng.queue_export):      # no queue yet
            with pytest.raises(L.EngineError) as ei:
                call()
            assert ei.value.code == L.ESTATE
        with pytest.raises(L.EngineError) as ei:
            eng.queue_positions([b.color[0] for b in bad], [b.color[1] for b in bad])
        assert ei.value.code == L.EINVAL and "position 4 " in str(ei.value)
        with pytest.raises(L.EngineError) as ei:        # two stones on one cell
            eng.queue_positions([1, 1], [0, 1])
        assert ei.value.code == L.EINVAL and "position 1 " in str(ei.value)
        eng.queue_positions([b.color[0] for b in good], [b.color[1] for b in good])
        with pytest.raises(L.EngineError) as ei:
            eng.queue_results(5, 5)
        assert ei.value.code == L.EINVAL
        eng.run_centre(max_launches=1 << 16)
        rows = eng.queue_results()
        assert (rows.state == 2).all() and rows.color0.tolist() == [b.color[0] for b in good]
        eng.reset()                                     # drops the queue: a plain stop-after-move engine again
        with pytest.raises(L.EngineError) as ei:
            eng.queue_results()
        assert ei.value.code == L.ESTATE
        eng.run_centre()
        assert [r.state for r in eng.read_roots()] == [L.SLOT_MOVE_DONE] * 4
    with Engine(4, **kw) as eng:                        # a plain engine
        with pytest.raises(L.EngineError) as ei:
            eng.queue_positions([0], [0])
        assert ei.value.code == L.ESTATE
        with pytest.raises(L.EngineError) as ei:
            eng.queue_progress()
        assert ei.value.code == L.ESTATE
    with pytest.raises(L.EngineError) as ei:
        Engine(4, 16, eval_mode=L.EVAL_EXTERNAL_F32, n_match_nets=2, position_queue=True, stop_after_move=True)
    assert ei.value.code == L.EINVAL
    with pytest.raises(L.EngineError) as ei:
        Engine(4, 16, eval_mode=L.EVAL_EXTERNAL_F32, n_match_nets=2, position_queue=True, stop_after_move=False, games_target=4)
    assert ei.value.code == L.EINVAL
    with pytest.raises(L.EngineError) as ei:            # one search per position
        Engine(4, 16, eval_mode=L.EVAL_CENTRE, position_queue=True, stop_after_move=False)
    assert ei.value.code == L.EINVAL


def test_match_steps_refuses_a_queue_engine():
    import torch

    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    net = evaluator("f32x3").net
    with Engine(16, SIMS, eval_mode=L.EVAL_EXTERNAL_F32, stop_after_move=True, position_queue=True) as eng:
        eng.queue_positions([0] * 3, [0] * 3)
        values = torch.zeros(16, dtype=torch.float32, device="cuda")
        priors = torch.zeros((16, 7), dtype=torch.float32, device="cuda")
        with pytest.raises(L.EngineError) as ei:
            eng.match_steps(net, 0, values, priors, 4)
        assert ei.value.code == L.ESTATE


def test_rows_are_untouched_or_whole_between_launches(oracle):
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    boards = random_undecided_positions(oracle, 40, seed=41, max_plies=20)
    with Engine(4, eval_mode=L.EVAL_CENTRE, stop_after_move=True, position_queue=True, max_inner_iters=5, **centre_cfg(16)) as eng:
        eng.queue_positions([b.key()[0] for b in boards], [b.key()[1] for b in boards])
        seen, last = set(), 0
        for _ in range(4000):
            eng.step()
            states = eng.queue_results().state
            assert set(states.tolist()) <= {0, 2}
            done, total = eng.queue_progress()
            assert total == 40 and done == int((states == 2).sum()) >= last
            last = done
            seen.add(done)
            if eng.stats()["active_slots"] == 0:
                break
        assert last == 40 and len(seen) > 5 and min(seen) < 4      # rows were read while slots still searched


# ---------------------------------------------------------------- score_search
def test_score_search_feeds_the_exported_tensors_to_the_statistics():
    import torch

    from connect4_amd.analysis import run_queue
    from connect4_amd.mcts import MCTSConfig
    from connect4_amd.stats import CombinedStats, LabelledSet, ValueStats, score_search
    from test_gpu_stats import close_on_grid, float64_sums, host_stats
    rng = np.random.RandomState(43)
    boards = positions_50() + positions_50()[:10]
    n = len(boards)
    packed = torch.from_numpy(np.array([[b.color[0], b.color[1]] for b in boards], dtype=np.uint64).view(np.int64)).cuda()
    yv = rng.choice([0.0, 0.5, 1.0], size=n).astype(np.float32)
    yp = rng.random_sample((n, 7)).astype(np.float32)
    yp /= yp.sum(axis=1, keepdims=True)
    cfg, net = MCTSConfig(SIMS), evaluator("f32x3").net
    eng = run_queue(cfg, packed, evaluator("f32x3"), n_slots=18)
    try:
        out = {k: v.cpu().numpy() for k, v in eng.queue_export(("policy", "root_values")).items()}
    finally:
        eng.close()
    xv, xp = out["root_values"], out["policy"]
    assert ((xv > 0) & (xv < 1)).all() and np.allclose(xp.sum(axis=1), 1.0, atol=1e-6)

    st = score_search(cfg, net, LabelledSet(packed, torch.from_numpy(yv).cuda(), torch.from_numpy(yp).cuda()), n_slots=18)
    assert isinstance(st, CombinedStats)
    hv, hp = host_stats(xv, yv, xp, yp)
    v, p = st.value_stats, st.prior_stats
    assert (v.n, v.total, v.correct, v.smallest, v.largest) == (hv.n, hv.total, hv.correct, hv.smallest, hv.largest)
    assert (p.n, p.correct) == (hp.n, hp.correct) == (n, hp.correct) and v.non_finite == 0
    sums = float64_sums(xv, yv, xp, yp)
    assert close_on_grid(v.average_value, sums[0], n, 36) and close_on_grid(v.total_loss, sums[1], n, 36), (v.average_value, v.total_loss, sums)
    assert close_on_grid(p.total_loss * 7.0, sums[2], n, 32), (p.total_loss * 7.0, sums[2])

    st = score_search(cfg, net, LabelledSet(packed, torch.from_numpy(yv).cuda()), n_slots=60)      # a value-only set
    assert isinstance(st, ValueStats)
    assert (st.n, st.total, st.correct, st.smallest, st.largest) == (hv.n, hv.total, hv.correct, hv.smallest, hv.largest)
    assert close_on_grid(st.average_value, sums[0], n, 36) and close_on_grid(st.total_loss, sums[1], n, 36)
