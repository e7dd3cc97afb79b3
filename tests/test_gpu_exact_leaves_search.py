"""Searches with an ExactLeafNet against the host-callable path, field for field.

19 positions (three 8-slot blocks, the last ragged) with 12 to 16 empty squares, 150 simulations, no noise, max_empties = 10:
``MCTS(..., DeviceNetEvaluator(ExactLeafNet(FusedNet, 10)))`` drives c4_step / forward / overlay on the device; the other side
is the same engine fed leaf by leaf from the host (``_Searcher.kind == "host"``) by a callable whose value is ``overlay_host``
of ``net.evaluate_bits`` -- the host mirror of the solver, not the kernel -- and whose prior is the net's float32.  Every
comparison is ``==``; ``search_positions`` (the position queue, 8 slots for the 19 positions) gives the same rows.  The plain
net's roots differ on some position, so the overlay did reach the searches."""
import numpy as np
import pytest

from gpu_helpers import random_undecided_positions

pytestmark = pytest.mark.gpu

N, SIMS, MAX_EMPTIES = 19, 150, 10
FIELDS = ("root_visits", "child_visits", "child_value_sum", "child_status", "move", "expansions")


def _fields(r):
    bits = lambda x: np.asarray(x, dtype=np.float64).view(np.uint64).tolist()  # noqa: E731
    return dict(root_visits=r.root_visits, child_visits=list(r.child_visits), child_value_sum=bits(list(r.child_value_sum)),
                child_status=list(r.child_status), move=r.move, expansions=r.expansions)


def test_device_overlay_searches_equal_the_host_callables(oracle):
    from connect4_amd.analysis import search_positions
    from connect4_amd.board import Board
    from connect4_amd.config import MCTSConfig
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.exact_leaves import ExactLeafNet, overlay_host
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.mcts import _Searcher
    from connect4_amd.net import random_init_state_dict
    pool = [b for b in random_undecided_positions(oracle, 600, seed=31) if 12 <= 42 - (bin(b.key()[0]).count("1") + bin(b.key()[1]).count("1")) <= 16]
    assert len(pool) >= N
    boards = [Board.from_bits(*b.key()) for b in pool[:N]]
    cfg = MCTSConfig(SIMS)
    assert not cfg.root_exploration_fraction or not cfg.root_dirichlet_alpha
    net = FusedNet(random_init_state_dict(seed=0))
    exact = ExactLeafNet(net, MAX_EMPTIES, node_budget=1 << 20)
    memo, laid = {}, [0]

    def host_evaluator(board):
        key = (int(board.color[0]), int(board.color[1]))
        if key not in memo:
            v, p = net.evaluate_bits([key[0]], [key[1]])
            v, over = overlay_host([key[0]], [key[1]], v, MAX_EMPTIES)
            laid[0] += int(over[0])
            assert p.dtype == np.float32
            memo[key] = (v[0], p[0])
        return memo[key]

    searchers = [_Searcher(cfg, DeviceNetEvaluator(exact)), _Searcher(cfg, host_evaluator), _Searcher(cfg, DeviceNetEvaluator(net))]
    try:
        assert [s.kind for s in searchers] == ["device", "host", "device"]
        dev, host, plain = ([_fields(r) for r in s.run(boards)] for s in searchers)
        # the position queue takes the step path for a net without a c4_net handle, and refuses the fused kernels for it
        rows = search_positions(cfg, boards, DeviceNetEvaluator(exact), n_slots=8)
        queued = [_fields(rows[i]) for i in range(N)]
        with pytest.raises(ValueError):
            search_positions(cfg, boards, DeviceNetEvaluator(exact), n_slots=8, fused=True)
    finally:
        for s in searchers:
            s.close()
        counters = exact.counters()
        net.close()
    for i in range(N):
        for f in FIELDS:
            assert dev[i][f] == host[i][f], "position %d: %s differs: %r != %r" % (i, f, dev[i][f], host[i][f])
        assert dev[i]["root_visits"] == SIMS + 1
        assert {k: (int(v) if np.isscalar(v) else [int(x) for x in v]) for k, v in queued[i].items()} == dev[i], "position %d: the queue's row differs" % i
    differ = sum(dev[i] != plain[i] for i in range(N))
    print("%d of %d roots differ from the plain net's; the host laid over %d distinct positions; device counters %r" % (differ, N, laid[0], counters))
    assert differ >= 1 and laid[0] >= 1
    assert counters["over_budget"] == 0 and counters["overridden"] == counters["late"] >= laid[0]


def test_constructor_errors():
    from connect4_amd.exact_leaves import ExactLeafNet
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import random_init_state_dict
    net = FusedNet(random_init_state_dict(seed=0))
    try:
        with pytest.raises(TypeError):
            ExactLeafNet(net)                       # max_empties is required
        for bad in (-1, 25, 2.5, None):
            with pytest.raises(ValueError):
                ExactLeafNet(net, bad)
        for bad in (0, -1, None, 1.5):
            with pytest.raises(ValueError):
                ExactLeafNet(net, 8, node_budget=bad)
        with pytest.raises(ValueError):
            ExactLeafNet(lambda planes: None, 8)    # not a from_bitboards net
        e = ExactLeafNet(net, 8)
        assert e.from_bitboards and not isinstance(e, FusedNet) and e.counters() == dict(overridden=0, over_budget=0, nodes=0, late=0)
    finally:
        net.close()
