"""Search given positions -- a test set, a generation's positions, one board -- through the engine's position queue.

``search_positions(config, boards, evaluator)`` is a loop of the reference's ``mcts.search(config, board, evaluator)``
(mcts.py:94-121) over any number of positions, run by ``n_slots`` engine slots: the positions are queued on the device
(c4_queue_positions), a slot that finishes one leaves its root read-out in a device table and takes the next inside the
kernel, and the evaluation cache is shared by all of them.  With a fused net the whole list is searched by the launches
self-play uses (c4_selfplay_steps); the host does nothing between queueing and reading.  The rows are those of one
``MCTS.make_moves`` search per position; ``MCTS.make_moves`` / ``search`` themselves keep their one-slot-per-board path.
"""
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from .board import Board
from .config import MCTSConfig
from .engine import Engine, check_packed_boards
from .evaluators import DeviceNetEvaluator, evaluate_centre_with_prior, unwrap
from .fused_net import has_net_handle
from .tree import Tree

__all__ = ["search_positions", "run_queue", "trees", "pack_boards"]

DEFAULT_SLOTS = 4096


def pack_boards(boards):
    """The argument checks of search_positions, before anything touches the GPU: a non-empty sequence of undecided
    Boards -> (color0, color1) uint64 arrays and their ages; a torch int64 [n, 2] tensor of packed boards -> the tensor
    itself.  ValueError otherwise."""
    try:
        import torch
        is_tensor = isinstance(boards, torch.Tensor)
    except ImportError:     # (host-only use of the argument checks)
        is_tensor = False
    if is_tensor:
        check_packed_boards(boards)
        return boards
    if isinstance(boards, Board):
        boards = [boards]
    if isinstance(boards, np.ndarray) or not isinstance(boards, Sequence):
        raise ValueError("positions are a sequence of Boards or a torch int64 tensor [n, 2] of packed boards; got %s" % type(boards).__name__)
    if len(boards) == 0:
        raise ValueError("no positions to search: the list is empty")
    for i, b in enumerate(boards):
        if not isinstance(b, Board):
            raise ValueError("position %d is a %s, not a Board" % (i, type(b).__name__))
        if b.result is not None:
            raise ValueError("position %d is finished: cannot search a finished position" % i)
    c0 = np.array([b.color[0] for b in boards], dtype=np.uint64)
    c1 = np.array([b.color[1] for b in boards], dtype=np.uint64)
    return c0, c1, np.array([b.age for b in boards], dtype=np.int64)


def _draw_tapes(config, ages):
    """_Searcher._tapes for queued positions: row i is position i's, ply 0; drawn from np.random position by position in
    the reference's order (mcts.py:175-177, tree.py:80)."""
    n = len(ages)
    nz = np.zeros((n, 42, 7))
    u = np.full((n, 42), -1.0)
    noisy = bool(config.root_dirichlet_alpha and config.root_exploration_fraction)
    for i in range(n):
        if noisy:
            nz[i, 0] = np.random.gamma(config.root_dirichlet_alpha, 1, 7)
        if ages[i] < config.num_sampling_moves:
            u[i, 0] = np.random.random_sample()
    return nz, u


def _kind(evaluator):
    fn = unwrap(evaluator)
    if fn is evaluate_centre_with_prior:
        return "centre", None
    for e in (fn, evaluator):
        if isinstance(e, DeviceNetEvaluator):
            return "device", e
    if getattr(evaluator, "from_bitboards", False):      # a bare FusedNet
        return "device", DeviceNetEvaluator(evaluator, getattr(evaluator, "device", 0))
    return "host", None


def run_queue(config: MCTSConfig, boards, evaluator, n_slots: Optional[int] = None, device: int = 0,
              eval_cache_log2_entries: int = 0, steps_per_launch: int = 64, fused: Optional[bool] = None, on_launch=None):
    """Queue the positions and search them all; returns the Engine (every row finished, the caller closes it) for
    queue_results / queue_export.  The arguments are search_positions' and:
    fused: None = the fused kernels whenever the evaluator is a DeviceNetEvaluator over a FusedNet; False = the host-driven
    c4_step + forward loop on the same queue engine (same rows: which launch runs a simulation never changes a result).
    on_launch: called with the Engine after every c4_selfplay_steps launch (e.g. to ask it for last_fused_kernel()).
    Root noise and sampled moves are drawn from np.random with the reference's calls, position by position, as
    MCTS.make_moves draws them, and reach the kernel as tapes indexed by position."""
    packed = pack_boards(boards)
    kind, dev_eval = _kind(evaluator)
    if kind == "device":
        device = getattr(dev_eval, "device", device)
    is_tensor = not isinstance(packed, tuple)
    n = int(packed.shape[0]) if is_tensor else len(packed[0])
    G = int(n_slots) if n_slots else min(n, DEFAULT_SLOTS)
    if G <= 0:
        raise ValueError("n_slots must be positive")
    G = min(G, n)
    random = bool(config.root_dirichlet_alpha and config.root_exploration_fraction) or config.num_sampling_moves > 0
    tapes = None
    if random:
        if is_tensor:
            b = packed.detach().cpu().numpy().view(np.uint64)
            ages = np.array([bin(int(x)).count("1") + bin(int(y)).count("1") for x, y in b], dtype=np.int64)
        else:
            ages = packed[2]
        tapes = _draw_tapes(config, ages)

    handle = kind == "device" and has_net_handle(dev_eval.net)      # the fused kernels take a c4_net handle (an ExactLeafNet has none)
    use_fused = handle if fused is None else bool(fused)
    if use_fused and not handle:
        raise ValueError("the fused kernels need a DeviceNetEvaluator over a FusedNet")
    f32 = True
    if kind == "centre":
        mode = L.EVAL_CENTRE
    elif kind == "device":
        mode = L.EVAL_EXTERNAL_F32
    else:       # the prior's dtype decides the score arithmetic (float32 net output vs float64), as in MCTS
        c0, c1 = (int(packed[0, 0]), int(packed[0, 1])) if is_tensor else (int(packed[0][0]), int(packed[1][0]))
        first = Board.from_bits(c0 & (2 ** 64 - 1), c1 & (2 ** 64 - 1))
        f32 = np.asarray(evaluator(first)[1]).dtype == np.float32
        mode = L.EVAL_EXTERNAL_F32 if f32 else L.EVAL_EXTERNAL_F64
    kw = dict(max_inner_iters=32, time_budget_cycles=80000) if use_fused else {}
    eng = Engine(G, eval_mode=mode, rng_mode=L.RNG_TAPE, stop_after_move=True, position_queue=True, device=device,
                 eval_cache_log2_entries=eval_cache_log2_entries, **kw, **config.engine_kwargs())
    try:
        if tapes is not None:
            eng.set_tapes(*tapes)
        if is_tensor:
            import torch
            eng.queue_positions_dev(packed.to(torch.device("cuda", device)))
        else:
            eng.queue_positions(packed[0], packed[1])
        if kind == "centre":
            while True:
                eng.run_centre(max_launches=1 << 20)
                if eng.stats()["active_slots"] == 0:
                    break
        elif use_fused:
            _drive_fused(eng, dev_eval.net, max(1, int(steps_per_launch)), on_launch=on_launch)
        else:
            from .mcts import _Searcher
            s = _Searcher(config, evaluator, device)      # its step loops, on this engine
            if kind == "device":
                s._drive_device(eng)
            else:
                s._drive_host(eng, np.float32 if f32 else np.float64)
        done, total = eng.queue_progress()
        if done != total:
            raise RuntimeError("the queue stopped with %d of %d positions searched" % (done, total))
    except BaseException:
        eng.close()
        raise
    return eng


def _drive_fused(eng, net, steps_per_launch, launches_per_poll=4, on_launch=None):
    """c4_selfplay_steps until every slot has parked: the launches self-play uses; the host only polls."""
    import ctypes as C

    import torch
    dev = torch.device("cuda", eng.device)
    with torch.cuda.device(dev):
        values = torch.zeros(eng.n_slots, dtype=torch.float32, device=dev)
        priors = torch.full((eng.n_slots, 7), 1.0 / 7.0, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        eng.set_stream(stream)
        while True:
            for _ in range(launches_per_poll):
                L.check(eng._lib.c4_selfplay_steps(eng._h, net._h, C.c_void_p(values.data_ptr()), C.c_void_p(priors.data_ptr()),
                                                   steps_per_launch, C.c_void_p(stream)), eng._h)
                if on_launch is not None:
                    on_launch(eng)
            if eng.stats()["active_slots"] == 0:
                return


def search_positions(config: MCTSConfig, boards, evaluator, n_slots: Optional[int] = None, device: int = 0,
                     eval_cache_log2_entries: int = 0, steps_per_launch: int = 64, **kw):
    """One search per position, any number of positions on n_slots engine slots (default min(N, 4096)).
    boards     a sequence of undecided Boards, or a torch int64 [n, 2] tensor of packed boards (PackedGames.boards,
               LabelledSet.boards; queued from the device when it lives there);
    evaluator  what MCTS takes: evaluate_centre_with_prior (in-kernel, c4_run_centre), a DeviceNetEvaluator -- over a
               FusedNet the fused kernels (c4_selfplay_steps, steps_per_launch steps per launch), over any other device
               net the c4_step loop -- or any host callable (c4_step loop);
    eval_cache_log2_entries  0: the engine's automatic size (on for a net), < 0 off.
    Returns the rows, a NumPy record array of c4_search_result in the order of `boards`: rows[i].move, .value,
    .child_visits, .values_policy ...; rows.move is the column of all of them.  **kw: run_queue's `fused`."""
    eng = run_queue(config, boards, evaluator, n_slots, device, eval_cache_log2_entries, steps_per_launch, **kw)
    try:
        return eng.queue_results()
    finally:
        eng.close()


def trees(rows, boards=None):
    """The reference's Tree (root and children) of every row: a row reads like the root read-out Tree is built from.
    boards: the Boards searched (default: rebuilt from the rows' own bitboards)."""
    out = []
    for i in range(len(rows)):
        r = rows[i]
        b = boards[i] if boards is not None else Board.from_bits(int(r.color0), int(r.color1))
        out.append(Tree(r, b))
    return out
