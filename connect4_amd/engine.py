"""Thin object wrapper over the C ABI (connect4_amd/_lib.py -> libc4engine.so).

Host plumbing only: numpy for host arrays, torch tensors only as device buffers whose
`data_ptr()` is handed across the ABI.  All search work happens in the HIP kernels.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def check_packed_boards(boards):
    """ValueError unless `boards` is a non-empty torch int64 [n, 2] tensor of packed boards {color0, color1}."""
    import torch
    if not isinstance(boards, torch.Tensor) or boards.dtype != torch.int64 or boards.dim() != 2 or boards.shape[1] != 2:
        raise ValueError("packed boards are a torch int64 tensor [n, 2] = {color0, color1} per row; got %s %s" % (
            getattr(boards, "dtype", type(boards).__name__), tuple(getattr(boards, "shape", ()))))
    if boards.shape[0] == 0:
        raise ValueError("no positions to search: the tensor is empty")


class Engine:
    """One engine per GPU per process; not thread safe (one host thread drives it)."""

    def __init__(self, n_slots, simulations, pb_c_base=19652, pb_c_init=1.25,
                 root_dirichlet_alpha=0.0, root_exploration_fraction=0.0, num_sampling_moves=0,
                 eval_mode=L.EVAL_EXTERNAL_F32, rng_mode=L.RNG_PHILOX, seed=0, stop_after_move=False,
                 games_target=-1, record_capacity_games=0, max_inner_iters=0,
                 planes_dtype=L.PLANES_F32, eval_cache_log2_entries=0, level_budget=0, time_budget_cycles=0, device=0,
                 n_match_nets=0, position_queue=False):
        self._lib = L.load()
        self.cfg = L.Config()
        self.cfg.abi_version = L.ABI_VERSION
        self.cfg.n_slots = int(n_slots)
        self.cfg.simulations = int(simulations)
        self.cfg.pb_c_base = int(pb_c_base)
        self.cfg.pb_c_init = float(pb_c_init)
        self.cfg.root_dirichlet_alpha = float(root_dirichlet_alpha)
        self.cfg.root_exploration_fraction = float(root_exploration_fraction)
        self.cfg.num_sampling_moves = int(num_sampling_moves)
        self.cfg.eval_mode = int(eval_mode)
        self.cfg.rng_mode = int(rng_mode)
        self.cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.cfg.stop_after_move = 1 if stop_after_move else 0
        self.cfg.games_target = int(games_target)
        self.cfg.record_capacity_games = int(record_capacity_games)
        self.cfg.max_inner_iters = int(max_inner_iters)
        self.cfg.planes_dtype = int(planes_dtype)
        self.cfg.eval_cache_log2_entries = int(eval_cache_log2_entries)
        self.cfg.level_budget = int(level_budget)
        self.cfg.time_budget_cycles = int(time_budget_cycles)
        self.cfg.reserved[0] = int(n_match_nets)     # > 0: a match engine, one evaluation cache per net (match_steps)
        self.n_match_nets = int(n_match_nets)
        self.cfg.reserved[1] = 1 if position_queue else 0   # a position-queue engine (queue_positions); stop_after_move
        self.position_queue = bool(position_queue)
        self.n_slots = int(n_slots)
        self.device = int(device)
        self._h = C.c_void_p()
        L.check(self._lib.c4_engine_create(C.byref(self.cfg), self.device, C.byref(self._h)))

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.c4_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        L.check(rc, self._h)

    def clear_eval_cache(self):
        self._check(self._lib.c4_clear_eval_cache(self._h))

    def set_stream(self, stream_handle):
        self._check(self._lib.c4_set_stream(self._h, C.c_void_p(int(stream_handle))))

    def reset(self, color0=None, color1=None, n_active=None):
        if color0 is None:
            n = self.n_slots if n_active is None else int(n_active)
            self._check(self._lib.c4_reset(self._h, None, None, n))
            return
        c0, c1 = _u64(color0), _u64(color1)
        n = len(c0) if n_active is None else int(n_active)
        assert len(c0) == len(c1) >= n
        self._check(self._lib.c4_reset(self._h, _ptr(c0, C.c_uint64), _ptr(c1, C.c_uint64), n))

    def set_tapes(self, gamma_noise, uniforms):
        """gamma_noise [games][42][7] raw Gamma(alpha,1) draws, uniforms [games][42] (u<0: best_move)."""
        nz = np.ascontiguousarray(gamma_noise, dtype=np.float64)
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        n = nz.shape[0]
        assert nz.shape == (n, 42, 7) and u.shape == (n, 42)
        self._check(self._lib.c4_set_tapes(self._h, _ptr(nz, C.c_double), _ptr(u, C.c_double), n))

    # -- hot path ----------------------------------------------------------------------------
    def step_ptrs(self, values_ptr, priors_ptr, planes_ptr):
        self._check(self._lib.c4_step(self._h, C.c_void_p(values_ptr or 0), C.c_void_p(priors_ptr or 0),
                                      C.c_void_p(planes_ptr or 0)))

    def step(self, values=None, priors=None, planes=None):
        """values/priors/planes are torch device tensors (or None)."""
        self.step_ptrs(0 if values is None else values.data_ptr(),
                       0 if priors is None else priors.data_ptr(),
                       0 if planes is None else planes.data_ptr())

    def step_range(self, values, priors, planes, slot_lo, slot_count, stream=0):
        self._check(self._lib.c4_step_range(
            self._h, C.c_void_p(0 if values is None else values.data_ptr()),
            C.c_void_p(0 if priors is None else priors.data_ptr()),
            C.c_void_p(0 if planes is None else planes.data_ptr()), int(slot_lo), int(slot_count), C.c_void_p(stream or 0)))

    def match_assign(self, net_o, net_x):
        """Per slot, the index of the net that moves o and of the net that moves x (c4_match_assign); slots beyond
        len(net_o) have no game.  Call after reset() with the openings."""
        o = np.ascontiguousarray(net_o, dtype=np.int32)
        x = np.ascontiguousarray(net_x, dtype=np.int32)
        assert o.shape == x.shape and o.ndim == 1
        self._check(self._lib.c4_match_assign(self._h, _ptr(o, C.c_int32), _ptr(x, C.c_int32), len(o)))

    def match_steps(self, net, net_index, values, priors, n_steps, stream=0):
        """One launch of the match kernel for net `net_index` (a FusedNet): the slots where that net is to move search,
        choose and make their move; all others pass through (c4_match_steps).  Asynchronous on `stream`."""
        self._check(self._lib.c4_match_steps(self._h, net._h, int(net_index), C.c_void_p(values.data_ptr()),
                                             C.c_void_p(priors.data_ptr()), int(n_steps), C.c_void_p(stream or 0)))

    def match_configure(self, net_index, simulations=None, pb_c_base=None, pb_c_init=None, kernel="wave"):
        """The player behind net `net_index` of a match engine (c4_match_configure): its simulations per move (at most the
        engine's), pb_c_base, pb_c_init -- None: the engine's -- and its match kernel, "wave" (c4_match_wave_kernel) or
        "split" (c4_match_split_kernel, which also holds the 64-filter "f32x3w" net).  After reset(), before match_assign()."""
        kernels = {"wave": L.MATCH_KERNEL_WAVE, "split": L.MATCH_KERNEL_SPLIT}
        if kernel not in kernels:
            raise ValueError("kernel must be 'wave' or 'split', not %r" % (kernel,))
        p = L.MatchPlayer()
        p.simulations = 0 if simulations is None else int(simulations)
        p.pb_c_base = 0 if pb_c_base is None else int(pb_c_base)
        p.pb_c_init = float(self.cfg.pb_c_init if pb_c_init is None else pb_c_init)
        p.kernel = kernels[kernel]
        if (simulations is not None and p.simulations == 0) or (pb_c_base is not None and p.pb_c_base == 0):
            raise ValueError("simulations and pb_c_base must be positive (None: the engine's)")
        self._check(self._lib.c4_match_configure(self._h, int(net_index), C.byref(p)))

    def last_fused_kernel(self):
        """The fused kernel the last selfplay_steps / match_steps call launched, e.g.
        "c4_selfplay_split_kernel<16,1,3,false> spread=0 grid=3" (c4_debug_last_fused_kernel); "" before the first one.
        Host bookkeeping: nothing is launched or waited for."""
        buf = C.create_string_buffer(128)
        rc = self._lib.c4_debug_last_fused_kernel(self._h, buf, len(buf))
        if rc < 0:
            self._check(rc)
        return buf.value.decode("ascii")

    # -- position queue (c4_queue_positions ...; Engine(..., stop_after_move=True, position_queue=True)) ------
    def queue_positions(self, color0, color1):
        """Queue len(color0) positions of any number for the engine's slots: slot i starts on position i, and a slot
        that finishes one takes the next inside the kernel.  Resets counters and the result table like reset()."""
        c0, c1 = _u64(color0), _u64(color1)
        if c0.ndim != 1 or c0.shape != c1.shape or len(c0) == 0:
            raise ValueError("queue_positions takes two equally long, non-empty lists of bitboards")
        self._check(self._lib.c4_queue_positions(self._h, _ptr(c0, C.c_uint64), _ptr(c1, C.c_uint64), len(c0)))

    def queue_positions_dev(self, boards):
        """The same from a torch int64 [n, 2] device tensor of packed boards (PackedGames.boards, LabelledSet.boards):
        no host copy; the engine keeps a copy of its own."""
        check_packed_boards(boards)
        if boards.device.type != "cuda" or (boards.device.index or 0) != self.device:
            raise ValueError("queue_positions_dev takes a tensor on cuda:%d, got %s" % (self.device, boards.device))
        boards = boards.contiguous()
        self._check(self._lib.c4_queue_positions_dev(self._h, C.c_void_p(boards.data_ptr()), int(boards.shape[0])))

    def queue_progress(self):
        """(rows finished, rows in all); waits for the device."""
        done, total = C.c_int64(), C.c_int64()
        self._check(self._lib.c4_queue_progress(self._h, C.byref(done), C.byref(total)))
        return done.value, total.value

    def queue_results(self, first=0, n=None):
        """Rows [first, first + n) of the result table (default: all) as a NumPy record array of c4_search_result:
        rows[i].child_visits, rows.move, ...; a row reads like the RootResult of read_roots().  state 0: not searched yet."""
        if n is None:
            n = self.queue_progress()[1] - int(first)
        out = np.zeros(max(int(n), 0), dtype=L.search_result_dtype())
        self._check(self._lib.c4_queue_results(self._h, C.c_void_p(out.ctypes.data), int(first), int(n)))
        return out.view(np.recarray)

    def queue_export(self, fields=("policy", "visit_policy", "root_values", "move_values", "moves"), stream=0):
        """The rows as packed device tensors in the replay window's layout (c4_queue_export_dev): a dict with the asked
        ones of policy F32[n,7] (values policy), visit_policy F32[n,7], root_values F32[n] (root value sum / visits),
        move_values F32[n] (NaN for None) and moves U8[n].  One launch on `stream` (default: torch's current stream),
        no host synchronisation beyond the row count."""
        import torch
        n = self.queue_progress()[1]
        dev = torch.device("cuda", self.device)
        shapes = dict(policy=((n, 7), torch.float32), visit_policy=((n, 7), torch.float32), root_values=((n,), torch.float32),
                      move_values=((n,), torch.float32), moves=((n,), torch.uint8))
        for f in fields:
            if f not in shapes:
                raise ValueError("queue_export fields are %s" % ", ".join(shapes))
        t = {f: torch.empty(shapes[f][0], dtype=shapes[f][1], device=dev) for f in fields}
        if not stream:
            stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._lib.c4_queue_export_dev(self._h, C.c_void_p(stream), *[
            C.c_void_p(t[f].data_ptr()) if f in t else None for f in ("policy", "visit_policy", "root_values", "move_values", "moves")]))
        return t

    def run_centre(self, max_launches=64):
        self._check(self._lib.c4_run_centre(self._h, int(max_launches)))

    def leaf_buffers(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._lib.c4_leaf_buffers(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def read_leaves(self):
        c0 = np.zeros(self.n_slots, dtype=np.uint64)
        c1 = np.zeros(self.n_slots, dtype=np.uint64)
        has = np.zeros(self.n_slots, dtype=np.int32)
        self._check(self._lib.c4_read_leaves(self._h, _ptr(c0, C.c_uint64), _ptr(c1, C.c_uint64),
                                             _ptr(has, C.c_int32)))
        return c0, c1, has

    # -- read-out ----------------------------------------------------------------------------
    def stats(self):
        s = L.Stats()
        self._check(self._lib.c4_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def read_roots(self):
        out = (L.RootResult * self.n_slots)()
        self._check(self._lib.c4_read_roots(self._h, out))
        return out

    # -- whole trees -------------------------------------------------------------------------
    def _slots(self, slots):
        if slots is None:
            return None, self.n_slots
        a = np.ascontiguousarray(slots, dtype=np.int32)
        return a, len(a)

    def tree_sizes(self, slots=None, min_visits=0, max_depth=None):
        """Rows of each slot's tree table under the two filters (int64 [n])."""
        a, n = self._slots(slots)
        out = np.zeros(n, dtype=np.int64)
        self._check(self._lib.c4_tree_sizes(self._h, None if a is None else _ptr(a, C.c_int32), n, int(min_visits),
                                            -1 if max_depth is None else int(max_depth), _ptr(out, C.c_int64)))
        return out

    def export_trees(self, slots=None, min_visits=0, max_depth=None, capacity=None):
        """The whole search trees of `slots` (default: every slot), walked and filtered on the device: one TreeTable
        (connect4_amd.tree) per slot, all of them views into ONE structured NumPy buffer of c4_tree_node rows.
        min_visits drops nodes with fewer visits (0 keeps the unvisited children), max_depth nodes further below the
        root; a dropped node drops its subtree.  A slot without a tree gives an empty table.  `capacity` (rows of
        the buffer) defaults to what c4_tree_sizes reports."""
        from .tree import TreeTable
        a, n = self._slots(slots)
        if capacity is None:
            capacity = int(self.tree_sizes(slots, min_visits, max_depth).sum())
        nodes = np.zeros(int(capacity), dtype=L.tree_node_dtype())
        off = np.zeros(n + 1, dtype=np.int64)
        self._check(self._lib.c4_export_trees(self._h, None if a is None else _ptr(a, C.c_int32), n, int(min_visits),
                                              -1 if max_depth is None else int(max_depth), C.c_void_p(nodes.ctypes.data),
                                              int(capacity), _ptr(off, C.c_int64)))
        ids = range(n) if a is None else a.tolist()
        return [TreeTable(nodes[off[i]:off[i + 1]], int(g)) for i, g in enumerate(ids)]

    def principal_variations(self, slots=None, rule="value", max_len=42):
        """The line each slot's search expects, walked on the device: per slot (moves int32[k], visits uint32[k],
        values float64[k]; NaN where the reference's absolute_value is None).  rule "value": Tree.best_move for the
        side to move at every node; "visits": Tree.most_visited."""
        if rule not in ("value", "visits"):
            raise ValueError("rule is 'value' or 'visits'")
        a, n = self._slots(slots)
        max_len = int(max_len)
        moves = np.zeros((n, max(max_len, 1)), dtype=np.int32)
        visits = np.zeros((n, max(max_len, 1)), dtype=np.uint32)
        values = np.zeros((n, max(max_len, 1)), dtype=np.float64)
        lens = np.zeros(n, dtype=np.int32)
        self._check(self._lib.c4_principal_variations(
            self._h, None if a is None else _ptr(a, C.c_int32), n, L.PV_VALUE if rule == "value" else L.PV_VISITS, max_len,
            _ptr(moves, C.c_int32), _ptr(lens, C.c_int32), _ptr(visits, C.c_uint32), _ptr(values, C.c_double)))
        return [(moves[i, :lens[i]], visits[i, :lens[i]], values[i, :lens[i]]) for i in range(n)]

    @property
    def record_capacity(self):
        return int(self.cfg.record_capacity_games or 2 * self.n_slots)

    def finished_games(self):
        """(finished games waiting in the device ring, finished games lost to a full ring)."""
        ready, dropped = C.c_int64(), C.c_int64()
        self._check(self._lib.c4_finished_games(self._h, C.byref(ready), C.byref(dropped)))
        return ready.value, dropped.value

    def drain_games(self, cap=None):
        """Host copy of the finished games (float64 values/policies, for parity tests and GameData)."""
        ready, _ = self.finished_games()
        cap = int(min(cap, ready) if cap is not None else ready)
        if cap <= 0:
            return []
        out = (L.GameRecord * cap)()
        n = C.c_int32()
        self._check(self._lib.c4_drain_games(self._h, out, cap, C.byref(n)))
        return [out[i] for i in range(n.value)]

    _EXPORT_FIELDS = ("boards", "moves", "values", "policy", "targets", "game_index", "lengths", "results", "ids")

    def export_buffers(self, max_games=None, cap_positions=None):
        """Device tensors an export writes into: (dict of tensors, counts int64[2] = {games, positions})."""
        import torch
        max_games = min(int(max_games if max_games is not None else self.record_capacity), self.record_capacity)
        cap_positions = int(cap_positions if cap_positions is not None else 42 * max_games)
        dev = torch.device("cuda", self.device)
        t = dict(boards=torch.empty((cap_positions, 2), dtype=torch.int64, device=dev),
                 moves=torch.empty(cap_positions, dtype=torch.uint8, device=dev),
                 values=torch.empty(cap_positions, dtype=torch.float32, device=dev),
                 policy=torch.empty((cap_positions, 7), dtype=torch.float32, device=dev),
                 targets=torch.empty(cap_positions, dtype=torch.float32, device=dev),
                 game_index=torch.empty(cap_positions, dtype=torch.int32, device=dev),
                 lengths=torch.empty(max_games, dtype=torch.int32, device=dev),
                 results=torch.empty(max_games, dtype=torch.int8, device=dev),
                 ids=torch.empty(max_games, dtype=torch.int64, device=dev))
        return t, torch.zeros(2, dtype=torch.int64, device=dev)

    def export_games_async(self, tensors, counts, stream=0):
        """Queue one device-side export (c4_export_games_dev) behind the launches on `stream`: consumes the
        finished games that fit `tensors`, writes {games, positions} to `counts`.  No host synchronisation."""
        import torch
        if not stream:
            stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        b = L.ExportBuffers(*[tensors[k].data_ptr() for k in self._EXPORT_FIELDS])
        self._check(self._lib.c4_export_games_dev(self._h, C.byref(b), int(tensors["lengths"].shape[0]),
                                                  int(tensors["moves"].shape[0]), C.c_void_p(counts.data_ptr()),
                                                  C.c_void_p(stream)))

    def export_games(self, max_games=None, cap_positions=None, stream=0):
        """Device-side export: consume up to max_games finished games into torch DEVICE tensors (compact
        record, ~50 B/position) with no per-game host work.  Returns PackedGames (connect4_amd.packed)."""
        from .packed import PackedGames
        t, counts = self.export_buffers(max_games, cap_positions)
        self.export_games_async(t, counts, stream)
        n_games, n_pos = [int(x) for x in counts.tolist()]     # the one synchronisation of the export
        per_pos = ("boards", "moves", "values", "policy", "targets", "game_index")
        return PackedGames(**{k: (v[:n_pos] if k in per_pos else v[:n_games]) for k, v in t.items()})

    def cache_lookup(self, color0, color1):
        """What the evaluation cache answers for the positions: (values f32[n], priors f32[n,7], found bool[n])."""
        c0, c1 = _u64(color0), _u64(color1)
        n = len(c0)
        v = np.zeros(n, dtype=np.float32)
        p = np.zeros((n, 7), dtype=np.float32)
        f = np.zeros(n, dtype=np.int32)
        self._check(self._lib.c4_eval_cache_lookup(self._h, _ptr(c0, C.c_uint64), _ptr(c1, C.c_uint64), n,
                                                   _ptr(v, C.c_float), _ptr(p, C.c_float), _ptr(f, C.c_int32)))
        return v, p, f.astype(bool)


# -- pure board functions executed by the device code ------------------------------------------
def board_make_move(color0, color1, cols, device=0):
    c0, c1 = _u64(color0), _u64(color1)
    col = np.ascontiguousarray(cols, dtype=np.int32)
    o0, o1 = np.zeros_like(c0), np.zeros_like(c1)
    res = np.zeros(len(c0), dtype=np.int32)
    lib = L.load()
    L.check(lib.c4_board_make_move(device, _ptr(c0, C.c_uint64), _ptr(c1, C.c_uint64), _ptr(col, C.c_int32),
                                   len(c0), _ptr(o0, C.c_uint64), _ptr(o1, C.c_uint64), _ptr(res, C.c_int32)))
    return o0, o1, res


def board_wins(stones, device=0):
    s = _u64(stones)
    out = np.zeros(len(s), dtype=np.int32)
    L.check(L.load().c4_board_wins(device, _ptr(s, C.c_uint64), len(s), _ptr(out, C.c_int32)))
    return out


def board_valid_mask(color0, color1, device=0):
    c0, c1 = _u64(color0), _u64(color1)
    out = np.zeros(len(c0), dtype=np.int32)
    L.check(L.load().c4_board_valid_mask(device, _ptr(c0, C.c_uint64), _ptr(c1, C.c_uint64), len(c0),
                                         _ptr(out, C.c_int32)))
    return out


def board_planes(color0, color1, device=0):
    c0, c1 = _u64(color0), _u64(color1)
    out = np.zeros((len(c0), 3, 6, 7), dtype=np.float32)
    L.check(L.load().c4_board_planes(device, _ptr(c0, C.c_uint64), _ptr(c1, C.c_uint64), len(c0),
                                     _ptr(out, C.c_float)))
    return out


def board_fliplr(color0, color1, device=0):
    c0, c1 = _u64(color0), _u64(color1)
    o0, o1 = np.zeros_like(c0), np.zeros_like(c1)
    L.check(L.load().c4_board_fliplr(device, _ptr(c0, C.c_uint64), _ptr(c1, C.c_uint64), len(c0),
                                     _ptr(o0, C.c_uint64), _ptr(o1, C.c_uint64)))
    return o0, o1


def training_tensors(boards, targets, policy, add_fliplr=True, stream=0):
    """native_to_pytorch (data.py:78-105) on device: torch device tensors in (int64 [n,2], f32 [n], f32 [n,7]),
    torch device tensors out (boards F32[m,3,6,7], values F32[m], priors F32[m,7]), m = 2n with the mirrored copies."""
    import torch
    n = int(boards.shape[0])
    dev = boards.device
    m = n * (2 if add_fliplr else 1)
    ob = torch.empty((m, 3, 6, 7), dtype=torch.float32, device=dev)
    ov = torch.empty(m, dtype=torch.float32, device=dev)
    op = torch.empty((m, 7), dtype=torch.float32, device=dev)
    if n:
        boards, targets, policy = boards.contiguous(), targets.contiguous(), policy.contiguous()
        if not stream:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.load().c4_training_tensors_dev(dev.index or 0, C.c_void_p(stream), C.c_void_p(boards.data_ptr()),
                                                 C.c_void_p(targets.data_ptr()), C.c_void_p(policy.data_ptr()), n,
                                                 1 if add_fliplr else 0, C.c_void_p(ob.data_ptr()), C.c_void_p(ov.data_ptr()),
                                                 C.c_void_p(op.data_ptr())))
    return ob, ov, op


def _check_window(rc):
    if rc != L.OK:
        msg = L.load().c4_window_last_error()
        raise L.EngineError(rc, msg.decode("utf-8", "replace") if msg else "")


def _need_gpu(dev, what):
    if dev.type != "cuda":
        raise RuntimeError("%s runs on the GPU; move the tensors to a cuda device first -- there is no CPU fallback" % what)


def window_gather(segments_ptr, n_segments, index, boards_out, values_out, priors_out, counter=None, stream=0):
    """c4_window_gather_dev: rows `index` (int64 device tensor) of the window whose segment table (c4_window_segment
    [n_segments], device memory) is at `segments_ptr`, into the three float32 device tensors.  `counter`: device int32
    tensor that receives the number of indices outside the window (their rows are zeros), or None.  One launch on
    `stream` (default: torch's current stream); nothing is allocated and nothing waited for."""
    import torch
    dev = index.device
    _need_gpu(dev, "window_gather (c4_window_gather_dev)")
    m = int(index.numel())
    assert index.dtype == torch.int64 and index.is_contiguous()
    for t, shape in ((boards_out, (m, 3, 6, 7)), (values_out, (m,)), (priors_out, (m, 7))):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape and t.device == dev, (tuple(t.shape), shape)
    if not stream:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _check_window(L.load().c4_window_gather_dev(dev.index or 0, C.c_void_p(stream), C.c_void_p(segments_ptr), int(n_segments),
                                                C.c_void_p(index.data_ptr()), m, C.c_void_p(boards_out.data_ptr()),
                                                C.c_void_p(values_out.data_ptr()), C.c_void_p(priors_out.data_ptr()),
                                                C.c_void_p(counter.data_ptr()) if counter is not None else None))


def planes_to_boards(planes, stream=0):
    """c4_planes_to_boards_dev, the inverse of board_planes on device tensors: F32[n,3,6,7] -> (int64 [n,2] bitboards,
    int32 [1] number of rows that no board encodes), both on the planes' device; no host synchronisation."""
    import torch
    assert planes.dtype == torch.float32 and tuple(planes.shape[1:]) == (3, 6, 7)
    planes = planes.contiguous()
    dev = planes.device
    _need_gpu(dev, "planes_to_boards (c4_planes_to_boards_dev)")
    n = int(planes.shape[0])
    boards = torch.empty((n, 2), dtype=torch.int64, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if not stream:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _check_window(L.load().c4_planes_to_boards_dev(dev.index or 0, C.c_void_p(stream), C.c_void_p(planes.data_ptr()), n,
                                                   C.c_void_p(boards.data_ptr()), C.c_void_p(n_bad.data_ptr())))
    return boards, n_bad


def window_merge(segments_ptr, n_segments, n_positions, device, mirror=True, log2_capacity=None, wave_combine=True, stream=0):
    """c4_window_merge_dev over the window whose segment table is at `segments_ptr`: (boards int64 [n,2], targets
    float32 [n], policy float32 [n,7], counts int32 [n], heads int32 [2] = (n_distinct, n_bad)), device tensors with
    room for every position; the first n_distinct rows are the merged window (include/c4_engine.h states the rule).
    log2_capacity=None: the next power of two at or above 2 n_positions.  wave_combine=False: the plain insert, one
    lane one set of atomics (the same results; the measured A/B is in profiles/window_merge.json).  The table and
    work buffers are allocated here; the launches go on `stream` (default: torch's current stream) and nothing is
    waited for."""
    import torch
    dev = torch.device(device)
    _need_gpu(dev, "window_merge (c4_window_merge_dev)")
    n = int(n_positions)
    if log2_capacity is None:
        log2_capacity = max(2 * n - 1, 0).bit_length()
    log2_capacity = int(log2_capacity)
    slots = (1 << log2_capacity) if 0 <= log2_capacity <= 30 and (1 << log2_capacity) >= n else 0      # (refused below: nothing to allocate)
    table = torch.empty(max(slots, 1) * L.WINDOW_MERGE_SLOT_BYTES, dtype=torch.uint8, device=dev)
    work = torch.empty(max(L.window_merge_work_bytes(n) // 4, 1), dtype=torch.int32, device=dev)
    out = (torch.empty((n, 2), dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
           torch.empty((n, 7), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    heads = torch.empty(2, dtype=torch.int32, device=dev)
    if not stream:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _check_window(L.load().c4_window_merge_dev(dev.index or 0, C.c_void_p(stream), C.c_void_p(segments_ptr), int(n_segments), n,
                                               1 if mirror else 0, 1 if wave_combine else 0, log2_capacity,
                                               C.c_void_p(table.data_ptr()), C.c_void_p(work.data_ptr()),
                                               *[C.c_void_p(t.data_ptr()) for t in out], C.c_void_p(heads.data_ptr()),
                                               C.c_void_p(heads.data_ptr() + 4)))
    return out + (heads,)


def debug_root_noise(seed, alpha, game_id, ply, legal_mask, device=0):
    gid = np.ascontiguousarray(game_id, dtype=np.int64)
    pl = np.ascontiguousarray(ply, dtype=np.int32)
    lm = np.ascontiguousarray(legal_mask, dtype=np.int32)
    n = len(gid)
    raw = np.zeros((n, 7))
    dr = np.zeros((n, 7))
    L.check(L.load().c4_debug_root_noise(device, int(seed) & 0xFFFFFFFFFFFFFFFF, float(alpha), _ptr(gid, C.c_int64), _ptr(pl, C.c_int32),
                                         _ptr(lm, C.c_int32), n, _ptr(raw, C.c_double), _ptr(dr, C.c_double)))
    return raw, dr


def debug_sample_move(seed, game_id, ply, child_values, n_children, uniforms=None, device=0):
    gid = np.ascontiguousarray(game_id, dtype=np.int64)
    pl = np.ascontiguousarray(ply, dtype=np.int32)
    cv = np.ascontiguousarray(child_values, dtype=np.float64)
    nc = np.ascontiguousarray(n_children, dtype=np.int32)
    n = len(gid)
    assert cv.shape == (n, 7)
    u_in = None if uniforms is None else np.ascontiguousarray(uniforms, dtype=np.float64)
    u = np.zeros(n)
    ch = np.zeros(n, dtype=np.int32)
    L.check(L.load().c4_debug_sample_move(device, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(gid, C.c_int64), _ptr(pl, C.c_int32),
                                          _ptr(cv, C.c_double), _ptr(nc, C.c_int32),
                                          None if u_in is None else _ptr(u_in, C.c_double), n, _ptr(u, C.c_double), _ptr(ch, C.c_int32)))
    return u, ch


def debug_div_mismatches(max_parent_visits=4096, max_child_visits=4096, n_random=1 << 26, device=0):
    """Quotients of the engine's written-out float64 division that differ from `a / b` on the device (must be 0)."""
    out = np.zeros(1, dtype=np.int64)
    L.check(L.load().c4_debug_div_mismatches(device, int(max_parent_visits), int(max_child_visits), int(n_random), _ptr(out, C.c_int64)))
    return int(out[0])


def board_centre_value(color0, color1, device=0):
    c0, c1 = _u64(color0), _u64(color1)
    out = np.zeros(len(c0), dtype=np.float64)
    L.check(L.load().c4_board_centre_value(device, _ptr(c0, C.c_uint64), _ptr(c1, C.c_uint64), len(c0),
                                           _ptr(out, C.c_double)))
    return out
