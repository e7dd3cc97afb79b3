"""ctypes binding of libc4engine.so -- the ONLY way host Python reaches the HIP engine.

Mirrors include/c4_engine.h one to one.  There is no CPU fallback: if the shared library has not
been built (python -c "import __graft_entry__ as g; g.build()") importing the symbols fails loudly,
and every compute entry point fails with C4_EDEVICE when no gfx950 device is visible.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# C4_ENGINE_LIB: tuning aid -- load another build of the same library (A/B runs of kernel variants in one process tree)
LIB_PATH = os.environ.get("C4_ENGINE_LIB") or os.path.join(_HERE, "libc4engine.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "c4_engine.h")

ABI_VERSION = 4
OK, EINVAL, EDEVICE, ENOMEM, ESTATE, ECAPACITY = 0, -1, -2, -3, -4, -5
RESULT_NONE, RESULT_XWIN, RESULT_DRAW, RESULT_OWIN = -1, 0, 1, 2
EVAL_EXTERNAL_F32, EVAL_EXTERNAL_F64, EVAL_CENTRE = 0, 1, 2
RNG_PHILOX, RNG_TAPE = 0, 1
PLANES_F32, PLANES_F16, PLANES_BF16 = 0, 1, 2
SLOT_ACTIVE, SLOT_PARKED, SLOT_MOVE_DONE = 0, 1, 2
PRIOR_NONE, PRIOR_F32, PRIOR_F64 = 0, 1, 2
PV_VALUE, PV_VISITS = 0, 1
NET_F16, NET_F32X3, NET_F32X3_WIDE = 0, 1, 2   # c4_net_desc.precision
MATCH_MAX_NETS = 16
MATCH_KERNEL_WAVE, MATCH_KERNEL_SPLIT = 0, 1   # c4_match_player.kernel
SOLVE_MAX_EMPTIES = 24
SOLVE_DEEP_MAX_EMPTIES = 42
SOLVE_TABLE_MIN_LOG2, SOLVE_TABLE_MAX_LOG2 = 10, 30
SOLVE_SOLVED, SOLVE_TERMINAL, SOLVE_UNKNOWN, SOLVE_TOO_DEEP, SOLVE_INVALID = 0, 1, 2, 3, 4
SOLVE_BOUND_NONE, SOLVE_BOUND_LOWER, SOLVE_BOUND_UPPER, SOLVE_BOUND_EXACT = 0, 1, 2, 3     # c4_solve_window's bound
# c4_solve_graph's state of a node
SOLVE_NODE_INTERIOR, SOLVE_NODE_SELF, SOLVE_NODE_ANSWERED, SOLVE_NODE_OVER_BUDGET, SOLVE_NODE_DROPPED, SOLVE_NODE_PENDING = 0, 1, 2, 3, 4, 5
SOLVE_GRAPH_MAX_PLIES = 8
SOLVE_DEFAULT_NODES_PER_LAUNCH = 1 << 14
REVIEW_COLUMNS = ("late", "outcome_known", "kept_known", "kept", "blunders", "target_agrees", "contradictions")     # C4_REVIEW_*
EXACT_LEAVES_COLUMNS = ("overridden", "over_budget", "nodes", "late")                                               # C4_EXACT_LEAVES_*
REVIEW_GAME_COLUMNS = ("n_late", "n_kept_known", "n_blunders", "last_blunder_age")                                  # C4_REVIEW_GAME_*


class EngineError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("c4 engine error %d: %s" % (code, message))
        self.code = code


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_slots", C.c_int32), ("simulations", C.c_int32),
                ("pb_c_base", C.c_int32), ("pb_c_init", C.c_double),
                ("root_dirichlet_alpha", C.c_double), ("root_exploration_fraction", C.c_double),
                ("num_sampling_moves", C.c_int32), ("eval_mode", C.c_int32), ("rng_mode", C.c_int32),
                ("seed", C.c_uint64), ("stop_after_move", C.c_int32), ("games_target", C.c_int64),
                ("record_capacity_games", C.c_int32), ("max_inner_iters", C.c_int32),
                ("planes_dtype", C.c_int32), ("eval_cache_log2_entries", C.c_int32), ("level_budget", C.c_int32), ("time_budget_cycles", C.c_int32), ("reserved", C.c_int32 * 4)]


class MatchPlayer(C.Structure):
    """c4_match_player: the player behind one net index of a match engine (c4_match_configure)."""
    _fields_ = [("simulations", C.c_int32), ("pb_c_base", C.c_int32), ("pb_c_init", C.c_double), ("kernel", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "simulations", "expansions", "children_created", "terminal_sims", "leaf_evals", "depth_sum",
        "moves", "games_started", "games_finished", "launches", "active_slots", "capped_slots",
        "eval_cache_hits", "eval_cache_probes", "bad_evals", "dropped_games", "speculative_evals")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RootResult(C.Structure):
    _fields_ = [("state", C.c_int32), ("move", C.c_int32), ("value", C.c_double),
                ("root_visits", C.c_uint32), ("root_value_sum", C.c_double),
                ("child_visits", C.c_uint32 * 7), ("child_value_sum", C.c_double * 7),
                ("child_status", C.c_int32 * 7), ("root_prior", C.c_double * 7),
                ("values_policy", C.c_double * 7), ("color0", C.c_uint64), ("color1", C.c_uint64),
                ("expansions", C.c_int64), ("simulations", C.c_int64)]


class SearchResult(C.Structure):
    """c4_search_result: one row of a position queue's result table -- the fields of RootResult, so whatever reads a
    root read-out (connect4_amd.tree.Tree) reads a row (search_result_dtype is the same layout for NumPy)."""
    _fields_ = list(RootResult._fields_)


def search_result_dtype():
    import numpy as np
    dt = np.dtype({"names": ["state", "move", "value", "root_visits", "root_value_sum", "child_visits", "child_value_sum",
                             "child_status", "root_prior", "values_policy", "color0", "color1", "expansions", "simulations"],
                   "formats": ["<i4", "<i4", "<f8", "<u4", "<f8", ("<u4", (7,)), ("<f8", (7,)), ("<i4", (7,)), ("<f8", (7,)),
                               ("<f8", (7,)), "<u8", "<u8", "<i8", "<i8"],
                   "offsets": [getattr(SearchResult, n).offset for n, _ in SearchResult._fields_],
                   "itemsize": C.sizeof(SearchResult)})
    return dt


class TreeNode(C.Structure):
    """c4_tree_node: one row of an exported tree (TREE_NODE_DTYPE is the same layout for NumPy)."""
    _fields_ = [("parent", C.c_int32), ("first_child", C.c_int32), ("visits", C.c_int32), ("move", C.c_int8),
                ("depth", C.c_int8), ("n_children", C.c_int8), ("status", C.c_int8), ("value_sum", C.c_double),
                ("color0", C.c_uint64), ("color1", C.c_uint64), ("prior", C.c_double * 7), ("prior_kind", C.c_int32),
                ("reserved", C.c_int32)]


def tree_node_dtype():
    import numpy as np
    dt = np.dtype([("parent", "<i4"), ("first_child", "<i4"), ("visits", "<i4"), ("move", "i1"), ("depth", "i1"),
                   ("n_children", "i1"), ("status", "i1"), ("value_sum", "<f8"), ("color0", "<u8"), ("color1", "<u8"),
                   ("prior", "<f8", (7,)), ("prior_kind", "<i4"), ("reserved", "<i4")])
    assert dt.itemsize == C.sizeof(TreeNode)
    return dt


class GameRecord(C.Structure):
    _fields_ = [("game_id", C.c_int64), ("length", C.c_int32), ("result", C.c_int32),
                ("color0", C.c_uint64 * 42), ("color1", C.c_uint64 * 42), ("move", C.c_int32 * 42),
                ("value", C.c_double * 42), ("policy", (C.c_double * 7) * 42)]


class ExportBuffers(C.Structure):
    """c4_export_buffers: device pointers (torch.Tensor.data_ptr()) or None."""
    _fields_ = [(n, C.c_void_p) for n in ("boards_dev", "moves_dev", "values_dev", "policy_dev", "targets_dev",
                                          "game_index_dev", "lengths_dev", "results_dev", "ids_dev")]


WINDOW_MAX_SEGMENTS = 64
WINDOW_MERGE_MAX_POSITIONS = 1 << 23        # C4_WINDOW_MERGE_MAX_POSITIONS
WINDOW_MERGE_SLOT_BYTES = 80                # C4_WINDOW_MERGE_SLOT_BYTES
WINDOW_MERGE_BLOCK = 256                    # C4_WINDOW_MERGE_BLOCK


def window_merge_work_bytes(n: int) -> int:
    """C4_WINDOW_MERGE_WORK_BYTES(n)."""
    return 4 * (n + (n + WINDOW_MERGE_BLOCK - 1) // WINDOW_MERGE_BLOCK)


class WindowSegment(C.Structure):
    """c4_window_segment: one generation of a device-resident training window (device pointers)."""
    _fields_ = [("boards", C.c_void_p), ("targets", C.c_void_p), ("policy", C.c_void_p), ("n_positions", C.c_int64)]


class ScoreAcc(C.Structure):
    """c4_score_acc: the accumulator of c4_score_update_dev, as read back from the device (112 bytes)."""
    _fields_ = [("n", C.c_int64), ("total", C.c_int64 * 3), ("correct", C.c_int64 * 3), ("prior_n", C.c_int64),
                ("prior_correct", C.c_int64), ("non_finite", C.c_int64), ("sum_outputs", C.c_double),
                ("value_sq_err_sum", C.c_double), ("prior_bce_sum", C.c_double), ("smallest", C.c_float), ("largest", C.c_float)]


class NetDesc(C.Structure):
    _fields_ = [("channels", C.c_int32), ("filters", C.c_int32), ("n_residuals", C.c_int32), ("precision", C.c_int32)] + \
        [(n, C.POINTER(C.c_float)) for n in ("stem_w", "stem_b", "conv_w", "conv_b", "head_w", "head_b",
                                             "vfc_w", "vfc_b", "vout_w", "pfc_w", "pfc_b")] + \
        [("vout_b", C.c_float), ("w1", C.c_float), ("w2", C.c_float), ("reserved2", C.c_float)]


_P = C.POINTER
_u64p, _i32p, _f32p, _f64p, _i64p = _P(C.c_uint64), _P(C.c_int32), _P(C.c_float), _P(C.c_double), _P(C.c_int64)

# name -> (restype, argtypes); every symbol include/c4_engine.h declares
SIGNATURES = {
    "c4_abi_version": (C.c_int, []),
    "c4_engine_create": (C.c_int, [_P(Config), C.c_int, _P(C.c_void_p)]),
    "c4_engine_destroy": (C.c_int, [C.c_void_p]),
    "c4_last_error": (C.c_char_p, [C.c_void_p]),
    "c4_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c4_clear_eval_cache": (C.c_int, [C.c_void_p]),
    "c4_reset": (C.c_int, [C.c_void_p, _u64p, _u64p, C.c_int32]),
    "c4_set_tapes": (C.c_int, [C.c_void_p, _f64p, _f64p, C.c_int32]),
    "c4_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c4_step_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "c4_run_centre": (C.c_int, [C.c_void_p, C.c_int32]),
    "c4_leaf_buffers": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_void_p)]),
    "c4_read_leaves": (C.c_int, [C.c_void_p, _u64p, _u64p, _i32p]),
    "c4_get_stats": (C.c_int, [C.c_void_p, _P(Stats)]),
    "c4_read_roots": (C.c_int, [C.c_void_p, _P(RootResult)]),
    "c4_tree_sizes": (C.c_int, [C.c_void_p, _i32p, C.c_int32, C.c_int32, C.c_int32, _i64p]),
    "c4_export_trees": (C.c_int, [C.c_void_p, _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _i64p]),
    "c4_export_trees_dev": (C.c_int, [C.c_void_p, _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _i64p]),
    "c4_principal_variations": (C.c_int, [C.c_void_p, _i32p, C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _P(C.c_uint32), _f64p]),
    "c4_drain_games": (C.c_int, [C.c_void_p, _P(GameRecord), C.c_int32, _i32p]),
    "c4_finished_games": (C.c_int, [C.c_void_p, _i64p, _i64p]),
    "c4_export_games_dev": (C.c_int, [C.c_void_p, _P(ExportBuffers), C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "c4_training_tensors_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "c4_window_gather_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "c4_planes_to_boards_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "c4_window_merge_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32] +
                            [C.c_void_p] * 8),
    "c4_window_last_error": (C.c_char_p, []),
    "c4_eval_cache_lookup": (C.c_int, [C.c_void_p, _u64p, _u64p, C.c_int32, _f32p, _f32p, _i32p]),
    "c4_debug_root_noise": (C.c_int, [C.c_int, C.c_uint64, C.c_double, _i64p, _i32p, _i32p, C.c_int32, _f64p, _f64p]),
    "c4_debug_sample_move": (C.c_int, [C.c_int, C.c_uint64, _i64p, _i32p, _f64p, _i32p, _f64p, C.c_int32, _f64p, _i32p]),
    "c4_debug_div_mismatches": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, _i64p]),
    "c4_board_make_move": (C.c_int, [C.c_int, _u64p, _u64p, _i32p, C.c_int32, _u64p, _u64p, _i32p]),
    "c4_board_wins": (C.c_int, [C.c_int, _u64p, C.c_int32, _i32p]),
    "c4_board_valid_mask": (C.c_int, [C.c_int, _u64p, _u64p, C.c_int32, _i32p]),
    "c4_board_planes": (C.c_int, [C.c_int, _u64p, _u64p, C.c_int32, _f32p]),
    "c4_board_fliplr": (C.c_int, [C.c_int, _u64p, _u64p, C.c_int32, _u64p, _u64p]),
    "c4_board_centre_value": (C.c_int, [C.c_int, _u64p, _u64p, C.c_int32, _f64p]),
    "c4_grid_search": (C.c_int, [C.c_int, _u64p, _u64p, C.c_int32, C.c_int32, _f64p, _f64p, _i32p]),
    "c4_grid_frontier": (C.c_int, [C.c_int, _u64p, _u64p, C.c_int32, C.c_int32, _u64p, _u64p, C.c_int64, _i64p]),
    "c4_grid_finish": (C.c_int, [C.c_int, _u64p, _u64p, C.c_int32, C.c_int32, _f64p, C.c_int64, _f64p, _f64p, _i32p]),
    "c4_grid_last_error": (C.c_char_p, []),
    "c4_debug_stamps": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "c4_debug_fused_net_stamps": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "c4_debug_latency_stamps": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "c4_debug_last_fused_kernel": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "c4_net_create": (C.c_int, [C.c_int, _P(NetDesc), _P(C.c_void_p)]),
    "c4_net_destroy": (C.c_int, [C.c_void_p]),
    "c4_net_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "c4_net_forward_wave": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "c4_net_last_error": (C.c_char_p, []),
    "c4_selfplay_steps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "c4_match_assign": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int32]),
    "c4_match_steps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "c4_match_configure": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MatchPlayer)]),
    "c4_queue_positions": (C.c_int, [C.c_void_p, _u64p, _u64p, C.c_int64]),
    "c4_queue_positions_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "c4_queue_progress": (C.c_int, [C.c_void_p, _i64p, _i64p]),
    "c4_queue_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "c4_queue_results_dev": (C.c_int, [C.c_void_p, _P(C.c_void_p), _i64p]),
    "c4_queue_export_dev": (C.c_int, [C.c_void_p] * 7),
    "c4_net_debug_stamps": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "c4_bn_workspace_floats": (C.c_longlong, [C.c_int, C.c_int]),
    "c4_bn_train_forward": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 4 + [C.c_float] * 3 + [C.c_void_p]),
    "c4_bn_train_backward": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 4 + [C.c_float, C.c_void_p]),
    "c4_conv3x3_wrw_workspace_floats": (C.c_longlong, []),
    "c4_conv3x3_wrw": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]),
    "c4_score_workspace_bytes": (C.c_longlong, [C.c_longlong]),
    "c4_score_reset_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
    "c4_score_update_dev": (C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_longlong] * 2 + [C.c_void_p] * 2),
    "c4_score_last_error": (C.c_char_p, []),
    "c4_solve_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 4),
    "c4_solve": (C.c_int, [C.c_int, _u64p, _u64p, C.c_int64, C.c_int64, C.c_int64, _P(C.c_int8), _P(C.c_int8), _P(C.c_int8), _i64p]),
    "c4_solve_children_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "c4_solve_last_error": (C.c_char_p, []),
    "c4_solve_table_create": (C.c_int, [C.c_int, C.c_int, _P(C.c_void_p)]),
    "c4_solve_table_destroy": (C.c_int, [C.c_void_p]),
    "c4_solve_table_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c4_solve_table_read": (C.c_int, [C.c_void_p, _u64p, C.c_int64]),
    "c4_solve_book_create": (C.c_int, [C.c_int, _u64p, C.c_int64, C.c_int, _P(C.c_void_p)]),
    "c4_solve_book_destroy": (C.c_int, [C.c_void_p]),
    "c4_solve_table_attach_book": (C.c_int, [C.c_void_p, C.c_void_p]),
    "c4_solve_table_create_entryless": (C.c_int, [C.c_int, _P(C.c_void_p)]),
    "c4_solve_deep_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 5),
    "c4_solve_deep": (C.c_int, [C.c_int, C.c_void_p, _u64p, _u64p, C.c_int64, C.c_int64, C.c_int64, _P(C.c_int8), _P(C.c_int8),
                                _P(C.c_int8), _i64p, _i64p]),
    "c4_solve_window_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                      C.c_int64] + [C.c_void_p] * 7),
    "c4_solve_window": (C.c_int, [C.c_int, C.c_void_p, _u64p, _u64p, _P(C.c_int8), _P(C.c_int8), C.c_int64, C.c_int64, C.c_int64] +
                        [_P(C.c_int8)] * 5 + [_i64p, _i64p]),
    "c4_solve_graph": (C.c_int, [C.c_int, C.c_void_p, _u64p, _u64p, _i64p, C.c_int, _P(C.c_int32), _P(C.c_int8), _P(C.c_int8), C.c_int64,
                                 C.c_int64] + [_P(C.c_int8)] * 5 + [_i64p, _i64p] + [_P(C.c_int8)] * 3 + [_i64p, _i64p]),
    "c4_review_select_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "c4_review_outcomes_dev": (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3),
    "c4_review_fold_dev": (C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64] + [C.c_void_p] * 14),
    "c4_exact_leaves_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
}

_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7).  Two HIP
    runtimes in one process fight over the device ("No HIP GPUs are available"), so make sure the
    one torch will use is the one already mapped when libc4engine.so resolves libamdhip64.so.7.
    Only the runtime library is preloaded here -- torch itself is not imported."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return  # torch (and its runtime) is already loaded; the SONAME match does the rest
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libc4engine.so and bind every symbol.  Raises if the HIP extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "HIP engine %s is not built. Run `python -c \"import __graft_entry__ as g; g.build()\"` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    if L.c4_abi_version() != ABI_VERSION:
        raise ImportError("libc4engine.so ABI %d != binding %d" % (L.c4_abi_version(), ABI_VERSION))
    _lib = L
    return L


def last_error(handle=None):
    msg = load().c4_last_error(handle)
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, handle=None):
    if rc != OK:
        raise EngineError(rc, last_error(handle))
