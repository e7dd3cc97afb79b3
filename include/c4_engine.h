/*
 * c4_engine.h -- C ABI of the MI355X-native Connect4 self-play / MCTS engine (libc4engine.so).
 *
 * This is the drop-in boundary for the hot path of willis-richard/connect4 (`oinkoink`).  The
 * reference has no FFI: its seam is two duck-typed Python protocols.  Each
 * entry point below names the reference interface it stands in for (file:line relative to the
 * reference root).  Host code (Python ctypes in connect4_amd/_lib.py, or any cgo/JNI/ctypes binding,
 * see INTEGRATION.md) calls ONLY these functions; no HIP, torch or C++ types cross the boundary.
 *
 * Conventions
 *   - every function returns 0 on success or a negative C4_E* code; nothing throws across the ABI;
 *     c4_last_error() returns a static/engine-owned message for the last failure;
 *   - the engine owns all tree memory in HBM; the caller owns I/O buffers and keeps them alive
 *     until the stream has been synchronised;
 *   - pointers named *_dev are DEVICE pointers (e.g. torch.Tensor.data_ptr()); all others are host;
 *   - one engine per GPU per process, one host thread drives a handle (mirrors "one player serves
 *     one game at a time", game_pool.py:29-32,45-49);
 *   - there is NO CPU backend: creating an engine without a usable gfx950 device fails loudly.
 */
#ifndef C4_ENGINE_H
#define C4_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C4_ABI_VERSION 4

/* error codes */
#define C4_OK 0
#define C4_EINVAL (-1)   /* bad argument */
#define C4_EDEVICE (-2)  /* no usable HIP device / HIP call failed */
#define C4_ENOMEM (-3)
#define C4_ESTATE (-4)   /* call not valid in the current engine state */
#define C4_ECAPACITY (-5)

/* Result codes (utils.py:19-22): value = code * 0.5 */
#define C4_RESULT_NONE (-1)
#define C4_RESULT_XWIN 0
#define C4_RESULT_DRAW 1
#define C4_RESULT_OWIN 2

/* How leaf positions are evaluated (the `evaluator` argument of mcts.py:70-76 / :94-97). */
#define C4_EVAL_EXTERNAL_F32 0 /* values float32[n], priors float32[n][7] written by the caller (the
                                  net: model.py:269-282).  PUCT score arithmetic follows what the
                                  reference does with a float32 prior under NumPy>=2 (float32). */
#define C4_EVAL_EXTERNAL_F64 1 /* values float64[n], priors float64[n][7] (a Python evaluator
                                  returning float64, e.g. a table or heuristic): float64 scoring. */
#define C4_EVAL_CENTRE 2       /* evaluators.py:28-38 evaluate_centre_with_prior computed in-kernel;
                                  whole searches run inside one launch (no leaf round trip). */

#define C4_RNG_PHILOX 0 /* counter-based in-kernel RNG keyed by (seed, game id, ply) */
#define C4_RNG_TAPE 1   /* caller-injected Gamma draws / uniforms (parity tests: the reference uses
                           NumPy's global Mersenne state, mcts.py:175-177, tree.py:80) */

#define C4_PLANES_F32 0
#define C4_PLANES_F16 1
#define C4_PLANES_BF16 2

/* mcts.py:13-26 MCTSConfig + engine shape. */
typedef struct {
    int32_t abi_version;               /* = C4_ABI_VERSION */
    int32_t n_slots;                   /* games advanced in lock-step on this GPU */
    int32_t simulations;               /* mcts.py:15 */
    int32_t pb_c_base;                 /* mcts.py:16 (19652) */
    double  pb_c_init;                 /* mcts.py:17 (1.25) */
    double  root_dirichlet_alpha;      /* mcts.py:18 */
    double  root_exploration_fraction; /* mcts.py:19 */
    int32_t num_sampling_moves;        /* mcts.py:20 */
    int32_t eval_mode;                 /* C4_EVAL_* */
    int32_t rng_mode;                  /* C4_RNG_* */
    uint64_t seed;
    int32_t stop_after_move;           /* 1: a slot parks after choosing ONE move (MCTS.make_move,
                                          mcts.py:78-88); 0: continuous self-play (training_game.py:8-19) */
    int64_t games_target;              /* self-play: slots park once this many games were started;
                                          <0 = unbounded (bench) */
    int32_t record_capacity_games;     /* rows of the device ring of finished games (completion order).  Moves
                                          are staged per slot while a game is in flight and copied to a ring row
                                          when it ends; a game that finds every row unread is dropped and counted
                                          (c4_stats.dropped_games), never mixed with another game.  0 = 2 x n_slots */
    int32_t max_inner_iters;           /* cap on simulations a slot may complete inside one step call
                                          without needing the evaluator (terminal or cached leaves);
                                          bounds the duration of c4_step and of one tree call inside
                                          the fused kernels.  0 = default */
    int32_t planes_dtype;              /* C4_PLANES_* layout of the leaf batch handed to the net */
    int32_t eval_cache_log2_entries;   /* device-wide evaluation cache = the reference's memo table
                                          (evaluators.py:9-25), shared by every slot and game: a leaf
                                          whose position was already answered is applied in place, no
                                          evaluator round trip.  Results are unchanged for a
                                          deterministic evaluator.  <0 off, 0 auto (on for self-play
                                          with C4_EVAL_EXTERNAL_F32: 256 x n_slots x simulations entries
                                          of 48 bytes, at most 2^30 and a quarter of the free device
                                          memory), else log2 of the table size */
    int32_t level_budget;              /* descent levels a slot may walk per launch; a descent that runs
                                          out is suspended and resumed by the next launch, so no launch
                                          waits for the deepest tree of the batch.  0 = unlimited */
    int32_t time_budget_cycles;        /* c4_step / block-mode fused kernel: a slot starts no further evaluator-free
                                          simulation once its step call has run this many shader cycles (balances
                                          the waves of a launch by cost instead of by count).  Wave-autonomous
                                          fused kernel: length of one step in shader cycles.  Which launch runs
                                          a simulation never changes results.  0 = off / 80,000 */
    int32_t reserved[4];               /* must be 0; reserved[0] = n_match_nets: > 0 creates a match engine (c4_match_steps) with that
                                          many evaluation caches, one per net (at most C4_MATCH_MAX_NETS); the auto size is
                                          divided among them.  Needs C4_EVAL_EXTERNAL_F32 and stop_after_move = 0;
                                          reserved[1] = 1 creates a position-queue engine (c4_queue_positions): needs stop_after_move = 1,
                                          any eval_mode; with C4_EVAL_EXTERNAL_F32 the auto size of the evaluation cache applies.
                                          reserved[0] > 0 together with reserved[1] is C4_EINVAL */
} c4_config;

typedef struct c4_engine c4_engine;

/* Aggregate counters since the last c4_reset (units defined in SURVEY.md section 8d). */
typedef struct {
    int64_t simulations;        /* iterations of mcts.py:107-120 completed */
    int64_t expansions;         /* expand_node calls that materialise children (mcts.py:115) */
    int64_t children_created;
    int64_t terminal_sims;      /* simulations that ended on a terminal leaf (no evaluator call) */
    int64_t leaf_evals;         /* leaves handed to the evaluator (incl. one root per move) */
    int64_t depth_sum;          /* sum over simulations of leaf depth */
    int64_t moves;              /* moves chosen (mcts.py:78-88) */
    int64_t games_started;
    int64_t games_finished;
    int64_t launches;           /* rollout-step kernel launches */
    int64_t active_slots;       /* slots not parked right now */
    int64_t capped_slots;       /* slot-launches that hit max_inner_iters */
    int64_t eval_cache_hits;    /* leaves answered by the evaluation cache (subset of leaf_evals) */
    int64_t eval_cache_probes;
    int64_t bad_evals;          /* evaluator answers that were not finite / out of range and were replaced
                                   (value 0.5, prior 0; an all-zero prior becomes uniform) -- the reference
                                   asserts instead (model.py:258-263); must be 0 in a healthy run */
    int64_t dropped_games;      /* finished games that found the record ring full (nobody drained or exported
                                   for record_capacity_games games) and were not recorded; 0 in a healthy run */
    int64_t speculative_evals;  /* c4_selfplay_steps: network passes on positions evaluated ahead of the search (the
                                   best-prior child of a fresh expansion) and put into the evaluation cache; not part
                                   of leaf_evals -- network passes in total = leaf_evals - eval_cache_hits + this */
} c4_stats;

/* Root read-out of one slot (tree.py:66-117; what MCTS.make_move returns, mcts.py:88). */
typedef struct {
    int32_t  state;             /* 0 searching, 1 parked (no game), 2 move chosen */
    int32_t  move;              /* chosen column or -1 */
    double   value;             /* child.data.absolute_value of the chosen child (NaN if None) */
    uint32_t root_visits;
    double   root_value_sum;
    uint32_t child_visits[7];
    double   child_value_sum[7];
    int32_t  child_status[7];   /* -2 absent, -1 non-terminal, else C4_RESULT_* */
    double   root_prior[7];     /* normalised (+ noise) prior used at the root */
    double   values_policy[7];  /* tree.py:104-109 */
    uint64_t color0, color1;    /* root position searched */
    int64_t  expansions;
    int64_t  simulations;
} c4_root_result;

/* One finished self-play game (training_game.py:42-67 GameData). */
typedef struct {
    int64_t  game_id;
    int32_t  length;
    int32_t  result;            /* C4_RESULT_* */
    uint64_t color0[42], color1[42];   /* board BEFORE each move (training_game.py:12) */
    int32_t  move[42];
    double   value[42];         /* child.data.absolute_value (training_game.py:13) */
    double   policy[42][7];     /* tree.get_values_policy() (training_game.py:14) */
} c4_game_record;

/* -- lifecycle ------------------------------------------------------------------------------- */
/* Replaces constructing MCTS(name, MCTSConfig, evaluator) (mcts.py:70-76) + the game_pool /
 * InferenceServer scaffolding (game_pool.py:15-42, inference_server.py:15-63).
 * The config's doubles are checked, because a PUCT score that is NaN has no place in the argmax (evaluator answers are
 * made finite for the same reason, c4_stats.bad_evals): C4_EINVAL with a message for a pb_c_init that is not finite
 * (inf times a zero prior), a root_dirichlet_alpha that is not finite or negative (the Gamma shape of the in-kernel RNG),
 * and a root_exploration_fraction that is not finite or outside [0, 1].  Negative pb_c_init and any pb_c_base >= 1 are
 * served.  (With C4_EVAL_EXTERNAL_F32 the exploration factor is rounded to float32, as the reference's is: keep pb_c_init
 * inside float32's range.)  (A stricter check, not a new layout: C4_ABI_VERSION stays.) */
int c4_engine_create(const c4_config *cfg, int device, c4_engine **out);
int c4_engine_destroy(c4_engine *e);
const char *c4_last_error(const c4_engine *e /* may be NULL */);
/* Order the engine's kernels with the caller's stream (torch.cuda.current_stream().cuda_stream). */
int c4_set_stream(c4_engine *e, void *hip_stream);
/* Forget all cached evaluations (call when the evaluator's weights change; evaluators.py: a new
 * Evaluator / position_table per generation, game_pool.py:21-27). */
int c4_clear_eval_cache(c4_engine *e);

/* Start positions for the first n_active slots (Tree(board), tree.py:62-64); NULL => empty boards
 * (Board(), board.py:36-41).  Remaining slots park.  Clears counters, records and game ids. */
int c4_reset(c4_engine *e, const uint64_t *color0, const uint64_t *color1, int32_t n_active);

/* C4_RNG_TAPE: gamma_noise[game][ply][7] raw Gamma(alpha,1) draws (mcts.py:175-177) and
 * uniforms[game][ply] (the one uniform np.random.choice consumes, tree.py:80). `n_games` rows.
 * A Gamma draw that is negative or not finite, or a uniform that is NaN (a negative uniform means "no sampling: take
 * best_move"), is C4_EINVAL and the engine stays as it was, its earlier tapes included.
 * THE CALLER'S OBLIGATION: a row used at a root must not sum to zero over that root's legal columns.  Which columns are
 * legal depends on the position, so this call cannot know; the reference divides 0 / 0 there too (mcts.py:178, 197-202),
 * and the NaN prior that follows has no defined search. */
int c4_set_tapes(c4_engine *e, const double *gamma_noise, const double *uniforms, int32_t n_games);

/* -- the hot path --------------------------------------------------------------------------- */
/* One rollout step for every live slot, asynchronous on the engine's stream:
 *   1. apply the evaluator's answer for the slot's pending leaf (mcts.py:124-135 evaluate_node:
 *      mask + normalise prior, store; root: add_exploration_noise mcts.py:171-181), create the
 *      children (tree.py:119-132) and back the value up the path (mcts.py:164-168);
 *   2. run simulations (mcts.py:107-116: PUCT descent ucb_score/select_child mcts.py:138-161)
 *      until the slot needs the evaluator again; terminal leaves are scored in place
 *      (mcts.py:125-128); after `simulations` sims choose the move (mcts.py:81-86), record it
 *      (training_game.py:12-15) and re-root;
 *   3. write the slot's leaf as NN input planes (board.py:147-154 to_array) into planes_dev
 *      [n_slots][3][6][7] and its bitboards into the engine's leaf buffers.
 * values_dev / priors_dev hold the answers for the leaves emitted by the PREVIOUS step, in slot
 * order (dtype per eval_mode; ignored by C4_EVAL_CENTRE; may be NULL on the first step).
 * planes_dev may be NULL when the caller evaluates from the bitboards instead. */
int c4_step(c4_engine *e, const void *values_dev, const void *priors_dev, void *planes_dev);

/* The same step for slots [slot_lo, slot_lo+slot_count) only, on `hip_stream` (NULL = the engine's
 * stream).  Lets the host pipeline two halves of the batch on two streams: the tree kernel of one half
 * runs while the network evaluates the other half's leaves.  Buffers stay indexed by absolute slot. */
int c4_step_range(c4_engine *e, const void *values_dev, const void *priors_dev, void *planes_dev,
                  int32_t slot_lo, int32_t slot_count, void *hip_stream);

/* C4_EVAL_CENTRE convenience: launch until every slot has parked (stop_after_move) or
 * max_launches is reached.  Synchronous. */
int c4_run_centre(c4_engine *e, int32_t max_launches);

/* Leaves emitted by the last step: device views (engine-owned, valid until destroy) ... */
int c4_leaf_buffers(c4_engine *e, const uint64_t **color0_dev, const uint64_t **color1_dev,
                    const int32_t **has_leaf_dev);
/* ... and a synchronous host copy (for Python evaluators, evaluators.py:18-25). */
int c4_read_leaves(c4_engine *e, uint64_t *color0, uint64_t *color1, int32_t *has_leaf);

/* -- read-out ------------------------------------------------------------------------------- */
int c4_get_stats(c4_engine *e, c4_stats *out);                 /* synchronous */
int c4_read_roots(c4_engine *e, c4_root_result *out /* [n_slots] */);   /* synchronous */
/* Up to `cap` finished games not yet consumed (oldest first; the batch is returned sorted by game id;
 * training.py:131 games.extend).  One or two device-to-host copies for the whole batch. */
int c4_drain_games(c4_engine *e, c4_game_record *out, int32_t cap, int32_t *n_out);
/* Finished games waiting in the ring / finished games lost to a full ring.  Synchronous. */
int c4_finished_games(c4_engine *e, int64_t *n_ready, int64_t *n_dropped);

/* -- whole search trees --------------------------------------------------------------------- */
/* One node of an exported tree: what the reference keeps per anytree Node (tree.py:18-64 NodeData, mcts.py:29-66).
 * A tree is a table of these in breadth-first order -- within a level by parent, within a parent by ascending
 * column -- so row 0 is the root, a node's children are the rows first_child .. first_child + n_children - 1 and stand
 * in the order of the reference's node.children (tree.py:125-129).
 * Shape: the reference creates a node's children when the node is reached a second time (mcts.py:113-116), the engine
 * when the node's evaluation is applied; the export follows the reference: a non-terminal node has children iff
 * visits >= 2.  A once-visited node has none, but its prior is known (it comes from its child records). */
#define C4_PRIOR_NONE 0 /* position_value is None: never evaluated, or the position is finished (mcts.py:125-128) */
#define C4_PRIOR_F32 1  /* prior[] holds float32 values widened exactly (a net's answer, normalised in float32) */
#define C4_PRIOR_F64 2  /* prior[] is float64 (table / heuristic evaluator, or the root after the noise, mcts.py:180) */
typedef struct {
    int32_t  parent;        /* row of node.parent, -1 for the root */
    int32_t  first_child;   /* row of the first exported child, -1 when n_children == 0 */
    int32_t  visits;        /* search_value.visit_count; 0 with value_sum 0.0: search_value is None */
    int8_t   move;          /* node.name: the column played into this node, -1 for the root */
    int8_t   depth;         /* plies below the root */
    int8_t   n_children;    /* exported children (after the filters) */
    int8_t   status;        /* node.data.board.result: -1 undecided, else C4_RESULT_* */
    double   value_sum;     /* search_value.value_sum (absolute: o's point of view, as the reference keeps it) */
    uint64_t color0, color1;   /* node.data.board, rebuilt on the device from the parent's board and the move */
    double   prior[7];      /* position_value.prior of THIS node by column: normalised over the legal columns, zeros
                               elsewhere; the root's after the Dirichlet noise; all zero when prior_kind is C4_PRIOR_NONE */
    int32_t  prior_kind;    /* C4_PRIOR_* */
    int32_t  reserved;
} c4_tree_node;

/* When a tree may be read: between launches, in any slot state, for engines driven by c4_step / c4_step_range /
 * c4_run_centre AND by c4_selfplay_steps (the fused kernels keep node 0 and the pool current -- the backups write the
 * root record like any other -- and write the slot state back when a launch ends).  A slot that is still searching
 * gives a consistent snapshot: a leaf waiting for its evaluation has not been backed up, so the counts add up.  A
 * slot without a tree of its root position -- parked, or its root still waits for the evaluator -- exports 0 nodes.
 * Filters, applied on the device: nodes with fewer than min_visits visits are dropped (0 keeps the unvisited
 * children), and nodes deeper than max_depth (< 0: no limit); a dropped node drops its subtree, and n_children /
 * first_child refer to what was exported.  slots[n]: distinct slot indices, NULL = slots 0..n-1.
 * A bad or repeated slot, a null buffer or too little capacity: C4_EINVAL, nothing is written beyond `capacity` and
 * the engine stays usable.  All three calls are synchronous. */
/* n_nodes[i] = rows of the table of slots[i] under the two filters */
int c4_tree_sizes(c4_engine *e, const int32_t *slots, int32_t n, int32_t min_visits, int32_t max_depth, int64_t *n_nodes);
/* nodes[capacity] (host) receives the tables back to back, offsets[n + 1] where each starts (offsets[n] = rows in all) */
int c4_export_trees(c4_engine *e, const int32_t *slots, int32_t n, int32_t min_visits, int32_t max_depth, c4_tree_node *nodes,
                    int64_t capacity, int64_t *offsets);
/* the same into a DEVICE buffer (offsets stays a host array) */
int c4_export_trees_dev(c4_engine *e, const int32_t *slots, int32_t n, int32_t min_visits, int32_t max_depth, c4_tree_node *nodes_dev,
                        int64_t capacity, int64_t *offsets);

/* Principal variations, walked on the device: from the root repeatedly the child that Tree.best_move takes for the
 * side to move AT THAT NODE (C4_PV_VALUE: largest data.value(side) -- unvisited 0.0, a finished position its exact
 * result; tree.py:38-44,69-73) or that Tree.most_visited takes (C4_PV_VISITS, tree.py:84-91), ties to the higher
 * column (tree.py:11-15), until a node without children in reference shape or max_len (1..64) moves.
 * moves / visits / values [n][max_len]: column, visit count and absolute_value (tree.py:27-36; NaN for None) of each
 * node on the line; beyond lengths[i]: -1, 0, 0.0. */
#define C4_PV_VALUE 0
#define C4_PV_VISITS 1
int c4_principal_variations(c4_engine *e, const int32_t *slots, int32_t n, int32_t rule, int32_t max_len, int32_t *moves,
                            int32_t *lengths, uint32_t *visits, double *values);

/* Device-side export: pack up to max_games finished games (oldest first, whole games only, at most
 * cap_positions positions) into caller-owned DEVICE buffers and consume them -- no host round trip, so
 * it can be queued behind c4_selfplay_steps on the same stream.  Layout = the compact record of
 * SURVEY.md 8e (what training_game.py:42-67 GameData holds, ~50 B/position); any pointer may be NULL.
 * counts_dev (device int64[2], may be NULL) receives {games, positions} exported.
 * Stands in for pool.imap_unordered(...) / games.extend (training.py:122-131) + the per-position
 * Python of TrainingDataStorage.save (data.py:52-64). */
typedef struct {
    int64_t *boards_dev;      /* [cap_positions][2]  color0, color1 of the board BEFORE the move */
    uint8_t *moves_dev;       /* [cap_positions] */
    float   *values_dev;      /* [cap_positions]     child.data.absolute_value (NaN if None) */
    float   *policy_dev;      /* [cap_positions][7]  tree.get_values_policy() */
    float   *targets_dev;     /* [cap_positions]     game result value (create_training_values) */
    int32_t *game_index_dev;  /* [cap_positions]     index of the position's game inside this export */
    int32_t *lengths_dev;     /* [max_games] */
    int8_t  *results_dev;     /* [max_games]         C4_RESULT_* */
    int64_t *ids_dev;         /* [max_games] */
} c4_export_buffers;
int c4_export_games_dev(c4_engine *e, const c4_export_buffers *bufs, int32_t max_games, int64_t cap_positions,
                        int64_t *counts_dev, void *hip_stream);
/* native_to_pytorch(boards, values, priors, add_fliplr) (data.py:78-105) on device: boards
 * float32 [m][3][6][7] (board.py:147-154), values float32 [m], priors float32 [m][7], m = n or 2n with
 * the left-right mirrored copies after the originals (board.py:115-145, priors reversed). */
int c4_training_tensors_dev(int device, void *hip_stream, const int64_t *boards_dev, const float *targets_dev,
                            const float *policy_dev, int64_t n, int32_t add_fliplr, float *out_boards_dev,
                            float *out_values_dev, float *out_priors_dev);

/* -- the sliding training window on the device (c4_window.hip) ------------------------------- */
/* TrainingDataStorage.get_dataset (data.py:66-75) + native_to_pytorch (data.py:78-105) without the
 * materialised tensors: the window is a device table of segments, one per generation, newest first, each the
 * packed positions of that generation (what c4_export_games_dev wrote: boards int64 [n][2], targets float32 [n],
 * policy float32 [n][7]).  Segment s contributes 2 n_s virtual rows -- its positions as stored, then their
 * left-right mirrors (board.py:115-145, priors reversed, value duplicated) -- and rows are numbered across the
 * segments in table order: the row order of the reference's ConcatDataset over the generations' data.pth.
 * c4_window_gather_dev writes, for each of m int64 indices, boards_out float32 [m][3][6][7] (board.py:147-154),
 * values_out float32 [m], priors_out float32 [m][7]: the bits that indexing the concatenated
 * c4_training_tensors_dev outputs gives.  An index outside [0, rows) reads nothing, its row is zeros, and it is
 * added to *n_out_of_range_dev (device int32, may be NULL; the caller zeroes it).  1 <= n_segments <=
 * C4_WINDOW_MAX_SEGMENTS, else C4_EINVAL.  One launch on hip_stream; allocates nothing, waits for nothing
 * (capturable in a HIP graph).  Messages of both calls: c4_window_last_error(). */
#define C4_WINDOW_MAX_SEGMENTS 64
typedef struct {
    const int64_t *boards;    /* device [n_positions][2] */
    const float   *targets;   /* device [n_positions] */
    const float   *policy;    /* device [n_positions][7] */
    int64_t        n_positions;
} c4_window_segment;
int c4_window_gather_dev(int device, void *hip_stream, const c4_window_segment *segments_dev, int32_t n_segments,
                         const int64_t *index_dev, int64_t m, float *boards_out, float *values_out, float *priors_out,
                         int32_t *n_out_of_range_dev /* may be NULL */);
/* The inverse of c4_board_planes (board.py:147-154): planes_dev float32 [n][3][6][7] -> boards_out int64 [n][2].
 * Adds to *n_bad_dev (device int32; the caller zeroes it) the rows that no board encodes: a cell that is neither
 * 0.0 nor 1.0, a cell set in both colours, a to-move plane that is not constant, or one that contradicts the
 * parity of the stone count.  For data.pth files the library did not write.  One launch on hip_stream. */
int c4_planes_to_boards_dev(int device, void *hip_stream, const float *planes_dev, int64_t n, int64_t *boards_out,
                            int32_t *n_bad_dev);
/* Identical positions of the window merged into one row each, carrying the mean of their targets and priors.
 * Input: the n_positions positions of the n_segments segments in table order, as stored (mirror rows are no inputs);
 * n_positions must be the table's total -- a position the table does not hold counts as a bad row.
 *   key       occ = c0 | c1, mover = c1 when popcount(occ) is odd, else c0; key = mover + occ + BOTTOM (c4_solve.hip's
 *             tt_key), mkey = the key of the left-right mirror image.  With `mirror` the group key is min(key, mkey) and
 *             a member with key > mkey is REVERSED; without, the group key is key and nobody is reversed.
 *   bad rows  c0 & c1 != 0, a stone outside the 42 cells, a stone with no stone under it, a target or prior that is not
 *             finite or outside [0, 1].  They join no group and are counted in *n_bad_dev; the outputs then mean nothing.
 *   sums      per group a count and eight int64 sums: T = sum rne(target 2^40), P[c] = sum rne(prior[c'] 2^40) with
 *             c' = 6 - c for a reversed member, else c.  Integer sums: the order of addition does not matter.
 *             n_positions < C4_WINDOW_MERGE_MAX_POSITIONS keeps every sum below 2^63; else C4_EINVAL.
 *   output    one row per group, groups in the order of their first members; the board is the first member's as stored;
 *             target = float32(float64(T) / (float64(count) 2^40)), prior[c] likewise from P[c], or from P[6 - c] when the
 *             first member is reversed; counts int32.  A group of one copies its target and priors bit for bit.
 * table_dev: C4_WINDOW_MERGE_SLOT_BYTES << log2_capacity bytes, cleared by the call; 2^log2_capacity < n_positions is
 * C4_EINVAL (log2_capacity 0..30).  work_dev: C4_WINDOW_MERGE_WORK_BYTES(n_positions) bytes.  The four outputs have room
 * for n_positions rows; *n_distinct_dev (device int32) says how many were written.  wave_combine != 0 sums equal keys
 * inside a wave before going to memory: the same results, sooner when many positions repeat (self-play windows).
 * A few launches and memsets on hip_stream; allocates nothing, waits for nothing.  Messages: c4_window_last_error().
 * (An addition: C4_ABI_VERSION stays.) */
#define C4_WINDOW_MERGE_MAX_POSITIONS (1 << 23)
#define C4_WINDOW_MERGE_SLOT_BYTES 80
#define C4_WINDOW_MERGE_BLOCK 256
#define C4_WINDOW_MERGE_WORK_BYTES(n) (4 * ((int64_t)(n) + ((int64_t)(n) + C4_WINDOW_MERGE_BLOCK - 1) / C4_WINDOW_MERGE_BLOCK))
int c4_window_merge_dev(int device, void *hip_stream, const c4_window_segment *segments_dev, int32_t n_segments,
                        int64_t n_positions, int32_t mirror, int32_t wave_combine, int32_t log2_capacity, void *table_dev,
                        void *work_dev, int64_t *boards_out, float *targets_out, float *policy_out, int32_t *counts_out,
                        int32_t *n_distinct_dev, int32_t *n_bad_dev);
const char *c4_window_last_error(void);

/* Read-out of the evaluation cache (the memo table of evaluators.py:9-25): what it answers for the given
 * positions.  found[i] = 0 when the position is absent (never evaluated, or evicted).  Synchronous.
 * Lets a test replay device games on the oracle with exactly the evaluations the device used. */
int c4_eval_cache_lookup(c4_engine *e, const uint64_t *color0, const uint64_t *color1, int32_t n, float *value,
                         float *prior /* [n][7] */, int32_t *found);

/* Read-outs of the PRODUCTION random streams (C4_RNG_PHILOX), computed by the very device functions the
 * engine's kernels call, for statistical tests: the root noise of (seed, game id, ply) -- gamma_raw[n][7] =
 * Gamma(alpha,1) draws (mcts.py:175-177), dirichlet[n][7] = zeroed on illegal columns and normalised
 * (mcts.py:178) -- and the sampled opening move (tree.py:75-82): child index chosen among n_children
 * values (from the root mover's side, child k in lane k) with the engine's uniform of (seed, game id, ply),
 * or with uniforms[i] when given. */
int c4_debug_root_noise(int device, uint64_t seed, double alpha, const int64_t *game_id, const int32_t *ply,
                        const int32_t *legal_mask, int32_t n, double *gamma_raw, double *dirichlet);
int c4_debug_sample_move(int device, uint64_t seed, const int64_t *game_id, const int32_t *ply,
                         const double *child_values /* [n][7] */, const int32_t *n_children,
                         const double *uniforms /* may be NULL */, int32_t n, double *uniform_out, int32_t *choice_out);

/* The level loop and the backups divide with an instruction sequence written out for normal-range operands (the compiler's
 * IEEE float64 division minus its scaling / fix-up instructions; c4_engine.hip: div_normal).  This runs that sequence and the
 * plain division on the device for every (parent visits N < max_parent_visits, child visits n < max_child_visits) pair of the
 * PUCT score's sqrt(N) / (n + 1) (mcts.py:153-154) and for n_random value-sum / visit-count quotients of the backups
 * (mcts.py:164-168), and returns the number of quotients whose bits differ (must be 0). */
int c4_debug_div_mismatches(int device, int32_t max_parent_visits, int32_t max_child_visits, int64_t n_random, int64_t *mismatches);

/* -- pure board functions, executed by the device code (bit-exact parity tests) ------------- */
/* board.py:160-170 make_move + result */
int c4_board_make_move(int device, const uint64_t *color0, const uint64_t *color1, const int32_t *col,
                       int32_t n, uint64_t *out0, uint64_t *out1, int32_t *result);
/* board.py:173-184 _check_terminal_position */
int c4_board_wins(int device, const uint64_t *stones, int32_t n, int32_t *out);
/* board.py:88-92 valid_moves as a 7-bit mask (0 when the position is decided, board.py:56-62) */
int c4_board_valid_mask(int device, const uint64_t *color0, const uint64_t *color1, int32_t n, int32_t *out);
/* board.py:147-154 to_array, float32 [n][3][6][7] */
int c4_board_planes(int device, const uint64_t *color0, const uint64_t *color1, int32_t n, float *out);
/* board.py:115-145 create_fliplr / flip_color */
int c4_board_fliplr(int device, const uint64_t *color0, const uint64_t *color1, int32_t n,
                    uint64_t *out0, uint64_t *out1);
/* evaluators.py:28-33 evaluate_centre (float64) */
int c4_board_centre_value(int device, const uint64_t *color0, const uint64_t *color1, int32_t n, double *out);

/* -- fixed-depth negamax, the reference's GridSearch (c4_grid.hip) ---------------------------- */
/* grid_search.py:10-71 + tree.py:68-72,119-131: exhaustive negamax `plies` deep (1..42) below each of n
 * undecided positions, evaluate_centre (evaluators.py:28-33) at the depth-0 leaves.  Per position:
 * child_values float64 [n][7] = the root children's absolute_value (tree.py:27-38: a finished child gives
 * its result without the age term; NaN for an illegal column), root_value float64 [n] = the root's
 * search_value, move int32 [n] = Tree.best_move (ties to the higher column).  A finished or malformed
 * position, or plies out of range: C4_EINVAL.  Messages of all c4_grid_* calls: c4_grid_last_error().
 * Test aids (environment, read per call): C4_GRID_LEVEL_CAP (most nodes of one expanded level, >= 7;
 * default 2^21) and C4_GRID_FILL_NODES (level size at which the depth-first tail starts; default half the
 * device's resident lanes) change how the work is split, never the answers. */
int c4_grid_search(int device, const uint64_t *color0, const uint64_t *color1, int32_t n, int32_t plies,
                   double *child_values, double *root_value, int32_t *move);
/* grid_search.py:51-54 with any other scalar evaluator, step 1: the undecided positions `plies` deep, in
 * the order the reference calls its evaluator on them (repeats included), into leaf0/leaf1 [cap];
 * *n_leaves = their number (C4_ECAPACITY if it exceeds cap: call again with a larger buffer). */
int c4_grid_frontier(int device, const uint64_t *color0, const uint64_t *color1, int32_t n, int32_t plies,
                     uint64_t *leaf0, uint64_t *leaf1, int64_t cap, int64_t *n_leaves);
/* step 2: leaf_values float64 [n_leaves], the evaluator's value of each c4_grid_frontier leaf in its
 * order (C4_EINVAL if n_leaves is not the frontier's size); outputs as c4_grid_search. */
int c4_grid_finish(int device, const uint64_t *color0, const uint64_t *color1, int32_t n, int32_t plies,
                   const double *leaf_values, int64_t n_leaves, double *child_values, double *root_value, int32_t *move);
const char *c4_grid_last_error(void);

/* -- fused leaf-batch network (c4_net.hip) -------------------------------------------------- */
/* Eval-mode forward of the reference's Net (oinkoink/neural/pytorch/model.py:120-134) as ONE
 * gfx950 MFMA kernel reading the leaves' bitboards; stands in for ModelWrapper._call_list
 * (model.py:269-282) + the InferenceServer round trip (inference_server.py:50-63).
 * All weights are host float32 with BatchNorm already folded (eval mode):
 *   stem_w [F][3][3][3], stem_b [F]            body.0 (model.py:20-31)
 *   conv_w [2R][F][F][3][3], conv_b [2R][F]    residual blocks, conv1 then conv2 (model.py:36-55)
 *   head_w [3][F], head_b [3]                  value 1x1 conv, then the 2 policy 1x1 channels
 *   vfc_w [42][42], vfc_b [42]                 the activation-free Linear stack collapsed (model.py:69-70,83)
 *   vout_w [42], vout_b                        value_head.fc1 (model.py:72,85)
 *   pfc_w [7][84], pfc_b [7]                   policy_head.fc1 (model.py:104,113)
 *   w1, w2                                     value_head.w1/w2 (model.py:74-75,88) */
/* arithmetic of the fused forwards */
#define C4_NET_F16 0    /* fp16 storage, fp32 accumulation: one MFMA per k-step */
#define C4_NET_F32X3 1  /* reference precision: fp32 operands split into fp16 hi + scaled lo, three MFMAs per k-step; 32 filters */
#define C4_NET_F32X3_WIDE 2  /* the same arithmetic for 64 filters (a layer in two cout halves); the stand-alone forward runs
                              * four waves per workgroup, c4_selfplay_steps four tree + four network waves (split kernel only:
                              * C4_FUSED_MODE=wave / block return C4_ESTATE) */
typedef struct {
    int32_t channels, filters, n_residuals;
    int32_t precision;   /* C4_NET_F16, C4_NET_F32X3 (32 filters only) or C4_NET_F32X3_WIDE (64 filters only) */
    const float *stem_w, *stem_b, *conv_w, *conv_b, *head_w, *head_b;
    const float *vfc_w, *vfc_b, *vout_w, *pfc_w, *pfc_b;
    float vout_b, w1, w2, reserved2;
} c4_net_desc;
typedef struct c4_net c4_net;
int c4_net_create(int device, const c4_net_desc *desc, c4_net **out);
int c4_net_destroy(c4_net *net);
/* values_dev float32[n] in [0,1] (o's side), priors_dev float32[n][7]; bitboards as emitted by
 * c4_step (c4_leaf_buffers).  Asynchronous on hip_stream. */
int c4_net_forward(c4_net *net, void *hip_stream, const uint64_t *color0_dev, const uint64_t *color1_dev,
                   int32_t n, float *values_dev, float *priors_dev);
/* c4_net_forward evaluated by the wave-private forward the fused self-play kernel uses (one wave = one
 * position, no workgroup barrier).  Same arguments, bit-identical answers. */
int c4_net_forward_wave(c4_net *net, void *hip_stream, const uint64_t *color0_dev, const uint64_t *color1_dev,
                        int32_t n, float *values_dev, float *priors_dev);
const char *c4_net_last_error(void);

/* Fused persistent self-play: the rollout step and the leaf evaluation of n_steps steps in ONE launch,
 * no kernel boundary and no global barrier; slot state, leaves and answers stay in LDS for the whole
 * launch.  Default (split kernel): on every CU four tree waves own the workgroup's 16 (32) slots and walk their
 * trees; a slot that needs the evaluator posts its leaf in LDS and idles while its wave's other slots walk on;
 * four network waves claim posted leaves, run the forward and write the answer back (and, when no leaf waits,
 * evaluate the best-prior child of the position just answered into the evaluation cache: c4_stats.speculative_evals)
 * -- no workgroup barrier;
 * a "step" is a time quantum of c4_config.time_budget_cycles shader cycles (80,000 if 0) and the launch runs
 * for n_steps quanta, however many simulations the trees needed per network answer.  With the environment
 * variable C4_FUSED_MODE=wave: every wave owns 2 (4) slots and alternates their tree walk with the network on
 * exactly their leaves; C4_FUSED_MODE=block: n_steps rounds of {tree step of the workgroup's 16/32 slots;
 * barrier; network on
 * the emitted leaves, 16 per pass; barrier}.  Either way the games are exactly those that alternating
 * c4_step / c4_net_forward_wave launches play (which launch runs a simulation never changes a result).
 * values_dev float32 [n_slots], priors_dev float32 [n_slots][7] are the hand-off buffers (must persist
 * between calls).  Needs C4_EVAL_EXTERNAL_F32.  Per-slot rows of the statistics are only exact per
 * workgroup after this call (c4_get_stats sums them; the sums are exact). */
int c4_selfplay_steps(c4_engine *e, c4_net *net, float *values_dev, float *priors_dev, int32_t n_steps,
                      void *hip_stream);
/* -- net-vs-net matches (the reference's Match, match.py:15-70; TrainingLoop._match, neural/training.py:176-207) ----
 * An engine created with c4_config.reserved[0] = n_match_nets > 0 (continuous: stop_after_move = 0, games_target = the
 * number of games, no root noise, num_sampling_moves = 0) plays one game per slot between nets 0 .. n_match_nets - 1,
 * each with an evaluation cache of its own (c4_clear_eval_cache clears them all).
 * c4_match_assign: net_o[i] / net_x[i] (host, n <= n_slots entries) = the net that moves o / x in slot i; the other
 * slots have no game.  Call it after c4_reset with the openings; synchronous.
 * c4_match_steps: one launch of c4_match_wave_kernel for net `net_index` -- c4_selfplay_steps' wave-autonomous kernel
 * restricted to the slots where that net is to move (o moves when the root holds an even number of stones).  A slot
 * that chooses its move records it, makes it and waits for a launch of the opponent's net; every other slot passes
 * through unchanged.  The host cycles over the nets until c4_stats.active_slots == 0; every slot plays ONE game and
 * parks, and the games come out of the record ring (c4_drain_games / c4_export_games_dev; game_id = slot).
 * Which launch runs a simulation, and in which order the nets are served, never changes a game: the games are those
 * that alternating c4_step / c4_net_forward searches of the two nets play, position by position.
 * values_dev / priors_dev as c4_selfplay_steps (one pair of buffers for all nets, persisting between the calls).
 * The kernel is the one the net index was configured with (c4_match_configure below); an index that was never
 * configured runs c4_match_wave_kernel with the engine's search config.  c4_match_wave_kernel cannot hold the 64-filter
 * C4_NET_F32X3_WIDE net (C4_ESTATE, as with C4_FUSED_MODE=wave): configure its index with C4_MATCH_KERNEL_SPLIT.
 * c4_match_configure: the player behind net index `net_index` (an addition: C4_ABI_VERSION stays).  The nets of a match
 * need not be alike: a slot's whole search is run by the launches of the net that is to move in it, and between two
 * nets' turns the slot holds a root and nothing else, so every net index may have its own
 *   simulations   1 .. c4_config.simulations (the node pools are sized by the engine's value: create the engine with the
 *                 largest); 0 = the engine's
 *   pb_c_base     >= 1; 0 = the engine's
 *   pb_c_init     finite (the rule of c4_engine_create)
 *   kernel        C4_MATCH_KERNEL_WAVE  c4_match_wave_kernel
 *                 C4_MATCH_KERNEL_SPLIT c4_match_split_kernel: c4_selfplay_steps' split kernel (tree waves + network
 *                                       waves) under the same one-net-per-launch rule; holds every net mode
 * and nets on different kernels meet in one match.  The engine builds the index's score table with the host libm code
 * of c4_engine_create and owns it.  Valid on a match engine while no game is in progress -- after c4_reset, before
 * c4_match_assign -- else C4_ESTATE; a bad value is C4_EINVAL and leaves the engine as it was (reserved must be 0).  The
 * configuration holds until the next c4_match_configure of that index or c4_engine_destroy.  Synchronous. */
#define C4_MATCH_MAX_NETS 16
#define C4_MATCH_KERNEL_WAVE  0
#define C4_MATCH_KERNEL_SPLIT 1
typedef struct {
    int32_t simulations;
    int32_t pb_c_base;
    double pb_c_init;
    int32_t kernel;
    int32_t reserved[3];
} c4_match_player;
int c4_match_assign(c4_engine *e, const int32_t *net_o, const int32_t *net_x, int32_t n);
int c4_match_steps(c4_engine *e, c4_net *net, int32_t net_index, float *values_dev, float *priors_dev, int32_t n_steps,
                   void *hip_stream);
int c4_match_configure(c4_engine *e, int32_t net_index, const c4_match_player *p);
/* -- position queue: search a list of positions of any length on the engine's slots -------------------------------
 * (stands in for a loop of mcts.search(config, board, evaluator), mcts.py:94-121, over a test set or a generation's
 * positions.)  An engine created with c4_config.reserved[1] = 1 (and stop_after_move = 1; any eval_mode) searches N
 * queued positions with its G slots, N of any size: a slot that has chosen its move writes its root read-out into row
 * `index` of a device result table, takes the next index with one atomic add and starts on that position -- inside the
 * kernel, in whichever stepping call is running: c4_step / c4_step_range with any evaluator, c4_run_centre, and
 * c4_selfplay_steps (all three kernels, the 64-filter C4_NET_F32X3_WIDE net in the split kernel included).  The
 * evaluation cache is shared by all positions.  A slot that finds the queue empty parks; the queue is done when
 * c4_stats.active_slots == 0.  Which slot searches a position, and in which launch, never changes its row: the rows are
 * those of one c4_reset / c4_read_roots search per position.  Without a queue the engine is a plain stop-after-move
 * engine.  c4_match_steps has no match to play on it (C4_ESTATE).
 * A row has the fields of c4_root_result, so whatever reads one reads the other; `state` is 0 until the row's search
 * is finished and 2 from then on, and is written after every other field: a row read between launches is either
 * untouched or whole.  `expansions` counts the expand_node calls of this search (the evaluated nodes that were visited
 * again), `simulations` its simulations. */
typedef struct {
    int32_t  state;             /* 0 not searched yet, 2 done */
    int32_t  move;              /* chosen column */
    double   value;             /* child.data.absolute_value of the chosen child (NaN if None) */
    uint32_t root_visits;
    double   root_value_sum;
    uint32_t child_visits[7];
    double   child_value_sum[7];
    int32_t  child_status[7];   /* -2 absent, -1 non-terminal, else C4_RESULT_* */
    double   root_prior[7];     /* normalised (+ noise) prior used at the root */
    double   values_policy[7];  /* tree.py:104-109 */
    uint64_t color0, color1;    /* the position searched */
    int64_t  expansions;
    int64_t  simulations;
} c4_search_result;
/* c4_queue_positions: n >= 1 host positions; c4_queue_positions_dev: the same from DEVICE memory, boards_dev int64
 * [n][2] = {color0, color1} per row (the layout of c4_export_buffers.boards_dev; the engine keeps a copy of its own).
 * Both behave as c4_reset does: counters, game ids and the result table are cleared, slots 0 .. min(G, n) - 1 start on
 * positions 0 .. with game_id = index, the other slots park, the next index handed out is min(G, n); the evaluation
 * cache is kept.  The game id of a search is its index: c4_set_tapes rows are indexed by position and row [i][0] is
 * used (ply 0); the C4_RNG_PHILOX streams are those of (seed, index, 0).  The positions are checked on the device by
 * the rule of c4_reset: a decided or inconsistent one gives C4_EINVAL with the index of the first in the message,
 * nothing is queued and the engine stays as it was.  On an engine without reserved[1]: C4_ESTATE.  Synchronous.
 * c4_reset on a queue engine drops the queue (and its result table). */
int c4_queue_positions(c4_engine *e, const uint64_t *color0, const uint64_t *color1, int64_t n);
int c4_queue_positions_dev(c4_engine *e, const int64_t *boards_dev, int64_t n);
/* rows finished / rows in all.  Synchronous.  No queue: C4_ESTATE (as the three calls below). */
int c4_queue_progress(c4_engine *e, int64_t *n_done, int64_t *n_total);
/* rows [first, first + n) into host memory; a range outside the table: C4_EINVAL.  Synchronous. */
int c4_queue_results(c4_engine *e, c4_search_result *out, int64_t first, int64_t n);
/* the table itself: engine-owned device memory, valid until the next c4_queue_positions* / c4_reset / destroy */
int c4_queue_results_dev(c4_engine *e, const c4_search_result **rows_dev, int64_t *n);
/* The rows as packed float32 device tensors in the layout of the replay window (c4_export_games_dev), one launch on
 * hip_stream (NULL = the engine's), no host synchronisation; any pointer may be NULL:
 *   policy_dev [n][7]        values_policy rounded to float32 (tree.get_values_policy(), training_game.py:14)
 *   visit_policy_dev [n][7]  the children's visit counts over their sum in float64, rounded (tree.py:111-117)
 *   root_values_dev [n]      root_value_sum / root_visits in float64, rounded
 *   move_values_dev [n]      value (NaN for None)
 *   moves_dev uint8 [n]      move
 * A row that is not finished gives zeros, NaN, NaN and 255. */
int c4_queue_export_dev(c4_engine *e, void *hip_stream, float *policy_dev, float *visit_policy_dev, float *root_values_dev,
                        float *move_values_dev, uint8_t *moves_dev);

/* diagnostic build aid: per-phase s_memtime stamps of workgroup 0, [8 waves][16]; needs the
 * environment variable C4_NET_STAMPS=1 when the net is created, else C4_ESTATE. */
int c4_net_debug_stamps(c4_net *net, unsigned long long *out);

/* diagnostic build aid: per-phase s_memtime stamps of the last c4_step launch, [256 workgroups][8]
 * (0 start, 1 slot state loaded, 2 apply done, 3 descent done, 4 before emit, 5 end, 6 depth), or of
 * the last c4_selfplay_steps launch, [128 workgroups][16] (0-7 tree-phase cycles of each wave, 8 tree
 * phase incl. barrier, 9 network phase, 10 steps);
 * needs C4_TREE_STAMPS=1 in the environment when the engine is created, else C4_ESTATE. */
int c4_debug_stamps(c4_engine *e, unsigned long long *out);

/* diagnostic build aid: s_memtime stamps of the last network pass of every wave of workgroups 0..15 inside the last
 * c4_selfplay_steps launch, [16][8][16] (phase order as c4_net_debug_stamps); needs C4_TREE_STAMPS=1, else C4_ESTATE. */
int c4_debug_fused_net_stamps(c4_engine *e, unsigned long long *out);

/* diagnostic build aid (library built with -DC4_SPLIT_PHASES=1; zeros otherwise): the life of the evaluator requests of the last
 * c4_selfplay_steps launch, workgroups 0..127, [128][4] = {posted -> claimed by a network wave, claimed -> answered,
 * answered -> picked up by its tree wave} summed in units of 64 shader cycles, and the number of requests; needs
 * C4_TREE_STAMPS=1, else C4_ESTATE. */
int c4_debug_latency_stamps(c4_engine *e, unsigned long long *out);

/* diagnostic: which fused kernel the last c4_selfplay_steps / c4_match_steps call launched, as the instantiation's name with
 * the template arguments its family has (TS, MODE, TW, QUEUE in that order; MODE is the net's mode 0 fp16 32 filters, 1 f32x3,
 * 2 fp16 64 filters, 3 f32x3w), the run-time slot packing and the grid, e.g.
 *     "c4_selfplay_split_kernel<16,1,3,false> spread=0 grid=3"    "c4_selfplay_wave_kernel<32,2,true> spread=0 grid=2"
 *     "c4_selfplay_kernel<16,false> spread=0 grid=3"              "c4_match_wave_kernel<16,2> spread=0 grid=1"
 *     "c4_match_split_kernel<16,3,4> spread=0 grid=7"             (TS, MODE, TW; a net index configured with C4_MATCH_KERNEL_SPLIT)
 * and "" before the first such launch.  A launch that the runtime refused (the call returned C4_EDEVICE) is not recorded: the
 * name stays that of the last launch that started.  Host bookkeeping only: no device work, no synchronisation.  Returns the length written
 * (without the terminator), or C4_EINVAL for a null argument or a `cap` that cannot hold the name and its terminator (128
 * bytes always can).  The environment variables that choose among the kernels (C4_FUSED_MODE, C4_FUSED_SLOTS, C4_SPLIT_TW)
 * are ignored where they do not apply; this call is how a caller learns what ran.  tests/fused_matrix.py lists every
 * instantiation and how to reach it.  (An addition: C4_ABI_VERSION stays.) */
int c4_debug_last_fused_kernel(c4_engine *e, char *buf, int cap);

/* ---- train step (the reference: ModelWrapper.train, neural/pytorch/model.py:200-240) ----------
 * The convolutions, linear layers, losses and SGD of the train step are stock PyTorch-ROCm; batch normalisation in
 * training mode -- half of a stock step's GPU time at this net's shape -- is the library's own, fused with the residual add
 * and the LeakyReLU that follow it in the reference's net (model.py:20-31, 36-55, 60-117):
 *     y = act(bn(x) + residual),   bn(x) = (x - mean_c) * invstd_c * weight_c + bias_c,   act = LeakyReLU(slope) (1 = none)
 * float32, contiguous [rows][channels][hw] (NCHW, hw = 42).  Batch statistics (mean, biased variance; two passes) come from
 * the first valid_rows rows (the trainer pads the ragged last batch of an epoch, connect4_amd/net.py:_BatchNorm2d);
 * running_mean / running_var (may both be NULL) and *num_batches_tracked (may be NULL) are updated as torch.nn.BatchNorm2d
 * updates them; save_mean / save_invstd [channels] are kept for the backward.  workspace: c4_bn_workspace_floats(rows,
 * channels) floats.  Launches on hip_stream (capturable in a HIP graph); every reduction has a fixed order. */
long long c4_bn_workspace_floats(int rows, int channels);
int c4_bn_train_forward(const float *x_dev, const float *residual_dev, const float *weight_dev, const float *bias_dev,
                        float *running_mean_dev, float *running_var_dev, long long *num_batches_tracked_dev, float *y_dev,
                        float *save_mean_dev, float *save_invstd_dev, float *workspace_dev, int rows, int valid_rows, int channels,
                        int hw, float momentum, float eps, float slope, void *hip_stream);
/* dz = dy * (y > 0 ? 1 : slope); dresidual (may be NULL) = dz; dbias = sum dz; dweight = sum dz * xhat;
 * dx = weight * invstd * (dz - dbias / M - xhat * dweight / M) over the valid rows (M = valid_rows * hw). */
int c4_bn_train_backward(const float *x_dev, const float *y_dev, const float *dy_dev, const float *weight_dev, const float *save_mean_dev,
                         const float *save_invstd_dev, float *dx_dev, float *dresidual_dev, float *dweight_dev, float *dbias_dev,
                         float *workspace_dev, int rows, int valid_rows, int channels, int hw, float slope, void *hip_stream);

/* Weight gradient of the tower's convolutions (model.py:36-55: 3x3, 32 -> 32 filters, padding 1, no bias; the autograd backward of
 * F.conv2d inside ModelWrapper.train, model.py:226): dweight[co][ci][ky][kx] = sum_n sum_yx dy[n][co][y][x] * x[n][ci][y+ky-1][x+kx-1],
 * float32, contiguous NCHW [rows][32][6][7] (other shapes: C4_EINVAL -- the caller keeps PyTorch's own backward for them).  One pass
 * over x and dy on the f32-input MFMA (exact float32 products), per-workgroup partials summed in a fixed order: reproducible.
 * workspace: c4_conv3x3_wrw_workspace_floats() floats.  Launches on hip_stream (capturable). */
long long c4_conv3x3_wrw_workspace_floats(void);
int c4_conv3x3_wrw(const float *x_dev, const float *dy_dev, float *dweight_dev, float *workspace_dev, int rows, int channels, int height, int width,
                   void *hip_stream);

/* ---- value and policy statistics (c4_train.hip; the reference: neural/stats.py) ---------------------------------------
 * ValueStats.update / PriorStats.update (stats.py:53-71, 99-113) on device tensors: what ModelWrapper.train(print_stats=True)
 * feeds per batch (model.py:228-234) and what evaluate / evaluate_value_only accumulate over a labelled set
 * (model.py:180-198, 307-342), without the .cpu() round trip per batch.  Row by row, as the reference:
 *   category of an output  floorf(x * 3.0f) / 2.0f in float32 (stats.py:67-71); a row with label k in {0, 0.5, 1} counts in
 *                          total[2k] and, when its category equals the label, in correct[2k] (an output of exactly 1.0f is
 *                          category 1.5: never correct); any other label counts in n only;
 *   policy                 correct when the first index of the largest output (np.argmax) is among the indices where the
 *                          label row equals its maximum (stats.py:103-113);
 *   losses                 the reference adds batch_mean_loss * len(batch) (stats.py:56, 101) = the sum of the row losses;
 *                          these are accumulated directly: (x - y)^2 per value row, and per policy row the sum over 7 of
 *                          -(y * max(log x, -100) + (1 - y) * max(log(1 - x), -100)) (torch.nn.BCELoss), formed in float64;
 *                          PriorStats.loss = prior_bce_sum / (7 * prior_n);
 *   smallest / largest     min / max of the outputs; +inf / -inf after a reset -- the reference's starting values 1.0 / 0.0
 *                          (stats.py:9-10) are applied by the reader, as min(1.0, .) / max(0.0, .) do there;
 *   non_finite             rows with a NaN / inf value output, a value output or label beyond +-1024 (the net's outputs lie
 *                          in [0, 1]; larger terms would not fit the integer sums), or a policy output outside [0, 1];
 *                          they add nothing to the sums, and whatever else is reported for such a batch is unspecified.
 * Each row's three float64 terms are rounded to a fixed binary grid (2^-36 for the output and the squared error, 2^-32 for
 * the BCE row) and added as integers: the result does not depend on the launch grid, on dispatch order or on how the rows
 * are split over calls, bit for bit, while a sum stays below 2^53 grid units (sum_outputs, value_sq_err_sum: 131,072, i.e.
 * some 260,000 rows at a mean output of 0.5; prior_bce_sum: 2,097,152); beyond that -- an epoch over a large window --
 * the doubles round as float64 sums do: still deterministic for a given sequence of calls, no longer independent of the
 * split.  c4_score_update_dev adds the first valid_rows (0..rows) of `rows` rows to *acc_dev: two
 * launches on hip_stream (workgroup partials into workspace_dev -- c4_score_workspace_bytes(rows) bytes --, then one
 * workgroup adds them up: integers and min / max, in no particular order); allocates nothing, waits for nothing, capturable in a HIP graph.  All pointers are
 * device pointers; x_prior / y_prior float32 [rows][7], both NULL = the value-only form (prior_n stays); rows <= 0, one prior
 * pointer without the other, or valid_rows outside [0, rows]: C4_EINVAL.  Messages: c4_score_last_error().
 * (Additions like these leave C4_ABI_VERSION alone: it changes when an existing struct or signature does.) */
typedef struct {                 /* 112 bytes, all fields naturally aligned */
    int64_t n;                   /* rows seen (ValueStats.n) */
    int64_t total[3], correct[3];/* labels == 0.0 / 0.5 / 1.0, and of those the rows categorised alike (stats.py:62-65) */
    int64_t prior_n, prior_correct;
    int64_t non_finite;
    double  sum_outputs, value_sq_err_sum, prior_bce_sum;   /* average_value, total_loss of ValueStats / PriorStats */
    float   smallest, largest;
} c4_score_acc;
long long c4_score_workspace_bytes(long long rows);
int c4_score_reset_dev(int device, void *hip_stream, c4_score_acc *acc_dev);
int c4_score_update_dev(int device, void *hip_stream, const float *x_value, const float *y_value,
                        const float *x_prior /* [rows][7] or NULL */, const float *y_prior /* or NULL */,
                        long long rows, long long valid_rows, c4_score_acc *acc_dev, void *workspace_dev);
const char *c4_score_last_error(void);

/* -- exact values of late-game positions (c4_solve.hip) ------------------------------------------------------------------ */
/* What the reference's GridSearch(plies >= empty squares) returns for a position (grid_search.py:38-71: no evaluator is
 * reached, so it is the game-theoretic result, faster wins and slower losses preferred), found by alpha-beta instead of
 * exhaustively: the outcome under best play and the age (stone count) at which that play ends the game.  The reference's
 * float64 follows from the two: an o win 1.0 - age / 10000.0, an x win age / 10000.0, a draw 0.5 + 42 / 10000.0.
 * One position per lane, depth first, no transposition table, nothing shared between lanes; node counts are deterministic.
 * Per row:
 *   status     C4_SOLVE_SOLVED    searched to the end: outcome (C4_RESULT_*) and final_age are the answer
 *              C4_SOLVE_TERMINAL  already finished: outcome and final_age are its own; not searched
 *              C4_SOLVE_UNKNOWN   the search would have needed more than node_budget nodes; outcome, final_age -1
 *              C4_SOLVE_TOO_DEEP  more than C4_SOLVE_MAX_EMPTIES empty squares; not searched; outcome, final_age -1
 *              C4_SOLVE_INVALID   the colours overlap or leave the 42 cells, a stone floats, the stone counts differ by other
 *                                 than 0 or 1 with o first, or both sides have four in a row; not searched; -1, -1
 *   nodes      positions entered by the search (the root is one; a position whose mover wins at once is never entered
 *              below the root); 0 for a row that was not searched; exactly node_budget for an UNKNOWN row
 * node_budget: most nodes of one row (0: 2^26).  nodes_per_launch: most nodes a row gets in one kernel launch (0: 2^14); a
 * row over it parks its stack in device memory and the next launch, which carries only unfinished rows, resumes it -- so
 * no launch runs longer than nodes_per_launch nodes of one lane, and neither answers nor node counts depend on it.
 * c4_solve_dev: boards_dev int64 [n][2] packed boards on the device (color0, color1: what c4_export_games_dev writes), the
 * four outputs device arrays of n.  Launches on hip_stream and waits for it between launches (synchronous).  c4_solve: the
 * same from and to host memory.  c4_solve_children_dev: children_dev int64 [n][7][2] = the position after each column,
 * legal_dev int8 [n][7] = 1 where the column is playable; all zero for a finished or invalid row.  One launch, no wait.
 * A null pointer or a negative count: C4_EINVAL.  Messages: c4_solve_last_error(). */
#define C4_SOLVE_MAX_EMPTIES 24
#define C4_SOLVE_SOLVED 0
#define C4_SOLVE_TERMINAL 1
#define C4_SOLVE_UNKNOWN 2
#define C4_SOLVE_TOO_DEEP 3
#define C4_SOLVE_INVALID 4
int c4_solve_dev(int device, void *hip_stream, const int64_t *boards_dev, int64_t n, int64_t node_budget, int64_t nodes_per_launch,
                 int8_t *status_dev, int8_t *outcome_dev, int8_t *final_age_dev, int64_t *nodes_dev);
int c4_solve(int device, const uint64_t *color0, const uint64_t *color1, int64_t n, int64_t node_budget, int64_t nodes_per_launch,
             int8_t *status, int8_t *outcome, int8_t *final_age, int64_t *nodes);
int c4_solve_children_dev(int device, void *hip_stream, const int64_t *boards_dev, int64_t n, int64_t *children_dev, int8_t *legal_dev);
const char *c4_solve_last_error(void);

/* -- positions of any depth: the same search with 42 plies of stack and a shared transposition table (c4_solve.hip) ------ */
/* c4_solve_deep_dev / c4_solve_deep answer like c4_solve_dev / c4_solve for positions with up to
 * C4_SOLVE_DEEP_MAX_EMPTIES = 42 empty squares -- every position: they never answer C4_SOLVE_TOO_DEEP.  Statuses, nodes,
 * node_budget and nodes_per_launch mean what they mean above.
 * table: a handle from c4_solve_table_create, or NULL.  With NULL this is the table-free search: node counts are
 * deterministic and the ones c4_solve_dev has where both answer.  With a table, every lane of every launch of every call
 * probes and stores in the same 2^log2_entries entries of device memory.  An entry is one aligned 64-bit word = the
 * position's full 49-bit key (mover's stones + occupied squares + bottom row: injective), a 7-bit score and whether that
 * score is a lower bound, an upper bound or exact; it is read and written by one 64-bit access, so a reader sees a whole
 * entry, and a hit is a hit on the position itself, never on a hash.  The score is the mover's and depends on the position
 * alone, so an entry holds for every row, launch and call, and the table never has to be cleared for correctness.
 * Answers (status other than UNKNOWN, outcome, final_age) are exact and do not depend on the table's size or contents,
 * on nodes_per_launch or on what else is in the batch.  NODE COUNTS WITH A TABLE ARE NOT DETERMINISTIC: they depend on
 * what other lanes stored first, and so does which rows a tight node_budget leaves UNKNOWN.  Replacement: always.
 * table_hits_dev / table_hits: int64 [n] or NULL -- per row, the probes that returned the stored score or narrowed the
 * window (0 without a table).
 * c4_solve_table_create: log2_entries in 10..30 (8 bytes an entry), else C4_EINVAL; zero-filled, on `device`; the table
 * must be used on the device it was created on (else C4_EINVAL).  c4_solve_table_clear zero-fills on hip_stream and waits for it (a
 * matter of measurement, not of correctness).  Two calls that share a table may run concurrently.
 * c4_solve_table_read copies all 2^log2_entries words to entries_host (n must be that count, else C4_EINVAL; a null argument
 * likewise): it waits for the device first, so it sees every store of every solver call that has returned.  For audits of the
 * table (an entry must be a true bound of its position); no search needs it. */
#define C4_SOLVE_DEEP_MAX_EMPTIES  42
typedef struct c4_solve_table c4_solve_table;
int c4_solve_table_create(int device, int log2_entries, c4_solve_table **out);
int c4_solve_table_destroy(c4_solve_table *table);
int c4_solve_table_clear(c4_solve_table *table, void *hip_stream);
int c4_solve_table_read(c4_solve_table *table, uint64_t *entries_host, int64_t n);
/* The book: one ply solved once (an addition: C4_ABI_VERSION stays).  c4_solve_book_create copies n entry words from host
 * memory -- the table's layout: key in bits 0..48, score + 64 in bits 49..55, kind 1..3 in bits 56..57 -- of positions
 * that all have `age` stones into a read-only image on `device`.  A key is the canonical one of its mirror pair: the
 * smaller of the key and the key with its seven 7-bit column fields reversed; every entry must be a true bound of its
 * position's value -- that, and whether the two sides' stone counts fit the mover, is the caller's to ensure; everything
 * else is checked.  C4_EINVAL: a null argument, n < 0, an age outside 0..41, bits above the kind, a kind of 0, a score
 * outside +-42, a key that is not canonical or whose column fields do not decode to a position with `age` stones, a key
 * that occurs twice.  c4_solve_table_attach_book makes every later call that is given `table` probe the book (NULL: none)
 * wherever it reaches a position of the book's age, root included; a hit counts into table_hits.  The book must live on the
 * table's device (else C4_EINVAL) and outlive the attachment; it is never written, so any number of tables and concurrent
 * calls may share it.  c4_solve_table_create_entryless: a handle without entries -- the table-free search, deterministic
 * node counts -- whose only use is to carry a book; c4_solve_table_clear / _read refuse it.  Answers never depend on a book. */
typedef struct c4_solve_book c4_solve_book;
int c4_solve_book_create(int device, const uint64_t *words, int64_t n, int age, c4_solve_book **out);
int c4_solve_book_destroy(c4_solve_book *book);
int c4_solve_table_attach_book(c4_solve_table *table, const c4_solve_book *book);
int c4_solve_table_create_entryless(int device, c4_solve_table **out);
int c4_solve_deep_dev(int device, void *hip_stream, c4_solve_table *table, const int64_t *boards_dev, int64_t n, int64_t node_budget,
                      int64_t nodes_per_launch, int8_t *status_dev, int8_t *outcome_dev, int8_t *final_age_dev, int64_t *nodes_dev,
                      int64_t *table_hits_dev);
int c4_solve_deep(int device, c4_solve_table *table, const uint64_t *color0, const uint64_t *color1, int64_t n, int64_t node_budget,
                  int64_t nodes_per_launch, int8_t *status, int8_t *outcome, int8_t *final_age, int64_t *nodes, int64_t *table_hits);

/* -- the deep search from a root window per row (c4_solve.hip) ----------------------------------------------------------- */
/* c4_solve_window_dev / c4_solve_window are c4_solve_deep_dev / c4_solve_deep with the root's alpha-beta window given per
 * row: alpha, beta int8 [n] on the mover's score (a game the mover wins at age a scores 43 - a, one the mover loses
 * a - 43, a draw 0), -42 <= alpha < beta <= 42.  Both NULL: the full window (-42, 42) for every row; one NULL, or a bad
 * window in any row: C4_EINVAL, the message names the first bad row, nothing is launched.  The search is fail-hard
 * alpha-beta from that window, and a row that is searched to the end (status C4_SOLVE_SOLVED) answers with
 *   score  int8, the mover's score as the root returns it
 *   bound  int8, that score's kind against the caller's window:
 *            C4_SOLVE_BOUND_EXACT  alpha < score < beta: the position's exact score
 *            C4_SOLVE_BOUND_LOWER  score >= beta: the exact score is at least `score`
 *            C4_SOLVE_BOUND_UPPER  score <= alpha: the exact score is at most `score`
 *          The score of a bound may lie beyond the window (a mover who wins at once returns 42 - age whatever the window
 *          is, a root that is decided without a move returns its value as it is); it is a true bound of its kind always.
 *   outcome, final_age  as c4_solve_deep where bound is exact, else -1.
 * Rows of every other status have score 0, bound C4_SOLVE_BOUND_NONE and the outcome and final_age c4_solve_deep gives
 * them.  Statuses, nodes, table, table_hits, node_budget and nodes_per_launch are c4_solve_deep's; a window never makes a
 * table-free search enter more nodes than a window that contains it.  A table may be shared between windowed and exact
 * calls in any order: its entries are true bounds of their positions whatever window found them.  With (-1, 1) the score
 * is the sign of the outcome for the mover; with (v - 1, v) it says whether the score is at least v. */
#define C4_SOLVE_BOUND_NONE  0
#define C4_SOLVE_BOUND_LOWER  1
#define C4_SOLVE_BOUND_UPPER  2
#define C4_SOLVE_BOUND_EXACT  3
int c4_solve_window_dev(int device, void *hip_stream, c4_solve_table *table, const int64_t *boards_dev, const int8_t *alpha_dev,
                        const int8_t *beta_dev, int64_t n, int64_t node_budget, int64_t nodes_per_launch, int8_t *status_dev,
                        int8_t *score_dev, int8_t *bound_dev, int8_t *outcome_dev, int8_t *final_age_dev, int64_t *nodes_dev,
                        int64_t *table_hits_dev);
int c4_solve_window(int device, c4_solve_table *table, const uint64_t *color0, const uint64_t *color1, const int8_t *alpha,
                    const int8_t *beta, int64_t n, int64_t node_budget, int64_t nodes_per_launch, int8_t *status, int8_t *score,
                    int8_t *bound, int8_t *outcome, int8_t *final_age, int64_t *nodes, int64_t *table_hits);

/* -- the root driver: alpha-beta over a graph of positions (c4_solve.hip) ------------------------------------------------ */
/* c4_solve_graph answers the rows of level 0 of a layered graph from windowed searches of its last level: one hard
 * position spread over many lanes, folded back as intervals, so that an unfinished descendant costs the answer only
 * where the proof needs it.  (An addition: C4_ABI_VERSION stays.)  Every array is in host memory.
 *   color0, color1  uint64 [n_nodes], the levels concatenated, level 0 first
 *   level_start     int64 [n_levels + 1]: level j is the nodes level_start[j] .. level_start[j + 1] - 1; level_start[0] = 0,
 *                   not decreasing; 2 <= n_levels <= C4_SOLVE_GRAPH_MAX_PLIES + 1; the last level has at most 2^20 nodes
 *   child           int32 [n_nodes][7]: the node of the position after each column -- a node of the next level -- or -1;
 *                   every node below level 0 is some node's child, the last level has no children
 *   alpha, beta     int8 [n_0], the windows of level 0 as c4_solve_window takes them, or both NULL
 * A malformed graph or window is C4_EINVAL, the message names the first offender, and no device is touched.
 * Windows are static: a child of a node with (a, b) has (-b, -a), a node with several parents the union.  The last level
 * is searched by c4_solve_window's kernels from those windows, with `table` (or NULL), node_budget and nodes_per_launch as
 * there.  A node that has no child answers for itself: a finished position with its score, anything else not at all.
 * Every node has an interval [lo, hi] that contains its exact score for its mover: [s, s] for an exact answer, [s, 42]
 * for a lower bound, [-42, s] for an upper bound, [-42, 42] without an answer; above the leaves lo = max over children of
 * -hi, hi = max over children of -lo.  A row of level 0 with window (a, b) is answered once lo == hi (the score, its kind
 * against the window), lo >= b (a lower bound lo) or hi <= a (an upper bound hi).  After k_solve_init and after every
 * launch the intervals are folded and the leaves that no unanswered row can still use are dropped: they leave the search.
 *   status .. table_hits  [n_0], as c4_solve_window answers a row: SOLVED where the row is decided, UNKNOWN where it is not,
 *                         TERMINAL / INVALID for a row that answers for itself; nodes and table_hits are the sums over
 *                         the row's distinct nodes of the last level
 *   node_lo, node_hi int8, node_state int8 (C4_SOLVE_NODE_*), node_nodes, node_table_hits int64 [n_nodes]: each may be
 *                         NULL; nodes and table_hits are zero above the last level
 * Table-free, every output is a function of the inputs: connect4_amd/solver.py drive_graph_host computes the same. */
#define C4_SOLVE_GRAPH_MAX_PLIES  8
#define C4_SOLVE_NODE_INTERIOR     0   /* has children: its interval is folded from theirs */
#define C4_SOLVE_NODE_SELF         1   /* no child above the last level, or a finished or invalid position in it */
#define C4_SOLVE_NODE_ANSWERED     2   /* a searched node whose root returned */
#define C4_SOLVE_NODE_OVER_BUDGET  3   /* a searched node that reached node_budget */
#define C4_SOLVE_NODE_DROPPED      4   /* a searched node taken out of the search: no undecided row needed it */
#define C4_SOLVE_NODE_PENDING      5   /* between launches only: never reported */
int c4_solve_graph(int device, c4_solve_table *table, const uint64_t *color0, const uint64_t *color1, const int64_t *level_start,
                   int n_levels, const int32_t *child, const int8_t *alpha, const int8_t *beta, int64_t node_budget,
                   int64_t nodes_per_launch, int8_t *status, int8_t *score, int8_t *bound, int8_t *outcome, int8_t *final_age,
                   int64_t *nodes, int64_t *table_hits, int8_t *node_lo, int8_t *node_hi, int8_t *node_state, int64_t *node_nodes,
                   int64_t *node_table_hits);

/* -- the review of finished games against exact play (c4_solve.hip) ------------------------------------------------------ */
/* A batch of finished games in the layout c4_export_games_dev writes: a game is a run of consecutive rows with one
 * game_index, plies ascending; row i + 1 of a game is the position after moves[i] on row i, and after the last row's move the
 * game is over with results[g] (C4_RESULT_*, or -1: the game carries no result).  A position is late when it is undecided and
 * has at most max_empties empty squares.  The three calls are the book-keeping around one c4_solve_window_dev call on the
 * distinct late rows with alpha = -1, beta = +1, which the caller makes between the first and the second.  All pointers are
 * device pointers; each call is one launch (the fold: two) on hip_stream and waits for nothing.  Every kernel is one lane a
 * position and straight-line: no LDS, no scratch, no lane waits for another; the counters are integer atomics, so every
 * output is a function of the inputs.  A null pointer that is not marked optional, a negative count, max_empties outside
 * 0..42: C4_EINVAL.  Messages: c4_solve_last_error().  (Additions: C4_ABI_VERSION stays.)
 *
 * c4_review_select_dev: late_dev uint8 [n] = 1 for a late row, 0 for every other -- one with more empty squares, a finished
 * position, a row that is no position (C4_SOLVE_INVALID); the fold counts the last two as chain errors.
 *
 * c4_review_outcomes_dev: the answers of the m searched rows (searched_status_dev, searched_score_dev int8 [m] and, optional
 * together with nodes_dev, searched_nodes_dev int64 [m]: c4_solve_window_dev's status, score and nodes) spread over the
 * positions through row_of_dev int64 [n], the searched row of every late position (read for late rows only).  status_dev
 * int8 [n]: the searched row's C4_SOLVE_SOLVED or C4_SOLVE_UNKNOWN (also for an index outside 0..m-1), C4_SOLVE_TOO_DEEP for
 * a row that is not late -- here: more empty squares than asked for.  outcome_dev int8 [n]: C4_RESULT_* under best play,
 * absolute, from the sign of the mover's score and the parity of the age; -1 unless the status is C4_SOLVE_SOLVED.
 * nodes_dev int64 [n] (optional): the searched row's count, 0 for a row that is not late.
 *
 * c4_review_fold_dev: the rule.  With next[i] = outcome[i + 1] if row i + 1 belongs to the same game, else results[g]:
 *   kept_dev           int8 [n]: 1 if outcome[i] and next[i] are both known and equal, 0 if both are known and differ -- a
 *                      blunder of the side to move at i --, -1 otherwise and for every row that is not late
 *   target_agrees_dev  int8 [n]: 1 if the row is late, outcome[i] is known and equals results[g]; else 0
 *   by_ply_dev         int64 [42][7], indexed by the position's age, columns C4_REVIEW_*: late rows, rows with a known outcome,
 *                      rows with a known kept, kept, blunders (kept + blunders = kept_known), target_agrees, and
 *                      contradictions: blunders that change the outcome in the mover's FAVOUR, which best play rules out --
 *                      a tripwire for the solver, zero unless it is wrong
 *   per_game_dev       int32 [n_games][4], columns C4_REVIEW_GAME_*: late rows, rows with a known kept, blunders, and the age
 *                      of the last blunder (-1: none)
 *   exact_targets_dev  float32 [n], optional (then targets_in_dev float32 [n] is read): 0.5f * outcome[i] for a late row with
 *                      a known outcome -- Result's value: 1.0 o win, 0.5 draw, 0.0 x win --, targets_in_dev[i] for every other
 *   exact_priors_dev   float32 [n][7], optional (then keep_dev uint8 [n][7], the moves that keep the outcome, keep_known_dev
 *                      uint8 [n], 1 where that mask is known, and policy_in_dev float32 [n][7] are read): uniform over the
 *                      keeping moves of a late row whose mask is known and not empty, policy_in_dev[i] for every other
 * The chain is checked, not trusted: a row must be an undecided position, its game_index within 0..n_games-1, results[g]
 * within -1..2, its move a playable column, and the position after the move (c4_board.h make_move) must equal row i + 1
 * exactly or, behind a game's last row, be finished -- with the result results[g] where that is not -1.  Rows that fail
 * are counted in chain_errors_dev int32 [1] and take no part in the aggregates; first_error_dev int32 [1] (optional) is the
 * smallest such row, INT32_MAX if there is none.  A batch with chain errors has no answer: the caller discards the
 * outputs.  The fold zeroes its aggregates first (one more launch); n and 4 * n_games must fit 32 bits. */
#define C4_REVIEW_PLIES 42
#define C4_REVIEW_COLUMNS 7
#define C4_REVIEW_LATE 0
#define C4_REVIEW_OUTCOME_KNOWN 1
#define C4_REVIEW_KEPT_KNOWN 2
#define C4_REVIEW_KEPT 3
#define C4_REVIEW_BLUNDERS 4
#define C4_REVIEW_TARGET_AGREES 5
#define C4_REVIEW_CONTRADICTIONS 6
#define C4_REVIEW_GAME_COLUMNS 4
#define C4_REVIEW_GAME_LATE 0
#define C4_REVIEW_GAME_KEPT_KNOWN 1
#define C4_REVIEW_GAME_BLUNDERS 2
#define C4_REVIEW_GAME_LAST_BLUNDER_AGE 3
int c4_review_select_dev(int device, void *hip_stream, const int64_t *boards_dev, int64_t n, int max_empties, uint8_t *late_dev);
int c4_review_outcomes_dev(int device, void *hip_stream, const int64_t *boards_dev, const uint8_t *late_dev, const int64_t *row_of_dev, int64_t n,
                           const int8_t *searched_status_dev, const int8_t *searched_score_dev, const int64_t *searched_nodes_dev, int64_t m,
                           int8_t *status_dev, int8_t *outcome_dev, int64_t *nodes_dev);
int c4_review_fold_dev(int device, void *hip_stream, const int64_t *boards_dev, const uint8_t *moves_dev, const int32_t *game_index_dev,
                       const int8_t *results_dev, int64_t n, int64_t n_games, const int8_t *outcome_dev, const uint8_t *late_dev,
                       const float *targets_in_dev, int8_t *kept_dev, int8_t *target_agrees_dev, int64_t *by_ply_dev, int32_t *per_game_dev,
                       int32_t *chain_errors_dev, int32_t *first_error_dev, float *exact_targets_dev, const uint8_t *keep_dev,
                       const uint8_t *keep_known_dev, const float *policy_in_dev, float *exact_priors_dev);

/* -- exact values over a leaf batch: the solver laid over the net (c4_solve.hip) ------------------------------------------- */
/* The rows are a leaf batch in the layout of c4_leaf_buffers / c4_net_forward: color0_dev, color1_dev uint64 [n], values_dev
 * float32 [n] as the network has just written them.  A row is late when it is an undecided position (C4_SOLVE_SOLVED before
 * any search) with at most max_empties empty squares.  Every late row is searched table-free from the window (-1, +1) for at
 * most node_budget nodes -- c4_solve_window_dev's rule: the root is node 1, a row that would need a node beyond the budget
 * has no answer, and the node count is c4_solve_window_dev's table-free count -- and an answered row's values_dev[i] becomes
 * 1.0f (o wins), 0.5f (draw) or 0.0f (x wins): the evaluator's convention, from o's side whoever moves.  Every other row
 * keeps its values_dev[i] bit for bit: more empty squares, a finished position, a row that is no position (a zero or stale
 * leaf row), a late row over budget.  Nothing else is written; priors are not an argument.
 * counters_dev int64 [4] (optional), columns C4_EXACT_LEAVES_*: the call ADDS rows overridden, late rows over budget, nodes
 * entered and late rows (overridden + over budget) to what is there -- integer atomics, reduced over a wave first, so the
 * sums are exact; the caller clears them.
 * One launch on hip_stream; no allocation, no copy, no wait: the call can be captured in a HIP graph.  max_empties is
 * 0..C4_SOLVE_MAX_EMPTIES, and 0 launches nothing; node_budget is at least 1 (above 2^40 it is 2^40).  n < 0, a value outside
 * these ranges or a null color0_dev, color1_dev or values_dev: C4_EINVAL.  Messages: c4_solve_last_error().
 * (An addition: C4_ABI_VERSION stays.) */
#define C4_EXACT_LEAVES_OVERRIDDEN 0
#define C4_EXACT_LEAVES_OVER_BUDGET 1
#define C4_EXACT_LEAVES_NODES 2
#define C4_EXACT_LEAVES_LATE 3
int c4_exact_leaves_dev(int device, void *hip_stream, const uint64_t *color0_dev, const uint64_t *color1_dev, int32_t n, int max_empties,
                        int64_t node_budget, float *values_dev, int64_t *counters_dev);

int c4_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
