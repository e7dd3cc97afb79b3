// c4_solve.hip -- exact values of positions by alpha-beta on gfx950, behind c4_solve / c4_solve_deep / c4_solve_window, their
// _dev twins, the c4_solve_table_* calls, c4_solve_children_dev, the c4_review_*_dev calls and c4_exact_leaves_dev of
// include/c4_engine.h.
//
// The answer is the one the reference's GridSearch(plies >= empty squares) computes exhaustively
// (oinkoink/grid_search.py:38-71: no evaluator is reached, the terminal scoring prefers faster wins and
// slower losses): the game-theoretic outcome and the age (stone count) at which best play ends the game.
//
// Score.  A game that o wins at age a scores 43 - a, one that x wins at age a scores a - 43, a draw 0 --
// an integer that is strictly monotone in the reference's float64 (1 - a/10000, a/10000, 0.5 + 42/10000).
// The search keeps it from the side to move (negamax); outcome and final age leave the kernel, the float64
// is formed from them by the caller as the reference writes it.
//
// Search.  One position per lane, iterative depth-first alpha-beta:
//   * a node is entered only when its mover cannot win at once (the root is checked, below the root the
//     move list guarantees it), so an immediate win never costs a node;
//   * the move list holds the non-losing moves only: a forced block if the opponent threatens, no move
//     under a square the opponent wins on; an empty list is a loss two plies on;
//   * the window is clipped to what is still possible (no win before age + 3, no loss before age + 4);
//   * moves are ordered by the number of winning squares they create, ties centre first.
// Pruning and ordering change the node count, never the value.
//
// Stack.  A frame is two 32-bit words (the ordered rest of the move list with the move played; alpha and
// beta, and with a table the alpha the node's moves were entered with).  The top frame lives in registers, the
// frames below in LDS laid out [ply][lane] -- a lane's column, so no lane reads another's and there is no
// barrier.  Boards are not stacked: the move played is undone on the way back.
//
// Termination.  Every loop is bounded: a launch gives each lane a quota of nodes; a lane that has used
// it parks -- its registers go into one word a row (pack_parked) and its frames into global memory -- and
// stops.  The host relaunches the unfinished positions, compacted into a dense index list, until all are done
// or a position's total has reached its budget (status UNKNOWN).  No lane waits for another lane, wave or
// workgroup.
//
// One search, three options.  k_solve_init classifies every row and enters its root; k_solve_search<MAXP, T> is the
// kernel that unparks, runs the quota (run_lane) and answers or parks again.  What a call chooses:
//   * the frame depth MAXP.  k_solve_search<MAX_PLY, NoTable> (c4_solve, c4_solve_dev) has 24 plies of frames: 2 x 24 x 64
//     x 4 B = 12 KiB of LDS a one-wave workgroup, thirteen workgroups a CU, rows with more empty squares are TOO_DEEP.
//     k_solve_search<DEEP_MAX_PLY, TableRef> (c4_solve_deep*, c4_solve_window*) has 42: 21 KiB, all frames still in LDS,
//     seven workgroups a CU, every position.  These two are the only instantiations; k_exact_leaves (c4_exact_leaves_dev) runs
//     the first one's search, run_lane<MAX_PLY, LdsStack, NoTable>, without parking.
//   * the table T.  NoTable compiles no table, hit-count or window code.  A TableRef is a transposition table in device
//     memory that every lane of every launch of every call shares, or none (e == nullptr: the table-free deep search).
//   * the root window (c4_solve_window*, a Window of per-row arrays): alpha < beta on the mover's score instead of the
//     whole range.
// Table-free, neither the frame depth nor the launch quota changes a node count: it is solver._Search's.
//
// The table.
//   * An entry is one aligned 64-bit word: the position's key in bits 0..48 (mover's stones + occupied + BOTTOM, which
//     is injective), the score + 64 in bits 49..55, the bound's kind in bits 56..57 (lower, upper, exact; 0: empty).
//     It is read by one relaxed 64-bit atomic load and written by one relaxed 64-bit atomic store: a reader sees a
//     whole entry, old or new, and a hit compares the whole key, so it is a hit on this very position.
//   * The score is the mover's 43 - final age form and is a true bound of the position's value whatever window it was
//     found with, so an entry holds for every row, launch and call, windowed or not; a stale entry does not exist.
//   * A node probes after enter_node says interior: an entry that closes the window is returned, another narrows
//     it.  A node stores when it closes (its moves are used up, or one cuts off), against the window its moves were
//     searched with: the frame keeps that alpha in bits 16..23 of its alpha / beta word.  Always replace.  Nodes with
//     fewer than TT_MIN_EMPTIES empty squares neither probe nor store.
//   * Probe and store are straight-line code: the termination argument above holds word for word -- no lane waits for
//     another, the only atomics are that load and that store.
//   * Answers are exact and do not depend on the table (alpha-beta returns the same root value for every sound set of
//     bounds).  NODE COUNTS WITH A TABLE ARE NOT DETERMINISTIC: they depend on what other lanes stored first.
//
// The book (c4_solve_book_*, carried by the TableRef).
//   * A read-only set of table-format words, all of positions with one stone count: solved once, kept in a file, and
//     probed where the search reaches that ply -- in run_lane after enter_node says interior and in k_solve_init for the
//     root, exactly where the table is probed, but whatever TT_MIN_EMPTIES says and whether or not there is a table
//     (e == nullptr).  NoTable compiles none of it.
//   * One entry serves a position and its mirror image: the key stored and looked up is the smaller of the key and the
//     key with its seven column fields reversed (tt_mirror_key).
//   * The device image is open-addressed with linear probing, a power-of-two capacity of at least twice the entries;
//     the host lays it out and records the longest probe sequence, and book_probe's loop runs at most that many steps:
//     plain loads, no atomics, no writes, no LDS.  The termination argument above holds word for word: every loop is
//     bounded, no lane waits for another.
//   * The book is probed first and feeds the same Probe into the same code.  An entry that closes the node returns and
//     the table is not probed; one that narrows the window hands the narrowed window to the table probe.  A node the book
//     closes stores nothing; a node it narrowed closes against the alpha its moves were entered with, like any node.
//   * A book hit (returned or narrowed) counts into the row's table_hits like a table hit.
//   * Every entry is a true bound of its position's value, so answers do not depend on the book; node counts do, and
//     table-free they stay deterministic: solver._Search with a HostBook enters the same nodes.
//
// The root window.  Fail-hard alpha-beta from the caller's window, the search every node below a root already is.  A
// row answers with the score its root returns and that score's kind against the caller's window (C4_SOLVE_BOUND_*):
// exact inside it, else a lower bound at or above beta or an upper bound at or below alpha.  The root's table probe and
// enter_node may narrow the window the moves are searched with -- the root's own entry is stored against that one,
// like any node's -- but the kind is judged against the window the caller gave, which stays in the caller's arrays while
// the row is parked.  A call without a window enters the nodes of the full window (-42, 42).
//
// The root driver (c4_solve_graph).  A layered graph of positions, built by the caller: its last level is searched by the
// two kernels above, unchanged, from static windows -- a child of (a, b) has (-b, -a), a node with several parents the
// union -- and between the launches a few one-lane-a-node kernels turn the answers into intervals, fold them up
// (lo = max -hi_c, hi = max -lo_c), answer the rows of level 0 whose interval decides their window, mark down what an
// undecided row can still use, and clear the unfinished flag of every row that is not marked: it is dropped instead of
// running out its budget.  Every interval contains the node's exact score whatever was dropped or left unknown, so every
// answer is a true bound.  The termination argument holds word for word: the new kernels are straight-line, no lane
// waits for another, and the only new atomics are atomicMin / atomicMax on the 32-bit words of a child's window.  They use
// no LDS and a handful of VGPRs.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/c4_engine.h"
#include "c4_board.h"

using namespace c4;

namespace {

constexpr int MAX_EMPTIES = C4_SOLVE_MAX_EMPTIES;
constexpr int MAX_PLY = MAX_EMPTIES;            // frames of one lane (a node with one empty square is a leaf)
constexpr int DEEP_MAX_EMPTIES = C4_SOLVE_DEEP_MAX_EMPTIES;
constexpr int DEEP_MAX_PLY = DEEP_MAX_EMPTIES;  // k_solve_search<DEEP_MAX_PLY, TableRef>'s frames
constexpr int TT_MIN_EMPTIES = 6;               // nodes nearer the end are cheaper to search than to look up
constexpr int TT_MIN_LOG2 = 10, TT_MAX_LOG2 = 30;
constexpr int BLOCK = 64;                       // one wave per workgroup: 2 x MAXP x 64 x 4 B of LDS
constexpr uint64_t BOARD = BOTTOM * COLMASK;    // the 42 cells
constexpr int SCORE_MAX = 42;                   // beyond every score (the fastest win, at age 7, scores 36)
constexpr int64_t DEFAULT_BUDGET = (int64_t)1 << 26;
constexpr int64_t DEFAULT_PER_LAUNCH = (int64_t)1 << 14;
constexpr int64_t CHUNK_ROWS = (int64_t)1 << 20;   // rows searched per pass: bounds the work memory (224 B a row)

// the empty squares on which `p` completes four in a row, given the occupied squares `occ`
C4_HD uint64_t winning_squares(uint64_t p, uint64_t occ)
{
    uint64_t r = (p << 1) & (p << 2) & (p << 3);    // vertical
    uint64_t q = (p << 7) & (p << 14);              // horizontal
    r |= q & (p << 21);
    r |= q & (p >> 7);
    q = (p >> 7) & (p >> 14);
    r |= q & (p << 7);
    r |= q & (p >> 21);
    q = (p << 6) & (p << 12);                       // diagonal '\'
    r |= q & (p << 18);
    r |= q & (p >> 6);
    q = (p >> 6) & (p >> 12);
    r |= q & (p << 6);
    r |= q & (p >> 18);
    q = (p << 8) & (p << 16);                       // diagonal '/'
    r |= q & (p << 24);
    r |= q & (p >> 8);
    q = (p >> 8) & (p >> 16);
    r |= q & (p << 8);
    r |= q & (p >> 24);
    return r & (BOARD ^ occ);
}

// Move list: up to 7 columns of 3 bits each, next move lowest; the number left at bits 24..26; the move
// played from this node (to undo on the way back) at bits 27..29.
C4_HD int moves_left(uint32_t m) { return (int)((m >> 24) & 7); }

// `cand` has at most one square per column.  More winning squares first, ties centre first (3,2,4,1,5,0,6).
C4_HD uint32_t order_moves(uint64_t mine, uint64_t occ, uint64_t cand)
{
    int key[WIDTH];
#pragma unroll
    for (int c = 0; c < WIDTH; ++c) {
        const uint64_t bit = cand & (COLMASK << (H1 * c));
        const int prio = c == 3 ? 6 : c == 2 ? 5 : c == 4 ? 4 : c == 1 ? 3 : c == 5 ? 2 : c == 0 ? 1 : 0;
        key[c] = bit ? popc64(winning_squares(mine | bit, occ | bit)) * 8 + prio + 1 : 0;
    }
    uint32_t list = 0;
    int n = 0;
#pragma unroll
    for (int c = 0; c < WIDTH; ++c) {
        int rank = 0;                  // keys of candidates are distinct: ranks 0..n-1
#pragma unroll
        for (int j = 0; j < WIDTH; ++j) rank += (j != c && key[j] > key[c]) ? 1 : 0;
        if (key[c]) {
            list |= (uint32_t)c << (3 * rank);
            ++n;
        }
    }
    return list | ((uint32_t)n << 24);
}

// A node whose mover (`mine`, `age` stones on the board) cannot win at once.  Returns true for a leaf
// (`value` is its score for the mover), false for an interior node: alpha and beta are clipped to the
// scores still possible and `moves` is its ordered move list.
C4_HD bool enter_node(uint64_t mine, uint64_t theirs, int age, int &alpha, int &beta, uint32_t &moves, int &value)
{
    if (age == CELLS - 1) { value = 0; return true; }       // the last square, and it does not win
    const uint64_t occ = mine | theirs;
    uint64_t possible = (occ + BOTTOM) & BOARD;
    const uint64_t opp_win = winning_squares(theirs, occ);
    const uint64_t forced = possible & opp_win;
    if (forced) {
        if (forced & (forced - 1)) { value = age - 41; return true; }   // two threats: lost at age + 2
        possible = forced;
    }
    possible &= ~(opp_win >> 1);
    if (!possible) { value = age - 41; return true; }
    const int lo = age + 4 <= CELLS ? age - 39 : 0;     // no loss before age + 4
    const int hi = age + 3 <= CELLS ? 40 - age : 0;     // no win before age + 3
    if (beta > hi) {
        beta = hi;
        if (alpha >= beta) { value = beta; return true; }
    }
    if (alpha < lo) {
        alpha = lo;
        if (alpha >= beta) { value = alpha; return true; }
    }
    if ((possible & (possible - 1)) == 0)       // one move (a forced block, mostly): nothing to order
        moves = (uint32_t)(__builtin_ctzll(possible) / H1) | (1u << 24);
    else
        moves = order_moves(mine, occ, possible);
    return false;
}

struct Lane {
    uint64_t c0, c1;
    uint32_t moves;
    int d, alpha, beta, ret;
    int alpha0 = 0;     // with a table: the alpha the node's moves were entered with
    int hits = 0;       // with a table: probes that returned or narrowed
    bool pending;       // the node at depth d has returned `ret`
    bool done;          // the root has returned
};

C4_HD uint32_t pack_ab(int alpha, int beta) { return (uint32_t)(alpha + 64) | ((uint32_t)(beta + 64) << 8); }

// -- the transposition table ------------------------------------------------------------------------------------------
constexpr uint64_t TT_KEY_MASK = (1ULL << 49) - 1;
constexpr int TT_LOWER = 1, TT_UPPER = 2, TT_EXACT = 3;

struct NoTable {        // k_solve_search<MAX_PLY, NoTable>: no table, hit-count or window code is compiled
    static constexpr bool compiled = false;
};

struct TableRef {       // k_solve_search<DEEP_MAX_PLY, TableRef>: e == nullptr is the table-free search
    static constexpr bool compiled = true;
    uint64_t *e;
    int shift;          // 64 - log2(entries)
    // the book (c4_solve_book): a read-only open-addressed image of table-format words, all of positions with book_age
    // stones; book == nullptr: none.  Kernel arguments, so uniform.
    const uint64_t *book;
    uint32_t book_mask; // capacity - 1, the capacity a power of two
    int book_age;
    int book_steps;     // the longest probe sequence of any entry: what bounds book_probe's loop
};

// The parked word: the top frame of a lane that has stopped at its quota, Work::misc[row].  alpha | beta << 8 | third << 16
// | d << 24 | pending << 30, the scores + 64.  The third field is what the lane needs of ret and alpha0, which are never
// both live: ret if the node at depth d has returned (pending) or there is no table code (T = NoTable), else the alpha0
// of the top frame -- a pending lane closes no node with the alpha0 it had, so unpark_lane gives it alpha.
C4_HD uint32_t pack_parked(int alpha, int beta, int third, int d, int pending)
{
    return pack_ab(alpha, beta) | ((uint32_t)(third + 64) << 16) | ((uint32_t)d << 24) | ((uint32_t)pending << 30);
}

template <class T>
C4_HD uint32_t park_lane(const Lane &L)
{
    int third = L.ret;
    if constexpr (T::compiled) third = L.pending ? L.ret : L.alpha0;
    return pack_parked(L.alpha, L.beta, third, L.d, L.pending ? 1 : 0);
}

template <class T>
C4_HD void unpark_lane(uint32_t w, Lane &L)
{
    L.alpha = (int)(w & 0xff) - 64;
    L.beta = (int)((w >> 8) & 0xff) - 64;
    L.d = (int)((w >> 24) & 0x3f);
    L.pending = ((w >> 30) & 1) != 0;
    const int third = (int)((w >> 16) & 0xff) - 64;
    if constexpr (T::compiled) {
        L.ret = L.pending ? third : 0;
        L.alpha0 = L.pending ? L.alpha : third;
    } else
        L.ret = third;
    L.done = false;
}

C4_HD uint64_t tt_key(uint64_t mine, uint64_t occ) { return mine + occ + BOTTOM; }
C4_HD bool tt_covers(const TableRef t, int age) { return t.e != nullptr && CELLS - age >= TT_MIN_EMPTIES; }
C4_HD size_t tt_slot(const TableRef t, uint64_t key) { return (size_t)((key * 0x9E3779B97F4A7C15ULL) >> t.shift); }

// hit 0: nothing known; 1: the entry narrowed alpha or beta; 2: the entry closes the window, `value` is what the node
// returns.  By value and branch-free: a store through a selected reference would put the window into scratch.
struct Probe {
    int hit, alpha, beta, value;
};

// what the entry word `w` says about the position `key` under the window (alpha, beta)
C4_HD Probe probe_word(uint64_t w, uint64_t key, int alpha, int beta)
{
    const bool match = (w & TT_KEY_MASK) == key;
    const int s = (int)((w >> 49) & 0x7f) - 64, kind = (int)((w >> 56) & 3);
    const bool closes = kind == TT_EXACT || (kind == TT_LOWER && s >= beta) || (kind == TT_UPPER && s <= alpha);
    const bool up = kind == TT_LOWER && s > alpha, down = kind == TT_UPPER && s < beta;
    Probe p;
    p.hit = !match ? 0 : closes ? 2 : (up || down) ? 1 : 0;
    p.alpha = p.hit == 1 && up ? s : alpha;
    p.beta = p.hit == 1 && down ? s : beta;
    p.value = s;
    return p;
}

__device__ __forceinline__ Probe tt_probe(const TableRef t, uint64_t key, int alpha, int beta)
{
    return probe_word(__hip_atomic_load(t.e + tt_slot(t, key), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), key, alpha, beta);
}

// The book.  No 7-bit column field of a key carries into the next (a column of height h holds 2^h + the mover's stones in
// it, at most 127), so the key of the mirror image is the key with its seven fields reversed, and the book stores, and a
// probe looks up, the smaller of the two: no board is mirrored.
C4_HD uint64_t tt_mirror_key(uint64_t k)
{
    constexpr uint64_t F = (1ULL << H1) - 1;
    return ((k & F) << (6 * H1)) | ((k >> (6 * H1)) & F) | ((k & (F << H1)) << (4 * H1)) | ((k >> (4 * H1)) & (F << H1)) |
           ((k & (F << (2 * H1))) << (2 * H1)) | ((k >> (2 * H1)) & (F << (2 * H1))) | (k & (F << (3 * H1)));
}
C4_HD uint64_t book_key(uint64_t key) { const uint64_t m = tt_mirror_key(key); return m < key ? m : key; }
C4_HD uint32_t book_home(uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ULL) >> 32); }
C4_HD bool book_covers(const TableRef t, int age) { return t.book != nullptr && age == t.book_age; }

// Linear probing from the key's home slot, plain loads: the loop ends at the key, at an empty word or after book_steps
// slots -- the host laid no entry further from its home -- so it is bounded by a kernel argument.
__device__ __forceinline__ Probe book_probe(const TableRef t, uint64_t key, int alpha, int beta)
{
    const uint64_t k = book_key(key);
    const uint32_t home = book_home(k);
    uint64_t w = 0;
    for (int i = 0; i < t.book_steps; ++i) {
        const uint64_t x = t.book[(home + (uint32_t)i) & t.book_mask];
        if ((x & TT_KEY_MASK) == k) w = x;
        if ((x & TT_KEY_MASK) == k || x == 0) break;
    }
    return probe_word(w, k, alpha, beta);
}

__device__ __forceinline__ void tt_store(const TableRef t, uint64_t key, int score, int kind)
{
    const uint64_t w = key | ((uint64_t)(score + 64) << 49) | ((uint64_t)kind << 56);
    __hip_atomic_store(t.e + tt_slot(t, key), w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the node the lane stands at closes with L.ret
template <class T>
__device__ __forceinline__ void tt_close(const T tt, const Lane &L, int kind)
{
    if constexpr (T::compiled) {
        const uint64_t occ = L.c0 | L.c1;
        const int age = popc64(occ);
        if (tt_covers(tt, age)) tt_store(tt, tt_key((age & 1) ? L.c1 : L.c0, occ), L.ret, kind);
    }
}

// The status of a row before any search (c4_engine.h C4_SOLVE_*; SOLVED here means: to be searched).  A
// finished position carries its own outcome and age.
C4_HD int classify(uint64_t c0, uint64_t c1, int &outcome, int &final_age, int max_empties = MAX_EMPTIES)
{
    const uint64_t occ = c0 | c1;
    const int n0 = popc64(c0), n1 = popc64(c1);
    outcome = -1;
    final_age = -1;
    if ((c0 & c1) || (occ & ~BOARD) || (occ & (occ + BOTTOM)) || n0 - n1 < 0 || n0 - n1 > 1 || (wins(c0) && wins(c1)))
        return C4_SOLVE_INVALID;
    const uint32_t st = position_status(c0, c1);
    if (st != ST_FRESH) {
        outcome = (int)st - (int)ST_XWIN;
        final_age = n0 + n1;
        return C4_SOLVE_TERMINAL;
    }
    if (CELLS - (n0 + n1) > max_empties) return C4_SOLVE_TOO_DEEP;
    return C4_SOLVE_SOLVED;
}

C4_HD void root_answer(int age, int score, int &outcome, int &final_age)
{
    const int abs_score = (age & 1) ? -score : score;       // o moves at even ages
    outcome = abs_score > 0 ? C4_RESULT_OWIN : abs_score < 0 ? C4_RESULT_XWIN : C4_RESULT_DRAW;
    final_age = abs_score > 0 ? 43 - abs_score : abs_score < 0 ? 43 + abs_score : CELLS;
}

// alpha, beta: the caller's window on the mover's score (the full range for every search but a windowed one)
C4_HD void enter_root(uint64_t c0, uint64_t c1, Lane &L, int alpha = -SCORE_MAX, int beta = SCORE_MAX)
{
    const uint64_t occ = c0 | c1;
    const int age = popc64(occ);
    const uint64_t mine = (age & 1) ? c1 : c0, theirs = (age & 1) ? c0 : c1;
    L.c0 = c0;
    L.c1 = c1;
    L.d = 0;
    L.moves = 0;
    L.alpha = alpha;
    L.beta = beta;
    L.ret = 0;
    L.pending = false;
    L.done = false;
    if (winning_squares(mine, occ) & (occ + BOTTOM)) {       // the mover wins at once
        L.ret = 42 - age;
        L.done = true;
        return;
    }
    int value = 0;
    if (enter_node(mine, theirs, age, L.alpha, L.beta, L.moves, value)) {
        L.ret = value;
        L.done = true;
    }
}

// Run lane L for at most `quota` more nodes.  S: the frames below the top one, S.moves(p) / S.ab(p) for ply p.
// Returns the nodes entered.  Every iteration pops a frame, closes a node or enters one, so 3 * quota + 64
// iterations cover the quota and the unwinding of a full stack.  MAXP: the frames S holds.  tt: NoTable, or a TableRef
// (probe on entering an interior node, store on closing one; neither adds an iteration).
template <int MAXP, class S, class T>
C4_HD int64_t run_lane(Lane &L, S &stk, const T tt, int64_t quota)
{
    int64_t used = 0;
    const int64_t max_iter = 3 * quota + 64;
    for (int64_t it = 0; it < max_iter && !L.done && (L.pending || used < quota); ++it) {
        if (L.pending) {
            if (L.d == 0) { L.done = true; break; }
            --L.d;
            const uint32_t m = stk.moves(L.d), ab = stk.ab(L.d);
            const int col = (int)((m >> 27) & 7);
            // undo: the top stone of `col` belongs to the mover of the node returned to
            const uint64_t occ = L.c0 | L.c1;
            const uint64_t bit = 1ULL << (H1 * col + col_count(occ, col) - 1);
            if ((popc64(occ) - 1) & 1) L.c1 ^= bit; else L.c0 ^= bit;
            L.moves = m;
            L.alpha = (int)(ab & 0xff) - 64;
            L.beta = (int)((ab >> 8) & 0xff) - 64;
            if constexpr (T::compiled) L.alpha0 = (int)((ab >> 16) & 0xff) - 64;
            const int v = -L.ret;
            if (v >= L.beta) {                      // cut-off: this node returns as well
                L.ret = v;
                tt_close(tt, L, TT_LOWER);
            } else {
                if (v > L.alpha) L.alpha = v;
                L.pending = false;
            }
        }
        if (!L.pending && used < quota) {
            if (moves_left(L.moves) == 0) {
                L.ret = L.alpha;
                L.pending = true;
                tt_close(tt, L, L.alpha > L.alpha0 ? TT_EXACT : TT_UPPER);
            } else if (L.d < MAXP) {
                const int col = (int)(L.moves & 7);
                const uint32_t rest = ((L.moves & 0xffffffu) >> 3) | ((uint32_t)(moves_left(L.moves) - 1) << 24);
                stk.moves(L.d) = rest | ((uint32_t)col << 27);
                if constexpr (T::compiled) stk.ab(L.d) = pack_ab(L.alpha, L.beta) | ((uint32_t)(L.alpha0 + 64) << 16);
                else stk.ab(L.d) = pack_ab(L.alpha, L.beta);
                ++L.d;
                (void)make_move(L.c0, L.c1, col);
                ++used;
                const uint64_t occ = L.c0 | L.c1;
                const int age = popc64(occ);
                const uint64_t mine = (age & 1) ? L.c1 : L.c0, theirs = (age & 1) ? L.c0 : L.c1;
                int a = -L.beta, b = -L.alpha, value = 0;
                uint32_t moves = 0;
                if (enter_node(mine, theirs, age, a, b, moves, value)) {
                    L.ret = value;
                    L.pending = true;
                } else {
                    L.alpha = a;
                    L.beta = b;
                    L.moves = moves;
                    if constexpr (T::compiled) {
                        if (book_covers(tt, age)) {             // the book first: whatever TT_MIN_EMPTIES and tt.e are
                            const Probe p = book_probe(tt, tt_key(mine, occ), a, b);
                            L.hits += p.hit ? 1 : 0;
                            L.alpha = p.alpha;
                            L.beta = p.beta;
                            if (p.hit == 2) {
                                L.ret = p.value;
                                L.pending = true;
                            }
                        }
                        if (!L.pending && tt_covers(tt, age)) {  // the table sees the window the book left
                            const Probe p = tt_probe(tt, tt_key(mine, occ), L.alpha, L.beta);
                            L.hits += p.hit ? 1 : 0;
                            L.alpha = p.alpha;
                            L.beta = p.beta;
                            if (p.hit == 2) {
                                L.ret = p.value;
                                L.pending = true;
                            }
                        }
                        L.alpha0 = L.alpha;
                    }
                }
            } else {
                L.ret = L.alpha;        // not reachable: a node MAXP deep has no empty square
                L.pending = true;
            }
        }
    }
    return used;
}

thread_local char solve_err[512] = "";

void set_solve_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(solve_err, sizeof(solve_err), fmt, ap);
    va_end(ap);
}

// work memory of one pass over `n` rows (row-indexed; frames [ply][row])
struct Work {
    uint64_t *c0, *c1;          // the position a stopped lane stands at
    uint32_t *moves, *misc;     // its top frame: the move list; the parked word (pack_parked)
    uint32_t *stk_moves, *stk_ab;
    int64_t n;
};

struct LdsStack {
    uint32_t (*m)[BLOCK];
    uint32_t (*a)[BLOCK];
    int lane;
    __device__ __forceinline__ uint32_t &moves(int p) { return m[p][lane]; }
    __device__ __forceinline__ uint32_t &ab(int p) { return a[p][lane]; }
};

// A windowed search (c4_solve_window*): where a row's window lives and where its answer goes.  score == nullptr: not a
// windowed search, nothing here is read.  alpha == nullptr (then beta is, too): every row has the full window.  The
// caller's arrays are the window's home for as long as the row is parked: the parked word holds the window of the top
// frame, which the root's probe and the search narrow, and the answer's kind is judged against the caller's own.
struct Window {
    const int8_t *alpha, *beta;
    int8_t *score, *bound;
    Window at(int64_t lo) const { return Window{alpha ? alpha + lo : nullptr, beta ? beta + lo : nullptr, score ? score + lo : nullptr, bound ? bound + lo : nullptr}; }
};

C4_HD int bound_kind(int score, int alpha, int beta)
{
    return score >= beta ? C4_SOLVE_BOUND_LOWER : score <= alpha ? C4_SOLVE_BOUND_UPPER : C4_SOLVE_BOUND_EXACT;
}

// the root of windowed row `row` has returned `ret`: score and kind, and outcome and final age where the score is exact
__device__ __forceinline__ void window_answer(const Window win, int64_t row, int age, int ret, int &outcome, int &final_age)
{
    const int a = win.alpha ? (int)win.alpha[row] : -SCORE_MAX, b = win.beta ? (int)win.beta[row] : SCORE_MAX;
    const int kind = bound_kind(ret, a, b);
    win.score[row] = (int8_t)ret;
    win.bound[row] = (int8_t)kind;
    outcome = -1;
    final_age = -1;
    if (kind == C4_SOLVE_BOUND_EXACT) root_answer(age, ret, outcome, final_age);
}

// The root of `row` has returned `ret` in k_solve_search: the row's outcome and final age, by window_answer in a windowed
// search (T has window code and win.score is not null), else by root_answer.  Each branch stores for itself, as the two
// kernels this one replaced did: a common tail is other device code.
template <class T>
__device__ __forceinline__ void store_root_answer(const int64_t *boards, int64_t row, int ret, const Window win, int8_t *outcome, int8_t *final_age)
{
    int o, fa;
    if constexpr (T::compiled) {
        if (win.score) {
            window_answer(win, row, popc64((uint64_t)boards[2 * row] | (uint64_t)boards[2 * row + 1]), ret, o, fa);
            outcome[row] = (int8_t)o;
            final_age[row] = (int8_t)fa;
            return;
        }
    }
    root_answer(popc64((uint64_t)boards[2 * row] | (uint64_t)boards[2 * row + 1]), ret, o, fa);
    outcome[row] = (int8_t)o;
    final_age[row] = (int8_t)fa;
}

// one lane per row: status, the answers that need no search, the root of the others; unfinished[row] = 1
// for a row that k_solve_search has to continue
// deep: the row goes to k_solve_search<DEEP_MAX_PLY, TableRef> -- every depth is searchable and the root probes the table
// `tt` like any interior node -- else to k_solve_search<MAX_PLY, NoTable>; hits: or null;
// win: a windowed search's arrays (the root starts from the row's window, and a row answered here -- an immediate win, a
// leaf root, a table entry that closes the window -- is judged like one answered by k_solve_search), or nulls
__global__ void __launch_bounds__(BLOCK) k_solve_init(const int64_t *__restrict__ boards, int64_t n, int64_t node_budget, Work w,
                                                      int8_t *__restrict__ status, int8_t *__restrict__ outcome,
                                                      int8_t *__restrict__ final_age, int64_t *__restrict__ nodes,
                                                      uint8_t *__restrict__ unfinished, bool deep, TableRef tt,
                                                      int64_t *__restrict__ hits, Window win)
{
    const int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (row >= n) return;
    const uint64_t c0 = (uint64_t)boards[2 * row], c1 = (uint64_t)boards[2 * row + 1];
    int o, fa;
    int st = classify(c0, c1, o, fa, deep ? DEEP_MAX_EMPTIES : MAX_EMPTIES);
    int64_t nd = 0;
    uint8_t more = 0;
    int hit = 0;
    if (win.score) {        // a row without an answer keeps these
        win.score[row] = 0;
        win.bound[row] = C4_SOLVE_BOUND_NONE;
    }
    if (st == C4_SOLVE_SOLVED) {
        Lane L;
        if (win.score && win.alpha) enter_root(c0, c1, L, win.alpha[row], win.beta[row]);
        else enter_root(c0, c1, L);
        nd = 1;
        if (deep && !L.done) {
            const uint64_t occ = c0 | c1;
            const int age = popc64(occ);
            if (book_covers(tt, age)) {
                const Probe p = book_probe(tt, tt_key((age & 1) ? c1 : c0, occ), L.alpha, L.beta);
                hit = p.hit ? 1 : 0;
                L.alpha = p.alpha;
                L.beta = p.beta;
                if (p.hit == 2) {
                    L.ret = p.value;
                    L.done = true;
                }
            }
            if (!L.done && tt_covers(tt, age)) {
                const Probe p = tt_probe(tt, tt_key((age & 1) ? c1 : c0, occ), L.alpha, L.beta);
                hit += p.hit ? 1 : 0;
                L.alpha = p.alpha;
                L.beta = p.beta;
                if (p.hit == 2) {
                    L.ret = p.value;
                    L.done = true;
                }
            }
            L.ret = L.done ? L.ret : L.alpha;       // a root that parks is not pending: the third field is its alpha0 (pack_parked)
        }
        if (L.done && win.score) window_answer(win, row, popc64(c0 | c1), L.ret, o, fa);
        else if (L.done) root_answer(popc64(c0 | c1), L.ret, o, fa);
        else if (nd >= node_budget) st = C4_SOLVE_UNKNOWN;
        else {
            more = 1;
            w.c0[row] = L.c0;
            w.c1[row] = L.c1;
            w.moves[row] = L.moves;
            w.misc[row] = pack_parked(L.alpha, L.beta, L.ret, 0, 0);     // depth 0, not pending
        }
    }
    status[row] = (int8_t)st;
    outcome[row] = (int8_t)o;
    final_age[row] = (int8_t)fa;
    nodes[row] = nd;
    unfinished[row] = more;
    if (hits) hits[row] = hit;
}

// One lane per unfinished row, through the dense list `active`: unpark, search up to the quota, answer or park again.
// MAXP: the frames a lane has, in LDS and in `w`.  T: NoTable -- tt, hits and win are not read -- or TableRef.
template <int MAXP, class T>
__global__ void __launch_bounds__(BLOCK) k_solve_search(const int64_t *__restrict__ boards, const int32_t *__restrict__ active, int32_t m,
                                                        int64_t node_budget, int64_t nodes_per_launch, Work w, T tt,
                                                        int8_t *__restrict__ status, int8_t *__restrict__ outcome,
                                                        int8_t *__restrict__ final_age, int64_t *__restrict__ nodes,
                                                        int64_t *__restrict__ hits, uint8_t *__restrict__ unfinished, Window win)
{
    __shared__ uint32_t s_moves[MAXP][BLOCK];
    __shared__ uint32_t s_ab[MAXP][BLOCK];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    const int64_t row = active[i];
    if (row < 0 || row >= w.n) return;
    LdsStack stk{s_moves, s_ab, (int)threadIdx.x};
    Lane L;
    L.c0 = w.c0[row];
    L.c1 = w.c1[row];
    L.moves = w.moves[row];
    unpark_lane<T>(w.misc[row], L);
    if (L.d > MAXP) L.d = MAXP;
    for (int p = 0; p < MAXP; ++p) {        // the frames below the top one, from `w` into LDS
        if (p < L.d) {
            s_moves[p][threadIdx.x] = w.stk_moves[(int64_t)p * w.n + row];
            s_ab[p][threadIdx.x] = w.stk_ab[(int64_t)p * w.n + row];
        }
    }
    const int64_t total = nodes[row];
    const int64_t left = node_budget - total;
    const int64_t quota = left < nodes_per_launch ? left : nodes_per_launch;
    const int64_t used = run_lane<MAXP>(L, stk, tt, quota);
    nodes[row] = total + used;
    if constexpr (T::compiled) {
        if (hits) hits[row] += L.hits;
    }
    if (L.done) {
        store_root_answer<T>(boards, row, L.ret, win, outcome, final_age);
        unfinished[i] = 0;
        return;
    }
    if (total + used >= node_budget) {      // it would take a node beyond the budget to go on
        status[row] = C4_SOLVE_UNKNOWN;
        unfinished[i] = 0;
        return;
    }
    unfinished[i] = 1;
    w.c0[row] = L.c0;
    w.c1[row] = L.c1;
    w.moves[row] = L.moves;
    w.misc[row] = park_lane<T>(L);
    for (int p = 0; p < MAXP; ++p) {        // and back
        if (p < L.d) {
            w.stk_moves[(int64_t)p * w.n + row] = s_moves[p][threadIdx.x];
            w.stk_ab[(int64_t)p * w.n + row] = s_ab[p][threadIdx.x];
        }
    }
}

// -- exact values over a leaf batch (c4_exact_leaves_dev) --------------------------------------------------------------------
// One launch between the network and the next tree step: the late rows of a leaf batch -- classify says searchable, at most
// max_empties empty squares -- are searched table-free from the window (-1, +1) by run_lane<MAX_PLY, LdsStack, NoTable>, the
// search of k_solve_search<MAX_PLY, NoTable>, and an answered row's value becomes who wins.  Nothing is parked: the quota of
// the one run_lane call is the whole budget less the root, so a lane ends answered or over budget, and the loop bound is
// run_lane's own 3 * quota + 64.
//
// A workgroup is LEAF_WAVES waves over LEAF_WAVES x 64 consecutive rows, each wave with a stack of its own (k_solve_search's
// 12 KiB).  Late rows are few for most of a game, so they are packed before the search: every lane classifies its row, the
// waves' ballots give each late row a dense place in s_rows (two barriers, which every lane of the workgroup reaches before
// any leaves), lanes 0..m-1 search s_rows[lane] and the waves behind m leave.  After the second barrier no lane waits for
// another.  The counters are reduced over the wave (ballots, one shuffle tree for the nodes) and added once a wave with 64-bit
// integer atomics: exact sums, whatever the grid.
constexpr int LEAF_WAVES = 4;
constexpr int LEAF_BLOCK = LEAF_WAVES * BLOCK;

__global__ void __launch_bounds__(LEAF_BLOCK) k_exact_leaves(const uint64_t *__restrict__ color0, const uint64_t *__restrict__ color1, int32_t n,
                                                             int max_empties, int64_t node_budget, float *__restrict__ values,
                                                             unsigned long long *__restrict__ counters)
{
    __shared__ uint32_t s_moves[LEAF_WAVES][MAX_PLY][BLOCK];
    __shared__ uint32_t s_ab[LEAF_WAVES][MAX_PLY][BLOCK];
    __shared__ int32_t s_rows[LEAF_BLOCK];
    __shared__ int32_t s_count[LEAF_WAVES];
    const int tid = (int)threadIdx.x, wave = tid / BLOCK, lane = tid % BLOCK;
    const int64_t mine = (int64_t)blockIdx.x * LEAF_BLOCK + tid;
    bool late = false;
    if (mine < n) {
        int o, fa;
        late = classify(color0[mine], color1[mine], o, fa, max_empties) == C4_SOLVE_SOLVED;
    }
    const unsigned long long ballot = __ballot(late);
    if (lane == 0) s_count[wave] = __popcll(ballot);
    __syncthreads();
    int base = 0, m = 0;
#pragma unroll
    for (int w = 0; w < LEAF_WAVES; ++w) {
        const int c = s_count[w];
        base += w < wave ? c : 0;
        m += c;
    }
    if (late) s_rows[base + __popcll(ballot & ((1ULL << lane) - 1))] = (int32_t)mine;     // base + rank < m <= LEAF_BLOCK
    __syncthreads();
    if (wave * BLOCK >= m) return;      // the same in every lane of the wave
    const bool work = tid < m;
    int64_t nodes = 0;
    bool answered = false;
    if (work) {
        const int32_t row = s_rows[tid];        // a late row of this workgroup: 0 <= row < n
        const uint64_t c0 = color0[row], c1 = color1[row];
        LdsStack stk{s_moves[wave], s_ab[wave], lane};
        Lane L;
        enter_root(c0, c1, L, -1, 1);
        nodes = 1;                              // the root is node 1, as in k_solve_init
        if (!L.done && node_budget > 1) nodes += run_lane<MAX_PLY>(L, stk, NoTable{}, node_budget - 1);
        if (L.done) {                           // else: it would take a node beyond the budget to go on
            const int sign = L.ret > 0 ? 1 : L.ret < 0 ? -1 : 0;
            values[row] = 0.5f * (float)(((popc64(c0 | c1) & 1) ? -sign : sign) + 1);       // o moves at even ages
            answered = true;
        }
    }
    if (counters) {
        const unsigned long long n_work = __popcll(__ballot(work)), n_answered = __popcll(__ballot(answered));
        long long sum = (long long)nodes;
#pragma unroll
        for (int off = BLOCK / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, BLOCK);
        if (lane == 0) {
            atomicAdd(&counters[C4_EXACT_LEAVES_OVERRIDDEN], n_answered);
            atomicAdd(&counters[C4_EXACT_LEAVES_OVER_BUDGET], n_work - n_answered);
            atomicAdd(&counters[C4_EXACT_LEAVES_NODES], (unsigned long long)sum);
            atomicAdd(&counters[C4_EXACT_LEAVES_LATE], n_work);
        }
    }
}

// the children of every row in column order: children[row][col] = the position after `col`, legal[row][col] = 1;
// an illegal column, or any column of a row that is not a searchable or too deep position: zeros
__global__ void __launch_bounds__(256) k_solve_children(const int64_t *__restrict__ boards, int64_t n, int64_t *__restrict__ children,
                                                        int8_t *__restrict__ legal)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint64_t c0 = (uint64_t)boards[2 * row], c1 = (uint64_t)boards[2 * row + 1];
    int o, fa;
    const int st = classify(c0, c1, o, fa);
    const bool open = st == C4_SOLVE_SOLVED || st == C4_SOLVE_TOO_DEEP;
    const int mask = open ? legal_mask(c0 | c1) : 0;
#pragma unroll
    for (int c = 0; c < WIDTH; ++c) {
        uint64_t n0 = 0, n1 = 0;
        const bool ok = ((mask >> c) & 1) != 0;
        if (ok) {
            n0 = c0;
            n1 = c1;
            (void)make_move(n0, n1, c);
        }
        children[(row * WIDTH + c) * 2] = (int64_t)n0;
        children[(row * WIDTH + c) * 2 + 1] = (int64_t)n1;
        legal[row * WIDTH + c] = ok ? 1 : 0;
    }
}

// -- the review of finished games against exact play (c4_review_*_dev) ------------------------------------------------------
// Book-keeping around c4_solve_window_dev, which searches the distinct late positions of a batch of games from the window
// (-1, +1): one lane a position, straight-line, every index checked, no LDS, no scratch, no lane waits for another, the
// only loop the seven columns of legal_mask / col_count.  The counters are 64- and 32-bit integer atomics (atomicAdd,
// atomicMax, atomicMin), so every output is a function of the inputs whatever the dispatch order.
constexpr int REVIEW_PLIES = C4_REVIEW_PLIES, REVIEW_COLUMNS = C4_REVIEW_COLUMNS, REVIEW_GAME_COLUMNS = C4_REVIEW_GAME_COLUMNS;

// late[row] = 1 for an undecided position with at most max_empties empty squares: the rows that are searched
__global__ void __launch_bounds__(256) k_review_select(const int64_t *__restrict__ boards, int64_t n, int max_empties, uint8_t *__restrict__ late)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    int o, fa;
    late[row] = classify((uint64_t)boards[2 * row], (uint64_t)boards[2 * row + 1], o, fa, max_empties) == C4_SOLVE_SOLVED ? 1 : 0;
}

// the searched rows' answers spread over the positions: status, outcome (absolute, from the sign of the mover's score and
// the parity of the age -- solver.outcomes) and nodes of row_of[row]; a position that is not late is TOO_DEEP, -1, 0
__global__ void __launch_bounds__(256) k_review_outcomes(const int64_t *__restrict__ boards, const uint8_t *__restrict__ late,
                                                         const int64_t *__restrict__ row_of, int64_t n, const int8_t *__restrict__ s_status,
                                                         const int8_t *__restrict__ s_score, const int64_t *__restrict__ s_nodes, int64_t m,
                                                         int8_t *__restrict__ status, int8_t *__restrict__ outcome, int64_t *__restrict__ nodes)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    int st = C4_SOLVE_TOO_DEEP, o = -1;
    int64_t nd = 0;
    if (late[row]) {
        const int64_t r = row_of[row];
        st = C4_SOLVE_UNKNOWN;      // an index outside the searched rows answers nothing
        if (r >= 0 && r < m) {
            st = s_status[r];
            nd = s_nodes ? s_nodes[r] : 0;
            if (st == C4_SOLVE_SOLVED) {
                const int age = popc64((uint64_t)boards[2 * row] | (uint64_t)boards[2 * row + 1]);
                const int score = s_score[r];
                const int sign = score > 0 ? 1 : score < 0 ? -1 : 0;
                o = ((age & 1) ? -sign : sign) + 1;     // o moves at even ages
            }
        }
    }
    status[row] = (int8_t)st;
    outcome[row] = (int8_t)o;
    if (nodes) nodes[row] = nd;
}

// the aggregates before a fold: zeros, and -1 for every game's last_blunder_age
__global__ void __launch_bounds__(256) k_review_clear(int64_t *__restrict__ by_ply, int32_t *__restrict__ per_game, int64_t n_games,
                                                      int32_t *__restrict__ chain_errors, int32_t *__restrict__ first_error)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < REVIEW_PLIES * REVIEW_COLUMNS) by_ply[i] = 0;
    if (i < n_games * REVIEW_GAME_COLUMNS) per_game[i] = (i % REVIEW_GAME_COLUMNS) == C4_REVIEW_GAME_LAST_BLUNDER_AGE ? -1 : 0;
    if (i == 0) {
        *chain_errors = 0;
        if (first_error) *first_error = INT32_MAX;
    }
}

struct ReviewFold {
    const int64_t *boards;          // [n][2]
    const uint8_t *moves;           // [n]
    const int32_t *game_index;      // [n]
    const int8_t *results;          // [n_games]
    const int8_t *outcome;          // [n], k_review_outcomes'
    const uint8_t *late;            // [n], k_review_select's
    const float *targets_in;        // [n], with exact_targets
    int8_t *kept, *target_agrees;   // [n]
    int64_t *by_ply;                // [42][7]
    int32_t *per_game;              // [n_games][4]
    int32_t *chain_errors, *first_error;
    float *exact_targets;           // [n] or nullptr
    const uint8_t *keep;            // [n][7], the moves that keep the outcome; with exact_priors
    const uint8_t *keep_known;      // [n], 1 where the row's keep mask is known
    const float *policy_in;         // [n][7]
    float *exact_priors;            // [n][7] or nullptr
    int64_t n, n_games;
};

// The rule of the review (c4_engine.h) for one position: the chain to the next row -- row + 1 is read by a plain load,
// every input is complete before this launch --, kept / target_agrees, the counters, the exact target.
__global__ void __launch_bounds__(256) k_review_fold(ReviewFold f)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= f.n) return;
    const uint64_t c0 = (uint64_t)f.boards[2 * row], c1 = (uint64_t)f.boards[2 * row + 1];
    const int g = f.game_index[row];
    const int mv = f.moves[row];
    int o_self, fa;
    const int st = classify(c0, c1, o_self, fa, DEEP_MAX_EMPTIES);
    const uint64_t occ = c0 | c1;
    const int age = popc64(occ);
    // the chain: a row is an undecided position of a game of the batch, its move is playable, and the position after the
    // move is the next row of the game or, behind the last row, finished with the game's result
    bool ok = st == C4_SOLVE_SOLVED && g >= 0 && g < f.n_games && mv < WIDTH;
    int result = -1;
    bool has_next = false;
    if (ok) {
        result = f.results[g];
        ok = result >= -1 && result <= C4_RESULT_OWIN && col_count(occ, mv) < HEIGHT;
    }
    if (ok) {
        uint64_t n0 = c0, n1 = c1;
        const uint32_t after = make_move(n0, n1, mv);
        has_next = row + 1 < f.n && f.game_index[row + 1] == g;
        if (has_next)
            ok = after == ST_FRESH && (uint64_t)f.boards[2 * row + 2] == n0 && (uint64_t)f.boards[2 * row + 3] == n1;
        else
            ok = after != ST_FRESH && (result < 0 || result == (int)after - (int)ST_XWIN);
    }
    int kept = -1, agrees = 0;
    float target = f.exact_targets ? f.targets_in[row] : 0.0f;
    if (!ok) {
        atomicAdd(f.chain_errors, 1);
        if (f.first_error) atomicMin(f.first_error, (int32_t)row);
    } else if (f.late[row]) {
        const int o = f.outcome[row];
        const int next = has_next ? (int)f.outcome[row + 1] : result;
        if (o >= 0 && next >= 0) kept = o == next ? 1 : 0;
        agrees = (o >= 0 && o == result) ? 1 : 0;
        // o, who moves at even ages, gains by a larger code; a known gain for the mover contradicts the solver
        const bool contradiction = kept == 0 && ((age & 1) ? next < o : next > o);
        if (o >= 0) target = 0.5f * (float)o;
        int64_t *ply = f.by_ply + age * REVIEW_COLUMNS;
        atomicAdd((unsigned long long *)&ply[C4_REVIEW_LATE], 1ULL);
        if (o >= 0) atomicAdd((unsigned long long *)&ply[C4_REVIEW_OUTCOME_KNOWN], 1ULL);
        if (kept >= 0) atomicAdd((unsigned long long *)&ply[C4_REVIEW_KEPT_KNOWN], 1ULL);
        if (kept == 1) atomicAdd((unsigned long long *)&ply[C4_REVIEW_KEPT], 1ULL);
        if (kept == 0) atomicAdd((unsigned long long *)&ply[C4_REVIEW_BLUNDERS], 1ULL);
        if (agrees) atomicAdd((unsigned long long *)&ply[C4_REVIEW_TARGET_AGREES], 1ULL);
        if (contradiction) atomicAdd((unsigned long long *)&ply[C4_REVIEW_CONTRADICTIONS], 1ULL);
        int32_t *game = f.per_game + (int64_t)g * REVIEW_GAME_COLUMNS;
        atomicAdd(&game[C4_REVIEW_GAME_LATE], 1);
        if (kept >= 0) atomicAdd(&game[C4_REVIEW_GAME_KEPT_KNOWN], 1);
        if (kept == 0) {
            atomicAdd(&game[C4_REVIEW_GAME_BLUNDERS], 1);
            atomicMax(&game[C4_REVIEW_GAME_LAST_BLUNDER_AGE], age);
        }
    }
    f.kept[row] = (int8_t)kept;
    f.target_agrees[row] = (int8_t)agrees;
    if (f.exact_targets) f.exact_targets[row] = target;
    if (f.exact_priors) {
        // uniform over the keeping moves where the mask is known (and the chain holds), the input policy elsewhere
        int count = 0;
        if (ok && f.late[row] && f.keep_known[row]) {
#pragma unroll
            for (int c = 0; c < WIDTH; ++c) count += f.keep[row * WIDTH + c] ? 1 : 0;
        }
        const float share = count ? 1.0f / (float)count : 0.0f;
#pragma unroll
        for (int c = 0; c < WIDTH; ++c)
            f.exact_priors[row * WIDTH + c] = count ? (f.keep[row * WIDTH + c] ? share : 0.0f) : f.policy_in[row * WIDTH + c];
    }
}

// -- the root driver: alpha-beta over a graph of positions (c4_solve_graph) ------------------------------------------------
// The levels of the graph lie one after the other; the last one is searched by k_solve_init and k_solve_search<DEEP_MAX_PLY,
// TableRef> from static windows, every kernel below is the book-keeping around that search: one lane a node, or a node and
// a column, straight-line, every index checked.  Where several parents write one child they write with atomicMin /
// atomicMax on a 32-bit word or store the same byte.  None of them uses LDS.
struct GraphDev {
    const int64_t *boards;      // [n_nodes][2]
    const int32_t *child;       // [n_nodes][7]
    int32_t *wa, *wb;           // the static window of every node
    int32_t *lo, *hi;           // its interval
    uint8_t *state;             // C4_SOLVE_NODE_*
    uint8_t *needed;            // the marks of one mark-down
    int32_t n_nodes, first_leaf;
};

C4_HD bool graph_decided(int lo, int hi, int a, int b) { return lo == hi || lo >= b || hi <= a; }

// level 0's windows from the caller's, every other node's the empty union
__global__ void __launch_bounds__(256) k_graph_window_init(GraphDev g, int32_t n0, const int8_t *__restrict__ alpha, const int8_t *__restrict__ beta)
{
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= g.n_nodes) return;
    const bool top = i < n0;
    g.wa[i] = top ? (alpha ? (int)alpha[i] : -SCORE_MAX) : SCORE_MAX;
    g.wb[i] = top ? (beta ? (int)beta[i] : SCORE_MAX) : -SCORE_MAX;
}

// one level's nodes [lo, hi) hand (-b, -a) to their children in [c_lo, c_hi): the union over the parents
__global__ void __launch_bounds__(256) k_graph_windows(GraphDev g, int32_t lo, int32_t hi, int32_t c_lo, int32_t c_hi)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)(hi - lo) * WIDTH) return;
    const int32_t node = lo + (int32_t)(t / WIDTH);
    const int32_t c = g.child[(int64_t)node * WIDTH + (int)(t % WIDTH)];
    if (c < c_lo || c >= c_hi) return;
    atomicMin(&g.wa[c], -g.wb[node]);
    atomicMax(&g.wb[c], -g.wa[node]);
}

// the windows of the last level as the search takes them
__global__ void __launch_bounds__(256) k_graph_leaf_windows(GraphDev g, int8_t *__restrict__ alpha, int8_t *__restrict__ beta)
{
    const int32_t r = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= g.n_nodes - g.first_leaf) return;
    alpha[r] = (int8_t)g.wa[g.first_leaf + r];
    beta[r] = (int8_t)g.wb[g.first_leaf + r];
}

// every node's own interval and state from the answers the last level has so far; a node with children starts from
// [-42, 42] and is folded afterwards
__global__ void __launch_bounds__(256) k_graph_leaves(GraphDev g, const int8_t *__restrict__ status, const int8_t *__restrict__ score,
                                                      const int8_t *__restrict__ bound, const int8_t *__restrict__ outcome,
                                                      const int8_t *__restrict__ final_age)
{
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= g.n_nodes) return;
    bool inner = false;
#pragma unroll
    for (int c = 0; c < WIDTH; ++c) inner |= g.child[(int64_t)i * WIDTH + c] >= 0;
    int lo = -SCORE_MAX, hi = SCORE_MAX, state = C4_SOLVE_NODE_INTERIOR;
    if (!inner) {
        const uint64_t c0 = (uint64_t)g.boards[2 * (int64_t)i], c1 = (uint64_t)g.boards[2 * (int64_t)i + 1];
        const int age = popc64(c0 | c1);
        int st, o, fa;
        int s = 0, kind = C4_SOLVE_BOUND_NONE;
        if (i >= g.first_leaf) {
            const int32_t r = i - g.first_leaf;
            st = status[r];
            o = outcome[r];
            fa = final_age[r];
            s = score[r];
            kind = bound[r];
        } else {
            st = classify(c0, c1, o, fa, DEEP_MAX_EMPTIES);
            st = st == C4_SOLVE_SOLVED ? C4_SOLVE_INVALID : st;     // a position to be searched above the last level: no answer
        }
        state = C4_SOLVE_NODE_SELF;
        if (st == C4_SOLVE_TERMINAL) {
            const int abs_score = o == C4_RESULT_OWIN ? 43 - fa : o == C4_RESULT_XWIN ? fa - 43 : 0;
            lo = hi = (age & 1) ? -abs_score : abs_score;
        } else if (st == C4_SOLVE_UNKNOWN) {
            state = C4_SOLVE_NODE_OVER_BUDGET;
        } else if (st == C4_SOLVE_SOLVED) {
            state = kind != C4_SOLVE_BOUND_NONE ? C4_SOLVE_NODE_ANSWERED : g.state[i] == C4_SOLVE_NODE_DROPPED ? C4_SOLVE_NODE_DROPPED : C4_SOLVE_NODE_PENDING;
            lo = kind == C4_SOLVE_BOUND_EXACT || kind == C4_SOLVE_BOUND_LOWER ? s : lo;
            hi = kind == C4_SOLVE_BOUND_EXACT || kind == C4_SOLVE_BOUND_UPPER ? s : hi;
        }
    }
    g.lo[i] = lo;
    g.hi[i] = hi;
    g.state[i] = (uint8_t)state;
}

// fold one level [lo, hi) up from its children in [c_lo, c_hi)
__global__ void __launch_bounds__(256) k_graph_fold(GraphDev g, int32_t lo, int32_t hi, int32_t c_lo, int32_t c_hi)
{
    const int32_t i = lo + (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= hi) return;
    int f_lo = -99, f_hi = -99;
    bool inner = false;
#pragma unroll
    for (int c = 0; c < WIDTH; ++c) {
        const int32_t ch = g.child[(int64_t)i * WIDTH + c];
        const bool ok = ch >= c_lo && ch < c_hi;
        const int32_t at = ok ? ch : i;     // a column without a child loads the node's own words: always a valid index
        const int l = g.lo[at], h = g.hi[at];
        inner |= ok;
        f_lo = ok && -h > f_lo ? -h : f_lo;
        f_hi = ok && -l > f_hi ? -l : f_hi;
    }
    if (inner) {
        g.lo[i] = f_lo;
        g.hi[i] = f_hi;
    }
}

// the answers of level 0 from its intervals, and its marks: a row is needed iff it is undecided
__global__ void __launch_bounds__(256) k_graph_roots(GraphDev g, int32_t n0, int8_t *__restrict__ status, int8_t *__restrict__ score,
                                                     int8_t *__restrict__ bound, int8_t *__restrict__ outcome, int8_t *__restrict__ final_age)
{
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n0) return;
    const uint64_t c0 = (uint64_t)g.boards[2 * (int64_t)i], c1 = (uint64_t)g.boards[2 * (int64_t)i + 1];
    int o, fa;
    int st = classify(c0, c1, o, fa, DEEP_MAX_EMPTIES);
    int s = 0, kind = C4_SOLVE_BOUND_NONE;
    bool need = false;
    if (st == C4_SOLVE_SOLVED) {
        const int lo = g.lo[i], hi = g.hi[i], a = g.wa[i], b = g.wb[i];
        if (lo == hi) { s = lo; kind = bound_kind(lo, a, b); }
        else if (lo >= b) { s = lo; kind = C4_SOLVE_BOUND_LOWER; }
        else if (hi <= a) { s = hi; kind = C4_SOLVE_BOUND_UPPER; }
        else { st = C4_SOLVE_UNKNOWN; need = g.state[i] == C4_SOLVE_NODE_INTERIOR; }
        if (kind == C4_SOLVE_BOUND_EXACT) root_answer(popc64(c0 | c1), s, o, fa);
    }
    status[i] = (int8_t)st;
    score[i] = (int8_t)s;
    bound[i] = (int8_t)kind;
    outcome[i] = (int8_t)o;
    final_age[i] = (int8_t)fa;
    g.needed[i] = need ? 1 : 0;
}

// mark one level [lo, hi) down: an open node needs the children that can still raise it above max(alpha, lo)
__global__ void __launch_bounds__(256) k_graph_mark(GraphDev g, int32_t lo, int32_t hi, int32_t c_lo, int32_t c_hi)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)(hi - lo) * WIDTH) return;
    const int32_t node = lo + (int32_t)(t / WIDTH);
    const int32_t c = g.child[(int64_t)node * WIDTH + (int)(t % WIDTH)];
    if (c < c_lo || c >= c_hi) return;
    const int n_lo = g.lo[node], n_hi = g.hi[node], a = g.wa[node], b = g.wb[node];
    if (!g.needed[node] || graph_decided(n_lo, n_hi, a, b)) return;
    const int raised = a > n_lo ? a : n_lo;
    const int c_lo_s = g.lo[c], c_hi_s = g.hi[c];
    if (c_lo_s < c_hi_s && -c_lo_s > raised) g.needed[c] = 1;
}

// a row that would go on although no undecided row needs its leaf leaves the search: unfinished[i] = 0, state dropped.
// active: the dense list the flags belong to, or null -- the flags are k_solve_init's, one a row
__global__ void __launch_bounds__(256) k_graph_filter(GraphDev g, const int32_t *__restrict__ active, int32_t m, uint8_t *__restrict__ unfinished)
{
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= m) return;
    const int32_t row = active ? active[i] : i;
    if (row < 0 || row >= g.n_nodes - g.first_leaf) return;
    const int32_t node = g.first_leaf + row;
    if (unfinished[i] && !g.needed[node]) {
        unfinished[i] = 0;
        g.state[node] = C4_SOLVE_NODE_DROPPED;
    }
}

#define SOLVE_CHECK(expr)                                                               \
    do {                                                                                   \
        hipError_t _r = (expr);                                                            \
        if (_r != hipSuccess) {                                                            \
            set_solve_err("%s failed: %s", #expr, hipGetErrorString(_r));                  \
            return C4_EDEVICE;                                                             \
        }                                                                                  \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t get(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    template <typename T> T *as() { return (T *)p; }
};

int pick_device(int device)
{
    int count = 0;
    hipError_t r = hipGetDeviceCount(&count);
    if (r != hipSuccess || count <= 0) { set_solve_err("no HIP device available: there is no CPU fallback"); return C4_EDEVICE; }
    if (device < 0 || device >= count) { set_solve_err("device %d out of range (have %d)", device, count); return C4_EDEVICE; }
    SOLVE_CHECK(hipSetDevice(device));
    return C4_OK;
}

// what every call answers, one entry a row; hits (a deep call's table_hits): or null
struct Answers {
    int8_t *status, *outcome, *final_age;
    int64_t *nodes, *hits;
    Answers at(int64_t lo) const { return Answers{status + lo, outcome + lo, final_age + lo, nodes + lo, hits ? hits + lo : nullptr}; }
};

constexpr Window NO_WINDOW{nullptr, nullptr, nullptr, nullptr};

// what c4_solve_graph hangs into solve_chunk's launch loop: the graph, the answers of its last level (the rows of the
// search) and of level 0
struct GraphPass {
    GraphDev g;
    const int64_t *level_start;     // host, n_levels + 1 entries
    int n_levels;
    Answers leaf;
    Window leaf_win;
    int8_t *status, *score, *bound, *outcome, *final_age;      // level 0
};

inline dim3 graph_grid(int64_t lanes) { return dim3((unsigned)((lanes + 255) / 256 > 0 ? (lanes + 255) / 256 : 1)); }

// Between two launches of the search: the leaves' answers to intervals, fold up, level 0's answers, mark down, and the
// filter over the flags the host is about to read (`active` and `m` as k_graph_filter takes them).  a memset and 2 * plies + 3 launches
// of a few lanes a node, all enqueued on the search's stream: no lane waits for another.
int graph_pass(hipStream_t stream, const GraphPass &p, const int32_t *active, int32_t m, uint8_t *unfinished)
{
    const GraphDev &g = p.g;
    const int64_t *ls = p.level_start;
    const int32_t n0 = (int32_t)ls[1];
    SOLVE_CHECK(hipMemsetAsync(g.needed, 0, (size_t)g.n_nodes, stream));
    hipLaunchKernelGGL(k_graph_leaves, graph_grid(g.n_nodes), dim3(256), 0, stream, g, p.leaf.status, p.leaf_win.score, p.leaf_win.bound,
                       p.leaf.outcome, p.leaf.final_age);
    for (int j = p.n_levels - 2; j >= 0; --j)
        hipLaunchKernelGGL(k_graph_fold, graph_grid(ls[j + 1] - ls[j]), dim3(256), 0, stream, g, (int32_t)ls[j], (int32_t)ls[j + 1],
                           (int32_t)ls[j + 1], (int32_t)ls[j + 2]);
    hipLaunchKernelGGL(k_graph_roots, graph_grid(n0), dim3(256), 0, stream, g, n0, p.status, p.score, p.bound, p.outcome, p.final_age);
    for (int j = 0; j <= p.n_levels - 2; ++j)
        hipLaunchKernelGGL(k_graph_mark, graph_grid((ls[j + 1] - ls[j]) * WIDTH), dim3(256), 0, stream, g, (int32_t)ls[j], (int32_t)ls[j + 1],
                           (int32_t)ls[j + 1], (int32_t)ls[j + 2]);
    hipLaunchKernelGGL(k_graph_filter, graph_grid(m), dim3(256), 0, stream, g, active, m, unfinished);
    SOLVE_CHECK(hipGetLastError());
    return C4_OK;
}

// one pass: rows [0, n) of `boards`, n <= CHUNK_ROWS.  deep: k_solve_search<DEEP_MAX_PLY, TableRef> with the table `tt` (or
// none), 42 plies of parked frames (360 B a row) and the windows `win` (or none); else k_solve_search<MAX_PLY, NoTable>
// graph: c4_solve_graph's pass (graph_pass) after k_solve_init and after every launch, before the flags are read; else null
int solve_chunk(hipStream_t stream, const int64_t *boards, int64_t n, int64_t node_budget, int64_t per_launch, bool deep, TableRef tt,
                Answers out, Window win, const GraphPass *graph = nullptr)
{
    DevBuf mem, flags, act;
    const int max_ply = deep ? DEEP_MAX_PLY : MAX_PLY;
    const size_t words = (size_t)n * (4 + 2 + 2 * max_ply);      // 32-bit words a row
    SOLVE_CHECK(mem.get(words * 4));
    SOLVE_CHECK(flags.get((size_t)n));
    SOLVE_CHECK(act.get((size_t)n * 4));
    Work w;
    w.n = n;
    w.c0 = mem.as<uint64_t>();
    w.c1 = w.c0 + n;
    w.moves = (uint32_t *)(w.c1 + n);
    w.misc = w.moves + n;
    w.stk_moves = w.misc + n;
    w.stk_ab = w.stk_moves + (size_t)n * max_ply;
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(k_solve_init, dim3(grid), dim3(BLOCK), 0, stream, boards, n, node_budget, w, out.status, out.outcome, out.final_age,
                       out.nodes, flags.as<uint8_t>(), deep, tt, out.hits, win);
    SOLVE_CHECK(hipGetLastError());
    if (graph) {
        const int rc = graph_pass(stream, *graph, nullptr, (int32_t)n, flags.as<uint8_t>());
        if (rc) return rc;
    }
    std::vector<uint8_t> host_flags((size_t)n);
    std::vector<int32_t> active, next;
    SOLVE_CHECK(hipMemcpyAsync(host_flags.data(), flags.p, (size_t)n, hipMemcpyDeviceToHost, stream));
    SOLVE_CHECK(hipStreamSynchronize(stream));
    for (int64_t i = 0; i < n; ++i)
        if (host_flags[(size_t)i]) active.push_back((int32_t)i);
    // every launch adds min(per_launch, budget left) nodes to each row it carries, or finishes the row
    const int64_t max_launches = node_budget / per_launch + 2;
    for (int64_t launch = 0; !active.empty(); ++launch) {
        if (launch >= max_launches) {
            set_solve_err("internal: %lld rows unfinished after %lld launches", (long long)active.size(), (long long)launch);
            return C4_ESTATE;
        }
        const int32_t m = (int32_t)active.size();
        SOLVE_CHECK(hipMemcpyAsync(act.p, active.data(), (size_t)m * 4, hipMemcpyHostToDevice, stream));
        const dim3 blocks((unsigned)((m + BLOCK - 1) / BLOCK));
        if (deep)
            hipLaunchKernelGGL((k_solve_search<DEEP_MAX_PLY, TableRef>), blocks, dim3(BLOCK), 0, stream, boards, act.as<int32_t>(), m, node_budget,
                               per_launch, w, tt, out.status, out.outcome, out.final_age, out.nodes, out.hits, flags.as<uint8_t>(), win);
        else
            // NoTable{}, out.hits and win are arguments this instantiation never reads
            hipLaunchKernelGGL((k_solve_search<MAX_PLY, NoTable>), blocks, dim3(BLOCK), 0, stream, boards, act.as<int32_t>(), m, node_budget,
                               per_launch, w, NoTable{}, out.status, out.outcome, out.final_age, out.nodes, out.hits, flags.as<uint8_t>(), win);
        SOLVE_CHECK(hipGetLastError());
        if (graph) {
            const int rc = graph_pass(stream, *graph, act.as<int32_t>(), m, flags.as<uint8_t>());
            if (rc) return rc;
        }
        SOLVE_CHECK(hipMemcpyAsync(host_flags.data(), flags.p, (size_t)m, hipMemcpyDeviceToHost, stream));
        SOLVE_CHECK(hipStreamSynchronize(stream));
        next.clear();
        for (int32_t i = 0; i < m; ++i)
            if (host_flags[(size_t)i]) next.push_back(active[(size_t)i]);
        active.swap(next);
    }
    return C4_OK;
}

// the device path of every entry point: n rows on the device, CHUNK_ROWS at a time
int solve_rows(hipStream_t stream, const int64_t *boards, int64_t n, int64_t node_budget, int64_t per_launch, bool deep, TableRef tt,
               Answers out, Window win)
{
    for (int64_t lo = 0; lo < n; lo += CHUNK_ROWS) {
        const int64_t m = n - lo < CHUNK_ROWS ? n - lo : CHUNK_ROWS;
        const int rc = solve_chunk(stream, boards + 2 * lo, m, node_budget, per_launch, deep, tt, out.at(lo), win.at(lo));
        if (rc) return rc;
    }
    return C4_OK;
}

int check_args(int64_t n, int64_t &node_budget, int64_t &per_launch, const Answers &out)
{
    if (n < 0) { set_solve_err("n < 0"); return C4_EINVAL; }
    if (n > 0 && (!out.status || !out.outcome || !out.final_age || !out.nodes)) { set_solve_err("null argument"); return C4_EINVAL; }
    if (node_budget < 0 || per_launch < 0) { set_solve_err("node_budget and nodes_per_launch must not be negative (0: the default)"); return C4_EINVAL; }
    if (node_budget == 0) node_budget = DEFAULT_BUDGET;
    if (per_launch == 0) per_launch = DEFAULT_PER_LAUNCH;
    if (per_launch > ((int64_t)1 << 40)) per_launch = (int64_t)1 << 40;
    return C4_OK;
}

// the pointers of a windowed call: alpha and beta come together (both null: the full window for every row)
int check_window_args(const Window &win, int64_t n)
{
    if (n > 0 && (!win.score || !win.bound)) { set_solve_err("null argument"); return C4_EINVAL; }
    if ((win.alpha == nullptr) != (win.beta == nullptr)) { set_solve_err("alpha and beta are given together, or both are null"); return C4_EINVAL; }
    return C4_OK;
}

// host copies of the windows of n rows: -42 <= alpha < beta <= 42 in every row
int check_windows(const int8_t *alpha, const int8_t *beta, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) {
        const int a = alpha[i], b = beta[i];
        if (a < -SCORE_MAX || b > SCORE_MAX || a >= b) {
            set_solve_err("row %lld: the window (%d, %d) is not -%d <= alpha < beta <= %d", (long long)i, a, b, SCORE_MAX, SCORE_MAX);
            return C4_EINVAL;
        }
    }
    return C4_OK;
}

}  // namespace

struct c4_solve_book {
    int device;
    int age;
    int64_t n;              // entries
    uint64_t *image;        // device: `mask + 1` words, open-addressed by book_home, linear probing, 0 = empty
    uint32_t mask;
    int steps;              // the longest probe sequence of any entry (0 for an empty book)
};

struct c4_solve_table {
    int device;
    int log2_entries;       // 0 with entries == nullptr: c4_solve_table_create_entryless
    uint64_t *entries;
    const c4_solve_book *book;      // c4_solve_table_attach_book, or nullptr
};

namespace {

// the table's reference for a call on `device`: C4_EINVAL for a table of another device
int table_ref(const c4_solve_table *table, int device, TableRef &tt)
{
    tt = TableRef{nullptr, 0, nullptr, 0, 0, 0};
    if (!table) return C4_OK;
    const bool entryless = !table->entries && table->log2_entries == 0;
    if (!entryless && (!table->entries || table->log2_entries < TT_MIN_LOG2 || table->log2_entries > TT_MAX_LOG2)) {
        set_solve_err("not a table of c4_solve_table_create");
        return C4_EINVAL;
    }
    if (table->device != device) {
        set_solve_err("the table lives on device %d, the call is for device %d", table->device, device);
        return C4_EINVAL;
    }
    if (!entryless) {
        tt.e = table->entries;
        tt.shift = 64 - table->log2_entries;
    }
    if (const c4_solve_book *b = table->book) {
        tt.book = b->image;
        tt.book_mask = b->mask;
        tt.book_age = b->age;
        tt.book_steps = b->steps;
    }
    return C4_OK;
}

// The checks of every entry point, in the order callers rely on: null and negative arguments; a windowed call's (`win` not
// null) pointer pairing and, where its windows are in host memory, their ranges; the table's device.  Then n == 0 is
// C4_OK before any device is touched, and the call's device is selected: the caller goes on if this returns C4_OK and n > 0.
int check_call(int device, const c4_solve_table *table, bool have_boards, int64_t n, int64_t &node_budget, int64_t &per_launch,
               const Answers &out, const Window *win, bool windows_on_host, TableRef &tt)
{
    if (n > 0 && !have_boards) { set_solve_err("null argument"); return C4_EINVAL; }
    int rc = check_args(n, node_budget, per_launch, out);
    if (rc == C4_OK && win) rc = check_window_args(*win, n);
    if (rc == C4_OK && win && win->alpha && windows_on_host) rc = check_windows(win->alpha, win->beta, n);
    if (rc == C4_OK) rc = table_ref(table, device, tt);
    if (rc || n == 0) return rc;
    return pick_device(device);
}

// The host-memory entry points: pack the boards, stage on the device the arrays the call has -- an entry of `host` or
// `host_win` that is null is neither allocated nor copied -- search, and copy the answers back.  Nothing is written to
// the caller's arrays unless the search returns C4_OK.
int solve_staged(const uint64_t *color0, const uint64_t *color1, int64_t n, int64_t node_budget, int64_t per_launch, bool deep, TableRef tt,
                 Answers host, Window host_win)
{
    std::vector<int64_t> packed((size_t)n * 2);
    for (int64_t i = 0; i < n; ++i) {
        packed[(size_t)(2 * i)] = (int64_t)color0[i];
        packed[(size_t)(2 * i + 1)] = (int64_t)color1[i];
    }
    enum { NODES, HITS, STATUS, OUTCOME, AGE, SCORE, BOUND, ALPHA, BETA, ARRAYS };
    struct Staged {
        void *host;
        size_t width;       // bytes an entry: the 8-byte arrays come first, so every array is aligned
        bool upload;        // an input; else an answer, copied back
        char *dev;
    } arrays[ARRAYS];
    arrays[NODES] = {host.nodes, 8, false, nullptr};
    arrays[HITS] = {host.hits, 8, false, nullptr};
    arrays[STATUS] = {host.status, 1, false, nullptr};
    arrays[OUTCOME] = {host.outcome, 1, false, nullptr};
    arrays[AGE] = {host.final_age, 1, false, nullptr};
    arrays[SCORE] = {host_win.score, 1, false, nullptr};
    arrays[BOUND] = {host_win.bound, 1, false, nullptr};
    arrays[ALPHA] = {(void *)host_win.alpha, 1, true, nullptr};
    arrays[BETA] = {(void *)host_win.beta, 1, true, nullptr};
    size_t bytes = 0;
    for (const Staged &a : arrays) bytes += a.host ? (size_t)n * a.width : 0;
    DevBuf b, mem;
    SOLVE_CHECK(b.get((size_t)n * 16));
    SOLVE_CHECK(mem.get(bytes));
    SOLVE_CHECK(hipMemcpy(b.p, packed.data(), (size_t)n * 16, hipMemcpyHostToDevice));
    char *at = mem.as<char>();
    for (Staged &a : arrays) {
        if (!a.host) continue;
        a.dev = at;
        at += (size_t)n * a.width;
        if (a.upload) SOLVE_CHECK(hipMemcpy(a.dev, a.host, (size_t)n * a.width, hipMemcpyHostToDevice));
    }
    const Answers out{(int8_t *)arrays[STATUS].dev, (int8_t *)arrays[OUTCOME].dev, (int8_t *)arrays[AGE].dev, (int64_t *)arrays[NODES].dev,
                      (int64_t *)arrays[HITS].dev};
    const Window win{(const int8_t *)arrays[ALPHA].dev, (const int8_t *)arrays[BETA].dev, (int8_t *)arrays[SCORE].dev, (int8_t *)arrays[BOUND].dev};
    const int rc = solve_rows(nullptr, b.as<int64_t>(), n, node_budget, per_launch, deep, tt, out, win);
    if (rc) return rc;
    for (const Staged &a : arrays)
        if (a.host && !a.upload) SOLVE_CHECK(hipMemcpy(a.host, a.dev, (size_t)n * a.width, hipMemcpyDeviceToHost));
    return C4_OK;
}

}  // namespace

extern "C" {

const char *c4_solve_last_error(void) { return solve_err; }

int c4_solve_dev(int device, void *hip_stream, const int64_t *boards_dev, int64_t n, int64_t node_budget, int64_t nodes_per_launch,
                 int8_t *status_dev, int8_t *outcome_dev, int8_t *final_age_dev, int64_t *nodes_dev)
{
    const Answers out{status_dev, outcome_dev, final_age_dev, nodes_dev, nullptr};
    TableRef tt;
    const int rc = check_call(device, nullptr, boards_dev != nullptr, n, node_budget, nodes_per_launch, out, nullptr, false, tt);
    if (rc || n == 0) return rc;
    return solve_rows((hipStream_t)hip_stream, boards_dev, n, node_budget, nodes_per_launch, false, tt, out, NO_WINDOW);
}

int c4_solve(int device, const uint64_t *color0, const uint64_t *color1, int64_t n, int64_t node_budget, int64_t nodes_per_launch,
             int8_t *status, int8_t *outcome, int8_t *final_age, int64_t *nodes)
{
    const Answers out{status, outcome, final_age, nodes, nullptr};
    TableRef tt;
    const int rc = check_call(device, nullptr, color0 && color1, n, node_budget, nodes_per_launch, out, nullptr, false, tt);
    if (rc || n == 0) return rc;
    return solve_staged(color0, color1, n, node_budget, nodes_per_launch, false, tt, out, NO_WINDOW);
}

int c4_solve_table_create(int device, int log2_entries, c4_solve_table **out)
{
    if (!out) { set_solve_err("null argument"); return C4_EINVAL; }
    *out = nullptr;
    if (log2_entries < TT_MIN_LOG2 || log2_entries > TT_MAX_LOG2) {
        set_solve_err("log2_entries %d outside %d..%d", log2_entries, TT_MIN_LOG2, TT_MAX_LOG2);
        return C4_EINVAL;
    }
    int rc = pick_device(device);
    if (rc) return rc;
    const size_t bytes = (size_t)8 << log2_entries;
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_solve_err("no device memory for a table of 2^%d entries (%zu bytes)", log2_entries, bytes);
        return C4_ENOMEM;
    }
    hipError_t r = hipMemset(p, 0, bytes);
    if (r == hipSuccess) r = hipDeviceSynchronize();
    if (r != hipSuccess) {
        (void)hipFree(p);
        set_solve_err("clearing the table failed: %s", hipGetErrorString(r));
        return C4_EDEVICE;
    }
    *out = new c4_solve_table{device, log2_entries, (uint64_t *)p};
    return C4_OK;
}

int c4_solve_table_destroy(c4_solve_table *table)
{
    if (!table) return C4_OK;
    if (pick_device(table->device) == C4_OK && table->entries) (void)hipFree(table->entries);
    delete table;
    return C4_OK;
}

int c4_solve_table_clear(c4_solve_table *table, void *hip_stream)
{
    if (!table || !table->entries) { set_solve_err("null argument"); return C4_EINVAL; }
    int rc = pick_device(table->device);
    if (rc) return rc;
    SOLVE_CHECK(hipMemsetAsync(table->entries, 0, (size_t)8 << table->log2_entries, (hipStream_t)hip_stream));
    SOLVE_CHECK(hipStreamSynchronize((hipStream_t)hip_stream));
    return C4_OK;
}

// Every solver call waits for its last launch before it returns, so after the device-wide wait the copy sees all its stores.
int c4_solve_table_read(c4_solve_table *table, uint64_t *entries_host, int64_t n)
{
    if (!table || !table->entries || !entries_host) { set_solve_err("null argument"); return C4_EINVAL; }
    if (table->log2_entries < TT_MIN_LOG2 || table->log2_entries > TT_MAX_LOG2) {
        set_solve_err("not a table of c4_solve_table_create");
        return C4_EINVAL;
    }
    const int64_t entries = (int64_t)1 << table->log2_entries;
    if (n != entries) {
        set_solve_err("n = %lld, the table has 2^%d = %lld entries", (long long)n, table->log2_entries, (long long)entries);
        return C4_EINVAL;
    }
    int rc = pick_device(table->device);
    if (rc) return rc;
    SOLVE_CHECK(hipDeviceSynchronize());
    SOLVE_CHECK(hipMemcpy(entries_host, table->entries, (size_t)entries * 8, hipMemcpyDeviceToHost));
    return C4_OK;
}

int c4_solve_table_create_entryless(int device, c4_solve_table **out)
{
    if (!out) { set_solve_err("null argument"); return C4_EINVAL; }
    *out = nullptr;
    int rc = pick_device(device);
    if (rc) return rc;
    *out = new c4_solve_table{device, 0, nullptr, nullptr};
    return C4_OK;
}

int c4_solve_table_attach_book(c4_solve_table *table, const c4_solve_book *book)
{
    if (!table) { set_solve_err("null argument"); return C4_EINVAL; }
    if (book && book->device != table->device) {
        set_solve_err("the book lives on device %d, the table on device %d", book->device, table->device);
        return C4_EINVAL;
    }
    table->book = book;
    return C4_OK;
}

// The image is laid out on the host, entry by entry in the order given: home slot, then the next free one.  Checked here,
// whatever built the words: no bits above the kind, a kind of 1..3, a score within +-42, a canonical key whose seven
// column fields are each 2^h + stones (h <= 6) with the heights adding up to `age`, and no key twice.  Not checked: that
// the two sides' stone counts fit the mover, and -- it cannot be -- that the score is a true bound of the position.
int c4_solve_book_create(int device, const uint64_t *words, int64_t n, int age, c4_solve_book **out)
{
    if (!out) { set_solve_err("null argument"); return C4_EINVAL; }
    *out = nullptr;
    if (n < 0 || (n > 0 && !words)) { set_solve_err(n < 0 ? "n < 0" : "null argument"); return C4_EINVAL; }
    if (age < 0 || age > CELLS - 1) { set_solve_err("age %d outside 0..%d", age, CELLS - 1); return C4_EINVAL; }
    if (n > (int64_t)1 << 28) { set_solve_err("%lld entries: a book takes 2^28", (long long)n); return C4_EINVAL; }
    uint64_t cap = 16;
    while (cap < 2 * (uint64_t)n) cap <<= 1;
    const uint32_t mask = (uint32_t)(cap - 1);
    std::vector<uint64_t> image((size_t)cap, 0);
    int steps = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t w = words[i], key = w & TT_KEY_MASK;
        const int kind = (int)((w >> 56) & 3), score = (int)((w >> 49) & 0x7f) - 64;
        if (key == 0 || (w >> 58) != 0 || kind == 0 || score < -SCORE_MAX || score > SCORE_MAX || book_key(key) != key) {
            set_solve_err("entry %lld (%#llx) is not a canonical table entry", (long long)i, (unsigned long long)w);
            return C4_EINVAL;
        }
        int stones = 0;
        bool fields_ok = true;
        for (int c = 0; c < WIDTH; ++c) {
            const unsigned f = (unsigned)((key >> (H1 * c)) & 0x7f);
            if (f == 0) { fields_ok = false; break; }
            stones += 31 - __builtin_clz(f);       // the column's height: floor(log2 f) <= 6
        }
        if (!fields_ok || stones != age) {
            set_solve_err("entry %lld: the key %#llx is not a position with %d stones", (long long)i, (unsigned long long)key, age);
            return C4_EINVAL;
        }
        const uint32_t home = book_home(key);
        int d = 0;
        for (;; ++d) {       // ends: the image is at most half full
            uint64_t &x = image[(size_t)((home + (uint32_t)d) & mask)];
            if (x == 0) { x = w; break; }
            if ((x & TT_KEY_MASK) == key) { set_solve_err("entry %lld: the key %#llx occurs twice", (long long)i, (unsigned long long)key); return C4_EINVAL; }
        }
        steps = d + 1 > steps ? d + 1 : steps;
    }
    int rc = pick_device(device);
    if (rc) return rc;
    void *p = nullptr;
    if (hipMalloc(&p, (size_t)cap * 8) != hipSuccess) {
        (void)hipGetLastError();
        set_solve_err("no device memory for a book of %lld entries", (long long)n);
        return C4_ENOMEM;
    }
    hipError_t r = hipMemcpy(p, image.data(), (size_t)cap * 8, hipMemcpyHostToDevice);
    if (r != hipSuccess) {
        (void)hipFree(p);
        set_solve_err("copying the book failed: %s", hipGetErrorString(r));
        return C4_EDEVICE;
    }
    *out = new c4_solve_book{device, age, n, (uint64_t *)p, mask, steps};
    return C4_OK;
}

int c4_solve_book_destroy(c4_solve_book *book)
{
    if (!book) return C4_OK;
    if (pick_device(book->device) == C4_OK && book->image) (void)hipFree(book->image);
    delete book;
    return C4_OK;
}

int c4_solve_deep_dev(int device, void *hip_stream, c4_solve_table *table, const int64_t *boards_dev, int64_t n, int64_t node_budget,
                      int64_t nodes_per_launch, int8_t *status_dev, int8_t *outcome_dev, int8_t *final_age_dev, int64_t *nodes_dev,
                      int64_t *table_hits_dev)
{
    const Answers out{status_dev, outcome_dev, final_age_dev, nodes_dev, table_hits_dev};
    TableRef tt;
    const int rc = check_call(device, table, boards_dev != nullptr, n, node_budget, nodes_per_launch, out, nullptr, false, tt);
    if (rc || n == 0) return rc;
    return solve_rows((hipStream_t)hip_stream, boards_dev, n, node_budget, nodes_per_launch, true, tt, out, NO_WINDOW);
}

int c4_solve_deep(int device, c4_solve_table *table, const uint64_t *color0, const uint64_t *color1, int64_t n, int64_t node_budget,
                  int64_t nodes_per_launch, int8_t *status, int8_t *outcome, int8_t *final_age, int64_t *nodes, int64_t *table_hits)
{
    const Answers out{status, outcome, final_age, nodes, table_hits};
    TableRef tt;
    const int rc = check_call(device, table, color0 && color1, n, node_budget, nodes_per_launch, out, nullptr, false, tt);
    if (rc || n == 0) return rc;
    return solve_staged(color0, color1, n, node_budget, nodes_per_launch, true, tt, out, NO_WINDOW);
}

int c4_solve_window_dev(int device, void *hip_stream, c4_solve_table *table, const int64_t *boards_dev, const int8_t *alpha_dev,
                        const int8_t *beta_dev, int64_t n, int64_t node_budget, int64_t nodes_per_launch, int8_t *status_dev,
                        int8_t *score_dev, int8_t *bound_dev, int8_t *outcome_dev, int8_t *final_age_dev, int64_t *nodes_dev,
                        int64_t *table_hits_dev)
{
    const Answers out{status_dev, outcome_dev, final_age_dev, nodes_dev, table_hits_dev};
    const Window win{alpha_dev, beta_dev, score_dev, bound_dev};
    TableRef tt;
    int rc = check_call(device, table, boards_dev != nullptr, n, node_budget, nodes_per_launch, out, &win, false, tt);
    if (rc || n == 0) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (alpha_dev) {        // the windows are checked on the host before the first launch
        std::vector<int8_t> ab((size_t)n * 2);
        SOLVE_CHECK(hipMemcpyAsync(ab.data(), alpha_dev, (size_t)n, hipMemcpyDeviceToHost, stream));
        SOLVE_CHECK(hipMemcpyAsync(ab.data() + n, beta_dev, (size_t)n, hipMemcpyDeviceToHost, stream));
        SOLVE_CHECK(hipStreamSynchronize(stream));
        rc = check_windows(ab.data(), ab.data() + n, n);
        if (rc) return rc;
    }
    return solve_rows(stream, boards_dev, n, node_budget, nodes_per_launch, true, tt, out, win);
}

int c4_solve_window(int device, c4_solve_table *table, const uint64_t *color0, const uint64_t *color1, const int8_t *alpha,
                    const int8_t *beta, int64_t n, int64_t node_budget, int64_t nodes_per_launch, int8_t *status, int8_t *score,
                    int8_t *bound, int8_t *outcome, int8_t *final_age, int64_t *nodes, int64_t *table_hits)
{
    const Answers out{status, outcome, final_age, nodes, table_hits};
    const Window win{alpha, beta, score, bound};
    TableRef tt;
    const int rc = check_call(device, table, color0 && color1, n, node_budget, nodes_per_launch, out, &win, true, tt);
    if (rc || n == 0) return rc;
    return solve_staged(color0, color1, n, node_budget, nodes_per_launch, true, tt, out, win);
}

// the graph of a c4_solve_graph call, all in host memory: C4_EINVAL names the first offender
static int check_graph(const int64_t *level_start, int n_levels, const int32_t *child, const int8_t *alpha, const int8_t *beta)
{
    if (n_levels - 1 < 1 || n_levels - 1 > C4_SOLVE_GRAPH_MAX_PLIES) {
        set_solve_err("a graph has 2..%d levels; got %d", C4_SOLVE_GRAPH_MAX_PLIES + 1, n_levels);
        return C4_EINVAL;
    }
    if (level_start[0] != 0) { set_solve_err("level_start[0] = %lld, not 0", (long long)level_start[0]); return C4_EINVAL; }
    for (int j = 0; j < n_levels; ++j)
        if (level_start[j + 1] < level_start[j]) {
            set_solve_err("level %d: level_start decreases from %lld to %lld", j, (long long)level_start[j], (long long)level_start[j + 1]);
            return C4_EINVAL;
        }
    const int64_t n_nodes = level_start[n_levels];
    if (n_nodes > (int64_t)1 << 30) { set_solve_err("%lld nodes: a graph takes 2^30", (long long)n_nodes); return C4_EINVAL; }
    if (n_nodes - level_start[n_levels - 1] > CHUNK_ROWS) {
        set_solve_err("the last level has %lld nodes, a graph takes %lld", (long long)(n_nodes - level_start[n_levels - 1]), (long long)CHUNK_ROWS);
        return C4_EINVAL;
    }
    std::vector<uint8_t> has_parent((size_t)n_nodes, 0);
    for (int j = 0; j < n_levels; ++j) {
        const int64_t c_lo = level_start[j + 1], c_hi = j + 1 < n_levels ? level_start[j + 2] : level_start[j + 1];     // the last level: none
        for (int64_t i = level_start[j]; i < level_start[j + 1]; ++i)
            for (int c = 0; c < WIDTH; ++c) {
                const int64_t ch = child[i * WIDTH + c];
                if (ch == -1) continue;
                if (ch < c_lo || ch >= c_hi) {
                    set_solve_err("node %lld, column %d: child %lld is not a node of the next level", (long long)i, c, (long long)ch);
                    return C4_EINVAL;
                }
                has_parent[(size_t)ch] = 1;
            }
    }
    for (int64_t i = level_start[1]; i < n_nodes; ++i)
        if (!has_parent[(size_t)i]) { set_solve_err("node %lld has no parent", (long long)i); return C4_EINVAL; }
    if ((alpha == nullptr) != (beta == nullptr)) { set_solve_err("alpha and beta are given together, or both are null"); return C4_EINVAL; }
    return alpha ? check_windows(alpha, beta, level_start[1]) : C4_OK;
}

int c4_solve_graph(int device, c4_solve_table *table, const uint64_t *color0, const uint64_t *color1, const int64_t *level_start,
                   int n_levels, const int32_t *child, const int8_t *alpha, const int8_t *beta, int64_t node_budget,
                   int64_t nodes_per_launch, int8_t *status, int8_t *score, int8_t *bound, int8_t *outcome, int8_t *final_age,
                   int64_t *nodes, int64_t *table_hits, int8_t *node_lo, int8_t *node_hi, int8_t *node_state, int64_t *node_nodes,
                   int64_t *node_table_hits)
{
    if (!level_start || !child || !color0 || !color1) { set_solve_err("null argument"); return C4_EINVAL; }
    int rc = check_graph(level_start, n_levels, child, alpha, beta);
    if (rc) return rc;
    const int64_t n_nodes = level_start[n_levels], n0 = level_start[1], first_leaf = level_start[n_levels - 1], n_leaf = n_nodes - first_leaf;
    const Answers out{status, outcome, final_age, nodes, table_hits};
    rc = check_args(n0, node_budget, nodes_per_launch, out);
    if (rc) return rc;
    if (n0 > 0 && (!score || !bound || !table_hits)) { set_solve_err("null argument"); return C4_EINVAL; }
    TableRef tt;
    rc = table_ref(table, device, tt);
    if (rc || n0 == 0) return rc;
    rc = pick_device(device);
    if (rc) return rc;

    std::vector<int64_t> packed((size_t)n_nodes * 2);
    for (int64_t i = 0; i < n_nodes; ++i) {
        packed[(size_t)(2 * i)] = (int64_t)color0[i];
        packed[(size_t)(2 * i + 1)] = (int64_t)color1[i];
    }
    // device memory: per node the boards, the children, window, interval, state and mark; per row of the last level the
    // search's answers and windows; per row of level 0 its answers and the caller's windows
    DevBuf d_boards, d_child, d_words, d_bytes, d_leaf64, d_leaf8, d_root8;
    SOLVE_CHECK(d_boards.get((size_t)n_nodes * 16));
    SOLVE_CHECK(d_child.get((size_t)n_nodes * WIDTH * 4));
    SOLVE_CHECK(d_words.get((size_t)n_nodes * 4 * 4));
    SOLVE_CHECK(d_bytes.get((size_t)n_nodes * 2));
    SOLVE_CHECK(d_leaf64.get((size_t)n_leaf * 2 * 8));
    SOLVE_CHECK(d_leaf8.get((size_t)n_leaf * 7));
    SOLVE_CHECK(d_root8.get((size_t)n0 * 7));
    SOLVE_CHECK(hipMemcpy(d_boards.p, packed.data(), (size_t)n_nodes * 16, hipMemcpyHostToDevice));
    SOLVE_CHECK(hipMemcpy(d_child.p, child, (size_t)n_nodes * WIDTH * 4, hipMemcpyHostToDevice));
    SOLVE_CHECK(hipMemset(d_bytes.p, 0, (size_t)n_nodes * 2));
    SOLVE_CHECK(hipMemset(d_leaf64.p, 0, (size_t)n_leaf * 2 * 8 ? (size_t)n_leaf * 2 * 8 : 16));
    int8_t *r8 = d_root8.as<int8_t>();
    if (alpha) {
        SOLVE_CHECK(hipMemcpy(r8 + 5 * n0, alpha, (size_t)n0, hipMemcpyHostToDevice));
        SOLVE_CHECK(hipMemcpy(r8 + 6 * n0, beta, (size_t)n0, hipMemcpyHostToDevice));
    }
    GraphPass p;
    p.g.boards = d_boards.as<int64_t>();
    p.g.child = d_child.as<int32_t>();
    p.g.wa = d_words.as<int32_t>();
    p.g.wb = p.g.wa + n_nodes;
    p.g.lo = p.g.wb + n_nodes;
    p.g.hi = p.g.lo + n_nodes;
    p.g.state = d_bytes.as<uint8_t>();
    p.g.needed = p.g.state + n_nodes;
    p.g.n_nodes = (int32_t)n_nodes;
    p.g.first_leaf = (int32_t)first_leaf;
    p.level_start = level_start;
    p.n_levels = n_levels;
    int8_t *l8 = d_leaf8.as<int8_t>();
    p.leaf = Answers{l8, l8 + n_leaf, l8 + 2 * n_leaf, d_leaf64.as<int64_t>(), d_leaf64.as<int64_t>() + n_leaf};
    p.leaf_win = Window{l8 + 3 * n_leaf, l8 + 4 * n_leaf, l8 + 5 * n_leaf, l8 + 6 * n_leaf};
    p.status = r8;
    p.score = r8 + n0;
    p.bound = r8 + 2 * n0;
    p.outcome = r8 + 3 * n0;
    p.final_age = r8 + 4 * n0;
    hipStream_t stream = nullptr;
    // the static windows, top-down
    hipLaunchKernelGGL(k_graph_window_init, graph_grid(n_nodes), dim3(256), 0, stream, p.g, (int32_t)n0, alpha ? r8 + 5 * n0 : nullptr,
                       alpha ? r8 + 6 * n0 : nullptr);
    for (int j = 0; j + 1 < n_levels; ++j)
        hipLaunchKernelGGL(k_graph_windows, graph_grid((level_start[j + 1] - level_start[j]) * WIDTH), dim3(256), 0, stream, p.g,
                           (int32_t)level_start[j], (int32_t)level_start[j + 1], (int32_t)level_start[j + 1], (int32_t)level_start[j + 2]);
    hipLaunchKernelGGL(k_graph_leaf_windows, graph_grid(n_leaf), dim3(256), 0, stream, p.g, l8 + 3 * n_leaf, l8 + 4 * n_leaf);
    SOLVE_CHECK(hipGetLastError());
    if (n_leaf > 0) {
        rc = solve_chunk(stream, p.g.boards + 2 * first_leaf, n_leaf, node_budget, nodes_per_launch, true, tt, p.leaf, p.leaf_win, &p);
        if (rc) return rc;
    } else {
        rc = graph_pass(stream, p, nullptr, 0, p.g.needed);      // nothing to search: every row answers for itself
        if (rc) return rc;
    }
    SOLVE_CHECK(hipStreamSynchronize(stream));

    std::vector<int32_t> words((size_t)n_nodes * 2);
    std::vector<uint8_t> state((size_t)n_nodes);
    std::vector<int64_t> leaf64((size_t)n_leaf * 2);
    SOLVE_CHECK(hipMemcpy(words.data(), p.g.lo, (size_t)n_nodes * 8, hipMemcpyDeviceToHost));
    SOLVE_CHECK(hipMemcpy(state.data(), p.g.state, (size_t)n_nodes, hipMemcpyDeviceToHost));
    if (n_leaf) SOLVE_CHECK(hipMemcpy(leaf64.data(), d_leaf64.p, (size_t)n_leaf * 16, hipMemcpyDeviceToHost));
    int8_t *const root_out[5] = {status, score, bound, outcome, final_age};
    for (int k = 0; k < 5; ++k) SOLVE_CHECK(hipMemcpy(root_out[k], r8 + (int64_t)k * n0, (size_t)n0, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n_nodes; ++i) {
        if (node_lo) node_lo[i] = (int8_t)words[(size_t)i];
        if (node_hi) node_hi[i] = (int8_t)words[(size_t)(n_nodes + i)];
        if (node_state) node_state[i] = (int8_t)state[(size_t)i];
        if (node_nodes) node_nodes[i] = i >= first_leaf ? leaf64[(size_t)(i - first_leaf)] : 0;
        if (node_table_hits) node_table_hits[i] = i >= first_leaf ? leaf64[(size_t)(n_leaf + i - first_leaf)] : 0;
    }
    // nodes and table_hits of a row: the sums over its distinct nodes of the last level, found by walking its descendants
    std::vector<int64_t> seen((size_t)n_nodes, -1);
    std::vector<int64_t> walk;
    for (int64_t r = 0; r < n0; ++r) {
        int64_t sum_nodes = 0, sum_hits = 0;
        walk.assign(1, r);
        seen[(size_t)r] = r;
        while (!walk.empty()) {
            const int64_t i = walk.back();
            walk.pop_back();
            if (i >= first_leaf) {
                sum_nodes += leaf64[(size_t)(i - first_leaf)];
                sum_hits += leaf64[(size_t)(n_leaf + i - first_leaf)];
                continue;
            }
            for (int c = 0; c < WIDTH; ++c) {
                const int64_t ch = child[i * WIDTH + c];
                if (ch >= 0 && seen[(size_t)ch] != r) {
                    seen[(size_t)ch] = r;
                    walk.push_back(ch);
                }
            }
        }
        nodes[r] = sum_nodes;
        table_hits[r] = sum_hits;
    }
    return C4_OK;
}

int c4_solve_children_dev(int device, void *hip_stream, const int64_t *boards_dev, int64_t n, int64_t *children_dev, int8_t *legal_dev)
{
    if (n < 0) { set_solve_err("n < 0"); return C4_EINVAL; }
    if (n == 0) return C4_OK;
    if (!boards_dev || !children_dev || !legal_dev) { set_solve_err("null argument"); return C4_EINVAL; }
    int rc = pick_device(device);
    if (rc) return rc;
    hipLaunchKernelGGL(k_solve_children, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, boards_dev, n,
                       children_dev, legal_dev);
    SOLVE_CHECK(hipGetLastError());
    return C4_OK;
}

int c4_exact_leaves_dev(int device, void *hip_stream, const uint64_t *color0_dev, const uint64_t *color1_dev, int32_t n, int max_empties,
                        int64_t node_budget, float *values_dev, int64_t *counters_dev)
{
    if (n < 0) { set_solve_err("n < 0"); return C4_EINVAL; }
    if (max_empties < 0 || max_empties > MAX_EMPTIES) { set_solve_err("max_empties %d outside 0..%d", max_empties, MAX_EMPTIES); return C4_EINVAL; }
    if (node_budget < 1) { set_solve_err("node_budget must be at least 1"); return C4_EINVAL; }
    if (!color0_dev || !color1_dev || !values_dev) { set_solve_err("null argument"); return C4_EINVAL; }
    if (n == 0 || max_empties == 0) return C4_OK;       // no row can be late: nothing is launched
    if (node_budget > ((int64_t)1 << 40)) node_budget = (int64_t)1 << 40;       // run_lane's loop bound is 3 * quota + 64
    int rc = pick_device(device);
    if (rc) return rc;
    hipLaunchKernelGGL(k_exact_leaves, dim3((unsigned)(((int64_t)n + LEAF_BLOCK - 1) / LEAF_BLOCK)), dim3(LEAF_BLOCK), 0, (hipStream_t)hip_stream,
                       color0_dev, color1_dev, n, max_empties, node_budget, values_dev, (unsigned long long *)counters_dev);
    SOLVE_CHECK(hipGetLastError());
    return C4_OK;
}

int c4_review_select_dev(int device, void *hip_stream, const int64_t *boards_dev, int64_t n, int max_empties, uint8_t *late_dev)
{
    if (n < 0) { set_solve_err("n < 0"); return C4_EINVAL; }
    if (max_empties < 0 || max_empties > CELLS) { set_solve_err("max_empties %d outside 0..%d", max_empties, CELLS); return C4_EINVAL; }
    if (n == 0) return C4_OK;
    if (!boards_dev || !late_dev) { set_solve_err("null argument"); return C4_EINVAL; }
    int rc = pick_device(device);
    if (rc) return rc;
    hipLaunchKernelGGL(k_review_select, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, boards_dev, n, max_empties,
                       late_dev);
    SOLVE_CHECK(hipGetLastError());
    return C4_OK;
}

int c4_review_outcomes_dev(int device, void *hip_stream, const int64_t *boards_dev, const uint8_t *late_dev, const int64_t *row_of_dev, int64_t n,
                           const int8_t *searched_status_dev, const int8_t *searched_score_dev, const int64_t *searched_nodes_dev, int64_t m,
                           int8_t *status_dev, int8_t *outcome_dev, int64_t *nodes_dev)
{
    if (n < 0 || m < 0) { set_solve_err("n < 0 or m < 0"); return C4_EINVAL; }
    if (n == 0) return C4_OK;
    if (!boards_dev || !late_dev || !row_of_dev || !status_dev || !outcome_dev || (m > 0 && (!searched_status_dev || !searched_score_dev)) ||
        (nodes_dev && m > 0 && !searched_nodes_dev)) {
        set_solve_err("null argument");
        return C4_EINVAL;
    }
    int rc = pick_device(device);
    if (rc) return rc;
    hipLaunchKernelGGL(k_review_outcomes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, boards_dev, late_dev,
                       row_of_dev, n, searched_status_dev, searched_score_dev, searched_nodes_dev, m, status_dev, outcome_dev, nodes_dev);
    SOLVE_CHECK(hipGetLastError());
    return C4_OK;
}

int c4_review_fold_dev(int device, void *hip_stream, const int64_t *boards_dev, const uint8_t *moves_dev, const int32_t *game_index_dev,
                       const int8_t *results_dev, int64_t n, int64_t n_games, const int8_t *outcome_dev, const uint8_t *late_dev,
                       const float *targets_in_dev, int8_t *kept_dev, int8_t *target_agrees_dev, int64_t *by_ply_dev, int32_t *per_game_dev,
                       int32_t *chain_errors_dev, int32_t *first_error_dev, float *exact_targets_dev, const uint8_t *keep_dev,
                       const uint8_t *keep_known_dev, const float *policy_in_dev, float *exact_priors_dev)
{
    if (n < 0 || n_games < 0) { set_solve_err("n < 0 or n_games < 0"); return C4_EINVAL; }
    if (n > INT32_MAX || n_games > INT32_MAX / REVIEW_GAME_COLUMNS) { set_solve_err("more rows or games than 32-bit indices hold"); return C4_EINVAL; }
    if (!by_ply_dev || !chain_errors_dev || (n_games > 0 && (!per_game_dev || !results_dev)) ||
        (n > 0 && (!boards_dev || !moves_dev || !game_index_dev || !outcome_dev || !late_dev || !kept_dev || !target_agrees_dev)) ||
        (n > 0 && exact_targets_dev && !targets_in_dev) || (n > 0 && exact_priors_dev && (!keep_dev || !keep_known_dev || !policy_in_dev))) {
        set_solve_err("null argument");
        return C4_EINVAL;
    }
    int rc = pick_device(device);
    if (rc) return rc;
    const int64_t cells = n_games * REVIEW_GAME_COLUMNS > REVIEW_PLIES * REVIEW_COLUMNS ? n_games * REVIEW_GAME_COLUMNS : REVIEW_PLIES * REVIEW_COLUMNS;
    hipLaunchKernelGGL(k_review_clear, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, by_ply_dev, per_game_dev,
                       n_games, chain_errors_dev, first_error_dev);
    SOLVE_CHECK(hipGetLastError());
    if (n == 0) return C4_OK;
    const ReviewFold f{boards_dev, moves_dev, game_index_dev, results_dev, outcome_dev, late_dev, targets_in_dev, kept_dev, target_agrees_dev,
                       by_ply_dev, per_game_dev, chain_errors_dev, first_error_dev, exact_targets_dev, keep_dev, keep_known_dev, policy_in_dev,
                       exact_priors_dev, n, n_games};
    hipLaunchKernelGGL(k_review_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, f);
    SOLVE_CHECK(hipGetLastError());
    return C4_OK;
}

}  // extern "C"
