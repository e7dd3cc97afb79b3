// c4_grid.hip -- exhaustive fixed-depth negamax (the reference's GridSearch, oinkoink/grid_search.py:10-71)
// on gfx950, behind c4_grid_search / c4_grid_frontier / c4_grid_finish of include/c4_engine.h.
//
// The reference expands every node to `plies` (tree.py:119-131, children in ascending column order, no
// expansion below a terminal position) and folds the values back with max (o to move) / min (x to move)
// starting from -2 / 2 (grid_search.py:59-70).  Here:
//   * levels: the batch of roots is expanded level by level into compacted device arrays of bitboards;
//     node i's children are contiguous at [off[i], off[i+1]) of the next level and in column order
//     (count kernel, exclusive scan, expand kernel).  A level's node order is therefore the reference's
//     depth-first visiting order of that depth;
//   * depth-first tail: once a level holds enough nodes to fill the GPU (and at most R_MAX plies remain),
//     one lane per node runs the remaining plies as nested loops (dfs<R>, compile-time depth): the move of
//     each level is its loop variable and the level's running value a register -- no recursion, no
//     per-node memory traffic, no scratch.  A lane never searches more than R_MAX plies, which bounds a
//     kernel's run time; a launch covers at least one full occupancy of the device (CUs x 4 SIMDs x 4
//     waves x 64 lanes) and at most that many x 7^(R_MAX - R) lanes, i.e. no more work than one
//     device-wide pass at R_MAX;
//   * reduction: each level's values fold into its parents' in column order with the reference's exact
//     comparisons (`max(value, v)` keeps value unless v > value), then the root kernel applies
//     Tree.best_move (tree.py:68-72,11-15: the larger side value, ties to the higher column).
// Max and min of exact float64 values do not depend on where they are computed, so the answers equal the
// reference's bit for bit; terminal values are computed as the reference writes them (a float64 division
// by 10000.0; the library builds with -ffp-contract=off).
//
// Leaves: evaluate_centre runs in-kernel (c4::centre_value).  Any other evaluator goes through the
// frontier / finish pair: the device enumerates the non-terminal positions `plies` deep (in the order the
// reference evaluates them), the caller evaluates them and hands the float64 values back, and the device
// does the reduction.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/c4_engine.h"
#include "c4_board.h"

using namespace c4;

namespace {

constexpr int R_MAX = 6;                    // most plies one lane searches depth-first (<= 7^6 leaves)
constexpr int64_t LEVEL_CAP = 1 << 21;      // most nodes of one expanded level (chunks beyond)
constexpr int WAVES_PER_SIMD = 4;           // k_grid_dfs<6> needs 127 VGPRs: 4 waves fit one SIMD
constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_ITEMS = 4;               // per thread: one block scans 1024 entries
constexpr int SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;

enum { MODE_CENTRE = 0, MODE_FRONTIER = 1, MODE_FINISH = 2 };

thread_local char grid_err[512] = "";

void set_grid_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(grid_err, sizeof(grid_err), fmt, ap);
    va_end(ap);
}

// grid_search.py:43-50: value of a finished position; `age` is its stone count.  An o win is
// 1 - age/10000, anything else (x win 0.0, draw 0.5: same_side(draw, o) is False) result + age/10000.
C4_HD double terminal_value(uint32_t st, int age)
{
    if (st == ST_OWIN) return 1.0 - (double)age / 10000.0;
    return (st == ST_DRAW ? 0.5 : 0.0) + (double)age / 10000.0;
}

// grid_search.py:62-70: max(value, v) / min(value, v) keep `value` unless v is strictly better
C4_HD double fold(bool o_to_move, double acc, double v)
{
    return o_to_move ? (v > acc ? v : acc) : (v < acc ? v : acc);
}

// Nested-loop negamax over the R plies below a non-terminal node (grid_search.py:38-71).
template <int R>
__device__ __forceinline__ double dfs(uint64_t c0, uint64_t c1)
{
    const uint64_t occ = c0 | c1;
    const int age = popc64(occ);
    const bool o_to_move = (age & 1) == 0;
    double acc = o_to_move ? -2.0 : 2.0;
    int mask = legal_mask(occ);
    while (mask) {
        const int col = __builtin_ctz(mask);
        mask &= mask - 1;
        uint64_t n0 = c0, n1 = c1;
        const uint32_t st = make_move(n0, n1, col);
        double v;
        if (st != ST_FRESH) v = terminal_value(st, age + 1);
        else if constexpr (R == 1) v = centre_value(n0, n1);
        else v = dfs<R - 1>(n0, n1);
        acc = fold(o_to_move, acc, v);
    }
    return acc;
}

template <int R>
__device__ __forceinline__ double node_value(uint64_t c0, uint64_t c1)
{
    const uint32_t st = position_status(c0, c1);
    if (st != ST_FRESH) return terminal_value(st, popc64(c0 | c1));
    if constexpr (R == 0) return centre_value(c0, c1);
    else return dfs<R>(c0, c1);
}

// one lane per node: its value with `R` plies left (centre leaves)
template <int R>
__global__ void __launch_bounds__(256) k_grid_dfs(const uint64_t *__restrict__ c0, const uint64_t *__restrict__ c1, int n,
                                                  double *__restrict__ val)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) val[i] = node_value<R>(c0[i], c1[i]);
}

// children per node (0 for a terminal node) -- tree.py:119-131 expand_node
__global__ void k_grid_count(const uint64_t *c0, const uint64_t *c1, int n, int32_t *cnt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t st = position_status(c0[i], c1[i]);
    cnt[i] = st == ST_FRESH ? popc64((uint64_t)legal_mask(c0[i] | c1[i])) : 0;
}

// 1 per non-terminal node (the positions an evaluator sees, grid_search.py:51-54)
__global__ void k_grid_flag_open(const uint64_t *c0, const uint64_t *c1, int n, int32_t *cnt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cnt[i] = position_status(c0[i], c1[i]) == ST_FRESH ? 1 : 0;
}

// exclusive scan of cnt[0..n) into off[0..n], three launches: tile scans + tile sums, scan of the tile sums
// (one block), tile offsets added.
__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_tiles(const int32_t *cnt, int n, int64_t *off, int64_t *tile_sum)
{
    __shared__ int64_t part[SCAN_BLOCK];
    const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    int64_t v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? cnt[base + k] : 0;
        s += v[k];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < SCAN_BLOCK; d <<= 1) {          // inclusive Hillis-Steele over the thread sums
        const int64_t t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += t;
        __syncthreads();
    }
    int64_t run = part[threadIdx.x] - s;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) off[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == SCAN_BLOCK - 1) tile_sum[blockIdx.x] = part[SCAN_BLOCK - 1];
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_sums(int64_t *tile_sum, int tiles, int64_t *total)
{
    __shared__ int64_t carry;
    __shared__ int64_t part[SCAN_BLOCK];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b = 0; b < tiles; b += SCAN_BLOCK) {
        const int i = b + threadIdx.x;
        const int64_t s = i < tiles ? tile_sum[i] : 0;
        part[threadIdx.x] = s;
        __syncthreads();
        for (int d = 1; d < SCAN_BLOCK; d <<= 1) {
            const int64_t t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < tiles) tile_sum[i] = carry + part[threadIdx.x] - s;
        __syncthreads();
        if (threadIdx.x == 0) carry += part[SCAN_BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ void k_scan_add(int64_t *off, int n, const int64_t *tile_sum, const int64_t *total)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) off[i] += tile_sum[i / SCAN_TILE];
    if (i == 0) off[n] = *total;
}

// children of node i at [off[i], off[i+1]) of the next level, ascending column (valid_moves order)
__global__ void k_grid_expand(const uint64_t *c0, const uint64_t *c1, int n, const int64_t *off, uint64_t *o0, uint64_t *o1)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || off[i] == off[i + 1]) return;
    int64_t k = off[i];
    int mask = legal_mask(c0[i] | c1[i]);
    while (mask) {
        const int col = __builtin_ctz(mask);
        mask &= mask - 1;
        uint64_t n0 = c0[i], n1 = c1[i];
        (void)make_move(n0, n1, col);
        o0[k] = n0;
        o1[k] = n1;
        ++k;
    }
}

// non-terminal leaves, in level order, at [off[i]] of the frontier buffer
__global__ void k_grid_gather_open(const uint64_t *c0, const uint64_t *c1, int n, const int64_t *off, int64_t *lo_hi,
                                   uint64_t *l0, uint64_t *l1)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || off[i] == off[i + 1]) return;
    const int64_t k = lo_hi[0] + off[i];
    if (k < lo_hi[1]) {
        l0[k - lo_hi[0]] = c0[i];
        l1[k - lo_hi[0]] = c1[i];
    }
}

// depth-0 values from the caller's evaluator: the leaves' values in frontier order
__global__ void k_grid_leaf_values(const uint64_t *c0, const uint64_t *c1, int n, const int64_t *off, const double *ext,
                                   double *val)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t st = position_status(c0[i], c1[i]);
    val[i] = st != ST_FRESH ? terminal_value(st, popc64(c0[i] | c1[i])) : ext[off[i]];
}

// grid_search.py:59-70: a node's value from its children's, in column order
__global__ void k_grid_reduce(const uint64_t *c0, const uint64_t *c1, int n, const int64_t *off, const double *child_val,
                              double *val)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t occ = c0[i] | c1[i];
    const uint32_t st = position_status(c0[i], c1[i]);
    if (st != ST_FRESH) { val[i] = terminal_value(st, popc64(occ)); return; }
    const bool o_to_move = (popc64(occ) & 1) == 0;
    double acc = o_to_move ? -2.0 : 2.0;
    for (int64_t k = off[i]; k < off[i + 1]; ++k) acc = fold(o_to_move, acc, child_val[k]);
    val[i] = acc;
}

// The roots: the children's absolute_value (tree.py:27-38: a finished child gives its result without the age
// term; NaN for an illegal column), the root's search_value and Tree.best_move (tree.py:68-72).
__global__ void k_grid_root(const uint64_t *c0, const uint64_t *c1, int n, const int64_t *off, const uint64_t *k0,
                            const uint64_t *k1, const double *child_val, double *child_abs, double *root_val, int32_t *move)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t occ = c0[i] | c1[i];
    const bool o_to_move = (popc64(occ) & 1) == 0;
    double abs7[WIDTH];
#pragma unroll
    for (int c = 0; c < WIDTH; ++c) abs7[c] = __builtin_nan("");
    double acc = o_to_move ? -2.0 : 2.0, best = 0.0;
    int best_col = -1;
    for (int64_t k = off[i]; k < off[i + 1]; ++k) {
        const uint64_t stone = (k0[k] | k1[k]) ^ occ;
        const int col = __builtin_ctzll(stone) / H1;
        const uint32_t st = position_status(k0[k], k1[k]);
        const double a = st != ST_FRESH ? 0.5 * (double)(st - ST_XWIN) : child_val[k];
        const double side = o_to_move ? a : 1.0 - a;        // utils.py:33-34 value_to_side
        if (best_col < 0 || side >= best) { best = side; best_col = col; }   // ties: the later (higher) column
        acc = fold(o_to_move, acc, child_val[k]);
#pragma unroll
        for (int c = 0; c < WIDTH; ++c)
            if (c == col) abs7[c] = a;
    }
#pragma unroll
    for (int c = 0; c < WIDTH; ++c) child_abs[(int64_t)i * WIDTH + c] = abs7[c];
    root_val[i] = acc;
    move[i] = best_col;
}

inline unsigned blocks(int64_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }

// Device memory of one call: a stack of chunks, released in the reverse order of the recursion that takes
// it (Mark), so a search costs a few hipMalloc calls, not one per level.  Every kernel and copy runs on the
// null stream, so memory handed out again is only written after the kernels that read it have finished.
struct Arena {
    std::vector<std::pair<char *, size_t>> chunks;
    size_t cur = 0, off = 0;
    hipError_t r = hipSuccess;
    ~Arena() { for (auto &c : chunks) (void)hipFree(c.first); }
    template <typename T>
    T *get(int64_t n)
    {
        const size_t bytes = ((n > 0 ? (size_t)n * sizeof(T) : 16) + 255) & ~(size_t)255;
        if (r != hipSuccess) return nullptr;
        for (; cur < chunks.size(); ++cur, off = 0) {
            if (off + bytes <= chunks[cur].second) {
                char *p = chunks[cur].first + off;
                off += bytes;
                return (T *)p;
            }
        }
        size_t size = chunks.empty() ? (size_t)4 << 20 : chunks.back().second * 2;
        size = size < bytes ? bytes : size;
        void *q = nullptr;
        r = hipMalloc(&q, size);
        if (r != hipSuccess) return nullptr;
        chunks.emplace_back((char *)q, size);
        cur = chunks.size() - 1;
        off = bytes;
        return (T *)q;
    }
};

struct Mark {
    Arena &a;
    size_t cur, off;
    explicit Mark(Arena &arena) : a(arena), cur(arena.cur), off(arena.off) {}
    ~Mark() { a.cur = cur; a.off = off; }
};

struct Search {
    int mode;
    Arena mem;
    int64_t level_cap = LEVEL_CAP;  // C4_GRID_LEVEL_CAP (tests: small values run the chunked paths)
    int64_t device_lanes = 0;       // lanes the device holds at once (k_grid_dfs<R_MAX> occupancy)
    int64_t fill_nodes = 0;         // a level this large goes depth-first; C4_GRID_FILL_NODES (tests)
    // MODE_FRONTIER: leaves copied to the caller's arrays while they fit; MODE_FINISH: their values
    uint64_t *leaf0 = nullptr, *leaf1 = nullptr;
    int64_t leaf_cap = 0;
    const double *leaf_values_dev = nullptr;
    int64_t n_leaf_values = 0;
    int64_t cursor = 0;            // leaves seen so far, in the reference's evaluation order
    int64_t *scratch = nullptr;    // device int64[2]: cursor / end for the gather kernel
};

#define GRID_CHECK(expr)                                                                   \
    do {                                                                                   \
        hipError_t _r = (expr);                                                            \
        if (_r != hipSuccess) {                                                            \
            set_grid_err("%s failed: %s", #expr, hipGetErrorString(_r));                   \
            return C4_EDEVICE;                                                             \
        }                                                                                  \
    } while (0)

int64_t env_int(const char *name, int64_t dflt, int64_t lo)
{
    const char *v = getenv(name);
    if (!v || !*v) return dflt;
    const long long x = atoll(v);
    return x < lo ? lo : (int64_t)x;
}

int setup(Search &s, int device, int mode)
{
    s.mode = mode;
    int cus = 0;
    GRID_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    s.device_lanes = (int64_t)(cus > 0 ? cus : 1) * 4 * WAVES_PER_SIMD * 64;
    // one node has at most 7 children: a cap of 7 still lets a single node expand
    s.level_cap = env_int("C4_GRID_LEVEL_CAP", LEVEL_CAP, WIDTH);
    s.fill_nodes = env_int("C4_GRID_FILL_NODES", s.device_lanes / 2, 1);
    s.scratch = s.mem.get<int64_t>(2);
    GRID_CHECK(s.mem.r);
    return C4_OK;
}

// off[0..n] = exclusive scan of cnt; returns the total through *total
int scan(Search &s, const int32_t *cnt, int n, int64_t *off, int64_t *total)
{
    Mark m(s.mem);
    const int tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    int64_t *tile_sum = s.mem.get<int64_t>(tiles), *tot = s.mem.get<int64_t>(1);
    GRID_CHECK(s.mem.r);
    hipLaunchKernelGGL(k_scan_tiles, dim3(tiles), dim3(SCAN_BLOCK), 0, 0, cnt, n, off, tile_sum);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_BLOCK), 0, 0, tile_sum, tiles, tot);
    hipLaunchKernelGGL(k_scan_add, dim3(blocks(n)), dim3(256), 0, 0, off, n, tile_sum, tot);
    GRID_CHECK(hipGetLastError());
    GRID_CHECK(hipMemcpy(total, tot, sizeof(int64_t), hipMemcpyDeviceToHost));
    return C4_OK;
}

// Lanes per launch: at least the device's full occupancy, at most that many x 7^(R_MAX - R) -- every launch
// does no more work than one device-wide pass at R_MAX.
template <int R>
void launch_dfs(const Search &s, const uint64_t *c0, const uint64_t *c1, int n, double *val)
{
    int64_t step = s.device_lanes;
    for (int k = R; k < R_MAX; ++k) step *= 7;
    for (int64_t lo = 0; lo < n; lo += step) {
        const int m = (int)(n - lo < step ? n - lo : step);
        hipLaunchKernelGGL(k_grid_dfs<R>, dim3(blocks(m)), dim3(256), 0, 0, c0 + lo, c1 + lo, m, val + lo);
    }
}

int run_dfs(const Search &s, const uint64_t *c0, const uint64_t *c1, int n, double *val, int left)
{
    switch (left) {
    case 0: launch_dfs<0>(s, c0, c1, n, val); break;
    case 1: launch_dfs<1>(s, c0, c1, n, val); break;
    case 2: launch_dfs<2>(s, c0, c1, n, val); break;
    case 3: launch_dfs<3>(s, c0, c1, n, val); break;
    case 4: launch_dfs<4>(s, c0, c1, n, val); break;
    case 5: launch_dfs<5>(s, c0, c1, n, val); break;
    case 6: launch_dfs<6>(s, c0, c1, n, val); break;
    default: set_grid_err("internal: depth-first tail of %d plies", left); return C4_EINVAL;
    }
    static_assert(R_MAX == 6, "run_dfs instantiates depths 0..R_MAX");
    GRID_CHECK(hipGetLastError());
    return C4_OK;
}

// Leaves of the caller's evaluator (`left` == 0): enumerate them or take their values.
int leaf_level(Search &s, const uint64_t *c0, const uint64_t *c1, int n, double *val)
{
    Mark mk(s.mem);
    int32_t *cnt = s.mem.get<int32_t>(n);
    int64_t *off = s.mem.get<int64_t>(n + 1);
    GRID_CHECK(s.mem.r);
    hipLaunchKernelGGL(k_grid_flag_open, dim3(blocks(n)), dim3(256), 0, 0, c0, c1, n, cnt);
    int64_t total = 0;
    int rc = scan(s, cnt, n, off, &total);
    if (rc) return rc;
    if (s.mode == MODE_FRONTIER) {
        if (total > 0 && s.cursor < s.leaf_cap) {
            const int64_t room = s.leaf_cap - s.cursor < total ? s.leaf_cap - s.cursor : total;
            uint64_t *l0 = s.mem.get<uint64_t>(room), *l1 = s.mem.get<uint64_t>(room);
            GRID_CHECK(s.mem.r);
            const int64_t dev_lo_hi[2] = {s.cursor, s.cursor + room};
            GRID_CHECK(hipMemcpy(s.scratch, dev_lo_hi, sizeof(dev_lo_hi), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_grid_gather_open, dim3(blocks(n)), dim3(256), 0, 0, c0, c1, n, off, s.scratch, l0, l1);
            GRID_CHECK(hipGetLastError());
            GRID_CHECK(hipMemcpy(s.leaf0 + s.cursor, l0, room * sizeof(uint64_t), hipMemcpyDeviceToHost));
            GRID_CHECK(hipMemcpy(s.leaf1 + s.cursor, l1, room * sizeof(uint64_t), hipMemcpyDeviceToHost));
        }
    } else {
        // the caller's values must cover these leaves before the kernel reads them
        if (s.cursor + total > s.n_leaf_values) {
            set_grid_err("%lld leaf values given, the search has more leaves", (long long)s.n_leaf_values);
            return C4_EINVAL;
        }
        hipLaunchKernelGGL(k_grid_leaf_values, dim3(blocks(n)), dim3(256), 0, 0, c0, c1, n, off,
                           s.leaf_values_dev + s.cursor, val);
        GRID_CHECK(hipGetLastError());
    }
    s.cursor += total;
    return C4_OK;
}

int expand(Search &s, const uint64_t *c0, const uint64_t *c1, int n, int64_t *off, int64_t *total)
{
    Mark mk(s.mem);
    int32_t *cnt = s.mem.get<int32_t>(n);
    GRID_CHECK(s.mem.r);
    hipLaunchKernelGGL(k_grid_count, dim3(blocks(n)), dim3(256), 0, 0, c0, c1, n, cnt);
    return scan(s, cnt, n, off, total);
}

// val[0..n) = negamax values of n nodes of one level with `left` plies to go (grid_search.py:38-71)
int solve(Search &s, const uint64_t *c0, const uint64_t *c1, int n, double *val, int left)
{
    if (n == 0) return C4_OK;
    if (s.mode != MODE_CENTRE && left == 0) return leaf_level(s, c0, c1, n, val);
    if (s.mode == MODE_CENTRE && left <= R_MAX && (left == 0 || n >= s.fill_nodes)) return run_dfs(s, c0, c1, n, val, left);
    Mark mk(s.mem);
    int64_t *off = s.mem.get<int64_t>(n + 1);
    GRID_CHECK(s.mem.r);
    int64_t total = 0;
    int rc = expand(s, c0, c1, n, off, &total);
    if (rc) return rc;
    if (total > s.level_cap) {
        if (s.mode == MODE_CENTRE && left <= R_MAX) return run_dfs(s, c0, c1, n, val, left);
        const int h = n / 2;            // n >= 2 here: one node has at most 7 <= level_cap children
        rc = solve(s, c0, c1, h, val, left);
        return rc ? rc : solve(s, c0 + h, c1 + h, n - h, val + h, left);
    }
    uint64_t *k0 = s.mem.get<uint64_t>(total), *k1 = s.mem.get<uint64_t>(total);
    double *kv = s.mem.get<double>(total);
    GRID_CHECK(s.mem.r);
    if (total > 0) {
        hipLaunchKernelGGL(k_grid_expand, dim3(blocks(n)), dim3(256), 0, 0, c0, c1, n, off, k0, k1);
        GRID_CHECK(hipGetLastError());
        rc = solve(s, k0, k1, (int)total, kv, left - 1);
        if (rc) return rc;
    }
    if (s.mode != MODE_FRONTIER) {
        hipLaunchKernelGGL(k_grid_reduce, dim3(blocks(n)), dim3(256), 0, 0, c0, c1, n, off, kv, val);
        GRID_CHECK(hipGetLastError());
    }
    return C4_OK;
}

int check_roots(int device, const uint64_t *c0, const uint64_t *c1, int32_t n, int32_t plies)
{
    if (!c0 || !c1) { set_grid_err("null argument"); return C4_EINVAL; }
    if (n < 0) { set_grid_err("n < 0"); return C4_EINVAL; }
    if (plies < 1 || plies > CELLS) { set_grid_err("plies=%d out of range [1,%d]", plies, CELLS); return C4_EINVAL; }
    const uint64_t cells = BOTTOM * COLMASK;
    for (int i = 0; i < n; ++i) {
        if ((c0[i] & c1[i]) || ((c0[i] | c1[i]) & ~cells)) { set_grid_err("position %d is not a board", i); return C4_EINVAL; }
        if (position_status(c0[i], c1[i]) != ST_FRESH) { set_grid_err("position %d is finished", i); return C4_EINVAL; }
    }
    int count = 0;
    hipError_t r = hipGetDeviceCount(&count);
    if (r != hipSuccess || count <= 0) { set_grid_err("no HIP device available: there is no CPU fallback"); return C4_EDEVICE; }
    if (device < 0 || device >= count) { set_grid_err("device %d out of range (have %d)", device, count); return C4_EDEVICE; }
    GRID_CHECK(hipSetDevice(device));
    return C4_OK;
}

// The whole batch, roots in chunks whose first level fits the level cap.
int run(Search &s, const uint64_t *c0, const uint64_t *c1, int32_t n, int32_t plies, double *child_abs, double *root_val,
        int32_t *move)
{
    const int chunk = (int)(s.level_cap / WIDTH);
    for (int lo = 0; lo < n; lo += chunk) {
        const int m = n - lo < chunk ? n - lo : chunk;
        Mark mk(s.mem);
        uint64_t *r0 = s.mem.get<uint64_t>(m), *r1 = s.mem.get<uint64_t>(m);
        int64_t *off = s.mem.get<int64_t>(m + 1);
        GRID_CHECK(s.mem.r);
        GRID_CHECK(hipMemcpy(r0, c0 + lo, m * sizeof(uint64_t), hipMemcpyHostToDevice));
        GRID_CHECK(hipMemcpy(r1, c1 + lo, m * sizeof(uint64_t), hipMemcpyHostToDevice));
        int64_t total = 0;
        int rc = expand(s, r0, r1, m, off, &total);
        if (rc) return rc;
        uint64_t *k0 = s.mem.get<uint64_t>(total), *k1 = s.mem.get<uint64_t>(total);
        double *kv = s.mem.get<double>(total);
        GRID_CHECK(s.mem.r);
        hipLaunchKernelGGL(k_grid_expand, dim3(blocks(m)), dim3(256), 0, 0, r0, r1, m, off, k0, k1);
        GRID_CHECK(hipGetLastError());
        rc = solve(s, k0, k1, (int)total, kv, plies - 1);
        if (rc) return rc;
        if (s.mode == MODE_FRONTIER) continue;
        double *abs_d = s.mem.get<double>((int64_t)m * WIDTH), *root_d = s.mem.get<double>(m);
        int32_t *move_d = s.mem.get<int32_t>(m);
        GRID_CHECK(s.mem.r);
        hipLaunchKernelGGL(k_grid_root, dim3(blocks(m)), dim3(256), 0, 0, r0, r1, m, off, k0, k1, kv, abs_d, root_d, move_d);
        GRID_CHECK(hipGetLastError());
        GRID_CHECK(hipMemcpy(child_abs + (int64_t)lo * WIDTH, abs_d, (size_t)m * WIDTH * sizeof(double), hipMemcpyDeviceToHost));
        GRID_CHECK(hipMemcpy(root_val + lo, root_d, m * sizeof(double), hipMemcpyDeviceToHost));
        GRID_CHECK(hipMemcpy(move + lo, move_d, m * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return C4_OK;
}

}  // namespace

extern "C" {

const char *c4_grid_last_error(void) { return grid_err; }

int c4_grid_search(int device, const uint64_t *color0, const uint64_t *color1, int32_t n, int32_t plies,
                   double *child_values, double *root_value, int32_t *move)
{
    if (!child_values || !root_value || !move) { set_grid_err("null argument"); return C4_EINVAL; }
    int rc = check_roots(device, color0, color1, n, plies);
    if (rc || n == 0) return rc;
    Search s;
    rc = setup(s, device, MODE_CENTRE);
    return rc ? rc : run(s, color0, color1, n, plies, child_values, root_value, move);
}

int c4_grid_frontier(int device, const uint64_t *color0, const uint64_t *color1, int32_t n, int32_t plies,
                     uint64_t *leaf0, uint64_t *leaf1, int64_t cap, int64_t *n_leaves)
{
    if (!n_leaves || cap < 0 || (cap > 0 && (!leaf0 || !leaf1))) { set_grid_err("bad leaf buffer"); return C4_EINVAL; }
    *n_leaves = 0;
    int rc = check_roots(device, color0, color1, n, plies);
    if (rc || n == 0) return rc;
    Search s;
    rc = setup(s, device, MODE_FRONTIER);
    if (rc) return rc;
    s.leaf0 = leaf0;
    s.leaf1 = leaf1;
    s.leaf_cap = cap;
    rc = run(s, color0, color1, n, plies, nullptr, nullptr, nullptr);
    if (rc) return rc;
    *n_leaves = s.cursor;
    if (s.cursor > cap) { set_grid_err("%lld leaves do not fit a buffer of %lld", (long long)s.cursor, (long long)cap); return C4_ECAPACITY; }
    return C4_OK;
}

int c4_grid_finish(int device, const uint64_t *color0, const uint64_t *color1, int32_t n, int32_t plies,
                   const double *leaf_values, int64_t n_leaves, double *child_values, double *root_value, int32_t *move)
{
    if (!child_values || !root_value || !move || n_leaves < 0 || (n_leaves > 0 && !leaf_values)) {
        set_grid_err("null argument");
        return C4_EINVAL;
    }
    int rc = check_roots(device, color0, color1, n, plies);
    if (rc || n == 0) return rc;
    Search s;
    rc = setup(s, device, MODE_FINISH);
    if (rc) return rc;
    double *lv = s.mem.get<double>(n_leaves);
    GRID_CHECK(s.mem.r);
    if (n_leaves > 0) GRID_CHECK(hipMemcpy(lv, leaf_values, n_leaves * sizeof(double), hipMemcpyHostToDevice));
    s.leaf_values_dev = lv;
    s.n_leaf_values = n_leaves;     // leaf_level checks every leaf level against it before reading
    rc = run(s, color0, color1, n, plies, child_values, root_value, move);
    if (rc) return rc;
    if (s.cursor != n_leaves) {
        set_grid_err("%lld leaf values given, the search has %lld leaves", (long long)n_leaves, (long long)s.cursor);
        return C4_EINVAL;
    }
    return C4_OK;
}

}  // extern "C"
