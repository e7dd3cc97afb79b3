// c4_window.hip -- the sliding training window (oinkoink/neural/pytorch/data.py:66-75) kept on the device as
// packed positions, behind c4_window_gather_dev / c4_planes_to_boards_dev of include/c4_engine.h.
//
// The reference concatenates the materialised data.pth tensors of window_generations(gen) and lets a
// DataLoader index them.  A materialised row is 134 floats (126 planes + value + 7 priors) and every position
// is stored twice (plain and mirrored): 1,072 B for what two bitboards, a target and seven priors say in 48 B.
// Here the window stays a table of per-generation segments of packed positions (what PackedGames holds), and a
// batch is built by reading the table:
//   * k_window_gather: one wave per output row.  Virtual rows run across the segments in table order, segment s
//     giving its n_s positions as stored and then their n_s mirrors -- the row order of torch.cat over the
//     generations' k_training_tensors outputs.  The wave finds its segment once (lane s holds the end of segment
//     s: an inclusive scan over at most 64 lanes, then one ballot per row), reads the two bitboards, and its lanes
//     write the 126 plane floats as two coalesced stores, the 7 priors and the value.  Planes, mirroring and the
//     to-move plane come from c4_board.h exactly as k_training_tensors takes them, so the floats are the same bits.
//     An index outside [0, rows) reads nothing: its row is zeros and it is counted.
//   * k_planes_to_boards: the inverse of c4_board_planes (board.py:147-154), one wave per row: two loads per
//     lane, two ballots give the 126 cells as a bit mask, lane b of the wave looks up bitboard bit b and two more
//     ballots are the bitboards.  A row that no board encodes is counted.
//   * c4_window_merge_dev: identical positions of the window merged into one row each, with the mean of their targets
//     (include/c4_engine.h states the rule).  k_merge_insert, one lane per position, checks the row, forms its key
//     (mover's stones + occupied + BOTTOM, the form of c4_solve.hip's tt_key; the smaller of it and its mirror image's)
//     and finds the key's slot in an open-addressed table by linear probing: one 64-bit atomicCAS claims an empty
//     slot, and a CAS either claims the slot, finds the lane's own key there or moves on -- no lane waits for another,
//     and the probe ends within `capacity` steps because slots are never emptied and there are at most n <= capacity
//     keys.  The lane adds its target and priors, as integers (rne(x 2^40)), to the slot's eight int64 sums, so the
//     sums do not depend on the order of arrival, and atomicMax on (INT_MAX - index) keeps the group's first member.
//     The empty board's group gets about n / 30 members, all on the same nine words: with wave_combine (the default of
//     the Python side; 2.2x on a real window, profiles/window_merge.json) equal keys of a wave are summed in registers
//     first -- one ballot per distinct key, then the group's lowest lane collects its members' values by shuffles --
//     and only that lane goes to memory.  k_merge_insert<false> is the plain form: every lane its own atomics.
//     k_merge_count marks the first members and counts them per block, k_merge_scan (one block) turns the counts into
//     offsets, and k_merge_emit writes one row per first member, in input order.
// Every launch goes on the caller's stream, allocates nothing and waits for nothing: they can be captured in a graph.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cstdio>

#include "../../include/c4_engine.h"
#include "c4_board.h"

using namespace c4;

namespace {

constexpr int WAVE = 64;
constexpr int ROW_FLOATS = 3 * CELLS;        // 126
constexpr int WAVES_PER_BLOCK = 4;
constexpr int BLOCK = WAVE * WAVES_PER_BLOCK;
constexpr long long MAX_BLOCKS = 1 << 16;    // waves stride over the rows beyond

thread_local char window_err[256] = "";

void set_window_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(window_err, sizeof(window_err), fmt, ap);
    va_end(ap);
}

int use_device(int device)
{
    int count = 0;
    hipError_t r = hipGetDeviceCount(&count);
    if (r != hipSuccess || count <= 0) { set_window_err("no HIP device available: there is no CPU fallback"); return C4_EDEVICE; }
    if (device < 0 || device >= count) { set_window_err("device %d out of range (have %d)", device, count); return C4_EDEVICE; }
    r = hipSetDevice(device);
    if (r != hipSuccess) { set_window_err("hipSetDevice(%d) failed: %s", device, hipGetErrorString(r)); return C4_EDEVICE; }
    return C4_OK;
}

unsigned grid_for(long long rows)
{
    const long long blocks = (rows + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    return (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

__device__ __forceinline__ long long wave_uniform(long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__global__ __launch_bounds__(BLOCK) void k_window_gather(const c4_window_segment *segs, int n_segs, const int64_t *index, long long m,
                                                         float *ob, float *ov, float *op, int32_t *n_out_of_range)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long wave = (long long)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * WAVES_PER_BLOCK;
    // lane s: the virtual row after the last one of segment s (2 n_s rows each; lanes past the table repeat the total)
    long long mine = 0;
    if (lane < n_segs) { const long long n = segs[lane].n_positions; mine = n > 0 ? 2 * n : 0; }
    long long end = mine;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const long long v = __shfl_up(end, o, WAVE);
        if (lane >= o) end += v;
    }
    const long long rows = __shfl(end, WAVE - 1, WAVE);
    for (long long i = wave; i < m; i += n_waves) {
        const long long idx = wave_uniform(index[i]);
        float *row = ob + i * ROW_FLOATS;
        if (idx < 0 || idx >= rows) {            // nothing is read for it
            row[lane] = 0.0f;
            if (lane + WAVE < ROW_FLOATS) row[lane + WAVE] = 0.0f;
            if (lane < 7) op[i * 7 + lane] = 0.0f;
            if (lane == 7) ov[i] = 0.0f;
            if (lane == 0 && n_out_of_range) atomicAdd(n_out_of_range, 1);
            continue;
        }
        // segments that end at or before idx come first in the table: their number is idx's segment (idx < rows: < n_segs)
        const int s = __popcll(__ballot(lane < n_segs && end <= idx));
        const long long local = idx - wave_uniform(__shfl(end - mine, s, WAVE));
        const c4_window_segment seg = segs[s];
        const bool mirrored = local >= seg.n_positions;
        const long long src = mirrored ? local - seg.n_positions : local;
        uint64_t c0 = (uint64_t)seg.boards[2 * src], c1 = (uint64_t)seg.boards[2 * src + 1];
        if (mirrored) { c0 = flip_color(c0); c1 = flip_color(c1); }
        const int o_to_move = (popc64(c0 | c1) & 1) ? 0 : 1;
        row[lane] = plane_element(c0, c1, o_to_move, lane);
        if (lane + WAVE < ROW_FLOATS) row[lane + WAVE] = plane_element(c0, c1, o_to_move, lane + WAVE);
        if (lane < 7) op[i * 7 + lane] = seg.policy[src * 7 + (mirrored ? 6 - lane : lane)];
        if (lane == 7) ov[i] = seg.targets[src];
    }
}

__global__ __launch_bounds__(BLOCK) void k_planes_to_boards(const float *planes, long long n, int64_t *boards, int32_t *n_bad)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long wave = (long long)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * WAVES_PER_BLOCK;
    // lane b stands for bitboard bit b = 7 col + height (c4_board.h); its cell is element (5 - height) * 7 + col of a plane
    const int col = lane / H1, height = lane - col * H1;
    const bool is_cell = lane < WIDTH * H1 && height < HEIGHT;
    const int cell = is_cell ? (HEIGHT - 1 - height) * WIDTH + col : 0;
    constexpr unsigned long long PLANE = (1ULL << CELLS) - 1;
    for (long long i = wave; i < n; i += n_waves) {
        const float *row = planes + i * ROW_FLOATS;
        const bool has_b = lane + WAVE < ROW_FLOATS;
        const float a = row[lane];
        const float b = has_b ? row[lane + WAVE] : 0.0f;
        const unsigned long long lo = __ballot(a == 1.0f);            // elements 0..63
        const unsigned long long hi = __ballot(has_b && b == 1.0f);   // elements 64..125
        bool bad = __ballot(!(a == 0.0f || a == 1.0f) || !(b == 0.0f || b == 1.0f)) != 0;
        const int e0 = CELLS + cell, e1 = 2 * CELLS + cell;           // plane 1 = color[0], plane 2 = color[1]
        const bool s0 = is_cell && ((((e0 < WAVE ? lo : hi) >> (e0 & (WAVE - 1))) & 1) != 0);
        const bool s1 = is_cell && (((hi >> (e1 - WAVE)) & 1) != 0);
        const uint64_t c0 = __ballot(s0), c1 = __ballot(s1);
        const unsigned long long to_move = lo & PLANE;
        bad = bad || (c0 & c1) != 0 || (to_move != 0 && to_move != PLANE);
        bad = bad || (to_move != 0) != ((popc64(c0 | c1) & 1) == 0);   // plane 0 is 1 when o moves: an even stone count
        if (lane == 0) {
            boards[2 * i] = (int64_t)c0;
            boards[2 * i + 1] = (int64_t)c1;
            if (bad) atomicAdd(n_bad, 1);
        }
    }
}

// -- merging duplicate positions ---------------------------------------------------------------------------------------
constexpr uint64_t BOARD = BOTTOM * COLMASK;                 // the 42 cells
constexpr double FIXED_ONE = 1099511627776.0;                // 2^40
constexpr int MERGE_BLOCK = C4_WINDOW_MERGE_BLOCK;
constexpr int SCAN_BLOCK = 1024;

struct MergeSlot {                   // zero = empty: a key holds BOTTOM and is never 0
    unsigned long long key;
    unsigned long long sum[8];       // T, P[0..6]
    int count;
    int first_inv;                   // INT_MAX - the smallest member index (atomicMax; 0 = none yet)
};
static_assert(sizeof(MergeSlot) == C4_WINDOW_MERGE_SLOT_BYTES, "c4_engine.h states the slot size");

// the key of (c0, c1) and of its mirror image
__device__ __forceinline__ void position_keys(uint64_t c0, uint64_t c1, uint64_t &key, uint64_t &mkey)
{
    const uint64_t occ = c0 | c1;
    const bool odd = popc64(occ) & 1;
    key = (odd ? c1 : c0) + occ + BOTTOM;
    const uint64_t f0 = flip_color(c0), f1 = flip_color(c1);
    mkey = (odd ? f1 : f0) + (f0 | f1) + BOTTOM;
}

// ends[s] = positions in segments 0..s (lanes past the table repeat the total); every thread of the block calls it
__device__ __forceinline__ void segment_ends(const c4_window_segment *segs, int n_segs, long long *ends)
{
    if (threadIdx.x < WAVE) {
        const int lane = threadIdx.x;
        long long end = 0;
        if (lane < n_segs) { const long long n = segs[lane].n_positions; end = n > 0 ? n : 0; }
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const long long v = __shfl_up(end, o, WAVE);
            if (lane >= o) end += v;
        }
        ends[lane] = end;
    }
    __syncthreads();
}

// position i of the window: its segment and its row there; false when the table holds no position i
__device__ __forceinline__ bool locate_position(const long long *ends, int n_segs, long long i, int &s, long long &local)
{
    s = 0;
    for (int k = 0; k < n_segs; ++k) s += ends[k] <= i ? 1 : 0;
    if (s >= n_segs) return false;
    local = i - (s ? ends[s - 1] : 0);
    return true;
}

__device__ __forceinline__ bool unit_interval(float x) { return x >= 0.0f && x <= 1.0f; }      // (false for a NaN)
__device__ __forceinline__ unsigned long long to_fixed(float x) { return (unsigned long long)__double2ll_rn((double)x * FIXED_ONE); }

// the slot of `key`: claimed, or found.  -1 is unreachable while the table has room for every key (capacity >= n).
__device__ __forceinline__ int find_slot(MergeSlot *table, unsigned mask, uint64_t key)
{
    unsigned s = (unsigned)((key * 0x9E3779B97F4A7C15ULL) >> 32) & mask;
    for (unsigned p = 0; p <= mask; ++p, s = (s + 1) & mask) {
        unsigned long long k = __hip_atomic_load(&table[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) k = atomicCAS(&table[s].key, 0ULL, (unsigned long long)key);
        if (k == 0 || k == key) return (int)s;
    }
    return -1;
}

template <bool COMBINE>
__global__ __launch_bounds__(MERGE_BLOCK) void k_merge_insert(const c4_window_segment *segs, int n_segs, long long n, int mirror,
                                                              MergeSlot *table, unsigned mask, int32_t *slot_of, int32_t *n_bad)
{
    __shared__ long long ends[WAVE];
    segment_ends(segs, n_segs, ends);
    const long long i = (long long)blockIdx.x * MERGE_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    bool valid = false;
    uint64_t key = 0;
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int s;
    long long local;
    if (i < n && locate_position(ends, n_segs, i, s, local)) {
        const c4_window_segment seg = segs[s];
        const uint64_t c0 = (uint64_t)seg.boards[2 * local], c1 = (uint64_t)seg.boards[2 * local + 1];
        const uint64_t occ = c0 | c1;
        const float t = seg.targets[local];
        float p[WIDTH];
#pragma unroll
        for (int c = 0; c < WIDTH; ++c) p[c] = seg.policy[local * WIDTH + c];
        valid = !(c0 & c1) && !(occ & ~BOARD) && !(occ & (occ + BOTTOM)) && unit_interval(t);
#pragma unroll
        for (int c = 0; c < WIDTH; ++c) valid = valid && unit_interval(p[c]);
        uint64_t mkey;
        position_keys(c0, c1, key, mkey);
        const bool reversed = mirror && key > mkey;
        if (reversed) key = mkey;
        v[0] = to_fixed(t);
#pragma unroll
        for (int c = 0; c < WIDTH; ++c) v[1 + c] = to_fixed(reversed ? p[WIDTH - 1 - c] : p[c]);
    }
    int count = 1, slot = -1;
    bool adds = valid;
    unsigned long long mine = 0;
    if (COMBINE) {
        // equal keys of the wave first: the lowest lane of each key (the smallest index) adds for all of them
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const int first = __ffsll((long long)todo) - 1;
            const uint64_t k = (uint64_t)__shfl((long long)key, first, WAVE);
            const unsigned long long same = __ballot(valid && key == k);
            if (valid && key == k) mine = same;
            todo &= ~same;
        }
        adds = valid && lane == __ffsll((long long)mine) - 1;
        count = __popcll(mine);
        unsigned long long rest = adds ? mine & (mine - 1) : 0;
        while (__ballot(rest != 0)) {
            const int src = rest ? __ffsll((long long)rest) - 1 : lane;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned long long x = (unsigned long long)__shfl((long long)v[k], src, WAVE);
                if (rest) v[k] += x;
            }
            rest &= rest - 1;
        }
    }
    if (adds) {
        slot = find_slot(table, mask, key);
        if (slot >= 0) {
            MergeSlot *e = table + slot;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (v[k]) atomicAdd(&e->sum[k], v[k]);
            atomicAdd(&e->count, count);
            atomicMax(&e->first_inv, INT_MAX - (int)i);
        }
    }
    if (COMBINE && valid) slot = __shfl(slot, __ffsll((long long)mine) - 1, WAVE);
    if (i < n) {
        slot_of[i] = slot;
        if (slot < 0) atomicAdd(n_bad, 1);
    }
}

// slot_of[i] stays a slot only where i is the first member of its group; block_counts[b] = the first members of block b
__global__ __launch_bounds__(MERGE_BLOCK) void k_merge_count(long long n, const MergeSlot *table, int32_t *slot_of, int32_t *block_counts)
{
    __shared__ int per_wave[MERGE_BLOCK / WAVE];
    const long long i = (long long)blockIdx.x * MERGE_BLOCK + threadIdx.x;
    bool first = false;
    if (i < n) {
        const int slot = slot_of[i];
        first = slot >= 0 && INT_MAX - table[slot].first_inv == (int)i;
        if (!first) slot_of[i] = -1;
    }
    const unsigned long long firsts = __ballot(first);
    if ((threadIdx.x & (WAVE - 1)) == 0) per_wave[threadIdx.x >> 6] = __popcll(firsts);
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < MERGE_BLOCK / WAVE; ++w) total += per_wave[w];
        block_counts[blockIdx.x] = total;
    }
}

// one block: block_counts[0..n_blocks) -> their exclusive prefix sums, in place; *n_distinct = the total
__global__ __launch_bounds__(SCAN_BLOCK) void k_merge_scan(int32_t *block_counts, int n_blocks, int32_t *n_distinct)
{
    __shared__ int wave_sum[SCAN_BLOCK / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int per = (n_blocks + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const int lo = threadIdx.x * per, hi = lo + per < n_blocks ? lo + per : n_blocks;
    int own = 0;
    for (int b = lo; b < hi; ++b) own += block_counts[b];
    int incl = own;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int x = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += x;
    }
    if (lane == WAVE - 1) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_BLOCK / WAVE; ++w) {
        before += w < wave ? wave_sum[w] : 0;
        total += wave_sum[w];
    }
    int at = before + incl - own;
    for (int b = lo; b < hi; ++b) {
        const int c = block_counts[b];
        block_counts[b] = at;
        at += c;
    }
    if (threadIdx.x == 0) *n_distinct = total;
}

__global__ __launch_bounds__(MERGE_BLOCK) void k_merge_emit(const c4_window_segment *segs, int n_segs, long long n, int mirror,
                                                            const MergeSlot *table, const int32_t *slot_of, const int32_t *block_offsets,
                                                            int64_t *ob, float *ot, float *op, int32_t *oc)
{
    __shared__ long long ends[WAVE];
    __shared__ int per_wave[MERGE_BLOCK / WAVE];
    segment_ends(segs, n_segs, ends);
    const long long i = (long long)blockIdx.x * MERGE_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int slot = i < n ? slot_of[i] : -1;
    const unsigned long long firsts = __ballot(slot >= 0);
    if (lane == 0) per_wave[wave] = __popcll(firsts);
    __syncthreads();
    long long row = block_offsets[blockIdx.x] + __popcll(firsts & ((1ULL << lane) - 1));
#pragma unroll
    for (int w = 0; w < MERGE_BLOCK / WAVE; ++w) row += w < wave ? per_wave[w] : 0;
    int s;
    long long local;
    if (slot < 0 || !locate_position(ends, n_segs, i, s, local)) return;
    const c4_window_segment seg = segs[s];
    const uint64_t c0 = (uint64_t)seg.boards[2 * local], c1 = (uint64_t)seg.boards[2 * local + 1];
    const MergeSlot *e = table + slot;
    const int count = e->count;
    ob[2 * row] = (int64_t)c0;
    ob[2 * row + 1] = (int64_t)c1;
    oc[row] = count;
    if (count == 1) {                // the row itself, bit for bit
        ot[row] = seg.targets[local];
#pragma unroll
        for (int c = 0; c < WIDTH; ++c) op[row * WIDTH + c] = seg.policy[local * WIDTH + c];
        return;
    }
    uint64_t key, mkey;
    position_keys(c0, c1, key, mkey);
    const bool reversed = mirror && key > mkey;
    const double d = (double)count * FIXED_ONE;
    ot[row] = (float)((double)(long long)e->sum[0] / d);
#pragma unroll
    for (int c = 0; c < WIDTH; ++c) op[row * WIDTH + c] = (float)((double)(long long)e->sum[1 + (reversed ? WIDTH - 1 - c : c)] / d);
}

}  // namespace

extern "C" {

const char *c4_window_last_error(void) { return window_err; }

int c4_window_gather_dev(int device, void *hip_stream, const c4_window_segment *segments_dev, int32_t n_segments,
                         const int64_t *index_dev, int64_t m, float *boards_out, float *values_out, float *priors_out,
                         int32_t *n_out_of_range_dev)
{
    if (n_segments < 1 || n_segments > C4_WINDOW_MAX_SEGMENTS) {
        set_window_err("c4_window_gather_dev: %d segments (1..%d)", n_segments, C4_WINDOW_MAX_SEGMENTS);
        return C4_EINVAL;
    }
    if (m < 0 || !segments_dev || (m > 0 && (!index_dev || !boards_out || !values_out || !priors_out))) {
        set_window_err("c4_window_gather_dev: bad argument");
        return C4_EINVAL;
    }
    int rc = use_device(device);
    if (rc || m == 0) return rc;
    hipLaunchKernelGGL(k_window_gather, dim3(grid_for(m)), dim3(BLOCK), 0, (hipStream_t)hip_stream, segments_dev, (int)n_segments,
                       index_dev, (long long)m, boards_out, values_out, priors_out, n_out_of_range_dev);
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) { set_window_err("k_window_gather launch failed: %s", hipGetErrorString(r)); return C4_EDEVICE; }
    return C4_OK;
}

int c4_planes_to_boards_dev(int device, void *hip_stream, const float *planes_dev, int64_t n, int64_t *boards_out, int32_t *n_bad_dev)
{
    if (n < 0 || !n_bad_dev || (n > 0 && (!planes_dev || !boards_out))) { set_window_err("c4_planes_to_boards_dev: bad argument"); return C4_EINVAL; }
    int rc = use_device(device);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(k_planes_to_boards, dim3(grid_for(n)), dim3(BLOCK), 0, (hipStream_t)hip_stream, planes_dev, (long long)n, boards_out,
                       n_bad_dev);
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) { set_window_err("k_planes_to_boards launch failed: %s", hipGetErrorString(r)); return C4_EDEVICE; }
    return C4_OK;
}

int c4_window_merge_dev(int device, void *hip_stream, const c4_window_segment *segments_dev, int32_t n_segments, int64_t n_positions,
                        int32_t mirror, int32_t wave_combine, int32_t log2_capacity, void *table_dev, void *work_dev, int64_t *boards_out,
                        float *targets_out, float *policy_out, int32_t *counts_out, int32_t *n_distinct_dev, int32_t *n_bad_dev)
{
    if (n_segments < 1 || n_segments > C4_WINDOW_MAX_SEGMENTS) {
        set_window_err("c4_window_merge_dev: %d segments (1..%d)", n_segments, C4_WINDOW_MAX_SEGMENTS);
        return C4_EINVAL;
    }
    if (n_positions < 0 || n_positions >= C4_WINDOW_MERGE_MAX_POSITIONS) {
        set_window_err("c4_window_merge_dev: %lld positions (the int64 sums hold fewer than %d)", (long long)n_positions,
                       C4_WINDOW_MERGE_MAX_POSITIONS);
        return C4_EINVAL;
    }
    if (log2_capacity < 0 || log2_capacity > 30 || (1LL << log2_capacity) < n_positions) {
        set_window_err("c4_window_merge_dev: a table of 2^%d slots cannot hold %lld positions", log2_capacity, (long long)n_positions);
        return C4_EINVAL;
    }
    if (!segments_dev || !n_distinct_dev || !n_bad_dev ||
        (n_positions > 0 && (!table_dev || !work_dev || !boards_out || !targets_out || !policy_out || !counts_out))) {
        set_window_err("c4_window_merge_dev: bad argument");
        return C4_EINVAL;
    }
    int rc = use_device(device);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    const long long n = n_positions;
    const size_t capacity = (size_t)1 << log2_capacity;
    hipError_t r = hipMemsetAsync(n_distinct_dev, 0, sizeof(int32_t), stream);
    if (r == hipSuccess) r = hipMemsetAsync(n_bad_dev, 0, sizeof(int32_t), stream);
    if (r == hipSuccess && n > 0) r = hipMemsetAsync(table_dev, 0, capacity * sizeof(MergeSlot), stream);
    if (r != hipSuccess) { set_window_err("c4_window_merge_dev: clearing the table failed: %s", hipGetErrorString(r)); return C4_EDEVICE; }
    if (n == 0) return C4_OK;
    const unsigned n_blocks = (unsigned)((n + MERGE_BLOCK - 1) / MERGE_BLOCK);
    MergeSlot *table = (MergeSlot *)table_dev;
    int32_t *slot_of = (int32_t *)work_dev, *block_counts = slot_of + n;
    const unsigned mask = (unsigned)(capacity - 1);
    if (wave_combine)
        hipLaunchKernelGGL(k_merge_insert<true>, dim3(n_blocks), dim3(MERGE_BLOCK), 0, stream, segments_dev, (int)n_segments, n, (int)mirror,
                           table, mask, slot_of, n_bad_dev);
    else
        hipLaunchKernelGGL(k_merge_insert<false>, dim3(n_blocks), dim3(MERGE_BLOCK), 0, stream, segments_dev, (int)n_segments, n, (int)mirror,
                           table, mask, slot_of, n_bad_dev);
    r = hipGetLastError();
    if (r != hipSuccess) { set_window_err("k_merge_insert launch failed: %s", hipGetErrorString(r)); return C4_EDEVICE; }
    hipLaunchKernelGGL(k_merge_count, dim3(n_blocks), dim3(MERGE_BLOCK), 0, stream, n, table, slot_of, block_counts);
    r = hipGetLastError();
    if (r != hipSuccess) { set_window_err("k_merge_count launch failed: %s", hipGetErrorString(r)); return C4_EDEVICE; }
    hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(SCAN_BLOCK), 0, stream, block_counts, (int)n_blocks, n_distinct_dev);
    r = hipGetLastError();
    if (r != hipSuccess) { set_window_err("k_merge_scan launch failed: %s", hipGetErrorString(r)); return C4_EDEVICE; }
    hipLaunchKernelGGL(k_merge_emit, dim3(n_blocks), dim3(MERGE_BLOCK), 0, stream, segments_dev, (int)n_segments, n, (int)mirror, table,
                       slot_of, block_counts, boards_out, targets_out, policy_out, counts_out);
    r = hipGetLastError();
    if (r != hipSuccess) { set_window_err("k_merge_emit launch failed: %s", hipGetErrorString(r)); return C4_EDEVICE; }
    return C4_OK;
}

}  // extern "C"
