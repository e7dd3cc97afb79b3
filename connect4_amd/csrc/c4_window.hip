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
// Both launches go on the caller's stream, allocate nothing and wait for nothing: they can be captured in a graph.
#include <hip/hip_runtime.h>

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

}  // extern "C"
