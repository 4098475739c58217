// gact_path.hpp -- the path run (gact_hip_candidates_paths): every selected candidate's alignment, one code per column,
// compacted into BAM-style CIGAR ops.  A second pass, opt-in, on the int32 chain kernel; nothing of the normal run changes.
//
//   ColumnSink          chain_kernel's chain walk (gact_chain_kernel.hpp) whose walker also writes every column's
//                       GACT_PATH_OP_* byte (walk_chain<..., PATH = true>) into the candidate's buffer
//   path_ops_kernel     run-length compaction, one wave per candidate: WRITE = false counts the ops, WRITE = true writes
//                       them at the offsets the exclusive scan of the counts gave
//
// Candidate k of a chunk owns cols[col_off[k], col_off[k+1]), ref_len + query_len bytes: the left phase writes downwards
// from the end, the right phase upwards from the start.  Every column consumes a ref or a query base and no base is
// consumed twice, so the two never meet; the alignment is the left part followed by the right part.
#pragma once

#include "gact_chain_kernel.hpp"

namespace gact {

struct PathArgs {
    uint8_t *cols;                // column bytes of the chunk
    const int64_t *col_off;       // [n + 1]: candidate k owns cols[col_off[k], col_off[k+1])
    int32_t *n_cols;              // [2n]: columns of the left phase, of the right phase (zeroed by the caller)
};

// The path run's sink of chain_kernel (gact_chain_kernel.hpp): the column cursor round the walk.  n_left / n_right are the
// columns the candidate's two phases have written so far (the walking lane's).
struct ColumnSink {
    PathArgs pa;
    int n_left, n_right;

    __device__ __forceinline__ int first() const { return 0; }
    __device__ __forceinline__ void begin() { n_left = 0; n_right = 0; }
    __device__ __forceinline__ void picked(const ChainState &, const ChainQueues &, bool, bool) const {}
    template <int C>
    __device__ __forceinline__ void walk(const TileWalk &t, const ChainState &s, const KParams &kp, ScoreWalk &wk,
                                         int &ref_steps, int &query_steps, int &nst)
    {
        // this tile's columns go on where the phase's last tile left off
        const int64_t b0 = pa.col_off[s.cand], b1 = pa.col_off[s.cand + 1];
        const bool left = s.phase == 0;
        PathCursor pc;
        pc.p = left ? pa.cols + b1 - 1 - n_left : pa.cols + b0 + n_right;
        pc.lo = pa.cols + b0;
        pc.hi = pa.cols + b1 - n_left;
        pc.dir = left ? -1 : 1;
        uint8_t *const start = pc.p;
        walk_chain<C, 0, C / 4, kGroup, true>(t.ws, t.scratch, t.R, t.Q, t.l0, t.c0, t.k0, kp.early, t.rrow, 1, t.qrow, s.phase,
                                              kp, wk, ref_steps, query_steps, nst, 0, nullptr, -1, nullptr, &pc);
        const int cols = (int)((pc.p - start) * pc.dir);
        if (left) n_left += cols; else n_right += cols;
        pa.n_cols[2 * s.cand] = n_left;
        pa.n_cols[2 * s.cand + 1] = n_right;
    }
    __device__ __forceinline__ void advanced(const ChainState &, const ChainQueues &, const KParams &, bool) const {}
};

// column t of candidate k's alignment (left part, then right part)
__device__ __forceinline__ uint32_t path_col(const uint8_t *cols, int64_t b0, int64_t b1, int n_left, int t)
{
    return t < n_left ? cols[b1 - n_left + t] : cols[b0 + (t - n_left)];
}

// One wave per candidate, 64 columns per step: a column that differs from the one before it starts a run (ballot); the
// run it ends is written by that lane, its length the distance to the run's own start (the boundary below it in the
// ballot, or the last one of an earlier step).  WRITE = false: n_ops[k] = runs; true: ops[op_off[k] ...] = len << 4 | op.
template <bool WRITE>
__global__ __launch_bounds__(256) void path_ops_kernel(const uint8_t *__restrict__ cols, const int64_t *__restrict__ col_off,
                                                       const int32_t *__restrict__ n_cols, int n, int32_t *__restrict__ n_ops,
                                                       const int64_t *__restrict__ op_off, uint32_t *__restrict__ ops)
{
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_waves = (int)((gridDim.x * blockDim.x) >> 6);
    const uint64_t below_me = (1ull << lane) - 1;
    for (int k = wave; k < n; k += n_waves) {                   // (wave-uniform)
        const int64_t b0 = col_off[k], b1 = col_off[k + 1];
        const int64_t cap = b1 - b0;
        const int n_left = (int)(n_cols[2 * k] < cap ? n_cols[2 * k] : cap);
        const int n_right = (int)(n_cols[2 * k + 1] < cap - n_left ? n_cols[2 * k + 1] : cap - n_left);
        const int len = n_left + n_right;
        int64_t j = WRITE ? op_off[k] : 0;
        int open = 0;                                           // start of the run that is still open
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int t = c0 + lane;
            const bool in = t < len;
            const uint32_t code = in ? path_col(cols, b0, b1, n_left, t) : 0u;
            const uint32_t prev = (in && t > 0) ? path_col(cols, b0, b1, n_left, t - 1) : code;
            const bool starts = in && t > 0 && code != prev;
            const uint64_t m = __ballot(starts);
            if (WRITE && starts) {
                const uint64_t below = m & below_me;
                const int from = below ? c0 + 63 - __clzll((long long)below) : open;
                ops[j + __popcll(below)] = ((uint32_t)(t - from) << 4) | prev;
            }
            j += __popcll(m);
            if (m) open = c0 + 63 - __clzll((long long)m);
        }
        if (lane == 0) {
            if (WRITE) {
                if (len > 0) ops[j] = ((uint32_t)(len - open) << 4) | path_col(cols, b0, b1, n_left, len - 1);
            } else {
                n_ops[k] = len > 0 ? (int32_t)j + 1 : 0;
            }
        }
    }
}

}  // namespace gact
