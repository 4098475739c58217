// gact_path.hpp -- the path run (gact_hip_candidates_paths): every selected candidate's alignment, one code per column,
// compacted into BAM-style CIGAR ops.  A second pass, opt-in, on the int32 chain kernel; nothing of the normal run changes.
//
//   path_kernel<C>      extend_kernel's chain walk (seed mode off) whose walker also writes every column's
//                       GACT_PATH_OP_* byte (walk_chain<..., PATH = true>) into the candidate's buffer
//   path_ops_kernel     run-length compaction, one wave per candidate: WRITE = false counts the ops, WRITE = true writes
//                       them at the offsets the exclusive scan of the counts gave
//
// Candidate k of a chunk owns cols[col_off[k], col_off[k+1]), ref_len + query_len bytes: the left phase writes downwards
// from the end, the right phase upwards from the start.  Every column consumes a ref or a query base and no base is
// consumed twice, so the two never meet; the alignment is the left part followed by the right part.
#pragma once

#include "gact_kernels.hpp"

namespace gact {

struct PathArgs {
    uint8_t *cols;                // column bytes of the chunk
    const int64_t *col_off;       // [n + 1]: candidate k owns cols[col_off[k], col_off[k+1])
    int32_t *n_cols;              // [2n]: columns of the left phase, of the right phase (zeroed by the caller)
};

// The path run's chain kernel: extend_kernel's loop (gact_kernels.hpp) with seed mode off and the column cursor.  It is a
// copy and not a template switch on extend_kernel because every way of sharing the body that was tried (an inlined
// template function, by value or by reference, LDS and __restrict__ left in the kernel) changed extend_kernel's own code
// (4,735 -> 4,719 instructions at C = 20, differences throughout the loop).  A change to one loop belongs in the other;
// tests/test_gpu_paths.py and tests/test_gpu_paths_exact.py hold the two together (records byte for byte, and tile by tile
// through the model's CIGARs, at both scorings and at C = 20 and C = 32).
template <int C>
__global__ __launch_bounds__(kBlockThreads, 3) void path_kernel(
    KParams kp, SeqSetDev refs, SeqSetDev qfwd, SeqSetDev qrc,
    const gact_candidate *__restrict__ cands, int n, int rc_from, int same_file,
    gact_overlap *__restrict__ out, ChainQueues cq, PathArgs pa, uint32_t *__restrict__ ws_all)
{
    using G = Geometry<C>;
    __shared__ uint8_t lds[(kBlockThreads / 64) * kGroupsPerWave * G::kGroupLds];
    __shared__ __attribute__((aligned(16))) uint32_t tb_lds[(kBlockThreads / 64) * kGroupsPerWave][kTbScratchWords];

    const WaveCtx w = wave_ctx();
    const int wave_in_block = threadIdx.x >> 6;
    uint8_t *ref_lds_g = lds + (wave_in_block * kGroupsPerWave + w.g) * G::kGroupLds;
    uint8_t *q_lds_g = ref_lds_g + G::kRefLds;
    const uint8_t *ref_lds_lane = ref_lds_g + (kGroup - 1 - w.gl);
    uint32_t *ws = ws_all + (size_t)w.slot * kp.ws_words;
    const bool raw = refs.use_raw | qfwd.use_raw | qrc.use_raw;

    ChainState s;
    s.comp = 0; s.cand = -1; s.phase = 2;
    bool exhausted = false;
    int n_left = 0, n_right = 0;                // columns written so far (the walking lane's)
    __builtin_amdgcn_s_setprio(3);

    for (;;) {
        TilePick pk;
        pk.have = false; pk.R = 0; pk.Q = 0; pk.reverse = false; pk.rp0 = 0; pk.qp0 = 0;
        for (int guard = 0; guard < 3 && !pk.have; guard++) {
            if (s.phase == 2) {
                if (exhausted) break;
                if (!seed_pop(s, cq, w.gl == 0, [](int v) { return __shfl(v, 0, kGroup); }, cands, 0, n, rc_from, refs, qfwd,
                              qrc)) { exhausted = true; break; }
                n_left = 0; n_right = 0;
            }
            pk = chain_pick(s, kp, same_file, out, w.gl == 0);
        }
        if (!__any(pk.have)) {
            if (__all(exhausted && s.phase == 2)) break;
            continue;
        }
        GroupTile gt{pk.R, pk.Q, pk.have ? s.first_tile : 0, 0};

        const bool active = gt.R > 0 && gt.Q > 0;
        const WavePlan wp = align_starts(last_step<C>(gt.R, gt.Q),
                                         first_pointer_step<C>(gt.R, gt.Q, kp.early, gt.first), active, gt.shift);
        uint32_t qb[C];
        load_tile<C>(refs, s.comp ? qrc : qfwd, raw, pk.rp0, pk.qp0, gt.R, gt.Q, pk.reverse, w.gl, ref_lds_g,
                     q_lds_g, qb, gt.shift);
        wave_sync();
        const bool any_first = __any(gt.first != 0);

        PassOut po;
        __builtin_amdgcn_s_setprio(0);
        if (any_first) dp_pass<C, true>(kp, w.gl, ref_lds_lane, qb, gt, wp.T_end, wp.tB, ws, po);
        else           dp_pass<C, false>(kp, w.gl, ref_lds_lane, qb, gt, wp.T_end, wp.tB, ws, po);
        __builtin_amdgcn_s_setprio(3);
        po.tB -= gt.shift;

        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // see align_tiles_kernel

        if (pk.have) {
            s.n_tiles++;
            s.cells += (int64_t)gt.R * gt.Q;
            int i0 = gt.R, j0 = gt.Q;
            bool stop = false;
            if (s.first_tile) {
                i0 = po.bi; j0 = po.bj;
                stop = chain_first_tile(s, kp, gt.R, gt.Q, po.best, po.bi, po.bj);
            }
            int ref_steps = 0, query_steps = 0, nst = 0;
            ScoreWalk wk;
            wk.load(s);
            if (!stop && w.gl == 0) {
                // this tile's columns go on where the phase's last tile left off
                const int64_t b0 = pa.col_off[s.cand], b1 = pa.col_off[s.cand + 1];
                const bool left = s.phase == 0;
                PathCursor pc;
                pc.p = left ? pa.cols + b1 - 1 - n_left : pa.cols + b0 + n_right;
                pc.lo = pa.cols + b0;
                pc.hi = pa.cols + b1 - n_left;
                pc.dir = left ? -1 : 1;
                uint8_t *const start = pc.p;
                const int l0 = (j0 - 1) / C;
                walk_chain<C, 0, C / 4, kGroup, true>(ws, tb_lds[wave_in_block * kGroupsPerWave + w.g], i0, j0, l0,
                                                      (j0 - 1) - l0 * C, i0 + l0 - po.tB, kp.early, ref_lds_g + kGroup + gt.shift,
                                                      1, q_lds_g, s.phase, kp, wk, ref_steps, query_steps, nst, 0, nullptr,
                                                      -1, nullptr, &pc);
                const int cols = (int)((pc.p - start) * pc.dir);
                if (left) n_left += cols; else n_right += cols;
                pa.n_cols[2 * s.cand] = n_left;
                pa.n_cols[2 * s.cand + 1] = n_right;
            }
            chain_advance(s, stop, wk, ref_steps, query_steps, nst, 0);
        }
        wave_sync();
    }
}

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
