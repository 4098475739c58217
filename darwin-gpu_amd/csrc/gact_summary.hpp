// gact_summary.hpp -- the summary run (gact_hip_candidates_summaries): what a caller that wants identity, NM or a PAF line
// needs of every selected candidate's alignment -- columns and CIGAR ops of each kind -- without the alignment itself.  A
// second pass, opt-in, on the int32 chain kernel, as the path run (gact_path.hpp) is; nothing of the normal run changes.
//
//   CountSink           chain_kernel's chain walk (gact_chain_kernel.hpp) whose walker counts every column's kind and every
//                       run's start (walk_chain<..., COUNT = true>) in the walking lane's registers
//
// No column buffers, no compaction, no chunks: one launch for any selection, 32 bytes out per candidate.  sums[k] is what
// reducing the ops of gact_hip_candidates_paths gives for the same candidate (tests/test_gpu_summaries.py holds the two
// together): the alignment is the left part followed by the right part, and a run that goes on across a tile boundary or
// across the junction of the two parts is one run (PathCount, gact_chain.hpp).
#pragma once

#include "gact_chain_kernel.hpp"

namespace gact {

// The summary run's sink of chain_kernel (gact_chain_kernel.hpp): the counters where the path run has its column cursor.
struct CountSink {
    gact_path_summary *sums;
    PathCount pc;                               // the candidate's counts so far (the walking lane's)
    bool in_right;                              // the right phase has taken over pc.prev

    __device__ __forceinline__ int first() const { return 0; }
    __device__ __forceinline__ void begin() { pc = PathCount{}; in_right = false; }
    __device__ __forceinline__ void picked(const ChainState &, const ChainQueues &, bool, bool) const {}
    template <int C>
    __device__ __forceinline__ void walk(const TileWalk &t, const ChainState &s, const KParams &kp, ScoreWalk &wk,
                                         int &ref_steps, int &query_steps, int &nst)
    {
        // the right phase's first column comes after the column the left phase emitted first (none: no column)
        if (s.phase == 1 && !in_right) { in_right = true; pc.prev = pc.first; }
        walk_chain<C, 0, C / 4, kGroup, false, true>(t.ws, t.scratch, t.R, t.Q, t.l0, t.c0, t.k0, kp.early, t.rrow, 1, t.qrow,
                                                     s.phase, kp, wk, ref_steps, query_steps, nst, 0, nullptr, -1, nullptr,
                                                     nullptr, &pc);
        // (after every tile, as ColumnSink writes its column counts: the chain's end is seen by chain_pick alone)
        int4 *dst = reinterpret_cast<int4 *>(sums + s.cand);
        dst[0] = make_int4(pc.n_eq, pc.n_x, pc.n_i, pc.n_d);
        dst[1] = make_int4(pc.r_eq, pc.r_x, pc.r_i, pc.r_d);
    }
    __device__ __forceinline__ void advanced(const ChainState &, const ChainQueues &, const KParams &, bool) const {}
};

}  // namespace gact
