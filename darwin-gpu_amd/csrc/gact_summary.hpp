// gact_summary.hpp -- the summary run (gact_hip_candidates_summaries): what a caller that wants identity, NM or a PAF line
// needs of every selected candidate's alignment -- columns and CIGAR ops of each kind -- without the alignment itself.  A
// second pass, opt-in, on the int32 chain kernel, as the path run (gact_path.hpp) is; nothing of the normal run changes.
//
//   summary_kernel<C>   extend_kernel's chain walk (seed mode off) whose walker counts every column's kind and every
//                       run's start (walk_chain<..., COUNT = true>) in the walking lane's registers
//
// No column buffers, no compaction, no chunks: one launch for any selection, 32 bytes out per candidate.  sums[k] is what
// reducing the ops of gact_hip_candidates_paths gives for the same candidate (tests/test_gpu_summaries.py holds the two
// together): the alignment is the left part followed by the right part, and a run that goes on across a tile boundary or
// across the junction of the two parts is one run (PathCount, gact_chain.hpp).
#pragma once

#include "gact_kernels.hpp"

namespace gact {

// The summary run's chain kernel: path_kernel's loop (gact_path.hpp; a copy of extend_kernel's for the reason given there)
// with the counters where path_kernel has its column cursor.  A change to one loop belongs in the others.
template <int C>
__global__ __launch_bounds__(kBlockThreads, 3) void summary_kernel(
    KParams kp, SeqSetDev refs, SeqSetDev qfwd, SeqSetDev qrc,
    const gact_candidate *__restrict__ cands, int n, int rc_from, int same_file,
    gact_overlap *__restrict__ out, ChainQueues cq, gact_path_summary *__restrict__ sums, uint32_t *__restrict__ ws_all)
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
    PathCount pc{};                             // the candidate's counts so far (the walking lane's)
    bool in_right = false;                      // the right phase has taken over pc.prev
    __builtin_amdgcn_s_setprio(3);

    for (;;) {
        TilePick pk;
        pk.have = false; pk.R = 0; pk.Q = 0; pk.reverse = false; pk.rp0 = 0; pk.qp0 = 0;
        for (int guard = 0; guard < 3 && !pk.have; guard++) {
            if (s.phase == 2) {
                if (exhausted) break;
                if (!seed_pop(s, cq, w.gl == 0, [](int v) { return __shfl(v, 0, kGroup); }, cands, 0, n, rc_from, refs, qfwd,
                              qrc)) { exhausted = true; break; }
                pc = PathCount{};
                in_right = false;
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
                // the right phase's first column comes after the column the left phase emitted first (none: no column)
                if (s.phase == 1 && !in_right) { in_right = true; pc.prev = pc.first; }
                const int l0 = (j0 - 1) / C;
                walk_chain<C, 0, C / 4, kGroup, false, true>(ws, tb_lds[wave_in_block * kGroupsPerWave + w.g], i0, j0, l0,
                                                             (j0 - 1) - l0 * C, i0 + l0 - po.tB, kp.early,
                                                             ref_lds_g + kGroup + gt.shift, 1, q_lds_g, s.phase, kp, wk, ref_steps,
                                                             query_steps, nst, 0, nullptr, -1, nullptr, nullptr, &pc);
                // (after every tile, as path_kernel writes its column counts: the chain's end is seen by chain_pick alone)
                int4 *dst = reinterpret_cast<int4 *>(sums + s.cand);
                dst[0] = make_int4(pc.n_eq, pc.n_x, pc.n_i, pc.n_d);
                dst[1] = make_int4(pc.r_eq, pc.r_x, pc.r_i, pc.r_d);
            }
            chain_advance(s, stop, wk, ref_steps, query_steps, nst, 0);
        }
        wave_sync();
    }
}

}  // namespace gact
