// gact_chain_kernel.hpp -- the persistent chain kernel (int32 scores): the loop that takes a candidate through its tiles,
// written once.  What differs between the runs that use it -- where a walk's columns go, what happens to a chain once
// its first tile is done -- is a Sink, a small struct passed by value:
//
//   SeedSink     (gact_kernels.hpp)   the int32 run and the int32 seed launch: nothing is kept of a walk but its steps
//   ColumnSink   (gact_path.hpp)      the path run: every column's GACT_PATH_OP_* byte into the candidate's buffer
//   CountSink    (gact_summary.hpp)   the summary run: columns and runs of each kind, counted in registers
//
// A Sink answers five calls, all __device__ __forceinline__:
//   first()                        index of the first candidate of the launch
//   begin()                        the group has popped a new candidate: per-candidate state starts over
//   picked(s, cq, have, leader)    after chain_pick
//   walk<C>(t, s, kp, wk, ...)     the walking lane's walk_chain of tile t (TileWalk, gact_kernels.hpp), with this run's
//                                  template switches and what surrounds it
//   advanced(s, cq, kp, leader)    after chain_advance
#pragma once

#include "gact_kernels.hpp"

namespace gact {

// Per-group state mirrors the locals of GACT() (gact_chain.hpp); every lane of the group carries an identical copy,
// only the traceback runs on one lane and its results are broadcast.
template <int C, class Sink>
__global__ __launch_bounds__(kBlockThreads, 3) void chain_kernel(
    KParams kp, SeqSetDev refs, SeqSetDev qfwd, SeqSetDev qrc,
    const gact_candidate *__restrict__ cands, int n, int rc_from, int same_file,
    gact_overlap *__restrict__ out, ChainQueues cq, Sink sink, uint32_t *__restrict__ ws_all)
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
    sink.begin();                               // (whatever the host passed in the sink's per-candidate members is not read)
    __builtin_amdgcn_s_setprio(3);

    for (;;) {
        // ---- pick the next tile of this group, finishing / fetching candidates on the way
        TilePick pk;
        pk.have = false; pk.R = 0; pk.Q = 0; pk.reverse = false; pk.rp0 = 0; pk.qp0 = 0;
        for (int guard = 0; guard < 3 && !pk.have; guard++) {
            if (s.phase == 2) {
                if (exhausted) break;
                if (!seed_pop(s, cq, w.gl == 0, [](int v) { return __shfl(v, 0, kGroup); }, cands, sink.first(), n, rc_from, refs,
                              qfwd, qrc)) { exhausted = true; break; }
                sink.begin();
            }
            pk = chain_pick(s, kp, same_file, out, w.gl == 0);
            sink.picked(s, cq, pk.have, w.gl == 0);
        }
        if (!__any(pk.have)) {
            // nobody in this wave has a tile: either all exhausted, or some group
            // still has transitions pending (guard ran out) -- loop again for those
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
        __builtin_amdgcn_s_setprio(0);          // throughput work; the serial sections around it run at priority 3
        if (any_first) dp_pass<C, true>(kp, w.gl, ref_lds_lane, qb, gt, wp.T_end, wp.tB, ws, po);
        else           dp_pass<C, false>(kp, w.gl, ref_lds_lane, qb, gt, wp.T_end, wp.tB, ws, po);
        __builtin_amdgcn_s_setprio(3);
        po.tB -= gt.shift;      // the traceback indexes steps in the tile's own (undelayed) time

        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // see align_tiles_kernel

        // ---- consume the tile exactly as gact.cpp:95-133 / :158-194 do
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
                const int l0 = (j0 - 1) / C;
                const TileWalk t{ws, tb_lds[wave_in_block * kGroupsPerWave + w.g], i0, j0, l0, (j0 - 1) - l0 * C,
                                 i0 + l0 - po.tB, ref_lds_g + kGroup + gt.shift, q_lds_g};
                sink.template walk<C>(t, s, kp, wk, ref_steps, query_steps, nst);
            }
            chain_advance(s, stop, wk, ref_steps, query_steps, nst, 0);
            sink.advanced(s, cq, kp, w.gl == 0);
        }
        wave_sync();
    }
}

}  // namespace gact
