// gact_two_bank.hpp -- the two-bank DP wave: what the cooperative launch (gact_coop.hpp, the default for large and shared
// runs) and the role launch (gact_roles.hpp) have in common.
//
// A DP wave carries TWO banks of eight tiles (2 x 4 groups x {A, B}).  It runs one bank's pass, posts the bank's eight walks
// as jobs in LDS, and goes on with its other bank; when it comes back it takes the walks' results, advances its chains
// (gact.cpp:111-133), picks and loads their next tiles, and so on.  Who walks a job, and how the wave waits for it, is the
// launch's own: walker waves and a sequence word there, whichever wave needs a result first and a state word here.
//
// Hand-over: LDS words only, no barrier inside the loop.  A job's fields are written before the word that publishes it, a
// result's before the word that says it is done (LDS operations of one wave are performed in order; a release fence at
// work-group scope stands between); the pointer words a walk reads were stored by the posting wave and waited for
// (s_waitcnt vmcnt(0)) before the job was posted, and are read past the L1 (sc1) from the XCD's L2 -- both waves sit on
// one CU.  The walker cuts the two bases of a cell out of the loader's staging words (the tile's two slices as they lie
// in the 2-bit image), which stay in LDS until their bank is loaded again: the DP wave's unpacked base arrays belong to
// the other bank by then.
#pragma once

#include "gact_lin.hpp"

namespace gact {

// One walk: posting wave -> walking lane.  (A launch's own record adds what publishes it.)
struct TileJob {
    uint32_t ws_off;             // the tile's pointer words: byte offset of its (wsA | wsB) from ws_all
    int R, Q;
    int k0;                      // stored step of the start cell (L::walk_start)
    int v0;                      // H[R][Q] from the pass
    int band_lim;                // see walk_chain_lin; -1: every block is there
    uint32_t where;              // bits 0-7: staged position of the ref slice's first base, 8-15: the query slice's,
                                 // 16: AlignWithBT's `reverse`, 17-31: dword index of the tile's ref segment in the stage array
};
// ... and its result: walking lane -> posting wave
struct TileDone {
    int ref_steps, query_steps;
    int dv;                      // v0 - v: what the columns of the tile scored
    int redo;
};

// words the linear-gap pass writes per wave and bank: [flush block][uint4 n < QD][kWsRow]
template <class L> constexpr size_t two_bank_words() { return (size_t)L::G::kMaxFlush * L::kWalkQuads * kWsRow * 4; }

// What a bank's pass leaves behind for its consume step lives in LDS, like the chain states (the DP loop owns the register
// file): per group and bank, R and Q of slot A and of slot B (R == 0: no tile) and what the bank's jobs in flight read
// when they are done (0: none in flight).  The wave's job counter sits in the spare word of its first group's bank 0.
enum BankWord { kBankRA, kBankQA, kBankRB, kBankQB, kBankWant, kBankSeq, kBankWords };

__device__ __forceinline__ void bank_reset(int *group_banks, bool lead)
{
    if (lead)
        for (int n = 0; n < 2 * kBankWords; n++) group_banks[n] = 0;
}

// Lane h (< kSlots) of the group fills the job of slot h's tile after its pass; `stage_word`: dword index of the group's
// and bank's staging words in the block's stage array.  The release fence behind the fields is here; the store that
// publishes the job is the caller's next statement.
template <class L>
__device__ __forceinline__ void post_job(TileJob *jb, int h, const KParams &kp, const PairTile &pt, int tB, const uint32_t *ws_tile,
                                         const uint32_t *ws_all, int v0, int stage_word)
{
    constexpr int kSeg = StageGeom<L::kSlotsPerLane, L::kLanes>::kSeg;
    const int Rh = h ? pt.R[1] : pt.R[0], Qh = h ? pt.Q[1] : pt.Q[0], sh = h ? pt.shift[1] : pt.shift[0];
    int l0, c0, k0;
    L::walk_start(Rh, Qh, L::tile_tB(tB, sh), l0, c0, k0);
    jb->ws_off = (uint32_t)((const char *)ws_tile - (const char *)ws_all);
    jb->R = Rh; jb->Q = Qh; jb->k0 = k0; jb->v0 = v0;
    jb->band_lim = ((kp.band & 0xffff) > 0 && !(h ? pt.full[1] : pt.full[0])) ? (kp.band & 0xffff) - kLinWalkSpan : -1;
    const uint32_t seg_index = (uint32_t)(stage_word + (2 * h) * kSeg);
    constexpr uint32_t kFrontBits = 16u * StageGeom<L::kSlotsPerLane, L::kLanes>::kFront;
    jb->where = (kFrontBits + (uint32_t)((h ? pt.rp0[1] : pt.rp0[0]) & 15)) |
                ((kFrontBits + (uint32_t)((h ? pt.qp0[1] : pt.qp0[0]) & 15)) << 8) |
                ((h ? pt.reverse[1] : pt.reverse[0]) ? 1u << 16 : 0u) | (seg_index << 17);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
}

}  // namespace gact
