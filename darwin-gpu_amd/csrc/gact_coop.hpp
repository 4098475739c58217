// gact_coop.hpp -- the split linear-gap main launch with COOPERATIVE, BATCHED traceback walks (round 5).
//
// What round 5 measured first (gact_roles.hpp, profiles/r05/): taking the walk off the DP waves -- dedicated walker waves, two
// banks of tiles per DP wave -- does not make the launch faster.  The machine is bound by VALU issue (one wave64 instruction
// per ~4 cycles and SIMD, two waves inside a pass saturate it), so a wave that
// idles through its walk costs nothing the other waves of its SIMD do not make up, and a walker wave that runs all the time
// with a few lanes at work executes as many instructions as the 8-lane walks it replaced (SQ_INSTS_VALU 1.608e10 against
// 1.656e10).  What does help is FEWER instructions: the walk (align.cpp:185-230) is 213 dependent steps of ~45 VALU
// instructions per tile, executed in extend_p16_kernel with 8 of a wave's 64 lanes at work -- 16-18 % of the launch's
// instructions.  So here
//
//   * every wave of a block (4 waves, 3 blocks per CU: the shape of extend_p16_kernel) is a DP wave with TWO banks of
//     eight tiles; after a pass it posts the bank's eight walks as jobs in LDS and goes on with its other bank;
//   * nobody walks until somebody needs a result: a wave that comes back to a bank whose jobs are still unclaimed takes the
//     block's walk lock and walks EVERY posted job of the block -- its own and the other three waves', up to 64, one per
//     lane -- in one instruction stream, then goes on.  A walk batch is ~30 jobs in the steady state: the walk's
//     instructions per tile drop by that factor over 8;
//   * the walk itself is walk_chain_lin's, move for move (same cells, same order, same stop tests, same band rule), as
//     straight-line code: eight moves per trip without a branch, finished lanes riding along with their updates masked,
//     positions carried from move to move (gact_walk_pos.hpp).  The bases of a cell come out of the loader's
//     staging words, which stay in LDS until their bank is loaded again.
//
// Hand-over (gact_two_bank.hpp: the two-bank DP wave, its job record and bank words, shared with the role launch): a job's
// fields are written before its state word (posted), a lane claims a job with a compare-and-swap on the state word, a
// result is written before the state word says done.
// Progress: a wave that needs a result either finds it, or finds the job unclaimed and walks it itself (after the lock), or
// finds it claimed -- then the lock holder is walking it and finishes in bounded time.  A watchdog turns a hang into a
// reported error (bit 30 of the band_redos counter).
#pragma once

#include "gact_two_bank.hpp"
#include "gact_walk_pos.hpp"

namespace gact {

constexpr int kCoopBanks = 2;
constexpr int kCoopJobs = (kBlockThreads / 64) * 8 * kCoopBanks;       // tile slots of a block x banks = the lanes of a walking wave
static_assert(kCoopJobs == 64, "a walking wave serves every job of its block, one per lane");
constexpr int kCoopCacheStride = 36;                                   // dwords of region cache per walking lane (32 used)

// a job and its result (gact_two_bank.hpp)
struct CoopJob : TileJob { int pad_; };      // posting wave -> walking lane
using CoopDone = TileDone;
// state word of a job: (sequence number << 2) | phase; phase 1 posted, 2 claimed by a walking lane, 3 done

template <class L> __host__ constexpr size_t coop_ws_words(int blocks) { return (size_t)blocks * (kBlockThreads / 64) * kCoopBanks * two_bank_words<L>(); }

// One batch: lane j claims job j if it is posted, all claimed jobs are walked in lock step, results written.
template <class L>
__device__ __forceinline__ void coop_walk_batch(const KParams &kp, const uint32_t *__restrict__ ws_all, const CoopJob *jobs, uint32_t *jstate,
                                                CoopDone *done, const uint32_t *stage_all, uint32_t *cache_all)
{
    constexpr int CW = L::kWalkCols, QN = L::kWalkQuads, ROW = kWsRow;
    constexpr int kSeg = StageGeom<L::kSlotsPerLane, L::kLanes>::kSeg;
    constexpr uint32_t kM = 3u, kI = 2u, kD = 1u;               // align.h:23 numbering, as the pass tags them
    typedef __attribute__((address_space(3))) const uint8_t LdsByte;
    typedef __attribute__((address_space(3))) const uint32_t LdsWord;
    const int lane = threadIdx.x & 63;
    uint32_t *scratch = cache_all + lane * kCoopCacheStride;
    LdsByte *cache = (LdsByte *)scratch;
    LdsWord *stage = (LdsWord *)stage_all;
    const int early = kp.early;
    int v_gap, v_mism, v_match;
    asm volatile("s_nop 1\n\tv_mov_b32 %0, %1" : "=v"(v_gap) : "s"(__builtin_amdgcn_readfirstlane(kp.ext)));
    asm volatile("s_nop 1\n\tv_mov_b32 %0, %1" : "=v"(v_mism) : "s"(__builtin_amdgcn_readfirstlane(kp.mismatch)));
    asm volatile("s_nop 1\n\tv_mov_b32 %0, %1" : "=v"(v_match) : "s"(__builtin_amdgcn_readfirstlane(kp.match)));

    // ---- claim
    const uint32_t st0 = __hip_atomic_load(&jstate[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    bool active = false;
    if ((st0 & 3u) == 1u) active = atomicCAS(&jstate[lane], st0, st0 + 1u) == st0;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (!__any(active)) return;
    int kA = 0, nlim_i = 0, nlim_j = 0, nis = 0, njs = 0, v0 = 0, band_lim = -1;
    uint32_t ws_off = 0;
    int rpos0 = 0, qpos0 = 0, dir = 0, seg = 0;
    int l = 0, c = 0, k = 0;
    bool go = false, redo = false;
    if (active) {
        const CoopJob jb = jobs[lane];
        const int R = jb.R, Q = jb.Q;
        ws_off = jb.ws_off; v0 = jb.v0; band_lim = jb.band_lim;
        int l0, c0, k0;
        L::walk_start(R, Q, 0, l0, c0, k0);                       // (lane and column of (R, Q); the step comes with the job)
        k0 = jb.k0;
        kA = k0 - l0;
        nlim_i = -imin(early, R); nlim_j = -imin(early, Q);
        const bool rev = (jb.where >> 16) & 1u;
        seg = (int)(jb.where >> 17);
        dir = rev ? -1 : 1;                                        // a step up the tile (nis - 1): slice index + 1 when reversed
        rpos0 = (int)(jb.where & 0xffu) + (rev ? 0 : R - 1);
        qpos0 = (int)((jb.where >> 8) & 0xffu) + (rev ? 0 : Q - 1);
        l = l0; c = c0; k = k0;
        go = (R >= 1) & (Q >= 1) & (early > 0) & (v0 != 0);
    }
    uint32_t cur = 0, rcode = 0, qcode = 0;
    TbRegion<CW> rg;
    rg.l0 = 0; rg.fbase[0] = rg.fbase[1] = rg.fbase[2] = 0; rg.qbase0 = 0;
    // What a trip (a refill and its eight moves) keeps, gact_walk_pos.hpp: the column relative to lane rg.l0 (cr < 0: in
    // the lane before), its clamp, kA + rg.l0, and the byte address of column 0's half-word in the region cache for lane
    // rg.l0 (off_a) and what the lane before adds to it (off_d).  A finished lane keeps those of its last refill.
    int cr = 0, cr_min = 0, k_lane = 0, dv = 0;
    uint32_t off_a = 0, off_d = 0;
    const uint32_t cache_a = (uint32_t)(uintptr_t)cache;                   // LDS byte addresses: the lane's region cache,
    const uint32_t seg_a = (uint32_t)(uintptr_t)(stage + seg);             // the tile's ref segment (the query's: kSeg words on)
    // (twice the bit position of a base from LDS address 0: rpos0 + dir * nis bases into the segment, walk_pos2)
    const int dir2 = 2 * dir, rfix2 = 2 * rpos0 + 8 * (int)seg_a, qfix2 = 2 * qpos0 + 8 * (int)seg_a;
    // The three LDS reads of a cell -- its column's half-word of pointer codes out of the region cache, the staged words
    // of its two bases (load_pair_packed: base d of a slice sits at bit 2 * (16 kFront + bit0 + d) of its segment) --
    // are issued together; what does not need them runs before land() waits for all three at once.
    uint32_t pw = 0, rw = 0, qw = 0;
    int rp2 = 0, qp2 = 0;
    auto issue = [&]() {
        const uint32_t pa = ((uint32_t)k >> 3 << 5) + (((uint32_t)cr << 1) + off_a) + ((uint32_t)walk_lane_before(cr) & off_d);
        rp2 = walk_pos2(rfix2, dir2, nis); qp2 = walk_pos2(qfix2, dir2, njs);   // nis, njs <= 0; forward slices are walked downwards
        const uint32_t ra = ((uint32_t)rp2 >> 3) & ~3u, qa = ((uint32_t)qp2 >> 3) & ~3u;
        asm volatile("ds_read_u16 %0, %3\n\t"
                     "ds_read_b32 %1, %4\n\t"
                     "ds_read_b32 %2, %5 offset:%6"
                     : "=&v"(pw), "=&v"(rw), "=&v"(qw) : "v"(pa), "v"(ra), "v"(qa), "n"(4 * kSeg) : "memory");
    };
    auto land = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pw), "+v"(rw), "+v"(qw) :: "memory");
        // (v_bfe_u32 takes the low five bits of its offset: 2 * (position & 15) of a base; a half-word's rows run from bit 14 down)
        cur = __builtin_amdgcn_ubfe(pw, (uint32_t)(__mul24(k, -2) + 14) & 15u, 2u);
        rcode = __builtin_amdgcn_ubfe(rw, (uint32_t)rp2, 2u);
        qcode = __builtin_amdgcn_ubfe(qw, (uint32_t)qp2, 2u);
    };
#ifdef GACT_STAMPS
    unsigned long long n_trips = 0, n_lane_trips = 0;
#endif
    // ---- refill (every walking lane at the same trip: one memory round trip), then eight moves: walk_chain_lin's, move for
    //      move, as straight-line code.  `go` and `redo` are data: a lane that has finished rides along to the end of the
    //      trip and every update of its state is masked by `go`, so its nis, njs, dv, l, c, k and redo stay what they were --
    //      no branch inside a move, one wave-uniform test per trip (`go` only ever falls).
    while (__any(go)) {
        if (go) {
            tb_refill_oct<CW, QN, ROW>(ws_all, ws_off, scratch, l, c, k, rg);
            off_a = cache_a + (uint32_t)(4 * (-8 * rg.fbase[0] - 4 * rg.qbase0));
            off_d = cache_a + (uint32_t)(4 * (16 - 8 * rg.fbase[1] - 4 * (QN - 2)) + 2 * CW) - off_a;
            walk_trip_begin<CW>(l, c, cr, cr_min);
            k_lane = kA + l;
            issue();
            land();
        }
#pragma unroll
        for (int m = 0; m < 8; m++) {
#ifdef GACT_STAMPS
            n_trips += __any(go) ? 1ull : 0ull; n_lane_trips += (unsigned long long)__builtin_popcountll(__ballot(go));
#endif
            const bool diag = cur == kM;
            const int sub = rcode == qcode ? v_match : v_mism;
            const int cost = diag ? sub : v_gap;
            dv += go ? cost : 0;
            nis -= (int)(go & (cur != kD));
            const int dj = (int)(go & (cur != kI));
            njs -= dj;
            walk_col_left(cr, cr_min, dj);
            k = imax(k_lane + nis + walk_lane_before(cr), 0);
            if (m == 7) {
                // (the next refill is due: still a refill's worth of moves inside the stored band?  gact_lin.hpp LinBand)
                redo = redo | (go & (band_lim >= 0) & ((unsigned)(nis - njs + band_lim) > (unsigned)(2 * band_lim)));
            } else {
                issue();
            }
            go = go & !((diag && dv == v0) || nis <= nlim_i || njs <= nlim_j || redo);
            if (m != 7) land();
        }
        walk_trip_end<CW>(rg.l0, cr, l, c);
    }
    if (active) {
        done[lane].ref_steps = -nis; done[lane].query_steps = -njs; done[lane].dv = dv; done[lane].redo = redo ? 1 : 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __hip_atomic_store(&jstate[lane], st0 + 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#ifdef GACT_STAMPS
    {
        const unsigned long long n_jobs = (unsigned long long)__builtin_popcountll(__ballot(active));
        if (lane == 0) { atomicAdd(&g_coop_counts[0], 1ull); atomicAdd(&g_coop_counts[1], n_trips); atomicAdd(&g_coop_counts[2], n_lane_trips);
                         atomicAdd(&g_coop_counts[3], n_jobs); }
    }
#endif
}

// ---------------------------------------------------------------------------
// L: SplitLayoutLin<7, 13> (2-bit sets, linear gaps).  TWO_SETS as in extend_p16_kernel (overlapped seeding).
template <class L, bool TWO_SETS = false>
__global__ __launch_bounds__(kBlockThreads, 3) void extend_coop_kernel(
    KParams kp, P16Consts kc, SeqSetDev refs, SeqSetDev qfwd, SeqSetDev qrc,
    int same_file, gact_overlap *__restrict__ out, ChainQueues cq,
    uint32_t *__restrict__ ws_all)
{
    using G = typename L::G;
    constexpr int LANES = L::kLanes;
    static_assert(LANES == kGroup && L::kWalkFmt == 3 && L::kEndAligned, "the split linear-gap layout");
    constexpr int kGroupsOfWave = 64 / LANES;
    constexpr int kGroupsPerBlock = (kBlockThreads / 64) * kGroupsOfWave;
    constexpr int kStageWords = StageGeom<L::kSlotsPerLane, LANES>::kWords;
    constexpr int kSeg = StageGeom<L::kSlotsPerLane, LANES>::kSeg;
    static_assert(((kGroupsPerBlock * kCoopBanks * kStageWords) >> 15) == 0, "stage index fits CoopJob::where");
    constexpr int kRefBytes = (G::kRefBytes + 15) & ~15;          // the ref stream alone: the walker keeps no query bytes
    __shared__ __attribute__((aligned(16))) uint8_t lds[kGroupsPerBlock * kRefBytes];
    __shared__ ChainState chain_lds[kGroupsPerBlock][kCoopBanks][kSlots];
    // the loader's staging words of a group's two tiles, per bank: they stay until the bank is loaded again -- a walking
    // lane reads the bases of its cells from them
    __shared__ __attribute__((aligned(16))) uint32_t stage_lds[kGroupsPerBlock][kCoopBanks][kStageWords];
    __shared__ __attribute__((aligned(16))) CoopJob jobs[kCoopJobs];
    __shared__ CoopDone done[kCoopJobs];
    __shared__ uint32_t jstate[kCoopJobs];
    __shared__ __attribute__((aligned(16))) uint32_t cache_lds[kCoopJobs * kCoopCacheStride];
    __shared__ int bank_lds[kGroupsPerBlock][kCoopBanks][kBankWords];   // (BankWord; in flight: the jobs' state word when done)
    __shared__ uint32_t walk_lock;

    uint32_t *const lin_lut = LinLutLds<L::kLutWords>::get();      // the pass's table of look-up words (gact_lin.hpp 8.)
    for (int n = threadIdx.x; n < kCoopJobs; n += kBlockThreads) jstate[n] = 0;
    if (threadIdx.x == 0) walk_lock = 0;
    lin_lut_fill_for_pass<L>(lin_lut, kc, (int)threadIdx.x);
    __syncthreads();

    const int wave_in_block = threadIdx.x >> 6;
    WaveCtx w;
    {
        const int lane = threadIdx.x & 63;
        w.gl = lane & (LANES - 1);
        w.g = lane / LANES;
        w.slot = (blockIdx.x * (kBlockThreads / 64) + wave_in_block) * kGroupsOfWave + w.g;
        w.n_slots = gridDim.x * (kBlockThreads / 64) * kGroupsOfWave;
    }
    const int group_in_block = wave_in_block * kGroupsOfWave + w.g;
    uint8_t *ref8 = lds + group_in_block * kRefBytes;
    uint8_t *q8 = ref8;                                                 // (never written: load_pair_packed<..., false>)
    const uint16_t *ref16_lane = reinterpret_cast<const uint16_t *>(ref8) + (L::kRow0 - 1 - w.gl);
    // a wave's pointer words: [bank][flush block][uint4 n][tile A | tile B][the wave's 64 lanes]
    uint32_t *ws_wave = ws_all + (size_t)(blockIdx.x * (kBlockThreads / 64) + wave_in_block) * (kCoopBanks * two_bank_words<L>());
    // this lane's job of bank b: ((group in block) * 2 + slot) * 2 + b   (lanes 0 and 1 of a group: slots A and B)
    const int job_base = (group_in_block * kSlots + (w.gl & 1)) * kCoopBanks;

    for (int b = 0; b < kCoopBanks; b++)
        if (w.gl < kSlots) { chain_lds[group_in_block][b][w.gl].phase = 2; chain_lds[group_in_block][b][w.gl].cand = -1; }
    bank_reset(&bank_lds[group_in_block][0][0], w.gl == 0);
    wave_sync();
    bool exhausted = false;
    int my_bucket = 0;
    const int bucket_first = main_first_bucket(cq);
    bool second_set = false;
    constexpr bool one_set = !TWO_SETS;
    int idle_polls = 0;
    // (the ranking against the longest chain running: every kRankEvery-th tile, the waves of a launch taking turns; the first tile always)
    int rank_turn = 0, rank_cached = 0;
    int bank = 0;
    __builtin_amdgcn_s_setprio(3);
    GACT_STAMPS_BEGIN;

    for (;;) {
        ChainState *st = chain_lds[group_in_block][bank];
        GACT_STAMP(t_w0);
        // ---- the results of this bank's walks (posted one pass of the other bank ago): gact.cpp:111-133 / :172-194
        int *bk = bank_lds[group_in_block][bank];
        const uint32_t want = (uint32_t)__builtin_amdgcn_readfirstlane(bk[kBankWant]);       // (the same for the wave's four groups)
        if (want != 0) {
            const int sv_R[kSlots] = {bk[kBankRA], bk[kBankRB]}, sv_Q[kSlots] = {bk[kBankQA], bk[kBankQB]};
            const bool mine = w.gl < kSlots && ((w.gl & 1) ? sv_R[1] : sv_R[0]) > 0;
            const int my_job = job_base + bank;
            // somebody has to walk: whoever needs a result first walks every posted job of the block (see the header)
            const unsigned long long wd0 = __builtin_amdgcn_s_memrealtime();
            for (;;) {
                const uint32_t s = mine ? __hip_atomic_load(&jstate[my_job], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : want;
                if (__all(s == want)) break;
                if (__any(mine && (s & 3u) == 1u)) {
                    uint32_t got = 1;
                    if ((threadIdx.x & 63) == 0) got = atomicCAS(&walk_lock, 0u, 1u);
                    got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
                    if (got == 0) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        coop_walk_batch<L>(kp, ws_all, jobs, jstate, done, &stage_lds[0][0][0], cache_lds);
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        if ((threadIdx.x & 63) == 0) __hip_atomic_store(&walk_lock, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        continue;
                    }
                }
                __builtin_amdgcn_s_sleep(4);
                if (__builtin_amdgcn_s_memrealtime() - wd0 > 200000000ull) {      // two seconds: never hang the machine
                    if ((threadIdx.x & 63) == 0) atomicOr(cq.band_redos, 1 << 30);
                    break;
                }
            }
            // (from here to the end of the block: the same text in extend_roles_kernel (gact_roles.hpp) -- as one function it moved spills, profiles/r16)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            int ref_steps = 0, query_steps = 0, nst = 0, redo = 0;
            ScoreWalk wk;
            wk.score = 0; wk.pend_gap = 0; wk.open_flag = 0; wk.have_left = 0; wk.left_first_gap = 0;
            if (mine) {
                const TileDone d = done[my_job];
                wk.load(st[w.gl & 1]);
                wk.score += d.dv;                                        // (open == extend: the gap bookkeeping decides nothing)
                ref_steps = d.ref_steps; query_steps = d.query_steps; nst = d.ref_steps + d.query_steps; redo = d.redo;
            }
#pragma unroll
            for (int h = 0; h < kSlots; h++) {
                if (sv_R[h] > 0) {
                    ChainState s = st[h];
                    if (__shfl(redo, h, LANES)) {
                        s.full = 1;
                        if (w.gl == 0) atomicAdd(cq.band_redos, 1);
                    } else {
                        main_count_advance<LANES>(s, sv_R[h], sv_Q[h], h, wk, ref_steps, query_steps, nst);
                    }
                    wave_sync();
                    if (w.gl == 0) st[h] = s;
                }
                wave_sync();
            }
            wave_sync();
            if (w.gl == 0) bk[kBankWant] = 0;
            wave_sync();
        }
        // ---- the queues are empty: chains move out of bank 1 into free slots of bank 0, so that what is left of the launch runs
        //      one bank per wave -- a chain then advances once per pass + walk, not once per two passes (with both banks
        //      in use to the end the launch of ecoli10x ran 37 ms where its queues were empty after 25).  Bank 1's chains are at
        //      rest here (their results have just been consumed); a free slot of bank 0 has no job in flight even while bank 0
        //      has, and its next pick finds the chain.
        if (bank == 1 && exhausted) {
            ChainState *st0 = chain_lds[group_in_block][0];
#pragma unroll
            for (int h = 0; h < kSlots; h++) {
                const int ph1 = st[h].phase, f0 = st0[0].phase == 2 ? 0 : st0[1].phase == 2 ? 1 : -1;
                wave_sync();
                if (ph1 != 2 && f0 >= 0 && w.gl == 0) {
                    st0[f0] = st[h];
                    st[h].phase = 2; st[h].cand = -1;
                }
                wave_sync();
            }
        }
        GACT_STAMP(t_a);
        // ---- control phase: both slots of the bank pick their next tile
        PairTile pt;
        bool have[kSlots];
        int Tend_h[kSlots], tB_h[kSlots];
        int longest = 0;
        // (the pick below, to the end of the loop over h: one of three copies, the others in extend_p16_kernel (gact_p16.hpp) and extend_roles_kernel (gact_roles.hpp))
#pragma unroll
        for (int h = 0; h < kSlots; h++) {
            ChainState s = st[h];
            TilePick pk;
            pk.have = false; pk.R = 0; pk.Q = 0; pk.reverse = false; pk.rp0 = 0; pk.qp0 = 0;
            for (int guard = 0; guard < 3 && !pk.have; guard++) {
                if (s.phase == 2) {
                    if (exhausted) break;
                    // (bank 1 takes chains to the end: closing it once the launch is down to its classes of fewer than 16 / 24 / 40
                    //  tiles, so that the last chains run one bank per wave, cost 4 / 6 / 9 % with four runs in flight --
                    //  8,223 -> 7,903 / 7,751 / 7,446 GCUPS on ecoli10x, profiles/r05/ab_coop_bank1_throttle.txt.  Nor does it make
                    //  this launch the faster one for a run that has the machine to itself: "lean" waves -- no new chains into the
                    //  other bank of a wave that holds a chain longer than 4..13 sixteenths of the longest one running -- bring
                    //  ecoli10x alone from 37.7 ms to 34.1-35.6 where extend_p16_kernel takes 32.0, and cost pacbio50mb alone
                    //  1-4 %: with twice the chains in flight the queues run dry at 21 ms and twice as many half-done chains are
                    //  left to finish in waves that are no longer full, profiles/r05/ab_coop_lean_waves.txt; closing bank 1 to the
                    //  classes of fewer than 8 ... 48 tiles for such a run: ecoli10x 38.0 -> 32.5-36.3 ms, still behind; pacbio50mb
                    //  alone has no tail to cut -- queues dry at 132.9 of 135.4 ms --, single_run_vs_in_flight_experiments.txt)
                    const int cand = main_pop<TWO_SETS, LANES>(cq, w.gl == 0, bucket_first, my_bucket, second_set);
                    if (cand < 0) {
                        if (second_set || one_set) {
                            exhausted = true;
                            GACT_STAMPS_DO(note_empty());
                        }
                        break;
                    }
                    s = cq.states[cand];
                }
                pk = chain_pick(s, kp, same_file, out, w.gl == 0);
            }
            have[h] = pk.have;
            pt.R[h] = pk.R; pt.Q[h] = pk.Q; pt.reverse[h] = pk.reverse;
            pt.rp0[h] = pk.rp0; pt.qp0[h] = pk.qp0; pt.comp[h] = s.comp; pt.shift[h] = 0;
            pt.full[h] = s.full != 0;
            if (pk.have) longest = imax(longest, chain_remaining(s));
            Tend_h[h] = L::last_step(pk.R, pk.Q);
            tB_h[h] = L::first_pointer_step(pk.R, pk.Q, kp.early);
            wave_sync();
            if (w.gl == 0) st[h] = s;
            wave_sync();
        }
        if (w.gl == 0) {
            bk[kBankRA] = have[0] ? pt.R[0] : 0; bk[kBankQA] = pt.Q[0]; bk[kBankRB] = have[1] ? pt.R[1] : 0; bk[kBankQB] = pt.Q[1];
        }
        const bool any_here = have[0] | have[1];
        if (!__any(any_here)) {
            // nothing for this bank.  The other bank may have walks in flight or chains of its own: go there; with neither,
            // the wave is done once the queues are (or waits for the second set of overlapped seeding, as extend_p16_kernel)
            const bool other_busy = __builtin_amdgcn_readfirstlane(bank_lds[group_in_block][bank ^ 1][kBankWant]) != 0;
            if (!other_busy) {
                const ChainState *so = chain_lds[group_in_block][bank ^ 1];
                if (__all(exhausted && st[0].phase == 2 && st[1].phase == 2 && so[0].phase == 2 && so[1].phase == 2)) break;
                if (!second_set && !one_set) {                  // (the wait of extend_p16_kernel, where it is explained; a third copy in extend_roles_kernel)
                    __builtin_amdgcn_s_sleep(127);
                    if (++idle_polls > 512) { second_set = true; exhausted = true; my_bucket = kBuckets; }
                }
            }
            bank ^= 1;
            continue;
        }
        int T_end, tB;
        pair_starts<L>(kp, have, Tend_h, tB_h, lin_lut, pt, T_end, tB);

        GACT_STAMP(t_b);
        uint32_t qb[L::kSlotsPerLane];
        uint32_t *stage = stage_lds[group_in_block][bank];
        load_pair_packed<L::kSlotsPerLane, LANES, typename L::Cols, false, kLinPadRow>(refs, qfwd, qrc, pt, w.gl, ref8, G::kRefBytes, G::kRow0, q8, G::kTileMax, qb,
                                                                          stage, typename L::Cols{});
        wave_sync();
        GACT_STAMP(t_c);

        const int wave_longest = wave_max_groups<LANES>(longest);
        pass_prio(cq, kp, wave_longest, rank_turn, rank_cached);
        uint32_t *wsA = ws_wave + (size_t)bank * two_bank_words<L>() + (w.g * LANES) * 4;
        uint32_t *wsB = wsA + 64 * 4;
        const uint32_t fin = L::template pass<false>(kc, w.gl, ref16_lane, qb, T_end, tB, wsA, wsB, pt);
        __builtin_amdgcn_s_setprio(3);
        const int v0A = (int)(int16_t)(__shfl(fin, L::fin_lane(pt.Q[0]), LANES) & 0xffffu);
        const int v0B = (int)(int16_t)(__shfl(fin, L::fin_lane(pt.Q[1]), LANES) >> 16);
        GACT_STAMP(t_d);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the pointer stores have reached the L2 before a walker is told
        GACT_STAMP(t_e);

        // ---- post the walks of this bank: lane h of the group writes slot h's job, its state word last
        // (jobs of this wave are numbered 1, 2, ... over both banks; the counter sits in the first group's spare LDS word)
        const uint32_t wave_seq = (uint32_t)__builtin_amdgcn_readfirstlane(bank_lds[wave_in_block * kGroupsOfWave][0][kBankSeq]) + 1u;
        if (w.gl < kSlots && (w.gl ? have[1] : have[0])) {
            post_job<L>(&jobs[job_base + bank], w.gl, kp, pt, tB, w.gl ? wsB : wsA, ws_all, w.gl ? v0B : v0A,
                        (group_in_block * kCoopBanks + bank) * kStageWords);
            __hip_atomic_store(&jstate[job_base + bank], (wave_seq << 2) | 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        wave_sync();
        if (w.gl == 0) bk[kBankWant] = (int)((wave_seq << 2) | 3u);      // what the bank's jobs read when done
        if ((threadIdx.x & 63) == 0) bank_lds[wave_in_block * kGroupsOfWave][0][kBankSeq] = (int)wave_seq;
        wave_sync();
        // (walking eagerly -- a wave that has just posted walks at once when 16 / 24 / 32 / 48 jobs of the block are pending, so that
        //  nobody waits for a result later -- takes the waiting out of the stamps, 24 % -> 9 % of a wave's time, and changes
        //  nothing: pacbio50mb with four runs in flight 8,433 lazy against 8,211 / 8,347 / 8,362 / 8,406,
        //  profiles/r05/ab_coop_eager_batches.txt.  The machine is bound by issue, not by waves that wait: DESIGN 3.13)
        GACT_STAMP(t_f);
        GACT_ACC(0, t_a, t_b); GACT_ACC(1, t_b, t_c); GACT_ACC(2, t_c, t_d); GACT_ACC(3, t_d, t_e);
        GACT_ACC(4, t_w0, t_a); GACT_ACC(5, t_e, t_f);
        GACT_STAMPS_DO(pass_done(T_end - tB + 1));
        bank ^= 1;
    }
    GACT_STAMPS_DO(finish(blockIdx.x * (kBlockThreads / 64) + wave_in_block));
}

}  // namespace gact
