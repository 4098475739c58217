// gact_pileup.hpp -- per-base pileup and consensus of the reads of GACT_SET_REF from the overlaps' alignments
// (gact_hip_pileup_begin / _add / _finish), the inserted bases and the corrected reads (gact_hip_pileup_begin_ins / _corrected).
//
// What a consumer of an overlapper's alignments does with them: stack every overlap's alignment on its target read, count at
// every position what the other reads say, take the majority (daccord, the polishing rounds behind miniasm).  The path run
// writes every selected candidate's alignment columns into device buffers (gact_path.hpp) right beside the read bytes they
// refer to, so the counting is done there; the rules are stated in include/gact_hip.h.
//
//   pileup_kernel            behind chain_kernel in every chunk of an add, one wave per candidate, 64 columns per step (the shape
//                            of path_ops_kernel).  A first pass counts the ref-consuming and the query-consuming columns (two
//                            ballots per step): the alignment starts at (ae - ref columns, be - query columns).  The second pass
//                            gives each lane its target position r and query position q from the same two ballots under the lane
//                            mask plus the two running bases (wave-uniform); an '=' / 'X' lane loads its query byte (consecutive
//                            lanes of a stretch read consecutive bytes) and adds 1 to that kind and to DEPTH at r, a 'D' lane to
//                            DEL and DEPTH, and an 'I' lane whose left neighbour (the last lane of the step before for lane 0) is
//                            no 'I' adds 1 to INS at min(r, len - 1).  Ordinary no-return vector atomics on uint32: the sums are
//                            the same in whichever order they land, from whichever slot's stream.
//                            A candidate whose record was not emitted, or that has no columns, adds nothing.  Every index is
//                            checked before it is used: a read outside the window or a span outside its reads sets the flag word
//                            and adds nothing.
//                            pileup_kernel<true> (a window with ins_slots = K > 0) also keeps the inserted bases: an 'I' lane has
//                            r and q already, and its index j inside its run is the length of the stretch of set bits directly
//                            below it in the ballot of 'I' lanes, plus a wave-uniform carry (the open run's length at the end of
//                            the step before) when that stretch reaches lane 0; j < K, r < len, a base of kind A C G T: one
//                            more add, to ins[r][j].n[kind].  The lanes with j == K are the runs longer than K, counted per wave.
//                            pileup_kernel<false> is the kernel as it was: a window without slots runs that.
//   pileup_consensus_kernel  one thread per position: the consensus byte
//   pileup_reads_kernel      one wave per read, grid-stride, 64 positions per step: called / changed / deleted / ins_flagged from
//                            the popcounts of four ballots, the highest depth from a per-lane running max reduced once
//   pileup_spell_kernel      the corrected reads, one wave per read, grid-stride, 64 positions per step.  A lane calls its
//                            position's slots (pileup_slots) and reads its consensus byte; what a position gives is at most
//                            K + 1 bytes.  <false>: the read's length, inserted bases, sites, deleted and changed positions from
//                            the popcounts of the ballots "slot j emitted" and "byte kept".  <true>, behind the scan: a position's
//                            offset is the read's start, the carry of the steps before and the same ballots' popcounts under
//                            the lane mask; it writes its bytes there.
//   pileup_scan_kernel       one block: the reads' lengths -> their exclusive scan (block_scan_step; no block waits for another)
// No LDS but the scan's, no look-back, no spinning.  All results are integers and the same on every call.
//
// The counts belong to the engine (Pileup in gact_engine.hip): 32 + 16 K bytes per position of the open window, 13.4 GB for
// 418 Mb of reads at K = 0 -- hence the window.
//
// Included by gact_engine.hip behind every other kernel and behind the engine's definitions, inside its extern "C" block, as
// gact_cover.hpp is.
#pragma once

extern "C++" {                  // (templates: not in gact_engine.hip's extern "C")
namespace gact {

constexpr int kPileupBadRead = 1, kPileupBadSpan = 2;       // bits of the flag word

struct PileupState {                              // 48 bytes behind the counts, zeroed by begin, copied back by every add
    int flag, pad;
    unsigned long long alignments, columns;       // counted since begin
    unsigned long long runs_truncated;            // runs of 'I' longer than the window's ins_slots
    unsigned long long slot_adds, reserved;       // adds to the slots
};

struct PileupWin {
    uint32_t *counts;                             // [positions][8]
    int32_t *n_aln;                               // [n_reads]
    PileupState *state;
    int read_first, n_reads;
    long long base;                               // the window's first base in the ref set's concatenation
    uint32_t *ins;                                // [positions][ins_slots][4]; pileup_kernel<true> only
    int ins_slots;
};

// A C G T -> 0 1 2 3 in either case, anything else -> 4
__device__ __forceinline__ int pileup_kind(uint32_t b)
{
    switch (b | 0x20u) {
        case 'a': return GACT_PILEUP_A;
        case 'c': return GACT_PILEUP_C;
        case 'g': return GACT_PILEUP_G;
        case 't': return GACT_PILEUP_T;
        default: return GACT_PILEUP_OTHER;
    }
}

template <bool kSlots>
__global__ void __launch_bounds__(kPassBlock)
pileup_kernel(const uint8_t *__restrict__ cols, const int64_t *__restrict__ col_off, const int32_t *__restrict__ n_cols,
              const gact_candidate *__restrict__ cands, const gact_overlap *__restrict__ records, int n, SeqSetDev refs,
              SeqSetDev qfwd, SeqSetDev qrc, PileupWin win)
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
        const gact_overlap rec = records[k];
        if (len <= 0 || !rec.emitted) continue;
        const gact_candidate c = cands[k];
        const bool comp = (c.query_id & kCompBit) != 0;
        const int qid = c.query_id & (kCompBit - 1), rid = c.ref_id;
        const SeqSetDev &qs = comp ? qrc : qfwd;
        if (rid < win.read_first || rid >= win.read_first + win.n_reads || rid >= refs.n || qid >= qs.n) {
            if (lane == 0) atomicOr(&win.state->flag, kPileupBadRead);
            continue;
        }
        // ---- where the alignment starts: its end less the columns that consume a base of each read
        int n_r = 0, n_q = 0;
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int t = c0 + lane;
            const uint32_t code = t < len ? path_col(cols, b0, b1, n_left, t) : 0u;
            n_r += __popcll(__ballot(t < len && code != GACT_PATH_OP_I));
            n_q += __popcll(__ballot(t < len && code != GACT_PATH_OP_D));
        }
        const long long r_off = refs.offsets[rid], q_off = qs.offsets[qid];
        const long long r_len = refs.offsets[rid + 1] - r_off, q_len = qs.offsets[qid + 1] - q_off;
        int r_base = rec.ae - n_r, q_base = rec.be - n_q;
        if (r_base < 0 || rec.ae > r_len || q_base < 0 || rec.be > q_len || r_len <= 0) {
            if (lane == 0) atomicOr(&win.state->flag, kPileupBadSpan);
            continue;
        }
        uint32_t *mine = win.counts + (size_t)(r_off - win.base) * 8;       // the read's first position
        const uint8_t *qraw = qs.raw + q_off;
        // ---- the columns
        uint32_t last = 0;                                      // the code of the step before's last column (none: no 'I')
        uint32_t *slots = kSlots ? win.ins + (size_t)(r_off - win.base) * win.ins_slots * 4 : nullptr;
        int open_run = 0, n_slot = 0, n_long = 0;               // (kSlots: the open run's length so far; this alignment's adds
                                                                //  to slots and runs longer than ins_slots; wave-uniform)
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int t = c0 + lane;
            const bool in = t < len;
            const uint32_t code = in ? path_col(cols, b0, b1, n_left, t) : 0u;
            const uint32_t up = __shfl_up(code, 1);
            const uint32_t prev = lane ? up : last;
            const bool on_r = in && code != GACT_PATH_OP_I, on_q = in && code != GACT_PATH_OP_D;
            const uint64_t m_r = __ballot(on_r), m_q = __ballot(on_q);
            const int r = r_base + __popcll(m_r & below_me), q = q_base + __popcll(m_q & below_me);
            if (on_r) {
                const int kind = code == GACT_PATH_OP_D ? GACT_PILEUP_DEL : pileup_kind(qraw[q]);
                uint32_t *at = mine + (size_t)r * 8;
                atomicAdd(at + kind, 1u);
                atomicAdd(at + GACT_PILEUP_DEPTH, 1u);
            } else if (in && prev != GACT_PATH_OP_I) {          // the first column of a run of 'I'
                const long long rr = r < r_len - 1 ? r : r_len - 1;
                atomicAdd(mine + (size_t)rr * 8 + GACT_PILEUP_INS, 1u);
            }
            if constexpr (kSlots) {                             // the inserted base: column j of its run, in front of r
                const bool is_i = in && !on_r;
                const uint64_t m_i = __ballot(is_i);
                const uint64_t gaps = ~m_i & below_me;          // the lanes below mine that are no 'I'
                const int j = gaps ? lane - (64 - __clzll(gaps)) : lane + open_run;
                const int kind = is_i && j < win.ins_slots && r < r_len ? pileup_kind(qraw[q]) : GACT_PILEUP_OTHER;
                if (kind < GACT_PILEUP_OTHER) atomicAdd(slots + ((size_t)r * win.ins_slots + j) * 4 + kind, 1u);
                n_slot += __popcll(__ballot(kind < GACT_PILEUP_OTHER));
                n_long += __popcll(__ballot(is_i && j == win.ins_slots));
                open_run = ~m_i ? __clzll(~m_i) : open_run + 64;                // the 'I' lanes at the step's top
            }
            r_base += __popcll(m_r);
            q_base += __popcll(m_q);
            last = __shfl(code, 63);
        }
        if (lane == 0) {
            atomicAdd(&win.n_aln[rid - win.read_first], 1);
            atomicAdd(&win.state->alignments, 1ull);
            atomicAdd(&win.state->columns, (unsigned long long)len);
            if (kSlots && n_slot) atomicAdd(&win.state->slot_adds, (unsigned long long)n_slot);
            if (kSlots && n_long) atomicAdd(&win.state->runs_truncated, (unsigned long long)n_long);
        }
    }
}

// the consensus byte of a position with the counts n, the read's own byte there
__device__ __forceinline__ uint8_t pileup_call(const uint32_t *n, uint8_t own, uint32_t min_depth)
{
    if (n[GACT_PILEUP_DEPTH] < min_depth) return own;
    const uint32_t five[5] = {n[GACT_PILEUP_A], n[GACT_PILEUP_C], n[GACT_PILEUP_G], n[GACT_PILEUP_T], n[GACT_PILEUP_DEL]};
    uint32_t best = 0;
    for (int k = 0; k < 5; k++) best = five[k] > best ? five[k] : best;
    if (best == 0) return own;
    int pick = 4;
    for (int k = 4; k >= 0; k--) pick = five[k] == best ? k : pick;          // the first of the tied kinds in the order A C G T DEL
    const int mine = pileup_kind(own);
    if (mine < 4 && five[mine] == best) pick = mine;
    return (uint8_t)"ACGT-"[pick];
}

__global__ void __launch_bounds__(kPassBlock)
pileup_consensus_kernel(const uint32_t *__restrict__ counts, const uint8_t *__restrict__ own, long long positions, uint32_t min_depth,
                        uint8_t *__restrict__ cons)
{
    const long long step = (long long)gridDim.x * kPassBlock;
    for (long long p = (long long)blockIdx.x * kPassBlock + threadIdx.x; p < positions; p += step) {
        const uint4 *c = (const uint4 *)(counts + (size_t)p * 8);
        const uint4 lo = c[0], hi = c[1];
        const uint32_t n[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        cons[p] = pileup_call(n, own[p], min_depth);
    }
}

__global__ void __launch_bounds__(kPassBlock)
pileup_reads_kernel(const uint32_t *__restrict__ counts, const uint8_t *__restrict__ own, const uint8_t *__restrict__ cons,
                    const int64_t *__restrict__ offsets, long long base, int n_reads, uint32_t min_depth,
                    const int32_t *__restrict__ n_aln, gact_read_pileup *__restrict__ reads)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (kPassBlock / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (kPassBlock / 64);
    for (int read = wave; read < n_reads; read += n_waves) {    // (offsets: the window's first read's onwards)
        const long long first = offsets[read] - base, len = offsets[read + 1] - offsets[read];
        int called = 0, changed = 0, deleted = 0, flagged = 0;
        uint32_t lane_max = 0;
        for (long long c0 = 0; c0 < len; c0 += 64) {
            const long long p = first + c0 + lane;
            const bool valid = c0 + lane < len;
            uint4 hi = make_uint4(0, 0, 0, 0);
            uint32_t mine = 0, made = 0;
            if (valid) {
                hi = ((const uint4 *)(counts + (size_t)p * 8))[1];           // OTHER, DEL, INS, DEPTH
                mine = own[p];
                made = cons[p];
            }
            lane_max = hi.w > lane_max ? hi.w : lane_max;
            const bool is_called = valid && hi.w >= min_depth;
            called += __popcll(__ballot(is_called));
            deleted += __popcll(__ballot(is_called && made == '-'));
            changed += __popcll(__ballot(is_called && made != '-' && (made | 0x20u) != (mine | 0x20u)));
            flagged += __popcll(__ballot(is_called && 2ull * hi.z > hi.w));
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = __shfl_xor(lane_max, o);
            lane_max = other > lane_max ? other : lane_max;
        }
        if (lane == 0) {
            int4 *r = (int4 *)&reads[read];
            r[0] = make_int4(n_aln[read], (int)lane_max, called, changed);
            r[1] = make_int4(deleted, flagged, 0, 0);
        }
    }
}

// The slot call of position p with K slots: how many are emitted -- the leading ones whose four counts together are more than
// half the depth, at a called position -- and their bytes, slot j's in bits [8 j, 8 j + 8)
__device__ __forceinline__ int pileup_slots(const uint32_t *__restrict__ ins, size_t p, int K, uint32_t depth, uint32_t min_depth,
                                            uint32_t &bytes)
{
    bytes = 0;
    if (depth < min_depth) return 0;
    int e = 0;
    for (; e < K; e++) {
        const uint4 n = ((const uint4 *)ins)[p * (size_t)K + e];
        if (2ull * ((unsigned long long)n.x + n.y + n.z + n.w) <= depth) break;
        uint32_t best = n.x, b = 'A';                           // the first of equal ones in the order A C G T
        if (n.y > best) { best = n.y; b = 'C'; }
        if (n.z > best) { best = n.z; b = 'G'; }
        if (n.w > best) { best = n.w; b = 'T'; }
        bytes |= b << (8 * e);
    }
    return e;
}

// kWrite false: read_at[read] = the corrected read's length, reads[read] its record.  kWrite true, behind pileup_scan_kernel:
// the read's bytes at seq + read_at[read]; a position that would write at or beyond seq_cap writes nothing.
template <bool kWrite>
__global__ void __launch_bounds__(kPassBlock)
pileup_spell_kernel(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ ins, int K, const uint8_t *__restrict__ own,
                    const uint8_t *__restrict__ cons, const int64_t *__restrict__ offsets, long long base, int n_reads,
                    uint32_t min_depth, long long *__restrict__ read_at, gact_read_corrected *__restrict__ reads,
                    uint8_t *__restrict__ seq, long long seq_cap)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (kPassBlock / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (kPassBlock / 64);
    const uint64_t below_me = (1ull << lane) - 1;
    for (int read = wave; read < n_reads; read += n_waves) {    // (offsets: the window's first read's onwards)
        const long long first = offsets[read] - base, len = offsets[read + 1] - offsets[read];
        long long at = kWrite ? read_at[read] : 0;              // where the step's first byte goes (kWrite false: from 0)
        int inserted = 0, sites = 0, deleted = 0, changed = 0;
        for (long long c0 = 0; c0 < len; c0 += 64) {
            const long long p = first + c0 + lane;
            const bool valid = c0 + lane < len;
            uint32_t depth = 0, mine = 0, made = '-', bytes = 0;
            int e = 0;                                          // emitted slots of my position
            if (valid) {
                depth = counts[(size_t)p * 8 + GACT_PILEUP_DEPTH];
                mine = own[p];
                made = cons[p];
                e = pileup_slots(ins, (size_t)p, K, depth, min_depth, bytes);
            }
            const bool keep = valid && made != '-';
            const uint64_t m_keep = __ballot(keep);
            int step = __popcll(m_keep), before = __popcll(m_keep & below_me);  // bytes of the step, of the lanes below mine
            for (int j = 0; j < K; j++) {                       // (wave-uniform)
                const uint64_t m = __ballot(e > j);
                step += __popcll(m);
                before += __popcll(m & below_me);
                if (j == 0) sites += __popcll(m);
            }
            if (kWrite) {
                const long long o = at + before;
                if (valid && o >= 0 && o + e + (keep ? 1 : 0) <= seq_cap) {
                    for (int j = 0; j < e; j++) seq[o + j] = (uint8_t)(bytes >> (8 * j));
                    if (keep) seq[o + e] = (uint8_t)made;
                }
            } else {
                inserted += step - __popcll(m_keep);
                deleted += __popcll(__ballot(valid && made == '-'));
                changed += __popcll(__ballot(keep && depth >= min_depth && (made | 0x20u) != (mine | 0x20u)));
            }
            at += step;
        }
        if (!kWrite && lane == 0) {
            read_at[read] = at;
            int4 *r = (int4 *)&reads[read];
            r[0] = make_int4((int)at, inserted, sites, deleted);
            r[1] = make_int4(changed, 0, 0, 0);
        }
    }
}

// one block: read_at[0, n_reads) (the lengths) -> their exclusive scan, in place; read_at[n_reads] = all bases,
// read_at[n_reads + 1] = the inserted ones
__global__ void __launch_bounds__(kPassBlock)
pileup_scan_kernel(int n_reads, long long *__restrict__ read_at, const gact_read_corrected *__restrict__ reads)
{
    long long carry = 0, carry_ins = 0;
    for (int base = 0; base < n_reads; base += kPassBlock) {
        const int k = base + (int)threadIdx.x;
        long long own[2] = {0, 0}, before[2], total[2];
        if (k < n_reads) { own[0] = read_at[k]; own[1] = reads[k].inserted; }  // (one branch: the loads fly together)
        block_scan_step(own, before, total);
        if (k < n_reads) read_at[k] = carry + before[0];
        carry += total[0];
        carry_ins += total[1];
    }
    if (threadIdx.x == 0) { read_at[n_reads] = carry; read_at[n_reads + 1] = carry_ins; }
}

}  // namespace gact
}  // extern "C++"

static int pileup_refuse_big_tiles(gact_hip_engine *e, const char *who)
{
    return refuse_big_tiles(e, who, "the pileup counts the path run's columns, which come from");
}

// One allocation: counts (32 positions) | slots (16 ins_slots positions) | consensus (positions) | read table (32 n_reads) |
// alignments per read (4 n_reads) | state (48) | corrected reads' table (32 n_reads) | read_at (8 (n_reads + 2)).  Everything but
// the consensus is zeroed here.
int gact_hip_pileup_begin_ins(gact_hip_engine *e, int32_t read_first, int32_t n_reads, int32_t ins_slots)
{
    if (!e) return fail(GACT_HIP_EINVAL, "engine is NULL");
    Pileup &pl = e->pileup;
    pl.open = false;                          // (a begin that is refused leaves no window open, an earlier one's neither)
    int rc = pileup_refuse_big_tiles(e, "pileup_begin");
    if (rc) return rc;
    if (ins_slots < 0 || ins_slots > GACT_PILEUP_MAX_INS_SLOTS)
        return fail(GACT_HIP_EINVAL, "pileup_begin: ins_slots = %d outside [0, %d]", ins_slots, GACT_PILEUP_MAX_INS_SLOTS);
    const SeqSet &rs = e->sets[GACT_SET_REF];
    if (rs.n == 0 || !rs.d_raw) return fail(GACT_HIP_EINVAL, "pileup_begin: GACT_SET_REF not uploaded");
    if (read_first < 0 || n_reads < 0 || (int64_t)read_first + n_reads > rs.n)
        return fail(GACT_HIP_EINVAL, "pileup_begin: the window [%d, %lld) lies outside the %d reads of GACT_SET_REF", read_first,
                    (long long)read_first + n_reads, rs.n);
    if ((rc = set_device(e))) return rc;
    PassScratch<gact_pileup_stats> &ps = pl.scratch;
    if ((rc = ps.timer.create("pileup_begin"))) return rc;
    const int64_t base = rs.h_offsets[(size_t)read_first];
    const int64_t positions = rs.h_offsets[(size_t)read_first + (size_t)n_reads] - base;
    const size_t at_ins = (size_t)positions * sizeof(gact_pileup_col);
    const size_t at_cons = at_ins + (size_t)positions * (size_t)ins_slots * sizeof(gact_pileup_ins);
    const size_t at_reads = up16(at_cons + (size_t)positions);
    const size_t at_aln = at_reads + (size_t)n_reads * sizeof(gact_read_pileup);
    const size_t at_state = up16(at_aln + (size_t)n_reads * sizeof(int32_t));
    const size_t at_corrected = at_state + sizeof(gact::PileupState);
    const size_t at_read_at = at_corrected + (size_t)n_reads * sizeof(gact_read_corrected);
    const size_t bytes = at_read_at + ((size_t)n_reads + 2) * sizeof(int64_t);
    if (ps.reserve(bytes))
        return fail(GACT_HIP_ENOMEM, "pileup_begin: device allocation failed (%d reads, %lld positions, %zu bytes)", n_reads,
                    (long long)positions, bytes);
    hipStream_t stream = e->slots[0].stream;
    // GACT_HIP_POISON_SCRATCH: here and nowhere else; from now to the next begin the window is kept state, which add, finish,
    // corrected and variants build on
    if ((rc = ps.refill(stream))) return rc;
    if (at_cons) HIP_TRY(hipMemsetAsync(ps.p, 0, at_cons, stream));
    HIP_TRY(hipMemsetAsync(ps.p + at_reads, 0, bytes - at_reads, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    pl.at_ins = at_ins; pl.at_cons = at_cons; pl.at_reads = at_reads; pl.at_aln = at_aln; pl.at_state = at_state;
    pl.at_corrected = at_corrected; pl.at_read_at = at_read_at;
    pl.read_first = read_first; pl.n_reads = n_reads; pl.ins_slots = ins_slots;
    pl.base = base; pl.positions = positions;
    pl.ref_epoch = e->ref_epoch;
    {
        std::lock_guard<std::mutex> lk(pl.mu);
        ps.stats = gact_pileup_stats{};
        ps.stats.positions = positions;
        ps.stats.scratch_bytes = (int64_t)ps.bytes;
        pl.ins_stats = gact_pileup_ins_stats{};
        pl.ins_stats.ins_slots = ins_slots;
        pl.ins_stats.table_bytes = (int64_t)(at_cons - at_ins);
    }
    pl.open = true;
    return 0;
}

int gact_hip_pileup_begin(gact_hip_engine *e, int32_t read_first, int32_t n_reads)
{
    return gact_hip_pileup_begin_ins(e, read_first, n_reads, 0);
}

static int pileup_window(gact_hip_engine *e, const char *who)
{
    const Pileup &pl = e->pileup;
    if (!pl.open) return fail(GACT_HIP_EINVAL, "%s: no window is open (gact_hip_pileup_begin first)", who);
    if (pl.ref_epoch != e->ref_epoch)
        return fail(GACT_HIP_EINVAL, "%s: GACT_SET_REF was uploaded after gact_hip_pileup_begin opened the window; begin again", who);
    return 0;
}

// The selection of gact_hip_candidates_paths, less the candidates outside the window, through the path run's chunks:
// chain_kernel (ColumnSink) into the slot's column buffers, pileup_kernel behind it, the next chunk behind that on the same stream.
int gact_hip_pileup_add(gact_hip_engine *e, int slot, int32_t n_sel, const int32_t *sel, int32_t rc_from, int same_file)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (n_sel < 0) return fail(GACT_HIP_EINVAL, "pileup_add: bad arguments");
    if ((rc = pileup_refuse_big_tiles(e, "pileup_add"))) return rc;
    if ((rc = pileup_window(e, "pileup_add"))) return rc;
    if (n_sel == 0) return 0;                 // (as gact_hip_candidates_paths)
    Pileup &pl = e->pileup;
    Slot &sl = e->slots[slot];
    Selection sn;
    if ((rc = select_candidates(e, slot, n_sel, sel, rc_from, "pileup_add", sn))) return rc;
    size_t kept = 0;
    for (size_t k = 0; k < sn.tagged.size(); k++) {
        const int32_t id = sn.tagged[k].ref_id;
        if (id < pl.read_first || id >= pl.read_first + pl.n_reads) continue;
        sn.tagged[kept] = sn.tagged[k];
        sn.cap[kept++] = sn.cap[k];
    }
    sn.tagged.resize(kept);
    sn.cap.resize(kept);
    const int32_t n_in = (int32_t)kept;
    if ((rc = path_bufs_init(sl.path, "pileup_add"))) return rc;
    Slot::PathBufs &pb = sl.path;
    gact::PileupWin win;
    win.counts = (uint32_t *)pl.scratch.p;
    win.n_aln = (int32_t *)(pl.scratch.p + pl.at_aln);
    win.state = (gact::PileupState *)(pl.scratch.p + pl.at_state);
    win.read_first = pl.read_first; win.n_reads = pl.n_reads;
    win.base = pl.base;
    win.ins = (uint32_t *)(pl.scratch.p + pl.at_ins);
    win.ins_slots = pl.ins_slots;
    const auto kernel = pl.ins_slots ? gact::pileup_kernel<true> : gact::pileup_kernel<false>;
    // Every chunk's arrays at their largest before the first launch: a DevBuf that grows frees its old memory, and chunk i's
    // kernels, which the host does not wait for, still read it while chunk i + 1 is being queued.
    {
        size_t most = 0;
        int64_t most_bytes = 0;
        for (int32_t first = 0; first < n_in;) {
            int64_t bytes = 0;
            const int32_t end = path_chunk_end(e, sn.cap, first, n_in, bytes);
            most = std::max(most, (size_t)(end - first));
            most_bytes = std::max(most_bytes, bytes);
            first = end;
        }
        if (pb.cands.reserve(most) || pb.records.reserve(most) || pb.col_off.reserve(most + 1) || pb.op_off.reserve(most) ||
            pb.n_cols.reserve(2 * most) || pb.n_ops.reserve(most) || pb.cols.reserve((size_t)most_bytes + 64))
            return fail(GACT_HIP_ENOMEM, "pileup_add: device allocation failed (%zu candidates, %lld column bytes)", most,
                        (long long)most_bytes);
    }
    std::deque<std::vector<int64_t> > col_offs;          // (every chunk's, alive until the stream has been waited for)
    int32_t chunks = 0;
    gact::PileupState st{};
    float ms = 0;
    auto queue_and_wait = [&]() -> int {
        int trc = sl.pile_timer.start(sl.stream, "pileup_add");
        if (trc) return trc;
        for (int32_t first = 0; first < n_in;) {
            int32_t end = first;
            int64_t bytes = 0;
            col_offs.emplace_back();
            const int crc = launch_path_chunk(e, sl, sn, first, n_in, same_file, "pileup_add", col_offs.back(), end, bytes);
            if (crc) return crc;
            const int32_t n = end - first;
            const int blocks = std::max(1, std::min((n + 3) / 4, 4096));
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(gact::kPassBlock), 0, sl.stream, pb.cols.p, pb.col_off.p,
                               pb.n_cols.p, pb.cands.p, pb.records.p, n, sn.d_rs, sn.d_qf, sn.d_qr, win);
            HIP_TRY(hipGetLastError());
            first = end;
            chunks++;
        }
        HIP_TRY(hipMemcpyAsync(&st, win.state, sizeof st, hipMemcpyDeviceToHost, sl.stream));
        return sl.pile_timer.stop(sl.stream, &ms);
    };
    if ((rc = queue_and_wait())) {
        // earlier chunks' copies out of col_offs and sn.tagged, and their kernels, may still be queued: wait before those go
        const std::string why = g_err;
        (void)hipStreamSynchronize(sl.stream);
        g_err = why;
        return rc;
    }
    {
        std::lock_guard<std::mutex> lk(pl.mu);
        gact_pileup_stats &ts = pl.scratch.stats;
        ts.device_ms += ms;
        ts.adds++;
        ts.chunks += chunks;
        ts.alignments = std::max(ts.alignments, (int64_t)st.alignments);       // (counted since begin, by every slot's adds)
        ts.columns = std::max(ts.columns, (int64_t)st.columns);
        pl.ins_stats.slot_adds = std::max(pl.ins_stats.slot_adds, (int64_t)st.slot_adds);
        pl.ins_stats.runs_truncated = std::max(pl.ins_stats.runs_truncated, (int64_t)st.runs_truncated);
    }
    if (st.flag) {
        // reported once: the flag word is cleared, so that later adds (of other slots too) answer for themselves.  The other
        // candidates of this add have been counted; the caller begins again if it wants the window without them.
        (void)hipMemsetAsync(&win.state->flag, 0, sizeof(int), sl.stream);
        (void)hipStreamSynchronize(sl.stream);
        return fail(GACT_HIP_ERANGE, "pileup_add: an alignment lies outside the window or outside its two reads (flag %d); it was "
                                     "left out, the add's other alignments are counted", st.flag);
    }
    return 0;
}

// the consensus bytes of the open window for min_depth, on `stream`
static int pileup_launch_consensus(gact_hip_engine *e, hipStream_t stream, int32_t min_depth)
{
    Pileup &pl = e->pileup;
    if (pl.positions <= 0) return 0;
    const size_t want = lane_blocks((size_t)pl.positions).x;
    hipLaunchKernelGGL(gact::pileup_consensus_kernel, dim3((unsigned)std::min(want, full_device_blocks(e) * 4)), dim3(gact::kPassBlock), 0, stream,
                       (const uint32_t *)pl.scratch.p, e->sets[GACT_SET_REF].d_raw + pl.base, (long long)pl.positions,
                       (uint32_t)min_depth, pl.scratch.p + pl.at_cons);
    HIP_TRY(hipGetLastError());
    return 0;
}

int gact_hip_pileup_finish(gact_hip_engine *e, int32_t min_depth, gact_pileup_col *counts, uint8_t *consensus, gact_read_pileup *reads)
{
    if (!e) return fail(GACT_HIP_EINVAL, "engine is NULL");
    if (min_depth < 1) return fail(GACT_HIP_EINVAL, "pileup_finish: min_depth = %d, at least 1", min_depth);
    int rc = pileup_window(e, "pileup_finish");
    if (rc) return rc;
    if ((rc = set_device(e))) return rc;
    Pileup &pl = e->pileup;
    const SeqSet &rs = e->sets[GACT_SET_REF];
    hipStream_t stream = e->slots[0].stream;
    PassScratch<gact_pileup_stats> &ps = pl.scratch;
    const uint32_t *d_counts = (const uint32_t *)ps.p;
    uint8_t *d_cons = ps.p + pl.at_cons;
    gact_read_pileup *d_reads = (gact_read_pileup *)(ps.p + pl.at_reads);
    const uint8_t *own = rs.d_raw + pl.base;
    if ((rc = ps.timer.start(stream, "pileup_finish"))) return rc;
    if ((rc = pileup_launch_consensus(e, stream, min_depth))) return rc;
    if (pl.n_reads > 0) {
        hipLaunchKernelGGL(gact::pileup_reads_kernel, wave_blocks(e, (size_t)pl.n_reads), dim3(gact::kPassBlock), 0, stream, d_counts,
                           own, d_cons, rs.d_offsets + pl.read_first, (long long)pl.base, pl.n_reads, (uint32_t)min_depth,
                           (const int32_t *)(ps.p + pl.at_aln), d_reads);
        HIP_TRY(hipGetLastError());
    }
    if (counts && pl.positions > 0)
        HIP_TRY(hipMemcpyAsync(counts, d_counts, (size_t)pl.positions * sizeof(gact_pileup_col), hipMemcpyDeviceToHost, stream));
    if (consensus && pl.positions > 0) HIP_TRY(hipMemcpyAsync(consensus, d_cons, (size_t)pl.positions, hipMemcpyDeviceToHost, stream));
    if (reads && pl.n_reads > 0)
        HIP_TRY(hipMemcpyAsync(reads, d_reads, (size_t)pl.n_reads * sizeof(gact_read_pileup), hipMemcpyDeviceToHost, stream));
    float ms = 0;
    if ((rc = ps.timer.stop(stream, &ms))) return rc;
    std::lock_guard<std::mutex> lk(pl.mu);
    ps.stats.device_ms += ms;
    return 0;
}

// The consensus, then pileup_spell_kernel<false> (lengths and the table), pileup_scan_kernel (read_at and the two totals, which
// the host waits for: they size the bytes), then, where the caller has room, pileup_spell_kernel<true> into pl.seq.
int gact_hip_pileup_corrected(gact_hip_engine *e, int32_t min_depth, gact_pileup_ins *ins, gact_read_corrected *reads,
                              int64_t *read_at, uint8_t *seq, int64_t seq_cap, int64_t *seq_len)
{
    if (!e) return fail(GACT_HIP_EINVAL, "engine is NULL");
    if (seq_len) *seq_len = 0;
    if (min_depth < 1) return fail(GACT_HIP_EINVAL, "pileup_corrected: min_depth = %d, at least 1", min_depth);
    if (seq_cap < 0) return fail(GACT_HIP_EINVAL, "pileup_corrected: seq_cap = %lld", (long long)seq_cap);
    int rc = pileup_window(e, "pileup_corrected");
    if (rc) return rc;
    Pileup &pl = e->pileup;
    if (ins && pl.ins_slots == 0)
        return fail(GACT_HIP_EINVAL, "pileup_corrected: the window was opened without slots (gact_hip_pileup_begin_ins), there is no table");
    if ((rc = set_device(e))) return rc;
    const SeqSet &rs = e->sets[GACT_SET_REF];
    hipStream_t stream = e->slots[0].stream;
    PassScratch<gact_pileup_stats> &ps = pl.scratch;
    const uint32_t *d_counts = (const uint32_t *)ps.p;
    const uint32_t *d_ins = pl.ins_slots ? (const uint32_t *)(ps.p + pl.at_ins) : nullptr;
    const uint8_t *d_cons = ps.p + pl.at_cons;
    gact_read_corrected *d_reads = (gact_read_corrected *)(ps.p + pl.at_corrected);
    long long *d_read_at = (long long *)(ps.p + pl.at_read_at);
    const uint8_t *own = rs.d_raw + pl.base;
    const int K = pl.ins_slots;
    const dim3 grid = wave_blocks(e, (size_t)pl.n_reads), block(gact::kPassBlock);
    if ((rc = ps.timer.start(stream, "pileup_corrected"))) return rc;
    if ((rc = pileup_launch_consensus(e, stream, min_depth))) return rc;
    if (pl.n_reads > 0) {
        hipLaunchKernelGGL(gact::pileup_spell_kernel<false>, grid, block, 0, stream, d_counts, d_ins, K, own, d_cons,
                           rs.d_offsets + pl.read_first, (long long)pl.base, pl.n_reads, (uint32_t)min_depth, d_read_at, d_reads,
                           (uint8_t *)nullptr, 0ll);
        hipLaunchKernelGGL(gact::pileup_scan_kernel, dim3(1), block, 0, stream, pl.n_reads, d_read_at, d_reads);
        HIP_TRY(hipGetLastError());
    }
    long long totals[2] = {0, 0};                                 // all bases, the inserted ones (n_reads == 0: zeroed by begin)
    HIP_TRY(hipMemcpyAsync(totals, d_read_at + pl.n_reads, sizeof totals, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (totals[0] < 0 || totals[0] > pl.positions * (K + 1) || totals[1] < 0 || totals[1] > totals[0])
        return fail(GACT_HIP_EDEVICE, "pileup_corrected: the device counted %lld bases, %lld of them inserted, at %lld positions",
                    totals[0], totals[1], (long long)pl.positions);
    if (seq_len) *seq_len = totals[0];
    const bool room = !seq || seq_cap >= totals[0];
    if (seq && room && totals[0] > 0) {
        if ((size_t)totals[0] > pl.seq_cap) {
            if (pl.seq) (void)hipFree(pl.seq);
            pl.seq = nullptr; pl.seq_cap = 0;
            if (hipMalloc((void **)&pl.seq, (size_t)totals[0]) != hipSuccess) {
                (void)hipGetLastError();
                return fail(GACT_HIP_ENOMEM, "pileup_corrected: device allocation failed (%lld bases)", totals[0]);
            }
            pl.seq_cap = (size_t)totals[0];
        }
        if ((rc = poison_scratch(e, pl.seq, pl.seq_cap, stream))) return rc;       // (the bytes are scratch: every call spells them anew)
        hipLaunchKernelGGL(gact::pileup_spell_kernel<true>, grid, block, 0, stream, d_counts, d_ins, K, own, d_cons,
                           rs.d_offsets + pl.read_first, (long long)pl.base, pl.n_reads, (uint32_t)min_depth, d_read_at, d_reads,
                           pl.seq, totals[0]);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(seq, pl.seq, (size_t)totals[0], hipMemcpyDeviceToHost, stream));
    }
    if (ins && pl.positions > 0)
        HIP_TRY(hipMemcpyAsync(ins, d_ins, (size_t)pl.positions * (size_t)K * sizeof(gact_pileup_ins), hipMemcpyDeviceToHost, stream));
    if (read_at) HIP_TRY(hipMemcpyAsync(read_at, d_read_at, ((size_t)pl.n_reads + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    if (reads && pl.n_reads > 0)
        HIP_TRY(hipMemcpyAsync(reads, d_reads, (size_t)pl.n_reads * sizeof(gact_read_corrected), hipMemcpyDeviceToHost, stream));
    float ms = 0;
    if ((rc = ps.timer.stop(stream, &ms))) return rc;
    {
        std::lock_guard<std::mutex> lk(pl.mu);
        pl.ins_stats.device_ms += ms;
        pl.ins_stats.emitted = totals[1];
    }
    if (!room)
        return fail(GACT_HIP_EINVAL, "pileup_corrected: %lld bases, room for %lld: call again with room for *seq_len", totals[0],
                    (long long)seq_cap);
    return 0;
}

int gact_hip_last_pileup_ins_stats(gact_hip_engine *e, gact_pileup_ins_stats *stats)
{
    if (!e || !stats) return fail(GACT_HIP_EINVAL, "last_pileup_ins_stats: NULL argument");
    Pileup &pl = e->pileup;
    if (!pl.open) return fail(GACT_HIP_EINVAL, "last_pileup_ins_stats: no window is open (gact_hip_pileup_begin first)");
    std::lock_guard<std::mutex> lk(pl.mu);
    *stats = pl.ins_stats;
    return 0;
}

int gact_hip_last_pileup_stats(gact_hip_engine *e, gact_pileup_stats *stats)
{
    if (!e || !stats) return fail(GACT_HIP_EINVAL, "last_pileup_stats: NULL argument");
    Pileup &pl = e->pileup;
    if (!pl.open) return fail(GACT_HIP_EINVAL, "last_pileup_stats: no window is open (gact_hip_pileup_begin first)");
    std::lock_guard<std::mutex> lk(pl.mu);
    *stats = pl.scratch.stats;
    return 0;
}
