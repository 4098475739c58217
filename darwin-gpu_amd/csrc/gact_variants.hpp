// gact_variants.hpp -- variants of the open pileup window, called from its counts (gact_hip_pileup_variants), and the VCF line
// of one (gact_hip_format_vcf).  The rule is stated in include/gact_hip.h.
//
// The targets are reference sequences: a few, possibly megabases long.  So the work is cut by position, not by sequence: one
// wave takes GACT_VARIANT_CHUNK consecutive positions of the window, 64 a step (consecutive lanes read consecutive positions'
// counts: 32 bytes a lane), and a lane finds its sequence from the window's offsets -- one search a step where the step lies
// inside one sequence, which is almost always.
//
//   variant_count_kernel   per position one byte of bits: INS, deleted, SNV to A C G T, examined, first of its sequence -- kept
//                          for the write pass, which then reads 1 byte a position where this pass read 32 + 16 K.  A chunk's
//                          records are the popcounts of the ballots of INS, of the deleted lanes that START a run (the lane
//                          below is not deleted, or the lane is its sequence's first; for lane 0 the step before's lane 63,
//                          and for the chunk's first step the position in front of the chunk, called from its counts) and of
//                          the four SNV bits.  The per-sequence table takes integer atomic adds: one per wave and step where
//                          the step lies inside one sequence, one per lane with something to add elsewhere.
//   variant_scan_kernel    one block (block_scan_step): the chunks' counts -> their exclusive scan and the total; then the
//                          sequences' records -> `first`, and the totals per kind.  No block waits for another.
//   variant_write_kernel   a chunk's steps from LAST TO FIRST, carrying the length of the run that is open to the right: a run's
//                          first lane needs the run's length, which is 1 + the stretch of set bits directly above the lane in
//                          the ballot of the lanes that go on a run (deleted and not their sequence's first), plus the carry
//                          when that stretch reaches lane 63.  The carry into the chunk's last step comes from a peek past the
//                          chunk's end through the bytes of the count pass; it almost always ends in its first step, and is
//                          not made at all unless the chunk's last position is deleted.  A record's index is counted from the
//                          chunk's END: the scan's base of the next chunk, less the records of the steps behind, of the lanes
//                          above and the lane's own.  A chunk without records is passed over.
// No look-back, no spinning, no atomics but the table's adds, whose sums do not depend on their order.  Every index is checked
// before it is used.  All results are integers and the same on every call.
//
// Included by gact_engine.hip behind gact_pileup.hpp, inside its extern "C" block.
#pragma once

extern "C++" {                  // (templates: not in gact_engine.hip's extern "C")
namespace gact {

constexpr int kVariantChunk = GACT_VARIANT_CHUNK;
static_assert(kVariantChunk % 64 == 0 && kVariantChunk > 0, "a chunk is whole steps: only the window's last step may be partial");

// the byte of a position
constexpr uint32_t kVarIns = 1, kVarDel = 2, kVarSnv = 4 /* << base */, kVarExamined = 64, kVarFirst = 128;

struct VariantWin {
    const uint32_t *counts;                       // [positions][8]
    const uint32_t *ins;                          // [positions][K][4]
    const uint8_t *own;                           // the window's raw bytes
    const int64_t *offsets;                       // of the window's first sequence onwards, n_seqs + 1 of them
    long long base, positions;
    int n_seqs, K, seq_first;
    gact_variant_params p;
};

__device__ __forceinline__ bool variant_qualifies(unsigned long long a, uint32_t d, const gact_variant_params &p)
{
    return a >= (unsigned long long)p.min_alt && 1000ull * a >= (unsigned long long)p.min_permille * d;
}

__device__ __forceinline__ int variant_gt(unsigned long long a, uint32_t d, const gact_variant_params &p)
{
    return 1000ull * a >= (unsigned long long)p.hom_permille * d ? 2 : 1;
}

// the sequence of window position p (0 <= p < positions), searched from lo, a sequence that starts at or in front of p:
// the last one that does, so empty sequences are passed over
__device__ __forceinline__ int variant_seq_of(const VariantWin &w, long long p, int lo)
{
    int hi = w.n_seqs;                            // offsets[hi] - base == positions > p
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (w.offsets[mid] - w.base <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// the bits of position p but kVarFirst
__device__ __forceinline__ uint32_t variant_bits(const VariantWin &w, long long p)
{
    const uint4 *c = (const uint4 *)(w.counts + (size_t)p * 8);
    const uint4 hi = c[1];                        // OTHER, DEL, INS, DEPTH
    const uint32_t d = hi.w;
    if (d < (uint32_t)w.p.min_depth) return 0;
    uint32_t bits = kVarExamined;
    if (variant_qualifies(hi.y, d, w.p)) bits |= kVarDel;
    if (w.K > 0) {
        const uint4 s = ((const uint4 *)w.ins)[(size_t)p * (size_t)w.K];
        if (variant_qualifies((unsigned long long)s.x + s.y + s.z + s.w, d, w.p)) bits |= kVarIns;
    }
    const int mine = pileup_kind(w.own[p]);
    if (mine < 4) {
        const uint4 lo = c[0];
        const uint32_t n[4] = {lo.x, lo.y, lo.z, lo.w};
        for (int b = 0; b < 4; b++)
            if (b != mine && variant_qualifies(n[b], d, w.p)) bits |= kVarSnv << b;
    }
    return bits;
}

__global__ void __launch_bounds__(kPassBlock)
variant_count_kernel(VariantWin w, int n_chunks, uint8_t *__restrict__ bytes, long long *__restrict__ chunk_at,
                     gact_seq_variants *__restrict__ seqs)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kPassWaves + (threadIdx.x >> 6), n_waves = gridDim.x * kPassWaves;
    for (int chunk = wave; chunk < n_chunks; chunk += n_waves) {               // (wave-uniform)
        const long long c0 = (long long)chunk * kVariantChunk;
        const long long c1 = c0 + kVariantChunk < w.positions ? c0 + kVariantChunk : w.positions;
        bool below_deleted = c0 > 0 && (variant_bits(w, c0 - 1) & kVarDel);     // lane 0's neighbour (wave-uniform)
        int i0 = 0, n = 0;
        for (long long s0 = c0; s0 < c1; s0 += 64) {
            const long long p = s0 + lane, last = s0 + 63 < c1 ? s0 + 63 : c1 - 1;
            const bool valid = p < c1;
            i0 = variant_seq_of(w, s0, i0);
            const bool one_seq = last < w.offsets[i0 + 1] - w.base;           // the step lies inside one sequence
            int i = i0;
            uint32_t bits = 0;
            if (valid) {
                if (!one_seq) i = variant_seq_of(w, p, i0);
                bits = variant_bits(w, p);
                if (p == w.offsets[i] - w.base) bits |= kVarFirst;
                bytes[p] = (uint8_t)bits;
            }
            const uint64_t m_del = __ballot((bits & kVarDel) != 0);
            const bool below = lane ? (m_del >> (lane - 1)) & 1 : below_deleted;
            const bool starts = (bits & kVarDel) && !(below && !(bits & kVarFirst));
            const uint64_t m_ex = __ballot((bits & kVarExamined) != 0), m_ins = __ballot((bits & kVarIns) != 0),
                           m_start = __ballot(starts);
            int n_snv = 0;
            for (int b = 0; b < 4; b++) n_snv += __popcll(__ballot((bits & (kVarSnv << b)) != 0));
            n += __popcll(m_ins) + __popcll(m_start) + n_snv;
            if (one_seq) {
                if (lane == 0) {
                    gact_seq_variants *t = seqs + i0;
                    if (m_ex) atomicAdd(&t->examined, __popcll(m_ex));
                    if (m_ins) atomicAdd(&t->n_ins, __popcll(m_ins));
                    if (m_start) atomicAdd(&t->n_del, __popcll(m_start));
                    if (n_snv) atomicAdd(&t->n_snv, n_snv);
                }
            } else if (bits & ~kVarFirst) {
                gact_seq_variants *t = seqs + i;
                atomicAdd(&t->examined, 1);
                if (bits & kVarIns) atomicAdd(&t->n_ins, 1);
                if (starts) atomicAdd(&t->n_del, 1);
                const int mine = __popc((bits / kVarSnv) & 15u);
                if (mine) atomicAdd(&t->n_snv, mine);
            }
            below_deleted = (m_del >> 63) & 1;
        }
        if (lane == 0) chunk_at[chunk] = n;
    }
}

// one block.  chunk_at[0, n_chunks) (the counts) -> their exclusive scan, in place, chunk_at[n_chunks] = all records; then
// seqs[i].first = the records of the sequences in front of i, and totals[0 .. 5) = records, examined, n_ins, n_del, n_snv
__global__ void __launch_bounds__(kPassBlock)
variant_scan_kernel(int n_chunks, long long *__restrict__ chunk_at, int n_seqs, gact_seq_variants *__restrict__ seqs,
                    long long *__restrict__ totals)
{
    long long carry = 0;
    for (int base = 0; base < n_chunks; base += kPassBlock) {
        const int k = base + (int)threadIdx.x;
        long long own[1] = {0}, before[1], total[1];
        if (k < n_chunks) own[0] = chunk_at[k];
        block_scan_step(own, before, total);
        if (k < n_chunks) chunk_at[k] = carry + before[0];
        carry += total[0];
    }
    if (threadIdx.x == 0) chunk_at[n_chunks] = carry;
    long long sum[5] = {0, 0, 0, 0, 0};
    for (int base = 0; base < n_seqs; base += kPassBlock) {
        const int k = base + (int)threadIdx.x;
        long long own[5] = {0, 0, 0, 0, 0}, before[5], total[5];
        if (k < n_seqs) {                                       // (one branch: the loads fly together)
            const gact_seq_variants t = seqs[k];
            own[1] = t.examined; own[2] = t.n_ins; own[3] = t.n_del; own[4] = t.n_snv;
            own[0] = own[2] + own[3] + own[4];
        }
        block_scan_step(own, before, total);
        const long long first = sum[0] + before[0];
        if (k < n_seqs) seqs[k].first = first < 0x7fffffffll ? (int)first : 0x7fffffff;     // (the host refuses such a total)
        for (int i = 0; i < 5; i++) sum[i] += total[i];
    }
    if (threadIdx.x == 0)
        for (int i = 0; i < 5; i++) totals[i] = sum[i];
}

__device__ __forceinline__ void variant_store(gact_variant *out, long long at, long long lo, long long hi, int seq, int pos, int kind,
                                              int len, uint32_t bases, uint32_t alt, uint32_t depth, int flags)
{
    if (at < lo || at >= hi) return;              // (never, when the two passes saw the same counts)
    int4 *r = (int4 *)(out + at);
    r[0] = make_int4(seq, pos, kind, len);
    r[1] = make_int4((int)bases, (int)alt, (int)depth, flags);
}

__global__ void __launch_bounds__(kPassBlock)
variant_write_kernel(VariantWin w, int n_chunks, const uint8_t *__restrict__ bytes, const long long *__restrict__ chunk_at,
                     gact_variant *__restrict__ out, long long out_cap)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kPassWaves + (threadIdx.x >> 6), n_waves = gridDim.x * kPassWaves;
    const uint64_t above_me = lane == 63 ? 0ull : ~0ull << (lane + 1);
    for (int chunk = wave; chunk < n_chunks; chunk += n_waves) {               // (wave-uniform)
        const long long begin = chunk_at[chunk], end = chunk_at[chunk + 1];
        if (end <= begin || begin < 0 || end > out_cap) continue;
        const long long c0 = (long long)chunk * kVariantChunk;
        const long long c1 = c0 + kVariantChunk < w.positions ? c0 + kVariantChunk : w.positions;
        // the run that goes on behind the chunk's last position: the positions from c1 on that are deleted and not the first
        // of their sequence
        long long carry = 0;
        if (c1 < w.positions && (bytes[c1 - 1] & kVarDel)) {
            for (long long q0 = c1; q0 < w.positions; q0 += 64) {
                const long long q = q0 + lane;
                const uint32_t b = q < w.positions ? bytes[q] : 0u;
                const uint64_t stop = ~__ballot((b & kVarDel) && !(b & kVarFirst));
                carry += stop ? __ffsll((unsigned long long)stop) - 1 : 64;
                if (stop) break;
            }
        }
        long long behind = 0;                                   // the records of the steps behind this one
        const int n_steps = (int)((c1 - c0 + 63) >> 6);
        for (int s = n_steps - 1; s >= 0; s--) {
            const long long p = c0 + (long long)s * 64 + lane;
            const bool valid = p < c1;
            const uint32_t bits = valid ? bytes[p] : 0u;
            const bool deleted = (bits & kVarDel) != 0, goes_on = deleted && !(bits & kVarFirst);
            const uint64_t m_del = __ballot(deleted), m_on = __ballot(goes_on);
            const bool below = lane ? (m_del >> (lane - 1)) & 1 : (p > 0 && (bytes[p - 1] & kVarDel));
            const bool starts = deleted && !(goes_on && below);
            const uint64_t m_ins = __ballot((bits & kVarIns) != 0), m_start = __ballot(starts);
            int above = __popcll(m_ins & above_me) + __popcll(m_start & above_me), all = __popcll(m_ins) + __popcll(m_start);
            for (int b = 0; b < 4; b++) {
                const uint64_t m = __ballot((bits & (kVarSnv << b)) != 0);
                above += __popcll(m & above_me);
                all += __popcll(m);
            }
            const int mine = (int)(bits & kVarIns) + (starts ? 1 : 0) + __popc((bits / kVarSnv) & 15u);
            if (mine) {
                long long at = end - behind - above - mine;
                const int i = variant_seq_of(w, p, 0);
                const int seq = w.seq_first + i, pos = (int)(p - (w.offsets[i] - w.base));
                const uint4 *c = (const uint4 *)(w.counts + (size_t)p * 8);
                const uint4 lo = c[0], hi = c[1];
                const uint32_t d = hi.w;
                if (bits & kVarIns) {
                    int len = 0;
                    uint32_t letters = 0, alt = 0;
                    for (; len < w.K; len++) {
                        const uint4 n = ((const uint4 *)w.ins)[(size_t)p * (size_t)w.K + len];
                        const unsigned long long sum = (unsigned long long)n.x + n.y + n.z + n.w;
                        if (!variant_qualifies(sum, d, w.p)) break;
                        if (len == 0) alt = (uint32_t)sum;
                        uint32_t best = n.x, b = 'A';           // the first of equal ones in the order A C G T
                        if (n.y > best) { best = n.y; b = 'C'; }
                        if (n.z > best) { best = n.z; b = 'G'; }
                        if (n.w > best) { best = n.w; b = 'T'; }
                        letters |= b << (8 * len);
                    }
                    variant_store(out, at++, begin, end, seq, pos, GACT_VARIANT_INS, len, letters, alt, d,
                                  variant_gt(alt, d, w.p) | (len == w.K ? GACT_VARIANT_TRUNCATED : 0));
                }
                if (starts) {
                    // the lanes directly above that go on the run; where they reach lane 63, the run open to the right
                    const uint64_t stop = lane == 63 ? 1ull : ~(m_on >> (lane + 1));     // (the zeros shifted in stop it at the top)
                    const int stretch = __ffsll((unsigned long long)stop) - 1;
                    const long long len = 1 + stretch + (stretch == 63 - lane ? carry : 0);
                    variant_store(out, at++, begin, end, seq, pos, GACT_VARIANT_DEL, (int)(len < 0x7fffffffll ? len : 0x7fffffff), 0u, hi.y, d,
                                  variant_gt(hi.y, d, w.p));
                }
                const uint32_t n[4] = {lo.x, lo.y, lo.z, lo.w};
                for (int b = 0; b < 4; b++)
                    if (bits & (kVarSnv << b))
                        variant_store(out, at++, begin, end, seq, pos, GACT_VARIANT_SNV, 1, (uint32_t)"ACGT"[b], n[b], d, variant_gt(n[b], d, w.p));
            }
            behind += all;
            // the run open at this step's first lane: the lanes from 0 up that go on a run
            const uint64_t stop = ~m_on;
            carry = stop ? __ffsll((unsigned long long)stop) - 1 : 64 + carry;
        }
    }
}

}  // namespace gact
}  // extern "C++"

static int variant_params_check(const gact_variant_params *params, gact_variant_params &p)
{
    p = params ? *params : gact_variant_params{GACT_VARIANT_DEFAULT_MIN_DEPTH, GACT_VARIANT_DEFAULT_MIN_ALT,
                                               GACT_VARIANT_DEFAULT_MIN_PERMILLE, GACT_VARIANT_DEFAULT_HOM_PERMILLE};
    if (p.min_depth < 1) return fail(GACT_HIP_EINVAL, "pileup_variants: min_depth = %d, at least 1", p.min_depth);
    if (p.min_alt < 1) return fail(GACT_HIP_EINVAL, "pileup_variants: min_alt = %d, at least 1", p.min_alt);
    if (!(0 <= p.min_permille && p.min_permille <= p.hom_permille && p.hom_permille <= 1000))
        return fail(GACT_HIP_EINVAL, "pileup_variants: min_permille = %d, hom_permille = %d: not 0 <= min_permille <= hom_permille <= 1000",
                    p.min_permille, p.hom_permille);
    return 0;
}

// One allocation (Pileup::variants): bytes (1 per position) | chunk_at (8 (chunks + 1)) | totals (8 x 5) | the sequences' table
// (32 per sequence) | the records (32 each).  The records' room is what the allocation has beyond the rest; a call that finds
// more records than that grows the allocation, which loses the first three parts, and counts again: the counts have not changed.
int gact_hip_pileup_variants(gact_hip_engine *e, const gact_variant_params *params, gact_variant *variants, int64_t cap,
                             int64_t *n_variants, gact_seq_variants *seqs)
{
    if (!e) return fail(GACT_HIP_EINVAL, "engine is NULL");
    gact_variant_params p;
    int rc = variant_params_check(params, p);
    if (rc) return rc;
    if (cap < 0) return fail(GACT_HIP_EINVAL, "pileup_variants: cap = %lld", (long long)cap);
    if ((rc = pileup_window(e, "pileup_variants"))) return rc;
    if ((rc = set_device(e))) return rc;
    Pileup &pl = e->pileup;
    const SeqSet &rs = e->sets[GACT_SET_REF];
    hipStream_t stream = e->slots[0].stream;
    PassScratch<gact_variant_stats> &ps = pl.variants;
    const int64_t positions = pl.positions;
    const int64_t chunks64 = (positions + gact::kVariantChunk - 1) / gact::kVariantChunk;
    if (chunks64 > 0x7fffffff) return fail(GACT_HIP_EINVAL, "pileup_variants: %lld positions are more chunks than an int counts", (long long)positions);
    const int n_chunks = (int)chunks64, n_seqs = pl.n_reads;
    const size_t at_chunk = up16((size_t)positions);
    const size_t at_totals = at_chunk + ((size_t)n_chunks + 1) * sizeof(long long);
    const size_t at_seqs = up16(at_totals + 5 * sizeof(long long));
    const size_t at_rec = up16(at_seqs + (size_t)n_seqs * sizeof(gact_seq_variants));
    int64_t room = variants && ps.bytes > at_rec ? (int64_t)((ps.bytes - at_rec) / sizeof(gact_variant)) : 0;
    if (ps.reserve(at_rec + (size_t)room * sizeof(gact_variant)))
        return fail(GACT_HIP_ENOMEM, "pileup_variants: device allocation failed (%lld positions, %d sequences)", (long long)positions, n_seqs);
    if ((rc = ps.begin(stream, "pileup_variants"))) return rc;
    gact::VariantWin w;
    w.counts = (const uint32_t *)pl.scratch.p;
    w.ins = pl.ins_slots ? (const uint32_t *)(pl.scratch.p + pl.at_ins) : nullptr;
    w.own = rs.d_raw + pl.base;
    w.offsets = rs.d_offsets + pl.read_first;
    w.base = pl.base; w.positions = positions;
    w.n_seqs = n_seqs; w.K = pl.ins_slots; w.seq_first = pl.read_first;
    w.p = p;
    const dim3 grid = wave_blocks(e, (size_t)n_chunks), block(gact::kPassBlock);
    long long totals[5] = {0, 0, 0, 0, 0};
    for (int attempt = 0; positions > 0; attempt++) {
        long long *d_chunk_at = (long long *)(ps.p + at_chunk);
        gact_seq_variants *d_seqs = (gact_seq_variants *)(ps.p + at_seqs);
        HIP_TRY(hipMemsetAsync(d_seqs, 0, (size_t)n_seqs * sizeof(gact_seq_variants), stream));
        hipLaunchKernelGGL(gact::variant_count_kernel, grid, block, 0, stream, w, n_chunks, ps.p, d_chunk_at, d_seqs);
        hipLaunchKernelGGL(gact::variant_scan_kernel, dim3(1), block, 0, stream, n_chunks, d_chunk_at, n_seqs, d_seqs,
                           (long long *)(ps.p + at_totals));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(totals, ps.p + at_totals, sizeof totals, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (totals[0] < 0 || totals[0] > 5 * positions || totals[0] != totals[2] + totals[3] + totals[4] || totals[1] < 0 || totals[1] > positions)
            return fail(GACT_HIP_EDEVICE, "pileup_variants: the device counted %lld records (%lld + %lld + %lld) at %lld examined of %lld positions",
                        totals[0], totals[2], totals[3], totals[4], totals[1], (long long)positions);
        if (totals[0] > 0x7fffffffll)
            return fail(GACT_HIP_ERANGE, "pileup_variants: %lld records are more than gact_seq_variants.first counts", totals[0]);
        if (!variants || cap < totals[0] || totals[0] <= room || attempt) break;
        room = totals[0];
        if (ps.reserve(at_rec + (size_t)room * sizeof(gact_variant)))
            return fail(GACT_HIP_ENOMEM, "pileup_variants: device allocation failed (%lld records)", totals[0]);
        if ((rc = ps.refill(stream))) return rc;           // GACT_HIP_POISON_SCRATCH: the new block, in front of the recount
    }
    const bool fits = !variants || cap >= totals[0];
    if (variants && fits && totals[0] > 0) {
        if (totals[0] > room) return fail(GACT_HIP_EDEVICE, "pileup_variants: %lld records, room for %lld", totals[0], (long long)room);
        gact_variant *d_out = (gact_variant *)(ps.p + at_rec);
        hipLaunchKernelGGL(gact::variant_write_kernel, grid, block, 0, stream, w, n_chunks, (const uint8_t *)ps.p,
                           (const long long *)(ps.p + at_chunk), d_out, totals[0]);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(variants, d_out, (size_t)totals[0] * sizeof(gact_variant), hipMemcpyDeviceToHost, stream));
    }
    if (seqs && n_seqs > 0) {
        if (positions > 0) HIP_TRY(hipMemcpyAsync(seqs, ps.p + at_seqs, (size_t)n_seqs * sizeof(gact_seq_variants), hipMemcpyDeviceToHost, stream));
        else memset(seqs, 0, (size_t)n_seqs * sizeof(gact_seq_variants));
    }
    if ((rc = ps.end(stream))) return rc;
    ps.stats.chunks = n_chunks;
    ps.stats.examined = totals[1];
    ps.stats.n_ins = totals[2]; ps.stats.n_del = totals[3]; ps.stats.n_snv = totals[4];
    ps.stats.scratch_bytes = (int64_t)ps.bytes;
    if (n_variants) *n_variants = totals[0];
    if (!fits)
        return fail(GACT_HIP_EINVAL, "pileup_variants: %lld records, room for %lld: call again with room for *n_variants", totals[0],
                    (long long)cap);
    return 0;
}

int gact_hip_last_variant_stats(gact_hip_engine *e, gact_variant_stats *stats)
{
    if (!e || !stats) return fail(GACT_HIP_EINVAL, "last_variant_stats: NULL argument");
    const PassScratch<gact_variant_stats> &ps = e->pileup.variants;
    if (!ps.timed) return fail(GACT_HIP_EINVAL, "last_variant_stats: no gact_hip_pileup_variants call has run yet");
    *stats = ps.stats;
    return 0;
}

// a reference byte as VCF prints it
static char vcf_ref(uint8_t b)
{
    const char c = (char)(b & ~0x20);
    return c == 'A' || c == 'C' || c == 'G' || c == 'T' ? c : 'N';
}

int gact_hip_format_vcf(const gact_variant *v, const char *seq_name, const uint8_t *seq, int64_t seq_len, char *buf, size_t cap)
{
    if (!v || !seq_name || !seq || seq_len < 0 || (cap > 0 && !buf)) return fail(GACT_HIP_EINVAL, "format_vcf: bad arguments");
    const int gt = v->flags & 3;
    if (gt != 1 && gt != 2) return fail(GACT_HIP_EINVAL, "format_vcf: gt %d is neither 1 nor 2", gt);
    const int64_t pos = v->pos, len = v->len;
    if (pos < 0 || pos >= seq_len || len < 1)
        return fail(GACT_HIP_EINVAL, "format_vcf: pos %lld, len %lld on a sequence of %lld bases", (long long)pos, (long long)len, (long long)seq_len);
    std::string ref, alt;
    int64_t at = pos;                             // POS - 1
    if (v->kind == GACT_VARIANT_SNV) {
        const char b = (char)(v->bases & 0xff);
        if (len != 1 || !strchr("ACGT", b) || !b) return fail(GACT_HIP_EINVAL, "format_vcf: an SNV of len %lld to the byte %d", (long long)len, (int)b);
        ref = vcf_ref(seq[pos]);
        alt = b;
    } else if (v->kind == GACT_VARIANT_DEL) {
        if (pos + len > seq_len)
            return fail(GACT_HIP_EINVAL, "format_vcf: the deletion [%lld, %lld) ends behind the sequence's %lld bases", (long long)pos,
                        (long long)(pos + len), (long long)seq_len);
        if (pos == 0 && len == seq_len) {         // the whole sequence: no line
            if (cap > 0) buf[0] = 0;
            return 0;
        }
        at = pos ? pos - 1 : 0;
        for (int64_t i = at; i < (pos ? pos + len : len + 1); i++) ref += vcf_ref(seq[i]);
        alt = vcf_ref(seq[pos ? pos - 1 : len]);
    } else if (v->kind == GACT_VARIANT_INS) {
        if (len > GACT_PILEUP_MAX_INS_SLOTS) return fail(GACT_HIP_EINVAL, "format_vcf: an insertion of len %lld", (long long)len);
        std::string bases;
        for (int j = 0; j < (int)len; j++) {
            const char b = (char)((v->bases >> (8 * j)) & 0xff);
            if (!b || !strchr("ACGT", b)) return fail(GACT_HIP_EINVAL, "format_vcf: inserted byte %d is none of A C G T", (int)b);
            bases += b;
        }
        at = pos ? pos - 1 : 0;
        ref = vcf_ref(seq[at]);
        alt = pos ? ref + bases : bases + ref;
    } else {
        return fail(GACT_HIP_EINVAL, "format_vcf: kind %d is none of GACT_VARIANT_INS, _DEL, _SNV", v->kind);
    }
    std::string line = seq_name;
    line += '\t' + std::to_string(at + 1) + "\t.\t" + ref + '\t' + alt + "\t.\t.\tDP=" + std::to_string(v->depth) + ";AD=" +
            std::to_string(v->alt) + "\tGT\t" + (gt == 2 ? "1/1" : "0/1") + '\n';
    if (line.size() > 0x7fffffffu) return fail(GACT_HIP_ERANGE, "format_vcf: the line has %zu bytes", line.size());
    if (cap > line.size()) memcpy(buf, line.c_str(), line.size() + 1);     // (with its terminator) when it fits; its length either way
    else if (cap > 0) buf[0] = 0;
    return (int)line.size();
}
