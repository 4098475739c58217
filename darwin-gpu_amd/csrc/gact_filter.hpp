// gact_filter.hpp -- the overlap set filtered on the device by identity, span and each read's best (gact_hip_filter_overlaps).
//
// Under +1/-1/-1/-1 two unrelated sequences align with a positive score, so a false seed hit becomes an emitted record, and
// every pass behind a run takes it (37 of 615 on truth block B, 4 wrong arcs after cleaning).  The summaries of
// gact_hip_candidates_summaries carry n_eq, and identity parts the two kinds; where it does not in absolute terms (a diverged
// copy of the reference), it does against the best record of the same read.  The rule is stated in include/gact_hip.h.
//
// Four stages on the slot's stream, nothing on the host between them:
//   1 filter_classify_kernel  one lane per chosen record: the record and its summary, tests 1 to 4, ident and the provisional
//                             why stored per record; a counted record's reads on the requested sides are checked against the
//                             window (one flag word; every later kernel returns at once when it is set, as the arc-graph
//                             passes do) and take atomicAdd(n_records); a passed record adds n_passed, eq_sum and col_sum and
//                             puts its ident into best with atomicMax.  Integer atomics only: the table is the same in whichever
//                             order they land.
//   2 filter_flag_kernel      the relative test against the finished best, the final why, atomicAdd(n_kept) per read; one
//                             ballot per wave (kept: 64 flags in one word), popcounts per wave, summed per block -- the shape
//                             of select_flag_kernel; the totals per reason through wave_count.
//   3 filter_scan_kernel      exclusive scan of the block counts, one block (block_scan_step), looping over the blocks
//   4 filter_write_kernel     every block writes kept_at and kept_sel at its offset in index order.
// Two levels of scan on purpose, as in gact_select.hpp: no block spins on another block's flag.
//
// Included by gact_engine.hip behind every other kernel and behind the engine's definitions (Slot, fail, HIP_TRY), inside its
// extern "C" block, as gact_select.hpp is.
#pragma once

namespace gact {

constexpr int32_t kFilterMaxRecords = 1 << 30;
constexpr int kFilterBadIndex = 1, kFilterBadRead = 2;      // bits of the flag word
constexpr int kFilterReasons = 6;                           // GACT_FILTER_KEPT .. GACT_FILTER_RELATIVE
constexpr int kFilterCounters = kFilterReasons + 1;         // records per final why, then the counted records

struct FilterRule {
    int min_identity, min_span, max_drop, sides;
    long long read_first;
    int n_reads;                                            // 0: no table, no per-read work (max_drop == 1000 then)
};

// the reads a record names on the requested sides, as indices into the window: x[0, return value); -1: outside the window
__device__ inline int filter_reads(const gact_overlap &r, const FilterRule &f, int (&x)[2])
{
    int m = 0;
    if (f.sides & GACT_COVER_REF) {
        const long long at = (long long)r.ref_id - f.read_first;
        x[m++] = at >= 0 && at < f.n_reads ? (int)at : -1;
    }
    if (f.sides & GACT_COVER_QUERY) {
        const long long at = (long long)r.query_id - f.read_first;
        x[m++] = at >= 0 && at < f.n_reads ? (int)at : -1;
    }
    return m;
}

__global__ void __launch_bounds__(kPassBlock)
filter_classify_kernel(const gact_overlap *__restrict__ rec, int n, const int *__restrict__ sel, int n_chosen,
                       const gact_path_summary *__restrict__ sums, FilterRule f, int *__restrict__ ident_out,
                       int *__restrict__ why_out, gact_read_filter *reads, int *flag)
{
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    if (k >= n_chosen) return;
    const int i = sel ? sel[k] : k;
    if (i < 0 || i >= n) { atomicOr(flag, kFilterBadIndex); ident_out[k] = 0; why_out[k] = GACT_FILTER_NOT_EMITTED; return; }
    const gact_overlap r = rec[i];
    const gact_path_summary s = sums[k];
    const long long m = (long long)s.n_eq + s.n_x;
    const long long cols = m + s.ins_bases + s.del_bases, t_span = m + s.del_bases, q_span = m + s.ins_bases;
    const int ident = cols > 0 ? (int)(1000ll * s.n_eq / cols) : 0;
    int why = GACT_FILTER_KEPT;
    if (!r.emitted) why = GACT_FILTER_NOT_EMITTED;
    else if (cols <= 0) why = GACT_FILTER_EMPTY;
    else if (ident < f.min_identity) why = GACT_FILTER_IDENTITY;
    else if ((t_span < q_span ? t_span : q_span) < f.min_span) why = GACT_FILTER_SPAN;
    ident_out[k] = ident;
    why_out[k] = why;
    if (f.n_reads == 0 || why == GACT_FILTER_NOT_EMITTED || why == GACT_FILTER_EMPTY) return;
    int x[2];
    const int sides = filter_reads(r, f, x);
    for (int j = 0; j < sides; j++)
        if (x[j] < 0) { atomicOr(flag, kFilterBadRead); return; }
    for (int j = 0; j < sides; j++) {
        gact_read_filter *t = reads + x[j];
        atomicAdd(&t->n_records, 1);
        if (why != GACT_FILTER_KEPT) continue;
        atomicAdd(&t->n_passed, 1);
        atomicMax(&t->best_permille, ident);
        atomicAdd((unsigned long long *)&t->eq_sum, (unsigned long long)s.n_eq);
        atomicAdd((unsigned long long *)&t->col_sum, (unsigned long long)cols);
    }
}

// flags[w]: the ballot of wave w (chosen records 64 w .. 64 w + 63); counts[b]: kept records of block b; counters: records per
// final why, then the counted ones
__global__ void __launch_bounds__(kPassBlock)
filter_flag_kernel(const gact_overlap *__restrict__ rec, const int *__restrict__ sel, int n_chosen, FilterRule f,
                   const int *__restrict__ ident_in, int *__restrict__ why_io, gact_read_filter *reads,
                   unsigned long long *__restrict__ flags, int *__restrict__ counts, unsigned long long *counters,
                   const int *__restrict__ flag)
{
    __shared__ int s_kept[kPassWaves];
    if (*flag) return;                                      // (the whole grid reads the same word: no wave is split at the barrier)
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    int why = -1;
    if (k < n_chosen) {
        why = why_io[k];
        if (why == GACT_FILTER_KEPT && f.n_reads > 0) {
            const gact_overlap r = rec[sel ? sel[k] : k];
            int x[2];
            const int sides = filter_reads(r, f, x);        // (inside the window: classify checked every counted record)
            if (f.max_drop < 1000) {
                const int ident = ident_in[k];
                for (int j = 0; j < sides; j++)
                    if (reads[x[j]].best_permille - ident > f.max_drop) why = GACT_FILTER_RELATIVE;
                if (why != GACT_FILTER_KEPT) why_io[k] = why;
            }
            if (why == GACT_FILTER_KEPT)
                for (int j = 0; j < sides; j++) atomicAdd(&reads[x[j]].n_kept, 1);
        }
    }
    const unsigned long long m_kept = __ballot(why == GACT_FILTER_KEPT);
    for (int reason = GACT_FILTER_NOT_EMITTED; reason < kFilterReasons; reason++) wave_count(counters + reason, why == reason);
    wave_count(counters + kFilterReasons, why >= 0 && why != GACT_FILTER_NOT_EMITTED && why != GACT_FILTER_EMPTY);
    if ((threadIdx.x & 63) == 0) {
        flags[(size_t)blockIdx.x * kPassWaves + wave] = m_kept;
        s_kept[wave] = __popcll(m_kept);
        if (m_kept) atomicAdd(counters + GACT_FILTER_KEPT, (unsigned long long)__popcll(m_kept));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0;
        for (int w = 0; w < kPassWaves; w++) a += s_kept[w];
        counts[blockIdx.x] = a;
    }
}

// one block: counts[0, nb) -> their exclusive scan, in place; *total = the kept records
__global__ void __launch_bounds__(kPassBlock)
filter_scan_kernel(int nb, int *__restrict__ counts, int *__restrict__ total_out, const int *__restrict__ flag)
{
    if (*flag) return;
    long long carry = 0;
    for (int base = 0; base < nb; base += kPassBlock) {
        const int k = base + (int)threadIdx.x;
        long long own[1] = {0}, before[1], total[1];
        if (k < nb) own[0] = counts[k];
        block_scan_step(own, before, total);
        if (k < nb) counts[k] = (int)(carry + before[0]);
        carry += total[0];
    }
    if (threadIdx.x == 0) *total_out = (int)carry;
}

// kept_at[offsets[b] + rank of k among block b's kept records] = k, kept_sel[same] = sel[k] (k without sel): ascending in k
__global__ void __launch_bounds__(kPassBlock)
filter_write_kernel(const unsigned long long *__restrict__ flags, const int *__restrict__ offsets, const int *__restrict__ sel,
                    int *__restrict__ kept_at, int *__restrict__ kept_sel, const int *__restrict__ flag)
{
    if (*flag) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long *fl = flags + (size_t)blockIdx.x * kPassWaves;
    const unsigned long long mine = fl[wave];
    if (!((mine >> lane) & 1)) return;
    int at = offsets[blockIdx.x] + __popcll(mine & ((1ull << lane) - 1));
    for (int w = 0; w < wave; w++) at += __popcll(fl[w]);
    const int k = blockIdx.x * kPassBlock + (int)threadIdx.x;
    kept_at[at] = k;
    kept_sel[at] = sel ? sel[k] : k;
}

}  // namespace gact

// One allocation: records (host ones only) | sel | sums | ident, why (4 each per chosen record) | flags (8 per wave) | block
// counts | counters, total, flag | table (32 n_reads) | kept_at | kept_sel.  counters .. table are zeroed together.
int gact_hip_filter_overlaps(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records, int32_t n_sel, const int32_t *sel,
                             const gact_path_summary *sums, int32_t sides, int32_t read_first, int32_t n_reads,
                             const gact_filter_params *params, int32_t *why, int32_t *kept_at, int32_t *kept_sel, int32_t cap,
                             int32_t *n_kept, gact_read_filter *reads)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (n_kept) *n_kept = 0;
    const gact_filter_params p = params ? *params : gact_filter_params{GACT_FILTER_DEFAULT_MIN_IDENTITY_PERMILLE,
                                                                       GACT_FILTER_DEFAULT_MIN_SPAN, GACT_FILTER_DEFAULT_MAX_DROP_PERMILLE};
    if (!sums) return fail(GACT_HIP_EINVAL, "filter_overlaps: sums is NULL (the identity comes from gact_hip_candidates_summaries)");
    if (p.min_identity_permille < 0 || p.min_identity_permille > 1000 || p.min_span < 0 || p.max_drop_permille < 0 ||
        p.max_drop_permille > 1000)
        return fail(GACT_HIP_EINVAL, "filter_overlaps: bad parameters (min_identity_permille = %d, 0 to 1000; min_span = %d, at least 0; "
                                     "max_drop_permille = %d, 0 to 1000)", p.min_identity_permille, p.min_span, p.max_drop_permille);
    if (sides != GACT_COVER_REF && sides != GACT_COVER_QUERY && sides != GACT_COVER_BOTH)
        return fail(GACT_HIP_EINVAL, "filter_overlaps: unknown sides %d (GACT_COVER_REF 1, GACT_COVER_QUERY 2, GACT_COVER_BOTH 3)", sides);
    // (n_sel as well: a kernel's lane forms its chosen record's position as an int, block index times kPassBlock plus thread)
    if (n < 0 || n > gact::kFilterMaxRecords || n_reads < 0 || (sel && (n_sel < 0 || n_sel > gact::kFilterMaxRecords)) || cap < 0)
        return fail(GACT_HIP_EINVAL, "filter_overlaps: bad arguments (n = %d, at most %d; n_reads = %d; n_sel = %d, at most %d; cap = %d)", n,
                    gact::kFilterMaxRecords, n_reads, n_sel, gact::kFilterMaxRecords, cap);
    if (p.max_drop_permille < 1000 && n_reads == 0)
        return fail(GACT_HIP_EINVAL, "filter_overlaps: max_drop_permille = %d needs the per-read table: n_reads is 0", p.max_drop_permille);
    Slot &sl = e->slots[slot];
    if ((rc = slot_records_check(sl, slot, n, records, "filter_overlaps"))) return rc;
    const int32_t n_chosen = n == 0 ? 0 : sel ? n_sel : n;
    if (n_chosen == 0) {                                    // (nothing for the device to do: a zeroed table)
        if (reads && n_reads > 0) std::memset(reads, 0, (size_t)n_reads * sizeof(gact_read_filter));
        return 0;
    }
    if ((rc = set_device(e))) return rc;
    PassScratch<gact_filter_stats> &fb = sl.filter;
    const size_t nb = ((size_t)n_chosen + gact::kPassBlock - 1) / gact::kPassBlock;
    const size_t at_sel = records ? up16((size_t)n * sizeof(gact_overlap)) : 0;
    const size_t at_sums = up16(at_sel + (sel ? (size_t)n_chosen * sizeof(int32_t) : 0));
    const size_t at_ident = up16(at_sums + (size_t)n_chosen * sizeof(gact_path_summary));
    const size_t at_why = up16(at_ident + (size_t)n_chosen * sizeof(int));
    const size_t at_flags = up16(at_why + (size_t)n_chosen * sizeof(int));
    const size_t at_counts = at_flags + nb * gact::kPassWaves * sizeof(unsigned long long);
    const size_t at_counters = up16(at_counts + nb * sizeof(int));
    const size_t at_total = at_counters + gact::kFilterCounters * sizeof(unsigned long long);      // total, flag: two ints
    const size_t at_table = up16(at_total + 2 * sizeof(int));
    const size_t at_kept = up16(at_table + (size_t)n_reads * sizeof(gact_read_filter));
    const size_t at_kept_sel = up16(at_kept + (size_t)n_chosen * sizeof(int));
    const size_t bytes = at_kept_sel + (size_t)n_chosen * sizeof(int);
    if (fb.reserve(bytes))
        return fail(GACT_HIP_ENOMEM, "filter_overlaps: device allocation failed (%d records, %d reads, %zu bytes)", n_chosen, n_reads, bytes);
    int *d_ident = (int *)(fb.p + at_ident), *d_why = (int *)(fb.p + at_why);
    unsigned long long *d_flags = (unsigned long long *)(fb.p + at_flags), *d_counters = (unsigned long long *)(fb.p + at_counters);
    int *d_counts = (int *)(fb.p + at_counts), *d_total = (int *)(fb.p + at_total), *d_flag = d_total + 1;
    gact_read_filter *d_reads = (gact_read_filter *)(fb.p + at_table);
    int *d_kept = (int *)(fb.p + at_kept), *d_kept_sel = (int *)(fb.p + at_kept_sel);
    // (a call that the device's own check refuses leaves the figures of the last call that was not refused: put back below)
    const gact_filter_stats stats_before = fb.stats;
    const bool timed_before = fb.timed;
    if ((rc = fb.begin(sl.stream, "filter_overlaps"))) return rc;
    DevRecords in;
    if ((rc = slot_records_stage(sl, fb.p, n, records, n_chosen, sel, at_sel, sums, at_sums, in))) return rc;
    HIP_TRY(hipMemsetAsync(d_counters, 0, at_kept - at_counters, sl.stream));
    const gact::FilterRule rule{p.min_identity_permille, p.min_span, p.max_drop_permille, sides, (long long)read_first, n_reads};
    const dim3 grid((unsigned)nb), block(gact::kPassBlock);
    hipLaunchKernelGGL(gact::filter_classify_kernel, grid, block, 0, sl.stream, in.rec, n, in.sel, n_chosen, in.sums, rule, d_ident,
                       d_why, d_reads, d_flag);
    hipLaunchKernelGGL(gact::filter_flag_kernel, grid, block, 0, sl.stream, in.rec, in.sel, n_chosen, rule, d_ident, d_why, d_reads,
                       d_flags, d_counts, d_counters, d_flag);
    hipLaunchKernelGGL(gact::filter_scan_kernel, dim3(1), block, 0, sl.stream, (int)nb, d_counts, d_total, d_flag);
    hipLaunchKernelGGL(gact::filter_write_kernel, grid, block, 0, sl.stream, d_flags, d_counts, in.sel, d_kept, d_kept_sel, d_flag);
    HIP_TRY(hipGetLastError());
    struct { unsigned long long counters[gact::kFilterCounters]; int total, flag; } h{};
    static_assert(sizeof h == gact::kFilterCounters * sizeof(unsigned long long) + 2 * sizeof(int), "counters | total | flag, as on the device");
    HIP_TRY(hipMemcpyAsync(&h, d_counters, sizeof h, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
    if (h.flag) { fb.stats = stats_before; fb.timed = timed_before; }
    if (h.flag & gact::kFilterBadIndex)
        return fail(GACT_HIP_EINVAL, "filter_overlaps: sel holds an index outside [0, %d)", n);
    if (h.flag)
        return fail(GACT_HIP_ERANGE, "filter_overlaps: a counted record names a read outside [%d, %lld) on a requested side", read_first,
                    (long long)read_first + n_reads);
    unsigned long long seen = 0;
    for (int reason = 0; reason < gact::kFilterReasons; reason++) seen += h.counters[reason];
    if (h.total < 0 || h.total > n_chosen || (unsigned long long)h.total != h.counters[GACT_FILTER_KEPT] || seen != (unsigned long long)n_chosen)
        return fail(GACT_HIP_EDEVICE, "filter_overlaps: the device kept %d of %d records and gave %llu a reason", h.total, n_chosen, seen);
    if (n_kept) *n_kept = h.total;
    const bool room = (!kept_at && !kept_sel) || cap >= h.total;
    if (why) HIP_TRY(hipMemcpyAsync(why, d_why, (size_t)n_chosen * sizeof(int), hipMemcpyDeviceToHost, sl.stream));
    if (reads && n_reads > 0)
        HIP_TRY(hipMemcpyAsync(reads, d_reads, (size_t)n_reads * sizeof(gact_read_filter), hipMemcpyDeviceToHost, sl.stream));
    if (room && kept_at && h.total > 0)
        HIP_TRY(hipMemcpyAsync(kept_at, d_kept, (size_t)h.total * sizeof(int), hipMemcpyDeviceToHost, sl.stream));
    if (room && kept_sel && h.total > 0)
        HIP_TRY(hipMemcpyAsync(kept_sel, d_kept_sel, (size_t)h.total * sizeof(int), hipMemcpyDeviceToHost, sl.stream));
    if ((rc = fb.end(sl.stream))) return rc;
    fb.stats.reads = n_reads;
    fb.stats.chosen = n_chosen;
    fb.stats.counted = (int64_t)h.counters[gact::kFilterReasons];
    fb.stats.kept = h.total;
    fb.stats.not_emitted = (int64_t)h.counters[GACT_FILTER_NOT_EMITTED];
    fb.stats.empty = (int64_t)h.counters[GACT_FILTER_EMPTY];
    fb.stats.identity = (int64_t)h.counters[GACT_FILTER_IDENTITY];
    fb.stats.span = (int64_t)h.counters[GACT_FILTER_SPAN];
    fb.stats.relative = (int64_t)h.counters[GACT_FILTER_RELATIVE];
    fb.stats.scratch_bytes = (int64_t)fb.bytes;
    if (!room)
        return fail(GACT_HIP_EINVAL, "filter_overlaps: %d records kept, room for %d: call again with room for *n_kept", h.total, cap);
    return 0;
}

int gact_hip_last_filter_stats(gact_hip_engine *e, int slot, gact_filter_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::filter, stats, "last_filter_stats", "has filtered nothing yet");
}
