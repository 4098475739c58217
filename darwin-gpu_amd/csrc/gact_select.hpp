// gact_select.hpp -- one overlap per class, selected on the device (gact_hip_select_overlaps).
//
// D-SOFT emits one candidate per diagonal bin over the threshold, a long overlap drifts over several bins, and the chains of
// those candidates converge on the same or nearly the same overlap.  The reference leaves the repeats to the shell
// (`cat darwin.*.out | sort | uniq`, README:25); here the records of a run are on the device already, and the selection runs
// ahead of the fetch and ahead of the second pass (paths, summaries) that would otherwise walk every repeat again.
//
//   GACT_SELECT_EXACT  class = the eight fields a line is printed from (gact.cpp:214-224); the lowest index survives
//   GACT_SELECT_PAIR   class = (ref_id, query_id, comp); the record with the highest score survives, then the larger
//                      (ae - ab) + (be - bb), then the lower index
// Records that were not emitted take no part.
//
// Three stages on the slot's stream, nothing on the host between them:
//   1 select_insert_kernel   every emitted record into a best-holder table of record indices with >= 2 n slots, keyed by its
//                            class (table_insert_best, gact_pass_device.hpp, which holds the argument); the class fields are
//                            read from the records, which no kernel here writes.  Each record keeps the slot it ended at.
//   2 select_flag_kernel     record i survives iff it is emitted and its slot holds i: one ballot per wave (kept: 64 flags in
//                            one word), popcounts per wave, summed per block.
//   3 select_scan_kernel     exclusive scan of the block counts, one block (block_scan_step);
//     select_write_kernel    every block writes its survivors at its offset in index order.
// Two levels on purpose: a single-pass scan has blocks spinning on other blocks' flags.  The list is ascending and the same on
// every run, whichever order the atomics landed in: the winner of a class is decided by a total order, not by arrival.
//
// Included by gact_engine.hip behind every other kernel and behind the engine's definitions (Slot, fail, HIP_TRY), inside its
// extern "C" block, as gact_gather.hpp is.
#pragma once

namespace gact {

constexpr int32_t kSelectMaxRecords = 1 << 30;    // (a slot position fits an int32)

__device__ inline uint32_t select_hash(const gact_overlap &r, int mode)
{
    uint32_t h = hash_mix(hash_mix(hash_mix(kHashSeed, (uint32_t)r.ref_id), (uint32_t)r.query_id), (uint32_t)r.comp);
    if (mode == GACT_SELECT_EXACT) {
        h = hash_mix(hash_mix(h, (uint32_t)r.ab), (uint32_t)r.ae);
        h = hash_mix(hash_mix(h, (uint32_t)r.bb), (uint32_t)r.be);
        h = hash_mix(h, (uint32_t)r.score);
    }
    return hash_final(h);
}

__device__ inline bool select_same_class(const gact_overlap &a, const gact_overlap &b, int mode)
{
    const bool pair = a.ref_id == b.ref_id && a.query_id == b.query_id && a.comp == b.comp;
    if (mode == GACT_SELECT_PAIR) return pair;
    return pair && a.ab == b.ab && a.ae == b.ae && a.bb == b.bb && a.be == b.be && a.score == b.score;
}

// is record i (a) better than record j (b) of its class?  i != j
__device__ inline bool select_better(int i, const gact_overlap &a, int j, const gact_overlap &b, int mode)
{
    if (mode == GACT_SELECT_PAIR) {
        if (a.score != b.score) return a.score > b.score;
        const long long sa = ((long long)a.ae - a.ab) + ((long long)a.be - a.bb);
        const long long sb = ((long long)b.ae - b.ab) + ((long long)b.be - b.bb);
        if (sa != sb) return sa > sb;
    }
    return i < j;
}

__global__ void __launch_bounds__(kPassBlock)
select_insert_kernel(const gact_overlap *__restrict__ rec, int n, int mode, int *table, uint32_t mask, int *__restrict__ pos)
{
    const int i = blockIdx.x * kPassBlock + threadIdx.x;
    if (i >= n) return;
    const gact_overlap r = rec[i];
    if (!r.emitted) { pos[i] = -1; return; }
    pos[i] = (int)table_insert_best(table, mask, select_hash(r, mode), i,
                                    [&](int j) { return select_same_class(r, rec[j], mode); },
                                    [&](int j) { return select_better(i, r, j, rec[j], mode); });
}

// flags[w]: the ballot of wave w (records 64 w .. 64 w + 63); counts[b] / emitted[b]: survivors / emitted records of block b
__global__ void __launch_bounds__(kPassBlock)
select_flag_kernel(int n, const int *__restrict__ table, const int *__restrict__ pos, unsigned long long *__restrict__ flags,
                   int *__restrict__ counts, int *__restrict__ emitted)
{
    __shared__ int s_sel[kPassBlock / 64], s_emit[kPassBlock / 64];
    const int i = blockIdx.x * kPassBlock + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    const int p = i < n ? pos[i] : -1;
    const bool survives = p >= 0 && table[p] == i;
    const unsigned long long m_sel = __ballot(survives), m_emit = __ballot(p >= 0);
    if ((threadIdx.x & 63) == 0) {
        flags[(size_t)blockIdx.x * (kPassBlock / 64) + wave] = m_sel;
        s_sel[wave] = __popcll(m_sel);
        s_emit[wave] = __popcll(m_emit);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
        for (int w = 0; w < kPassBlock / 64; w++) { a += s_sel[w]; b += s_emit[w]; }
        counts[blockIdx.x] = a;
        emitted[blockIdx.x] = b;
    }
}

// one block: counts[0, nb) -> their exclusive scan, in place; totals[0] = survivors, totals[1] = emitted records
__global__ void __launch_bounds__(kPassBlock)
select_scan_kernel(int nb, int *__restrict__ counts, const int *__restrict__ emitted, int *__restrict__ totals)
{
    long long carry = 0, carry_emit = 0;
    for (int base = 0; base < nb; base += kPassBlock) {
        const int k = base + (int)threadIdx.x;
        long long own[2] = {0, 0}, before[2], total[2];
        if (k < nb) { own[0] = counts[k]; own[1] = emitted[k]; }              // (one branch: the loads fly together)
        block_scan_step(own, before, total);
        if (k < nb) counts[k] = (int)(carry + before[0]);
        carry += total[0];
        carry_emit += total[1];
    }
    if (threadIdx.x == 0) { totals[0] = (int)carry; totals[1] = (int)carry_emit; }
}

// sel[offsets[b] + rank of i among block b's survivors] = i: ascending, since the offsets and the ranks are
__global__ void __launch_bounds__(kPassBlock)
select_write_kernel(const unsigned long long *__restrict__ flags, const int *__restrict__ offsets, int *__restrict__ sel)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long *f = flags + (size_t)blockIdx.x * (kPassBlock / 64);
    const unsigned long long mine = f[wave];
    if (!((mine >> lane) & 1)) return;
    int at = offsets[blockIdx.x] + __popcll(mine & ((1ull << lane) - 1));
    for (int w = 0; w < wave; w++) at += __popcll(f[w]);
    sel[at] = blockIdx.x * kPassBlock + (int)threadIdx.x;
}

}  // namespace gact

// records == NULL: records [0, n) of the slot's device array, behind the slot's last run (stream order); else the caller's n
// records, copied into the scratch first.  One allocation: records (host ones only) | table | positions | flags | block counts,
// emitted counts, totals | sel -- 4 * table_slots + about 8.2 bytes per record (+ 56 for a host record).
int gact_hip_select_overlaps(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records, int32_t mode, int32_t *sel,
                             int32_t sel_cap, int32_t *n_sel)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (!n_sel) return fail(GACT_HIP_EINVAL, "select_overlaps: n_sel is NULL");
    *n_sel = 0;
    if (mode != GACT_SELECT_EXACT && mode != GACT_SELECT_PAIR)
        return fail(GACT_HIP_EINVAL, "select_overlaps: unknown mode %d (GACT_SELECT_EXACT 0, GACT_SELECT_PAIR 1)", mode);
    if (n < 0 || n > gact::kSelectMaxRecords || sel_cap < 0)
        return fail(GACT_HIP_EINVAL, "select_overlaps: bad arguments (n = %d, at most %d; sel_cap = %d)", n, gact::kSelectMaxRecords, sel_cap);
    if (n == 0) return 0;
    Slot &sl = e->slots[slot];
    if ((rc = slot_records_check(sl, slot, n, records, "select_overlaps"))) return rc;
    if ((rc = set_device(e))) return rc;
    PassScratch<gact_select_stats> &sb = sl.select;
    size_t slots = 2;
    while (slots < 2 * (size_t)n) slots <<= 1;
    const size_t nb = ((size_t)n + gact::kPassBlock - 1) / gact::kPassBlock;
    const size_t at_table = records ? up16((size_t)n * sizeof(gact_overlap)) : 0;
    const size_t at_pos = at_table + slots * sizeof(int);
    const size_t at_flags = up16(at_pos + (size_t)n * sizeof(int));
    const size_t at_counts = at_flags + nb * (gact::kPassBlock / 64) * sizeof(unsigned long long);
    const size_t at_sel = up16(at_counts + (2 * nb + 2) * sizeof(int));
    const size_t bytes = at_sel + (size_t)n * sizeof(int);
    if (sb.reserve(bytes)) return fail(GACT_HIP_ENOMEM, "select_overlaps: device allocation failed (%d records, %zu bytes)", n, bytes);
    int *d_table = (int *)(sb.p + at_table), *d_pos = (int *)(sb.p + at_pos);
    unsigned long long *d_flags = (unsigned long long *)(sb.p + at_flags);
    int *d_counts = (int *)(sb.p + at_counts), *d_emitted = d_counts + nb, *d_totals = d_counts + 2 * nb;
    int *d_sel = (int *)(sb.p + at_sel);
    if ((rc = sb.begin(sl.stream, "select_overlaps"))) return rc;
    DevRecords in;
    if ((rc = slot_records_stage(sl, sb.p, n, records, n, nullptr, 0, nullptr, 0, in))) return rc;
    const gact_overlap *d_rec = in.rec;
    HIP_TRY(hipMemsetAsync(d_table, 0xff, slots * sizeof(int), sl.stream));          // kTableEmpty everywhere
    const dim3 grid((unsigned)nb), block(gact::kPassBlock);
    hipLaunchKernelGGL(gact::select_insert_kernel, grid, block, 0, sl.stream, d_rec, n, mode, d_table, (uint32_t)(slots - 1), d_pos);
    hipLaunchKernelGGL(gact::select_flag_kernel, grid, block, 0, sl.stream, n, d_table, d_pos, d_flags, d_counts, d_emitted);
    hipLaunchKernelGGL(gact::select_scan_kernel, dim3(1), block, 0, sl.stream, (int)nb, d_counts, d_emitted, d_totals);
    hipLaunchKernelGGL(gact::select_write_kernel, grid, block, 0, sl.stream, d_flags, d_counts, d_sel);
    HIP_TRY(hipGetLastError());
    int totals[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
    if (totals[0] < 0 || totals[0] > totals[1] || totals[1] > n)
        return fail(GACT_HIP_EDEVICE, "select_overlaps: the device counted %d survivors of %d emitted records of %d", totals[0], totals[1], n);
    *n_sel = totals[0];
    const bool room = sel && sel_cap >= totals[0];
    if (room && totals[0] > 0)
        HIP_TRY(hipMemcpyAsync(sel, d_sel, (size_t)totals[0] * sizeof(int), hipMemcpyDeviceToHost, sl.stream));
    if ((rc = sb.end(sl.stream))) return rc;
    sb.stats.emitted = totals[1];
    sb.stats.selected = totals[0];
    sb.stats.table_slots = (int64_t)slots;
    sb.stats.scratch_bytes = (int64_t)sb.bytes;
    if (!room)
        return fail(GACT_HIP_EINVAL, "select_overlaps: %d records selected, room for %d: call again with room for *n_sel", totals[0],
                    sel ? sel_cap : 0);
    return 0;
}

int gact_hip_last_select_stats(gact_hip_engine *e, int slot, gact_select_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::select, stats, "last_select_stats", "has made no selection yet");
}
