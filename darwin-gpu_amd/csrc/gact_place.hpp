// gact_place.hpp -- every read placed on the device: primary, supplementary, secondary, MAPQ (gact_hip_place_reads).
//
// Reads against a reference or against contigs: the records of a run say where pieces of a read align, and a user of a
// mapper asks where the read GOES, how sure that is, and whether it is split.  All records of a query read are on the slot that
// ran its batch, so the placement runs there, behind the run (and the selection, and the summaries), ahead of the fetch.  The
// rule is stated in include/gact_hip.h and restated in tests/place_model.py; all of it is integers.
//
// Four stages on the slot's stream, nothing on the host between them:
//   1 place_count_kernel    one lane per chosen record: its interval on the original read (the one GACT_COVER_QUERY puts there:
//                           mirrored for comp == 1, begun by the summary where one is given, clipped), kept with its score, its
//                           read and its span so that no later stage touches the records or the summaries; the window check in
//                           front of the one use of the id as an index (a bit of one flag word, read by the host before it copies
//                           anything out); the record's place as GACT_PLACE_NONE; and the count of its read.  A read's records
//                           sit together, so a run of lanes with one read makes ONE atomicAdd of the run's length (two ballots,
//                           one __ffsll); lanes of other reads make their own.
//   2 place_scan_kernel     one block: the exclusive scan of the per-read counts (block_scan_step) = where a read's list begins.
//   3 place_scatter_kernel  one lane per chosen record: a counted one goes to first[read] + atomicAdd(fill[read], 1) of the CSR
//                           list, as graph_scatter_kernel's holders do -- in arrival order, which the next stage removes, since
//                           it orders by a total order.
//   4 place_read_kernel     one wave per read, kPassWaves reads a block, grid-stride: the hot path.
//       rank   a lane holds one record of a 64-record chunk of the read's list and streams over the whole list, which is loaded
//              64 records at a time, one per lane, and passed round with v_readlane (a wave-uniform load per record waited
//              for memory at every step: 130 ns a step, measured), counting the records that precede its own; the record goes
//              to ord[first + rank].  Any m: a read of m records takes about m * m / 64 wave steps.
//       walk   the parents live ONE PER LANE: lane j holds (b, e), k, score, s2 and rank of the j-th parent in registers.  The
//              ranked records are loaded 64 at a time, one per lane, and broadcast in turn (four v_readlane with a wave-uniform
//              lane); every lane with a parent tests the mask rule, one __ballot follows, and __ffsll of it is the adopting
//              parent -- the first in the order the parents were made, which is the lanes' order.  A zero ballot with fewer than
//              64 parents makes the record lane n_parents' parent; with 64, an extra.  The lane that loaded a record keeps its
//              kind and parent and stores the 16-byte place after the chunk; a parent's place is stored once, at the end, by
//              its lane, with the MAPQ its secondaries left it; lane 0 stores the read's 32 bytes as two 16-byte vectors.
//              No LDS, no atomics and no barrier inside the walk: the waves of a block are independent.
// The statistics are kept per wave over its reads, added up over the block's four waves behind the loop (40 bytes of LDS a
// wave, one barrier) and leave as five atomics a block: one atomic per read on five addresses was most of the call's time
// with 70,001 reads (2.0 ms).  Ordinary vector global atomics on integers throughout, and every value they leave is the same
// in whichever order they land.
//
// Known limit: one wave per read and a ranking of m * m / 64 steps is right for reads against a reference (tens of records a
// read); a read with many thousands of records (a repeat against everything) is ranked correctly, and slowly.
//
// Included by gact_engine.hip behind every other kernel and behind the engine's definitions (Slot, fail, HIP_TRY), inside its
// extern "C" block, as gact_select.hpp is.
#pragma once

namespace gact {

constexpr int32_t kPlaceMaxRecords = 1 << 30;
constexpr int kPlaceBadIndex = 1, kPlaceBadRead = 2;    // bits of the flag word
// the statistics' counters
constexpr int kPlaceCounted = 0, kPlaceParents = 1, kPlaceSecondaries = 2, kPlaceExtras = 3, kPlaceMaxOnRead = 4, kPlaceCounters = 8;

// a chosen record as the later stages see it: x = b, y = e (b < e: counted), z = score, w = its read in the window
// (place_count_kernel) or its chosen index k (the CSR list and the ranked list)
typedef int4 PlaceItem;

// does record (score a, span sa, chosen index ka) precede (b, sb, kb) in a read's order?  A total order: k is unique
__device__ __forceinline__ bool place_precedes(int a, long long sa, int ka, int b, long long sb, int kb)
{
    if (a != b) return a > b;
    if (sa != sb) return sa > sb;
    return ka < kb;
}

// x of lane `from`, which is the same in every lane of the wave: one v_readlane, no LDS crossbar
__device__ __forceinline__ int lane_value(int x, int from)
{
    return __builtin_amdgcn_readlane(x, from);
}

__global__ void __launch_bounds__(kPassBlock)
place_count_kernel(const gact_overlap *__restrict__ rec, int n, const int *__restrict__ sel, int n_chosen,
                   const gact_path_summary *__restrict__ sums, int read_first, int n_reads, const int *__restrict__ lens,
                   int *counts, PlaceItem *__restrict__ items, long long *__restrict__ spans, gact_placement *__restrict__ place,
                   int *flag)
{
    const int k = blockIdx.x * kPassBlock + threadIdx.x, lane = threadIdx.x & 63;
    int q = -1, b = 0, e = 0, score = 0;
    long long span = 0;
    if (k < n_chosen) {
        const int i = sel ? sel[k] : k;
        if (i < 0 || i >= n) {
            atomicOr(flag, kPlaceBadIndex);
        } else {
            const gact_overlap r = rec[i];
            const long long at = (long long)r.query_id - read_first;
            if (r.emitted && (at < 0 || at >= n_reads)) {
                atomicOr(flag, kPlaceBadRead);
            } else if (r.emitted) {
                const long long len = lens[at];
                long long ab = r.ab, bb = r.bb, be = r.be;
                if (sums) begins_from_summary(r, sums[k], ab, bb);
                if (r.comp) { const long long t = bb; bb = len - be; be = len - t; }   // the reverse-complement strand's [bb, be) on the read itself
                if (bb < 0) bb = 0;
                if (be > len) be = len;
                if (bb < be) { q = (int)at; b = (int)bb; e = (int)be; }
                score = r.score;
                span = ((long long)r.ae - r.ab) + ((long long)r.be - r.bb);
            }
        }
        items[k] = make_int4(b, e, score, q);
        spans[k] = span;
        *(int4 *)&place[k] = make_int4(GACT_PLACE_NONE, 0, -1, -1);
    }
    // one atomicAdd per run of lanes with the same read: the head of a run adds the run's length
    const bool counted = q >= 0;
    const int q_below = __shfl_up(q, 1);
    const bool head = counted && (lane == 0 || q_below != q);
    const unsigned long long m_head = __ballot(head), m_counted = __ballot(counted);
    if (head) {
        const unsigned long long stops = (m_head | ~m_counted) & ~((2ull << lane) - 1);      // (lane 63: 2 << 63 = 0, no bit above)
        atomicAdd(&counts[q], (stops ? __ffsll(stops) - 1 : 64) - lane);
    }
}

// one block: counts[0, n_reads) -> their exclusive scan, in place; counts[n_reads] = the counted records
__global__ void __launch_bounds__(kPassBlock)
place_scan_kernel(int n_reads, int *__restrict__ counts)
{
    long long carry = 0;
    for (int base = 0; base < n_reads; base += kPassBlock) {
        const int i = base + (int)threadIdx.x;
        long long own[1] = {0}, before[1], total[1];
        if (i < n_reads) own[0] = counts[i];
        block_scan_step(own, before, total);
        if (i < n_reads) counts[i] = (int)(carry + before[0]);
        carry += total[0];
    }
    if (threadIdx.x == 0) counts[n_reads] = (int)carry;
}

__global__ void __launch_bounds__(kPassBlock)
place_scatter_kernel(int n_chosen, const PlaceItem *__restrict__ items, const long long *__restrict__ spans,
                     const int *__restrict__ first, int *fill, PlaceItem *__restrict__ csr, long long *__restrict__ csr_spans)
{
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    if (k >= n_chosen) return;
    const PlaceItem it = items[k];
    if (it.w < 0) return;
    const int at = first[it.w] + atomicAdd(&fill[it.w], 1);
    csr[at] = make_int4(it.x, it.y, it.z, k);
    csr_spans[at] = spans[k];
}

// ord is written in the rank phase and read in the walk by other lanes of the same wave: no __restrict__, and a fence between
__global__ void __launch_bounds__(kPassBlock)
place_read_kernel(int n_reads, const int *__restrict__ first, const PlaceItem *__restrict__ csr, const long long *__restrict__ csr_spans,
                  PlaceItem *ord, int mask_permille, int mapq_cap, gact_placement *__restrict__ place,
                  gact_read_place *__restrict__ reads, unsigned long long *counters)
{
    __shared__ unsigned long long s_stats[kPassWaves][kPlaceMaxOnRead + 1];
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kPassWaves + (threadIdx.x >> 6), n_waves = gridDim.x * kPassWaves;
    unsigned long long counted = 0, parents = 0, secondaries = 0, extras = 0, most = 0;       // of this wave's reads
    for (int read = wave; read < n_reads; read += n_waves) {
        const int at = first[read], m = first[read + 1] - at;
        int4 *out = (int4 *)&reads[read];
        if (m <= 0) {
            if (lane == 0) { out[0] = make_int4(0, -1, 0, 0); out[1] = make_int4(0, 0, 0, 0); }
            continue;
        }
        // rank: my record against every record of the read, which comes by 64 at a time, one per lane, and is passed round
        for (int c0 = 0; c0 < m; c0 += 64) {
            const bool valid = c0 + lane < m;
            const PlaceItem mine = valid ? csr[at + c0 + lane] : make_int4(0, 0, 0, 0);
            const long long my_span = valid ? csr_spans[at + c0 + lane] : 0;
            int rank = 0;
            for (int f0 = 0; f0 < m; f0 += 64) {
                const int there = min(64, m - f0);
                const PlaceItem o = lane < there ? csr[at + f0 + lane] : make_int4(0, 0, 0, 0);
                const long long o_span = lane < there ? csr_spans[at + f0 + lane] : 0;
                const int o_lo = (int)(o_span & 0xffffffffll), o_hi = (int)(o_span >> 32);
                for (int j = 0; j < there; j++) {
                    const long long span = ((long long)lane_value(o_hi, j) << 32) | (unsigned)lane_value(o_lo, j);
                    rank += place_precedes(lane_value(o.z, j), span, lane_value(o.w, j), mine.z, my_span, mine.w);
                }
            }
            if (valid) ord[at + rank] = mine;
        }
        __threadfence_block();
        // walk: lane j holds the j-th parent
        int pb = 0, pe = 0, pk = -1, ps1 = 0, ps2 = 0, prank = 0;
        int n_parents = 0, n_secondary = 0, n_extra = 0;
        for (int t0 = 0; t0 < m; t0 += 64) {
            const int here = min(64, m - t0);
            const PlaceItem it = lane < here ? ord[at + t0 + lane] : make_int4(0, 0, 0, 0);
            int my_kind = GACT_PLACE_NONE, my_parent = -1;
            for (int j = 0; j < here; j++) {
                const int tb = lane_value(it.x, j), te = lane_value(it.y, j), ts = lane_value(it.z, j), tk = lane_value(it.w, j);
                bool masks = false;
                if (lane < n_parents) {
                    const int ov = min(te, pe) - max(tb, pb);
                    masks = ov > 0 && 1000ll * ov >= (long long)mask_permille * min(te - tb, pe - pb);
                }
                const unsigned long long hit = __ballot(masks);
                int kind, parent = tk;
                if (hit) {
                    const int a = __ffsll(hit) - 1;
                    kind = GACT_PLACE_SECONDARY;
                    parent = lane_value(pk, a);
                    if (lane == a) ps2 = max(ps2, ts);
                    n_secondary++;
                } else if (n_parents < GACT_PLACE_MAX_PARENTS) {
                    kind = n_parents == 0 ? GACT_PLACE_PRIMARY : GACT_PLACE_SUPPLEMENTARY;
                    if (lane == n_parents) { pb = tb; pe = te; pk = tk; ps1 = ts; ps2 = 0; prank = t0 + j; }
                    n_parents++;
                } else {
                    kind = GACT_PLACE_EXTRA;
                    n_extra++;
                }
                if (lane == j) { my_kind = kind; my_parent = parent; }
            }
            // (a parent's place waits for its MAPQ)
            if (lane < here && (my_kind == GACT_PLACE_SECONDARY || my_kind == GACT_PLACE_EXTRA))
                *(int4 *)&place[it.w] = make_int4(my_kind, 0, my_parent, t0 + lane);
        }
        int s2 = 0, mapq = 0;
        if (lane < n_parents) {
            s2 = max(0, min(ps1, ps2));
            if (ps1 > 0) mapq = (int)((long long)mapq_cap * (ps1 - s2) / ps1);
            *(int4 *)&place[pk] = make_int4(lane == 0 ? GACT_PLACE_PRIMARY : GACT_PLACE_SUPPLEMENTARY, mapq, pk, prank);
        }
        if (lane == 0) {
            out[0] = make_int4(m, pk, n_parents - 1, n_secondary);
            out[1] = make_int4(n_extra, ps1, s2, mapq);
        }
        counted += m; parents += n_parents; secondaries += n_secondary; extras += n_extra;
        most = max(most, (unsigned long long)m);
    }
    // the statistics: the block's four waves added up, five atomics a block (every wave gets here: the loop has no return)
    if (lane == 0) {
        unsigned long long *mine = s_stats[threadIdx.x >> 6];
        mine[kPlaceCounted] = counted; mine[kPlaceParents] = parents; mine[kPlaceSecondaries] = secondaries;
        mine[kPlaceExtras] = extras; mine[kPlaceMaxOnRead] = most;
    }
    __syncthreads();
    if (threadIdx.x <= kPlaceMaxOnRead) {
        unsigned long long v = 0;
        for (int w = 0; w < kPassWaves; w++)
            v = threadIdx.x == kPlaceMaxOnRead ? max(v, s_stats[w][threadIdx.x]) : v + s_stats[w][threadIdx.x];
        if (v) {
            if (threadIdx.x == kPlaceMaxOnRead) atomicMax(&counters[kPlaceMaxOnRead], v);
            else atomicAdd(&counters[threadIdx.x], v);
        }
    }
}

}  // namespace gact

// One allocation: records (host ones only) | sel | sums | lens (4 n_reads) | first (4 (n_reads + 1)) | fill (4 n_reads) | flag,
// counters | reads (32 n_reads) | items (16 n_chosen) | CSR items (16 n_chosen) | ranked items (16 n_chosen) | place
// (16 n_chosen) | spans, CSR spans (8 n_chosen each).  first | fill | flag, counters are zeroed together.
int gact_hip_place_reads(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records, int32_t n_sel, const int32_t *sel,
                         const gact_path_summary *sums, int32_t read_first, int32_t n_reads, const int32_t *read_lens,
                         const gact_place_params *params, gact_placement *place, gact_read_place *reads)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    const gact_place_params p = params ? *params : gact_place_params{GACT_PLACE_DEFAULT_MASK_PERMILLE, GACT_PLACE_DEFAULT_MAPQ_CAP};
    if (p.mask_permille < 0 || p.mask_permille > 1000 || p.mapq_cap < 0 || p.mapq_cap > 255)
        return fail(GACT_HIP_EINVAL, "place_reads: bad parameters (mask_permille = %d, 0 .. 1000; mapq_cap = %d, 0 .. 255)",
                    p.mask_permille, p.mapq_cap);
    if (n < 0 || n > gact::kPlaceMaxRecords || n_sel < 0 || n_sel > gact::kPlaceMaxRecords || n_reads < 0 || read_first < 0)
        return fail(GACT_HIP_EINVAL, "place_reads: bad arguments (n = %d, n_sel = %d, at most %d; n_reads = %d; read_first = %d)", n,
                    n_sel, gact::kPlaceMaxRecords, n_reads, read_first);
    if (n_reads > 0 && !read_lens) return fail(GACT_HIP_EINVAL, "place_reads: read_lens is NULL");
    for (int32_t i = 0; i < n_reads; i++)
        if (read_lens[i] < 0)
            return fail(GACT_HIP_EINVAL, "place_reads: read %lld has the negative length %d", (long long)read_first + i, read_lens[i]);
    Slot &sl = e->slots[slot];
    if ((rc = slot_records_check(sl, slot, n, records, "place_reads"))) return rc;
    const int32_t n_chosen = sel ? n_sel : n;
    for (int32_t k = 0; sel && k < n_sel; k++)
        if (sel[k] < 0 || sel[k] >= n)
            return fail(GACT_HIP_EINVAL, "place_reads: sel[%d] = %d outside [0, %d)", k, sel[k], n);
    if (n_reads == 0) return 0;
    if (n_chosen == 0) {
        for (int32_t i = 0; reads && i < n_reads; i++) reads[i] = gact_read_place{0, -1, 0, 0, 0, 0, 0, 0};
        return 0;
    }
    if ((rc = set_device(e))) return rc;
    PassScratch<gact_place_stats> &pb = sl.place;
    const size_t nr = (size_t)n_reads, nc = (size_t)n_chosen;
    const size_t at_sel = records ? up16((size_t)n * sizeof(gact_overlap)) : 0;
    const size_t at_sums = up16(at_sel + (sel ? nc * sizeof(int32_t) : 0));
    const size_t at_lens = up16(at_sums + (sums ? nc * sizeof(gact_path_summary) : 0));
    const size_t at_first = up16(at_lens + nr * sizeof(int32_t));
    const size_t at_fill = at_first + (nr + 1) * sizeof(int32_t);
    const size_t at_flag = up16(at_fill + nr * sizeof(int32_t));
    const size_t at_counters = at_flag + 16;
    const size_t at_reads = at_counters + gact::kPlaceCounters * sizeof(unsigned long long);
    const size_t at_items = at_reads + nr * sizeof(gact_read_place);
    const size_t at_csr = at_items + nc * sizeof(gact::PlaceItem);
    const size_t at_ord = at_csr + nc * sizeof(gact::PlaceItem);
    const size_t at_place = at_ord + nc * sizeof(gact::PlaceItem);
    const size_t at_spans = at_place + nc * sizeof(gact_placement);
    const size_t at_csr_spans = at_spans + nc * sizeof(long long);
    const size_t bytes = at_csr_spans + nc * sizeof(long long);
    if (pb.reserve(bytes))
        return fail(GACT_HIP_ENOMEM, "place_reads: device allocation failed (%d records, %d reads, %zu bytes)", n_chosen, n_reads, bytes);
    int *d_lens = (int *)(pb.p + at_lens), *d_first = (int *)(pb.p + at_first), *d_fill = (int *)(pb.p + at_fill);
    int *d_flag = (int *)(pb.p + at_flag);
    unsigned long long *d_counters = (unsigned long long *)(pb.p + at_counters);
    gact_read_place *d_reads = (gact_read_place *)(pb.p + at_reads);
    gact::PlaceItem *d_items = (gact::PlaceItem *)(pb.p + at_items), *d_csr = (gact::PlaceItem *)(pb.p + at_csr);
    gact::PlaceItem *d_ord = (gact::PlaceItem *)(pb.p + at_ord);
    gact_placement *d_place = (gact_placement *)(pb.p + at_place);
    long long *d_spans = (long long *)(pb.p + at_spans), *d_csr_spans = (long long *)(pb.p + at_csr_spans);
    if ((rc = pb.begin(sl.stream, "place_reads"))) return rc;
    DevRecords in;
    if ((rc = slot_records_stage(sl, pb.p, n, records, n_chosen, sel, at_sel, sums, at_sums, in))) return rc;
    HIP_TRY(hipMemcpyAsync(d_lens, read_lens, nr * sizeof(int32_t), hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemsetAsync(d_first, 0, at_reads - at_first, sl.stream));
    const dim3 block(gact::kPassBlock), lanes = lane_blocks(nc);
    hipLaunchKernelGGL(gact::place_count_kernel, lanes, block, 0, sl.stream, in.rec, n, in.sel, n_chosen, in.sums, read_first, n_reads,
                       d_lens, d_first, d_items, d_spans, d_place, d_flag);
    hipLaunchKernelGGL(gact::place_scan_kernel, dim3(1), block, 0, sl.stream, n_reads, d_first);
    hipLaunchKernelGGL(gact::place_scatter_kernel, lanes, block, 0, sl.stream, n_chosen, d_items, d_spans, d_first, d_fill, d_csr,
                       d_csr_spans);
    hipLaunchKernelGGL(gact::place_read_kernel, wave_blocks(e, nr), block, 0, sl.stream, n_reads, d_first, d_csr, d_csr_spans, d_ord,
                       p.mask_permille, p.mapq_cap, d_place, d_reads, d_counters);
    HIP_TRY(hipGetLastError());
    int flag = 0;
    unsigned long long counters[gact::kPlaceCounters];
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
    if (flag & gact::kPlaceBadIndex)
        return fail(GACT_HIP_EINVAL, "place_reads: sel holds an index outside [0, %d)", n);
    if (flag)
        return fail(GACT_HIP_ERANGE, "place_reads: an emitted chosen record names a query read outside the window [%d, %lld)", read_first,
                    (long long)read_first + n_reads);
    if (place) HIP_TRY(hipMemcpyAsync(place, d_place, nc * sizeof(gact_placement), hipMemcpyDeviceToHost, sl.stream));
    if (reads) HIP_TRY(hipMemcpyAsync(reads, d_reads, nr * sizeof(gact_read_place), hipMemcpyDeviceToHost, sl.stream));
    if ((rc = pb.end(sl.stream))) return rc;
    pb.stats.reads = n_reads;
    pb.stats.max_records = (int32_t)counters[gact::kPlaceMaxOnRead];
    pb.stats.counted = (int64_t)counters[gact::kPlaceCounted];
    pb.stats.parents = (int64_t)counters[gact::kPlaceParents];
    pb.stats.secondaries = (int64_t)counters[gact::kPlaceSecondaries];
    pb.stats.extras = (int64_t)counters[gact::kPlaceExtras];
    pb.stats.scratch_bytes = (int64_t)pb.bytes;
    return 0;
}

int gact_hip_last_place_stats(gact_hip_engine *e, int slot, gact_place_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::place, stats, "last_place_stats", "has placed no reads yet");
}
