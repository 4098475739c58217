// gact_graph.hpp -- the overlap graph of an overlap set, made on the device (gact_hip_overlap_graph).
//
// What an assembler's layout stage reads: which reads lie inside another one, and for the rest the bidirected dovetail arcs,
// each once, with the ones a triangle explains flagged.  The records of a run are on the device already, and so are the indices
// of gact_hip_select_overlaps, the summaries of gact_hip_candidates_summaries and the spans of gact_hip_read_coverage; the rule
// is stated in include/gact_hip.h and restated in tests/graph_model.py.
//
// Nine kernels on the slot's stream, nothing on the host between them:
//   1 graph_class_kernel    one lane per chosen record: its class, and for a DOVETAIL record its two proposals (the arc and the
//                           complement, as gact_graph_arc; u = -1 for every other record).  atomicMin of the record index into
//                           contained_by (unsigned, 0xffffffff = none), atomicAdd into the read's counters, one wave_count per
//                           class into the statistics, atomicOr into a flag word for a sel index outside [0, n) or a read
//                           id outside [0, n_reads) -- the host reads that word before it copies anything out.
//   2 graph_insert_kernel   behind the kernel boundary (contained_by is final): one lane per proposal whose two reads are not
//                           contained, into a best-holder table of proposal indices (table_insert_best, gact_pass_device.hpp,
//                           which holds the argument) with >= twice the proposals slots, keyed (u, v); better is the higher
//                           score, then the lower record index, then the lower proposal index: a total order.
//   3 graph_degree_kernel   one lane per table slot: a holder adds 1 to the out-degree of its u.
//   4 graph_scan_kernel     exclusive scan of the 2 n_reads degrees, one block (block_scan_step; no look-back).
//   5 graph_scatter_kernel  one lane per table slot: the holder goes to first[u] + atomicAdd(fill[u], 1) of the CSR list -- in
//                           arrival order, which the next kernel removes.
//   6 graph_order_kernel    one wave per vertex, grid-stride: lanes stride over the vertex's list (it may be longer than 64), each
//                           counts the entries with a smaller (len, v) -- no two are equal, v is unique in a list -- and writes
//                           its proposal as the arc at first[u] + that rank, flags 0.  The arc array is ascending by (u, len, v).
//   7 graph_reduce_kernel   one wave per vertex u, lanes over the pairs (x, w) of its list: w -> x is looked up in the table, and
//                           len(u->w) + len(w->x) <= len(u->x) + fuzz sets bit 0 of u -> x with atomicOr.
//   8 graph_mirror_kernel   behind the kernel boundary, one lane per arc u -> x: finds x^1 -> u^1 in x^1's list, reads its bit 0,
//                           and sets bit 1 of its own arc.  It reads bit 0 and writes bit 1 only.
//   9 graph_reads_kernel    one lane per read: contained_by, deg and kept of its two vertices; the totals into the statistics.
// Ordinary vector global atomics on integers throughout, and every value they leave is the same in whichever order they land.
// No LDS but the scan's, no spinning on other waves.
//
// Known limit: a vertex of out-degree d costs about d^2 look-ups, made by one wave: right for reads after containment, slow
// for a repeat hub.
//
// Included by gact_engine.hip behind every other kernel and behind the engine's definitions (Slot, fail, HIP_TRY), inside its
// extern "C" block, as gact_cover.hpp is.
#pragma once

namespace gact {

constexpr int32_t kGraphMaxRecords = 1 << 28;     // (a proposal index 2 k + 1 and a table of >= 4 n slots fit an int32 / uint32)
constexpr int32_t kGraphMaxReads = 1 << 30;       // (a vertex 2 i + 1 fits an int32)
constexpr int kGraphBadIndex = 1, kGraphBadRead = 2;    // bits of the flag word
// the statistics' counters: by_class[8], then
constexpr int kGraphProposed = 8, kGraphKept = 9, kGraphContained = 10, kGraphCounters = 16;

__device__ inline uint32_t graph_hash(int u, int v)
{
    return hash_final(hash_mix(hash_mix(kHashSeed, (uint32_t)u), (uint32_t)v));
}

// is proposal a (index pa) better than proposal b (index pb) of its key?  pa != pb
__device__ inline bool graph_better(int pa, const gact_graph_arc &a, int pb, const gact_graph_arc &b)
{
    if (a.score != b.score) return a.score > b.score;
    if (a.record != b.record) return a.record < b.record;
    return pa < pb;
}

__global__ void __launch_bounds__(kPassBlock)
graph_class_kernel(const gact_overlap *__restrict__ rec, int n, const int *__restrict__ sel, int n_chosen,
                   const gact_path_summary *__restrict__ sums, int n_reads, const int *__restrict__ lens,
                   const int *__restrict__ clip, gact_graph_params p, gact_graph_read *reads, unsigned *contained_by,
                   uint8_t *__restrict__ classes, gact_graph_arc *__restrict__ props, unsigned long long *counters, int *flag)
{
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    int cls = -1;                                  // (a lane behind the last chosen record)
    if (k < n_chosen) {
        cls = GACT_GRAPH_NONE;
        gact_graph_arc a0, a1;
        a0.u = a1.u = -1;
        a0.v = a0.len = a0.ov_u = a0.ov_v = a0.record = a0.score = a0.flags = 0;
        a1 = a0;
        const int i = sel ? sel[k] : k;
        if (i < 0 || i >= n) atomicOr(flag, kGraphBadIndex);
        else {
            const gact_overlap r = rec[i];
            const int t = r.ref_id, q = r.query_id;
            if (!r.emitted) { }
            else if (t < 0 || t >= n_reads || q < 0 || q >= n_reads) atomicOr(flag, kGraphBadRead);
            else if (t == q) cls = GACT_GRAPH_SELF;
            else {
                const int rev = r.comp != 0;
                long long ab = r.ab, bb = r.bb;
                const long long ae = r.ae, be = r.be;
                if (sums) begins_from_summary(r, sums[k], ab, bb);
                const long long len_t = lens[t], len_q = lens[q];
                long long cbt = 0, cet = len_t, cbq = 0, ceq = len_q;
                if (clip) { cbt = clip[2 * t]; cet = clip[2 * t + 1]; cbq = clip[2 * q]; ceq = clip[2 * q + 1]; }
                if (rev) { const long long b = cbq; cbq = len_q - ceq; ceq = len_q - b; }
                // both reads' ends move together, by what the deeper clip cuts: (ts, qs) and (te, qe) stay points of the alignment
                const long long cut5 = max(max(cbt - ab, cbq - bb), 0LL), cut3 = max(max(ae - cet, be - ceq), 0LL);
                long long ts = ab + cut5, te = ae - cut3, qs = bb + cut5, qe = be - cut3;
                if (te <= ts || qe <= qs) cls = GACT_GRAPH_DROPPED;
                else {
                    ts -= cbt; te -= cbt; qs -= cbq; qe -= cbq;
                    const long long tl = cet - cbt, ql = ceq - cbq;
                    const long long t3 = tl - te, q3 = ql - qe;                    // what is left behind the overlap
                    const long long ext5 = min(qs, ts), ext3 = min(q3, t3), sq = qe - qs, st = te - ts;
                    const long long ov_q = sq + ext5 + ext3, ov_t = st + ext5 + ext3;
                    bool q_in = qs <= ts && q3 <= t3, t_in = qs >= ts && q3 >= t3;
                    if (q_in && t_in) { q_in = ql != tl ? ql < tl : q > t; t_in = !q_in; }
                    if (ext5 > p.max_hang || ext3 > p.max_hang || 1000 * sq < (long long)p.int_permille * ov_q)
                        cls = GACT_GRAPH_INTERNAL;
                    else if (q_in) cls = GACT_GRAPH_QUERY_CONTAINED;
                    else if (t_in) cls = GACT_GRAPH_TARGET_CONTAINED;
                    else if (ov_q < p.min_ovlp || ov_t < p.min_ovlp) cls = GACT_GRAPH_SHORT;
                    else {
                        cls = GACT_GRAPH_DOVETAIL;
                        const int vq = 2 * q + rev, vt = 2 * t;
                        a0.record = a1.record = i;
                        a0.score = a1.score = r.score;
                        if (qs > ts) {
                            a0.u = vq; a0.v = vt; a0.len = (int)(qs - ts); a0.ov_u = (int)ov_q; a0.ov_v = (int)ov_t;
                            a1.u = vt ^ 1; a1.v = vq ^ 1; a1.len = (int)(t3 - q3); a1.ov_u = (int)ov_t; a1.ov_v = (int)ov_q;
                        } else {
                            a0.u = vt; a0.v = vq; a0.len = (int)(ts - qs); a0.ov_u = (int)ov_t; a0.ov_v = (int)ov_q;
                            a1.u = vq ^ 1; a1.v = vt ^ 1; a1.len = (int)(q3 - t3); a1.ov_u = (int)ov_q; a1.ov_v = (int)ov_t;
                        }
                    }
                    atomicAdd(&reads[t].n_hits, 1);
                    atomicAdd(&reads[q].n_hits, 1);
                    if (cls == GACT_GRAPH_INTERNAL) {
                        atomicAdd(&reads[t].n_internal, 1);
                        atomicAdd(&reads[q].n_internal, 1);
                    } else if (cls == GACT_GRAPH_QUERY_CONTAINED) {
                        atomicMin(&contained_by[q], (unsigned)i);
                        atomicAdd(&reads[t].n_contains, 1);
                    } else if (cls == GACT_GRAPH_TARGET_CONTAINED) {
                        atomicMin(&contained_by[t], (unsigned)i);
                        atomicAdd(&reads[q].n_contains, 1);
                    }
                }
            }
        }
        classes[k] = (uint8_t)cls;
        props[2 * (size_t)k] = a0;
        props[2 * (size_t)k + 1] = a1;
    }
    for (int c = 0; c < 8; c++) wave_count(&counters[c], cls == c);
}

__global__ void __launch_bounds__(kPassBlock)
graph_insert_kernel(const gact_graph_arc *__restrict__ props, int n_props, const unsigned *__restrict__ contained_by, int *table,
                    uint32_t mask, unsigned long long *counters)
{
    const int pi = blockIdx.x * kPassBlock + threadIdx.x;
    bool live = false;
    gact_graph_arc a;
    if (pi < n_props) {
        a = props[pi];
        live = a.u >= 0 && contained_by[a.u >> 1] == 0xffffffffu && contained_by[a.v >> 1] == 0xffffffffu;
    }
    wave_count(&counters[kGraphProposed], live);
    if (!live) return;
    table_insert_best(table, mask, graph_hash(a.u, a.v), pi,
                      [&](int j) { return props[j].u == a.u && props[j].v == a.v; },
                      [&](int j) { return graph_better(pi, a, j, props[j]); });
}

__global__ void __launch_bounds__(kPassBlock)
graph_degree_kernel(const gact_graph_arc *__restrict__ props, const int *__restrict__ table, size_t slots, int *deg)
{
    const size_t s = (size_t)blockIdx.x * kPassBlock + threadIdx.x;
    if (s >= slots) return;
    const int j = table[s];
    if (j != kTableEmpty) atomicAdd(&deg[props[j].u], 1);
}

// one block: first[0, nv] = the exclusive scan of deg[0, nv), first[nv] = the number of arcs
__global__ void __launch_bounds__(kPassBlock)
graph_scan_kernel(int nv, const int *__restrict__ deg, int *__restrict__ first)
{
    long long carry = 0;
    for (int base = 0; base < nv; base += kPassBlock) {
        const int k = base + (int)threadIdx.x;
        long long own[1] = {0}, before[1], total[1];
        if (k < nv) own[0] = deg[k];
        block_scan_step(own, before, total);
        if (k < nv) first[k] = (int)(carry + before[0]);
        carry += total[0];
    }
    if (threadIdx.x == 0) first[nv] = (int)carry;
}

__global__ void __launch_bounds__(kPassBlock)
graph_scatter_kernel(const gact_graph_arc *__restrict__ props, const int *__restrict__ table, size_t slots,
                     const int *__restrict__ first, int *fill, int *__restrict__ csr)
{
    const size_t s = (size_t)blockIdx.x * kPassBlock + threadIdx.x;
    if (s >= slots) return;
    const int j = table[s];
    if (j == kTableEmpty) return;
    const int u = props[j].u;
    csr[first[u] + atomicAdd(&fill[u], 1)] = j;
}

__global__ void __launch_bounds__(kPassBlock)
graph_order_kernel(int nv, const gact_graph_arc *__restrict__ props, const int *__restrict__ first, const int *__restrict__ csr,
                   gact_graph_arc *__restrict__ arcs)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (kPassBlock / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (kPassBlock / 64);
    for (int u = wave; u < nv; u += n_waves) {
        const int b = first[u], d = first[u + 1] - b;
        for (int e = lane; e < d; e += 64) {
            const gact_graph_arc a = props[csr[b + e]];
            int rank = 0;
            for (int f = 0; f < d; f++) {
                const gact_graph_arc &o = props[csr[b + f]];
                rank += o.len < a.len || (o.len == a.len && o.v < a.v);
            }
            arcs[b + rank] = a;                    // (flags 0, as the proposal has them)
        }
    }
}

__global__ void __launch_bounds__(kPassBlock)
graph_reduce_kernel(int nv, const gact_graph_arc *__restrict__ props, const int *__restrict__ table, uint32_t mask,
                    const int *__restrict__ first, gact_graph_arc *arcs, int fuzz)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (kPassBlock / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (kPassBlock / 64);
    for (int u = wave; u < nv; u += n_waves) {
        const int b = first[u], d = first[u + 1] - b;
        if (d < 2) continue;
        const long long pairs = (long long)d * d;
        for (long long at = lane; at < pairs; at += 64) {
            const int ix = (int)(at / d), iw = (int)(at % d);
            if (ix == iw) continue;
            const int x = arcs[b + ix].v, w = arcs[b + iw].v;
            const long long len_ux = arcs[b + ix].len, len_uw = arcs[b + iw].len;
            if (len_uw > len_ux + fuzz) continue;              // (every len is >= 1: no w -> x can make up for it)
            const int j = table_find(table, mask, graph_hash(w, x), [&](int h) { return props[h].u == w && props[h].v == x; });
            if (j != kTableEmpty && len_uw + props[j].len <= len_ux + fuzz) atomicOr(&arcs[b + ix].flags, 1);
        }
    }
}

__global__ void __launch_bounds__(kPassBlock)
graph_mirror_kernel(int n_arcs, const int *__restrict__ first, gact_graph_arc *arcs)
{
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    if (k >= n_arcs) return;
    const int from = arcs[k].v ^ 1, to = arcs[k].u ^ 1;
    for (int e = first[from]; e < first[from + 1]; e++)
        if (arcs[e].v == to) {
            if (__hip_atomic_load(&arcs[e].flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1) atomicOr(&arcs[k].flags, 2);
            break;
        }
}

__global__ void __launch_bounds__(kPassBlock)
graph_reads_kernel(int n_reads, const unsigned *__restrict__ contained_by, const int *__restrict__ first,
                   const gact_graph_arc *__restrict__ arcs, gact_graph_read *reads, unsigned long long *counters)
{
    const int i = blockIdx.x * kPassBlock + threadIdx.x;
    int kept_here = 0;
    bool inside = false;
    if (i < n_reads) {
        inside = contained_by[i] != 0xffffffffu;
        reads[i].contained_by = (int)contained_by[i];
        for (int s = 0; s < 2; s++) {
            const int b = first[2 * i + s], e = first[2 * i + s + 1];
            int kept = 0;
            for (int k = b; k < e; k++) kept += arcs[k].flags == 0;
            reads[i].deg[s] = e - b;
            reads[i].kept[s] = kept;
            kept_here += kept;
        }
    }
    for (int o = 32; o > 0; o >>= 1) kept_here += __shfl_xor(kept_here, o);
    if (kept_here && (threadIdx.x & 63) == 0) atomicAdd(&counters[kGraphKept], (unsigned long long)kept_here);
    wave_count(&counters[kGraphContained], inside);
}

}  // namespace gact

// One allocation: records (host ones only) | sel | sums | lens (4 n_reads) | clip (8 n_reads, where given) |
// [ reads (32 n_reads) | deg, fill (4 each per vertex) | counters (128) | flag (16) ], zeroed together |
// first (4 (2 n_reads + 1)) | [ contained_by (4 n_reads) | table (4 slots) ], set to 0xff together |
// classes (1 per chosen record) | proposals (64) | csr (8) | arcs (64).
int gact_hip_overlap_graph(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records, int32_t n_sel, const int32_t *sel,
                           const gact_path_summary *sums, int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                           const gact_graph_params *params, gact_graph_read *reads, uint8_t *classes, gact_graph_arc *arcs,
                           int64_t arcs_cap, int64_t *n_arcs)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (!n_arcs) return fail(GACT_HIP_EINVAL, "overlap_graph: n_arcs is NULL");
    *n_arcs = 0;
    const gact_graph_params p = params ? *params : gact_graph_params{GACT_GRAPH_DEFAULT_MAX_HANG, GACT_GRAPH_DEFAULT_INT_PERMILLE,
                                                                     GACT_GRAPH_DEFAULT_MIN_OVLP, GACT_GRAPH_DEFAULT_FUZZ};
    if (p.max_hang < 0 || p.int_permille < 0 || p.int_permille > 1000 || p.min_ovlp < 0 || p.fuzz < 0)
        return fail(GACT_HIP_EINVAL, "overlap_graph: bad parameter (max_hang = %d, int_permille = %d, min_ovlp = %d, fuzz = %d: all >= 0, "
                    "int_permille at most 1000)", p.max_hang, p.int_permille, p.min_ovlp, p.fuzz);
    if (n < 0 || n > gact::kGraphMaxRecords || n_reads < 0 || n_reads > gact::kGraphMaxReads || (sel && (n_sel < 0 || n_sel > gact::kGraphMaxRecords)) ||
        arcs_cap < 0)
        return fail(GACT_HIP_EINVAL, "overlap_graph: bad arguments (n = %d, at most %d; n_reads = %d, at most %d; n_sel = %d; arcs_cap = %lld)",
                    n, gact::kGraphMaxRecords, n_reads, gact::kGraphMaxReads, n_sel, (long long)arcs_cap);
    if (n_reads > 0 && (!read_lens || !reads)) return fail(GACT_HIP_EINVAL, "overlap_graph: read_lens or reads is NULL");
    if (check_read_lens("overlap_graph", n_reads, read_lens, clip) < 0) return GACT_HIP_EINVAL;
    Slot &sl = e->slots[slot];
    if ((rc = slot_records_check(sl, slot, n, records, "overlap_graph"))) return rc;
    if (n_reads == 0) return 0;
    const int32_t n_chosen = n == 0 ? 0 : sel ? n_sel : n;
    if ((rc = set_device(e))) return rc;
    PassScratch<gact_graph_stats> &gb = sl.graph;
    const size_t nv = 2 * (size_t)n_reads, n_props = 2 * (size_t)n_chosen;
    size_t slots = 2;
    while (slots < 2 * n_props) slots <<= 1;
    const size_t at_sel = records ? up16((size_t)n * sizeof(gact_overlap)) : 0;
    const size_t at_sums = up16(at_sel + (sel ? (size_t)n_chosen * sizeof(int32_t) : 0));
    const size_t at_lens = up16(at_sums + (sums ? (size_t)n_chosen * sizeof(gact_path_summary) : 0));
    const size_t at_clip = up16(at_lens + (size_t)n_reads * sizeof(int32_t));
    const size_t at_reads = up16(at_clip + (clip ? nv * sizeof(int32_t) : 0));
    const size_t at_deg = at_reads + (size_t)n_reads * sizeof(gact_graph_read);
    const size_t at_fill = at_deg + nv * sizeof(int);
    const size_t at_counters = up16(at_fill + nv * sizeof(int));
    const size_t at_flag = at_counters + gact::kGraphCounters * sizeof(unsigned long long);
    const size_t at_first = at_flag + 16;
    const size_t at_cby = up16(at_first + (nv + 1) * sizeof(int));
    const size_t at_table = at_cby + (size_t)n_reads * sizeof(unsigned);
    const size_t at_classes = up16(at_table + slots * sizeof(int));
    const size_t at_props = up16(at_classes + (size_t)n_chosen);
    const size_t at_csr = at_props + n_props * sizeof(gact_graph_arc);
    const size_t at_arcs = up16(at_csr + n_props * sizeof(int));
    const size_t bytes = at_arcs + n_props * sizeof(gact_graph_arc);
    if (gb.reserve(bytes))
        return fail(GACT_HIP_ENOMEM, "overlap_graph: device allocation failed (%d reads, %d records, %zu bytes)", n_reads, n_chosen, bytes);
    int *d_lens = (int *)(gb.p + at_lens);
    const int *d_clip = clip ? (const int *)(gb.p + at_clip) : nullptr;
    gact_graph_read *d_reads = (gact_graph_read *)(gb.p + at_reads);
    int *d_deg = (int *)(gb.p + at_deg), *d_fill = (int *)(gb.p + at_fill), *d_flag = (int *)(gb.p + at_flag);
    unsigned long long *d_counters = (unsigned long long *)(gb.p + at_counters);
    int *d_first = (int *)(gb.p + at_first), *d_table = (int *)(gb.p + at_table), *d_csr = (int *)(gb.p + at_csr);
    unsigned *d_cby = (unsigned *)(gb.p + at_cby);
    uint8_t *d_classes = gb.p + at_classes;
    gact_graph_arc *d_props = (gact_graph_arc *)(gb.p + at_props), *d_arcs = (gact_graph_arc *)(gb.p + at_arcs);
    if ((rc = gb.begin(sl.stream, "overlap_graph"))) return rc;
    DevRecords in;
    if ((rc = slot_records_stage(sl, gb.p, n, records, n_chosen, sel, at_sel, sums, at_sums, in))) return rc;
    const gact_overlap *d_rec = in.rec;
    const int *d_sel = in.sel;
    const gact_path_summary *d_sums = in.sums;
    HIP_TRY(hipMemcpyAsync(d_lens, read_lens, (size_t)n_reads * sizeof(int32_t), hipMemcpyHostToDevice, sl.stream));
    if (clip) HIP_TRY(hipMemcpyAsync(gb.p + at_clip, clip, nv * sizeof(int32_t), hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemsetAsync(d_reads, 0, at_first - at_reads, sl.stream));
    HIP_TRY(hipMemsetAsync(d_cby, 0xff, at_table + slots * sizeof(int) - at_cby, sl.stream));        // no container, kTableEmpty everywhere
    const dim3 block(gact::kPassBlock);
    const dim3 wave_grid = wave_blocks(e, nv);
    const uint32_t mask = (uint32_t)(slots - 1);
    if (n_chosen > 0) {
        hipLaunchKernelGGL(gact::graph_class_kernel, lane_blocks((size_t)n_chosen), block, 0, sl.stream, d_rec, n, d_sel, n_chosen, d_sums,
                           n_reads, d_lens, d_clip, p, d_reads, d_cby, d_classes, d_props, d_counters, d_flag);
        hipLaunchKernelGGL(gact::graph_insert_kernel, lane_blocks(n_props), block, 0, sl.stream, d_props, (int)n_props, d_cby, d_table, mask,
                           d_counters);
        hipLaunchKernelGGL(gact::graph_degree_kernel, lane_blocks(slots), block, 0, sl.stream, d_props, d_table, slots, d_deg);
    }
    hipLaunchKernelGGL(gact::graph_scan_kernel, dim3(1), block, 0, sl.stream, (int)nv, d_deg, d_first);
    if (n_chosen > 0) {
        hipLaunchKernelGGL(gact::graph_scatter_kernel, lane_blocks(slots), block, 0, sl.stream, d_props, d_table, slots, d_first, d_fill, d_csr);
        hipLaunchKernelGGL(gact::graph_order_kernel, wave_grid, block, 0, sl.stream, (int)nv, d_props, d_first, d_csr, d_arcs);
        hipLaunchKernelGGL(gact::graph_reduce_kernel, wave_grid, block, 0, sl.stream, (int)nv, d_props, d_table, mask, d_first, d_arcs,
                           p.fuzz);
    }
    HIP_TRY(hipGetLastError());
    // the number of arcs sizes the mirror kernel's grid: the one value the host waits for in the middle
    int flag = 0, total = 0;
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipMemcpyAsync(&total, d_first + nv, sizeof total, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
    if (flag & gact::kGraphBadIndex)
        return fail(GACT_HIP_EINVAL, "overlap_graph: sel holds an index outside [0, %d)", n);
    if (flag)
        return fail(GACT_HIP_ERANGE, "overlap_graph: a counted record names a read outside [0, %d)", n_reads);
    if (total < 0 || (size_t)total > n_props)
        return fail(GACT_HIP_EDEVICE, "overlap_graph: the device counted %d arcs of %zu proposals", total, n_props);
    if (total > 0)
        hipLaunchKernelGGL(gact::graph_mirror_kernel, lane_blocks((size_t)total), block, 0, sl.stream, total, d_first, d_arcs);
    hipLaunchKernelGGL(gact::graph_reads_kernel, lane_blocks((size_t)n_reads), block, 0, sl.stream, n_reads, d_cby, d_first, d_arcs, d_reads,
                       d_counters);
    HIP_TRY(hipGetLastError());
    unsigned long long counters[gact::kGraphCounters];
    HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipMemcpyAsync(reads, d_reads, (size_t)n_reads * sizeof(gact_graph_read), hipMemcpyDeviceToHost, sl.stream));
    if (classes && n_chosen > 0) HIP_TRY(hipMemcpyAsync(classes, d_classes, (size_t)n_chosen, hipMemcpyDeviceToHost, sl.stream));
    *n_arcs = total;
    const bool room = total == 0 || (arcs && arcs_cap >= total);
    if (room && total > 0)
        HIP_TRY(hipMemcpyAsync(arcs, d_arcs, (size_t)total * sizeof(gact_graph_arc), hipMemcpyDeviceToHost, sl.stream));
    if ((rc = gb.end(sl.stream))) return rc;
    gb.stats.reads = n_reads;
    gb.stats.contained = (int32_t)counters[gact::kGraphContained];
    for (int c = 0; c < 8; c++) gb.stats.by_class[c] = (int64_t)counters[c];
    gb.stats.proposed = (int64_t)counters[gact::kGraphProposed];
    gb.stats.arcs = total;
    gb.stats.kept = (int64_t)counters[gact::kGraphKept];
    gb.stats.transitive = total - gb.stats.kept;
    gb.stats.table_slots = (int64_t)slots;
    gb.stats.scratch_bytes = (int64_t)gb.bytes;
    if (!room)
        return fail(GACT_HIP_EINVAL, "overlap_graph: %d arcs, room for %lld: call again with room for *n_arcs", total,
                    arcs ? (long long)arcs_cap : 0ll);
    return 0;
}

int gact_hip_last_graph_stats(gact_hip_engine *e, int slot, gact_graph_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::graph, stats, "last_graph_stats", "has made no overlap graph yet");
}
