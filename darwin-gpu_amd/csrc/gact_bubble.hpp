// gact_bubble.hpp -- the bubbles of an overlap graph, found and popped on the device (gact_hip_pop_bubbles).
//
// What an assembler's layout stage does between its two rounds of tip cutting: where two or more paths leave one vertex and
// meet again a few reads later, keep one and remove the rest.  The rule is stated in include/gact_hip.h and restated in
// tests/bubble_model.py.  The new ground is the search itself: a topological walk over at most 64 vertices, made by ONE WAVE
// with ONE SEEN VERTEX PER LANE.
//
// The search.  Lane j holds the record of the j-th vertex seen -- vertex, in-arcs not yet crossed, least distance, arc count,
// length and last arc of the best path -- in registers of its own (plain scalars: an array indexed by the vertex's number would
// live in scratch).  "Is w seen, and where" is one __ballot(vertex == w); an update runs in the owning lane under a predicate;
// what the wave needs of a lane's record comes through v_readlane, so it is wave-uniform and every branch of the search is
// taken by the whole wave.  The stack is 64 slots, slot i in lane i, and holds lane numbers: a push writes lane sp, a pop reads
// lane sp - 1.  The arcs of the popped vertex are crossed one after the other, in array order, so the first failure is the
// model's.  A vertex is popped once, so a search ends after at most 64 pops.
//
// The kernels, all on the slot's stream, nothing on the host between them.  The first two are arc_graph_index (gact_unitig.hpp),
// the others bubble_step below, which the cleaning rounds (gact_clean.hpp) call as well, on arcs that are already resident:
//   unitig_first_kernel, unitig_check_kernel   gact_unitig.hpp's own, with want_bases = 0: the stretches and the arc checks.
//                          EVERY LATER KERNEL RETURNS AT ONCE WHEN THE FLAG WORD IS SET
//   unitig_recount_kernel  gact_unitig.hpp's own, with skip widened to int as its cut: out over W
//   bubble_find_kernel     one wave per source, grid-stride over the 2 n_reads vertices (a vertex with out < 2 costs one load):
//                          the search; on success each lane claims atomicMin(&owner[read], s) for its interior vertex, found[s] = 1
//   bubble_scan_kernel     one block, in place (block_scan_step): found[] becomes the bubbles' numbers, ascending by source
//   bubble_pop_kernel      the same search again -- it is deterministic, so no vertex list is kept in memory between the two --
//                          then the kept path (a walk back along pred, one ballot a step), ownership with one ballot, the
//                          gact_bubble; for a popped one read_bubble and gone[] of the removed reads, and the arcs of rule 5 (b):
//                          the stretch of every path vertex, each arc looked up with one ballot, its complement by the walk
//                          unitig_check_kernel uses
//   bubble_flag_kernel     one lane per arc: the bit for a W arc that touches a removed read, OR the bits of rule 5 (b), OR flags
// Ordinary vector global atomics on integers (atomicMin, atomicOr, atomicAdd); every value they leave is the same in whichever
// order they land.  No LDS but the scan's, no spinning on other waves, no cooperative grid, no inline assembly.
//
// Included by gact_engine.hip behind gact_unitig.hpp, inside its extern "C" block.
#pragma once

namespace gact {

// how a search ends: the failures in the order of gact_bubble_stats.by_fail, then success
constexpr int kBubbleOpen = 0, kBubbleDead = 1, kBubbleTwice = 2, kBubbleDist = 3, kBubbleMany = 4, kBubbleFound = 5;
// the counters (0 and 1 are unitig_check_kernel's kUnitigE0 and unitig_recount_kernel's kUnitigE1: the arcs of W)
constexpr int kBubbleW = kUnitigE1, kBubbleSources = 2, kBubbleFoundN = 3, kBubblePopped = 4, kBubbleReadsRemoved = 5,
              kBubbleArcsRemoved = 6, kBubbleFail = 7, kBubbleCounters = 12;
static_assert(GACT_BUBBLE_MAX_VERTICES == 64, "one seen vertex per lane of a wave64");

// this lane's seen vertex (vert < 0: none yet)
struct BubbleLane {
    int vert, r, d, c, pred;
    long long pd;
};

// lane j's value, wave-uniform (j is)
__device__ __forceinline__ int lane_get(int x, int j) { return __builtin_amdgcn_readlane(x, j); }
__device__ __forceinline__ long long lane_get64(long long x, int j)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, j);
    const int hi = __builtin_amdgcn_readlane((int)(x >> 32), j);
    return ((long long)hi << 32) | lo;
}

// The search from s, by a whole wave.  -> how it ended; on kBubbleFound lanes [0, n_seen) hold the seen vertices, lane 0 the
// source and lane jt the sink.  out: the out-degrees over W; skip: NULL, or the reads whose arcs are not of W
__device__ __forceinline__ int bubble_search(int s, int lane, const gact_graph_arc *__restrict__ arcs, const int *__restrict__ first,
                                             const int *__restrict__ skip, const int *__restrict__ out, int max_dist, int max_vertices,
                                             BubbleLane &me, int &n_seen, int &jt)
{
    me.vert = lane == 0 ? s : -1;
    me.r = 0; me.d = 0; me.c = 0; me.pred = -1; me.pd = 0;
    int stk = 0;                                              // slot `lane` of the stack: a lane number (slot 0: the source's)
    int sp = 1, pending = 0;
    n_seen = 1;
    for (;;) {
        sp--;
        const int jv = lane_get(stk, sp);
        const int v = lane_get(me.vert, jv);
        if (out[v] == 0) return kBubbleDead;
        const int dv = lane_get(me.d, jv), cv = lane_get(me.c, jv);
        const long long pdv = lane_get64(me.pd, jv);
        const int end = first[v + 1];
        for (int k = first[v]; k < end; k++) {
            const gact_graph_arc a = arcs[k];
            if (!unitig_in_set(a, skip)) continue;
            const int w = a.v;
            const unsigned long long at_w = __ballot(me.vert == w), at_wc = __ballot(me.vert == (w ^ 1));
            if (w == s || at_wc) return kBubbleTwice;         // (w == s^1: s is seen)
            const unsigned dw = (unsigned)dv + (unsigned)a.len;   // (at most 2^30 + 2^31)
            if (dw > (unsigned)max_dist) return kBubbleDist;
            const long long pdw = pdv + a.len;
            int jw;
            if (!at_w) {
                if (n_seen >= max_vertices) return kBubbleMany;
                jw = n_seen++;
                if (lane == jw) { me.vert = w; me.r = out[w ^ 1]; me.d = (int)dw; me.c = cv + 1; me.pd = pdw; me.pred = k; }
                pending++;
            } else {
                jw = __ffsll(at_w) - 1;
                if (lane == jw) {
                    me.d = min(me.d, (int)dw);
                    if (cv + 1 > me.c || (cv + 1 == me.c && (pdw < me.pd || (pdw == me.pd && k < me.pred)))) {
                        me.c = cv + 1; me.pd = pdw; me.pred = k;
                    }
                }
            }
            if (lane == jw) me.r--;
            if (lane_get(me.r, jw) == 0) {
                if (lane == sp) stk = jw;
                sp++;
                pending--;
            }
        }
        if (sp == 1 && pending == 0) { jt = lane_get(stk, 0); return kBubbleFound; }
        if (sp == 0) return kBubbleOpen;
    }
}

// the lanes of the kept path, those of s and t among them: the walk back from t along pred
__device__ __forceinline__ unsigned long long bubble_path(const BubbleLane &me, int jt, const gact_graph_arc *__restrict__ arcs)
{
    unsigned long long on = 1ull | (1ull << jt);
    int cur = jt;
    for (int step = 0; step < 64 && cur != 0; step++) {
        const unsigned long long at_u = __ballot(me.vert == arcs[lane_get(me.pred, cur)].u);
        if (!at_u) break;                                     // (cannot be: pred leaves a seen vertex)
        cur = __ffsll(at_u) - 1;
        on |= 1ull << cur;
    }
    return on;
}

__global__ void __launch_bounds__(kPassBlock)
bubble_find_kernel(int nv, const gact_graph_arc *__restrict__ arcs, const int *__restrict__ first, const int *__restrict__ skip,
                   const int *__restrict__ out, int max_dist, int max_vertices, int *owner, int *__restrict__ found,
                   unsigned long long *counters, const int *__restrict__ flag)
{
    if (*flag) return;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kPassWaves + (threadIdx.x >> 6), n_waves = gridDim.x * kPassWaves;
    for (long long x = wave; x < nv; x += n_waves) {
        const int s = (int)x;
        if (out[s] < 2) continue;
        BubbleLane me;
        int n_seen, jt = 0;
        const int how = bubble_search(s, lane, arcs, first, skip, out, max_dist, max_vertices, me, n_seen, jt);
        wave_count(&counters[kBubbleSources], lane == 0);
        wave_count(&counters[how == kBubbleFound ? kBubbleFoundN : kBubbleFail + how], lane == 0);
        if (how != kBubbleFound) continue;
        if (lane > 0 && lane < n_seen && lane != jt) atomicMin(&owner[me.vert >> 1], s);
        if (lane == 0) found[s] = 1;
    }
}

// one block, in place: found[] becomes its exclusive scan over the vertex ids, *n_found its total
__global__ void __launch_bounds__(kPassBlock)
bubble_scan_kernel(int nv, int *__restrict__ found, long long *n_found, const int *__restrict__ flag)
{
    if (*flag) return;
    long long carry[1] = {0};
    for (int base = 0; base < nv; base += kPassBlock) {
        const int x = base + (int)threadIdx.x;
        long long own[1] = {0}, before[1], total[1];
        if (x < nv) own[0] = found[x];
        block_scan_step(own, before, total);
        if (x < nv) found[x] = (int)(carry[0] + before[0]);
        carry[0] += total[0];
    }
    if (threadIdx.x == 0) *n_found = carry[0];
}

// number: found[] behind the scan.  A source whose search succeeded in bubble_find_kernel succeeds here, with the same records
__global__ void __launch_bounds__(kPassBlock)
bubble_pop_kernel(int nv, const gact_graph_arc *__restrict__ arcs, const int *__restrict__ first, const int *__restrict__ skip,
                  const int *__restrict__ out, int max_dist, int max_vertices, const int *__restrict__ owner,
                  const int *__restrict__ number, gact_bubble *__restrict__ bubbles, int *__restrict__ read_bubble,
                  int *__restrict__ gone, int *bits, unsigned long long *counters, const int *__restrict__ flag)
{
    if (*flag) return;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kPassWaves + (threadIdx.x >> 6), n_waves = gridDim.x * kPassWaves;
    for (long long x = wave; x < nv; x += n_waves) {
        const int s = (int)x;
        if (out[s] < 2) continue;
        BubbleLane me;
        int n_seen, jt = 0;
        if (bubble_search(s, lane, arcs, first, skip, out, max_dist, max_vertices, me, n_seen, jt) != kBubbleFound) continue;
        const unsigned long long on = bubble_path(me, jt, arcs);
        const bool interior = lane > 0 && lane < n_seen && lane != jt;
        const bool popped = __ballot(interior && owner[me.vert >> 1] != s) == 0;
        const int id = number[s], n_path = __popcll(on) - 2;
        if (lane == 0) {
            gact_bubble b;
            b.source = s; b.sink = lane_get(me.vert, jt); b.n_vertices = n_seen; b.n_path = n_path; b.n_removed = n_seen - 2 - n_path;
            b.state = popped ? GACT_BUBBLE_POPPED : GACT_BUBBLE_LOST;
            b.path_len = lane_get64(me.pd, jt);
            bubbles[id] = b;
        }
        wave_count(&counters[kBubblePopped], lane == 0 && popped);
        if (!popped) continue;
        // (a) the interior reads that are not on the kept path; their arcs get the bit in bubble_flag_kernel
        const bool removed = interior && !((on >> lane) & 1);
        if (removed) { read_bubble[me.vert >> 1] = id; gone[me.vert >> 1] = 1; }
        wave_count(&counters[kBubbleReadsRemoved], removed);
        // (b) the arcs from a path vertex but t to a path vertex that are not the path's, and their complements
        for (unsigned long long todo = on & ~(1ull << jt); todo; todo &= todo - 1) {
            const int px = lane_get(me.vert, __ffsll(todo) - 1);
            const int end = first[px + 1];
            for (int k = first[px]; k < end; k++) {
                const gact_graph_arc a = arcs[k];
                if (!unitig_in_set(a, skip)) continue;
                const unsigned long long at_y = __ballot(me.vert == a.v) & on;
                if (!at_y || lane_get(me.pred, __ffsll(at_y) - 1) == k) continue;
                if (lane == 0) {
                    atomicOr(&bits[k], GACT_GRAPH_ARC_BUBBLE);
                    const int from = a.v ^ 1, to = px ^ 1;
                    for (int e = first[from]; e < first[from + 1]; e++)
                        if (arcs[e].v == to && arcs[e].flags == 0) { atomicOr(&bits[e], GACT_GRAPH_ARC_BUBBLE); break; }
                }
            }
        }
    }
}

// bits: in, the bits of rule 5 (b); out, arc_flags
__global__ void __launch_bounds__(kPassBlock)
bubble_flag_kernel(const gact_graph_arc *__restrict__ arcs, int n_arcs, const int *__restrict__ skip, const int *__restrict__ gone,
                   int *__restrict__ bits, unsigned long long *counters, const int *__restrict__ flag)
{
    if (*flag) return;
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    bool removed = false;
    if (k < n_arcs) {
        const gact_graph_arc a = arcs[k];
        int b = bits[k];
        if (unitig_in_set(a, skip) && (gone[a.u >> 1] || gone[a.v >> 1])) b = GACT_GRAPH_ARC_BUBBLE;
        removed = b != 0;
        bits[k] = a.flags | b;
    }
    wave_count(&counters[kBubbleArcsRemoved], removed);
}

}  // namespace gact

// The bubble step on an indexed graph (ArcGraphDev, gact_unitig.hpp), as the bubble call and the rounds of gact_clean.hpp
// make it: W is the arcs with flags == 0 that touch no read of g.skip.  out, found, gone, bits, *n_found and the counters are
// the caller's to have zeroed; owner and read_bubble are set here.  bits leaves as arc_flags
static int bubble_step(const gact_hip_engine *e, const ArcGraphDev &g, int *out, const gact_bubble_params &p, int *owner, int *found,
                       long long *n_found, gact_bubble *bubbles, int *read_bubble, int *gone, int *bits, unsigned long long *counters)
{
    const dim3 block(gact::kPassBlock);
    const size_t n = (size_t)g.n_reads, nv = (size_t)g.nv, na = (size_t)g.n_arcs;
    HIP_TRY(hipMemsetAsync(owner, 0x7f, n * sizeof(int), g.stream));
    HIP_TRY(hipMemsetAsync(read_bubble, 0xff, n * sizeof(int), g.stream));
    hipLaunchKernelGGL(gact::unitig_recount_kernel, lane_blocks(na), block, 0, g.stream, g.arcs, g.n_arcs, g.skip, out, counters, g.flag);
    hipLaunchKernelGGL(gact::bubble_find_kernel, wave_blocks(e, nv), block, 0, g.stream, g.nv, g.arcs, g.first, g.skip, out, p.max_dist,
                       p.max_vertices, owner, found, counters, g.flag);
    hipLaunchKernelGGL(gact::bubble_scan_kernel, dim3(1), block, 0, g.stream, g.nv, found, n_found, g.flag);
    hipLaunchKernelGGL(gact::bubble_pop_kernel, wave_blocks(e, nv), block, 0, g.stream, g.nv, g.arcs, g.first, g.skip, out, p.max_dist,
                       p.max_vertices, owner, found, bubbles, read_bubble, gone, bits, counters, g.flag);
    hipLaunchKernelGGL(gact::bubble_flag_kernel, lane_blocks(na), block, 0, g.stream, g.arcs, g.n_arcs, g.skip, gone, bits, counters, g.flag);
    return 0;
}

// One allocation: the graph (ArcGraphDev) | [ out of E0, out of W, found (4 each per vertex) | gone (4 n_reads) | bits (4 n_arcs)
// | counters (96) | n_found (16) | flag (16) ], zeroed together | first (4 (2 n_reads + 1)) | owner (4 n_reads, set to 0x7f) |
// read_bubble (4 n_reads, set to 0xff) | bubbles (32 per vertex: every source may find one).
int gact_hip_pop_bubbles(gact_hip_engine *e, int slot, int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                         const gact_graph_read *reads, int64_t n_arcs, const gact_graph_arc *arcs, const uint8_t *skip,
                         const gact_bubble_params *params, gact_bubble *bubbles, int64_t bubbles_cap, int64_t *n_bubbles,
                         int32_t *read_bubble, int32_t *arc_flags)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (!read_lens || !reads || !n_bubbles || !read_bubble || !arc_flags)
        return fail(GACT_HIP_EINVAL, "pop_bubbles: NULL argument (read_lens, reads, n_bubbles, read_bubble and arc_flags are needed)");
    const gact_bubble_params p = params ? *params : gact_bubble_params{GACT_BUBBLE_DEFAULT_MAX_DIST, GACT_BUBBLE_MAX_VERTICES};
    if (p.max_dist < 1 || p.max_dist > (1 << 30) || p.max_vertices < 3 || p.max_vertices > GACT_BUBBLE_MAX_VERTICES)
        return fail(GACT_HIP_EINVAL, "pop_bubbles: bad parameter (max_dist = %d: 1 .. 2^30; max_vertices = %d: 3 .. %d)", p.max_dist,
                    p.max_vertices, GACT_BUBBLE_MAX_VERTICES);
    if (check_arc_graph("pop_bubbles", n_reads, read_lens, clip, n_arcs, arcs, "bubbles_cap", bubbles_cap, bubbles_cap < 0) < 0)
        return GACT_HIP_EINVAL;
    if (n_reads == 0) {
        *n_bubbles = 0;
        return 0;
    }
    if ((rc = set_device(e))) return rc;
    Slot &sl = e->slots[slot];
    PassScratch<gact_bubble_stats> &bb = sl.bubble;
    ArcGraphDev g = arc_graph_layout(n_reads, clip, n_arcs, skip);
    const size_t n = (size_t)n_reads, nv = 2 * n, na = (size_t)n_arcs;
    const size_t at_out0 = g.end;
    const size_t at_out1 = at_out0 + nv * sizeof(int);
    const size_t at_found = at_out1 + nv * sizeof(int);
    const size_t at_gone = at_found + nv * sizeof(int);
    const size_t at_bits = at_gone + n * sizeof(int);
    const size_t at_counters = up16(at_bits + na * sizeof(int));
    const size_t at_n_found = at_counters + gact::kBubbleCounters * sizeof(unsigned long long);
    const size_t at_flag = at_n_found + 16;
    const size_t at_first = at_flag + 16;
    const size_t at_owner = up16(at_first + (nv + 1) * sizeof(int));
    const size_t at_read_bubble = at_owner + n * sizeof(int);
    const size_t at_bubbles = up16(at_read_bubble + n * sizeof(int));
    const size_t bytes = at_bubbles + nv * sizeof(gact_bubble);
    if ((rc = arc_graph_begin(g, bb, bytes, sl.stream, "pop_bubbles", read_lens, clip, reads, arcs))) return rc;
    int *d_out0 = (int *)(bb.p + at_out0), *d_out1 = (int *)(bb.p + at_out1), *d_found = (int *)(bb.p + at_found);
    int *d_gone = (int *)(bb.p + at_gone), *d_bits = (int *)(bb.p + at_bits), *d_flag = (int *)(bb.p + at_flag);
    unsigned long long *d_counters = (unsigned long long *)(bb.p + at_counters);
    long long *d_n_found = (long long *)(bb.p + at_n_found);
    int *d_first = (int *)(bb.p + at_first), *d_owner = (int *)(bb.p + at_owner), *d_read_bubble = (int *)(bb.p + at_read_bubble);
    gact_bubble *d_bubbles = (gact_bubble *)(bb.p + at_bubbles);
    HIP_TRY(hipMemsetAsync(d_out0, 0, at_first - at_out0, sl.stream));
    arc_graph_index(g, 0, d_first, d_out0, d_counters, d_flag);
    if ((rc = bubble_step(e, g, d_out1, p, d_owner, d_found, d_n_found, d_bubbles, d_read_bubble, d_gone, d_bits, d_counters))) return rc;
    // the one wait: the flag word and the number of bubbles, before the copies out
    long long n_found = 0;
    unsigned long long counters[gact::kBubbleCounters];
    HIP_TRY(hipMemcpyAsync(&n_found, d_n_found, sizeof n_found, hipMemcpyDeviceToHost, sl.stream));
    if ((rc = arc_graph_fetch(g, "pop_bubbles", d_counters, counters, gact::kBubbleCounters))) return rc;
    if (n_found < 0 || n_found > (long long)nv || n_found != (long long)counters[gact::kBubbleFoundN])
        return fail(GACT_HIP_EDEVICE, "pop_bubbles: the device numbered %lld bubbles and counted %llu", n_found, counters[gact::kBubbleFoundN]);
    const bool room = bubbles && bubbles_cap >= n_found;
    if (room && n_found)
        HIP_TRY(hipMemcpyAsync(bubbles, d_bubbles, (size_t)n_found * sizeof(gact_bubble), hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipMemcpyAsync(read_bubble, d_read_bubble, n * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
    if (na) HIP_TRY(hipMemcpyAsync(arc_flags, d_bits, na * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
    *n_bubbles = n_found;
    if ((rc = bb.end(sl.stream))) return rc;
    gact_bubble_stats &st = bb.stats;
    st.reads = n_reads;
    st.sources = (int32_t)counters[gact::kBubbleSources];
    st.found = (int32_t)n_found;
    st.popped = (int32_t)counters[gact::kBubblePopped];
    st.lost = st.found - st.popped;
    st.reads_removed = (int32_t)counters[gact::kBubbleReadsRemoved];
    st.working_arcs = (int64_t)counters[gact::kBubbleW];
    st.arcs_removed = (int64_t)counters[gact::kBubbleArcsRemoved];
    for (int i = 0; i < 5; i++) st.by_fail[i] = (int64_t)counters[gact::kBubbleFail + i];
    st.scratch_bytes = (int64_t)bb.bytes;
    if (!room)
        return fail(GACT_HIP_EINVAL, "pop_bubbles: %lld bubbles, room for %lld: call again with room for *n_bubbles", n_found,
                    bubbles ? (long long)bubbles_cap : 0ll);
    return 0;
}

int gact_hip_last_bubble_stats(gact_hip_engine *e, int slot, gact_bubble_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::bubble, stats, "last_bubble_stats", "has popped no bubbles yet");
}
