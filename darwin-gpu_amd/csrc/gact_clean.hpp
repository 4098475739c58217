// gact_clean.hpp -- the weak arcs of an overlap graph (gact_hip_prune_overlaps) and the cleaning rounds around the three steps --
// tips, bubbles, weak arcs -- with the arcs resident on the device (gact_hip_clean_graph).
//
// What an assembler's layout stage does about repeats: at every vertex the arcs whose overlap is much shorter than the vertex's
// best one are dropped, at a rising ratio, and tips and bubbles are cleaned again after each drop.  The rules are stated in
// include/gact_hip.h and restated in tests/clean_model.py.
//
// The prune kernels, all on the slot's stream, nothing on the host between them:
//   unitig_first_kernel, unitig_check_kernel   gact_unitig.hpp's own, with want_bases = 0, as the bubble call uses them.
//                          EVERY LATER KERNEL RETURNS AT ONCE WHEN THE FLAG WORD IS SET
//   prune_mark_kernel      one wave per vertex, grid-stride; the lanes stride over the vertex's stretch [first[x], first[x+1]) in
//                          steps of 64.  Sweep one: the wave maximum of ov_u over the lanes in W, and their count.  Sweep two: the
//                          weak bit of each of the vertex's own arcs, a plain store: an arc belongs to one stretch
//   prune_mirror_kernel    one lane per arc: a weak arc sets the removed bit of itself and, by the walk through v^1's stretch
//                          that unitig_check_kernel makes, of its complement (atomicOr: both may be weak)
//   prune_count_kernel     one lane per vertex: its W arcs before and after, bared, the removed ones, and bits[] becomes arc_flags
// prune_step launches the three; the stretches and the checks are arc_graph_index (gact_unitig.hpp).  The loop calls, on one
// upload and one index of the arcs, the stand-alone calls' own step functions -- unitig_sweep and the tip rule, bubble_step,
// prune_step -- each on the flags the steps in front left, and behind each one of its own kernels:
//   clean_init_kernel      one lane per read: its first state
//   clean_tip_kernel       one lane per arc, vertex and read: GACT_GRAPH_ARC_TIP into the flags of an arc that touches a cut read
//                          (its own arc: a plain store), the heads of the tip rule's chains, the state of a read cut for the
//                          first time
//   clean_apply_kernel     one lane per arc and read: a step's flags into arcs[].flags, the state of a read a bubble removed
//   clean_flags_kernel     one lane per arc: the flags words, gathered for the copy out
// Behind every step the host reads the step's counters and the flag word (132 bytes, one wait) and decides whether to go on.
// Ordinary vector global atomics on integers; every value they leave is the same in whichever order they land.  No LDS but the
// scan's, no spinning on other waves, no cooperative grid, no inline assembly.
//
// Included by gact_engine.hip behind gact_bubble.hpp, inside its extern "C" block.
#pragma once

namespace gact {

// the counters of a prune step (0 is unitig_check_kernel's kUnitigE0)
constexpr int kPruneW = 1, kPruneExamined = 2, kPruneWeak = 3, kPruneRemoved = 4, kPruneBared = 5;
// ... and of the loop's own kernels; a step's block holds the unitig counters, the bubble counters or the prune counters below them
constexpr int kCleanArcs = 12, kCleanHeads = 13, kCleanReads = 14, kCleanCounters = 16;
static_assert(kCleanArcs >= kBubbleCounters && kCleanArcs >= kUnitigCounters, "the loop's counters lie behind a step's own");
// bits[] between the prune kernels
constexpr int kPruneWeakBit = 1, kPruneRemovedBit = 2;

__device__ __forceinline__ int wave_sum(int x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__global__ void __launch_bounds__(kPassBlock)
prune_mark_kernel(int nv, const gact_graph_arc *__restrict__ arcs, const int *__restrict__ first, const int *__restrict__ skip,
                  int ratio, int *__restrict__ bits, int *__restrict__ best, unsigned long long *counters,
                  const int *__restrict__ flag)
{
    if (*flag) return;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kPassWaves + (threadIdx.x >> 6), n_waves = gridDim.x * kPassWaves;
    for (long long x = wave; x < nv; x += n_waves) {
        const int begin = first[x], end = first[x + 1];
        int top = INT_MIN, n = 0;
        for (int k = begin + lane; k < end; k += 64) {
            const gact_graph_arc a = arcs[k];
            if (unitig_in_set(a, skip)) { top = max(top, a.ov_u); n++; }
        }
        for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o));
        n = wave_sum(n);
        const bool examined = n >= 2;
        if (lane == 0) {
            if (best) best[x] = examined ? top : 0;
            if (n) atomicAdd(&counters[kPruneW], (unsigned long long)n);
            if (examined) atomicAdd(&counters[kPruneExamined], 1ull);
        }
        if (!examined) continue;
        const long long bound = (long long)ratio * top;
        int weak = 0;
        for (int k = begin + lane; k < end; k += 64) {
            const gact_graph_arc a = arcs[k];
            if (unitig_in_set(a, skip) && 1000ll * a.ov_u < bound) { bits[k] = kPruneWeakBit; weak++; }
        }
        weak = wave_sum(weak);
        if (lane == 0 && weak) atomicAdd(&counters[kPruneWeak], (unsigned long long)weak);
    }
}

__global__ void __launch_bounds__(kPassBlock)
prune_mirror_kernel(const gact_graph_arc *__restrict__ arcs, int n_arcs, const int *__restrict__ first, int *bits,
                    const int *__restrict__ flag)
{
    if (*flag) return;
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    if (k >= n_arcs || !(bits[k] & kPruneWeakBit)) return;
    const gact_graph_arc a = arcs[k];
    atomicOr(&bits[k], kPruneRemovedBit);
    // (the complement of a W arc joins the same two reads: it is of W iff its flags are 0, and the check kernel found one)
    const int from = a.v ^ 1, to = a.u ^ 1;
    for (int e = first[from]; e < first[from + 1]; e++)
        if (arcs[e].v == to && arcs[e].flags == 0) { atomicOr(&bits[e], kPruneRemovedBit); break; }
}

// bits: in, the weak and removed bits; out, arc_flags
__global__ void __launch_bounds__(kPassBlock)
prune_count_kernel(int nv, const gact_graph_arc *__restrict__ arcs, const int *__restrict__ first, const int *__restrict__ skip,
                   int *bits, unsigned long long *counters, const int *__restrict__ flag)
{
    if (*flag) return;
    const int x = blockIdx.x * kPassBlock + threadIdx.x;
    int before = 0, removed = 0;
    if (x < nv) {
        const int end = first[x + 1];
        for (int k = first[x]; k < end; k++) {
            const gact_graph_arc a = arcs[k];
            const bool gone = (bits[k] & kPruneRemovedBit) != 0;
            if (unitig_in_set(a, skip)) { before++; removed += gone; }
            bits[k] = a.flags | (gone ? GACT_GRAPH_ARC_SHORT : 0);
        }
    }
    wave_count(&counters[kPruneBared], before >= 1 && removed == before);
    removed = wave_sum(removed);
    if ((threadIdx.x & 63) == 0 && removed) atomicAdd(&counters[kPruneRemoved], (unsigned long long)removed);
}

__global__ void __launch_bounds__(kPassBlock)
clean_init_kernel(int n_reads, const gact_graph_read *__restrict__ reads, const int *__restrict__ lens, const int *__restrict__ clip,
                  gact_clean_read *__restrict__ state)
{
    const int i = blockIdx.x * kPassBlock + threadIdx.x;
    if (i >= n_reads) return;
    gact_clean_read s;
    s.state = reads[i].contained_by >= 0 ? GACT_UNITIG_CONTAINED : !unitig_live(reads, lens, clip, i) ? GACT_UNITIG_EMPTY : GACT_CLEAN_KEPT;
    s.step = -1;
    state[i] = s;
}

// behind unitig_tip_kernel: lane k is arc k, vertex k and read k, each where there is one
__global__ void __launch_bounds__(kPassBlock)
clean_tip_kernel(int n_reads, gact_graph_arc *__restrict__ arcs, int n_arcs, const gact_graph_read *__restrict__ reads,
                 const int *__restrict__ lens, const int *__restrict__ clip, const int *__restrict__ prev,
                 const int *__restrict__ cut, int step, gact_clean_read *__restrict__ state, unsigned long long *counters,
                 const int *__restrict__ flag)
{
    if (*flag) return;
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    bool gone = false, head = false, first_cut = false;
    if (k < n_arcs) {
        const gact_graph_arc a = arcs[k];
        gone = a.flags == 0 && (cut[a.u >> 1] || cut[a.v >> 1]);
        if (gone) arcs[k].flags = GACT_GRAPH_ARC_TIP;
    }
    if (k < 2 * n_reads) head = unitig_live(reads, lens, clip, k >> 1) && prev[k] < 0;
    if (k < n_reads && cut[k] && state[k].state == GACT_CLEAN_KEPT) {
        first_cut = true;
        gact_clean_read s;
        s.state = GACT_UNITIG_TIP; s.step = step;
        state[k] = s;
    }
    wave_count(&counters[kCleanArcs], gone);
    wave_count(&counters[kCleanHeads], head);
    wave_count(&counters[kCleanReads], first_cut);
}

// new_flags: what bubble_flag_kernel or prune_count_kernel left; gone: NULL, or the reads a bubble removed
__global__ void __launch_bounds__(kPassBlock)
clean_apply_kernel(gact_graph_arc *__restrict__ arcs, int n_arcs, const int *__restrict__ new_flags, int n_reads,
                   const int *__restrict__ gone, int step, gact_clean_read *__restrict__ state, const int *__restrict__ flag)
{
    if (*flag) return;
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    if (k < n_arcs) arcs[k].flags = new_flags[k];
    if (gone && k < n_reads && gone[k]) {
        gact_clean_read s;
        s.state = GACT_CLEAN_BUBBLE; s.step = step;
        state[k] = s;
    }
}

// the flags as the last step left them, one word per arc: what goes back to the host
__global__ void __launch_bounds__(kPassBlock)
clean_flags_kernel(const gact_graph_arc *__restrict__ arcs, int n_arcs, int *__restrict__ out_flags, const int *__restrict__ flag)
{
    if (*flag) return;
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    if (k < n_arcs) out_flags[k] = arcs[k].flags;
}

}  // namespace gact

// The prune step on an indexed graph (ArcGraphDev, gact_unitig.hpp), as the prune call and the rounds make it: W is the arcs
// with flags == 0 that touch no read of g.skip.  bits and the counters are the caller's to have zeroed; bits leaves as arc_flags,
// best (NULL: not wanted) as vertex_best
static void prune_step(const gact_hip_engine *e, const ArcGraphDev &g, int ratio, int *bits, int *best, unsigned long long *counters)
{
    const dim3 block(gact::kPassBlock);
    const size_t nv = (size_t)g.nv, na = (size_t)g.n_arcs;
    hipLaunchKernelGGL(gact::prune_mark_kernel, wave_blocks(e, nv), block, 0, g.stream, g.nv, g.arcs, g.first, g.skip, ratio, bits, best,
                       counters, g.flag);
    hipLaunchKernelGGL(gact::prune_mirror_kernel, lane_blocks(na), block, 0, g.stream, g.arcs, g.n_arcs, g.first, bits, g.flag);
    hipLaunchKernelGGL(gact::prune_count_kernel, lane_blocks(nv), block, 0, g.stream, g.nv, g.arcs, g.first, g.skip, bits, counters, g.flag);
}

// One allocation: the graph (ArcGraphDev) | [ out of E0 (4 per vertex) | bits (4 n_arcs) | counters (64) | flag (16) ], zeroed
// together | first (4 (2 n_reads + 1)) | best (4 per vertex).
int gact_hip_prune_overlaps(gact_hip_engine *e, int slot, int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                            const gact_graph_read *reads, int64_t n_arcs, const gact_graph_arc *arcs, const uint8_t *skip,
                            const gact_prune_params *params, int32_t *arc_flags, int32_t *vertex_best)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (!read_lens || !reads || !arc_flags)
        return fail(GACT_HIP_EINVAL, "prune_overlaps: NULL argument (read_lens, reads and arc_flags are needed)");
    const gact_prune_params p = params ? *params : gact_prune_params{GACT_PRUNE_DEFAULT_RATIO_PERMILLE};
    if (p.ratio_permille < 0 || p.ratio_permille > 1000)
        return fail(GACT_HIP_EINVAL, "prune_overlaps: bad parameter (ratio_permille = %d: 0 .. 1000)", p.ratio_permille);
    if (check_arc_graph("prune_overlaps", n_reads, read_lens, clip, n_arcs, arcs) < 0) return GACT_HIP_EINVAL;
    if (n_reads == 0) return 0;
    if ((rc = set_device(e))) return rc;
    Slot &sl = e->slots[slot];
    PassScratch<gact_prune_stats> &pb = sl.prune;
    ArcGraphDev g = arc_graph_layout(n_reads, clip, n_arcs, skip);
    const size_t nv = 2 * (size_t)n_reads, na = (size_t)n_arcs;
    const size_t at_out0 = g.end;
    const size_t at_bits = at_out0 + nv * sizeof(int);
    const size_t at_counters = up16(at_bits + na * sizeof(int));
    const size_t at_flag = at_counters + 8 * sizeof(unsigned long long);
    const size_t at_first = at_flag + 16;
    const size_t at_best = up16(at_first + (nv + 1) * sizeof(int));
    const size_t bytes = at_best + nv * sizeof(int);
    if ((rc = arc_graph_begin(g, pb, bytes, sl.stream, "prune_overlaps", read_lens, clip, reads, arcs))) return rc;
    int *d_out0 = (int *)(pb.p + at_out0), *d_bits = (int *)(pb.p + at_bits), *d_flag = (int *)(pb.p + at_flag);
    unsigned long long *d_counters = (unsigned long long *)(pb.p + at_counters);
    int *d_first = (int *)(pb.p + at_first), *d_best = (int *)(pb.p + at_best);
    HIP_TRY(hipMemsetAsync(d_out0, 0, at_first - at_out0, sl.stream));
    arc_graph_index(g, 0, d_first, d_out0, d_counters, d_flag);
    prune_step(e, g, p.ratio_permille, d_bits, d_best, d_counters);
    // the one wait: the flag word, before the copies out
    unsigned long long counters[8];
    if ((rc = arc_graph_fetch(g, "prune_overlaps", d_counters, counters, 8))) return rc;
    if (na) HIP_TRY(hipMemcpyAsync(arc_flags, d_bits, na * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
    if (vertex_best) HIP_TRY(hipMemcpyAsync(vertex_best, d_best, nv * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
    if ((rc = pb.end(sl.stream))) return rc;
    gact_prune_stats &st = pb.stats;
    st.reads = n_reads;
    st.examined = (int32_t)counters[gact::kPruneExamined];
    st.bared = (int32_t)counters[gact::kPruneBared];
    st.working_arcs = (int64_t)counters[gact::kPruneW];
    st.weak = (int64_t)counters[gact::kPruneWeak];
    st.arcs_removed = (int64_t)counters[gact::kPruneRemoved];
    st.scratch_bytes = (int64_t)pb.bytes;
    return 0;
}

int gact_hip_last_prune_stats(gact_hip_engine *e, int slot, gact_prune_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::prune, stats, "last_prune_stats", "has pruned no overlaps yet");
}

// One allocation: the graph (ArcGraphDev, no skip) | [ out, found (4 each per vertex) | gone (4 n_reads) | bits (4 n_arcs) |
// counters (128) | n_found (16) ], zeroed together in front of every step | flag (16), zeroed once | first (4 (2 n_reads + 1)) | prev, len_in, len_out (4 each per vertex) | cut, owner,
// read_bubble (4 each per read) | rank a, rank b (24 each per vertex) | bubbles (32 per vertex) | state (8 n_reads).
int gact_hip_clean_graph(gact_hip_engine *e, int slot, int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                         const gact_graph_read *reads, int64_t n_arcs, const gact_graph_arc *arcs, const gact_clean_params *params,
                         int32_t *arc_flags, gact_clean_read *read_state, gact_clean_step *steps, int64_t steps_cap, int64_t *n_steps)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (!read_lens || !reads || !arc_flags || !read_state || !n_steps)
        return fail(GACT_HIP_EINVAL, "clean_graph: NULL argument (read_lens, reads, arc_flags, read_state and n_steps are needed)");
    const gact_clean_params p = params ? *params
                                       : gact_clean_params{GACT_UNITIG_DEFAULT_TIP_READS, GACT_BUBBLE_DEFAULT_MAX_DIST, GACT_BUBBLE_MAX_VERTICES,
                                                           500, 700, 3, 4};
    if (p.tip_reads < 1 || p.max_dist < 1 || p.max_dist > (1 << 30) || p.max_vertices < 3 || p.max_vertices > GACT_BUBBLE_MAX_VERTICES)
        return fail(GACT_HIP_EINVAL, "clean_graph: bad parameter (tip_reads = %d: >= 1; max_dist = %d: 1 .. 2^30; max_vertices = %d: 3 .. %d)",
                    p.tip_reads, p.max_dist, p.max_vertices, GACT_BUBBLE_MAX_VERTICES);
    if (p.ratio_lo_permille < 0 || p.ratio_hi_permille > 1000 || p.ratio_lo_permille > p.ratio_hi_permille || p.n_ratios < 0 ||
        p.n_ratios > GACT_CLEAN_MAX_RATIOS || p.max_passes < 1 || p.max_passes > GACT_CLEAN_MAX_PASSES)
        return fail(GACT_HIP_EINVAL, "clean_graph: bad parameter (ratios %d .. %d: 0 <= lo <= hi <= 1000; n_ratios = %d: 0 .. %d; max_passes = %d: 1 .. %d)",
                    p.ratio_lo_permille, p.ratio_hi_permille, p.n_ratios, GACT_CLEAN_MAX_RATIOS, p.max_passes, GACT_CLEAN_MAX_PASSES);
    if (check_arc_graph("clean_graph", n_reads, read_lens, clip, n_arcs, arcs, "steps_cap", steps_cap, steps_cap < 0) < 0)
        return GACT_HIP_EINVAL;
    if (n_reads == 0) {
        *n_steps = 0;
        return 0;
    }
    if ((rc = set_device(e))) return rc;
    Slot &sl = e->slots[slot];
    PassScratch<gact_clean_stats> &cb = sl.clean;
    ArcGraphDev g = arc_graph_layout(n_reads, clip, n_arcs, nullptr);
    const size_t n = (size_t)n_reads, nv = 2 * n, na = (size_t)n_arcs;
    const size_t at_out = g.end;
    const size_t at_found = at_out + nv * sizeof(int);
    const size_t at_gone = at_found + nv * sizeof(int);
    const size_t at_bits = at_gone + n * sizeof(int);
    const size_t at_counters = up16(at_bits + na * sizeof(int));
    const size_t at_n_found = at_counters + gact::kCleanCounters * sizeof(unsigned long long);
    const size_t at_flag = at_n_found + 16;
    const size_t at_first = at_flag + 16;
    const size_t at_prev = up16(at_first + (nv + 1) * sizeof(int));
    const size_t at_len_in = at_prev + nv * sizeof(int);
    const size_t at_len_out = at_len_in + nv * sizeof(int);
    const size_t at_cut = at_len_out + nv * sizeof(int);
    const size_t at_owner = at_cut + n * sizeof(int);
    const size_t at_read_bubble = at_owner + n * sizeof(int);
    const size_t at_rank_a = up16(at_read_bubble + n * sizeof(int));
    const size_t at_rank_b = at_rank_a + nv * sizeof(gact::UnitigRank);
    const size_t at_bubbles = up16(at_rank_b + nv * sizeof(gact::UnitigRank));
    const size_t at_state = at_bubbles + nv * sizeof(gact_bubble);
    const size_t bytes = at_state + n * sizeof(gact_clean_read);
    if ((rc = arc_graph_begin(g, cb, bytes, sl.stream, "clean_graph", read_lens, clip, reads, arcs))) return rc;
    int *d_out = (int *)(cb.p + at_out), *d_found = (int *)(cb.p + at_found), *d_gone = (int *)(cb.p + at_gone);
    int *d_bits = (int *)(cb.p + at_bits), *d_flag = (int *)(cb.p + at_flag);
    unsigned long long *d_counters = (unsigned long long *)(cb.p + at_counters);
    long long *d_n_found = (long long *)(cb.p + at_n_found);
    int *d_first = (int *)(cb.p + at_first), *d_cut = (int *)(cb.p + at_cut), *d_owner = (int *)(cb.p + at_owner);
    int *d_read_bubble = (int *)(cb.p + at_read_bubble);
    const UnitigRankBufs rb{(int *)(cb.p + at_prev), (int *)(cb.p + at_len_in), (int *)(cb.p + at_len_out), nullptr,
                            {(gact::UnitigRank *)(cb.p + at_rank_a), (gact::UnitigRank *)(cb.p + at_rank_b)}};
    gact_bubble *d_bubbles = (gact_bubble *)(cb.p + at_bubbles);
    gact_clean_read *d_state = (gact_clean_read *)(cb.p + at_state);
    HIP_TRY(hipMemsetAsync(d_out, 0, at_first - at_out, sl.stream));
    const dim3 block(gact::kPassBlock);
    // the stretches and the arc checks, once: no step moves an arc, and every step leaves the arcs with flags == 0 closed under
    // complement and between live reads
    arc_graph_index(g, 0, d_first, d_out, d_counters, d_flag);
    hipLaunchKernelGGL(gact::clean_init_kernel, lane_blocks(n), block, 0, sl.stream, n_reads, g.reads, g.lens, g.clip, d_state);
    std::vector<gact_clean_step> log;
    gact_clean_stats st{};
    unsigned long long counters[gact::kCleanCounters];
    // what every step ends with: its counters and the flag word on the host
    auto fetch = [&]() { return arc_graph_fetch(g, "clean_graph", d_counters, counters, gact::kCleanCounters); };
    auto record = [&](int kind, int param, unsigned long long reads_removed, unsigned long long examined, unsigned long long had,
                      unsigned long long removed) {
        gact_clean_step s;
        s.kind = kind; s.param = param; s.reads_removed = (int32_t)reads_removed; s.examined = (int32_t)examined;
        s.arcs_removed = (int64_t)removed; s.arcs_left = (int64_t)(had - removed);
        log.push_back(s);
        st.arcs_removed[kind] += s.arcs_removed;
        st.arcs_left = s.arcs_left;
    };
    // T: the first sweep of the unitig call and its tip rule on the arcs as they are; -> the arcs removed, or < 0
    auto tips = [&]() -> long long {
        const gact::UnitigRank *ranks;
        HIP_TRY(hipMemsetAsync(d_out, 0, at_flag - at_out, sl.stream));      // (the step's block; the flag word stays)
        if (int bad = unitig_sweep(g, rb, nullptr, d_out, nullptr, d_counters, nullptr, &ranks, nullptr)) return bad;
        hipLaunchKernelGGL(gact::unitig_tip_kernel, lane_blocks(n), block, 0, sl.stream, n_reads, g.reads, g.lens, g.clip, rb.prev, d_out,
                           ranks, p.tip_reads, d_cut, d_counters, d_flag);
        hipLaunchKernelGGL(gact::clean_tip_kernel, lane_blocks(std::max(na, nv)), block, 0, sl.stream, n_reads, g.arcs, g.n_arcs, g.reads, g.lens,
                           g.clip, rb.prev, d_cut, (int)log.size(), d_state, d_counters, d_flag);
        if (int bad = fetch()) return bad < 0 ? bad : -1;
        record(GACT_CLEAN_TIPS, p.tip_reads, counters[gact::kCleanReads], counters[gact::kCleanHeads], counters[gact::kUnitigE1],
               counters[gact::kCleanArcs]);
        st.reads_tip += (int32_t)counters[gact::kCleanReads];
        return (long long)counters[gact::kCleanArcs];
    };
    // B: the bubble call's step, no read skipped
    auto bubbles = [&]() -> long long {
        HIP_TRY(hipMemsetAsync(d_out, 0, at_flag - at_out, sl.stream));      // (the step's block; the flag word stays)
        if (int bad = bubble_step(e, g, d_out, gact_bubble_params{p.max_dist, p.max_vertices}, d_owner, d_found, d_n_found, d_bubbles,
                                  d_read_bubble, d_gone, d_bits, d_counters))
            return bad;
        hipLaunchKernelGGL(gact::clean_apply_kernel, lane_blocks(std::max(na, n)), block, 0, sl.stream, g.arcs, g.n_arcs, d_bits, n_reads, d_gone,
                           (int)log.size(), d_state, d_flag);
        if (int bad = fetch()) return bad < 0 ? bad : -1;
        record(GACT_CLEAN_BUBBLES, p.max_dist, counters[gact::kBubbleReadsRemoved], counters[gact::kBubbleSources], counters[gact::kBubbleW],
               counters[gact::kBubbleArcsRemoved]);
        st.reads_bubble += (int32_t)counters[gact::kBubbleReadsRemoved];
        return (long long)counters[gact::kBubbleArcsRemoved];
    };
    // P: the prune call's step, no read skipped, vertex_best not wanted
    auto prune = [&](int ratio) -> long long {
        HIP_TRY(hipMemsetAsync(d_out, 0, at_flag - at_out, sl.stream));      // (the step's block; the flag word stays)
        prune_step(e, g, ratio, d_bits, nullptr, d_counters);
        hipLaunchKernelGGL(gact::clean_apply_kernel, lane_blocks(na), block, 0, sl.stream, g.arcs, g.n_arcs, d_bits, n_reads, nullptr,
                           (int)log.size(), d_state, d_flag);
        if (int bad = fetch()) return bad < 0 ? bad : -1;
        record(GACT_CLEAN_PRUNE, ratio, 0, counters[gact::kPruneExamined], counters[gact::kPruneW], counters[gact::kPruneRemoved]);
        return (long long)counters[gact::kPruneRemoved];
    };
    auto settle = [&]() -> int {
        for (int pass = 0; pass < p.max_passes; pass++) {
            const long long t = tips();
            if (t < 0) return (int)t;
            const long long b = bubbles();
            if (b < 0) return (int)b;
            st.passes++;
            if (t + b == 0) break;
        }
        return 0;
    };
    if ((rc = settle())) return rc;
    for (int j = 0; j < p.n_ratios; j++) {
        const int ratio = p.n_ratios == 1 ? p.ratio_lo_permille
                                          : p.ratio_lo_permille + (p.ratio_hi_permille - p.ratio_lo_permille) * j / (p.n_ratios - 1);
        const long long removed = prune(ratio);
        if (removed < 0) return (int)removed;
        if (removed > 0 && (rc = settle())) return rc;
    }
    hipLaunchKernelGGL(gact::clean_flags_kernel, lane_blocks(na), block, 0, sl.stream, g.arcs, g.n_arcs, d_bits, d_flag);
    HIP_TRY(hipGetLastError());
    if (na) HIP_TRY(hipMemcpyAsync(arc_flags, d_bits, na * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipMemcpyAsync(read_state, d_state, n * sizeof(gact_clean_read), hipMemcpyDeviceToHost, sl.stream));
    *n_steps = (int64_t)log.size();
    const bool room = steps && steps_cap >= (int64_t)log.size();
    if (room) memcpy(steps, log.data(), log.size() * sizeof(gact_clean_step));
    const gact_clean_stats sum = st;
    if ((rc = cb.end(sl.stream))) return rc;
    const float ms = cb.stats.device_ms;
    cb.stats = sum;
    cb.stats.device_ms = ms;
    cb.stats.reads = n_reads;
    cb.stats.steps = (int32_t)log.size();
    cb.stats.scratch_bytes = (int64_t)cb.bytes;
    if (!room)
        return fail(GACT_HIP_EINVAL, "clean_graph: %lld steps, room for %lld: call again with room for *n_steps", (long long)log.size(),
                    steps ? (long long)steps_cap : 0ll);
    return 0;
}

int gact_hip_last_clean_stats(gact_hip_engine *e, int slot, gact_clean_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::clean, stats, "last_clean_stats", "has cleaned no graph yet");
}
