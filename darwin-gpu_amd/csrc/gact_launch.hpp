// gact_launch.hpp -- the launching half of a run: gact_policy.hpp says WHAT a pass over `count` candidates runs as,
// gact_launch_table.hpp which kernels that names, and this file issues it -- lanes and their queues, the seed and main
// launches of a pass in each of the plan's sequences, and the choreography of a routed run (2-bit launches, raw-byte launches,
// the side lane).  Included by gact_engine.hip, inside its unnamed namespace, behind Slot and gact_hip_engine.
#pragma once

#include "gact_launch_table.hpp"

// what a seed launch + main launch pair runs on: the slot's own stream, counters, hand-off lists and workspace, or
// the slot's side lane.  Chain states and records are indexed by candidate and shared.
struct Lane {
    hipStream_t stream;
    int *d_counter;
    int *live;
    size_t live_cap;
    uint32_t *d_ws;
    size_t ws_words;
    int max_blocks;                      // 0: whatever the kernel's occupancy allows (the workspace is sized for it)
};

Lane main_lane(gact_hip_engine *e, Slot &sl) { return Lane{sl.stream, sl.d_counter, sl.live.p, sl.live.cap, sl.d_ws, e->ws_words_total, 0}; }

gact::ChainQueues queues(const Lane &ln, Slot &sl)
{
    gact::ChainQueues q;
    q.pop_seed = ln.d_counter;
    q.seed_cells = reinterpret_cast<unsigned long long *>(ln.d_counter + 2);
    q.bucket_count = ln.d_counter + 8;
    q.bucket_pop = ln.d_counter + 8 + gact::kBuckets;
    q.live = ln.live;
    q.live_stride = (int)(ln.live_cap / (2 * gact::kBuckets));       // (the second half: the second set of overlapped seeding)
    q.states = sl.chain_states.p;
    q.longest_now = ln.d_counter + 8 + 2 * gact::kBuckets;
    q.band_redos = ln.d_counter + 6;
    q.list_count = nullptr;
    q.list = nullptr;
    q.list_n = -1;
    q.more_flag = nullptr;
    q.more_count = q.more_pop = q.more_live = nullptr;
    q.leave_longest = 0;
    return q;
}

// the second set of queues of a lane as a launch's own set
gact::ChainQueues second_queues(const Lane &ln, Slot &sl)
{
    gact::ChainQueues q = queues(ln, sl);
    q.pop_seed = ln.d_counter + 1;
    q.bucket_count = ln.d_counter + kMoreCount;
    q.bucket_pop = ln.d_counter + kMorePop;
    q.live = ln.live + (size_t)gact::kBuckets * q.live_stride;
    return q;
}

// a lane's first set of queues for a launch that goes on with the second one once `d_counter + 7` says it is complete
// (both main launches of overlapped seeding; the empty warm-up launches of gact_hip_prepare)
gact::ChainQueues both_queues(const Lane &ln, Slot &sl)
{
    gact::ChainQueues q = queues(ln, sl);
    const gact::ChainQueues s2 = second_queues(ln, sl);
    q.more_flag = ln.d_counter + 7;
    q.more_count = s2.bucket_count; q.more_pop = s2.bucket_pop; q.more_live = s2.live;
    return q;
}

// the second stream of overlapped seeding and of the critical lane (run_overlapped, run_crit_lane)
int ensure_aux_stream(Slot &sl)
{
    if (sl.aux_stream) return 0;
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(hipStreamCreateWithPriority(&sl.aux_stream, hipStreamNonBlocking, hi));
    HIP_TRY(hipEventCreateWithFlags(&sl.aux_ev_a, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&sl.aux_ev_b, hipEventDisableTiming));
    return 0;
}

// GACT_HIP_POISON_WS: seeded garbage over a lane's whole traceback workspace (poison_kernel)
int poison_lane(gact_hip_engine *e, const Lane &ln, uint32_t salt)
{
    if (!e->poison) return 0;
    hipLaunchKernelGGL(gact::poison_kernel, dim3(e->prop.multiProcessorCount * 8), dim3(256), 0, ln.stream, ln.d_ws,
                       ln.ws_words + 64, e->poison * 0x01000193u + salt);
    HIP_TRY(hipGetLastError());
    return 0;
}

int poison_ws(gact_hip_engine *e, Slot &sl, uint32_t salt) { return poison_lane(e, main_lane(e, sl), salt); }

size_t ws_words_for(const gact_hip_engine *e, int blocks)
{
    const size_t groups = (size_t)blocks * (gact::kBlockThreads / 64) * gact::kGroupsPerWave;
    return groups * gact::kSlots * (size_t)e->kp.ws_words;             // two tiles per group in the p16 kernel
}

// the side lane of a slot, for `count` candidates on at most `blocks` blocks
int side_lane(gact_hip_engine *e, Slot &sl, int count, int blocks, Lane *out)
{
    if (!sl.side_stream) {
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        // ahead of the slot's own stream: its main launch must find room while the 2-bit seed launch drains
        HIP_TRY(hipStreamCreateWithPriority(&sl.side_stream, hipStreamNonBlocking, hi));
        HIP_TRY(hipEventCreateWithFlags(&sl.side_done, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&sl.side_go, hipEventDisableTiming));
        HIP_TRY(hipMalloc((void **)&sl.side_counter, kCounterInts * sizeof(int)));
    }
    if (blocks > sl.side_blocks) {
        if (sl.side_ws) (void)hipFree(sl.side_ws);
        sl.side_ws = nullptr; sl.side_blocks = 0;
        if (hipMalloc((void **)&sl.side_ws, (ws_words_for(e, blocks) + 64) * sizeof(uint32_t)) != hipSuccess)
            return fail(GACT_HIP_ENOMEM, "side workspace allocation failed (%zu MiB)", ws_words_for(e, blocks) * 4 >> 20);
        sl.side_blocks = blocks;
        HIP_TRY(hipMemsetAsync(sl.side_ws, 0xA5, (ws_words_for(e, blocks) + 64) * sizeof(uint32_t), sl.side_stream));
    }
    if (sl.side_live.reserve(2 * (size_t)count * gact::kBuckets)) return fail(GACT_HIP_ENOMEM, "device allocation failed");
    *out = Lane{sl.side_stream, sl.side_counter, sl.side_live.p, sl.side_live.cap, sl.side_ws, ws_words_for(e, sl.side_blocks), sl.side_blocks};
    return 0;
}

// int32 kernel alone, or (scoring permitting) int32 seed launch for the first
// tiles followed by the packed-int16 main launch for the rest of every chain
int launch_big_extend(gact_hip_engine *e, Slot &sl, int first, int n, int rc_from, int same_file)
{
    const SeqSet &rs = e->sets[GACT_SET_REF];
    const SeqSet &qf = e->sets[GACT_SET_QUERY], &qr = e->sets[GACT_SET_QUERY_RC];
    const Lane own = main_lane(e, sl);
    const int blocks = std::max(1, std::min((n + 3) / 4, e->big_blocks));
    auto k = e->big_cb == 16 ? gact::big_extend_kernel<16> : gact::big_extend_kernel<32>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(gact::kBlockThreads), 0, sl.stream, e->kp, rs.dev(true), qf.dev_or(true, rs),
                       qr.dev_or(true, rs), sl.cands.p, first, n, rc_from, same_file, sl.overlaps.p, queues(own, sl),
                       reinterpret_cast<uint8_t *>(sl.d_ws));
    HIP_TRY(hipGetLastError());
    return 0;
}

// the engine's capabilities as the launch policy sees them (gact_policy.hpp)
gact_policy::Caps policy_caps(const gact_hip_engine *e)
{
    gact_policy::Caps c;
    c.C = e->C; c.p16 = e->p16; c.seed16 = e->seed16; c.lin = e->lin; c.aff = e->aff; c.aff_seed = e->aff_seed; c.split = e->split; c.tagged = e->tagged;
    c.mismatch_below_extend = e->params.mismatch < e->params.gap_extend;
    c.shared_twelfths = e->shared_twelfths; c.lone_lane = e->lone_lane; c.overlap_big = e->overlap_big; c.roles = e->roles; c.coop = (e->lin && e->split && e->C == 20) ? e->coop : -1; c.overlap_seed = e->overlap_seed; c.crit_lane = e->crit_lane; c.crit_lane_always = e->crit_lane_always;
    c.lane_small = e->lane_small; c.lane_small_factor = e->lane_small_factor; c.lane_blocks = e->lane_blocks; c.team_when_shared = e->team_when_shared;
    c.wide = e->wide; c.wide_blocks_per_cu = e->wide_blocks_per_cu; c.cus = e->prop.multiProcessorCount;
    c.grid_blocks = e->grid_blocks; c.seed_grid_blocks = e->seed_grid_blocks; c.seed_lin_grid_blocks = e->seed_lin_grid_blocks;
    c.lin_grid_blocks = e->lin_grid_blocks; c.aff_grid_blocks = e->aff_grid_blocks; c.wide_lin_grid_blocks = e->wide_lin_grid_blocks;
    c.role_grid_blocks = e->role_grid_blocks; c.role_dp_waves = gact::kRoleDp;
    c.ws_words_per_tile = (size_t)e->kp.ws_words;
    c.role_ws_words_per_block = gact::role_ws_words<gact::SplitLayoutLin<7, 13>>(1);
    c.coop_ws_words_per_block = gact::coop_ws_words<gact::SplitLayoutLin<7, 13>>(1);
    return c;
}

// One run's launches (launch_extend; gact_hip_prepare's empty ones) ...
struct RunCtx {
    gact_hip_engine *e;
    Slot &sl;
    int first, n, rc_from, same_file;    // the candidate range
    gact::KParams kp;                    // the engine's, with this run's priority thresholds
    bool shared_machine;                 // another slot of this engine is running, or the caller keeps runs in flight
    bool trace;                          // GACT_HIP_TRACE: every launch named on stderr and waited for (a faulting kernel is the last one named)
};
// ... and one pass of them: a seed launch + main launch(es) over `count` candidates at most, on one lane, from one image of the sets
struct Pass {
    const Lane &ln;
    bool raw;
    gact::SeqSetDev d_rs, d_qf, d_qr;
    int count;
    bool first_pass;                     // the pass the run's statistics describe
};

int traced(const RunCtx &c, const Lane &ln, const char *what, int blocks, int count)
{
    if (!c.trace) return 0;
    fprintf(stderr, "[gact_hip] %s: %d blocks, %d candidates ... ", what, blocks, count);
    fflush(stderr);
    HIP_TRY(hipStreamSynchronize(ln.stream));
    int dbg[8];
    HIP_TRY(hipMemcpy(dbg, ln.d_counter, sizeof dbg, hipMemcpyDeviceToHost));
    fprintf(stderr, "done (popped %d)\n", dbg[0]);
    return 0;
}

// A main launch of table row `k` (gact_launch_table.hpp): the same arguments whatever the kernel.  The engine's C and its drift
// frame pick the form; two_sets asks for the form that goes on with a second set of queues.
int launch_main(const RunCtx &c, const Pass &ps, gact_policy::MainK k, bool two_sets, int blocks, hipStream_t stream, const gact::ChainQueues &q,
                uint32_t *ws)
{
    MainFn fn = nullptr;
    int threads = 0;
    if (int rc = resolve_main(c.e->C, k, c.e->lin_row, two_sets, &fn, &threads)) return rc;
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(threads), 0, stream, c.kp, c.e->kc, ps.d_rs, ps.d_qf, ps.d_qr, c.same_file, c.sl.overlaps.p, q, ws);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_seed(const RunCtx &c, const Pass &ps, gact_policy::SeedK k, int blocks, hipStream_t stream, const gact::ChainQueues &q, uint32_t *ws)
{
    gact_hip_engine *e = c.e;
    const dim3 g((unsigned)blocks), b256(gact::kBlockThreads);
    if (k == gact_policy::SeedK::Int32) {
        auto i32 = e->C == 20 ? gact::chain_kernel<20, gact::SeedSink> : gact::chain_kernel<32, gact::SeedSink>;
        hipLaunchKernelGGL(i32, g, b256, 0, stream, c.kp, ps.d_rs, ps.d_qf, ps.d_qr, c.sl.cands.p, c.n, c.rc_from, c.same_file, c.sl.overlaps.p, q,
                           gact::SeedSink{c.first, e->p16 ? 1 : 0}, ws);
    } else {
        SeedFn fn = nullptr;
        if (int rc = resolve_seed(e->C, k, &fn)) return rc;
        hipLaunchKernelGGL(fn, g, b256, 0, stream, c.kp, e->kc, ps.d_rs, ps.d_qf, ps.d_qr, c.sl.cands.p, c.first, c.n, c.rc_from, c.same_file,
                           c.sl.overlaps.p, q, ws);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// Overlapped, ordered seeding (round 4).  One at a time a run was: seed launch (every first tile, ~2 ms on ecoli10x) ->
// main launch, whose longest chains -- the ones that end last -- started only then.  Here the candidates are first
// sorted by the length class of the chain they can make (two tiny launches), and
//   slot stream : seed launch A (the longest nA: as many as main launch 1 has tile slots)  ->  main launch 1, on two
//                 thirds of the resident blocks, popping set 1 (A's hand-offs), later set 2
//   aux stream  : [after A] seed launch B (the rest, on the last third of the blocks, into a SECOND set of queues)
//                 -> flag -> main launch 2 (that third of the blocks, set 2)
// Every producer / consumer pair of a set of queues is still separated by a launch boundary (or by the flag written
// in stream order behind seed launch B plus an acquire, extend_p16_kernel): nothing is handed over between running
// launches.  The two thirds / one third of the workspace go with the blocks.
int run_overlapped(const RunCtx &c, const Pass &ps, const gact_policy::Plan &plan)
{
    namespace pol = gact_policy;
    Slot &sl = c.sl;
    const Lane &ln = ps.ln;
    const int count = ps.count;
    int rc = ensure_aux_stream(sl);
    if (rc) return rc;
    const int ob = std::max(1, std::min((count + 255) / 256, 1024));
    hipLaunchKernelGGL(gact::order_hist_kernel, dim3(ob), dim3(256), 0, ln.stream, sl.cands.p, c.first, count, c.rc_from, ps.d_rs.offsets,
                       ps.d_qf.offsets, ps.d_qr.offsets, c.kp.early, ln.d_counter + kOrderHist);
    hipLaunchKernelGGL(gact::order_scatter_kernel, dim3(ob), dim3(256), 0, ln.stream, sl.cands.p, c.first, count, c.rc_from,
                       ps.d_rs.offsets, ps.d_qf.offsets, ps.d_qr.offsets, c.kp.early, ln.d_counter + kOrderHist,
                       ln.d_counter + kOrderCursor, sl.order.p);
    HIP_TRY(hipGetLastError());
    const int nA = plan.nA;
    // seed launch A
    gact::ChainQueues qa = queues(ln, sl);
    qa.list = sl.order.p; qa.list_n = nA;
    if ((rc = launch_seed(c, ps, plan.seed, plan.seed_blocks, ln.stream, qa, ln.d_ws))) return rc;
    if (ps.first_pass) HIP_TRY(hipEventRecord(sl.ev_mid, ln.stream));
    HIP_TRY(hipEventRecord(sl.aux_ev_a, ln.stream));
    // aux stream: seed launch B into the second set, the flag, main launch 2
    HIP_TRY(hipStreamWaitEvent(sl.aux_stream, sl.aux_ev_a, 0));
    gact::ChainQueues qb = second_queues(ln, sl);
    qb.list = sl.order.p + nA; qb.list_n = count - nA;
    if (count > nA && (rc = launch_seed(c, ps, plan.seed, plan.seedB_blocks, sl.aux_stream, qb, ln.d_ws + plan.ws_split))) return rc;
    HIP_TRY(hipMemsetAsync(ln.d_counter + 7, 0xff, sizeof(int), sl.aux_stream));
    // (both main launches take set 1 -- the longer chains, complete since seed launch A ended -- and then set 2,
    //  open by the time main launch 2 starts)
    const gact::ChainQueues q2 = both_queues(ln, sl);
    // (the critical lane, ChainQueues::leave_longest: main launch 2 in the wide layout, main launch 1 leaves it that many
    //  of the longest chains -- GACT_HIP_CRIT_LANE_ALWAYS; a run this size is bound by throughput)
    if (count > nA && (rc = launch_main(c, ps, plan.lane ? pol::MainK::WideLin : plan.main, true, plan.main2_blocks, sl.aux_stream, q2, ln.d_ws + plan.ws_split))) return rc;
    HIP_TRY(hipEventRecord(sl.aux_ev_b, sl.aux_stream));
    // main launch 1: set 1, then set 2
    gact::ChainQueues q1 = q2;
    q1.leave_longest = plan.leave_longest;
    if ((rc = launch_main(c, ps, plan.main, true, plan.main_blocks, ln.stream, q1, ln.d_ws))) return rc;
    HIP_TRY(hipStreamWaitEvent(ln.stream, sl.aux_ev_b, 0));
    if (ps.first_pass) { sl.shape.wide = false; sl.shape.lin = true; sl.shape.lane = plan.lane; sl.shape.roles = plan.roles ? 1 : plan.coop ? 2 : 0; }
    sl.shape.overlapped = true;
    return 0;
}

// The critical lane beside a run's ONE split main launch (a run too small for overlapped seeding, e.g. the merged
// forward-strand calls of eight feeder threads: 33 k chains on 24.6 k tile slots last as long as their longest
// chain): the wide launch on a third of the blocks, on the second stream, behind the seed launch like the split one
int run_crit_lane(const RunCtx &c, const Pass &ps, const gact_policy::Plan &plan, const gact::ChainQueues &cq)
{
    Slot &sl = c.sl;
    const Lane &ln = ps.ln;
    int rc = ensure_aux_stream(sl);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(sl.aux_ev_a, ln.stream));
    HIP_TRY(hipStreamWaitEvent(sl.aux_stream, sl.aux_ev_a, 0));
    if ((rc = launch_main(c, ps, gact_policy::MainK::WideLin, false, plan.main2_blocks, sl.aux_stream, cq, ln.d_ws + plan.ws_split))) return rc;
    HIP_TRY(hipEventRecord(sl.aux_ev_b, sl.aux_stream));
    gact::ChainQueues cq1 = cq;
    cq1.leave_longest = plan.leave_longest;
    if ((rc = launch_main(c, ps, plan.main, false, plan.main_blocks, ln.stream, cq1, ln.d_ws))) return rc;
    HIP_TRY(hipStreamWaitEvent(ln.stream, sl.aux_ev_b, 0));
    if (ps.first_pass) sl.shape.lane = true;
    return 0;
}

// seed launch, then the main launch: one, or one with the critical lane beside it
int run_plain(const RunCtx &c, const Pass &ps, const gact_policy::Plan &plan, const gact::ChainQueues &cq)
{
    namespace pol = gact_policy;
    Slot &sl = c.sl;
    const Lane &ln = ps.ln;
    int rc = launch_seed(c, ps, plan.seed, plan.seed_blocks, ln.stream, cq, ln.d_ws);
    if (rc) return rc;
    if ((rc = traced(c, ln, ps.raw ? "seed launch (raw bytes)" : "seed launch (2-bit)", plan.seed_blocks, ps.count))) return rc;
    if (plan.seq == pol::Seq::SingleInt32) return 0;
    if (ps.first_pass) HIP_TRY(hipEventRecord(sl.ev_mid, ln.stream));
    if ((rc = poison_lane(c.e, ln, 0x5bd1e995u))) return rc;      // the main launch reads nothing the seed launch stored
    if (ps.first_pass) { sl.shape.wide = plan.wide; sl.shape.lin = plan.lin; sl.shape.aff = plan.aff; sl.shape.roles = plan.roles ? 1 : plan.coop ? 2 : 0; }
    if (plan.seq == pol::Seq::CritLane) return run_crit_lane(c, ps, plan, cq);
    if ((rc = launch_main(c, ps, plan.main, false, plan.main_blocks, ln.stream, cq, ln.d_ws))) return rc;
    return traced(c, ln, ps.raw ? "main launch (raw bytes)" : "main launch (2-bit)", plan.main_blocks, ps.count);
}

// One pass: `count` candidates at most -- all of the run's, or those of `list` (routing) -- on lane `ln`.
// second_set: the pass files and pops its chains in the lane's second set of queues (the raw-byte pass behind the 2-bit
// one on the same lane: the first set keeps its counts for the statistics, nothing is cleared between the passes).
// WHAT the pass runs as -- kernels, grids, sequence -- is gact_policy::plan_pass's answer (gact_policy.hpp: a pure function
// of the count and the engine's capabilities); what follows launches it.
int run_pass(const RunCtx &c, const Lane &ln, bool raw, const int *list, const int *list_count, int count, bool first_pass, bool second_set = false)
{
    namespace pol = gact_policy;
    gact_hip_engine *e = c.e;
    Slot &sl = c.sl;
    const SeqSet &rs = e->sets[GACT_SET_REF];
    const SeqSet &qf = e->sets[GACT_SET_QUERY], &qr = e->sets[GACT_SET_QUERY_RC];
    pol::Inputs in;
    in.count = count; in.raw = raw; in.listed = list != nullptr; in.second_set = second_set; in.shared_machine = c.shared_machine;
    in.own_lane = ln.stream == sl.stream; in.trace = c.trace; in.poison = e->poison != 0; in.lane_max_blocks = ln.max_blocks;
    const pol::Plan plan = pol::plan_pass(policy_caps(e), in);
    const Pass ps{ln, raw, rs.dev(raw), qf.dev_or(raw, rs), qr.dev_or(raw, rs), count, first_pass};
    gact::ChainQueues cq = second_set ? second_queues(ln, sl) : queues(ln, sl);
    cq.list = list; cq.list_count = list_count;
    if (c.trace) {
        fprintf(stderr, "[gact_hip] pass raw=%d listed=%d side=%d count=%d first=%d n=%d rc_from=%d plan=%s\n", (int)raw, list != nullptr,
                ln.stream != sl.stream, count, c.first, c.n, c.rc_from, pol::describe(plan).c_str());
        fprintf(stderr, "[gact_hip]   ws %p + %zu MiB, counter %p, cands %p (%zu), overlaps %p, live %p (%zu), states %p (%zu x %zu B)\n", (void *)ln.d_ws,
                ln.ws_words * 4 >> 20, (void *)ln.d_counter, (void *)sl.cands.p, sl.cands.cap, (void *)sl.overlaps.p, (void *)ln.live,
                ln.live_cap, (void *)sl.chain_states.p, sl.chain_states.cap, sizeof(gact::ChainState));
        fprintf(stderr, "[gact_hip]   ref raw %p packed %p offsets %p (%lld bases), query %p %p, rc %p %p\n", (void *)rs.d_raw, (void *)rs.d_packed,
                (void *)rs.d_offsets, (long long)rs.total, (void *)qf.d_raw, (void *)qf.d_packed, (void *)qr.d_raw, (void *)qr.d_packed);
    }
    return plan.seq == pol::Seq::Overlapped ? run_overlapped(c, ps, plan) : run_plain(c, ps, plan, cq);
}

// The lengths of route_kernel's two lists: candidates whose reads are plain A/C/G/T, and the rest.  They decide grids and
// layouts.  A list the host holds (uploaded, not merged, not made by the device filter) is counted on the host from the sets'
// per-sequence flags -- no wait: with other slots' persistent launches on the machine, route_kernel (14 registers: it does
// not fit beside three 168-register waves) starts only when a block of theirs has left, and the host sat in this wait for
// milliseconds (1 % dirty reads, four steps in flight: -10 %).  Any other list: the device's counts, the only host wait of a run.
int count_routed(const RunCtx &c, int strands, bool need_f, bool need_r, int routed[2])
{
    gact_hip_engine *e = c.e;
    Slot &sl = c.sl;
    const int first = c.first, n = c.n, rc_from = c.rc_from;
    const SeqSet &rs = e->sets[GACT_SET_REF];
    const SeqSet &qf = e->sets[GACT_SET_QUERY], &qr = e->sets[GACT_SET_QUERY_RC];
    const bool host_counts = strands < 0 && !sl.h_cands.empty() && (size_t)first + (size_t)n <= sl.h_cands.size() &&
                             (!rs.has_other || (int32_t)rs.h_other.size() == rs.n) && (!need_f || !qf.has_other || (int32_t)qf.h_other.size() == qf.n) &&
                             (!need_r || !qr.has_other || (int32_t)qr.h_other.size() == qr.n);
    if (host_counts) {
        const int64_t key[4] = {first, n, rc_from, e->sets_epoch};
        if (memcmp(key, sl.routed_key, sizeof key)) {
            int dirty = 0;
            for (int k = first; k < first + n; k++) {
                const gact_candidate &cd = sl.h_cands[(size_t)k];
                const SeqSet &qs = k >= rc_from ? qr : qf;
                dirty += ((rs.has_other && rs.h_other[(size_t)cd.ref_id]) || (qs.has_other && qs.h_other[(size_t)cd.query_id])) ? 1 : 0;
            }
            memcpy(sl.routed_key, key, sizeof key);
            sl.routed_host[0] = n - dirty; sl.routed_host[1] = dirty;
        }
        routed[0] = sl.routed_host[0]; routed[1] = sl.routed_host[1];
    } else {
        HIP_TRY(hipMemcpyAsync(routed, sl.d_counter + 4, 2 * sizeof(int), hipMemcpyDeviceToHost, sl.stream));
        HIP_TRY(hipStreamSynchronize(sl.stream));
    }
    return 0;
}

// One run of candidates [first, first + n) of the slot: its passes, and which lane each goes on.
// strands: -1 what [first, first + n) and rc_from say; else bit 0 = forward-strand candidates present, bit 1 =
// reverse-complement ones (merged runs: rc_from == kCompInCand, the strand travels with the candidate)
int launch_extend(gact_hip_engine *e, Slot &sl, int first, int n, int rc_from, int same_file, int strands = -1)
{
    const SeqSet &rs = e->sets[GACT_SET_REF];
    const SeqSet &qf = e->sets[GACT_SET_QUERY], &qr = e->sets[GACT_SET_QUERY_RC];
    const bool need_f = strands >= 0 ? (strands & 1) != 0 : first < rc_from, need_r = strands >= 0 ? (strands & 2) != 0 : first + n > rc_from;
    // Sets that hold bytes other than A/C/G/T (N, lower case) are compared as raw bytes like align.cpp:134.  With the
    // packed kernels that is decided per CANDIDATE: the launches on the 2-bit image put off every candidate one of whose
    // two reads holds such a byte (SeqSetDev::other, from pack_kernel), and a second pair of launches on the raw bytes
    // takes those -- one soft-masked read no longer moves a whole launch onto the slower kernels.
    const bool any_other = rs.has_other || (need_f && qf.has_other) || (need_r && qr.has_other);
    const bool mixed = any_other && e->p16 && e->route_other;
    static const bool trace = opt_env("trace") != nullptr;
    RunCtx c{e, sl, first, n, rc_from, same_file, e->kp, false, trace};
    const int64_t longest = std::min(rs.max_len, std::max(need_f ? qf.max_len : 0, need_r ? qr.max_len : 0));
    // GACT_HIP_STATIC_PRIO: thirds of the longest possible chain instead of the ranking against what is running
    const bool static_prio = e->static_prio;
    c.kp.prio_bases[0] = !e->chain_prio ? 0x7fffffff : static_prio ? (int32_t)std::min<int64_t>(longest / 3, 0x7fffffff) : 0;
    const int rank16 = e->rank16;                    // above 3/4 of the longest running chain: priority 2, above 1/2: 1
    c.kp.prio_bases[1] = !e->chain_prio ? 0x7fffffff : static_prio ? (int32_t)std::min<int64_t>(2 * longest / 3, 0x7fffffff) : rank16;
    sl.shape.two_phase = e->p16;
    // Is another slot of this engine still running?  Then this launch shares the machine (feeder threads, steps in
    // flight) and what counts is throughput: the wide layout -- faster per chain, slower per cell, made for a launch
    // that has the CUs to itself and lasts as long as its longest chain -- is not taken on its own account.
    c.shared_machine = e->caller_keeps_runs_in_flight.load(std::memory_order_relaxed);
    if (e->shared_hint && !c.shared_machine)
        for (const Slot &other : e->slots)
            if (&other != &sl && other.timed && other.ev1 && hipEventQuery(other.ev1) == hipErrorNotReady) { c.shared_machine = true; break; }
    (void)hipGetLastError();                 // (hipErrorNotReady is an answer, not a failure)

    const Lane own = main_lane(e, sl);
    if (!mixed) return run_pass(c, own, any_other, nullptr, nullptr, n, true);
    // the candidates sorted by what their two reads hold: two lists, their lengths back on the host
    const gact::SeqSetDev o_rs = rs.dev(false), o_qf = qf.dev_or(false, rs), o_qr = qr.dev_or(false, rs);
    hipLaunchKernelGGL(gact::route_kernel, dim3(std::max(1, std::min((n + 255) / 256, 1024))), dim3(256), 0, sl.stream, sl.cands.p, first, n,
                       rc_from, o_rs.other, need_f ? o_qf.other : nullptr, need_r ? o_qr.other : nullptr, sl.deferred.p, sl.d_counter + 4);
    HIP_TRY(hipGetLastError());
    int routed[2] = {0, 0};
    int rc = count_routed(c, strands, need_f, need_r, routed);
    if (rc) return rc;
    sl.shape.routed_raw = routed[1];
    // Few raw-byte candidates beside many others: their launches last as long as their longest chain (a wave alone on
    // its SIMD issues every ~8 cycles: a lone chain advances at a third of the machine's per-SIMD rate), so they run
    // BESIDE the 2-bit launches, on the slot's side lane, started first -- the 2-bit main launch's last blocks become
    // resident as the side lane's blocks leave.  Many of them (more than the side lane holds at one tile pair per
    // group): one pass after the other on the whole machine.
    const int side_cap = std::max(1, e->prop.multiProcessorCount / 2);
    const int raw_blocks = ((routed[1] + 2 * gact::kGroupsPerWave - 1) / (2 * gact::kGroupsPerWave) + 3) / 4;
    if (routed[0] > 0 && routed[1] > 0 && e->side_lane && raw_blocks <= side_cap) {
        Lane side;
        if ((rc = side_lane(e, sl, routed[1], std::max(raw_blocks, std::min(side_cap, 16)), &side))) return rc;
        // (the side lane's launches read route_kernel's lists: behind it on the device, whether or not the host waited for it)
        HIP_TRY(hipEventRecord(sl.side_go, sl.stream));
        HIP_TRY(hipStreamWaitEvent(side.stream, sl.side_go, 0));
        HIP_TRY(hipMemsetAsync(side.d_counter, 0, kCounterInts * sizeof(int), side.stream));
        // ... and the slot's own launches behind the side lane's reset: "started first" has to hold on the DEVICE.  With the
        // host no longer waiting for route_kernel the own lane's seed launch followed it at once, filled the machine, the own
        // main launch after it, and the side lane's blocks found room when that had ended: 31 + 14 ms one after the other.
        // Now both lanes' seed launches become eligible together and the side lane's stream has the higher priority.
        HIP_TRY(hipEventRecord(sl.side_go, side.stream));
        HIP_TRY(hipStreamWaitEvent(sl.stream, sl.side_go, 0));
        if ((rc = poison_lane(e, side, 0x1b873593u))) return rc;
        if ((rc = run_pass(c, side, true, sl.deferred.p + n, sl.d_counter + 5, routed[1], false))) return rc;
        HIP_TRY(hipEventRecord(sl.side_done, side.stream));
        sl.shape.side_used = true;
        rc = run_pass(c, own, false, sl.deferred.p, sl.d_counter + 4, routed[0], true);
        // (also when the own lane's pass could not be launched: the side lane's launches are under way and write this run's records)
        if (hipStreamWaitEvent(sl.stream, sl.side_done, 0) != hipSuccess && !rc) return fail(GACT_HIP_EDEVICE, "hipStreamWaitEvent failed");
        return rc;
    }
    if (routed[0] > 0 && (rc = run_pass(c, own, false, sl.deferred.p, sl.d_counter + 4, routed[0], true))) return rc;
    if (routed[1] == 0) return 0;
    if (routed[0] > 0) { int prc = poison_ws(e, sl, 0x1b873593u); if (prc) return prc; }
    // (behind a 2-bit pass on the same lane: the second set of queues, still empty)
    return run_pass(c, own, true, sl.deferred.p + n, sl.d_counter + 5, routed[1], routed[0] == 0, routed[0] > 0);
}
