// What the passes behind an alignment run share on the host (included by gact_engine.hip; host code only, no kernel).
//
// A pass runs on a slot's stream behind the slot's last run: CIGAR paths and summaries (gact_path_run.hpp), selection
// (gact_select.hpp), the filter by identity, span and each read's best (gact_filter.hpp), coverage (gact_cover.hpp), the
// overlap graph (gact_graph.hpp), its unitigs (gact_unitig.hpp), its bubbles
// (gact_bubble.hpp), its weak arcs and cleaning rounds (gact_clean.hpp), the placement of reads (gact_place.hpp), the pileup (gact_pileup.hpp) and its variants (gact_variants.hpp).  A new pass starts here.  It takes a PassScratch<its stats> in Slot (gact_engine.hip, beside DevBuf: Slot holds them by value, so
// the two records are defined in front of it), and its entry point reads:
//
//     the refusals that need no device (slot_records_check for "records of the slot or of the caller")
//     the early returns for an empty input
//     const size_t at_x = up16(...), ..., bytes = ...;      // the layout, documented where it is written
//     if (ps.reserve(bytes)) return fail(GACT_HIP_ENOMEM, "...", ...);
//     if ((rc = ps.begin(sl.stream, "who"))) return rc;      // stats zeroed, ev0 recorded
//     the copies in (slot_records_stage), the kernels, the copies out
//     if ((rc = ps.end(sl.stream))) return rc;               // ev1 recorded and waited for, stats.device_ms read once
//     the other figures of ps.stats, then any "room" refusal
//
// and its gact_hip_last_*_stats is one call of last_pass_stats.  Its kernels start from gact_pass_device.hpp: kPassBlock
// threads a block (the grids: lane_blocks, wave_blocks, full_device_blocks below), offsets by block_scan_step, a best-of-key table by
// table_insert_best / table_find, counters by wave_count.
//
// A pass on an arc graph (n_reads, read_lens, clip, reads, n_arcs, arcs[, skip]: unitigs, bubbles, weak arcs, the cleaning
// rounds) starts from the host part of gact_unitig.hpp, behind the kernels it launches.  Its entry point reads:
//
//     its own NULL list and parameter checks, then check_arc_graph (the bounds, the arcs, the lengths and clips)
//     ArcGraphDev g = arc_graph_layout(...);                 // arcs | reads | lens | clip | skip; its own ladder starts at g.end
//     arc_graph_begin(g, ps, bytes, ...): reserve, begin and the copies in; then the memset of its zeroed block
//     arc_graph_index(g, want_bases, first, out, counters, flag);   // the stretches and the arc checks; g keeps first and flag
//     its steps (unitig_sweep, bubble_step, prune_step, or kernels of its own that return at once when *flag is set)
//     arc_graph_fetch(g, who, ...): the wait, the counters, and arc_graph_refusal's one wording of what the check kernel refused
#pragma once

extern "C++" {                  // (templates: not in gact_engine.hip's extern "C")

// gact_hip_last_*_stats of a slot's pass: `pass` is the Slot member that holds `stats` and `timed`, none_yet the pass's own phrase
template <class Pass, class Stats>
static int last_pass_stats(gact_hip_engine *e, int slot, Pass Slot::*pass, Stats *stats, const char *who, const char *none_yet)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (!stats) return fail(GACT_HIP_EINVAL, "%s: NULL argument", who);
    const Pass &ps = e->slots[slot].*pass;
    if (!ps.timed) return fail(GACT_HIP_EINVAL, "%s: slot %d %s", who, slot, none_yet);
    *stats = ps.stats;
    return 0;
}

// The grids: of a kernel with one lane per item (at least one block); the blocks that fill the device for a grid-stride
// kernel, eight waves on every SIMD; and of a grid-stride kernel with one wave per item, the blocks that hold the items, at
// most the ones that fill the device
static dim3 lane_blocks(size_t lanes)
{
    return dim3((unsigned)((std::max(lanes, (size_t)1) + gact::kPassBlock - 1) / gact::kPassBlock));
}
static size_t full_device_blocks(const gact_hip_engine *e)
{
    return (size_t)std::max(1, e->prop.multiProcessorCount) * 8;
}
static dim3 wave_blocks(const gact_hip_engine *e, size_t items)
{
    return dim3((unsigned)std::min((std::max(items, (size_t)1) + gact::kPassWaves - 1) / gact::kPassWaves, full_device_blocks(e)));
}

// the lengths and, where given, the clips of a pass's n_reads reads (graph, unitigs) -> the clipped total, or the refusal's code (< 0)
static int64_t check_read_lens(const char *who, int32_t n_reads, const int32_t *read_lens, const int32_t *clip)
{
    int64_t clipped = 0;
    for (int32_t i = 0; i < n_reads; i++) {
        if (read_lens[i] < 0) return fail(GACT_HIP_EINVAL, "%s: read %d has the negative length %d", who, i, read_lens[i]);
        if (clip && !(0 <= clip[2 * (size_t)i] && clip[2 * (size_t)i] <= clip[2 * (size_t)i + 1] && clip[2 * (size_t)i + 1] <= read_lens[i]))
            return fail(GACT_HIP_EINVAL, "%s: the clip [%d, %d) of read %d is not inside [0, %d]", who, clip[2 * (size_t)i],
                        clip[2 * (size_t)i + 1], i, read_lens[i]);
        clipped += clip ? clip[2 * (size_t)i + 1] - clip[2 * (size_t)i] : read_lens[i];
    }
    return clipped;
}

// "Records of the slot or of the caller" (select, cover, graph).  records == NULL: records [0, n) of the slot's device array,
// behind the slot's last run (stream order); else the caller's n records, which slot_records_stage copies to the front of the
// pass's scratch.  The check: the slot has that many.
static int slot_records_check(const Slot &sl, int slot, int32_t n, const gact_overlap *records, const char *who)
{
    if (n <= 0 || records) return 0;
    if (sl.n_cands == 0 || !sl.overlaps.p)
        return fail(GACT_HIP_EINVAL, "%s: slot %d holds no records (run its candidates first, or pass records)", who, slot);
    if ((size_t)n > sl.n_cands || (size_t)n > sl.overlaps.cap)
        return fail(GACT_HIP_EINVAL, "%s: n = %d beyond the %zu records of slot %d", who, n, sl.n_cands, slot);
    return 0;
}

// ... and the inputs on the device: the scratch p begins records (the caller's only) | sel | sums | <the pass's own>, each
// 16-byte aligned; with no record chosen nothing is copied (no kernel reads them then).
struct DevRecords {
    const gact_overlap *rec;
    const int *sel;                           // NULL where the caller passed none: all n records
    const gact_path_summary *sums;            // NULL likewise
};
static int slot_records_stage(const Slot &sl, uint8_t *p, int32_t n, const gact_overlap *records, int32_t n_chosen, const int32_t *sel,
                              size_t at_sel, const gact_path_summary *sums, size_t at_sums, DevRecords &d)
{
    d.rec = sl.overlaps.p;
    d.sel = sel ? (const int *)(p + at_sel) : nullptr;
    d.sums = sums ? (const gact_path_summary *)(p + at_sums) : nullptr;
    if (n_chosen <= 0) return 0;
    if (records) {
        HIP_TRY(hipMemcpyAsync(p, records, (size_t)n * sizeof(gact_overlap), hipMemcpyHostToDevice, sl.stream));
        d.rec = (const gact_overlap *)p;
    }
    if (sel) HIP_TRY(hipMemcpyAsync(p + at_sel, sel, (size_t)n_chosen * sizeof(int32_t), hipMemcpyHostToDevice, sl.stream));
    if (sums) HIP_TRY(hipMemcpyAsync(p + at_sums, sums, (size_t)n_chosen * sizeof(gact_path_summary), hipMemcpyHostToDevice, sl.stream));
    return 0;
}

// the passes that walk alignments again (paths, summaries, pileup) need the register-tiled chain kernel; `what` says what
// of theirs comes from it
static int refuse_big_tiles(const gact_hip_engine *e, const char *who, const char *what)
{
    if (!e->big_cb) return 0;
    return fail(GACT_HIP_EINVAL, "%s: tile_size %d > GACT_HIP_FAST_TILE (%d): %s the register-tiled int32 chain kernel, which the "
                                 "tiles of gact_big.hpp do not run on", who, e->params.tile_size, GACT_HIP_FAST_TILE, what);
}

// The selection of a path run or a summary run (`who` names the entry in the refusals): the selected candidates as the host
// sees them (its copy of an uploaded list, else the device filter's list copied back), each tagged with its strand
// (kCompInCand, as a merged run does), the reads' lengths, and the read sets the chains are to read.
struct Selection {
    std::vector<gact_candidate> tagged;
    std::vector<int64_t> cap;                 // ref_len + query_len of each: every column consumes a base of one of the two reads
    gact::SeqSetDev d_rs, d_qf, d_qr;
};
static int select_candidates(gact_hip_engine *e, int slot, int32_t n_sel, const int32_t *sel, int32_t rc_from, const char *who,
                             Selection &sn)
{
    int rc;
    Slot &sl = e->slots[slot];
    if (sl.n_cands == 0)
        return fail(GACT_HIP_EINVAL, "%s: slot %d holds no candidates (upload a list or run the device filter first)", who, slot);
    for (int32_t k = 0; k < n_sel; k++) {
        const int64_t idx = sel ? sel[k] : k;
        if (idx < 0 || (size_t)idx >= sl.n_cands)
            return fail(GACT_HIP_EINVAL, "%s: sel[%d] = %lld outside the %zu candidates of slot %d", who, k, (long long)idx,
                        sl.n_cands, slot);
    }
    if ((rc = set_device(e))) return rc;
    const SeqSet &rs = e->sets[GACT_SET_REF];
    const SeqSet &qf = e->sets[GACT_SET_QUERY], &qr = e->sets[GACT_SET_QUERY_RC];
    // the candidates as the host sees them
    std::vector<gact_candidate> downloaded;
    const gact_candidate *hc = sl.h_cands.data();
    if (sl.h_cands.empty()) {
        if (sl.cands_epoch != e->sets_epoch)
            return fail(GACT_HIP_EINVAL, "%s: a read set was uploaded after the device filter made this slot's "
                                         "candidates; run gact_hip_dsoft_query again", who);
        downloaded.resize(sl.n_cands);
        HIP_TRY(hipMemcpyAsync(downloaded.data(), sl.cands.p, sl.n_cands * sizeof(gact_candidate), hipMemcpyDeviceToHost, sl.stream));
        HIP_TRY(hipStreamSynchronize(sl.stream));
        hc = downloaded.data();
    }
    // strands, lengths, checks
    sn.tagged.resize((size_t)n_sel);
    sn.cap.resize((size_t)n_sel);
    bool need_f = false, need_r = false;
    for (int32_t k = 0; k < n_sel; k++) {
        const int32_t idx = sel ? sel[k] : k;
        gact_candidate c = hc[idx];
        const bool comp = idx >= rc_from;
        const SeqSet &qs = comp ? qr : qf;
        (comp ? need_r : need_f) = true;
        if (rs.n == 0 || qs.n == 0) return fail(GACT_HIP_EINVAL, "%s: read sets not uploaded", who);
        if (c.ref_id < 0 || c.ref_id >= rs.n || c.query_id < 0 || c.query_id >= qs.n)
            return fail(GACT_HIP_ERANGE, "candidate %d: sequence id out of range", idx);
        const int64_t rl = rs.h_offsets[c.ref_id + 1] - rs.h_offsets[c.ref_id];
        const int64_t ql = qs.h_offsets[c.query_id + 1] - qs.h_offsets[c.query_id];
        if (c.ref_pos < 0 || c.ref_pos > rl || c.query_pos < 0 || c.query_pos > ql)
            return fail(GACT_HIP_ERANGE, "candidate %d: position outside its read", idx);
        if (comp) c.query_id |= gact::kCompBit;
        sn.tagged[(size_t)k] = c;
        sn.cap[(size_t)k] = rl + ql;
    }
    const bool raw = rs.has_other || (need_f && qf.has_other) || (need_r && qr.has_other);
    sn.d_rs = rs.dev(raw); sn.d_qf = qf.dev_or(raw, rs); sn.d_qr = qr.dev_or(raw, rs);
    return 0;
}

// GACT_HIP_POISON_SCRATCH over a DevBuf: all `cap` elements
template <class T> static int poison_buf(gact_hip_engine *e, DevBuf<T> &b, hipStream_t stream)
{
    return poison_scratch(e, b.p, b.cap * sizeof(T), stream);
}

// the path run's pop counter and events, made on the slot's first path run or pileup add
static int path_bufs_init(Slot::PathBufs &pb, const char *who)
{
    if (!pb.d_counter && hipMalloc((void **)&pb.d_counter, sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GACT_HIP_ENOMEM, "%s: device allocation failed", who);
    }
    return pb.timer.create(who);
}

// where the chunk of a path run that starts at candidate `first` ends: as many candidates as the budget's column bytes hold,
// at least one; bytes: their column bytes
static int32_t path_chunk_end(const gact_hip_engine *e, const std::vector<int64_t> &cap, int32_t first, int32_t n_sel, int64_t &bytes)
{
    int32_t end = first;
    bytes = 0;
    while (end < n_sel && (end == first || bytes + cap[(size_t)end] <= e->path_budget)) bytes += cap[(size_t)end++];
    return end;
}

// One launch of chain_kernel for a second pass over a selection (the path run's chunks, the summary run): candidates
// d_cands[0, n), tagged with their strands, popped through *d_counter (zeroed by the caller) into the sink.
template <class Sink>
static int launch_chain_kernel(gact_hip_engine *e, Slot &sl, const Selection &sn, const gact_candidate *d_cands, int n, int same_file,
                               gact_overlap *d_records, int *d_counter, Sink sink)
{
    gact::ChainQueues q{};
    q.pop_seed = d_counter;
    q.list_n = -1;
    const int groups_per_block = (gact::kBlockThreads / 64) * gact::kGroupsPerWave;
    // (the slot's workspace is sized for grid_blocks blocks of the chain kernels)
    const int blocks = std::max(1, std::min((n + groups_per_block - 1) / groups_per_block, e->grid_blocks));
    auto k = e->C == 20 ? gact::chain_kernel<20, Sink> : gact::chain_kernel<32, Sink>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(gact::kBlockThreads), 0, sl.stream, e->kp, sn.d_rs, sn.d_qf, sn.d_qr, d_cands, n,
                       gact::kCompInCand, same_file, d_records, q, sink, sl.d_ws);
    HIP_TRY(hipGetLastError());
    return 0;
}

// One chunk of a path run (gact_hip_candidates_paths, gact_hip_pileup_add): candidates [first, end) of the selection, as many
// as the budget's column bytes hold (at least one), their tagged copies, column offsets and zeroed column counts on the
// device, and chain_kernel with a ColumnSink behind them on the slot's stream.  pb.d_counter is the caller's to have made.
static int launch_path_chunk(gact_hip_engine *e, Slot &sl, const Selection &sn, int32_t first, int32_t n_sel, int same_file,
                             const char *who, std::vector<int64_t> &col_off, int32_t &end, int64_t &bytes)
{
    Slot::PathBufs &pb = sl.path;
    const std::vector<int64_t> &cap = sn.cap;
    end = path_chunk_end(e, cap, first, n_sel, bytes);
    const int32_t n = end - first;
    col_off.assign((size_t)n + 1, 0);
    for (int32_t k = 0; k < n; k++) col_off[(size_t)k + 1] = col_off[(size_t)k] + cap[(size_t)(first + k)];
    if (pb.cands.reserve((size_t)n) || pb.records.reserve((size_t)n) || pb.col_off.reserve((size_t)n + 1) ||
        pb.op_off.reserve((size_t)n) || pb.n_cols.reserve(2 * (size_t)n) || pb.n_ops.reserve((size_t)n) ||
        pb.cols.reserve((size_t)bytes + 64))
        return fail(GACT_HIP_ENOMEM, "%s: device allocation failed (%d candidates, %lld column bytes)", who, n, (long long)bytes);
    // GACT_HIP_POISON_SCRATCH: every array of the chunk, whole, in front of its copies and memsets.  A pileup add queues this
    // chunk while the one before may still run: its chain kernel and its pileup kernel were launched on sl.stream, as the fills
    // are, so they have read these arrays before a fill writes them (and pileup_add reserves them once, before its first chunk).
    if (e->scratch_poison.seed) {
        int rc;
        if ((rc = poison_buf(e, pb.cands, sl.stream)) || (rc = poison_buf(e, pb.records, sl.stream)) ||
            (rc = poison_buf(e, pb.col_off, sl.stream)) || (rc = poison_buf(e, pb.op_off, sl.stream)) ||
            (rc = poison_buf(e, pb.n_cols, sl.stream)) || (rc = poison_buf(e, pb.n_ops, sl.stream)) ||
            (rc = poison_buf(e, pb.cols, sl.stream)))
            return rc;
    }
    HIP_TRY(hipMemcpyAsync(pb.cands.p, sn.tagged.data() + first, (size_t)n * sizeof(gact_candidate), hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemcpyAsync(pb.col_off.p, col_off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemsetAsync(pb.n_cols.p, 0, 2 * (size_t)n * sizeof(int32_t), sl.stream));
    HIP_TRY(hipMemsetAsync(pb.d_counter, 0, sizeof(int), sl.stream));
    return launch_chain_kernel(e, sl, sn, pb.cands.p, n, same_file, pb.records.p, pb.d_counter,
                               gact::ColumnSink{{pb.cols.p, pb.col_off.p, pb.n_cols.p}});
}

}  // extern "C++"
