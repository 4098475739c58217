// The path run and the summary run (gact_path.hpp, gact_summary.hpp): a second pass over selected candidates of a slot,
// through chain_kernel with a sink (included by gact_engine.hip behind gact_pass.hpp).
#pragma once

// The path run (gact_path.hpp).  The host takes the selected candidates (its copy of an uploaded list, else the device
// filter's list copied back), tags each with its strand (kCompInCand, as a merged run does), and cuts the selection into
// chunks whose column buffers fit the budget; per chunk: the chain kernel, the op count, the counts back, the scan on the host,
// the op write, the ops back.
int gact_hip_candidates_paths(gact_hip_engine *e, int slot, int32_t n_sel, const int32_t *sel, int32_t rc_from,
                              int same_file, gact_overlap *records, gact_path *paths,
                              uint32_t *ops, int64_t ops_cap, int64_t *ops_needed)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (n_sel < 0 || (n_sel > 0 && (!records || !paths)) || ops_cap < 0)
        return fail(GACT_HIP_EINVAL, "candidates_paths: bad arguments");
    if ((rc = refuse_big_tiles(e, "candidates_paths", "paths come from"))) return rc;
    Slot &sl = e->slots[slot];
    if (ops_needed) *ops_needed = 0;
    if (n_sel == 0) return 0;                 // (nothing asked for: also on a slot without candidates, e.g. a feeder with no reads)
    Selection sn;
    if ((rc = select_candidates(e, slot, n_sel, sel, rc_from, "candidates_paths", sn))) return rc;
    Slot::PathBufs &pb = sl.path;
    if ((rc = path_bufs_init(pb, "candidates_paths"))) return rc;
    pb.stats = gact_paths_stats{};
    pb.timed = false;
    if ((rc = pb.timer.start(sl.stream, "candidates_paths"))) return rc;
    int64_t total_ops = 0;
    bool room = ops != nullptr;
    std::vector<int64_t> col_off, op_off;
    std::vector<int32_t> n_cols, n_ops;
    for (int32_t first = 0; first < n_sel;) {
        int32_t end = first;
        int64_t bytes = 0;
        if ((rc = launch_path_chunk(e, sl, sn, first, n_sel, same_file, "candidates_paths", col_off, end, bytes))) return rc;
        const int32_t n = end - first;
        const int op_blocks = std::max(1, std::min((n + 3) / 4, 4096));
        hipLaunchKernelGGL(gact::path_ops_kernel<false>, dim3(op_blocks), dim3(256), 0, sl.stream, pb.cols.p, pb.col_off.p, pb.n_cols.p,
                           n, pb.n_ops.p, nullptr, nullptr);
        HIP_TRY(hipGetLastError());
        n_cols.resize(2 * (size_t)n);
        n_ops.resize((size_t)n);
        HIP_TRY(hipMemcpyAsync(records + first, pb.records.p, (size_t)n * sizeof(gact_overlap), hipMemcpyDeviceToHost, sl.stream));
        HIP_TRY(hipMemcpyAsync(n_cols.data(), pb.n_cols.p, 2 * (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
        HIP_TRY(hipMemcpyAsync(n_ops.data(), pb.n_ops.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
        HIP_TRY(hipStreamSynchronize(sl.stream));
        // ---- the exclusive scan of the counts, and the ops themselves where the caller has room for them
        op_off.resize((size_t)n);
        int64_t chunk_ops = 0;
        for (int32_t k = 0; k < n; k++) {
            op_off[(size_t)k] = chunk_ops;
            gact_path &p = paths[first + k];
            p.op_offset = total_ops + chunk_ops;
            p.n_ops = n_ops[(size_t)k];
            p.n_columns = n_cols[2 * (size_t)k] + n_cols[2 * (size_t)k + 1];
            chunk_ops += n_ops[(size_t)k];
        }
        room = room && total_ops + chunk_ops <= ops_cap;
        if (room && chunk_ops > 0) {
            if (pb.ops.reserve((size_t)chunk_ops)) return fail(GACT_HIP_ENOMEM, "candidates_paths: device allocation failed (%lld ops)", (long long)chunk_ops);
            if ((rc = poison_buf(e, pb.ops, sl.stream))) return rc;
            HIP_TRY(hipMemcpyAsync(pb.op_off.p, op_off.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, sl.stream));
            hipLaunchKernelGGL(gact::path_ops_kernel<true>, dim3(op_blocks), dim3(256), 0, sl.stream, pb.cols.p, pb.col_off.p, pb.n_cols.p,
                               n, nullptr, pb.op_off.p, pb.ops.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(ops + total_ops, pb.ops.p, (size_t)chunk_ops * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
            HIP_TRY(hipStreamSynchronize(sl.stream));
        }
        total_ops += chunk_ops;
        first = end;
        pb.stats.chunks++;
        pb.stats.column_bytes = std::max(pb.stats.column_bytes, bytes);
        for (int32_t k = 0; k < n; k++) pb.stats.columns += n_cols[2 * (size_t)k] + n_cols[2 * (size_t)k + 1];
    }
    if ((rc = pb.timer.stop(sl.stream, &pb.stats.device_ms))) return rc;
    pb.stats.ops = total_ops;
    pb.timed = true;
    if (ops_needed) *ops_needed = total_ops;
    if (!room && total_ops > 0)
        return fail(GACT_HIP_EINVAL, "candidates_paths: the ops need room for %lld words, ops_cap is %lld", (long long)total_ops,
                    (long long)ops_cap);
    return 0;
}

int gact_hip_last_paths_stats(gact_hip_engine *e, int slot, gact_paths_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::path, stats, "last_paths_stats", "has made no path run yet");
}

// The summary run (gact_summary.hpp): the same selection, one chain_kernel launch (CountSink) over all of it, records and summaries back.
int gact_hip_candidates_summaries(gact_hip_engine *e, int slot, int32_t n_sel, const int32_t *sel, int32_t rc_from,
                                  int same_file, gact_overlap *records, gact_path_summary *sums)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (n_sel < 0 || (n_sel > 0 && (!records || !sums)))
        return fail(GACT_HIP_EINVAL, "candidates_summaries: bad arguments");
    if ((rc = refuse_big_tiles(e, "candidates_summaries", "summaries come from"))) return rc;
    Slot &sl = e->slots[slot];
    if (n_sel == 0) return 0;                 // (as gact_hip_candidates_paths)
    Selection sn;
    if ((rc = select_candidates(e, slot, n_sel, sel, rc_from, "candidates_summaries", sn))) return rc;
    PassScratch<gact_summaries_stats> &sb = sl.summary;
    // candidates | records | summaries | pop counter: 16 + 56 + 32 bytes per candidate, each array 16-byte aligned
    const size_t n = (size_t)n_sel;
    const size_t at_records = n * sizeof(gact_candidate);
    const size_t at_sums = (at_records + n * sizeof(gact_overlap) + 15) & ~(size_t)15;
    const size_t at_counter = at_sums + n * sizeof(gact_path_summary);
    const size_t bytes = at_counter + 16;
    if (sb.reserve(bytes))
        return fail(GACT_HIP_ENOMEM, "candidates_summaries: device allocation failed (%d candidates, %zu bytes)", n_sel, bytes);
    gact_candidate *d_cands = (gact_candidate *)sb.p;
    gact_overlap *d_records = (gact_overlap *)(sb.p + at_records);
    gact_path_summary *d_sums = (gact_path_summary *)(sb.p + at_sums);
    int *d_counter = (int *)(sb.p + at_counter);
    if ((rc = sb.begin(sl.stream, "candidates_summaries"))) return rc;
    HIP_TRY(hipMemcpyAsync(d_cands, sn.tagged.data(), n * sizeof(gact_candidate), hipMemcpyHostToDevice, sl.stream));
    // (a chain with no tile over the threshold never walks: its summary stays zero; the counter starts at zero)
    HIP_TRY(hipMemsetAsync(d_sums, 0, n * sizeof(gact_path_summary) + 16, sl.stream));
    if ((rc = launch_chain_kernel(e, sl, sn, d_cands, n_sel, same_file, d_records, d_counter, gact::CountSink{d_sums}))) return rc;
    HIP_TRY(hipMemcpyAsync(records, d_records, n * sizeof(gact_overlap), hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipMemcpyAsync(sums, d_sums, n * sizeof(gact_path_summary), hipMemcpyDeviceToHost, sl.stream));
    if ((rc = sb.end(sl.stream))) return rc;
    sb.stats.launches = 1;
    sb.stats.scratch_bytes = (int64_t)sb.bytes;
    return 0;
}

int gact_hip_last_summaries_stats(gact_hip_engine *e, int slot, gact_summaries_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::summary, stats, "last_summaries_stats", "has made no summary run yet");
}
