// gact_cover.hpp -- per-read coverage of an overlap set, computed on the device (gact_hip_read_coverage).
//
// What a consumer of an all-vs-all overlap set computes first: how deep every read is covered by the other reads, and which
// stretch of it is covered at least min_depth deep (miniasm clips the rest as adapter or chimera); for reads against contigs,
// the depth the reads give each contig.  The records of a run are on the device already, and so are the indices of
// gact_hip_select_overlaps and the summaries of gact_hip_candidates_summaries; the rule is stated in include/gact_hip.h.
//
// One scatter of interval ends and one scan per read, on the slot's stream, nothing on the host between them:
//   0 the host makes off[i] = sum(len[< i]) + i (int64, n_reads + 1 of them): every read has one slot more than it has
//     positions, and that slot takes the -1 of an interval that ends at the read's end -- no branch, nothing leaks into the
//     next read.  The difference array (int32, sum(len) + n_reads entries), the results and the error flag are zeroed by one
//     hipMemsetAsync.
//   1 cover_mark_kernel    one lane per chosen record: its interval on the ref side and / or the query side (mapped to the
//                          read's own strand, begins moved by the summary where one is given), clipped to the read;
//                          atomicAdd(+1) at the begin, atomicAdd(-1) at the end, atomicAdd(+1) into the read's n_intervals.
//                          Ordinary vector global atomics on integers: the sums are the same in whichever order they land.
//                          A sel index outside [0, n) or a read id outside [0, n_reads) sets a bit of one flag word, which the
//                          host reads before it copies anything out.
//   2 cover_sweep_kernel   one wave per read, grid-stride over the reads; the wave walks its read 64 positions at a time:
//                          a coalesced load of the differences (the next chunk's is issued before this one is worked on), an
//                          inclusive wave scan plus the carry of the chunk before = the depth, the optional store of the depth,
//                          a per-lane running max and 64-bit running sum (reduced once at the end), covered / well_covered
//                          from the popcounts of two ballots, and the longest run from the depth >= min_depth ballot, walked
//                          run by run with wave-uniform bit operations.  A run that is open at a chunk's end is carried on as
//                          its begin; a run replaces the best one only when strictly longer, so the leftmost of equal runs
//                          stays; invalid lanes of the last chunk load nothing and set no ballot bit.  Lane 0 writes the
//                          32-byte result as two 16-byte vectors (n_intervals goes back as it was read, so the compiler
//                          stores the 28 bytes behind it: a 16-byte and a 12-byte store).
// No lane waits for another wave, no look-back, no spinning; no LDS.  All results are integers and the same on every call.
//
// The depth goes to an array of its own (sum(len) int32, only when asked for) and not over the differences: read i's compact
// positions start at off[i] - i, inside the difference slots of the reads before it, which other waves may not have read yet.
//
// Known limit: one wave per sequence is right for reads (kilobases).  A chromosome-length sequence on the ref side is swept by
// one wave, 64 positions per step: correct, and slow.
//
// Included by gact_engine.hip behind every other kernel and behind the engine's definitions (Slot, fail, HIP_TRY), inside its
// extern "C" block, as gact_select.hpp is.
#pragma once

namespace gact {

constexpr int32_t kCoverMaxRecords = 1 << 30;
constexpr int32_t kCoverMaxLength = 0x7fffffff - 64;    // (the sweep's chunk begin stays an int32 one step past the end)
constexpr int kCoverBadIndex = 1, kCoverBadRead = 2;    // bits of the flag word

// the interval [b, e) on read `id`: clipped, counted, marked.  false: the id is outside [0, n_reads)
__device__ inline bool cover_mark(long long b, long long e, int id, bool mirror, int n_reads, const long long *__restrict__ off,
                                  int *diff, gact_read_cover *cover)
{
    if (id < 0 || id >= n_reads) return false;
    const long long base = off[id], len = off[id + 1] - base - 1;
    if (mirror) { const long long t = b; b = len - e; e = len - t; }       // the reverse-complement strand's [b, e) on the read itself
    if (b < 0) b = 0;
    if (e > len) e = len;
    if (b >= e) return true;
    atomicAdd(&diff[base + b], 1);
    atomicAdd(&diff[base + e], -1);
    atomicAdd(&cover[id].n_intervals, 1);
    return true;
}

__global__ void __launch_bounds__(kPassBlock)
cover_mark_kernel(const gact_overlap *__restrict__ rec, int n, const int *__restrict__ sel, int n_chosen,
                  const gact_path_summary *__restrict__ sums, int sides, int n_reads, const long long *__restrict__ off,
                  int *diff, gact_read_cover *cover, int *flag)
{
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    if (k >= n_chosen) return;
    const int i = sel ? sel[k] : k;
    if (i < 0 || i >= n) { atomicOr(flag, kCoverBadIndex); return; }
    const gact_overlap r = rec[i];
    if (!r.emitted) return;
    long long ab = r.ab, bb = r.bb;
    if (sums) begins_from_summary(r, sums[k], ab, bb);
    bool ok = true;
    if (sides & GACT_COVER_REF) ok = cover_mark(ab, r.ae, r.ref_id, false, n_reads, off, diff, cover);
    if (sides & GACT_COVER_QUERY) ok = cover_mark(bb, r.be, r.query_id, r.comp != 0, n_reads, off, diff, cover) && ok;
    if (!ok) atomicOr(flag, kCoverBadRead);
}

__global__ void __launch_bounds__(kPassBlock)
cover_sweep_kernel(int n_reads, const long long *__restrict__ off, const int *__restrict__ diff, int min_depth,
                   gact_read_cover *__restrict__ cover, int *__restrict__ depth_out)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (kPassBlock / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (kPassBlock / 64);
    for (int read = wave; read < n_reads; read += n_waves) {
        const long long base = off[read];
        const int len = (int)(off[read + 1] - base - 1);
        const int *d = diff + base;
        int *out = depth_out ? depth_out + (base - read) : nullptr;
        int carry = 0, lane_max = 0, covered = 0, well = 0;
        long long lane_sum = 0;
        int open = -1, best_b = 0, best_e = 0;            // the run that is open at the chunk's begin (-1: none), the best one
        int next = lane < len ? d[lane] : 0;
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int p = c0 + lane;
            const bool valid = p < len;
            const int x = next;
            next = p < len - 64 ? d[p + 64] : 0;
            const int depth = carry + wave_scan(x, lane); // (an invalid lane adds 0: the depth of the read's last position)
            carry = __shfl(depth, 63);
            if (valid) {
                if (out) out[p] = depth;
                lane_max = max(lane_max, depth);
                lane_sum += depth;
            }
            covered += __popcll(__ballot(valid && depth >= 1));
            const unsigned long long m = __ballot(valid && depth >= min_depth);
            well += __popcll(m);
            // the runs of m, left to right; `at` < 64 throughout: a bit is found below bit 64 - at of a word shifted by at
            int at = 0;
            for (;;) {
                if (open < 0) {
                    const unsigned long long rest = m >> at;
                    if (!rest) break;
                    at += __ffsll(rest) - 1;
                    open = c0 + at;
                }
                const unsigned long long gaps = ~m >> at;
                if (!gaps) break;                         // set up to bit 63: the run stays open
                at += __ffsll(gaps) - 1;
                if (c0 + at - open > best_e - best_b) { best_b = open; best_e = c0 + at; }
                open = -1;
            }
        }
        if (open >= 0 && len - open > best_e - best_b) { best_b = open; best_e = len; }
        for (int o = 32; o > 0; o >>= 1) {
            lane_max = max(lane_max, __shfl_xor(lane_max, o));
            lane_sum += __shfl_xor(lane_sum, o);
        }
        if (lane == 0) {
            int4 *c = (int4 *)&cover[read];
            const int n_intervals = cover[read].n_intervals;          // cover_mark_kernel's count, a launch ago
            c[0] = make_int4(n_intervals, lane_max, covered, well);
            c[1] = make_int4(best_b, best_e, (int)(unsigned)(lane_sum & 0xffffffffll), (int)(lane_sum >> 32));
        }
    }
}

}  // namespace gact

// One allocation: records (host ones only) | sel | sums | off (8 (n_reads + 1)) | cover (32 n_reads) | flag | differences
// (4 (sum(len) + n_reads)) | depth (4 sum(len), only when asked for).  cover | flag | differences are zeroed together.
int gact_hip_read_coverage(gact_hip_engine *e, int slot, int32_t n, const gact_overlap *records, int32_t n_sel, const int32_t *sel,
                           const gact_path_summary *sums, int32_t sides, int32_t min_depth, int32_t n_reads,
                           const int32_t *read_lens, gact_read_cover *cover, int32_t *depth)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (min_depth < 1) return fail(GACT_HIP_EINVAL, "read_coverage: min_depth = %d, at least 1", min_depth);
    if (sides != GACT_COVER_REF && sides != GACT_COVER_QUERY && sides != GACT_COVER_BOTH)
        return fail(GACT_HIP_EINVAL, "read_coverage: unknown sides %d (GACT_COVER_REF 1, GACT_COVER_QUERY 2, GACT_COVER_BOTH 3)", sides);
    if (n < 0 || n > gact::kCoverMaxRecords || n_reads < 0 || (sel && n_sel < 0))
        return fail(GACT_HIP_EINVAL, "read_coverage: bad arguments (n = %d, at most %d; n_reads = %d; n_sel = %d)", n,
                    gact::kCoverMaxRecords, n_reads, n_sel);
    if (n_reads > 0 && (!read_lens || !cover)) return fail(GACT_HIP_EINVAL, "read_coverage: read_lens or cover is NULL");
    std::vector<long long> off((size_t)n_reads + 1);
    long long positions = 0;
    for (int32_t i = 0; i < n_reads; i++) {
        if (read_lens[i] < 0) return fail(GACT_HIP_EINVAL, "read_coverage: read %d has the negative length %d", i, read_lens[i]);
        if (read_lens[i] > gact::kCoverMaxLength)
            return fail(GACT_HIP_EINVAL, "read_coverage: read %d has length %d, at most %d", i, read_lens[i], gact::kCoverMaxLength);
        off[(size_t)i] = positions + i;
        positions += read_lens[i];
    }
    off[(size_t)n_reads] = positions + n_reads;
    Slot &sl = e->slots[slot];
    if ((rc = slot_records_check(sl, slot, n, records, "read_coverage"))) return rc;
    if (n_reads == 0) return 0;
    const int32_t n_chosen = n == 0 ? 0 : sel ? n_sel : n;
    if ((rc = set_device(e))) return rc;
    PassScratch<gact_cover_stats> &cb = sl.cover;
    const size_t n_diff = (size_t)positions + (size_t)n_reads;
    const size_t at_sel = records ? up16((size_t)n * sizeof(gact_overlap)) : 0;
    const size_t at_sums = up16(at_sel + (sel ? (size_t)n_chosen * sizeof(int32_t) : 0));
    const size_t at_off = up16(at_sums + (sums ? (size_t)n_chosen * sizeof(gact_path_summary) : 0));
    const size_t at_cover = up16(at_off + off.size() * sizeof(long long));
    const size_t at_flag = at_cover + (size_t)n_reads * sizeof(gact_read_cover);
    const size_t at_diff = at_flag + 16;
    const size_t at_depth = up16(at_diff + n_diff * sizeof(int32_t));
    const size_t bytes = at_depth + (depth ? (size_t)positions * sizeof(int32_t) : 0);
    if (cb.reserve(bytes))
        return fail(GACT_HIP_ENOMEM, "read_coverage: device allocation failed (%d reads, %lld positions, %zu bytes)", n_reads,
                    positions, bytes);
    long long *d_off = (long long *)(cb.p + at_off);
    gact_read_cover *d_cover = (gact_read_cover *)(cb.p + at_cover);
    int *d_flag = (int *)(cb.p + at_flag), *d_diff = (int *)(cb.p + at_diff);
    int *d_depth = depth ? (int *)(cb.p + at_depth) : nullptr;
    if ((rc = cb.begin(sl.stream, "read_coverage"))) return rc;
    DevRecords in;
    if ((rc = slot_records_stage(sl, cb.p, n, records, n_chosen, sel, at_sel, sums, at_sums, in))) return rc;
    const gact_overlap *d_rec = in.rec;
    const int *d_sel = in.sel;
    const gact_path_summary *d_sums = in.sums;
    HIP_TRY(hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, sl.stream));
    HIP_TRY(hipMemsetAsync(d_cover, 0, at_diff + n_diff * sizeof(int32_t) - at_cover, sl.stream));
    if (n_chosen > 0)
        hipLaunchKernelGGL(gact::cover_mark_kernel, lane_blocks((size_t)n_chosen), dim3(gact::kPassBlock), 0, sl.stream, d_rec, n, d_sel,
                           n_chosen, d_sums, sides, n_reads, d_off, d_diff, d_cover, d_flag);
    hipLaunchKernelGGL(gact::cover_sweep_kernel, wave_blocks(e, (size_t)n_reads), dim3(gact::kPassBlock), 0, sl.stream, n_reads, d_off,
                       d_diff, min_depth, d_cover, d_depth);
    HIP_TRY(hipGetLastError());
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, sl.stream));
    HIP_TRY(hipStreamSynchronize(sl.stream));
    if (flag & gact::kCoverBadIndex)
        return fail(GACT_HIP_EINVAL, "read_coverage: sel holds an index outside [0, %d)", n);
    if (flag)
        return fail(GACT_HIP_ERANGE, "read_coverage: a counted record names a read outside [0, %d) on a requested side", n_reads);
    HIP_TRY(hipMemcpyAsync(cover, d_cover, (size_t)n_reads * sizeof(gact_read_cover), hipMemcpyDeviceToHost, sl.stream));
    if (depth && positions > 0)
        HIP_TRY(hipMemcpyAsync(depth, d_depth, (size_t)positions * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
    if ((rc = cb.end(sl.stream))) return rc;
    cb.stats.reads = n_reads;
    for (int32_t i = 0; i < n_reads; i++) cb.stats.intervals += cover[i].n_intervals;
    cb.stats.positions = positions;
    cb.stats.scratch_bytes = (int64_t)cb.bytes;
    return 0;
}

int gact_hip_last_cover_stats(gact_hip_engine *e, int slot, gact_cover_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::cover, stats, "last_cover_stats", "has taken no coverage yet");
}
