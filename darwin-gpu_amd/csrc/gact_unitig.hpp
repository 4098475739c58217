// gact_unitig.hpp -- the unitigs of an overlap graph, made on the device (gact_hip_unitigs).
//
// What an assembler's layout stage does with the arcs gact_hip_overlap_graph kept: cut the short dead ends, walk the
// unambiguous paths, spell one sequence per path.  The rule is stated in include/gact_hip.h and restated in
// tests/unitig_model.py.  The new ground is list ranking: weighted pointer jumping over a bidirected graph, with cycles.
//
// The kernels, all on the slot's stream, nothing on the host between them; the launch counts follow from 2 n_reads alone:
//   unitig_first_kernel    one lane per vertex: where its stretch of the sorted arc array begins (a lower bound on u; in range
//                          whatever the array holds)
//   unitig_check_kernel    one lane per arc: range, order against the arc in front of it, and for an arc with flags == 0 (E0)
//                          that both reads are live and that its complement v^1 -> u^1 is an E0 arc of v^1's stretch;
//                          atomicOr into a flag word, atomicAdd into out[u] for E0.  EVERY LATER KERNEL RETURNS AT ONCE WHEN THE
//                          FLAG WORD IS SET, so none of them indexes with a vertex that was not checked
//   unitig_links_kernel    one lane per arc of the current set: a join u -> v (out(u) == 1 and out(v^1) == 1) writes prev[v],
//                          the length into v's in-cell and u's out-cell: distinct cells, no atomics
//   unitig_init_kernel     one lane per vertex: its ranking record (below), pointing at prev or, for a head, at itself.  On the
//                          third sweep it first opens the cycles the second sweep found
//   unitig_jump_kernel     one round of pointer jumping, ONE LAUNCH THAT READS ONE BUFFER AND WRITES THE OTHER:
//                          rec[x] += rec[rec[x].ptr]; ceil(log2(2 n_reads)) rounds a sweep.  A head points at itself with
//                          zero weights, so jumping over it changes nothing and no round needs a condition; a vertex whose
//                          pointer is not a head after the rounds is on a cycle, and its minima are the whole cycle's
//   unitig_tip_kernel      one lane per read, behind the first sweep (E0): the chain of vertex 2 i is linear, has
//                          c = rank[x] + rank[x^1] + 1 <= tip_reads reads, head h = ptr[x], tail t = ptr[x^1]^1, and
//                          out(h^1) == 0 or out(t) == 0: the read is cut
//   unitig_recount_kernel  one lane per arc: the out-degrees of E1 = E0 without the arcs that touch a cut read
//   unitig_heads_kernel    one lane per vertex: an emitted head (x == ptr[x] < ptr[x^1]) leaves 1, its read count and its length
//                          (through its tail's record), every other vertex zeros; the longest and the circular ones counted
//   unitig_scan_kernel     one block, in place (block_scan_step): the exclusive scans of the three over the vertex ids, and
//                          their totals
//   unitig_fill_kernel     one lane per vertex: the entry and the place of a vertex of an emitted chain, the gact_unitig by the
//                          tail's lane, the place of a read that is not placed by its even vertex's lane
//   unitig_bases_kernel    one wave per layout entry, grid-stride; lanes stride over the entry's take: a forward entry reads
//                          ascending addresses, a reverse one descending addresses, both write ascending ones: coalesced on
//                          both sides, one byte per lane and step
// Three sweeps (unitig_sweep: links, init, the jumps): on E0 for the tip rule, on E1 to find the cycles and their lowest ids, and on
// E1 with the cycles opened.  first and check are arc_graph_index: what every pass on an arc graph starts with.
// Ordinary vector global atomics on integers; every value they leave is the same in whichever order they land.  No LDS but
// the scan's, no spinning on other waves, no cooperative grid.
//
// Included by gact_engine.hip behind every other kernel and behind the engine's definitions, inside its extern "C" block.
#pragma once

namespace gact {

constexpr int32_t kUnitigMaxReads = 1 << 30;               // (a vertex 2 i + 1 fits an int32)
constexpr int64_t kUnitigMaxArcs = 1 << 29;
// bits of the flag word (worded by arc_graph_refusal, below the kernels)
constexpr int kUnitigBadRange = 1, kUnitigBadOrder = 2, kUnitigNotLive = 4, kUnitigNoComplement = 8, kUnitigLongArc = 16;
// the counters
constexpr int kUnitigE0 = 0, kUnitigE1 = 1, kUnitigJoins = 2, kUnitigCut = 3, kUnitigContained = 4, kUnitigCircular = 5,
              kUnitigLongestReads = 6, kUnitigLongestBases = 7, kUnitigCounters = 8;

// what a vertex knows after some rounds: ptr is 2^rounds joins towards the head (or the head), n_joins and bases the joins and
// their lengths crossed on the way, low / low_c the lowest vertex id and the lowest complemented id among itself and the vertices
// jumped over (ptr not among them).  n_joins wraps on a cycle, where nobody reads it
struct UnitigRank {
    int ptr;
    unsigned n_joins;
    long long bases;
    int low, low_c;
};
static_assert(sizeof(UnitigRank) == 24, "two records to a 48-byte stretch");

// the scan's results: unitigs, entries, bases
struct UnitigTotals {
    long long unitigs, placed, length;
};

__device__ inline bool unitig_live(const gact_graph_read *__restrict__ reads, const int *__restrict__ lens,
                                   const int *__restrict__ clip, int i)
{
    const int cl = clip ? clip[2 * (size_t)i + 1] - clip[2 * (size_t)i] : lens[i];
    return reads[i].contained_by < 0 && cl > 0;
}

__global__ void __launch_bounds__(kPassBlock)
unitig_first_kernel(int nv, const gact_graph_arc *__restrict__ arcs, int n_arcs, int *__restrict__ first)
{
    const int x = blockIdx.x * kPassBlock + threadIdx.x;
    if (x > nv) return;
    int lo = 0, hi = n_arcs;                               // the first arc with u >= x
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (arcs[mid].u < x) lo = mid + 1; else hi = mid;
    }
    first[x] = lo;
}

__global__ void __launch_bounds__(kPassBlock)
unitig_check_kernel(int nv, const gact_graph_arc *__restrict__ arcs, int n_arcs, const int *__restrict__ first,
                    const gact_graph_read *__restrict__ reads, const int *__restrict__ lens, const int *__restrict__ clip,
                    int want_bases, int *out, unsigned long long *counters, int *flag)
{
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    bool e0 = false;
    if (k < n_arcs) {
        const gact_graph_arc a = arcs[k];
        int bad = 0;
        if (a.u < 0 || a.u >= nv || a.v < 0 || a.v >= nv || (a.u >> 1) == (a.v >> 1) || a.len < 1) bad |= kUnitigBadRange;
        if (k > 0) {
            const gact_graph_arc b = arcs[k - 1];
            const bool ascending = b.u != a.u ? b.u < a.u : b.len != a.len ? b.len < a.len : b.v < a.v;
            if (!ascending) bad |= kUnitigBadOrder;
        }
        if (!bad && a.flags == 0) {
            e0 = true;
            if (!unitig_live(reads, lens, clip, a.u >> 1) || !unitig_live(reads, lens, clip, a.v >> 1)) bad |= kUnitigNotLive;
            const int from = a.v ^ 1, to = a.u ^ 1;
            bool found = false;
            // (the stretch is ascending by (len, v) and the complement's len is its own: a walk, as graph_mirror_kernel's)
            for (int e = first[from]; e < first[from + 1] && !found; e++)
                found = arcs[e].u == from && arcs[e].v == to && arcs[e].flags == 0;
            if (!found) bad |= kUnitigNoComplement;
            if (want_bases) {
                const int i = a.u >> 1;
                const int cl = clip ? clip[2 * (size_t)i + 1] - clip[2 * (size_t)i] : lens[i];
                if (a.len > cl) bad |= kUnitigLongArc;
            }
            atomicAdd(&out[a.u], 1);
        }
        if (bad) atomicOr(flag, bad);
    }
    wave_count(&counters[kUnitigE0], e0);
}

// the arc is of the current set: E0, or E1 where cut is given
__device__ inline bool unitig_in_set(const gact_graph_arc &a, const int *__restrict__ cut)
{
    return a.flags == 0 && (!cut || (!cut[a.u >> 1] && !cut[a.v >> 1]));
}

__global__ void __launch_bounds__(kPassBlock)
unitig_recount_kernel(const gact_graph_arc *__restrict__ arcs, int n_arcs, const int *__restrict__ cut, int *out,
                      unsigned long long *counters, const int *__restrict__ flag)
{
    if (*flag) return;
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    bool in = false;
    if (k < n_arcs) {
        const gact_graph_arc a = arcs[k];
        in = unitig_in_set(a, cut);
        if (in) atomicAdd(&out[a.u], 1);
    }
    wave_count(&counters[kUnitigE1], in);
}

__global__ void __launch_bounds__(kPassBlock)
unitig_links_kernel(const gact_graph_arc *__restrict__ arcs, int n_arcs, const int *__restrict__ cut, const int *__restrict__ out,
                    int *__restrict__ prev, int *__restrict__ len_in, int *__restrict__ len_out, unsigned long long *counters,
                    const int *__restrict__ flag)
{
    if (*flag) return;
    const int k = blockIdx.x * kPassBlock + threadIdx.x;
    bool join = false;
    if (k < n_arcs) {
        const gact_graph_arc a = arcs[k];
        join = unitig_in_set(a, cut) && out[a.u] == 1 && out[a.v ^ 1] == 1;
        if (join) { prev[a.v] = a.u; len_in[a.v] = a.len; len_out[a.u] = a.len; }
    }
    if (counters) wave_count(&counters[kUnitigJoins], join);
}

// found: NULL, or the records the sweep in front left: a vertex on a cycle that is the cycle's place to open becomes a head,
// and closing[x] gets the length of the join cut in front of it (0: none).  The cycle that holds the lowest id m of itself and
// its complement (low < low_c) opens in front of m; its complement opens behind m^1, in front of the vertex whose prev is m^1
__global__ void __launch_bounds__(kPassBlock)
unitig_init_kernel(int nv, const int *__restrict__ prev, const int *__restrict__ len_in, const UnitigRank *__restrict__ found,
                   int *__restrict__ closing, UnitigRank *__restrict__ rank, const int *__restrict__ flag)
{
    if (*flag) return;
    const int x = blockIdx.x * kPassBlock + threadIdx.x;
    if (x >= nv) return;
    int p = prev[x];
    if (found) {
        int cut_len = 0;
        const UnitigRank f = found[x];
        if (p >= 0 && prev[f.ptr] >= 0 && (f.low < f.low_c ? x == f.low : p == (f.low_c ^ 1))) { cut_len = len_in[x]; p = -1; }
        closing[x] = cut_len;
    }
    UnitigRank r;
    r.ptr = p >= 0 ? p : x;
    r.n_joins = p >= 0 ? 1u : 0u;
    r.bases = p >= 0 ? (long long)len_in[x] : 0ll;
    r.low = x;
    r.low_c = x ^ 1;
    rank[x] = r;
}

__global__ void __launch_bounds__(kPassBlock)
unitig_jump_kernel(int nv, const UnitigRank *__restrict__ from, UnitigRank *__restrict__ to, const int *__restrict__ flag)
{
    if (*flag) return;
    const int x = blockIdx.x * kPassBlock + threadIdx.x;
    if (x >= nv) return;
    UnitigRank r = from[x];
    const UnitigRank p = from[r.ptr];
    r.ptr = p.ptr;
    r.n_joins += p.n_joins;
    r.bases += p.bases;
    r.low = min(r.low, p.low);
    r.low_c = min(r.low_c, p.low_c);
    to[x] = r;
}

__global__ void __launch_bounds__(kPassBlock)
unitig_tip_kernel(int n_reads, const gact_graph_read *__restrict__ reads, const int *__restrict__ lens, const int *__restrict__ clip,
                  const int *__restrict__ prev, const int *__restrict__ out, const UnitigRank *__restrict__ rank, int tip_reads,
                  int *__restrict__ cut, unsigned long long *counters, const int *__restrict__ flag)
{
    if (*flag) return;
    const int i = blockIdx.x * kPassBlock + threadIdx.x;
    bool tip = false, inside = false;
    if (i < n_reads) {
        inside = reads[i].contained_by >= 0;
        if (unitig_live(reads, lens, clip, i)) {
            const UnitigRank a = rank[2 * i], b = rank[2 * i + 1];
            const int h = a.ptr, t = b.ptr ^ 1;
            tip = prev[h] < 0 && (long long)a.n_joins + b.n_joins + 1 <= tip_reads && (out[h ^ 1] == 0 || out[t] == 0);
        }
        cut[i] = tip;
    }
    wave_count(&counters[kUnitigCut], tip);
    wave_count(&counters[kUnitigContained], inside);
}

// is x the head of a chain that is emitted?  and then its tail, read count, length and circular flag
__device__ inline bool unitig_emitted_head(int x, const gact_graph_read *__restrict__ reads, const int *__restrict__ lens,
                                           const int *__restrict__ clip, const int *__restrict__ cut,
                                           const UnitigRank *__restrict__ rank, const int *__restrict__ closing, int &tail,
                                           int &n, long long &length, int &circular)
{
    const int i = x >> 1;
    if (!unitig_live(reads, lens, clip, i) || cut[i]) return false;
    if (rank[x].ptr != x || x >= rank[x ^ 1].ptr) return false;
    tail = rank[x ^ 1].ptr ^ 1;
    const UnitigRank t = rank[tail];
    n = (int)t.n_joins + 1;
    circular = closing[x] > 0;
    const int ti = tail >> 1;
    length = t.bases + (circular ? closing[x] : clip ? clip[2 * (size_t)ti + 1] - clip[2 * (size_t)ti] : lens[ti]);
    return true;
}

// one lane per vertex: an emitted head leaves (1, its reads, its length) in (number, layout_at, seq_at), every other vertex
// zeros: what the scan sums.  The longest unitig and the circular ones go to the counters, once per wave
__global__ void __launch_bounds__(kPassBlock)
unitig_heads_kernel(int nv, const gact_graph_read *__restrict__ reads, const int *__restrict__ lens, const int *__restrict__ clip,
                    const int *__restrict__ cut, const UnitigRank *__restrict__ rank, const int *__restrict__ closing,
                    int *__restrict__ number, long long *__restrict__ layout_at, long long *__restrict__ seq_at,
                    unsigned long long *counters, const int *__restrict__ flag)
{
    if (*flag) return;
    const int x = blockIdx.x * kPassBlock + threadIdx.x;
    int head = 0, tail, n = 0, circular = 0;
    long long length = 0;
    if (x < nv && unitig_emitted_head(x, reads, lens, clip, cut, rank, closing, tail, n, length, circular)) head = 1;
    if (!head) { n = 0; length = 0; circular = 0; }
    if (x < nv) { number[x] = head; layout_at[x] = n; seq_at[x] = length; }
    int most_reads = n;
    long long most_bases = length;
    for (int o = 32; o > 0; o >>= 1) {
        most_reads = max(most_reads, __shfl_xor(most_reads, o));
        most_bases = max(most_bases, __shfl_xor(most_bases, o));
    }
    if ((threadIdx.x & 63) == 0) {
        if (most_reads) atomicMax(&counters[kUnitigLongestReads], (unsigned long long)most_reads);
        if (most_bases) atomicMax(&counters[kUnitigLongestBases], (unsigned long long)most_bases);
    }
    wave_count(&counters[kUnitigCircular], circular != 0);
}

// one block, in place: the exclusive scans of number, layout_at and seq_at over the vertex ids, and their totals
__global__ void __launch_bounds__(kPassBlock)
unitig_scan_kernel(int nv, int *__restrict__ number, long long *__restrict__ layout_at, long long *__restrict__ seq_at,
                   UnitigTotals *totals, const int *__restrict__ flag)
{
    if (*flag) return;
    long long carry[3] = {0, 0, 0};                             // heads, reads, bases
    for (int base = 0; base < nv; base += kPassBlock) {
        const int x = base + (int)threadIdx.x;
        long long own[3] = {0, 0, 0}, before[3], total[3];
        if (x < nv) { own[0] = number[x]; own[1] = layout_at[x]; own[2] = seq_at[x]; }     // (one branch: the loads fly together)
        block_scan_step(own, before, total);
        if (x < nv) {
            number[x] = (int)(carry[0] + before[0]);
            layout_at[x] = carry[1] + before[1];
            seq_at[x] = carry[2] + before[2];
        }
        for (int i = 0; i < 3; i++) carry[i] += total[i];
    }
    if (threadIdx.x == 0) { totals->unitigs = carry[0]; totals->placed = carry[1]; totals->length = carry[2]; }
}

__global__ void __launch_bounds__(kPassBlock)
unitig_fill_kernel(int nv, const gact_graph_read *__restrict__ reads, const int *__restrict__ lens, const int *__restrict__ clip,
                   const int *__restrict__ cut, const UnitigRank *__restrict__ rank, const int *__restrict__ closing,
                   const int *__restrict__ len_out, const int *__restrict__ number, const long long *__restrict__ layout_at,
                   const long long *__restrict__ seq_at, gact_unitig *__restrict__ unitigs, gact_unitig_entry *__restrict__ layout,
                   gact_unitig_place *__restrict__ places, const int *__restrict__ flag)
{
    if (*flag) return;
    const int x = blockIdx.x * kPassBlock + threadIdx.x;
    if (x >= nv) return;
    const int i = x >> 1;
    const bool live = unitig_live(reads, lens, clip, i);
    if (!live || cut[i]) {
        if (!(x & 1)) {
            gact_unitig_place p;
            p.unitig = -1; p.rank = -1; p.orient = 0;
            p.state = reads[i].contained_by >= 0 ? GACT_UNITIG_CONTAINED : !live ? GACT_UNITIG_EMPTY : GACT_UNITIG_TIP;
            places[i] = p;
        }
        return;
    }
    const UnitigRank r = rank[x];
    const int h = r.ptr, other = rank[x ^ 1].ptr;            // (the head of this chain and of its complement)
    if (h >= other) return;                                   // (the complement is the emitted one)
    const bool last = other == (x ^ 1);
    const int circular = closing[h] > 0;
    const int cl = clip ? clip[2 * (size_t)i + 1] - clip[2 * (size_t)i] : lens[i];
    gact_unitig_entry en;
    en.vertex = x;
    en.take = !last ? len_out[x] : circular ? closing[h] : cl;
    en.start = r.bases;
    layout[layout_at[h] + r.n_joins] = en;
    gact_unitig_place p;
    p.unitig = number[h]; p.rank = (int)r.n_joins; p.orient = x & 1; p.state = GACT_UNITIG_PLACED;
    places[i] = p;
    if (last) {
        gact_unitig u;
        u.first = h; u.last = x; u.n_reads = (int)r.n_joins + 1; u.circular = circular;
        u.layout_at = layout_at[h]; u.seq_at = seq_at[h]; u.length = r.bases + en.take;
        unitigs[number[h]] = u;
    }
}

__device__ inline uint8_t unitig_complement(uint8_t b)       // (revcomp_kernel's table, without its refusal)
{
    switch (b) {
        case 'a': return 't'; case 'A': return 'T';
        case 'c': return 'g'; case 'C': return 'G';
        case 'g': return 'c'; case 'G': return 'C';
        case 't': return 'a'; case 'T': return 'A';
        case 'n': return 'n'; case 'N': return 'N';
        default: return 'N';
    }
}

__global__ void __launch_bounds__(kPassBlock)
unitig_bases_kernel(const UnitigTotals *__restrict__ totals, const gact_unitig_entry *__restrict__ layout,
                    const gact_unitig_place *__restrict__ places, const gact_unitig *__restrict__ unitigs,
                    const uint8_t *__restrict__ raw, const int64_t *__restrict__ offsets, const int *__restrict__ lens,
                    const int *__restrict__ clip, uint8_t *__restrict__ seq, const int *__restrict__ flag)
{
    if (*flag) return;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (kPassBlock / 64) + (threadIdx.x >> 6), n_waves = (long long)gridDim.x * (kPassBlock / 64);
    const long long n = totals->placed;
    for (long long e = wave; e < n; e += n_waves) {
        const gact_unitig_entry en = layout[e];
        const int i = en.vertex >> 1;
        const int cb = clip ? clip[2 * (size_t)i] : 0, ce = clip ? clip[2 * (size_t)i + 1] : lens[i];
        const uint8_t *read = raw + offsets[i];
        uint8_t *to = seq + unitigs[places[i].unitig].seq_at + en.start;
        // (take <= ce - cb: the check kernel refused longer arcs before this kernel ran)
        if (en.vertex & 1)
            for (int j = lane; j < en.take; j += 64) to[j] = unitig_complement(read[ce - 1 - j]);
        else
            for (int j = lane; j < en.take; j += 64) to[j] = read[cb + j];
    }
}

}  // namespace gact

// ---- What a pass on an arc graph starts from (unitigs, gact_bubble.hpp, gact_clean.hpp; gact_pass.hpp says how)

// The refusals those calls share, behind each call's own NULL list and parameter checks: the bounds, the arcs, the lengths and
// clips -> the clipped total, or the refusal's code (< 0).  own: NULL, or the name of the call's own figure at the sentence's end
static int64_t check_arc_graph(const char *who, int32_t n_reads, const int32_t *read_lens, const int32_t *clip, int64_t n_arcs,
                               const gact_graph_arc *arcs, const char *own = nullptr, int64_t own_value = 0, bool own_bad = false)
{
    if (n_reads < 0 || n_reads > gact::kUnitigMaxReads || n_arcs < 0 || n_arcs > gact::kUnitigMaxArcs || (n_arcs > 0 && !arcs) || own_bad) {
        char tail[64] = "";
        if (own) snprintf(tail, sizeof tail, "; %s = %lld", own, (long long)own_value);
        return fail(GACT_HIP_EINVAL, "%s: bad arguments (n_reads = %d, at most %d; n_arcs = %lld, at most %lld%s)", who, n_reads,
                    gact::kUnitigMaxReads, (long long)n_arcs, (long long)gact::kUnitigMaxArcs, tail);
    }
    return check_read_lens(who, n_reads, read_lens, clip);
}

// The graph on the device.  A pass's scratch begins arcs (32 n_arcs) | reads (32 n_reads) | lens (4 n_reads) | clip (8 n_reads,
// where given) | skip as ints (4 n_reads, where given), and its own part begins at `end`.  first and flag are the pass's own,
// kept here by arc_graph_index because every later launch takes them.
struct ArcGraphDev {
    int n_reads, nv, n_arcs;
    size_t at_reads, at_lens, at_clip, at_skip, end;
    gact_graph_arc *arcs;
    const gact_graph_read *reads;
    const int *lens, *clip, *skip, *first;                     // clip, skip: NULL where the caller gave none
    int *flag;
    hipStream_t stream;
    std::vector<int> wide;                                     // skip as ints: alive until the copies in have been waited for
};

// the layout (n_reads > 0), and skip widened: host work in front of the call's first event
static ArcGraphDev arc_graph_layout(int32_t n_reads, const int32_t *clip, int64_t n_arcs, const uint8_t *skip)
{
    ArcGraphDev g{};
    const size_t n = (size_t)n_reads;
    g.n_reads = n_reads; g.nv = 2 * n_reads; g.n_arcs = (int)n_arcs;
    g.at_reads = up16((size_t)n_arcs * sizeof(gact_graph_arc));
    g.at_lens = g.at_reads + n * sizeof(gact_graph_read);
    g.at_clip = up16(g.at_lens + n * sizeof(int32_t));
    g.at_skip = up16(g.at_clip + (clip ? 2 * n * sizeof(int32_t) : 0));
    g.end = up16(g.at_skip + (skip ? n * sizeof(int) : 0));
    if (skip) g.wide.resize(n);
    for (size_t i = 0; skip && i < n; i++) g.wide[i] = skip[i] != 0;
    return g;
}

// the pass's scratch of `bytes`, its first event, and the copies in to the scratch's front, on the slot's stream
extern "C++" template <class Stats>
static int arc_graph_begin(ArcGraphDev &g, PassScratch<Stats> &ps, size_t bytes, hipStream_t stream, const char *who, const int32_t *read_lens,
                           const int32_t *clip, const gact_graph_read *reads, const gact_graph_arc *arcs)
{
    const size_t n = (size_t)g.n_reads;
    if (ps.reserve(bytes))
        return fail(GACT_HIP_ENOMEM, "%s: device allocation failed (%d reads, %d arcs, %zu bytes)", who, g.n_reads, g.n_arcs, bytes);
    if (int rc = ps.begin(stream, who)) return rc;
    uint8_t *p = ps.p;
    g.stream = stream;
    g.arcs = (gact_graph_arc *)p;
    g.reads = (const gact_graph_read *)(p + g.at_reads);
    g.lens = (const int *)(p + g.at_lens);
    g.clip = clip ? (const int *)(p + g.at_clip) : nullptr;
    g.skip = g.wide.empty() ? nullptr : (const int *)(p + g.at_skip);
    if (g.n_arcs) HIP_TRY(hipMemcpyAsync(p, arcs, (size_t)g.n_arcs * sizeof(gact_graph_arc), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(p + g.at_reads, reads, n * sizeof(gact_graph_read), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(p + g.at_lens, read_lens, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if (clip) HIP_TRY(hipMemcpyAsync(p + g.at_clip, clip, 2 * n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    if (g.skip) HIP_TRY(hipMemcpyAsync(p + g.at_skip, g.wide.data(), n * sizeof(int), hipMemcpyHostToDevice, stream));
    return 0;
}

// the stretches and the arc checks: out gets the out-degrees over E0, counters[kUnitigE0] their number, *flag the refusals
static void arc_graph_index(ArcGraphDev &g, int want_bases, int *first, int *out, unsigned long long *counters, int *flag)
{
    const dim3 block(gact::kPassBlock);
    g.first = first;
    g.flag = flag;
    hipLaunchKernelGGL(gact::unitig_first_kernel, lane_blocks((size_t)g.nv + 1), block, 0, g.stream, g.nv, g.arcs, g.n_arcs, first);
    hipLaunchKernelGGL(gact::unitig_check_kernel, lane_blocks((size_t)g.n_arcs), block, 0, g.stream, g.nv, g.arcs, g.n_arcs, first, g.reads,
                       g.lens, g.clip, want_bases, out, counters, flag);
}

// what the flag word says, once it is on the host
static int arc_graph_refusal(const char *who, int flag, int nv)
{
    if (flag & gact::kUnitigBadRange)
        return fail(GACT_HIP_EINVAL, "%s: an arc with u or v outside [0, %d), between the two vertices of one read, or with len < 1", who, nv);
    if (flag & gact::kUnitigBadOrder) return fail(GACT_HIP_EINVAL, "%s: the arcs are not ascending by (u, len, v)", who);
    if (flag & gact::kUnitigNotLive)
        return fail(GACT_HIP_EINVAL, "%s: an arc with flags == 0 names a read that is not live (contained, or clipped to nothing)", who);
    if (flag & gact::kUnitigNoComplement)
        return fail(GACT_HIP_EINVAL, "%s: an arc with flags == 0 whose complement v^1 -> u^1 is not among the arcs with flags == 0", who);
    if (flag & gact::kUnitigLongArc)
        return fail(GACT_HIP_EINVAL, "%s: bases asked for and an arc with flags == 0 is longer than the clipped read it leaves", who);
    if (flag) return fail(GACT_HIP_EDEVICE, "%s: the device left the flag word %d", who, flag);
    return 0;
}

// the wait of a call, or of a step of the rounds: its n counters and the flag word on the host -> what the flag word refuses
static int arc_graph_fetch(const ArcGraphDev &g, const char *who, const unsigned long long *d_counters, unsigned long long *counters, size_t n)
{
    int flag = 0;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flag, g.flag, sizeof flag, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipMemcpyAsync(counters, d_counters, n * sizeof *counters, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return arc_graph_refusal(who, flag, g.nv);
}

// One ranking sweep over the arc set (cut == NULL: E0), as the unitig call makes three and the cleaning rounds one a tip step:
// prev set to 0xff, the set's out-degrees counted into `out` where set_counters is given (else they are there), joins (counted
// where join_counters is given), records, ceil(log2 nv) jumps; with `found`, the records of the sweep in front, the joins stay
// and the cycles they found are opened.  *result: the buffer of rank[] that holds the result; *launches (NULL: not counted)
// grows by the jumps
struct UnitigRankBufs {
    int *prev, *len_in, *len_out, *closing;                    // closing: NULL where no sweep opens cycles
    gact::UnitigRank *rank[2];
};
static int unitig_sweep(const ArcGraphDev &g, const UnitigRankBufs &b, const int *cut, int *out, const gact::UnitigRank *found,
                        unsigned long long *set_counters, unsigned long long *join_counters, const gact::UnitigRank **result, int *launches)
{
    const dim3 block(gact::kPassBlock);
    const size_t nv = (size_t)g.nv, na = (size_t)g.n_arcs;
    if (!found) {
        HIP_TRY(hipMemsetAsync(b.prev, 0xff, nv * sizeof(int), g.stream));
        if (set_counters)
            hipLaunchKernelGGL(gact::unitig_recount_kernel, lane_blocks(na), block, 0, g.stream, g.arcs, g.n_arcs, cut, out, set_counters, g.flag);
        hipLaunchKernelGGL(gact::unitig_links_kernel, lane_blocks(na), block, 0, g.stream, g.arcs, g.n_arcs, cut, out, b.prev, b.len_in,
                           b.len_out, join_counters, g.flag);
    }
    int cur = found == b.rank[0] ? 1 : 0;                      // (the records of the sweep in front are read while these are made)
    hipLaunchKernelGGL(gact::unitig_init_kernel, lane_blocks(nv), block, 0, g.stream, g.nv, b.prev, b.len_in, found, b.closing, b.rank[cur],
                       g.flag);
    int rounds = 1;
    while (((size_t)1 << rounds) < nv) rounds++;
    for (int r = 0; r < rounds; r++, cur ^= 1)
        hipLaunchKernelGGL(gact::unitig_jump_kernel, lane_blocks(nv), block, 0, g.stream, g.nv, b.rank[cur], b.rank[cur ^ 1], g.flag);
    *result = b.rank[cur];
    if (launches) *launches += rounds;
    return 0;
}

// One allocation: the graph (ArcGraphDev, no skip) |
// [ out of E0, out of E1 (4 each per vertex) | counters (64) | totals (32) | flag (16) ], zeroed together |
// first (4 (2 n_reads + 1)) | prev (4 per vertex, set to 0xff in front of each links kernel) | len_in, len_out, closing (4 each
// per vertex) | cut (4 n_reads) | rank a, rank b (24 each per vertex) | number (4 per vertex) | layout_at, seq_at (8 each per
// vertex) | unitigs (40 n_reads) | layout (16 n_reads) | places (16 n_reads) | seq (the reads' clipped lengths, where asked for).
int gact_hip_unitigs(gact_hip_engine *e, int slot, int32_t n_reads, const int32_t *read_lens, const int32_t *clip,
                     const gact_graph_read *reads, int64_t n_arcs, const gact_graph_arc *arcs, const gact_unitig_params *params,
                     gact_unitig *unitigs, int32_t *n_unitigs, gact_unitig_entry *layout, gact_unitig_place *places, uint8_t *seq,
                     int64_t seq_cap, int64_t *seq_len)
{
    int rc = check_slot(e, slot);
    if (rc) return rc;
    if (!read_lens || !reads || !n_unitigs || !places || !unitigs || !layout)
        return fail(GACT_HIP_EINVAL, "unitigs: NULL argument (read_lens, reads, n_unitigs, places, unitigs and layout are needed)");
    if (seq && !seq_len) return fail(GACT_HIP_EINVAL, "unitigs: seq without seq_len (NULL argument)");
    const gact_unitig_params p = params ? *params : gact_unitig_params{GACT_UNITIG_DEFAULT_TIP_READS};
    if (p.tip_reads < 0) return fail(GACT_HIP_EINVAL, "unitigs: bad parameter (tip_reads = %d: >= 0)", p.tip_reads);
    const int64_t clipped = check_arc_graph("unitigs", n_reads, read_lens, clip, n_arcs, arcs, "seq_cap", seq_cap, seq && seq_cap < 0);
    if (clipped < 0) return GACT_HIP_EINVAL;
    const SeqSet &rs = e->sets[GACT_SET_REF];
    if (seq) {
        if (rs.n == 0 || !rs.d_raw) return fail(GACT_HIP_EINVAL, "unitigs: bases asked for while GACT_SET_REF is not uploaded");
        if (rs.n != n_reads)
            return fail(GACT_HIP_EINVAL, "unitigs: GACT_SET_REF holds %d sequences, not n_reads = %d", rs.n, n_reads);
        for (int32_t i = 0; i < n_reads; i++)
            if (rs.h_offsets[(size_t)i + 1] - rs.h_offsets[(size_t)i] != read_lens[i])
                return fail(GACT_HIP_EINVAL, "unitigs: sequence %d of GACT_SET_REF has the length %lld, read_lens says %d", i,
                            (long long)(rs.h_offsets[(size_t)i + 1] - rs.h_offsets[(size_t)i]), read_lens[i]);
    }
    if (n_reads == 0) {
        *n_unitigs = 0;
        if (seq_len) *seq_len = 0;
        return 0;
    }
    if ((rc = set_device(e))) return rc;
    Slot &sl = e->slots[slot];
    PassScratch<gact_unitig_stats> &ub = sl.unitig;
    ArcGraphDev g = arc_graph_layout(n_reads, clip, n_arcs, nullptr);
    const size_t n = (size_t)n_reads, nv = 2 * n, na = (size_t)n_arcs;
    const size_t at_out0 = g.end;
    const size_t at_out1 = at_out0 + nv * sizeof(int);
    const size_t at_counters = up16(at_out1 + nv * sizeof(int));
    const size_t at_totals = at_counters + gact::kUnitigCounters * sizeof(unsigned long long);
    const size_t at_flag = at_totals + 32;
    const size_t at_first = at_flag + 16;
    const size_t at_prev = up16(at_first + (nv + 1) * sizeof(int));
    const size_t at_len_in = at_prev + nv * sizeof(int);
    const size_t at_len_out = at_len_in + nv * sizeof(int);
    const size_t at_closing = at_len_out + nv * sizeof(int);
    const size_t at_cut = at_closing + nv * sizeof(int);
    const size_t at_rank_a = up16(at_cut + n * sizeof(int));
    const size_t at_rank_b = at_rank_a + nv * sizeof(gact::UnitigRank);
    const size_t at_number = at_rank_b + nv * sizeof(gact::UnitigRank);
    const size_t at_layout_at = up16(at_number + nv * sizeof(int));
    const size_t at_seq_at = at_layout_at + nv * sizeof(long long);
    const size_t at_unitigs = at_seq_at + nv * sizeof(long long);
    const size_t at_layout = at_unitigs + n * sizeof(gact_unitig);
    const size_t at_places = at_layout + n * sizeof(gact_unitig_entry);
    const size_t at_seq = at_places + n * sizeof(gact_unitig_place);
    const size_t bytes = at_seq + (seq ? (size_t)clipped : 0);
    if ((rc = arc_graph_begin(g, ub, bytes, sl.stream, "unitigs", read_lens, clip, reads, arcs))) return rc;
    int *d_out0 = (int *)(ub.p + at_out0), *d_out1 = (int *)(ub.p + at_out1), *d_flag = (int *)(ub.p + at_flag);
    unsigned long long *d_counters = (unsigned long long *)(ub.p + at_counters);
    gact::UnitigTotals *d_totals = (gact::UnitigTotals *)(ub.p + at_totals);
    int *d_first = (int *)(ub.p + at_first), *d_cut = (int *)(ub.p + at_cut);
    const UnitigRankBufs rb{(int *)(ub.p + at_prev), (int *)(ub.p + at_len_in), (int *)(ub.p + at_len_out), (int *)(ub.p + at_closing),
                            {(gact::UnitigRank *)(ub.p + at_rank_a), (gact::UnitigRank *)(ub.p + at_rank_b)}};
    int *d_number = (int *)(ub.p + at_number);
    long long *d_layout_at = (long long *)(ub.p + at_layout_at), *d_seq_at = (long long *)(ub.p + at_seq_at);
    gact_unitig *d_unitigs = (gact_unitig *)(ub.p + at_unitigs);
    gact_unitig_entry *d_layout = (gact_unitig_entry *)(ub.p + at_layout);
    gact_unitig_place *d_places = (gact_unitig_place *)(ub.p + at_places);
    uint8_t *d_seq = ub.p + at_seq;
    HIP_TRY(hipMemsetAsync(d_out0, 0, at_first - at_out0, sl.stream));
    const dim3 block(gact::kPassBlock);
    int launches = 0;
    // three sweeps: on E0 for the tip rule, on E1 to find the cycles and their lowest ids, and on E1 with the cycles opened
    const gact::UnitigRank *on_e0, *cycles, *ranks;
    arc_graph_index(g, seq ? 1 : 0, d_first, d_out0, d_counters, d_flag);
    if ((rc = unitig_sweep(g, rb, nullptr, d_out0, nullptr, nullptr, nullptr, &on_e0, &launches))) return rc;
    hipLaunchKernelGGL(gact::unitig_tip_kernel, lane_blocks(n), block, 0, sl.stream, n_reads, g.reads, g.lens, g.clip, rb.prev, d_out0, on_e0,
                       p.tip_reads, d_cut, d_counters, d_flag);
    if ((rc = unitig_sweep(g, rb, d_cut, d_out1, nullptr, d_counters, d_counters, &cycles, &launches))) return rc;
    if ((rc = unitig_sweep(g, rb, d_cut, d_out1, cycles, nullptr, nullptr, &ranks, &launches))) return rc;
    hipLaunchKernelGGL(gact::unitig_heads_kernel, lane_blocks(nv), block, 0, sl.stream, g.nv, g.reads, g.lens, g.clip, d_cut, ranks, rb.closing,
                       d_number, d_layout_at, d_seq_at, d_counters, d_flag);
    hipLaunchKernelGGL(gact::unitig_scan_kernel, dim3(1), block, 0, sl.stream, g.nv, d_number, d_layout_at, d_seq_at, d_totals, d_flag);
    hipLaunchKernelGGL(gact::unitig_fill_kernel, lane_blocks(nv), block, 0, sl.stream, g.nv, g.reads, g.lens, g.clip, d_cut, ranks, rb.closing,
                       rb.len_out, d_number, d_layout_at, d_seq_at, d_unitigs, d_layout, d_places, d_flag);
    if (seq)
        hipLaunchKernelGGL(gact::unitig_bases_kernel, wave_blocks(e, n), block, 0, sl.stream, d_totals, d_layout, d_places, d_unitigs,
                           rs.d_raw, rs.d_offsets, g.lens, g.clip, d_seq, d_flag);
    // the one wait: the flag word, the number of unitigs and the total length, before the copies out
    gact::UnitigTotals totals{};
    unsigned long long counters[gact::kUnitigCounters];
    HIP_TRY(hipMemcpyAsync(&totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, sl.stream));
    if ((rc = arc_graph_fetch(g, "unitigs", d_counters, counters, gact::kUnitigCounters))) return rc;
    if (totals.unitigs < 0 || totals.unitigs > n_reads || totals.placed < totals.unitigs || totals.placed > n_reads ||
        totals.length < 0 || (seq && totals.length > clipped))
        return fail(GACT_HIP_EDEVICE, "unitigs: the device counted %lld unitigs of %lld reads and %lld bases", totals.unitigs,
                    totals.placed, totals.length);
    if (totals.unitigs) {
        HIP_TRY(hipMemcpyAsync(unitigs, d_unitigs, (size_t)totals.unitigs * sizeof(gact_unitig), hipMemcpyDeviceToHost, sl.stream));
        HIP_TRY(hipMemcpyAsync(layout, d_layout, (size_t)totals.placed * sizeof(gact_unitig_entry), hipMemcpyDeviceToHost, sl.stream));
    }
    HIP_TRY(hipMemcpyAsync(places, d_places, n * sizeof(gact_unitig_place), hipMemcpyDeviceToHost, sl.stream));
    *n_unitigs = (int32_t)totals.unitigs;
    if (seq_len) *seq_len = totals.length;
    const bool room = !seq || seq_cap >= totals.length;
    if (seq && room && totals.length > 0)
        HIP_TRY(hipMemcpyAsync(seq, d_seq, (size_t)totals.length, hipMemcpyDeviceToHost, sl.stream));
    if ((rc = ub.end(sl.stream))) return rc;
    gact_unitig_stats &st = ub.stats;
    st.reads = n_reads;
    st.placed = (int32_t)totals.placed;
    st.cut = (int32_t)counters[gact::kUnitigCut];
    st.contained = (int32_t)counters[gact::kUnitigContained];
    st.unitigs = (int32_t)totals.unitigs;
    st.circular = (int32_t)counters[gact::kUnitigCircular];
    st.longest_reads = (int32_t)counters[gact::kUnitigLongestReads];
    st.longest_bases = (int64_t)counters[gact::kUnitigLongestBases];
    st.rank_launches = launches;
    st.e0_arcs = (int64_t)counters[gact::kUnitigE0];
    st.e1_arcs = (int64_t)counters[gact::kUnitigE1];
    st.joins = (int64_t)counters[gact::kUnitigJoins];
    st.links = st.e1_arcs - st.joins + 2 * (int64_t)st.circular;       // (a circular unitig's closing arc and its complement are links)
    st.scratch_bytes = (int64_t)ub.bytes;
    if (!room)
        return fail(GACT_HIP_EINVAL, "unitigs: %lld bases, room for %lld: call again with room for *seq_len", totals.length,
                    (long long)seq_cap);
    return 0;
}

int gact_hip_last_unitig_stats(gact_hip_engine *e, int slot, gact_unitig_stats *stats)
{
    return last_pass_stats(e, slot, &Slot::unitig, stats, "last_unitig_stats", "has made no unitigs yet");
}

