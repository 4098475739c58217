"""What the passes behind a run mean, held to the simulator's ground truth (gact_amd/synth.py): six checks in plain numpy.
Each takes a synth.ReadSet and one stage's output, raises AssertionError with the offending item, and returns the figures it
measured.  No engine, oracle or model is imported here: tests/test_truth_model.py hands these checks the reference path's
output, tests/test_gpu_truth.py the device's.

The truth mapping -- the frames are the point:

  genome_of(i, c)   c is a coordinate of read i AS STORED.  c+ = c on strand 0, len - 1 - c on strand 1 (the simulator stores a
                    strand-1 read reverse-complemented); the genome position is
                    start[i] + min(searchsorted(gmap[i], c+, 'left'), span[i] - 1): the first genome base of the read's span
                    whose read coordinate is not below c+ (an inserted base maps to the genome base behind it).
  a record          ab, ae are on the target as stored.  With comp set, bb, be are on the REVERSE COMPLEMENT of the stored query:
                    stored = len_q - 1 - b.  The begins come from the summary, as begins_from_summary and the PAF writer have
                    them: ab = ae - (n_eq + n_x + del_bases), bb = be - (n_eq + n_x + ins_bases); the raw ab / bb stay at the
                    hit where the left extension aligned nothing.
  a vertex          v = 2 i + s is read i as stored (s == 0) or reverse-complemented (s == 1); it runs along the genome in
                    direction +1 iff s == strand[i].
  its head          with [cb, ce) the clip in stored coordinates: genome_of(i, cb) for s == 0, genome_of(i, ce - 1) for s == 1;
                    its far end is the other one of the two.
  an arc u -> v     len is the number of u's bases in front of v's head: the genome distance head(v) - head(u) along the
                    direction, stretched by the simulator.

The stretch of the simulator (stretch_of, from simulate_reads' own arguments): a genome base gives 1 + p_ins - p_del read bases
on average, with a variance of p_ins (1 - p_ins) + p_del (1 - p_del) per genome base, so a length that should be scale * d may
miss it by B(d) = 6 sqrt(var * d) + 20: six standard deviations, and 20 for two alignment ends at the measured 4 bases each,
with room."""
import inspect

import numpy as np

from gact_amd import synth

END_SLACK = 20           # bases: two alignment ends, measured at most 4 each on the reference path, with room
SIGMAS = 6
RATE_SLACK = 0.02        # single reads' raw edit rates range from 0.12 to 0.148 around the block's 0.134
BAND = 600               # the banded distance's half width; sqrt(var * 15000) is 43
_INF = 1 << 40


def stretch_of(**simulate_args):
    """(scale, var) of simulate_reads called with these arguments (its defaults for the ones not named): read bases per genome
    base, and their variance per genome base"""
    sig = inspect.signature(synth.simulate_reads).parameters
    error = simulate_args.get("error", sig["error"].default)
    split = simulate_args.get("split", sig["split"].default)
    tot = float(sum(split))
    p_ins, p_del = error * split[1] / tot, error * split[2] / tot
    return 1.0 + p_ins - p_del, p_ins * (1.0 - p_ins) + p_del * (1.0 - p_del)


def bound(d, law):
    """B(d): how far a length may lie from scale * d"""
    return SIGMAS * float(np.sqrt(law[1] * abs(d))) + END_SLACK


# ---- the truth mapping

def genome_of(rs, i, c):
    n = len(rs.reads[i])
    assert 0 <= c < n, "coordinate %d outside read %d of %d bases" % (c, i, n)
    cp = n - 1 - c if rs.strand[i] else c
    return int(rs.start[i]) + min(int(np.searchsorted(rs.gmap[i], cp, "left")), int(rs.span[i]) - 1)


def _clip_of(rs, clip, i):
    if clip is None:
        return 0, len(rs.reads[i])
    c = np.asarray(clip).reshape(-1)
    return int(c[2 * i]), int(c[2 * i + 1])


def narrowed_clip(clip, by=300, keep=1600):
    """a clip with `by` bases more cut off both ends of every read whose clip holds more than `keep`: one under which every arc
    leaves and enters a read whose clip begins well inside it"""
    c = np.array(clip, dtype=np.int32).reshape(-1, 2)
    wide = c[:, 1] - c[:, 0] > keep
    c[wide, 0] += by
    c[wide, 1] -= by
    return c.reshape(-1)


def direction(rs, v):
    return 1 if (v & 1) == int(rs.strand[v >> 1]) else -1


def head(rs, clip, v):
    cb, ce = _clip_of(rs, clip, v >> 1)
    return genome_of(rs, v >> 1, cb if v & 1 == 0 else ce - 1)


def far_end(rs, clip, v):
    cb, ce = _clip_of(rs, clip, v >> 1)
    return genome_of(rs, v >> 1, ce - 1 if v & 1 == 0 else cb)


def spans_overlap(rs, a, b):
    return max(rs.start[a], rs.start[b]) < min(rs.start[a] + rs.span[a], rs.start[b] + rs.span[b])


def false_hits(rs, cands, n_forward):
    """(hits, pairs): the indices of the candidates (forward ones, then from n_forward on the reverse-complement strand's, as a
    run takes them) whose seed hit is false -- its two positions map to genome positions more than END_SLACK apart, or the
    query's strand is not the one that matches -- and, among them, those whose two reads have disjoint true spans.  Record i
    of a run is candidate i's, so these name the records and arcs that say nothing about the passes"""
    hits, pairs = set(), set()
    for i in range(len(cands)):
        t, q, comp = int(cands["ref_id"][i]), int(cands["query_id"][i]), i >= n_forward
        lt, lq = len(rs.reads[t]), len(rs.reads[q])
        tp, qp = min(int(cands["ref_pos"][i]), lt - 1), min(int(cands["query_pos"][i]), lq - 1)
        off = abs(genome_of(rs, t, tp) - genome_of(rs, q, lq - 1 - qp if comp else qp))
        if off > END_SLACK or comp != (rs.strand[t] != rs.strand[q]):
            hits.add(i)
            if not spans_overlap(rs, t, q):
                pairs.add(i)
    return hits, pairs


def truth_of(rs, i):
    """read i's genome span in the orientation the read is stored in"""
    g = rs.genome[rs.start[i]:rs.start[i] + rs.span[i]]
    return synth.revcomp(g) if rs.strand[i] else g


# ---- the edit distance

def edit_distance_full(a, b):
    """the unit-cost edit distance of two uint8 arrays, row by row: the dependency inside a row is min.accumulate(row - j) + j"""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    j = np.arange(len(b) + 1, dtype=np.int64)
    row = j.copy()
    for i in range(1, len(a) + 1):
        t = np.empty_like(row)
        t[0] = i
        t[1:] = np.minimum(row[1:] + 1, row[:-1] + (b != a[i - 1]))
        row = np.minimum.accumulate(t - j) + j
    return int(row[-1])


def edit_distance(a, b, band=BAND):
    """the same inside a band of +-band columns around the scaled diagonal j = i * len(b) / len(a): an upper bound of the full
    distance, equal to it when the best path stays inside (the CPU suite asserts that once, on a whole unitig)"""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return n + m
    cols = np.arange(m + 1, dtype=np.int64)
    row = np.full(m + 1, _INF, dtype=np.int64)
    hi = min(m, band)
    row[:hi + 1] = cols[:hi + 1]
    for i in range(1, n + 1):
        c = i * m // n
        lo, hi = max(0, c - band), min(m, c + band)
        first = max(lo, 1)
        t = np.minimum(row[first:hi + 1] + 1, row[first - 1:hi] + (b[first - 1:hi] != a[i - 1]))
        if lo == 0:
            t = np.concatenate(([i], t))
        j = cols[lo:hi + 1]
        row[lo:hi + 1] = np.minimum.accumulate(t - j) + j
        if lo > 0:
            row[lo - 1] = _INF                  # (row i - 1's value: the next row must not read it as row i's)
    return int(row[m])


def raw_rate(rs, i):
    """read i's edit distance to its own genome span, per genome base; kept on the read set"""
    kept = rs.__dict__.setdefault("_truth_raw_distance", {})
    if i not in kept:
        kept[i] = edit_distance(rs.reads[i], truth_of(rs, i))
    return kept[i] / float(rs.span[i])


# ---- the checks

def _begins(records, sel, sums, k):
    i = int(sel[k])
    s = sums[k]
    m = int(s["n_eq"]) + int(s["n_x"])
    ae, be = int(records["ae"][i]), int(records["be"][i])
    return ae - (m + int(s["del_bases"])), ae, be - (m + int(s["ins_bases"])), be


def record_ends(rs, records, sel, sums, false=()):
    """check 1: every selected, emitted record, at both ends: the target's and the query's coordinate map to genome positions
    at most END_SLACK apart.  false: the record indices left out (false_hits).  -> dict(ends, largest, left_out)"""
    sel = np.asarray(sel)
    assert len(sums) == len(sel)
    ends, largest, left_out = 0, 0, 0
    for k, i in enumerate(sel.tolist()):
        if not records["emitted"][i]:
            continue
        if i in false:
            left_out += 1
            continue
        t, q, comp = int(records["ref_id"][i]), int(records["query_id"][i]), int(records["comp"][i])
        ab, ae, bb, be = _begins(records, sel, sums, k)
        assert 0 <= ab < ae <= len(rs.reads[t]) and 0 <= bb < be <= len(rs.reads[q]), \
            "record %d (reads %d, %d): [%d, %d) x [%d, %d) leaves its reads" % (i, t, q, ab, ae, bb, be)
        lq = len(rs.reads[q])
        for name, tc, qc in (("begin", ab, bb), ("end", ae - 1, be - 1)):
            gt, gq = genome_of(rs, t, tc), genome_of(rs, q, lq - 1 - qc if comp else qc)
            off = abs(gt - gq)
            assert off <= END_SLACK, "record %d (reads %d, %d, comp %d): its %s is at genome %d on the target and %d on the " \
                "query, %d apart (> %d)" % (i, t, q, comp, name, gt, gq, off, END_SLACK)
            ends += 1
            largest = max(largest, off)
    return dict(ends=ends, largest=largest, left_out=left_out)


def _clipped_interval(rs, clip, i):
    a, b = head(rs, clip, 2 * i), far_end(rs, clip, 2 * i)
    return min(a, b), max(a, b)


def containments(rs, reads, records, clip, max_hang=1000):
    """check 2: a read with contained_by >= 0 has its clipped true interval inside the clipped true interval of the other read
    of that record, to within max_hang on either side.  -> dict(contained, largest_outside)"""
    contained, largest = 0, 0
    for i, r in enumerate(reads["contained_by"].tolist()):
        if r < 0:
            continue
        t, q = int(records["ref_id"][r]), int(records["query_id"][r])
        assert i in (t, q) and t != q, "read %d is contained by record %d, which joins reads %d and %d" % (i, r, t, q)
        outer = q if i == t else t
        (lo, hi), (olo, ohi) = _clipped_interval(rs, clip, i), _clipped_interval(rs, clip, outer)
        outside = max(olo - lo, hi - ohi, 0)
        assert outside <= max_hang, "read %d [%d, %d] is contained by read %d [%d, %d] (record %d) but lies %d outside it " \
            "(> %d)" % (i, lo, hi, outer, olo, ohi, r, outside, max_hang)
        contained += 1
        largest = max(largest, outside)
    return dict(contained=contained, largest_outside=largest)


def _arc_fault(rs, clip, law, u, v, ln):
    """None, or what is wrong with the arc; and (deviation, bound)"""
    if direction(rs, u) != direction(rs, v):
        return "its vertices run in opposite directions along the genome", (0, 1)
    if not spans_overlap(rs, u >> 1, v >> 1):
        return "the true spans of its reads do not overlap", (0, 1)
    d = (head(rs, clip, v) - head(rs, clip, u)) * direction(rs, u)
    if d <= 0:
        return "head(v) lies %d behind head(u)" % -d, (0, 1)
    dev, b = abs(ln - law[0] * d), bound(d, law)
    if dev > b:
        return "len %d against %.3f * %d = %.0f: off by %.0f (> %.0f)" % (ln, law[0], d, law[0] * d, dev, b), (dev, b)
    return None, (dev, b)


def arcs(rs, arcs, clip, law=None, count_only=False, false=()):
    """check 3: every arc with flags == 0: u and v run in one direction along the genome, the true spans of the two reads
    overlap, d = (head(v) - head(u)) * direction > 0 and |len - scale * d| <= B(d).  false: the arcs of these records are left
    out (false_hits).  -> dict(kept, checked, largest, worst_share); count_only: -> the number of wrong arcs"""
    law = law or stretch_of()
    kept = np.flatnonzero(arcs["flags"] == 0)
    wrong, checked, largest, share = 0, 0, 0.0, 0.0
    for k in kept.tolist():
        u, v, ln = int(arcs["u"][k]), int(arcs["v"][k]), int(arcs["len"][k])
        if int(arcs["record"][k]) in false:
            continue
        checked += 1
        fault, (dev, b) = _arc_fault(rs, clip, law, u, v, ln)
        if fault is not None:
            wrong += 1
            if not count_only:
                raise AssertionError("arc %d (%d -> %d, record %d): %s" % (k, u, v, int(arcs["record"][k]), fault))
        else:
            largest, share = max(largest, dev), max(share, dev / b)
    if count_only:
        return wrong
    return dict(kept=len(kept), checked=checked, largest=largest, worst_share=share)


def _entries(unitigs, layout, j):
    at, n = int(unitigs["layout_at"][j]), int(unitigs["n_reads"][j])
    return layout[at:at + n]


def false_joins(arcs, false):
    """the (u, v) of the arcs that come from the records `false`"""
    return set((int(a["u"]), int(a["v"])) for a in arcs if int(a["record"]) in false)


def layout(rs, unitigs, layout, places, clip, law=None, false=()):
    """check 4: inside a unitig every entry has one genome direction, the heads move strictly along it, and
    |start - scale * |head - head of the first entry|| <= B(that distance); places[i].orient is the low bit of the vertex the
    layout holds for read i.  false: the unitigs that hold one of these joins (u, v) are left out (false_joins).
    -> dict(unitigs, checked, entries, longest_reads, largest, worst_share)"""
    law = law or stretch_of()
    assert int(unitigs["n_reads"].sum()) == len(layout)
    checked, entries, largest, share = 0, 0, 0.0, 0.0
    for j in range(len(unitigs)):
        lay = _entries(unitigs, layout, j)
        vs = lay["vertex"].tolist()
        for x in vs:
            assert int(places["orient"][x >> 1]) == x & 1, "unitig %d holds vertex %d, places[%d].orient is %d" % (
                j, x, x >> 1, int(places["orient"][x >> 1]))
        if any(j2 in false for j2 in zip(vs[:-1], vs[1:])) or (unitigs["circular"][j] and (vs[-1], vs[0]) in false):
            continue
        checked += 1
        dirs = [direction(rs, x) for x in vs]
        assert len(set(dirs)) == 1, "unitig %d: vertices %s run in directions %s along the genome" % (j, vs, dirs)
        heads = [head(rs, clip, x) for x in vs]
        for r in range(len(vs)):
            if r:
                step = (heads[r] - heads[r - 1]) * dirs[0]
                assert step > 0, "unitig %d: the head of rank %d (vertex %d, genome %d) does not lie behind the head of rank %d " \
                    "(vertex %d, genome %d) in direction %+d" % (j, r, vs[r], heads[r], r - 1, vs[r - 1], heads[r - 1], dirs[0])
            d = abs(heads[r] - heads[0])
            dev, b = abs(int(lay["start"][r]) - law[0] * d), bound(d, law)
            assert dev <= b, "unitig %d rank %d (vertex %d): start %d against %.3f * %d = %.0f: off by %.0f (> %.0f)" % (
                j, r, vs[r], int(lay["start"][r]), law[0], d, law[0] * d, dev, b)
            largest, share = max(largest, dev), max(share, dev / b)
            entries += 1
    return dict(unitigs=len(unitigs), checked=checked, entries=entries,
                longest_reads=int(unitigs["n_reads"].max()) if len(unitigs) else 0, largest=largest, worst_share=share)


def unitig_truth(rs, unitigs, layout, clip, j):
    """the genome segment a spelled unitig stands for: from the first entry's head to the last entry's far end,
    reverse-complemented when the direction is -1"""
    vs = _entries(unitigs, layout, j)["vertex"].tolist()
    a, b, d = head(rs, clip, vs[0]), far_end(rs, clip, vs[-1]), direction(rs, vs[0])
    assert (b - a) * d >= 0, "unitig %d ends at genome %d, in front of its head at %d (direction %+d)" % (j, b, a, d)
    return rs.genome[a:b + 1] if d > 0 else synth.revcomp(rs.genome[b:a + 1])


def unitig_bases(rs, unitigs, layout, seq, clip):
    """check 5: every spelled unitig's edit rate against its truth is at most the mean raw edit rate of its own reads (each
    against its own genome span) + RATE_SLACK.  -> dict(rates: [(unitig, n_reads, its rate, its reads' mean raw rate)])"""
    seq = np.frombuffer(bytes(seq), dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)
    assert len(seq) == int(unitigs["length"].sum())
    rates = []
    for j in range(len(unitigs)):
        truth = unitig_truth(rs, unitigs, layout, clip, j)
        at, n = int(unitigs["seq_at"][j]), int(unitigs["length"][j])
        rate = edit_distance(seq[at:at + n], truth) / float(len(truth))
        own = float(np.mean([raw_rate(rs, x >> 1) for x in _entries(unitigs, layout, j)["vertex"].tolist()]))
        assert rate <= own + RATE_SLACK, "unitig %d of %d reads, %d bases: edit rate %.4f against its genome segment of %d; its " \
            "reads' raw rate is %.4f (+ %.2f)" % (j, int(unitigs["n_reads"][j]), n, rate, len(truth), own, RATE_SLACK)
        rates.append((j, int(unitigs["n_reads"][j]), rate, own))
    return dict(rates=rates)


def corrected(rs, read_at, seq, which):
    """check 6: each read of `which` has a corrected sequence strictly closer to its genome span than its raw bytes are, and
    over `which` the mean corrected rate is at most half the mean raw rate (read_at, seq: a window over all reads).
    -> dict(reads, worst_ratio, mean_corrected, mean_raw)"""
    seq = np.frombuffer(bytes(seq), dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)
    assert len(read_at) == rs.n + 1 and int(read_at[-1]) == len(seq)
    which = list(which)
    got, raw, worst = [], [], 0.0
    for i in which:
        r = raw_rate(rs, i)
        c = edit_distance(seq[int(read_at[i]):int(read_at[i + 1])], truth_of(rs, i)) / float(rs.span[i])
        assert c < r, "read %d: corrected edit rate %.4f, raw %.4f: not closer to its genome span" % (i, c, r)
        got.append(c)
        raw.append(r)
        worst = max(worst, c / r)
    mean_c, mean_r = float(np.mean(got)), float(np.mean(raw))
    assert mean_c <= 0.5 * mean_r, "mean corrected edit rate %.4f against raw %.4f: more than half" % (mean_c, mean_r)
    return dict(reads=len(which), worst_ratio=worst, mean_corrected=mean_c, mean_raw=mean_r)
