"""What the passes behind a run mean, held to the simulator's ground truth (gact_amd/synth.py): ten checks in plain numpy.
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
  a column          the ops of a record walk from its begins (ab, bb): = and X advance both coordinates, I the query's only, D
                    the target's only; the query's coordinate is in the record's frame (comp: the reverse complement's).
  a contig          a reference sequence that is genome[begin:end] (or a substituted copy of it): its coordinate c is genome
                    position begin + c, on the + strand; a read placed on it with comp set is a strand-1 read.
  a stored interval the genome interval [lo, hi) inside read i's span is [gmap[i][lo - start], gmap[i][hi - start]) of the read
                    in + orientation (its length where hi is the span's end), [b, e) as stored on strand 0 and
                    [len - e, len - b) on strand 1.

The stretch of the simulator (stretch_of, from simulate_reads' own arguments): a genome base gives 1 + p_ins - p_del read bases
on average, with a variance of p_ins (1 - p_ins) + p_del (1 - p_del) per genome base, so a length that should be scale * d may
miss it by B(d) = 6 sqrt(var * d) + 20: six standard deviations, and 20 for two alignment ends at the measured 4 bases each,
with room."""
import inspect

import numpy as np

from gact_amd import synth

END_SLACK = 20           # bases: two alignment ends, measured at most 4 each on the reference path, with room
REACH = 140              # bases an alignment may stop short of a true overlap's end: twice 70, the smallest multiple of 10 at
                         # which the reference path leaves no position of block A under the narrowed true depth (32 under at 50,
                         # 12 at 60); the aligner's property, measured by tests/test_truth_model.py, which asserts it
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8         # op words are len << 4 | op, BAM's numbering (include/gact_hip.h GACT_PATH_OP_*)
PRIMARY, SUPPLEMENTARY, SECONDARY = 1, 2, 3  # include/gact_hip.h GACT_PLACE_*
SIDES = ("ref", "query", "both")
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


def genome_of_many(rs, i, c):
    """genome_of for an array of coordinates of read i as stored"""
    n, c = len(rs.reads[i]), np.asarray(c, dtype=np.int64)
    assert len(c) == 0 or (0 <= c.min() and c.max() < n), "coordinates %d .. %d outside read %d of %d bases" % (
        c.min(), c.max(), i, n)
    cp = n - 1 - c if rs.strand[i] else c
    return int(rs.start[i]) + np.minimum(np.searchsorted(rs.gmap[i], cp, "left"), int(rs.span[i]) - 1)


def alignment_columns(rs, records, sel, sums, ops_of, false=()):
    """check 7: every selected, emitted record's ops (ops_of[k]: the op words of record sel[k]) walked from the summary's
    begins: the walk ends exactly at (ae, be), and at the first and the last column of every = and every X op the target's and
    the query's coordinate map to genome positions at most END_SLACK apart.  -> dict(records, run_ends, largest)"""
    sel = np.asarray(sel)
    assert len(sums) == len(sel) == len(ops_of)
    n_rec, run_ends, largest = 0, 0, 0
    for k, i in enumerate(sel.tolist()):
        if not records["emitted"][i] or i in false:
            continue
        t, q, comp = int(records["ref_id"][i]), int(records["query_id"][i]), int(records["comp"][i])
        ab, ae, bb, be = _begins(records, sel, sums, k)
        lt, lq = len(rs.reads[t]), len(rs.reads[q])
        assert 0 <= ab < ae <= lt and 0 <= bb < be <= lq, "record %d (reads %d, %d): [%d, %d) x [%d, %d) leaves its reads" % (
            i, t, q, ab, ae, bb, be)
        w = np.asarray(ops_of[k], dtype=np.uint32)
        n, op = (w >> 4).astype(np.int64), w & 15
        diag = (op == OP_EQ) | (op == OP_X)
        assert len(w) and (diag | (op == OP_I) | (op == OP_D)).all(), "record %d: no ops, or an op that is none of = X I D" % i
        t_end = ab + np.cumsum(np.where(diag | (op == OP_D), n, 0))
        q_end = bb + np.cumsum(np.where(diag | (op == OP_I), n, 0))
        assert (int(t_end[-1]), int(q_end[-1])) == (ae, be), "record %d (reads %d, %d, comp %d): the walk of its ops from " \
            "(%d, %d) ends at (%d, %d), not at its (ae, be) = (%d, %d)" % (i, t, q, comp, ab, bb, t_end[-1], q_end[-1], ae, be)
        tc = np.concatenate([(t_end - n)[diag], t_end[diag] - 1])
        qc = np.concatenate([(q_end - n)[diag], q_end[diag] - 1])
        off = np.abs(genome_of_many(rs, t, tc) - genome_of_many(rs, q, lq - 1 - qc if comp else qc))
        worst = int(np.argmax(off))
        assert off[worst] <= END_SLACK, "record %d (reads %d, %d, comp %d): the alignment column at (%d, %d) is at genome %d on " \
            "the target and %d bases from there on the query (> %d)" % (i, t, q, comp, tc[worst], qc[worst],
                                                                         genome_of(rs, t, int(tc[worst])), off[worst], END_SLACK)
        n_rec, run_ends, largest = n_rec + 1, run_ends + len(off), max(largest, int(off[worst]))
    return dict(records=n_rec, run_ends=run_ends, largest=largest)


def stored_interval(rs, i, lo, hi):
    """the genome interval [lo, hi), inside read i's span, in the read's stored coordinates"""
    n, st, g = len(rs.reads[i]), int(rs.start[i]), rs.gmap[i]
    assert st <= lo < hi <= st + int(rs.span[i])
    b, e = min(int(g[lo - st]), n), (min(int(g[hi - st]), n) if hi - st < len(g) else n)
    return (n - e, n - b) if rs.strand[i] else (b, e)


def true_depth(rs, records, sel, sides, by, false=()):
    """the depth the true overlaps give: every selected, emitted record puts the true overlap of its two reads' spans, in stored
    coordinates, moved outwards by `by` at both ends (inwards when negative) and clipped to the read, on its target ("ref"), its
    query ("query") or both.  -> (int64 depth of every position, read after read; the intervals counted per read)"""
    assert sides in SIDES
    lens = np.array([len(r) for r in rs.reads], dtype=np.int64)
    at = np.concatenate(([0], np.cumsum(lens)))
    diff, counted = np.zeros(int(at[-1]) + 1, dtype=np.int64), np.zeros(len(lens), dtype=np.int64)
    for i in np.asarray(sel).tolist():
        if not records["emitted"][i] or i in false:
            continue
        t, q = int(records["ref_id"][i]), int(records["query_id"][i])
        lo = max(int(rs.start[t]), int(rs.start[q]))
        hi = min(int(rs.start[t] + rs.span[t]), int(rs.start[q] + rs.span[q]))
        assert lo < hi, "record %d: the true spans of reads %d and %d do not overlap" % (i, t, q)
        for r in ((t,) if sides == "ref" else (q,) if sides == "query" else (t, q)):
            b, e = stored_interval(rs, r, lo, hi)
            counted[r] += 1
            b, e = max(b - by, 0), min(e + by, int(lens[r]))
            if b < e:
                diff[at[r] + b] += 1
                diff[at[r] + e] -= 1
    return np.cumsum(diff[:-1]), counted


def depth_misses(rs, records, sel, depth, sides="both", reach=REACH, slack=END_SLACK):
    """-> (positions whose depth is under the true depth narrowed by reach, positions over the one widened by slack)"""
    t_in, t_out = true_depth(rs, records, sel, sides, -reach)[0], true_depth(rs, records, sel, sides, slack)[0]
    return int((np.asarray(depth) < t_in).sum()), int((np.asarray(depth) > t_out).sum())


def _where(rs, p):
    at = np.concatenate(([0], np.cumsum([len(r) for r in rs.reads])))
    i = int(np.searchsorted(at, p, "right")) - 1
    return i, int(p - at[i])


def depth_against_truth(rs, records, sel, sums, depth, cover, sides="both", min_depth=3):
    """check 8, one side: T_in <= depth <= T_out at every position of every read, T_out the true depth of intervals widened by
    END_SLACK and T_in of intervals narrowed by REACH; a read has as many intervals as true overlaps; no position of the
    table's [span_begin, span_end) has T_out < min_depth.  -> dict(positions, intervals, ratio = depth.sum() / T.sum())"""
    assert len(sums) == len(sel)
    depth = np.asarray(depth)
    lens = np.array([len(r) for r in rs.reads], dtype=np.int64)
    at = np.concatenate(([0], np.cumsum(lens)))
    assert len(depth) == at[-1] and len(cover) == rs.n
    (t_in, _), (t_out, counted), (t, _) = (true_depth(rs, records, sel, sides, by) for by in (-REACH, END_SLACK, 0))
    for what, bad, truth, how in (("over", depth > t_out, t_out, "widened by %d" % END_SLACK),
                                  ("under", depth < t_in, t_in, "narrowed by %d" % REACH)):
        if bad.any():
            i, c = _where(rs, int(np.flatnonzero(bad)[0]))
            raise AssertionError("sides %s: %d of %d positions have a depth %s the true depth; the first is read %d (strand %d) "
                                 "position %d: depth %d, true depth %d of the overlaps %s" % (
                                     sides, int(bad.sum()), len(depth), what, i, rs.strand[i], c, depth[at[i] + c],
                                     truth[at[i] + c], how))
    for i in range(rs.n):
        assert int(cover["n_intervals"][i]) == counted[i], "sides %s: read %d has %d intervals, %d true overlaps" % (
            sides, i, int(cover["n_intervals"][i]), counted[i])
        b, e = int(cover["span_begin"][i]), int(cover["span_end"][i])
        assert 0 <= b <= e <= lens[i] and (b == e or t_out[at[i] + b:at[i] + e].min() >= min_depth), "sides %s: read %d's span " \
            "[%d, %d) holds a position whose true depth is under %d" % (sides, i, b, e, min_depth)
    return dict(positions=len(depth), intervals=int(counted.sum()), ratio=float(depth.sum()) / float(t.sum()))


def depth_of_sides(rs, records, sel, sums, by_side, min_depth=3):
    """check 8: by_side[s] = (the COVER_DTYPE table, the per-base depth) of read_coverage(sides=s, depth=True) for s in SIDES:
    each against the truth of its own side, and the "ref" and "query" depths add up to the "both" depth.  -> {side: figures}"""
    out = {s: depth_against_truth(rs, records, sel, sums, by_side[s][1], by_side[s][0], s, min_depth) for s in SIDES}
    both = np.asarray(by_side["ref"][1], dtype=np.int64) + by_side["query"][1]
    bad = np.flatnonzero(both != by_side["both"][1])
    assert len(bad) == 0, "the ref and query depths do not add up to the depth of both at %d positions, the first %s" % (
        len(bad), _where(rs, int(bad[0])))
    return out


def placements(rs, contigs, decoy, records, sums, place, table, decoy_share=1000):
    """check 9: reads placed on contigs.  contigs[c] = (begin, end): contig c is genome[begin:end], but contig `decoy`, a
    diverged copy of its interval.  Every record counts (no sel); a record's share is what its read's true span and its
    contig's interval have in common.  Every read with an emitted record has a primary, the record on a true contig with the
    largest share; both ends of every counted record are at most END_SLACK from the truth; a read's other records on true
    contigs are supplementaries; a decoy record with a share of decoy_share or more is a secondary of its read's record on the
    contig that holds the decoy's interval; every read with such a decoy record has a lower MAPQ than every read without.
    -> dict(kinds, ends, largest, mapq_with_decoy, mapq_without)"""
    n = len(records)
    assert len(sums) == len(place) == n and len(table) == rs.n
    sel = np.arange(n)
    home = [c for c, (b, e) in enumerate(contigs) if c != decoy and b <= contigs[decoy][0] and contigs[decoy][1] <= e]
    assert len(home) == 1
    kind, ends, largest = place["kind"].tolist(), 0, 0

    def share(k):
        i, (b, e) = int(records["query_id"][k]), contigs[int(records["ref_id"][k])]
        return max(0, min(e, int(rs.start[i] + rs.span[i])) - max(b, int(rs.start[i])))

    per_read = [[] for _ in range(rs.n)]
    for k in range(n):
        if records["emitted"][k]:
            assert kind[k] != 0, "record %d is emitted and was not counted" % k
            per_read[int(records["query_id"][k])].append(k)
        else:
            assert kind[k] == 0, "record %d is not emitted and has kind %d" % (k, kind[k])
    with_decoy, without = [], []
    for i, ks in enumerate(per_read):
        if not ks:
            continue
        true = [k for k in ks if int(records["ref_id"][k]) != decoy]
        assert true, "read %d has records on the decoy only" % i
        best = max(true, key=share)
        got = int(table["primary"][i])
        assert got == best and kind[best] == PRIMARY, "read %d: its primary is record %d (contig %d), not record %d on contig %d, " \
            "which holds %d of its %d genome bases (that record's kind: %d)" % (
                i, got, int(records["ref_id"][got]) if got >= 0 else -1, best, int(records["ref_id"][best]), share(best),
                int(rs.span[i]), kind[best])
        lq = len(rs.reads[i])
        for k in ks:
            c, comp = int(records["ref_id"][k]), int(records["comp"][k])
            ab, ae, bb, be = _begins(records, sel, sums, k)
            assert 0 <= ab < ae <= contigs[c][1] - contigs[c][0] and 0 <= bb < be <= lq, \
                "record %d (contig %d, read %d): [%d, %d) x [%d, %d) leaves its sequences" % (k, c, i, ab, ae, bb, be)
            for name, tc, qc in (("begin", ab, bb), ("end", ae - 1, be - 1)):
                gt, gq = contigs[c][0] + tc, genome_of(rs, i, lq - 1 - qc if comp else qc)
                assert abs(gt - gq) <= END_SLACK, "record %d (contig %d, read %d, comp %d): its %s is at genome %d on the contig " \
                    "and %d on the read, %d apart (> %d)" % (k, c, i, comp, name, gt, gq, abs(gt - gq), END_SLACK)
                ends, largest = ends + 1, max(largest, abs(gt - gq))
            if k in true and k != best:
                assert kind[k] == SUPPLEMENTARY, "record %d: read %d's piece on contig %d (%d genome bases) has kind %d, not " \
                    "SUPPLEMENTARY" % (k, i, c, share(k), kind[k])
        big = [k for k in ks if int(records["ref_id"][k]) == decoy and share(k) >= decoy_share]
        for k in big:
            at_home = [x for x in true if int(records["ref_id"][x]) == home[0]]
            assert kind[k] == SECONDARY and len(at_home) == 1 and int(place["parent"][k]) == at_home[0], \
                "record %d: read %d's record on the decoy (%d genome bases) has kind %d and parent %d; SECONDARY of %s expected" % (
                    k, i, share(k), kind[k], int(place["parent"][k]), at_home)
        (with_decoy if big else without).append(int(table["mapq"][i]))
    counts = np.bincount(place["kind"], minlength=5).tolist()
    comp = records["comp"][records["emitted"] != 0]
    assert comp.any() and not comp.all(), "one strand only"
    assert counts[SUPPLEMENTARY] >= 10 and counts[SECONDARY] >= 10 and with_decoy and without, \
        "the block is trivial: kinds %s, %d reads with a decoy record" % (counts, len(with_decoy))
    assert max(with_decoy) < min(without), "a read with a record on the decoy has MAPQ %d, one without has %d: not lower" % (
        max(with_decoy), min(without))
    return dict(kinds=counts, ends=ends, largest=largest, mapq_with_decoy=(min(with_decoy), max(with_decoy)),
                mapq_without=(min(without), max(without)))


def identities(records, sel, sums, false=()):
    """check 10: identity = n_eq / (n_eq + n_x + ins_bases + del_bases) of every selected, emitted record; the lowest of the
    true records is above the highest of the records `false` (false_hits).  -> dict(true, false: (records, lowest, highest))"""
    sel = np.asarray(sel)
    assert len(sums) == len(sel)
    ident = {True: [], False: []}
    for k, i in enumerate(sel.tolist()):
        if records["emitted"][i]:
            s = sums[k]
            cols = int(s["n_eq"]) + int(s["n_x"]) + int(s["ins_bases"]) + int(s["del_bases"])
            assert cols > 0, "record %d is emitted and has no columns" % i
            ident[i not in false].append(int(s["n_eq"]) / float(cols))
    t, f = ident[True], ident[False]
    assert t, "no true record"
    assert not f or min(t) > max(f), "identity does not tell the false records from the true ones: the lowest true record has " \
        "%.4f, the highest false one %.4f" % (min(t), max(f))
    return dict(true=(len(t), min(t), max(t)), false=(len(f), min(f), max(f)) if f else (0, None, None))
