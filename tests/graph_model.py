"""The overlap graph of gact_hip_overlap_graph in plain Python and numpy, restated from the entry's comment in include/gact_hip.h,
and the crafted record sets that tests/test_graph_model.py and tests/test_gpu_graph.py share.

  class of every counted record against the clipped reads (the first rule that applies: SELF, DROPPED, INTERNAL, a containment,
  SHORT, DOVETAIL); a read is contained iff some record says so; DOVETAIL records between two reads that are not contained
  propose an arc and its complement; one arc per (u, v): the higher score, then the lower record index; bit 0 of an arc u -> x:
  some w with u -> w, w -> x and len(u->w) + len(w->x) <= len(u->x) + fuzz; bit 1: bit 0 of x^1 -> u^1.
Dictionaries and loops, no cleverness."""
import numpy as np

from gact_amd import engine

NONE, SELF, DROPPED, INTERNAL, QUERY_CONTAINED, TARGET_CONTAINED, SHORT, DOVETAIL = range(8)
DEFAULTS = dict(max_hang=1000, int_permille=800, min_ovlp=1000, fuzz=1000)
PATTERNS = ("tiling", "contained", "mutual", "internal", "thresholds", "clip", "sums", "duplicates", "both_strands", "self",
            "not_emitted", "sel", "disagree", "hub", "blocks257", "blocks513", "many_reads", "random", "empty", "tiling128", "tiling129")


def classify(rec, k, i, lens, clip, sums, p):
    """-> (class, None) or (DOVETAIL, [arc, complement]); arcs are (u, v, len, ov_u, ov_v).  rec: dict of lists"""
    t, q, rev = rec["ref_id"][i], rec["query_id"][i], 1 if rec["comp"][i] else 0
    if t == q:
        return SELF, None
    ab, ae, bb, be = rec["ab"][i], rec["ae"][i], rec["bb"][i], rec["be"][i]
    if sums is not None:
        s = sums[k]
        m = int(s["n_eq"]) + int(s["n_x"])
        ab, bb = ae - (m + int(s["del_bases"])), be - (m + int(s["ins_bases"]))
    cbt, cet = (0, lens[t]) if clip is None else (clip[2 * t], clip[2 * t + 1])
    cbq, ceq = (0, lens[q]) if clip is None else (clip[2 * q], clip[2 * q + 1])
    if rev:
        cbq, ceq = lens[q] - ceq, lens[q] - cbq
    cut5, cut3 = max(cbt - ab, cbq - bb, 0), max(ae - cet, be - ceq, 0)
    ts, te, qs, qe = ab + cut5, ae - cut3, bb + cut5, be - cut3
    if te <= ts or qe <= qs:
        return DROPPED, None
    ts, te, qs, qe, tl, ql = ts - cbt, te - cbt, qs - cbq, qe - cbq, cet - cbt, ceq - cbq
    ext5, ext3, sq, st = min(qs, ts), min(ql - qe, tl - te), qe - qs, te - ts
    if ext5 > p["max_hang"] or ext3 > p["max_hang"] or 1000 * sq < p["int_permille"] * (sq + ext5 + ext3):
        return INTERNAL, None
    q_in = qs <= ts and ql - qe <= tl - te
    t_in = qs >= ts and ql - qe >= tl - te
    if q_in and t_in:
        if ql != tl:
            q_in = ql < tl
        else:
            q_in = q > t
        t_in = not q_in
    if q_in:
        return QUERY_CONTAINED, None
    if t_in:
        return TARGET_CONTAINED, None
    ov_q, ov_t = sq + ext5 + ext3, st + ext5 + ext3
    if ov_q < p["min_ovlp"] or ov_t < p["min_ovlp"]:
        return SHORT, None
    vq, vt = 2 * q + rev, 2 * t
    if qs > ts:
        arcs = [(vq, vt, qs - ts, ov_q, ov_t), (vt ^ 1, vq ^ 1, (tl - te) - (ql - qe), ov_t, ov_q)]
    else:
        arcs = [(vt, vq, ts - qs, ov_t, ov_q), (vq ^ 1, vt ^ 1, (ql - qe) - (tl - te), ov_q, ov_t)]
    assert arcs[0][2] >= 1 and arcs[1][2] >= 1
    return DOVETAIL, arcs


def graph(records, read_lens, sel=None, sums=None, clip=None, params=None):
    """-> dict(reads GRAPH_READ_DTYPE, arcs GRAPH_ARC_DTYPE, classes uint8 (one per chosen record), counts: the integer fields of
    gact_graph_stats).  IndexError: a sel index outside the records; ValueError: a counted record's read id outside the reads"""
    p = dict(DEFAULTS, **(params or {}))
    assert all(v >= 0 for v in p.values()) and p["int_permille"] <= 1000
    lens = [int(v) for v in read_lens]
    n_reads, n = len(lens), len(records)
    cl = None if clip is None else [int(v) for v in np.asarray(clip).reshape(-1)]
    if cl is not None:
        assert len(cl) == 2 * n_reads and all(0 <= cl[2 * i] <= cl[2 * i + 1] <= lens[i] for i in range(n_reads))
    assert all(v >= 0 for v in lens)
    rec = {name: records[name].tolist() for name in ("ref_id", "query_id", "ab", "ae", "bb", "be", "comp", "emitted", "score")}
    chosen = list(range(n)) if sel is None else [int(i) for i in sel]
    if n == 0:
        chosen = []
    classes = np.zeros(len(chosen), dtype=np.uint8)
    reads = np.zeros(n_reads, dtype=engine.GRAPH_READ_DTYPE)
    n_hits, n_internal, n_contains = [0] * n_reads, [0] * n_reads, [0] * n_reads
    contained_by = [-1] * n_reads
    dovetails = []
    for k, i in enumerate(chosen):
        if not 0 <= i < n:
            raise IndexError("sel[%d] = %d outside [0, %d)" % (k, i, n))
    for k, i in enumerate(chosen):
        if not rec["emitted"][i]:
            continue
        t, q = rec["ref_id"][i], rec["query_id"][i]
        if not (0 <= t < n_reads and 0 <= q < n_reads):
            raise ValueError("record %d names a read outside [0, %d)" % (i, n_reads))
        c, arcs = classify(rec, k, i, lens, cl, sums, p)
        classes[k] = c
        if c in (SELF, DROPPED):
            continue
        n_hits[t] += 1
        n_hits[q] += 1
        if c == INTERNAL:
            n_internal[t] += 1
            n_internal[q] += 1
        elif c in (QUERY_CONTAINED, TARGET_CONTAINED):
            inner, outer = (q, t) if c == QUERY_CONTAINED else (t, q)
            n_contains[outer] += 1
            contained_by[inner] = i if contained_by[inner] < 0 else min(contained_by[inner], i)
        elif c == DOVETAIL:
            dovetails.append((k, i, t, q, arcs))
    best, proposed = {}, 0
    for k, i, t, q, arcs in dovetails:
        if contained_by[t] >= 0 or contained_by[q] >= 0:
            continue
        for side, (u, v, ln, ov_u, ov_v) in enumerate(arcs):
            proposed += 1
            rank = (-rec["score"][i], i, 2 * k + side)
            if (u, v) not in best or rank < best[(u, v)][0]:
                best[(u, v)] = (rank, (u, v, ln, ov_u, ov_v, i, rec["score"][i]))
    rows = sorted((a for _, a in best.values()), key=lambda a: (a[0], a[2], a[1]))
    length = {(a[0], a[1]): a[2] for a in rows}
    out = {}
    for a in rows:
        out.setdefault(a[0], []).append(a[1])
    bit0 = {}
    for (u, x), lux in length.items():
        bit0[(u, x)] = int(any(w != x and (w, x) in length and length[(u, w)] + length[(w, x)] <= lux + p["fuzz"] for w in out[u]))
    arcs = np.zeros(len(rows), dtype=engine.GRAPH_ARC_DTYPE)
    deg, kept = [[0, 0] for _ in range(n_reads)], [[0, 0] for _ in range(n_reads)]
    for j, a in enumerate(rows):
        u, v = a[0], a[1]
        flags = bit0[(u, v)] | 2 * bit0[(v ^ 1, u ^ 1)]
        arcs[j] = a + (flags,)
        deg[u >> 1][u & 1] += 1
        kept[u >> 1][u & 1] += flags == 0
    reads["n_hits"], reads["n_internal"], reads["n_contains"], reads["contained_by"] = n_hits, n_internal, n_contains, contained_by
    if n_reads:
        reads["deg"], reads["kept"] = deg, kept
    by_class = np.bincount(classes, minlength=8).tolist()
    n_kept = int((arcs["flags"] == 0).sum())
    counts = dict(reads=n_reads, contained=sum(c >= 0 for c in contained_by), by_class=by_class, proposed=proposed,
                  arcs=len(rows), transitive=len(rows) - n_kept, kept=n_kept)
    return dict(reads=reads, arcs=arcs, classes=classes, counts=counts)


# ---- record sets

def records_of(rows):
    """[(ref_id, query_id, comp, ab, ae, bb, be, score, emitted)] -> OVERLAP_DTYPE records"""
    out = np.zeros(len(rows), dtype=engine.OVERLAP_DTYPE)
    if rows:
        cols = np.array(rows, dtype=np.int64).T
        for name, col in zip(("ref_id", "query_id", "comp", "ab", "ae", "bb", "be", "score", "emitted"), cols):
            out[name] = col
    return out


def layout_row(layout, t, q, score=None, emitted=1):
    """the exact overlap of reads t and q of a layout [(genome start, length, strand)]: target coordinates on the read as stored,
    query coordinates on the strand that matches it (gact_overlap's ab .. be); None when they share no base"""
    (st, lt, sdt), (sq, lq, sdq) = layout[t], layout[q]
    lo, hi = max(st, sq), min(st + lt, sq + lq)
    if hi <= lo:
        return None
    if sdt == 0:
        ab, ae, bb, be = lo - st, hi - st, lo - sq, hi - sq
    else:
        ab, ae, bb, be = st + lt - hi, st + lt - lo, sq + lq - hi, sq + lq - lo
    return (t, q, int(sdt != sdq), ab, ae, bb, be, hi - lo if score is None else score, emitted)


def layout_records(layout, min_overlap=1, ordered=True):
    """every pair of a layout that shares min_overlap bases: (t, q) and, when ordered, (q, t) as well"""
    rows = []
    for t in range(len(layout)):
        for q in range(len(layout)):
            if t == q or (not ordered and q < t):
                continue
            row = layout_row(layout, t, q)
            if row is not None and row[7] >= min_overlap:
                rows.append(row)
    return rows


def _random_layout(rng, n, genome, lo, hi):
    return [(int(rng.integers(0, genome)), int(rng.integers(lo, hi)), int(rng.integers(0, 2))) for _ in range(n)]


def _noise(rng, rec):
    """the fields no rule reads differ from record to record"""
    n = len(rec)
    rec["first_tile_score"] = rng.integers(0, 320, n)
    rec["n_tiles"] = rng.integers(1, 90, n)
    rec["cells"] = rng.integers(1, 1 << 40, n)
    return rec


def crafted(pattern, seed=20261019):
    """-> (records, read_lens int32, kwargs of graph()) of one of PATTERNS, the same on every call"""
    rng = np.random.default_rng([seed, PATTERNS.index(pattern)])
    kw = {}
    if pattern == "tiling":
        # six reads of 5000 every 2000 bases, strands mixed: neighbours share 3000, next neighbours 1000, a chain
        layout = [(2000 * i, 5000, s) for i, s in enumerate((0, 1, 1, 0, 1, 0))]
        rows = layout_records(layout)
    elif pattern == "contained":
        # read 2 lies inside read 0, read 3 inside read 1 (other strand); 0 - 1 - 4 is what is left
        layout = [(0, 8000, 0), (5000, 8000, 1), (1000, 3000, 1), (7000, 4000, 0), (10000, 8000, 0)]
        rows = layout_records(layout)
    elif pattern == "mutual":
        # both ends of both reads reached.  Reads 0, 1: equal lengths, the higher id is the contained one, whichever side it is
        # on; reads 2, 3 and 4, 5: an indel makes the lengths unequal, the shorter read is the contained one
        lens = [4000, 4000, 4000, 4100, 4100, 4000]
        rows = [(0, 1, 0, 0, 4000, 0, 4000, 3900, 1), (1, 0, 0, 0, 4000, 0, 4000, 3900, 1),
                (2, 3, 1, 0, 4000, 0, 4100, 3800, 1),
                (5, 4, 0, 0, 4000, 0, 4100, 3800, 1), (4, 5, 0, 0, 4100, 0, 4000, 3800, 1)]
        return _noise(rng, records_of(rows)), np.array(lens, dtype=np.int32), kw
    elif pattern == "internal":
        # a chimera-like hit: 1500 bases in the middle of both reads, 2000 unaligned on every side
        lens = [6000, 6000, 6000]
        rows = [(0, 1, 0, 2000, 3500, 2200, 3700, 1400, 1), (1, 2, 1, 2500, 4000, 2000, 3500, 1300, 1),
                (0, 2, 0, 3000, 6000, 0, 3000, 2900, 1)]
        return _noise(rng, records_of(rows)), np.array(lens, dtype=np.int32), kw
    elif pattern == "thresholds":
        lens, rows, H = [], [], DEFAULTS["max_hang"]

        def pair(lt, lq, ab, ae, bb, be, score=100):
            t = len(lens)
            lens.extend([lt, lq])
            rows.append((t, t + 1, 0, ab, ae, bb, be, score, 1))

        # ext5 = min(qs, ts) at max_hang on the target side, on the query side, and one over; the query ends with the overlap
        pair(20000, 20000, H, H + 15000, 5000, 20000)
        pair(20000, 20000, 5000, 20000, H, H + 15000)
        pair(20000, 20000, H + 1, H + 1 + 15000, 5000, 20000)
        # ext3 = min(ql - qe, tl - te) at max_hang and one over; the query begins with the overlap
        pair(20000, 20000, 5000, 20000 - H, 0, 15000 - H)
        pair(20000, 20000, 5000, 20000 - H - 1, 0, 15000 - H - 1)
        # 1000 sq >= 800 (sq + ext5 + ext3): sq = 800 and ext5 = 200 at equality; sq = 799 and ext5 = 200 one under
        pair(9000, 5800, 200, 1000, 5000, 5800)
        pair(9000, 5799, 200, 999, 5000, 5799)
        # ov = min_ovlp and min_ovlp - 1, on the query side and on the target side (an indel makes them differ)
        pair(9000, 9000, 8000, 9000, 0, 1000)
        pair(9000, 9000, 8001, 9000, 0, 999)
        pair(9000, 9000, 8000, 9000, 0, 1001)
        pair(9000, 9000, 7999, 9000, 0, 999)
        # the fuzz sum: a -> b -> c with len 3000 + 3000 against a -> c of 5000 (equality with fuzz 1000) and 4999 (one over)
        for lac in (5000, 4999):
            a = len(lens)
            lens.extend([10000, 10000, 10000])
            rows.append((a, a + 1, 0, 3000, 10000, 0, 7000, 7000, 1))
            rows.append((a + 1, a + 2, 0, 3000, 10000, 0, 7000, 7000, 1))
            rows.append((a, a + 2, 0, lac, 10000, 0, 10000 - lac, 10000 - lac, 1))
        return _noise(rng, records_of(rows)), np.array(lens, dtype=np.int32), kw
    elif pattern == "clip":
        # the tiling's reads with 300 bases of adapter on both ends of every read, clipped away; read 6 has an empty clip, read 7
        # a clip that leaves nothing of its only overlap, read 8 (other strand) an asymmetric one: 100 at its begin, 900 at its end
        layout = [(2000 * i - 300, 5600, s) for i, s in enumerate((0, 1, 1, 0, 1, 0))]
        layout += [(3000, 5000, 0), (11000, 6000, 1), (13000, 5000, 1)]
        rows = layout_records(layout)
        lens = [ln for _, ln, _ in layout]
        clip = [(300, 5300)] * 6 + [(2500, 2500), (0, 1500), (100, 4100)]
        kw = dict(clip=np.array(clip, dtype=np.int32).reshape(-1))
        return _noise(rng, records_of(rows)), np.array(lens, dtype=np.int32), kw
    elif pattern == "sums":
        # the tiling with every ab / bb left at a hit in the middle of the overlap: the summaries put the begins back
        layout = [(2000 * i, 5000, s) for i, s in enumerate((0, 1, 1, 0, 1, 0))]
        rows = layout_records(layout)
        rec = records_of(rows)
        order = rng.permutation(len(rec)).astype(np.int32)
        sums = np.zeros(len(rec), dtype=engine.SUMMARY_DTYPE)
        for k, i in enumerate(order):
            span = int(rec["ae"][i] - rec["ab"][i])
            x, gaps = int(rng.integers(0, 50)), int(rng.integers(0, 30))
            sums[k]["n_eq"], sums[k]["n_x"] = span - x - gaps, x
            sums[k]["ins_bases"] = sums[k]["del_bases"] = gaps
            for name in ("eq_runs", "x_runs", "ins_runs", "del_runs"):
                sums[k][name] = rng.integers(1, 9)
        rec["ab"] += (rec["ae"] - rec["ab"]) // 2
        rec["bb"] += (rec["be"] - rec["bb"]) // 3
        lens = [ln for _, ln, _ in layout]
        return _noise(rng, rec), np.array(lens, dtype=np.int32), dict(sel=order, sums=sums)
    elif pattern == "duplicates":
        # (0, 1), (1, 0) and (0, 1) again, equal scores: the lowest index wins both keys; (1, 2) twice, the later one better
        layout = [(0, 6000, 0), (3000, 6000, 1), (6000, 6000, 0)]
        a, b, c, d = layout_row(layout, 0, 1, 500), layout_row(layout, 1, 0, 500), layout_row(layout, 1, 2, 400), layout_row(layout, 2, 1, 450)
        shifted = (a[0], a[1], a[2], a[3] + 7, a[4], a[5] + 5, a[6], 500, 1)        # another len on the same key
        rows = [shifted, b, a, c, d]
    elif pattern == "both_strands":
        # read 1 follows read 0 on this strand, and (an inverted repeat) on the other one as well: 0 -> 1 and 0 -> 1^1
        lens = [6000, 6000]
        rows = [(0, 1, 0, 3000, 6000, 0, 3000, 2900, 1), (0, 1, 1, 3500, 6000, 0, 2500, 2400, 1)]
        return _noise(rng, records_of(rows)), np.array(lens, dtype=np.int32), kw
    elif pattern == "self":
        layout = [(0, 6000, 0), (3000, 6000, 0)]
        rows = layout_records(layout) + [(0, 0, 0, 0, 6000, 0, 6000, 6000, 1), (1, 1, 1, 100, 3000, 3000, 5900, 2800, 1)]
    elif pattern == "not_emitted":
        layout = [(2000 * i, 5000, i & 1) for i in range(8)]
        rows = [r[:8] + (k % 3 != 0,) for k, r in enumerate(layout_records(layout))]
    elif pattern == "sel":
        layout = [(2000 * i, 5000, i & 1) for i in range(8)]
        rows = [r[:8] + (k % 5 != 0,) for k, r in enumerate(layout_records(layout))]
        kw = dict(sel=rng.permutation(len(rows))[:2 * len(rows) // 3].astype(np.int32))
    elif pattern == "disagree":
        # (0, 1) says read 1 is inside read 0, (1, 0) -- with other coordinates -- says read 0 is inside read 1: both go, and
        # read 2, which overlaps both, keeps no arc
        lens = [5000, 5000, 6000]
        rows = [(0, 1, 0, 100, 5000, 0, 5000, 4800, 1), (1, 0, 0, 50, 5000, 0, 5000, 4900, 1),
                (0, 2, 0, 2000, 5000, 0, 3000, 2900, 1), (1, 2, 0, 2500, 5000, 0, 2500, 2400, 1)]
        return _noise(rng, records_of(rows)), np.array(lens, dtype=np.int32), kw
    elif pattern == "hub":
        # read 0 reaches 65 reads to its right, read 1 reaches 129 to its left; the reached reads are 10000 apart in their own
        # far ends, so none contains another, and they overlap one another: lists longer than one and two waves, with triangles
        layout = [(0, 9000, 0), (100000, 9000, 1)]
        layout += [(3000 + 20 * j, 9000 + 3 * j, j & 1) for j in range(65)]
        layout += [(103000 + 20 * j - (9000 + 3 * j), 9000 + 3 * j, (j >> 1) & 1) for j in range(129)]
        rows = layout_records(layout, min_overlap=1000, ordered=False)
        kw = dict(params=dict(fuzz=10))
    elif pattern in ("blocks257", "blocks513"):
        want = int(pattern[6:])
        layout = _random_layout(rng, 60, 40000, 3000, 7000)
        rows = layout_records(layout, min_overlap=500)
        assert len(rows) >= want
        rows = [rows[i] for i in sorted(rng.permutation(len(rows))[:want].tolist())]
    elif pattern == "many_reads":
        layout = [(700 * i, 3000 + int(rng.integers(0, 400)), int(rng.integers(0, 2))) for i in range(1500)]
        rows = [r for t in range(len(layout)) for q in range(max(0, t - 5), min(len(layout), t + 6)) if t != q
                for r in (layout_row(layout, t, q),) if r is not None]
    elif pattern == "random":
        layout = _random_layout(rng, 300, 150000, 2000, 9000)
        rows = layout_records(layout, min_overlap=300)
        keep = rng.permutation(len(rows))[:4000]
        rows = [rows[i] for i in sorted(keep.tolist())]
        rec = records_of(rows)
        # ends moved a little, as an aligner leaves them, some scores equal, some records not emitted
        for name in ("ab", "bb"):
            rec[name] += rng.integers(0, 60, len(rec))
        for name in ("ae", "be"):
            rec[name] -= rng.integers(0, 60, len(rec))
        rec["score"] = rng.integers(200, 260, len(rec))
        rec["emitted"] = rng.random(len(rec)) < 0.95
        lens = [ln for _, ln, _ in layout]
        clip = [(int(rng.integers(0, 200)), ln - int(rng.integers(0, 200))) for ln in lens]
        kw = dict(clip=np.array(clip, dtype=np.int32).reshape(-1), params=dict(max_hang=300, min_ovlp=600, fuzz=100))
        return _noise(rng, rec), np.array(lens, dtype=np.int32), kw
    elif pattern == "empty":
        layout = _random_layout(rng, 30, 20000, 3000, 7000)
        rows = [r[:8] + (0,) for r in layout_records(layout)]
    elif pattern in ("tiling128", "tiling129"):
        # the tiling with 128 and with 129 reads, strands at random: the 256 vertices of the one are the last that one chunk of
        # the degree scan holds, the last two of the other's 258 are the first that lie behind its carry
        layout = [(2000 * i, 5000, int(rng.integers(0, 2))) for i in range(int(pattern[6:]))]
        rows = [layout_row(layout, t, q) for t in range(len(layout)) for q in range(max(0, t - 2), min(len(layout), t + 3)) if t != q]
    else:
        raise ValueError(pattern)
    return _noise(rng, records_of(rows)), np.array([ln for _, ln, _ in layout], dtype=np.int32), kw
