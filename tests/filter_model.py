"""The filter of gact_hip_filter_overlaps in plain numpy, written from the rule in include/gact_hip.h, and the crafted record
sets that tests/test_filter_model.py and tests/test_gpu_filter.py share.

  chosen record k (records[sel[k]], record k without sel) with its summary sums[k]:
    cols = n_eq + n_x + ins_bases + del_bases, t_span = n_eq + n_x + del_bases, q_span = n_eq + n_x + ins_bases,
    ident = cols ? 1000 * n_eq // cols : 0
  why[k] = the first of: NOT_EMITTED (emitted == 0), EMPTY (cols == 0), IDENTITY (ident < min_identity), SPAN (min(t_span,
  q_span) < min_span), RELATIVE (max_drop < 1000 and best[x] - ident > max_drop for a read x the record names on a requested
  side; best[x]: the largest ident of the records that passed the four tests before and name x on a requested side), else KEPT.
  The table of reads [read_first, read_first + n_reads): counted records (emitted, cols > 0), passed ones, kept ones, best,
  and the sums of n_eq and cols over the passed ones; a record that names a read on both sides counts twice on it.
Lists and loops, no cleverness.  identity(), spans(), towards_best() and relative_sides() are the four places a kernel and a
model could misread together; tests/test_filter_model.py replaces each and sees a named assertion fail.  (Exchanging ins and
del in spans() shows in the t_span / q_span this model returns and nowhere else: the rule takes the shorter of the two, and
the entry returns no span, so the device's output cannot depend on it.)"""
import numpy as np

from gact_amd import engine

REF, QUERY, BOTH = 1, 2, 3
KEPT, NOT_EMITTED, EMPTY, IDENTITY, SPAN, RELATIVE = range(6)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)            # the wave and block edges of the ballot and the write
BIG = 70000                                             # more than 256 blocks of 256: the scan of the block counts loops


class Refused(ValueError):
    """what the entry refuses; code: "EINVAL" or "ERANGE" """
    def __init__(self, code, text):
        super().__init__(text)
        self.code = code


def identity(n_eq, n_x, ins, dele):
    cols = n_eq + n_x + ins + dele
    return 1000 * n_eq // cols if cols else 0


def spans(n_eq, n_x, ins, dele):
    """-> (t_span, q_span): a deleted base is a target base against a gap, an inserted base a query base against a gap"""
    return n_eq + n_x + dele, n_eq + n_x + ins


def towards_best(why):
    """does a record with this provisional reason count towards its reads' best?"""
    return why == KEPT


def relative_sides(sides):
    """the sides the relative test looks at"""
    return sides


def _named(ref, query, sides):
    return ([ref] if sides & REF else []) + ([query] if sides & QUERY else [])


def filter_overlaps(records, sums, sel=None, min_identity=650, min_span=0, max_drop=1000, sides=BOTH, n_reads=0, read_first=0):
    """-> dict(why int32 per chosen record, kept_at, kept_sel int32, reads FILTER_READ_DTYPE, ident, t_span, q_span per chosen
    record)"""
    if sums is None:
        raise Refused("EINVAL", "no summaries")
    if not 0 <= min_identity <= 1000 or min_span < 0 or not 0 <= max_drop <= 1000 or sides not in (REF, QUERY, BOTH):
        raise Refused("EINVAL", "a parameter out of range")
    if n_reads < 0 or (max_drop < 1000 and n_reads == 0):
        raise Refused("EINVAL", "no window for the relative test")
    n = len(records)
    chosen = list(range(n)) if sel is None else [int(i) for i in sel]
    assert len(sums) == len(chosen)
    for k, i in enumerate(chosen):
        if not 0 <= i < n:
            raise Refused("EINVAL", "sel[%d] = %d outside [0, %d)" % (k, i, n))
    f = {name: records[name].tolist() for name in ("ref_id", "query_id", "emitted")}
    s = {name: sums[name].tolist() for name in ("n_eq", "n_x", "ins_bases", "del_bases")}
    reads = np.zeros(n_reads, dtype=engine.FILTER_READ_DTYPE)
    table = [[0, 0, 0, 0, 0, 0] for _ in range(n_reads)]     # n_records, n_passed, n_kept, best, eq_sum, col_sum
    why, ident, t_spans, q_spans, named = [], [], [], [], []
    for k, i in enumerate(chosen):
        four = (s["n_eq"][k], s["n_x"][k], s["ins_bases"][k], s["del_bases"][k])
        cols = sum(four)
        idt = identity(*four)
        t_span, q_span = spans(*four)
        if not f["emitted"][i]:
            w = NOT_EMITTED
        elif cols == 0:
            w = EMPTY
        elif idt < min_identity:
            w = IDENTITY
        elif min(t_span, q_span) < min_span:
            w = SPAN
        else:
            w = KEPT
        xs = []
        if n_reads > 0 and w not in (NOT_EMITTED, EMPTY):
            xs = [x - read_first for x in _named(f["ref_id"][i], f["query_id"][i], sides)]
            for x in xs:
                if not 0 <= x < n_reads:
                    raise Refused("ERANGE", "chosen record %d names read %d outside [%d, %d)" % (k, x + read_first, read_first,
                                                                                                 read_first + n_reads))
            for x in xs:
                t = table[x]
                t[0] += 1
                if w == KEPT:
                    t[1] += 1
                    t[4] += four[0]
                    t[5] += cols
                if towards_best(w):
                    t[3] = max(t[3], idt)
        why.append(w); ident.append(idt); t_spans.append(t_span); q_spans.append(q_span); named.append(xs)
    for k, i in enumerate(chosen):
        if why[k] != KEPT or n_reads == 0:
            continue
        if max_drop < 1000:
            looked_at = [x - read_first for x in _named(f["ref_id"][i], f["query_id"][i], relative_sides(sides))]
            if any(table[x][3] - ident[k] > max_drop for x in looked_at):
                why[k] = RELATIVE
                continue
        for x in named[k]:
            table[x][2] += 1
    for x, t in enumerate(table):
        reads[x] = tuple(t)
    kept_at = [k for k, w in enumerate(why) if w == KEPT]
    return dict(why=np.array(why, dtype=np.int32), kept_at=np.array(kept_at, dtype=np.int32),
                kept_sel=np.array([chosen[k] for k in kept_at], dtype=np.int32), reads=reads,
                ident=np.array(ident, dtype=np.int64), t_span=np.array(t_spans, dtype=np.int64),
                q_span=np.array(q_spans, dtype=np.int64))


def records_of(rows):
    """[(ref_id, query_id, emitted)] -> OVERLAP_DTYPE records"""
    out = np.zeros(len(rows), dtype=engine.OVERLAP_DTYPE)
    for j, (ref, query, emitted) in enumerate(rows):
        out[j]["ref_id"], out[j]["query_id"], out[j]["emitted"] = ref, query, emitted
    return out


def sums_of(rows):
    """[(n_eq, n_x, ins_bases, del_bases)] -> SUMMARY_DTYPE summaries (one run of every kind that has a column)"""
    out = np.zeros(len(rows), dtype=engine.SUMMARY_DTYPE)
    for j, four in enumerate(rows):
        for name, runs, v in zip(("n_eq", "n_x", "ins_bases", "del_bases"), ("eq_runs", "x_runs", "ins_runs", "del_runs"), four):
            out[j][name], out[j][runs] = v, int(v > 0)
    return out


def hand_cases():
    """name -> (records, sums, kwargs of filter_overlaps, the expected why, {read of the window: its expected table row})"""
    cases = {}
    # ident exactly at the threshold and one under it, also where the division floors
    # and where a quarter of the columns are gaps
    cases["threshold"] = (records_of([(0, 1, 1)] * 6),
                          sums_of([(650, 350, 0, 0), (649, 351, 0, 0), (13, 7, 0, 0), (1299, 701, 0, 0), (650, 100, 125, 125), (649, 101, 125, 125)]),
                          dict(min_identity=650), [KEPT, IDENTITY, KEPT, IDENTITY, KEPT, IDENTITY], {})
    # no columns on an emitted record; records that are not emitted, named by sel, with and without columns; sel in no order
    cases["empty_and_not_emitted"] = (
        records_of([(0, 1, 1), (0, 1, 0), (1, 2, 1), (1, 2, 0), (2, 3, 1)]), sums_of([(0, 0, 0, 0), (0, 0, 0, 0), (90, 10, 0, 0), (90, 10, 0, 0)]),
        dict(sel=np.array([3, 0, 1, 2], dtype=np.int32), min_identity=0, n_reads=4, sides=BOTH),
        [NOT_EMITTED, EMPTY, NOT_EMITTED, KEPT],
        {0: (0, 0, 0, 0, 0, 0), 1: (1, 1, 1, 900, 90, 100), 2: (1, 1, 1, 900, 90, 100), 3: (0, 0, 0, 0, 0, 0)})
    # the span test takes the shorter of the two spans: ins != del, each way round; exactly at min_span
    cases["span"] = (records_of([(0, 1, 1)] * 4), sums_of([(80, 0, 30, 10), (80, 0, 10, 30), (90, 0, 10, 10), (80, 0, 30, 20)]),
                     dict(min_identity=0, min_span=100), [SPAN, SPAN, KEPT, KEPT], {})
    # the relative test exactly at max_drop and one over it
    cases["relative_at"] = (records_of([(9, 0, 1)] * 3), sums_of([(900, 100, 0, 0), (850, 150, 0, 0), (849, 151, 0, 0)]),
                            dict(min_identity=0, max_drop=50, sides=QUERY, n_reads=1), [KEPT, KEPT, RELATIVE],
                            {0: (3, 3, 2, 900, 2599, 3000)})
    # B (reads 1, 2) falls to A through its ref side and still is read 2's best: C (reads 2, 3) falls to B.  D (reads 3, 0)
    # falls to A through its query side only
    cases["relative_chain"] = (
        records_of([(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1)]), sums_of([(900, 100, 0, 0), (840, 160, 0, 0), (780, 220, 0, 0), (845, 155, 0, 0)]),
        dict(min_identity=0, max_drop=50, sides=BOTH, n_reads=4), [KEPT, RELATIVE, RELATIVE, RELATIVE],
        {0: (2, 2, 1, 900, 1745, 2000), 1: (2, 2, 1, 900, 1740, 2000), 2: (2, 2, 0, 840, 1620, 2000), 3: (2, 2, 0, 845, 1625, 2000)})
    # E (reads 4, 5) is nearly exact and too short: counted, not passed, and no part of read 5's best, so F (reads 5, 6) stays
    cases["best_of_passed"] = (
        records_of([(4, 5, 1), (5, 6, 1)]), sums_of([(99, 1, 0, 0), (900, 100, 0, 0)]),
        dict(min_identity=0, min_span=200, max_drop=50, sides=BOTH, n_reads=3, read_first=4), [SPAN, KEPT],
        {0: (1, 0, 0, 0, 0, 0), 1: (2, 1, 1, 900, 900, 1000), 2: (1, 1, 1, 900, 900, 1000)})
    # the three sides on the same records, in a window that begins at read 10; under REF and QUERY the other id is in no window
    rec = records_of([(10, 12, 1), (11, 12, 1), (10, 11, 1)])
    rec_far = rec.copy()
    sm = sums_of([(800, 200, 0, 0), (700, 300, 0, 0), (900, 100, 0, 0)])
    rec_far["query_id"] += 1000
    cases["side_ref"] = (rec_far, sm, dict(min_identity=0, max_drop=150, sides=REF, n_reads=3, read_first=10), [KEPT, KEPT, KEPT],
                         {0: (2, 2, 2, 900, 1700, 2000), 1: (1, 1, 1, 700, 700, 1000), 2: (0, 0, 0, 0, 0, 0)})
    rec_far = rec.copy()
    rec_far["ref_id"] -= 1000
    cases["side_query"] = (rec_far, sm, dict(min_identity=0, max_drop=50, sides=QUERY, n_reads=3, read_first=10), [KEPT, RELATIVE, KEPT],
                           {0: (0, 0, 0, 0, 0, 0), 1: (1, 1, 1, 900, 900, 1000), 2: (2, 2, 1, 800, 1500, 2000)})
    cases["side_both"] = (rec, sm, dict(min_identity=0, max_drop=150, sides=BOTH, n_reads=3, read_first=10), [KEPT, RELATIVE, KEPT],
                          {0: (2, 2, 2, 900, 1700, 2000), 1: (2, 2, 1, 900, 1600, 2000), 2: (2, 2, 1, 800, 1500, 2000)})
    # ref_id == query_id under BOTH: once per side
    cases["self"] = (records_of([(1, 1, 1), (0, 1, 1)]), sums_of([(70, 30, 0, 0), (80, 20, 0, 0)]),
                     dict(min_identity=0, sides=BOTH, n_reads=2), [KEPT, KEPT],
                     {0: (1, 1, 1, 800, 80, 100), 1: (3, 3, 3, 800, 220, 300)})
    return cases


def random_case(n_chosen, seed=20261021, with_sel=True, sides=BOTH, one_read=False, max_drop=60, n_reads=None):
    """-> (records, sums, kwargs): n_chosen chosen records whose identities lie on both sides of 650, one in eight not emitted,
    one in sixteen without columns, short ones among them; with sel, the records are twice as many and sel names them in no
    order, some twice.  one_read: every record names read 0 on its query side.  The same on every call"""
    rng = np.random.default_rng([seed, n_chosen, int(with_sel), sides, int(one_read)])
    n = 2 * n_chosen + 3 if with_sel else n_chosen
    n_reads = max(2, n_chosen // 6) if n_reads is None else n_reads
    read_first = 7
    rec = np.zeros(n, dtype=engine.OVERLAP_DTYPE)
    rec["ref_id"] = read_first + rng.integers(0, n_reads, n)
    rec["query_id"] = read_first if one_read else read_first + rng.integers(0, n_reads, n)
    rec["comp"] = rng.integers(0, 2, n)
    rec["emitted"] = rng.integers(0, 8, n) > 0
    rec["score"] = rng.integers(1, 9000, n)
    sel = rng.integers(0, n, n_chosen).astype(np.int32) if with_sel else None
    sums = np.zeros(n_chosen, dtype=engine.SUMMARY_DTYPE)
    cols = np.where(rng.integers(0, 4, n_chosen) == 0, rng.integers(1, 300, n_chosen), rng.integers(300, 6000, n_chosen))
    permille = np.where(rng.integers(0, 3, n_chosen) == 0, rng.integers(500, 600, n_chosen), rng.integers(600, 1001, n_chosen))
    sums["n_eq"] = cols * permille // 1000
    rest = cols - sums["n_eq"]
    sums["n_x"] = rest * rng.integers(0, 1001, n_chosen) // 1000
    rest = rest - sums["n_x"]
    sums["ins_bases"] = rest * rng.integers(0, 1001, n_chosen) // 1000
    sums["del_bases"] = rest - sums["ins_bases"]
    for name in ("eq_runs", "x_runs", "ins_runs", "del_runs"):
        sums[name] = rng.integers(1, 9, n_chosen)
    sums[rng.integers(0, 16, n_chosen) == 0] = np.zeros((), dtype=engine.SUMMARY_DTYPE)
    return rec, sums, dict(sel=sel, min_identity=650, min_span=200, max_drop=max_drop, sides=sides, n_reads=n_reads,
                           read_first=read_first)
