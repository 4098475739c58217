"""The per-read coverage of gact_hip_read_coverage in plain numpy (include/gact_hip.h), and the crafted record sets that
tests/test_cover_model.py and tests/test_gpu_cover.py share.

  a counted record (emitted, and named by sel where sel is given) puts [ab, ae) on read ref_id (sides & 1) and [bb, be) of its
  strand on read query_id (sides & 2): [bb, be) for comp == 0, [len - be, len - bb) for comp == 1; with summaries the begins
  are ae - (n_eq + n_x + del_bases) and be - (n_eq + n_x + ins_bases); every interval is clipped to its read and dropped when
  empty; the depth of a position is the number of intervals that hold it.
A difference array and a cumsum per read, no cleverness."""
import numpy as np

from gact_amd import engine

REF, QUERY, BOTH = 1, 2, 3
PATTERNS = ("lengths", "chunk_edges", "ties", "abut", "clip", "strand", "stack", "many_reads", "not_emitted", "not_emitted_sel",
            "sums", "random", "empty")
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097)
CHUNK_RUNS = ((0, 63), (64, 128), (129, 130), (191, 321), (900, 1000))


def intervals(records, read_lens, sel=None, sums=None, sides=BOTH):
    """-> [(read, begin, end)] of the counted records, clipped, the empty ones dropped.  IndexError: a sel index outside the
    records; ValueError: a read id outside the reads"""
    lens = [int(v) for v in read_lens]
    n = len(records)
    chosen = range(n) if sel is None else [int(i) for i in sel]
    f = {name: records[name].tolist() for name in ("ref_id", "query_id", "ab", "ae", "bb", "be", "comp", "emitted")}
    out = []

    def put(read, b, e):
        if not 0 <= read < len(lens):
            raise ValueError("read %d outside [0, %d)" % (read, len(lens)))
        b, e = max(b, 0), min(e, lens[read])
        if b < e:
            out.append((read, b, e))

    for k, i in enumerate(chosen):
        if not 0 <= i < n:
            raise IndexError("sel[%d] = %d outside [0, %d)" % (k, i, n))
        if not f["emitted"][i]:
            continue
        ab, ae, bb, be = f["ab"][i], f["ae"][i], f["bb"][i], f["be"][i]
        if sums is not None:
            s = sums[k]
            m = int(s["n_eq"]) + int(s["n_x"])
            ab, bb = ae - (m + int(s["del_bases"])), be - (m + int(s["ins_bases"]))
        if sides & REF:
            put(f["ref_id"][i], ab, ae)
        if sides & QUERY:
            q = f["query_id"][i]
            if not 0 <= q < len(lens):
                raise ValueError("read %d outside [0, %d)" % (q, len(lens)))
            if f["comp"][i]:
                bb, be = lens[q] - be, lens[q] - bb
            put(q, bb, be)
    return out


def longest_run(mask):
    """the leftmost longest run of True: (begin, end), (0, 0) when there is none"""
    if not mask.any():
        return 0, 0
    d = np.diff(np.concatenate(([0], mask.astype(np.int8), [0])))
    begins, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    k = int(np.argmax(ends - begins))                  # (the first of equal maxima)
    return int(begins[k]), int(ends[k])


def cover(records, read_lens, sel=None, sums=None, sides=BOTH, min_depth=3):
    """-> (COVER_DTYPE array, one per read; int32 depth of every position, read after read)"""
    assert sides in (REF, QUERY, BOTH) and min_depth >= 1
    lens = np.asarray(read_lens, dtype=np.int64)
    assert (lens >= 0).all()
    start = np.concatenate(([0], np.cumsum(lens)))
    per_read = [[] for _ in lens]
    for read, b, e in intervals(records, lens, sel, sums, sides):
        per_read[read].append((b, e))
    out = np.zeros(len(lens), dtype=engine.COVER_DTYPE)
    depth = np.zeros(int(start[-1]), dtype=np.int32)
    for i, iv in enumerate(per_read):
        n = int(lens[i])
        out[i]["n_intervals"] = len(iv)
        if not iv or not n:
            continue
        diff = np.zeros(n + 1, dtype=np.int64)
        b, e = np.array(iv, dtype=np.int64).T
        np.add.at(diff, b, 1)
        np.add.at(diff, e, -1)
        d = np.cumsum(diff[:n])
        depth[start[i]:start[i] + n] = d
        out[i]["max_depth"] = d.max()
        out[i]["covered"] = int((d >= 1).sum())
        out[i]["well_covered"] = int((d >= min_depth).sum())
        out[i]["span_begin"], out[i]["span_end"] = longest_run(d >= min_depth)
        out[i]["depth_sum"] = int(d.sum())
    return out, depth


def records_of(rows):
    """[(ref_id, query_id, comp, ab, ae, bb, be, emitted)] -> OVERLAP_DTYPE records"""
    out = np.zeros(len(rows), dtype=engine.OVERLAP_DTYPE)
    if rows:
        cols = np.array(rows, dtype=np.int64).T
        for name, col in zip(("ref_id", "query_id", "comp", "ab", "ae", "bb", "be", "emitted"), cols):
            out[name] = col
    return out


def _random_records(rng, lens, n, comp=True, slack=40):
    """n records between two different reads with coordinates on or a little over the reads' ends; the fields no interval is
    made of differ from record to record"""
    lens = np.asarray(lens, dtype=np.int64)
    r = np.zeros(n, dtype=engine.OVERLAP_DTYPE)
    r["ref_id"] = rng.integers(0, len(lens), n)
    r["query_id"] = (r["ref_id"] + rng.integers(1, len(lens), n)) % len(lens)
    r["comp"] = rng.integers(0, 2, n) if comp else 0
    for b, e, ids in (("ab", "ae", "ref_id"), ("bb", "be", "query_id")):
        length = lens[r[ids]]
        lo = rng.integers(-slack, length + 1)
        r[b] = lo
        r[e] = lo + rng.integers(0, length + slack + 1 - lo + slack)
    r["emitted"] = 1
    r["score"] = rng.integers(-50, 9000, n)
    r["first_tile_score"] = rng.integers(0, 320, n)
    r["n_tiles"] = rng.integers(1, 90, n)
    r["cells"] = rng.integers(1, 1 << 40, n)
    return r


def crafted(pattern, seed=20261018):
    """-> (records, read_lens int32, kwargs of cover()) of one of PATTERNS, the same on every call"""
    rng = np.random.default_rng([seed, PATTERNS.index(pattern)])
    kw = {}
    if pattern == "lengths":
        # every read: three intervals over all of it, three over its first base, three over its last one
        lens = list(LENGTHS)
        rows = []
        for i, n in enumerate(lens):
            other = (i + 1) % len(lens)
            for b, e in ((0, n), (0, 1), (n - 1, n)):
                rows += [(i, other, 0, b, e, 0, 0, 1)] * 3
        rec, kw = records_of(rows), dict(sides=REF)
    elif pattern == "chunk_edges":
        # one interval over the whole read, and three over every run of CHUNK_RUNS: depth 4 on the runs, 1 elsewhere
        lens = [1000, 10]
        rows = [(0, 1, 0, 0, 1000, 0, 0, 1)]
        for b, e in CHUNK_RUNS:
            rows += [(0, 1, 0, b, e, 0, 0, 1)] * 3
        rec, kw = records_of(rows), dict(sides=REF)
    elif pattern == "ties":
        # read 0: three runs of 100; read 1: the same, the last run one base longer
        lens = [700, 700]
        rows = []
        for read, last in ((0, 600), (1, 601)):
            for b, e in ((10, 110), (200, 300), (500, last)):
                rows += [(read, 1 - read, 0, b, e, 0, 0, 1)] * 3
        rec, kw = records_of(rows), dict(sides=REF)
    elif pattern == "abut":
        # [0, k) and [k, len) three deep, k on a chunk edge and off it
        lens = [500, 500, 64]
        rows = []
        for read, k in ((0, 64), (1, 77), (2, 63)):
            rows += [(read, (read + 1) % 3, 0, 0, k, 0, 0, 1), (read, (read + 1) % 3, 0, k, lens[read], 0, 0, 1)] * 3
        rec, kw = records_of(rows), dict(sides=REF)
    elif pattern == "clip":
        lens = [100, 100, 50]
        #        ref query comp  ab   ae   bb   be
        rows = [(0, 1, 0, -5, 40, 10, 20, 1),        # ab < 0: [0, 40) on read 0; [10, 20) on read 1
                (0, 1, 0, 60, 130, 90, 120, 1),      # ae > len: [60, 100); be > len: [90, 100)
                (0, 1, 0, 50, 30, 5, 6, 1),          # ab > ae: dropped; [5, 6)
                (0, 1, 0, 100, 140, -20, 0, 1),      # wholly outside on both sides: both dropped
                (0, 2, 1, 10, 20, -10, 30, 1),       # [10, 20); comp: [20, 60) of read 2 clips to [20, 50)
                (0, 2, 1, 0, 1, 45, 70, 1),          # [0, 1); comp: [-20, 5) clips to [0, 5)
                (0, 2, 1, 0, 1, 60, 80, 1)]          # [0, 1); comp: [-30, -10) is outside: dropped
        rec, kw = records_of(rows), dict(sides=BOTH, min_depth=1)
    elif pattern == "strand":
        lens = rng.integers(200, 3000, 20).tolist()
        rec = _random_records(rng, lens, 400)
        rec["comp"] = np.arange(400) & 1
    elif pattern == "stack":
        lens = [40000]
        rec = np.zeros(70001, dtype=engine.OVERLAP_DTYPE)
        rec["ae"], rec["emitted"] = 40000, 1
        rec["score"] = rng.integers(0, 9000, len(rec))
        kw = dict(sides=REF)
    elif pattern == "many_reads":
        lens = (1 + np.arange(70001) % 130).tolist()
        rec = _random_records(rng, lens, 100000, slack=5)
        kw = dict(min_depth=2)
    elif pattern in ("not_emitted", "not_emitted_sel"):
        rng = np.random.default_rng([seed, 1000])                     # (the same records with and without sel)
        lens = rng.integers(300, 2000, 10).tolist()
        rec = _random_records(rng, lens, 200)
        rec["emitted"] = 1 - (np.arange(200) & 1)
        if pattern == "not_emitted_sel":
            kw = dict(sel=np.arange(0, 200, 3, dtype=np.int32))       # names emitted and not emitted ones
        kw["min_depth"] = 2
    elif pattern == "sums":
        # the summaries move the begins (left or right of ab / bb); sums[k] goes with sel[k], and sel is in no order
        lens = rng.integers(500, 3000, 8).tolist()
        rec = _random_records(rng, lens, 60)
        sel = rng.permutation(60)[:40].astype(np.int32)
        sums = np.zeros(40, dtype=engine.SUMMARY_DTYPE)
        for name in ("n_eq", "n_x", "ins_bases", "del_bases"):
            sums[name] = rng.integers(0, 400, 40)
        for name in ("eq_runs", "x_runs", "ins_runs", "del_runs"):
            sums[name] = rng.integers(1, 9, 40)
        sums[7] = np.zeros((), dtype=engine.SUMMARY_DTYPE)            # no columns: both intervals empty
        rec["emitted"][sel[7]] = 1
        kw = dict(sel=sel, sums=sums, min_depth=2)
    elif pattern == "random":
        lens = rng.integers(1, 20001, 300).tolist()
        rec = _random_records(rng, lens, 5000)
    elif pattern == "empty":
        lens = rng.integers(1, 500, 30).tolist()
        rec = _random_records(rng, lens, 100)
        rec["emitted"] = 0
    else:
        raise ValueError(pattern)
    return rec, np.array(lens, dtype=np.int32), kw
