"""The placement of gact_hip_place_reads in plain Python over numpy records (include/gact_hip.h), and the crafted record sets
that tests/test_place_model.py and tests/test_gpu_place.py share.

  chosen   records sel[0..n_sel) (sel None: all), k = the position in that list; sums[k] goes with chosen record k
  counted  emitted, and the interval GACT_COVER_QUERY puts on the original read is not empty -- cover_model.intervals makes it
  order    per query read: higher score, larger (ae - ab) + (be - bb), lower k; rank = the position in that order
  walk     in rank order against the parents in the order they were made: p masks t iff ov > 0 and 1000 ov >= mask_permille *
           min(len t, len p); the first masking parent adopts t (SECONDARY); else t is a parent while fewer than 64 exist
           (PRIMARY the first, SUPPLEMENTARY the others); else EXTRA, which masks nothing
  mapq     of a parent: s1 its score, s2 the best score of its secondaries (0 without any) clamped to [0, s1];
           mapq = 0 if s1 <= 0 else mapq_cap * (s1 - s2) // s1
One loop per read, no cleverness."""
import functools

import numpy as np

import cover_model
from gact_amd import engine

NONE, PRIMARY, SUPPLEMENTARY, SECONDARY, EXTRA = range(5)
MAX_PARENTS = 64
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000)
SIZED = ("chain", "stack", "ties", "ties_perm", "ties_repeat", "strand", "clip", "not_emitted", "sums", "random")
PERMILLES = (0, 1, 500, 999, 1000)
CAPS = (0, 60, 255)
FIXED = tuple(("threshold", p) for p in PERMILLES) + tuple(("mapq", c) for c in CAPS) + \
        (("abut", None), ("late_mask", None), ("many_reads", None), ("one_read", None))
# every crafted case: (pattern, its size or parameter)
CASES = tuple((p, m) for p in SIZED for m in SIZES + ((66,) if p == "chain" else ())) + FIXED


def query_intervals(records, read_lens, read_first=0, sel=None, sums=None):
    """-> {k: (read of the window, begin, end)} of the counted chosen records.  IndexError: a sel index outside the records;
    ValueError: an emitted chosen record whose query_id is outside the window.  The interval itself is cover_model's: every
    chosen record is handed to it as the one record of a read of its own, which has its read's length"""
    lens = np.asarray(read_lens, dtype=np.int64)
    n = len(records)
    chosen = np.arange(n, dtype=np.int64) if sel is None else np.asarray(sel, dtype=np.int64)
    if len(chosen) and not ((chosen >= 0) & (chosen < n)).all():
        raise IndexError("sel holds an index outside [0, %d)" % n)
    mine = records[chosen].copy()
    q = mine["query_id"].astype(np.int64) - read_first
    inside = (q >= 0) & (q < len(lens))
    if (mine["emitted"].astype(bool) & ~inside).any():
        raise ValueError("an emitted chosen record names a read outside the window")
    own_lens = np.zeros(len(chosen), dtype=np.int64)
    own_lens[inside] = lens[q[inside]]
    mine["query_id"] = np.arange(len(chosen))
    return {k: (int(q[k]), b, e) for k, b, e in cover_model.intervals(mine, own_lens, None, sums, cover_model.QUERY)}


def mapq_of(s1, s2, mapq_cap):
    return 0 if s1 <= 0 else mapq_cap * (s1 - s2) // s1


def place(records, read_lens, read_first=0, sel=None, sums=None, mask_permille=500, mapq_cap=60):
    """-> (PLACE_DTYPE array, one per chosen record; READ_PLACE_DTYPE array, one per read of the window)"""
    assert 0 <= mask_permille <= 1000 and 0 <= mapq_cap <= 255
    iv = query_intervals(records, read_lens, read_first, sel, sums)
    chosen = range(len(records)) if sel is None else [int(i) for i in sel]
    score = records["score"].tolist()
    span = ((records["ae"].astype(np.int64) - records["ab"]) + (records["be"].astype(np.int64) - records["bb"])).tolist()
    out = np.zeros(len(chosen), dtype=engine.PLACE_DTYPE)
    out["parent"] = out["rank"] = -1
    reads = np.zeros(len(read_lens), dtype=engine.READ_PLACE_DTYPE)
    reads["primary"] = -1
    per_read = [[] for _ in range(len(read_lens))]
    for k in sorted(iv):
        per_read[iv[k][0]].append(k)

    def compare(a, b):
        ia, ib = chosen[a], chosen[b]
        if score[ia] != score[ib]:
            return -1 if score[ia] > score[ib] else 1
        if span[ia] != span[ib]:
            return -1 if span[ia] > span[ib] else 1
        return -1 if a < b else 1

    for read, ks in enumerate(per_read):
        if not ks:
            continue
        parents, best_child, counts = [], {}, {SUPPLEMENTARY: 0, SECONDARY: 0, EXTRA: 0, PRIMARY: 0}
        for rank, t in enumerate(sorted(ks, key=functools.cmp_to_key(compare))):
            _, bt, et = iv[t]
            kind, parent = None, t
            for p in parents:
                _, bp, ep = iv[p]
                ov = min(et, ep) - max(bt, bp)
                if ov > 0 and 1000 * ov >= mask_permille * min(et - bt, ep - bp):
                    kind, parent = SECONDARY, p
                    best_child[p] = max(best_child.get(p, 0), score[chosen[t]])
                    break
            if kind is None:
                if len(parents) < MAX_PARENTS:
                    kind = SUPPLEMENTARY if parents else PRIMARY
                    parents.append(t)
                else:
                    kind = EXTRA
            counts[kind] += 1
            out[t] = (kind, 0, parent, rank)
        for p in parents:
            s1 = score[chosen[p]]
            s2 = max(0, min(s1, best_child.get(p, 0)))
            out[p]["mapq"] = mapq_of(s1, s2, mapq_cap)
            if p == parents[0]:
                reads[read] = (len(ks), p, counts[SUPPLEMENTARY], counts[SECONDARY], counts[EXTRA], s1, s2, out[p]["mapq"])
    return out, reads


def stats_of(place_out, reads):
    """what gact_hip_last_place_stats counts, from a result"""
    kind = place_out["kind"]
    return dict(reads=len(reads), max_records=int(reads["n_records"].max()) if len(reads) else 0, counted=int((kind != NONE).sum()),
                parents=int(((kind == PRIMARY) | (kind == SUPPLEMENTARY)).sum()), secondaries=int((kind == SECONDARY).sum()),
                extras=int((kind == EXTRA).sum()))


def records_of(rows):
    """[(ref_id, query_id, comp, ab, ae, bb, be, score, emitted)] -> OVERLAP_DTYPE records"""
    out = np.zeros(len(rows), dtype=engine.OVERLAP_DTYPE)
    if rows:
        cols = np.array(rows, dtype=np.int64).T
        for name, col in zip(("ref_id", "query_id", "comp", "ab", "ae", "bb", "be", "score", "emitted"), cols):
            out[name] = col
    return out


def _random_records(rng, lens, read_first, per_read, slack=20, scores=(-50, 3000)):
    """per_read[i] records on read read_first + i, read after read: query intervals on or a little over the read's ends, either
    strand, spans that differ a little from the intervals', scores from a range narrow enough for ties"""
    ids = np.repeat(np.arange(len(lens)), per_read)
    n = len(ids)
    length = np.asarray(lens, dtype=np.int64)[ids]
    r = np.zeros(n, dtype=engine.OVERLAP_DTYPE)
    r["ref_id"] = rng.integers(0, 6, n)
    r["query_id"] = ids + read_first
    r["comp"] = rng.integers(0, 2, n)
    lo = rng.integers(-slack, length + 1)
    r["bb"] = lo
    r["be"] = lo + rng.integers(0, length + 2 * slack + 1 - lo)
    r["ab"] = rng.integers(0, 5000, n)
    r["ae"] = r["ab"] + np.maximum(0, (r["be"] - r["bb"]) + rng.integers(-3, 4, n))
    r["score"] = rng.integers(scores[0], scores[1], n)
    r["emitted"] = 1
    r["first_tile_score"] = rng.integers(0, 320, n)
    r["n_tiles"] = rng.integers(1, 90, n)
    r["cells"] = rng.integers(1, 1 << 40, n)
    return r


def crafted(pattern, m=None, seed=20261020):
    """-> dict(records, read_lens, and the keyword arguments of place()) of one of CASES, the same on every call"""
    names = SIZED + tuple(dict.fromkeys(p for p, _ in FIXED))
    rng = np.random.default_rng([seed, names.index(pattern), 0 if m is None else m])
    kw = {}
    if pattern == "chain":
        # read 3: m disjoint intervals of 10, scores in no order; read 4: five of them.  All parents, from the 65th on extras
        lens, kw["read_first"] = [10 * m + 10, 60], 3
        order = rng.permutation(m)
        rows = [(0, 3, 0, 10 * j, 10 * j + 10, 10 * j, 10 * j + 10, 1000 + int(order[j]), 1) for j in range(m)]
        rows += [(1, 4, 0, 0, 10, 10 * j, 10 * j + 10, 5 - j, 1) for j in range(min(m, 5))]
        rec = records_of(rows)
    elif pattern == "stack":
        # one interval m times: a primary and its secondaries
        lens = [500, 7]
        rec = records_of([(j % 3, 0, 0, 100, 400, 50, 350, 0, 1) for j in range(m)])
        rec["score"] = rng.integers(1, 5000, m)
    elif pattern in ("ties", "ties_perm", "ties_repeat"):
        # equal scores and spans on three intervals, two of which overlap by more than half: the order is k's
        lens, kw["read_first"] = [1000], 1
        at = (0, 300, 340)
        rec = records_of([(0, 1, 0, 0, 200, at[j % 3], at[j % 3] + 200, 77, 1) for j in range(m)])
        if pattern == "ties_perm":
            kw["sel"] = rng.permutation(m).astype(np.int32)
        if pattern == "ties_repeat":
            kw["sel"] = rng.integers(0, max(m, 1), m + 3 if m else 0).astype(np.int32)      # (some index comes twice)
    elif pattern == "strand":
        # comp == 1 on reads of odd and even length
        lens = [1001, 1000, 1, 2]
        rec = _random_records(rng, lens, 0, [m, m, min(m, 3), min(m, 3)])
        rec["comp"] = 1
    elif pattern == "clip":
        # intervals that reach over the read's ends or lie wholly outside it
        lens, kw["read_first"] = [300, 40], 2
        rec = _random_records(rng, lens, 2, [m, m], slack=200)
    elif pattern == "not_emitted":
        lens, kw["read_first"] = [800, 900], 5
        rec = _random_records(rng, lens, 5, [m, (m + 1) // 2])
        rec["emitted"] = np.arange(len(rec)) & 1
        rec["query_id"][::4] = 99                                  # (outside the window, and not emitted: never looked at)
    elif pattern == "sums":
        # the summaries move the begins; sums[k] goes with sel[k], and one summary has no columns
        lens = [2000, 1500, 1800]
        rec = _random_records(rng, lens, 0, [m, m // 2, 3], scores=(0, 200))
        sel = rng.permutation(len(rec))[:max(1, (2 * len(rec)) // 3)].astype(np.int32)
        sums = np.zeros(len(sel), dtype=engine.SUMMARY_DTYPE)
        for name in ("n_eq", "n_x", "ins_bases", "del_bases"):
            sums[name] = rng.integers(0, 300, len(sel))
        for name in ("eq_runs", "x_runs", "ins_runs", "del_runs"):
            sums[name] = rng.integers(1, 9, len(sel))
        sums[len(sel) // 2] = np.zeros((), dtype=engine.SUMMARY_DTYPE)
        kw.update(sel=sel, sums=sums)
    elif pattern == "random":
        lens, kw["read_first"] = rng.integers(1, 4000, 9).tolist(), 11
        rec = _random_records(rng, lens, 11, rng.integers(0, 2 * m + 1, 9), scores=(-5, 60))
        rec = rec[rng.permutation(len(rec))]
        rec["emitted"] = rng.integers(0, 8, len(rec)) > 0
    elif pattern == "threshold":
        # pairs whose overlap is exactly what the mask needs, one base less, one base more
        permille, lens, rows = m, [], []
        for shorter in (1000, 999, 7, 1):
            need = -(-permille * shorter // 1000)                 # the least ov with 1000 ov >= permille * shorter
            for ov in (need - 1, need, need + 1):
                if ov > shorter:
                    continue
                read = len(lens)
                lens.append(5000)
                rows += [(0, read, 0, 0, 2000, 1000, 3000, 100, 1),                            # the longer one, the parent
                         (1, read, 0, 0, shorter, 3000 - ov, 3000 - ov + shorter, 50, 1)]
        rec, kw["mask_permille"] = records_of(rows), permille
    elif pattern == "mapq":
        big = 2 ** 31 - 1
        lens = [100] * 8
        #        ref query comp ab ae  bb  be  score
        rows = [(0, 0, 0, 0, 50, 0, 50, 0, 1),                     # s1 == 0
                (0, 1, 0, 0, 50, 0, 50, -5, 1),                    # s1 < 0, and a secondary below it
                (1, 1, 0, 0, 50, 0, 50, -9, 1),
                (0, 2, 0, 0, 50, 0, 50, 40, 1),                    # s2 == s1
                (1, 2, 0, 0, 50, 0, 50, 40, 1),
                (0, 3, 0, 0, 50, 0, 50, 10, 1),                    # s2 < 0: counts as 0
                (1, 3, 0, 0, 50, 0, 50, -3, 1),
                (0, 4, 0, 0, 50, 0, 50, big, 1),                   # the product needs 64 bits
                (1, 4, 0, 0, 50, 0, 50, 1, 1),
                (0, 5, 0, 0, 50, 0, 50, big, 1),
                (1, 5, 0, 0, 50, 0, 50, big - 1, 1),
                (0, 6, 0, 0, 50, 0, 50, 1000, 1),                  # two secondaries: the better one is s2
                (1, 6, 0, 0, 50, 0, 50, 400, 1),
                (2, 6, 0, 0, 50, 5, 50, 700, 1),
                (0, 7, 0, 0, 40, 0, 40, 90, 1),                    # a supplementary with a secondary of its own
                (1, 7, 0, 0, 40, 60, 100, 80, 1),
                (2, 7, 0, 0, 40, 60, 100, 20, 1)]
        rec, kw["mapq_cap"] = records_of(rows), m
    elif pattern == "abut":
        lens = [100, 192]
        rows = [(0, 0, 0, 0, 50, 0, 50, 9, 1), (1, 0, 0, 0, 50, 50, 100, 8, 1)]
        rows += [(j, 1, j & 1, 0, 64, 64 * j, 64 * j + 64, 5, 1) for j in range(3)]
        rec, kw["mask_permille"] = records_of(rows), 0
    elif pattern == "late_mask":
        # 64 parents; a record that only the 64th masks; an extra; a record that only that extra would have masked
        lens = [8000]
        rows = [(0, 0, 0, 0, 100, 100 * j, 100 * j + 100, 5000 - j, 1) for j in range(64)]
        rows += [(1, 0, 0, 0, 80, 6310, 6390, 300, 1), (2, 0, 0, 0, 100, 7000, 7100, 200, 1), (3, 0, 0, 0, 100, 7000, 7100, 100, 1)]
        rec = records_of(rows)
    elif pattern == "many_reads":
        # the scan crosses blocks and its last block is partial; the records in no order
        lens = (40 + np.arange(70001) % 130).tolist()
        rec = _random_records(rng, lens, 0, rng.integers(0, 4, 70001), slack=5, scores=(0, 40))
        half = len(rec) // 2
        rec[half:] = rec[half:][rng.permutation(len(rec) - half)]
    elif pattern == "one_read":
        # the chunked ranking crosses 64 chunks
        lens, kw["read_first"] = [100000, 10], 7
        rec = _random_records(rng, lens, 7, [4097, 0], scores=(0, 500))
        rec["be"] = np.minimum(rec["be"], rec["bb"] + rng.integers(50, 500, len(rec)))
    else:
        raise ValueError(pattern)
    return dict(records=rec, read_lens=np.array(lens, dtype=np.int32), **kw)
