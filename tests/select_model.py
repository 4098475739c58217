"""The selection of gact_hip_select_overlaps in plain Python (include/gact_hip.h), and the crafted record sets that
tests/test_select_model.py and tests/test_gpu_select.py share.

  exact  class: emitted records that agree in ref_id, query_id, comp, ab, ae, bb, be, score; the lowest index survives
  pair   class: emitted records that agree in (ref_id, query_id, comp); the survivor has the highest score, then the largest
         (ae - ab) + (be - bb), then the lowest index
Records that were not emitted are never selected and enter no class."""
import numpy as np

from gact_amd import engine

MODES = ("exact", "pair")
EXACT_FIELDS = ("ref_id", "query_id", "comp", "ab", "ae", "bb", "be", "score")
PAIR_FIELDS = ("ref_id", "query_id", "comp")
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 70001)
PATTERNS = ("one_line", "one_pair", "distinct", "high_bits", "every_second", "none_emitted", "straddle", "ties", "mixed")


def select(records, mode):
    """-> the ascending int32 indices of the records that survive"""
    assert mode in MODES
    fields = EXACT_FIELDS if mode == "exact" else PAIR_FIELDS
    keys = list(zip(*(records[f].tolist() for f in fields)))
    emitted = records["emitted"].tolist()
    score = records["score"].tolist()
    span = ((records["ae"].astype(np.int64) - records["ab"]) + (records["be"].astype(np.int64) - records["bb"])).tolist()
    best = {}
    for i, key in enumerate(keys):
        if not emitted[i]:
            continue
        j = best.get(key)
        if j is None:
            best[key] = i
        elif mode == "pair" and (score[i], span[i]) > (score[j], span[j]):
            best[key] = i                       # (on a tie the earlier index stays: i > j here)
    return np.array(sorted(best.values()), dtype=np.int32)


def records_of(rows):
    """[(ref_id, query_id, comp, ab, ae, bb, be, score, emitted)] -> OVERLAP_DTYPE records"""
    out = np.zeros(len(rows), dtype=engine.OVERLAP_DTYPE)
    for k, row in enumerate(rows):
        for f, v in zip(EXACT_FIELDS + ("emitted",), row):
            out[k][f] = v
    return out


def crafted(pattern, n, seed=20261017):
    """n records of one of PATTERNS, the same for the same arguments.  Fields no class is made of (first_tile_score, n_tiles,
    cells) differ from record to record: the selection must not look at them."""
    rng = np.random.default_rng([seed, PATTERNS.index(pattern), n])
    r = np.zeros(n, dtype=engine.OVERLAP_DTYPE)
    idx = np.arange(n)
    r["emitted"] = 1
    r["first_tile_score"] = rng.integers(0, 320, n)
    r["n_tiles"] = rng.integers(1, 90, n)
    r["cells"] = rng.integers(1, 1 << 40, n)

    def coordinates(lo_span=1, hi_span=20000):
        r["ab"] = rng.integers(0, 5000, n)
        r["bb"] = rng.integers(0, 5000, n)
        r["ae"] = r["ab"] + rng.integers(lo_span, hi_span, n)
        r["be"] = r["bb"] + rng.integers(lo_span, hi_span, n)

    if pattern == "one_line":
        # every record prints the same line: one class in both modes, all contention on one table slot
        r["ref_id"], r["query_id"], r["comp"] = 7, 11, 1
        r["ab"], r["ae"], r["bb"], r["be"], r["score"] = 100, 9100, 40, 9000, 5000
    elif pattern == "one_pair":
        # one pair, scores from a narrow range and few spans: many ties at the top, broken by span and then by index
        r["ref_id"], r["query_id"], r["comp"] = 3, 2, 0
        r["score"] = rng.integers(900, 905, n)
        r["ab"] = rng.integers(0, 4, n)
        r["ae"] = 1000 + rng.integers(0, 3, n)
        r["bb"], r["be"] = 0, 1000
    elif pattern == "distinct":
        r["ref_id"] = rng.permutation(n)
        r["query_id"] = idx
        r["comp"] = idx & 1
        r["score"] = rng.integers(-50, 9000, n)
        coordinates()
    elif pattern == "high_bits":
        # ids whose low 16 bits are all zero; every pair twice, with different coordinates
        k = idx // 2
        r["ref_id"] = (k & 0x7fff) << 16
        r["query_id"] = (k >> 15) << 16
        r["score"] = rng.integers(100, 110, n)
        coordinates()
    elif pattern == "every_second":
        # the records that were not emitted have the best scores and the longest spans of their pairs
        r["ref_id"] = idx // 6
        r["query_id"] = (idx // 6) * 3 + 1
        r["score"] = rng.integers(100, 104, n)
        coordinates(1, 50)
        off = (idx & 1) == 1
        r["emitted"][off] = 0
        r["score"][off] += 1000
        r["ae"][off] += 100000
    elif pattern == "none_emitted":
        r["ref_id"] = idx // 3
        r["query_id"] = idx // 3 + 1
        r["score"] = rng.integers(0, 100, n)
        coordinates()
        r["emitted"] = 0
    elif pattern == "straddle":
        # distinct records, and around every multiple of 64 (wave ends; every fourth is a block end) a run of five exact
        # duplicates: indices 64 m - 2 .. 64 m + 2, so 63/64 and 255/256 are inside a run
        r["ref_id"] = idx
        r["query_id"] = idx + 1
        r["score"] = rng.integers(0, 9000, n)
        coordinates()
        for b in range(64, n, 64):
            lo, hi = b - 2, min(n, b + 3)
            for f in EXACT_FIELDS:
                r[f][lo:hi] = r[f][lo]
    elif pattern == "ties":
        # the members of a class are spread over the array and tie on score and on span, with different coordinates: each
        # is a class of its own in exact mode, and in pair mode the lowest index wins
        classes = max(1, n // 7)
        r["ref_id"] = idx % classes
        r["query_id"] = (idx % classes) ^ 0x10000
        r["comp"] = (idx % classes) & 1
        r["score"] = 4000
        r["ab"] = rng.integers(0, 1000, n)
        r["bb"] = rng.integers(0, 1000, n)
        shift = rng.integers(0, 300, n)
        r["ae"] = r["ab"] + 6000 + shift
        r["be"] = r["bb"] + 6000 - shift
    elif pattern == "mixed":
        # what a run gives, denser: few pairs, both strands, narrow score and span ranges, a fifth not emitted, and a third of
        # the records exact copies of an earlier one
        pairs = max(1, n // 5)
        r["ref_id"] = rng.integers(0, pairs, n)
        r["query_id"] = r["ref_id"] + rng.integers(1, 3, n)
        r["comp"] = rng.integers(0, 2, n)
        r["score"] = rng.integers(2000, 2004, n)
        coordinates(5000, 5004)
        r["emitted"] = rng.random(n) >= 0.2
        for k in np.flatnonzero(rng.random(n) < 1 / 3).tolist():
            if k:
                src = int(rng.integers(0, k))
                for f in EXACT_FIELDS:
                    r[f][k] = r[f][src]
    else:
        raise ValueError(pattern)
    return r
