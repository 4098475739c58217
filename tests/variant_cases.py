"""Planted cases for gact_hip_pileup_variants, shared by the CPU and GPU suites.

A window's targets are random sequences.  The queries of a target are d exact copies of it, of which `a` carry every edit
planted on that target: a substituted base, a run of bases left out, a few bases put in.  Every candidate is anchored in the
middle of the target's longest stretch without an edit, so every copy aligns across every planted site away from the target's
ends, and there alt == a and depth == d exactly.  With the default linear gap score a gap of n bases and n gaps of one base score the same, so any left-out
base that equals the base in front of the run or the one behind it could stay in that one's place, and the chain would split the
run.  The bases at an edit are therefore chosen so that no part of a gap can move: a left-out run is made of two letters and the
two bases around it of the other two; an inserted base is neither of its two neighbours; a substituted base neither.

The sites aim at the edges of the kernels of csrc/gact_variants.hpp.  A position's lane is its WINDOW position mod 64 and its
chunk its window position / CHUNK, so the targets that carry such sites are the first of their window: sites at 0, 63, 64,
CHUNK - 1, CHUNK and the last base; runs that start at lane 63, end at lane 0, cover a whole 64-step, cross a chunk's edge, and
lie behind the chunk's edge where the write pass peeks; target lengths 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1 and
2 CHUNK + 200; a window of several targets, with one of length 1 and one that nothing aligns to, behind the queries (so that
read_first > 0).

A substituted base at a target's first or last base (or the one beside it) is planted too, and makes no record: the chain ends
where its score is highest, in front of a mismatch that nothing follows, so those copies do not reach the counts there and the
position's depth is d - a.  Sites that do make a record, 4 and length - 5, stand beside them.
What an alignment cannot make at all is not here: a deleted position at a sequence's first or last base (no chain begins or ends with a
gap), hence a run that ends at a sequence's last base with the next sequence starting deleted.  The rule for those is held on
hand-made counts (tests/test_variant_model.py)."""
from collections import namedtuple

import numpy as np

from gact_amd import engine, synth

CHUNK = engine.VARIANT_CHUNK
THRESHOLD = 1                                   # of the first tile: a target of one base aligns too
K = 2                                           # ins_slots of the windows with insertions
CLIPPED = 1                                     # a substituted base this close to a target's end is clipped by the chain: no record
LONGEST_RUN = 130                               # the longest left-out run planted (the chain model carries it: test_variant_model.py)

# name, the window (read_first, n_reads), candidates (all forward), ins_slots, the rule's parameters, and the records the
# edits were planted for: (seq, pos, kind, len, bases, alt, depth, flags), in the stated order
Case = namedtuple("Case", "name rs window cands ins_slots params want")

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _other(rng, *avoid):
    """a base that is none of `avoid`"""
    left = [b for b in _ACGT.tolist() if b not in avoid]
    return left[int(rng.integers(0, len(left)))]


class _Window:
    def __init__(self, name, seed, d, a, ins_slots=0, queries_first=False, hom_permille=750):
        self.name, self.rng, self.d, self.a, self.ins_slots, self.queries_first = name, np.random.default_rng(seed), d, a, ins_slots, queries_first
        self.params = dict(min_depth=d, min_alt=max(a, 1), min_permille=250, hom_permille=hom_permille)
        self.targets, self.queries, self.want = [], [], []          # queries: (bytes, target, ref_pos, query_pos)

    def gt(self, a):
        return 2 if 1000 * a >= self.params["hom_permille"] * self.d else 1

    def target(self, length, edits=(), aligned=True, a=None):
        """edits: ("snv", pos), ("del", pos, len), ("ins", pos, n), apart from each other; a: the copies that carry them"""
        rng, a = self.rng, self.a if a is None else a
        t = _ACGT[rng.integers(0, 4, length)].copy()
        tid = len(self.targets)
        edits = sorted(edits, key=lambda e: e[1])
        for e in edits:                                 # the target's bases at the gaps, so that no part of a gap can move
            if e[0] == "del":
                p, n = e[1], e[2]
                assert 0 < p and p + n < length
                letters = rng.permutation(_ACGT)
                t[p:p + n] = letters[:2][rng.integers(0, 2, n)]
                t[p - 1], t[p + n] = letters[2:][rng.integers(0, 2, 2)]
        pieces, at, shift, want, spans = [], 0, [], [], []
        for e in edits:
            p = e[1]
            pieces.append(t[at:p])
            if e[0] == "snv":
                # (none of its neighbours either: two substituted bases side by side must not read as a gap, a match and a gap)
                b = _other(rng, t[p], t[p - 1] if p else None, t[p + 1] if p + 1 < length else None)
                pieces.append(np.array([b], np.uint8))
                at = p + 1
                if CLIPPED < p < length - 1 - CLIPPED:
                    want.append((tid, p, engine.VARIANT_SNV, 1, b, a, self.d, self.gt(a)))
                spans.append((p, p + 1))
            elif e[0] == "del":
                at = p + e[2]
                shift.append((p, -e[2]))
                want.append((tid, p, engine.VARIANT_DEL, e[2], 0, a, self.d, self.gt(a)))
                spans.append((p, p + e[2]))
            else:
                n = e[2]
                assert 0 < p < length and self.ins_slots
                block = np.array([_other(rng, t[p], t[p - 1]) for _ in range(n)], np.uint8)
                pieces.append(block)
                at = p
                shift.append((p, n))
                kept = min(n, self.ins_slots)
                bases = sum(int(block[j]) << (8 * j) for j in range(kept))
                want.append((tid, p, engine.VARIANT_INS, kept, bases, a, self.d,
                             self.gt(a) | (engine.VARIANT_TRUNCATED if kept == self.ins_slots else 0)))
                spans.append((p, p))
        pieces.append(t[at:])
        edited = np.concatenate(pieces)
        self.targets.append(t)
        if not aligned:
            return tid
        # the anchor: the middle of the longest stretch without an edit
        free = [(0, spans[0][0])] + [(spans[k][1], spans[k + 1][0]) for k in range(len(spans) - 1)] + [(spans[-1][1], length)] if spans else [(0, length)]
        lo, hi = max(free, key=lambda s: s[1] - s[0])
        anchor = (lo + hi) // 2 if length > 1 else 0
        moved = anchor + sum(n for p, n in shift if p <= anchor)
        for k in range(self.d):
            carries = k < a and len(edits) > 0
            self.queries.append((edited if carries else t.copy(), tid, anchor, moved if carries else anchor))
        if a > 0:
            self.want += want
        return tid

    def case(self):
        rs = synth.ReadSet()
        n_t, n_q = len(self.targets), len(self.queries)
        t_first, q_first = (n_q, 0) if self.queries_first else (0, n_t)
        seqs = ([q[0] for q in self.queries] + self.targets) if self.queries_first else (self.targets + [q[0] for q in self.queries])
        for k, s in enumerate(seqs):
            rs.reads.append(np.ascontiguousarray(s, dtype=np.uint8))
            rs.names.append("%s%d" % ("q" if (k < n_q) == self.queries_first else "t", k))
        cands = np.array([(t_first + tid, q_first + k, rp, qp) for k, (_, tid, rp, qp) in enumerate(self.queries)], dtype=engine.CAND_DTYPE)
        want = np.array([(t_first + w[0],) + w[1:] for w in sorted(self.want, key=lambda w: (w[0], w[1], w[2], w[4]))],
                        dtype=engine.VARIANT_DTYPE) if self.want else np.zeros(0, dtype=engine.VARIANT_DTYPE)
        assert sum(len(s) for s in seqs) <= 50000 and self.d <= 8
        return Case(self.name, rs, (t_first, n_t), cands, self.ins_slots, self.params, want)


_CASES = {}


def cases():
    """name -> Case, made once"""
    if _CASES:
        return _CASES
    made = []
    # one target of every length, an SNV at each of 0, 63, 64, CHUNK - 1, CHUNK and the last base that it has
    for k, length in enumerate((63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 200)):
        deep = length <= 65
        w = _Window("snv-L%d" % length, 100 + k, d=8 if deep else 4, a=4 if deep else 2)
        sites = sorted({p for p in (0, 4, 63, 64, CHUNK - 1, CHUNK, length - 5, length - 1) if p < length})
        w.target(length, [("snv", p) for p in sites])
        made.append(w)
    w = _Window("one-base", 120, d=8, a=0)
    w.target(1)
    made.append(w)
    # all reads differ: 1/1; and the boundary of hom_permille: 3 of 4 at 750 is 1/1, at 751 it is 0/1
    w = _Window("hom", 121, d=4, a=4)
    w.target(500, [("snv", 100), ("del", 200, 2)])
    made.append(w)
    for hom in (750, 751):
        w = _Window("three-of-four-at-%d" % hom, 122, d=4, a=3, hom_permille=hom)
        w.target(500, [("snv", 100), ("del", 300, 3)])
        made.append(w)
    # runs: 1; 2 from lane 63 to lane 0; 64 over a whole step; 130 that begins in front of the first chunk's edge and goes on for
    # a step and a half behind it (the write pass's peek takes two steps); 65 across the second chunk's edge
    w = _Window("runs", 130, d=4, a=2)
    w.target(2 * CHUNK + 200, [("del", 500, 1), ("del", 1023, 2), ("del", 1600, 64), ("del", CHUNK - 30, LONGEST_RUN),
                               ("del", 2 * CHUNK - 60, 65)])
    made.append(w)
    # a run that ends at a chunk's last position, one that begins at a chunk's first, one that ends at lane 63 of a step inside
    w = _Window("runs-at-edges", 131, d=4, a=2)
    w.target(2 * CHUNK + 200, [("del", CHUNK - 65, 65), ("del", 2 * CHUNK, 64), ("del", 1000, 24), ("del", 1535, 65)])
    made.append(w)
    # insertions of 1, K and K + 1 bases; at lane 0, at lane 63, in front of a chunk's first position
    w = _Window("ins", 140, d=4, a=2, ins_slots=K)
    w.target(CHUNK + 300, [("ins", 200, 1), ("ins", 640, K), ("ins", 1087, K + 1), ("ins", CHUNK, 1), ("snv", 1500), ("del", 2000, 3)])
    made.append(w)
    # several targets behind their queries: one base; nothing aligned; edits near both ends of neighbours
    w = _Window("several", 150, d=4, a=2, ins_slots=K, queries_first=True)
    w.target(1)
    w.target(300, [("del", 280, 4), ("snv", 40)])
    w.target(200, aligned=False)
    w.target(65, [("snv", 30)])
    w.target(CHUNK, [("del", 20, 2), ("ins", 600, K + 1), ("snv", CHUNK - 40), ("del", CHUNK - 20, 5)])
    w.target(700, [("ins", 30, 1), ("del", 300, 70)], a=4)
    made.append(w)
    for w in made:
        _CASES[w.name] = w.case()
    return _CASES


def own_and_offsets(case):
    """the window's own bytes and where its sequences begin in them"""
    first, n = case.window
    seqs = case.rs.reads[first:first + n]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return (np.concatenate(seqs) if n else np.zeros(0, np.uint8)), offs
