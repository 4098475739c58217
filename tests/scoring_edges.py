"""The edges of the packed int16 kernels' scoring guards, shared by the CPU and GPU suites.

Five host predicates decide, per scoring and tile size, which int16 kernels may run: p16_scoring_ok (any packed main launch),
p16_tagged_ok (tagged pointers), p16_argmax_ok (the packed seed launch), p16_lin_ok (the linear-gap pass) and p16_aff_ok
(the drifted affine pass).  EDGES holds, for each of them and several geometries, the last scoring a guard admits and the
first one past it, with the plan engine.plan gives for both.  The numbers are written out on purpose: a change to any
predicate must be a deliberate change to this table.

edge_reads() builds the reads that push a kernel's intermediate values to their extremes at a given tile size: exact
copies (every tile scores match * tile), copies with one indel per tile advance (gap-rich paths), disjoint alphabets
(every cell a mismatch), homopolymers and two-letter repeats (all three moves tie), reads of boundary lengths and reads
with N (the raw-byte kernels), on both strands."""
from collections import namedtuple

import numpy as np

from gact_amd import synth

S = 3 * 256 * 32          # resident tile slots of the default grid on 256 CUs: a count of 2 * S takes the split layout

# seed: the seed launch's kernel; split / wide: the main kernel at a count of 2 * S / of 100 ("-": int32-one-launch)
Plan = namedtuple("Plan", "seed split wide")
Edge = namedtuple("Edge", "name tile overlap guard last past at_last at_past")

_XS = "extend_kernel(seed)"
_LIN, _TAG, _PLAIN = ("SplitLayoutLin", "WideLayoutLin"), ("SplitLayout<tag>", "WideLayoutTagged"), ("SplitLayout", "WideLayout")


def _p(seed, mains):
    return Plan(seed, *mains)


EDGES = [
    # ---- 320 / 120: the default geometry
    Edge("lin-match-320", 320, 120, "p16_lin_ok", (18, -1, -1, -1), (19, -1, -1, -1), _p(_XS, _LIN), _p(_XS, _TAG)),
    Edge("lin-drift-320", 320, 120, "p16_lin_ok", (1, -12, -12, -12), (1, -13, -13, -13),
         _p("seed_p16<lin>", _LIN), _p("seed_p16", _TAG)),
    Edge("seed-320", 320, 120, "p16_argmax_ok", (6, -1, -1, -1), (7, -1, -1, -1), _p("seed_p16<lin>", _LIN), _p(_XS, _LIN)),
    Edge("aff-cbneg-320", 320, 120, "p16_aff_ok", (16, -3, -5, -2), (17, -3, -5, -2),
         _p(_XS, ("SplitLayoutAff<cbneg>", "WideLayoutTagged")), _p(_XS, _TAG)),
    Edge("tagged-320", 320, 120, "p16_tagged_ok", (24, -3, -5, -2), (25, -3, -5, -2), _p(_XS, _TAG), _p(_XS, _PLAIN)),
    Edge("p16-320", 320, 120, "p16_scoring_ok", (37, -3, -5, -2), (38, -3, -5, -2), _p(_XS, _PLAIN), _p(_XS, ("-", "-"))),
    Edge("aff-open-320", 320, 120, "p16_aff_ok", (1, -1, -1000, -1), (1, -1, -1001, -1),
         _p("seed_p16<aff>", ("SplitLayoutAff", "WideLayoutTagged")), _p("seed_p16", _PLAIN)),
    Edge("aff-drift-320", 320, 120, "p16_aff_ok", (1, -11, -13, -11), (1, -12, -14, -12),
         _p("seed_p16<aff>", ("SplitLayoutAff", "WideLayoutTagged")), _p("seed_p16", _TAG)),
    # ---- 320 / 100: early 220 is past the split layout's second region, the uniform layout
    Edge("tagged-320u", 320, 100, "p16_tagged_ok", (24, -3, -5, -2), (25, -3, -5, -2),
         _p(_XS, ("UniformLayout<tag>", "WideLayoutTagged")), _p(_XS, ("UniformLayout", "WideLayout"))),
    Edge("p16-320u", 320, 100, "p16_scoring_ok", (37, -3, -5, -2), (38, -3, -5, -2),
         _p(_XS, ("UniformLayout", "WideLayout")), _p(_XS, ("-", "-"))),
    # ---- 200 / 100
    Edge("lin-match-200", 200, 100, "p16_lin_ok", (30, -1, -1, -1), (31, -1, -1, -1), _p(_XS, _LIN), _p(_XS, _TAG)),
    Edge("lin-drift-200", 200, 100, "p16_lin_ok", (1, -16, -16, -16), (1, -17, -17, -17),
         _p("seed_p16<lin>", _LIN), _p("seed_p16", _TAG)),
    Edge("seed-200", 200, 100, "p16_argmax_ok", (10, -1, -1, -1), (11, -1, -1, -1), _p("seed_p16<lin>", _LIN), _p(_XS, _LIN)),
    # ---- 128 / 32
    Edge("lin-match-128", 128, 32, "p16_lin_ok", (47, -1, -1, -1), (48, -1, -1, -1), _p(_XS, _LIN), _p(_XS, _TAG)),
    Edge("lin-drift-128", 128, 32, "p16_lin_ok", (1, -20, -20, -20), (1, -21, -21, -21),
         _p("seed_p16<lin>", _LIN), _p("seed_p16", _TAG)),
    Edge("seed-128", 128, 32, "p16_argmax_ok", (15, -1, -1, -1), (16, -1, -1, -1), _p("seed_p16<lin>", _LIN), _p(_XS, _LIN)),
    Edge("aff-cbneg-128", 128, 32, "p16_aff_ok", (44, -3, -5, -2), (45, -3, -5, -2),
         _p(_XS, ("SplitLayoutAff<cbneg>", "WideLayoutTagged")), _p(_XS, _TAG)),
    Edge("tagged-128", 128, 32, "p16_tagged_ok", (60, -3, -5, -2), (61, -3, -5, -2), _p(_XS, _TAG), _p(_XS, _PLAIN)),
    Edge("p16-128", 128, 32, "p16_scoring_ok", (92, -3, -5, -2), (93, -3, -5, -2), _p(_XS, _PLAIN), _p(_XS, ("-", "-"))),
    # ---- 64 / 8 (the linear-gap pass is stopped by match - ext <= 63 first, and 63 - (-1) is past the tagged form too)
    Edge("lin-match-64", 64, 8, "p16_lin_ok", (62, -1, -1, -1), (63, -1, -1, -1), _p(_XS, _LIN), _p(_XS, _PLAIN)),
    Edge("lin-drift-64", 64, 8, "p16_lin_ok", (1, -26, -26, -26), (1, -27, -27, -27),
         _p("seed_p16<lin>", _LIN), _p("seed_p16", _TAG)),
    Edge("seed-64", 64, 8, "p16_argmax_ok", (31, -1, -1, -1), (32, -1, -1, -1), _p("seed_p16<lin>", _LIN), _p(_XS, _LIN)),
    # ---- 512 / 128: 32 columns per lane, uniform layout only
    Edge("tagged-512", 512, 128, "p16_tagged_ok", (15, -1, -1, -1), (16, -1, -1, -1),
         _p(_XS, ("UniformLayout<tag>",) * 2), _p(_XS, ("UniformLayout",) * 2)),
    Edge("p16-512", 512, 128, "p16_scoring_ok", (23, -1, -1, -1), (24, -1, -1, -1),
         _p(_XS, ("UniformLayout",) * 2), _p(_XS, ("-", "-"))),
]


def scorings():
    """every scoring of the table, each once"""
    out = []
    for e in EDGES:
        for sc in (e.last, e.past):
            if (e.tile, e.overlap, sc) not in out:
                out.append((e.tile, e.overlap, sc))
    return out


def threshold(edge, scoring):
    """a first-tile threshold that exact copies pass and unrelated reads do not: some candidates emit, some stop"""
    return max(1, scoring[0] * edge.tile // 4)


# ---------------------------------------------------------------------------------------------------------------------
class _Read:
    """fwd: the read in genome orientation, gpos[i]: the genome position of fwd[i] (None: not from the genome)"""

    def __init__(self, fwd, gpos, strand, kind):
        self.fwd, self.gpos, self.strand, self.kind = fwd, gpos, strand, kind
        self.seq = synth.revcomp(fwd) if strand else fwd

    def coord(self, g, rc=False):
        """the coordinate of genome position g in the read (rc: in its reverse complement)"""
        i = int(min(np.searchsorted(self.gpos, g), len(self.fwd) - 1))
        return len(self.fwd) - 1 - i if bool(self.strand) != rc else i


def _gap_copy(rng, src, gsrc, every, run=(1, 9), point=0.01):
    """src with one insertion or deletion of 1-8 bases every `every` bases and a few point errors; returns (seq, gpos)"""
    out, pos, i = [], [], 0
    nxt = int(rng.integers(every // 2, every))
    while i < len(src):
        if i >= nxt:
            n = int(rng.integers(*run))
            if rng.random() < 0.5:
                i += n                                                           # deletion
            else:
                out.extend(rng.choice(list(b"ACGT"), n).tolist())               # insertion
                pos.extend([gsrc[i]] * n)
            nxt = i + every
            continue
        b = int(src[i])
        if rng.random() < point:
            b = int(rng.choice(list(b"ACGT")))
        out.append(b)
        pos.append(gsrc[i])
        i += 1
    return np.array(out, dtype=np.uint8), np.array(pos, dtype=np.int64)


def _with_n(rng, seq, frac=0.01):
    seq = seq.copy()
    seq[rng.choice(len(seq), max(1, int(len(seq) * frac)), replace=False)] = ord("N")
    return seq


class EdgeReads:
    """the adversarial read set of one tile geometry: rs (synth.ReadSet), and per strand the candidate lists
    clean_f / clean_r (reads of A, C, G and T only) and raw_f / raw_r (at least one read holds N); exact_f / exact_r:
    which clean candidates sit on the true diagonal of two exact copies, at least a tile away from both reads' starts"""


def edge_reads(tile, overlap, seed=0):
    rng = np.random.default_rng(1000 + tile * 7 + overlap + seed)
    T, A = tile, tile - overlap
    G = 14 * T + 500
    genome = rng.choice(list(b"ACGT"), G).astype(np.uint8)
    reads = []

    def copy(a, b, strand, kind="exact"):
        reads.append(_Read(genome[a:b].copy(), np.arange(a, b), strand, kind))

    # exact copies, overlapping by several tiles, both strands
    for k, a in enumerate((0, 3 * T // 2, 3 * T, 9 * T // 2)):
        copy(a, a + 6 * T, k % 2)
    # gap runs: one indel per tile advance
    for k, (a, b) in enumerate(((T // 2, 13 * T // 2), (2 * T, 8 * T))):
        seq, pos = _gap_copy(rng, genome[a:b], np.arange(a, b), max(A, 8))
        reads.append(_Read(seq, pos, k % 2, "gap"))
    # boundary lengths next to the first exact copy
    for k, n in enumerate((T - 1, T, T + 1, 2 * T - overlap - 1, 2 * T - overlap + 1)):
        a = T // 3 + 37 * k
        copy(a, a + n, k % 2, "short")
    # with N
    for k, (a, b) in enumerate(((T, 5 * T), (4 * T, 9 * T))):
        r = _Read(_with_n(rng, genome[a:b]), np.arange(a, b), k % 2, "n")
        reads.append(r)
    # disjoint alphabets: A/C reads against G/T reads (and A/C against A/C on the complement strand: rc(A/C) is G/T)
    n_g = len(reads)
    for alpha in (b"AC", b"AC", b"GT"):
        reads.append(_Read(rng.choice(list(alpha), 4 * T).astype(np.uint8), None, 0, "disjoint"))
    # homopolymers and two-letter repeats
    for s in (b"A" * (3 * T), b"A" * (2 * T + 7), b"AC" * (3 * T // 2), b"CA" * (T + 5), b"AACC" * T):
        reads.append(_Read(np.frombuffer(s, dtype=np.uint8).copy(), None, 0, "repeat"))

    rs = synth.ReadSet()
    rs.genome = genome
    for k, r in enumerate(reads):
        rs.reads.append(r.seq)
        rs.names.append("E%d_%s" % (k, r.kind))

    lists = {(rc, raw): [] for rc in (False, True) for raw in (False, True)}
    exact = {False: [], True: []}

    def add(ri, qi, rp, qp, rc, on_diag=False):
        L, M = len(reads[ri].seq), len(reads[qi].seq)
        raw = "n" in (reads[ri].kind, reads[qi].kind)
        lists[(rc, raw)].append((ri, qi, min(max(rp, 0), L), min(max(qp, 0), M - 1)))
        if not raw:
            exact[rc].append(on_diag)

    for ri in range(n_g):
        for qi in range(n_g):
            r, q = reads[ri], reads[qi]
            lo, hi = max(r.gpos[0], q.gpos[0]), min(r.gpos[-1], q.gpos[-1]) + 1
            if hi - lo < T // 2 and "short" not in (r.kind, q.kind):
                continue
            if hi <= lo:
                continue
            rc = r.strand != q.strand
            both_exact = r.kind in ("exact", "short") and q.kind in ("exact", "short")
            for g in sorted({lo + T // 2, (lo + hi) // 2, hi - T // 2, lo, hi - 1}):
                if not lo <= g < hi:
                    continue
                rp, qp = r.coord(g), q.coord(g, rc=rc)
                if r.kind == "gap" or q.kind == "gap":
                    qp += int(rng.integers(-8, 9))
                diag = both_exact and min(rp, qp) >= T
                add(ri, qi, rp, qp, rc, diag)
            if "short" in (r.kind, q.kind):              # read starts and ends (the records' edge cases)
                L, M = len(r.seq), len(q.seq)
                for rp, qp in ((0, 0), (L, M - 1), (L, 0), (0, M - 1)):
                    add(ri, qi, rp, qp, rc)
    # disjoint alphabets and repeats: positions inside, near the ends and at the very ends, on both strands
    for ri in range(n_g, len(reads)):
        for qi in range(n_g, len(reads)):
            r, q = reads[ri], reads[qi]
            if r.kind != q.kind:
                continue
            L, M = len(r.seq), len(q.seq)
            for rp, qp in ((L // 2, M // 2), (T + 3, T), (L, M - 1), (3, 1)):
                for rc in (False, True):
                    add(ri, qi, rp, qp, rc)

    out = EdgeReads()
    out.rs = rs
    for rc, name in ((False, "f"), (True, "r")):
        setattr(out, "clean_" + name, np.array(lists[(rc, False)], dtype=synth.CAND_DTYPE))
        setattr(out, "raw_" + name, np.array(lists[(rc, True)], dtype=synth.CAND_DTYPE))
        setattr(out, "exact_" + name, np.array(exact[rc], dtype=bool))
    return out


def adversarial_tiles(tile, overlap, seed=0):
    """(ref, query, reverse, first) tiles for the single-tile aligners: exact copies, gap runs, disjoint alphabets,
    homopolymers, two-letter repeats, boundary lengths and N"""
    rng = np.random.default_rng(77 + tile + seed)
    T = tile
    g = bytes(rng.choice(list(b"ACGT"), 3 * T).astype(np.uint8))
    gap, _ = _gap_copy(rng, np.frombuffer(g, dtype=np.uint8), np.arange(len(g)), max(tile - overlap, 8))
    gap = gap.tobytes()
    ac = bytes(rng.choice(list(b"AC"), T).astype(np.uint8))
    gt = bytes(rng.choice(list(b"GT"), T).astype(np.uint8))
    nn = _with_n(rng, np.frombuffer(g[:T], dtype=np.uint8), 0.02).tobytes()
    tiles = [
        (g[:T], g[:T], 0, 1), (g[:T], g[:T], 1, 0), (g[T:2 * T], g[T:2 * T], 0, 0),
        (g[:T], gap[:T], 0, 1), (gap[T:2 * T], g[T:2 * T], 1, 1),
        (ac, gt, 0, 1), (gt, ac, 1, 0),
        (b"A" * T, b"A" * T, 0, 1), ((b"AC" * T)[:T], (b"CA" * T)[:T], 1, 1), ((b"AACC" * T)[:T], b"A" * T, 0, 0),
        (g[:T - 1], g[:T], 0, 1), (g[:T], g[1:T + 1], 1, 0), (g[:T], g[:T - 1], 0, 0), (nn, g[:T], 0, 1),
    ]
    return tiles
