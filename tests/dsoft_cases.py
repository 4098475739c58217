"""Seeded, named inputs of the D-SOFT filter for the paths its earlier tests never reached: a case is a read set, which is
reference set and query set at once (`same_file`: every read meets itself on diagonal 0), and the filter's parameters.
Both strands of every read are queried.  tests/test_dsoft_model.py proves on the model's trace (tests/dsoft_model.py)
that a case reaches the path it is here for; tests/test_gpu_dsoft_edges.py runs the same cases on the device.

k <= 12 everywhere: the device's direct table is 4^k words.  (num_seeds + 1) * max_occ stays under 26,000, which keeps
a wave's band table at 32,768 slots.
"""
import random

import dsoft_model

DEFAULTS = dict(seed_size=14, bin_size=64, window_size=4, threshold=21, num_seeds=800, seed_occurence_multiple=32,
                max_candidates=1000000)


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate(rng, seq, rate):
    return bytes(rng.choice(b"ACGT") if rng.random() < rate else c for c in seq)


class Case:
    def __init__(self, name, reads, **params):
        self.name, self.reads = name, [bytes(r) for r in reads]
        self.rc = [dsoft_model.revcomp(r) for r in self.reads]
        self.params = dict(DEFAULTS, **params)
        self._model = None

    def model(self):
        """(strand-major list, forward traces, reverse traces, per-query forward lists, per-query reverse lists), once"""
        if self._model is None:
            ix = dsoft_model.Index(self.reads, **self.params)
            fw = [ix.query(q) for q in self.reads]
            rv = [ix.query(q) for q in self.rc]
            self._model = (dsoft_model.strand_major([r[0] for r in fw], [r[0] for r in rv]), [r[1] for r in fw],
                           [r[1] for r in rv], [r[0] for r in fw], [r[0] for r in rv])
        return self._model

    def traces(self):
        m = self.model()
        return m[1] + m[2]

    def ref_len(self):
        """length of the padded concatenation"""
        b = self.params["bin_size"]
        return sum((len(r) + b - 1) // b * b for r in self.reads)

    def max_occ(self):
        return self.params["seed_occurence_multiple"] * (1 + (self.ref_len() >> (2 * self.params["seed_size"])))

    def band_slots(self):
        """slots of a wave's band table on the device (dsoft_engine.hpp): the order in which two cases share an engine"""
        size = 1024
        while size * 4 < (self.params["num_seeds"] + 1) * self.max_occ() * 5:
            size *= 2
        return size


def _many_hits(bin_size):
    """k = 8 and 128 kb of reference: max_occ = 64 * (1 + (131072 >> 16)) = 192.  Reads 0..3 start with tandem repeats
    of 100 and 150 copies, so their seeds have 65..128 and more than 128 hits, 37 or 23 bases apart: one bin at
    bin_size 4096, mostly different bins at 64.  num_seeds = 120 keeps a strand inside the repeats."""
    rng = random.Random(8001)
    m37, m23, shared = rand_seq(rng, 37), rand_seq(rng, 23), rand_seq(rng, 300)
    reads = [m37 * 100 + rand_seq(rng, 800),
             m23 * 150 + shared + rand_seq(rng, 500),
             mutate(rng, m37 * 20, 0.03) + shared + m23 * 12 + rand_seq(rng, 900),
             rand_seq(rng, 301) + mutate(rng, shared, 0.05) + m37 * 9]
    while sum(-(-len(r) // bin_size) * bin_size for r in reads) < 131072 + bin_size:
        reads.append(rand_seq(rng, rng.randrange(9000, 16000)))
    return Case("many_hits_bin%d" % bin_size, reads, seed_size=8, window_size=4, bin_size=bin_size, threshold=21,
                num_seeds=120, seed_occurence_multiple=64)


def _low_threshold(name, threshold):
    """threshold <= k: a bin crosses on its first hit, new and crossed in the same step"""
    rng = random.Random(8002)
    core = rand_seq(rng, 700)
    reads = [rand_seq(rng, 150) + core + rand_seq(rng, 277), mutate(rng, core, 0.08) + rand_seq(rng, 333),
             rand_seq(rng, 41) + mutate(rng, core[200:], 0.15), rand_seq(rng, 611),
             dsoft_model.revcomp(core[100:500]) + rand_seq(rng, 90)]
    return Case(name, reads, seed_size=10, window_size=4, threshold=threshold, num_seeds=60)


def _full_counter():
    """threshold + k = 255, the largest the device's 8-bit counter allows: a read, a copy of it and a bin larger than
    both, so one bin collects every seed until the count stands at 243 or more"""
    rng = random.Random(8003)
    a = rand_seq(rng, 2200)
    return Case("full_counter", [a, a, mutate(rng, a, 0.02) + rand_seq(rng, 150), rand_seq(rng, 900), dsoft_model.revcomp(a)],
                seed_size=12, window_size=4, bin_size=4096, threshold=243, num_seeds=800)


def _padding_reads(rng):
    reads = [rand_seq(rng, 300) + b"A" * 90 + rand_seq(rng, 211), rand_seq(rng, 130) + b"N" * 70 + rand_seq(rng, 255),
             b"A" * 150 + rand_seq(rng, 95), rand_seq(rng, 77) + b"a" * 64 + rand_seq(rng, 40) + b"T" * 120,
             b"N" * 45 + rand_seq(rng, 400), rand_seq(rng, 333)]
    return reads


def _padding():
    """k + w = 12 < 16, read lengths that are no multiple of 64, poly-A, poly-T and N stretches, and an occurrence cap
    of 512 that the all-A seed stays under: candidates whose hit lies in another read's padding, some beyond the
    read's length (clamped).  With k + w < 16 the index also holds the 16 - k - w positions at and past the padded
    length (seed_pos_table.cpp:60); the seeds there are all-A whatever the last read ends on, and hash32(0) is their
    windows' minimum here, so the poly-A strands hit them and emit candidates from them.  The reference is not
    defined for those strands: it stops at assert(hit < ref_size_) (seed_pos_table.cpp:134), and built without
    assertions it looks bin_to_chr_id up one bin past the last (darwin.cpp:217).  Those are 4 of the 14 strands and
    they carry nearly all of this case's candidates, its padding hits and clamps among them: here those paths are
    held by model, host and device against each other, and against the reference in `padding_k12`."""
    rng = random.Random(8004)
    reads = _padding_reads(rng) + [rand_seq(rng, 64 * 5 - 1)]
    return Case("padding", reads, seed_size=8, window_size=4, bin_size=64, threshold=21, num_seeds=40,
                seed_occurence_multiple=512)


def _padding_k12():
    """the same reads at k + w = 16: no position at or past the padded length is indexed (16 * (1 + length/16) - 16 <=
    length), so a hit past it is unreachable and the reference defines every strand; padding hits and the clamp remain"""
    rng = random.Random(8004)
    reads = _padding_reads(rng) + [rand_seq(rng, 64 * 5 - 1)]
    return Case("padding_k12", reads, seed_size=12, window_size=4, bin_size=64, threshold=21, num_seeds=40,
                seed_occurence_multiple=512)


def seed_kmer(seq, p, k, w):
    """(start, hash) of the k-mer that is the seed at position p: the minimum of the k-mers at p - w + 1 .. p"""
    seq = bytes(seq) + b"A" * (k + w)
    code = lambda m: sum(dsoft_model.two_bit(c) << (2 * j) for j, c in enumerate(seq[m:m + k]))
    return min((dsoft_model.hash32(code(m), k), -m) for m in range(max(p - w + 1, 0), p + 1))[::-1]


def stairs(rng, seq, spans, k, w):
    """a read that holds, for every (first, last) pair of seed positions of `seq`, the bases from the k-mer that is
    seed `first` to the k-mer that is seed `last` and nothing else of `seq`, between stretches of 80 to 149 random
    bases drawn again until both k-mers are minimizers of the read as well.  No seed before `first` has its k-mer
    there, and every span lies further along its own diagonal than the span before it, by more than a bin of 64: seed
    `first` is the first to meet the span's bin."""
    seq, out = bytes(seq) + b"A" * (k + w), b""
    for first, last in spans:
        (m0, v0), (m1, v1) = seed_kmer(seq, first, k, w), seed_kmer(seq, last, k, w)
        m0, m1 = -m0, -m1
        while True:
            piece = rand_seq(rng, rng.randrange(80, 150)) + seq[m0:m1 + k] + rand_seq(rng, 48)
            if {v0, v1} <= {v for _, v in dsoft_model.minimizers(piece, len(piece) // 16, k, w)}:
                break
        out += piece
    return out + rand_seq(rng, 70)


def seed_positions(seq, k, w):
    return [p for p, _ in dsoft_model.minimizers(seq, (len(seq) + 15) // 16, k, w)]


def chunk_edge(positions):
    """n such that seed n is the last of its 256-position chunk, not the only one in it, and seed n + 1 exists"""
    for n in range(1, len(positions) - 1):
        if positions[n] // 256 != positions[n + 1] // 256 and positions[n - 1] // 256 == positions[n] // 256:
            return n
    raise AssertionError("no chunk edge among the seeds")


def _seed_cut_reads():
    """read 0 and relatives of it, and a read of stairs (see there) for read 0's seeds 1 and 2 and for the five seeds
    around the end of its first 256-position chunk: at threshold <= k each of those seeds crosses a bin of its own, so
    the list tells one seed more or fewer apart"""
    rng = random.Random(8005)
    a = rand_seq(rng, 1500)
    pos = seed_positions(a, 11, 4)
    n = chunk_edge(pos)
    spans = [(pos[1], pos[1]), (pos[1], pos[2]), (pos[2], pos[2])] + [(pos[m], pos[m]) for m in range(n - 2, n + 3)]
    return [a, mutate(rng, a[300:], 0.05) + rand_seq(rng, 200), rand_seq(rng, 700) + a[:600], rand_seq(rng, 1000),
            dsoft_model.revcomp(a[:800]), stairs(rng, a, spans, 11, 4)]


def _seed_cut(name, num_seeds, threshold=11):
    """num_seeds + 1 seeds are applied.  threshold = k: a seed crosses every bin it is the first to hit; k + 1
    (seed_cut_1): a bin needs two seeds"""
    return Case(name, _seed_cut_reads(), seed_size=11, window_size=4, threshold=threshold, num_seeds=num_seeds)


def seed_cut_at_chunk_edge(first_of_next):
    """num_seeds for which the seed that read 0's forward strand is refused at (the cut) is the last seed under the cap
    of a 256-position chunk, or the first of the next chunk; chosen from the model's trace"""
    n = chunk_edge(_seed_cut("probe", 10 ** 6).model()[1][0].passing)
    refused = n + 1 if first_of_next else n                  # seeds 0 .. num_seeds are applied
    return refused - 1


def scanned(length, k, w):
    """`end`: the positions 0 .. end - 1 of a query are scanned for minimizers"""
    return 16 * ((length + 15) // 16) - k - w


def _lengths(name, seed_size, window_size, want_end):
    """queries one short of, at and past every boundary of the query side: k + w, the 16-base words and the
    256-position chunks (`end` = 16 * words - k - w positions are scanned).  The two reads scanned to `want_end` are
    cut from `base` where both of their strands have a minimizer at the last scanned position, and a read of stairs
    (see there) holds that seed's k-mer alone: at threshold = k it crosses a bin there, so a scan that stops one
    position early loses a candidate."""
    rng = random.Random(8006 + want_end)
    k, w = seed_size, window_size
    base = rand_seq(rng, 800)
    lens = [k + w - 1, k + w, k + w + 1, 15, 16, 17, 31, 32, 33, 1, want_end + k + w - 15, want_end + k + w]
    assert (want_end + k + w) % 16 == 0
    reads, spans = [base, mutate(rng, base, 0.04), dsoft_model.revcomp(base)], []
    for n, ln in enumerate(lens):
        at = (37 * n) % 200
        if scanned(ln, k, w) == want_end:
            at = 400 * (ln % 16 == 0)                        # apart: neither holds the other's last seed
            while any(seed_positions(s, k, w)[-1] != want_end - 1
                      for s in (base[at:at + ln], dsoft_model.revcomp(base[at:at + ln]))):
                at += 1
            spans += [(s, want_end - 1) for s in (base[at:at + ln], dsoft_model.revcomp(base[at:at + ln]))]
        reads.append(base[at:at + ln])
    tail = b"".join(stairs(rng, s, [(p, p)], k, w) for s, p in spans)
    return Case(name, reads + [tail], seed_size=k, window_size=w, threshold=k, num_seeds=800)


def _windows(name, **params):
    rng = random.Random(8007)
    a = rand_seq(rng, 1300)
    reads = [a, mutate(rng, a[100:1100], 0.06), rand_seq(rng, 500) + a[900:] + b"N" * 30, rand_seq(rng, 450),
             dsoft_model.revcomp(a[:700])]
    return Case(name, reads, **params)


def _max_candidates(name, threshold):
    rng = random.Random(8008)
    a = rand_seq(rng, 900)
    reads = [a, mutate(rng, a, 0.05) + rand_seq(rng, 100), rand_seq(rng, 60) + a[200:], a[:500] + rand_seq(rng, 300),
             dsoft_model.revcomp(a)]
    return Case(name, reads, seed_size=10, window_size=4, threshold=threshold, num_seeds=200, max_candidates=2)


_BUILDERS = {
    "many_hits_bin64": lambda: _many_hits(64),
    "many_hits_bin4096": lambda: _many_hits(4096),
    "low_threshold_eq_k": lambda: _low_threshold("low_threshold_eq_k", 10),
    "low_threshold_below_k": lambda: _low_threshold("low_threshold_below_k", 7),
    "low_threshold_1": lambda: _low_threshold("low_threshold_1", 1),
    "full_counter": _full_counter,
    "padding": _padding,
    "padding_k12": _padding_k12,
    "seed_cut_0": lambda: _seed_cut("seed_cut_0", 0),
    "seed_cut_1": lambda: _seed_cut("seed_cut_1", 1, threshold=12),
    "seed_cut_last_of_chunk": lambda: _seed_cut("seed_cut_last_of_chunk", seed_cut_at_chunk_edge(False)),
    "seed_cut_first_of_next": lambda: _seed_cut("seed_cut_first_of_next", seed_cut_at_chunk_edge(True)),
    "lengths_end255": lambda: _lengths("lengths_end255", 12, 5, 255),
    "lengths_end256": lambda: _lengths("lengths_end256", 12, 4, 256),
    "lengths_end257": lambda: _lengths("lengths_end257", 11, 4, 257),
    "windows_w1": lambda: _windows("windows_w1", seed_size=10, window_size=1),
    "windows_wk1": lambda: _windows("windows_wk1", seed_size=10, window_size=9),
    "windows_bin1": lambda: _windows("windows_bin1", seed_size=11, bin_size=1),
    "windows_bin48": lambda: _windows("windows_bin48", seed_size=11, bin_size=48),
    "windows_bin_over_reads": lambda: _windows("windows_bin_over_reads", seed_size=11, bin_size=2048),
    "max_candidates": lambda: _max_candidates("max_candidates", 21),
    "max_candidates_first_hit": lambda: _max_candidates("max_candidates_first_hit", 10),
}
NAMES = list(_BUILDERS)
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
        assert _CASES[name].name == name
    return _CASES[name]


def expected(reflib, c):
    """the list a case must give, strand-major: the reference's own (`reflib`: live, or its recorded calls) for every
    strand it defines, the model's for the strands whose trace says it does not (QueryTrace.undefined); those strands
    are never handed to the reference, which would stop at an assertion or leave counted bins behind"""
    _, tf, tr, mf, mr = c.model()
    lists = []
    for queries, traces, model_lists in ((c.reads, tf, mf), (c.rc, tr, mr)):
        ok = [q for q, t in enumerate(traces) if not t.undefined]
        got = reflib.dsoft_candidates(c.reads, [queries[q] for q in ok], **c.params)
        per_query = list(model_lists)
        for q, cands in zip(ok, got):
            per_query[q] = [tuple(x) for x in cands]
        lists.append(per_query)
    return dsoft_model.strand_major(lists[0], lists[1])
