"""A plain restatement of the D-SOFT seed filter, written for clarity, with a trace of the paths a query took.

What it states (the reference's behaviour; the line numbers are the reference's):

* 2-bit coding: A 0, C 1, G 2, T 3, lower case like upper, everything else A (ntcoding.cpp:56-69).  A sequence is
  followed by as many A as a seed needs: the zero bits of its last 2-bit word (ntcoding.cpp:87-103,115-124).
* hash32: Thomas Wang's integer hash, masked to 2k bits after every addition (ntcoding.cpp:74-85).
* (k, w) minimizers over the positions p of `n_words` 16-base words (ntcoding.cpp:126-182): the hash of the seed at p
  enters a ring of w hashes, m(p) is the ring's minimum, and (m, p) is emitted when m differs from the last emitted
  minimum or p is w or more past the last emitted position.  Both start at 0 (`last_m = 0`, `last_p = 0`), the ring
  starts with the hashes of positions 0..w-2, and p runs over [w-1, 16 n_words - k - w).  The emitted position is the
  window's LAST position, not the minimizer's own.
* the reference set: every sequence is followed by N (read as A) up to a whole number of bins, the padded sequences
  are concatenated (darwin.cpp:532-543); n_words = 1 + length/16, so with k + w < 16 positions at and past the
  padded length are emitted as well (seed_pos_table.cpp:60).
* the index (seed_pos_table.cpp:58-94): the emitted (m, p) sorted; per seed value the END offset of its positions in
  that order; a seed value with more than seed_occurence_multiple * (1 + (length >> 2k)) positions is never used.
* a query (seed_pos_table.cpp:100-167), n_words = (length + 15)/16: its minimizers in position order; those under
  the occurrence cap are applied until num_seeds + 1 have been (the counter is tested with `>` before it is
  incremented); a hit below the query offset is skipped; bin = (hit - offset)/bin_size holds (count, last offset);
  while count < threshold a hit adds k if the bin is new or the offset moved by more than k, else the distance the
  offset moved; the hit on which count reaches the threshold is emitted as (hit, offset).
* decode (darwin.cpp:215-224): the sequence that owns bin hit/bin_size, the position inside it, clamped to its length
  when `>` it.
* max_candidates: a query strand keeps its first max_candidates emissions, and every strand starts from clean bins.
  That is what the device does; where the reference differs from it, its behaviour depends on an earlier query (see
  QueryTrace.undefined).

Positions of a few tens of kilobases are meant; nothing here is fast.
"""
import bisect


def two_bit(c):
    return {"A": 0, "C": 1, "G": 2, "T": 3}.get(chr(c).upper(), 0)


_CODE = [two_bit(c) for c in range(256)]


def hash32(key, k):
    m = (1 << (2 * k)) - 1
    key = (~key + (key << 21)) & m
    key = key ^ (key >> 24)
    key = ((key + (key << 3)) + (key << 8)) & m
    key = key ^ (key >> 14)
    key = ((key + (key << 2)) + (key << 4)) & m
    key = key ^ (key >> 28)
    key = (key + (key << 31)) & m
    return key


def minimizers(seq, n_words, k, w):
    """[(position, minimum)] in position order, or None where 16 n_words < k + w: the reference's unsigned loop bound
    wraps there (ntcoding.cpp:139,168) and it reads far outside the sequence"""
    if 16 * n_words < k + w:
        return None
    codes = [_CODE[c] for c in seq] + [0] * (16 * n_words + k)
    # hashes[p]: hash of the seed at p, base p + j of it at bits 2j (ntcoding.cpp:115-124)
    hashes, seed = [], sum(codes[j] << (2 * j) for j in range(k))
    for p in range(16 * n_words):
        hashes.append(hash32(seed, k))
        seed = (seed >> 2) | (codes[p + k] << (2 * (k - 1)))

    ring = [0] * w
    for p in range(w - 1):
        ring[p] = hashes[p]
    out, last_m, last_p = [], 0, 0
    for p in range(w - 1, 16 * n_words - k - w):
        ring[p % w] = hashes[p]
        m = min(ring)
        if m != last_m or p - last_p >= w:
            out.append((p, m))
            last_m, last_p = m, p
    return out


class QueryTrace:
    """what one query strand did"""

    def __init__(self):
        self.seed_offsets = []         # query position of every applied seed
        self.seed_hits = []            # number of index positions of every applied seed
        self.group_boundaries = []     # (seed number, h, same bin) for every h = 64, 128, ... with hits h-1 and h both used
        self.first_hit_crossings = []  # bins that reached the threshold on their first hit
        self.max_counter = 0           # the largest count a bin reached
        self.padding = []              # emitted (hit, offset) whose hit lies in a sequence's padding
        self.past_end = []             # emitted (hit, offset) whose hit lies at or past the padded length
        self.clamped = []              # emitted (hit, offset) whose position was clamped to the sequence's length
        self.cut_at = None             # (query position, chunk, number in chunk, last of chunk) of the seed refused by num_seeds
        self.passing = []              # query positions of all minimizers under the cap, applied or not
        self.n_emitted = 0             # before max_candidates
        self.late_emissions = 0        # emissions from a hit that is not among the first 64 of its seed
        self.undefined = []            # why the reference's own answer is not defined for this strand


class Index:
    def __init__(self, reference_seqs, seed_size=14, bin_size=64, window_size=4, threshold=21, num_seeds=800,
                 seed_occurence_multiple=32, max_candidates=1000000):
        self.k, self.w, self.bin_size, self.threshold = seed_size, window_size, bin_size, threshold
        self.num_seeds, self.max_candidates = num_seeds, max_candidates
        concat, self.start_bin, self.bin_chr, self.lengths = b"", [], [], []
        for i, r in enumerate(reference_seqs):
            r = bytes(r)
            self.start_bin.append(len(self.bin_chr))
            self.lengths.append(len(r))
            n_bins = (len(r) + bin_size - 1) // bin_size
            concat += r + b"N" * (n_bins * bin_size - len(r))
            self.bin_chr += [i] * n_bins
        self.ref_len = len(concat)
        self.max_occ = seed_occurence_multiple * (1 + (self.ref_len >> (2 * self.k)))
        mins = minimizers(concat, 1 + self.ref_len // 16, self.k, self.w)
        order = sorted((m, p) for p, m in mins)
        self.pos = [p for m, p in order]
        # END offset of every seed value that occurs; a value's positions start where the value below it ends
        self.values = sorted(set(m for m, p in order))
        self.end = {}
        for n, (m, p) in enumerate(order):
            self.end[m] = n + 1

    def hits(self, value):
        if value not in self.end:
            return []
        at = bisect.bisect_left(self.values, value)
        start = self.end[self.values[at - 1]] if at else 0
        return self.pos[start:self.end[value]]

    def query(self, seq):
        """([(ref_id, ref_pos, query_pos)], QueryTrace) of one strand"""
        k, B, tr = self.k, self.bin_size, QueryTrace()
        mins = minimizers(bytes(seq), (len(seq) + 15) // 16, k, self.w)
        if mins is None:
            tr.undefined.append("16 * words < k + w: the minimizer loop's unsigned bound wraps (ntcoding.cpp:168)")
            return [], tr
        bins, emitted = {}, []                  # bin -> (count, last offset)
        passing = [(offset, self.hits(value)) for offset, value in mins]
        passing = [(offset, hits) for offset, hits in passing if len(hits) <= self.max_occ]
        tr.passing = [offset for offset, hits in passing]
        for n, (offset, hits) in enumerate(passing):
            if n > self.num_seeds:              # seeds 0 .. num_seeds are applied: N + 1 of them
                chunk = offset // 256
                in_chunk = [o for o in tr.passing if o // 256 == chunk]
                tr.cut_at = (offset, chunk, in_chunk.index(offset), offset == in_chunk[-1])
                break
            tr.seed_offsets.append(offset)
            tr.seed_hits.append(len(hits))
            if any(h >= self.ref_len for h in hits) and not tr.undefined:
                tr.undefined.append("a hit at or past the padded length: assert(hit < ref_size_) "
                                    "(seed_pos_table.cpp:134); without it, a bin past the last in bin_to_chr_id "
                                    "(darwin.cpp:217)")
            for h in range(64, len(hits), 64):
                if hits[h - 1] >= offset:
                    tr.group_boundaries.append((n, h, (hits[h - 1] - offset) // B == (hits[h] - offset) // B))
            for nth, hit in enumerate(hits):
                if hit < offset:
                    continue
                b = (hit - offset) // B
                count, last = bins.get(b, (0, 0))
                if count >= self.threshold:
                    continue
                count_new = count + (k if count == 0 else min(offset - last, k))
                bins[b] = (count_new, offset)
                tr.max_counter = max(tr.max_counter, count_new)
                if count_new >= self.threshold:
                    if count == 0:
                        tr.first_hit_crossings.append(b)
                        if len(emitted) >= self.max_candidates and not tr.undefined:
                            tr.undefined.append("max_candidates reached on a bin's first hit: the `break` leaves before "
                                                "the bin is listed for clearing (seed_pos_table.cpp:145-153) and the "
                                                "next query of the thread finds it counted")
                    emitted.append((hit, offset))
                    tr.late_emissions += nth >= 64
        tr.n_emitted = len(emitted)
        out = []
        for hit, offset in emitted[:self.max_candidates]:
            rbin = hit // B
            if rbin < len(self.bin_chr):
                chr_id = self.bin_chr[rbin]
            else:
                chr_id = 0                      # no sequence owns the bin; host and device say 0
                tr.past_end.append((hit, offset))
            ref_pos = hit - self.start_bin[chr_id] * B
            if rbin < len(self.bin_chr) and ref_pos >= self.lengths[chr_id]:
                tr.padding.append((hit, offset))
            if ref_pos > self.lengths[chr_id]:
                ref_pos = self.lengths[chr_id]
                tr.clamped.append((hit, offset))
            out.append((chr_id, ref_pos, offset))
        return out, tr


def revcomp(seq):
    """darwin.cpp:110-147 for the letters the cases use"""
    return bytes(seq).translate(bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan"))[::-1]


def candidates(reference_seqs, queries, **params):
    """per query [(ref_id, ref_pos, query_pos)], the shape of RefLib.dsoft_candidates, and the traces"""
    ix = Index(reference_seqs, **params)
    res = [ix.query(q) for q in queries]
    return [r[0] for r in res], [r[1] for r in res]


def strand_major(forward, reverse):
    """[(ref_id, query_id, ref_pos, query_pos, comp)]: all forward strands in query order, then all reverse
    complements, as the device lists them"""
    return [(c[0], q, c[1], c[2], comp) for comp, per_query in ((0, forward), (1, reverse))
            for q, cands in enumerate(per_query) for c in cands]
