"""Truth block V for the variants of the pileup: a sample with two haplotypes against a reference that differs from both.

A 20 kb random genome h1.  The second haplotype h2 is h1 with planted substitutions, left-out runs of 1 to 3 bases and
inserted runs of 1 to 2 bases: the het sites.  The reference is h1 with a further set of substitutions planted into it, so
that every read disagrees with it there -- the hom sites -- cut into two contigs.  All sites lie at least 60 bases apart and at
least 500 from the ends of a contig; no indel lies inside or beside a run of its own base, and none can slide.  The reads come
from synth.simulate_reads(genome=h1) and (genome=h2) in equal shares, 15x each, at the simulator's default error (15 %); one
candidate, from truth, for every read and every contig that share 300 genome bases, as test_truth_model.block_p makes them.

The rule's parameters on this block are the defaults but for hom_permille: min_depth 8, min_alt 4, min_permille 250,
hom_permille 600.  They were chosen on the CPU reference path (reference_path below), as block V is defined, and on nothing a
device gave: at the simulator's error an alignment shows its read's allele at a site in about three columns of four (the median
share of the allele that ALL reads carry is 750 per mille there, from 500 to 870), so the allele of half the reads is expected
near 375, and 600 lies between the two; at the default 750 only 16 of the 28 hom sites found have the planted genotype.

figures() counts, in integers, what a set of records finds of the planted sites."""
import numpy as np

from gact_amd import engine, synth

SEED, GENOME, CONTIGS = 20261023, 20000, ((0, 10000), (10000, 20000))
APART, FROM_ENDS, MIN_SHARE, COVERAGE, K = 60, 500, 300, 15, 2
N_HET_SNV, N_HOM_SNV, N_DEL, N_INS = 40, 30, 25, 25
PARAMS = dict(min_depth=8, min_alt=4, min_permille=250, hom_permille=600)
READS = dict(mean_len=3000, sd_len=600, min_len=1000, max_len=6000)

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_V = {}


def _other(rng, *avoid):
    left = [b for b in _ACGT.tolist() if b not in avoid]
    return left[int(rng.integers(0, len(left)))]


def block_v():
    """-> dict(h1, h2, seqs (the contigs), names, reads, read_names, rc (of read i), cands, nf, truth); truth: (contig, pos,
    kind, len, base or 0, gt) per planted site, in reference coordinates"""
    if "block" in _V:
        return _V["block"]
    rng = np.random.default_rng(SEED)
    h1 = _ACGT[rng.integers(0, 4, GENOME)].copy()
    ref = h1.copy()
    # the sites: a random order of the positions that lie far enough from a contig's ends, taken while they keep their distance
    allowed = np.concatenate([np.arange(b + FROM_ENDS, e - FROM_ENDS) for b, e in CONTIGS])
    kinds = ["het"] * N_HET_SNV + ["hom"] * N_HOM_SNV + ["del"] * N_DEL + ["ins"] * N_INS
    kinds = [kinds[k] for k in rng.permutation(len(kinds))]
    taken = np.zeros(GENOME, dtype=bool)
    sites = []                                          # (pos, kind, n, bases)
    for p in rng.permutation(allowed).tolist():
        if not kinds:
            break
        if taken[max(0, p - APART):p + APART].any():
            continue
        kind = kinds[-1]
        if kind in ("het", "hom"):
            site = (p, kind, 1, [_other(rng, h1[p], h1[p - 1], h1[p + 1])])
        elif kind == "del":
            n = int(rng.integers(1, 4))
            if any(b in (h1[p - 1], h1[p + n]) for b in h1[p:p + n].tolist()):
                continue                                # beside a run of its own base, or able to slide
            site = (p, kind, n, [])
        else:
            n = int(rng.integers(1, 3))
            if h1[p - 1] == h1[p]:
                continue
            free = [b for b in _ACGT.tolist() if b not in (h1[p - 1], h1[p])]
            site = (p, kind, n, [free[int(rng.integers(0, 2))] for _ in range(n)])
        kinds.pop()
        taken[p] = True
        sites.append(site)
    assert not kinds, "not every site found its place"
    sites.sort()
    pieces, at, truth = [], 0, []
    to_h2 = np.zeros(GENOME + 1, dtype=np.int64)        # h2 coordinate of h1 base g (of the next kept one for a left-out base)
    shift = 0
    for p, kind, n, bases in sites:
        c = next(k for k, (b, e) in enumerate(CONTIGS) if b <= p < e)
        at_c = p - CONTIGS[c][0]
        if kind == "hom":
            ref[p] = bases[0]
            truth.append((c, at_c, engine.VARIANT_SNV, 1, int(h1[p]), 2))
            continue
        pieces.append(h1[at:p])
        to_h2[at:p] = np.arange(at, p) + shift
        if kind == "het":
            pieces.append(np.array(bases, np.uint8))
            to_h2[p] = p + shift
            at = p + 1
            truth.append((c, at_c, engine.VARIANT_SNV, 1, bases[0], 1))
        elif kind == "del":
            to_h2[p:p + n] = p + shift
            shift -= n
            at = p + n
            truth.append((c, at_c, engine.VARIANT_DEL, n, 0, 1))
        else:
            pieces.append(np.array(bases, np.uint8))
            shift += n
            at = p
            truth.append((c, at_c, engine.VARIANT_INS, n, 0, 1))
    pieces.append(h1[at:])
    to_h2[at:] = np.arange(at, GENOME + 1) + shift
    h2 = np.concatenate(pieces)
    assert len(h2) == GENOME + shift
    to_h1 = np.searchsorted(to_h2[:GENOME], np.arange(len(h2) + 1), side="left")       # h1 coordinate of h2 base g
    seqs = [ref[b:e].copy() for b, e in CONTIGS]
    sets = [(synth.simulate_reads(GENOME, coverage=COVERAGE, seed=SEED + 1, genome=h1, **READS), None, None),
            (synth.simulate_reads(len(h2), coverage=COVERAGE, seed=SEED + 2, genome=h2, **READS), to_h1, to_h2)]
    reads, names, hits = [], [], {0: [], 1: []}
    for h, (rs, back, forth) in enumerate(sets):
        for i in range(rs.n):
            first, last = int(rs.start[i]), int(rs.start[i] + rs.span[i])      # on the read's own haplotype
            lo1, hi1 = (first, last) if back is None else (int(back[first]), int(back[last]))
            comp = int(rs.strand[i])
            for c, (b, e) in enumerate(CONTIGS):
                lo, hi = max(b, lo1), min(e, hi1)
                if hi - lo >= MIN_SHARE:
                    g = int(rng.integers(lo, hi))
                    own = g if forth is None else min(max(int(forth[g]), first), last - 1)
                    hits[comp].append((c, len(reads), g - b, synth._read_coord(rs, i, own, comp)))
            reads.append(rs.reads[i])
            names.append("h%d_%s" % (h + 1, rs.names[i]))
    _V["block"] = dict(h1=h1, h2=h2, seqs=seqs, names=["contig%d" % (c + 1) for c in range(len(CONTIGS))], reads=reads, read_names=names,
                       rc=[synth.revcomp(r) for r in reads], nf=len(hits[0]), cands=np.array(hits[0] + hits[1], dtype=engine.CAND_DTYPE),
                       truth=truth)
    return _V["block"]


def own_and_offsets():
    seqs = block_v()["seqs"]
    return np.concatenate(seqs), np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)


def write_fasta(path, names, seqs):
    with open(path, "wb") as f:
        for name, s in zip(names, seqs):
            f.write(b">" + name.encode() + b"\n" + bytes(s) + b"\n")


def figures(records, truth=None):
    """what VARIANT_DTYPE records find of the planted sites, all integers: a planted SNV is found by an SNV record at its exact
    position with its exact base; a found one is right when the record has the planted genotype; a planted indel is found by a
    record of its kind and length within 3 bases; an SNV record that finds no planted SNV is unmatched"""
    truth = block_v()["truth"] if truth is None else truth
    snv = {(int(r["seq"]), int(r["pos"]), int(r["bases"]) & 0xff): int(r["flags"]) & 3 for r in records if r["kind"] == engine.VARIANT_SNV}
    gaps = [(int(r["seq"]), int(r["pos"]), int(r["kind"]), int(r["len"])) for r in records if r["kind"] != engine.VARIANT_SNV]
    f = dict(snv_planted=0, snv_found=0, het_found=0, het_right=0, hom_found=0, hom_right=0, indel_planted=0, indel_found=0)
    matched = set()
    for c, pos, kind, n, base, gt in truth:
        if kind == engine.VARIANT_SNV:
            f["snv_planted"] += 1
            if (c, pos, base) in snv:
                matched.add((c, pos, base))
                which = "het" if gt == 1 else "hom"
                f["snv_found"] += 1
                f[which + "_found"] += 1
                f[which + "_right"] += snv[(c, pos, base)] == gt
        else:
            f["indel_planted"] += 1
            f["indel_found"] += any(s == c and k == kind and m == n and abs(p - pos) <= 3 for s, p, k, m in gaps)
    f["snv_unmatched"] = len(snv) - len(matched)
    f["records"] = len(records)
    return f


def check(f):
    """the conditions of block V on figures()"""
    assert 10 * f["snv_found"] >= 9 * f["snv_planted"], f
    assert 10 * f["het_right"] >= 9 * f["het_found"] and 10 * f["hom_right"] >= 9 * f["hom_found"], f
    assert 10 * f["indel_found"] >= 7 * f["indel_planted"], f
    assert 5000 * f["snv_unmatched"] <= GENOME, f


def reference_path(oracle):
    """the CPU reference path, computed once: the oracle's chain of every candidate (tests/path_model.py), the counts and slots
    of tests/pileup_model.py and tests/pileup_ins_model.py, the records of tests/variant_model.py at PARAMS.
    -> dict(counts, ins, records, table, figures)"""
    if "path" not in _V:
        import variant_model
        from path_model import gact_path
        from pileup_ins_model import slot_counts
        from pileup_model import pileup
        b = block_v()
        n_ref = len(b["seqs"])
        recs, cigars = [], []
        for k, c in enumerate(b["cands"]):
            q, comp = int(c["query_id"]), int(k >= b["nf"])
            m = gact_path(oracle.align_with_bt, b["seqs"][int(c["ref_id"])], b["rc"][q] if comp else b["reads"][q], int(c["ref_pos"]),
                          int(c["query_pos"]))
            # (one list for both sides, as the two models index it: the reads stand behind the contigs)
            recs.append(dict(ref_id=int(c["ref_id"]), query_id=n_ref + q, ae=m["ae"], be=m["be"], comp=comp, emitted=int(m["score"] > 0)))
            cigars.append(engine.cigar_string(m["ops"]))
        both, both_rc = b["seqs"] + b["reads"], [None] * n_ref + b["rc"]
        counts, _, _ = pileup(both, both_rc, recs, cigars, (0, n_ref), 1)
        ins, _ = slot_counts(both, both_rc, recs, cigars, (0, n_ref), K)
        own, offs = own_and_offsets()
        records, table = variant_model.variants(counts, ins, own, offs, **PARAMS)
        _V["path"] = dict(counts=counts, ins=ins, records=records, table=table, figures=figures(records))
    return _V["path"]
