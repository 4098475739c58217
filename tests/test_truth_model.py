"""CPU suite: the reference path behind a run -- the oracle's chains, then the models of selection, coverage, the overlap graph,
cleaning, the unitigs and the pileup with corrected reads -- held to the simulator's ground truth by tests/truth_checks.py, on
the `tiny` block with true candidates only (block A) and with the synthesiser's share of false hits (block B); the alignment
paths column by column, the per-base depth per side and the identities on the same blocks; the placement of the reads on
contigs with a diverged decoy (block P: the oracle's chains, then tests/place_model.py); and the checks' teeth: every
misreading of a frame, an end, a sign, a direction or a kind that kernel and model could share makes the named check raise.
tests/test_gpu_truth.py holds the device to the same checks."""
import numpy as np
import pytest

import clean_model
import cover_model
import graph_model
import path_cases
import select_model
import summary_cases
import truth_checks as tc
import unitig_model
from pileup_ins_model import pileup_ins

MIN_DEPTH, INS_SLOTS = 3, 2
_BLOCKS, _PATHS = {}, {}


def block(name):
    """A: the `tiny` workload with a candidate on every true overlap and none elsewhere; B: with synth_candidates' own share of
    false hits.  -> (rs, cf, cr, law)"""
    from gact_amd import synth, workload
    if name not in _BLOCKS:
        cfg = workload.CONFIGS["tiny"]
        rs = synth.simulate_reads(**cfg)
        extra = dict(false_frac=0.0) if name == "A" else {}
        cf, cr = synth.synth_candidates(rs, seed=8, include_self=False, **extra)
        _BLOCKS[name] = (rs, cf, cr, tc.stretch_of(**cfg))
    return _BLOCKS[name]


class _Rc:
    def __init__(self, rs):
        self.rs = rs

    def __getitem__(self, i):
        return self.rs.rc(i)


def graph_stages(rs, records, sel, sums, clip=None):
    """coverage (its spans are the clip, unless one is given) -> graph -> cleaning -> unitigs at tip_reads 0 on the graph's arcs
    and 3 on the cleaned ones, with bases"""
    lens = np.array([len(r) for r in rs.reads], dtype=np.int32)
    if clip is None:
        cover, _ = cover_model.cover(records, lens, sel=sel, sums=sums, min_depth=MIN_DEPTH)
        clip = np.stack([cover["span_begin"], cover["span_end"]], axis=1).astype(np.int32).reshape(-1)
    g = graph_model.graph(records, lens, sel=sel, sums=sums, clip=clip)
    cl = clean_model.clean(lens, g["reads"], g["arcs"], clip=clip)
    cleaned = clean_model.cleaned(g["arcs"], cl["arc_flags"])
    utg = {0: unitig_model.unitigs(lens, g["reads"], g["arcs"], clip=clip, tip_reads=0, seqs=rs.reads),
           3: unitig_model.unitigs(lens, g["reads"], cleaned, clip=clip, tip_reads=3, seqs=rs.reads)}
    return dict(lens=lens, clip=clip, reads=g["reads"], arcs=g["arcs"], cleaned=cleaned, utg=utg)


def reference_path(oracle, name):
    """the whole chain on a block, computed once"""
    if name in _PATHS:
        return _PATHS[name]
    from gact_amd import engine
    rs, cf, cr, law = block(name)
    cands, nf = np.concatenate([cf, cr]), len(cf)
    exp = path_cases.expected(oracle, rs, cands, nf)
    records = np.zeros(len(cands), dtype=engine.OVERLAP_DTYPE)
    records["ref_id"], records["query_id"], records["comp"] = cands["ref_id"], cands["query_id"], np.arange(len(cands)) >= nf
    for f in path_cases.RECORD_FIELDS:
        records[f] = [e[f] for e in exp]
    records["emitted"] = (records["score"] > 0) & (records["ref_id"] != records["query_id"])
    cigars = [e["cigar"] for e in exp]
    all_sums = np.array([engine.summarise(summary_cases.ops_of_cigar(c)) for c in cigars], dtype=engine.SUMMARY_DTYPE)
    sel = select_model.select(records, "pair")
    sums = all_sums[sel]
    p = graph_stages(rs, records, sel, sums)
    _, table, read_at, seq, _ = pileup_ins(rs.reads, _Rc(rs), records[sel], [cigars[i] for i in sel.tolist()], (0, rs.n),
                                           MIN_DEPTH, INS_SLOTS)
    by_side = {s: cover_model.cover(records, p["lens"], sel=sel, sums=sums, sides=tc.SIDES.index(s) + 1, min_depth=MIN_DEPTH)
               for s in tc.SIDES}
    p.update(rs=rs, law=law, cands=cands, nf=nf, records=records, sel=sel, sums=sums, n_candidates=len(cands), read_at=read_at,
             seq=seq, table=table, ops=[summary_cases.ops_of_cigar(cigars[i]) for i in sel.tolist()], by_side=by_side)
    _PATHS[name] = p
    return p


def nontrivial(p):
    """the block exercises what the checks are about"""
    lens, clip = p["lens"], p["clip"]
    assert ((clip[0::2] > 0) | (clip[1::2] < lens)).any(), "no clip is narrower than its read"
    assert (p["utg"][0]["layout"]["vertex"] & 1).any() and (p["utg"][3]["layout"]["vertex"] & 1).any(), "no layout vertex is odd"
    assert p["utg"][3]["unitigs"]["n_reads"].max() >= 8, "no unitig at tip_reads 3 holds 8 reads"
    assert (p["reads"]["contained_by"] >= 0).any(), "no read is contained"
    assert p["records"]["comp"][p["sel"]].any() and not p["records"]["comp"][p["sel"]].all()


def test_block_a_all_six_checks(oracle):
    p = reference_path(oracle, "A")
    rs, law, clip = p["rs"], p["law"], p["clip"]
    print("block A: %d candidates, %d selected; stretch %.4f, variance %.4f per genome base" % (
        p["n_candidates"], len(p["sel"]), law[0], law[1]))
    assert abs(law[0] - 1.045) < 1e-9 and abs(law[1] - 0.125) < 1e-3
    nontrivial(p)
    f = tc.record_ends(rs, p["records"], p["sel"], p["sums"])
    print("check 1, record ends:", f)
    assert not tc.false_hits(rs, p["cands"], p["nf"])[0] and f["ends"] == 2 * int(p["records"]["emitted"][p["sel"]].sum()) > 1000
    f = tc.containments(rs, p["reads"], p["records"], clip)
    print("check 2, containments:", f)
    assert f["contained"] == int((p["reads"]["contained_by"] >= 0).sum()) > 0
    for what, arcs in (("the graph's", p["arcs"]), ("the cleaned", p["cleaned"])):
        f = tc.arcs(rs, arcs, clip, law=law)
        print("check 3, %s arcs:" % what, f)
        assert f["checked"] == f["kept"] > 0 and tc.arcs(rs, arcs, clip, law=law, count_only=True) == 0
    clip2, g2 = narrowed_graph(p)
    f = tc.arcs(rs, g2["arcs"], clip2, law=law)
    print("check 3, the arcs under a clip 300 narrower at both ends:", f)
    print("check 2 under it:", tc.containments(rs, g2["reads"], p["records"], clip2))
    kept = g2["arcs"][g2["arcs"]["flags"] == 0]
    assert f["kept"] > 0 and (clip2[2 * (kept["u"] >> 1)] >= 300).all()
    for k in (0, 3):
        u = p["utg"][k]
        f = tc.layout(rs, u["unitigs"], u["layout"], u["places"], clip, law=law)
        print("check 4, layout at tip_reads %d:" % k, f, "reads per unitig", u["unitigs"]["n_reads"].tolist())
        assert f["checked"] == len(u["unitigs"]) > 0
        f = tc.unitig_bases(rs, u["unitigs"], u["layout"], u["seq"], clip)
        print("check 5, bases at tip_reads %d:" % k, [(j, n, round(r, 4), round(o, 4)) for j, n, r, o in f["rates"] if n > 1])
    f = tc.corrected(rs, p["read_at"], p["seq"], range(rs.n))
    print("check 6, corrected reads:", f, "inserted %d" % int(p["table"]["inserted"].sum()))
    assert f["reads"] == rs.n and int(p["table"]["inserted"].sum()) > 0


def test_the_banded_distance_is_the_full_one_on_a_whole_unitig(oracle):
    p = reference_path(oracle, "A")
    u = p["utg"][3]
    j = int(np.argmax(u["unitigs"]["length"]))
    at, n = int(u["unitigs"]["seq_at"][j]), int(u["unitigs"]["length"][j])
    truth = tc.unitig_truth(p["rs"], u["unitigs"], u["layout"], p["clip"], j)
    banded, full = tc.edit_distance(u["seq"][at:at + n], truth), tc.edit_distance_full(u["seq"][at:at + n], truth)
    print("unitig %d: %d bases against %d of the genome: banded %d, full %d" % (j, n, len(truth), banded, full))
    assert n > 10000 and banded == full
    # and on small cases at every band position: a band that holds the whole table, one that cuts it, empty sides
    rng = np.random.default_rng(3)
    for la, lb in ((0, 0), (0, 5), (7, 0), (1, 1), (30, 41), (41, 30), (200, 180)):
        a, b = rng.integers(0, 4, la).astype(np.uint8), rng.integers(0, 4, lb).astype(np.uint8)
        assert tc.edit_distance(a, b) == tc.edit_distance_full(a, b) <= tc.edit_distance(a, b, band=12)
    a = rng.integers(0, 4, 300).astype(np.uint8)
    b = np.concatenate([a[:100], a[105:250], rng.integers(0, 4, 3).astype(np.uint8), a[250:]])
    assert tc.edit_distance(a, b, band=12) == tc.edit_distance_full(a, b)


# ---- teeth: a misreading that kernel and model could share, applied to the reference path's output

def _swap_ins_del(p):
    sums = p["sums"].copy()
    sums["ins_bases"], sums["del_bases"] = p["sums"]["del_bases"], p["sums"]["ins_bases"]
    return lambda: tc.record_ends(p["rs"], p["records"], p["sel"], sums)


def _stored_frame_records(p):
    rec = p["records"].copy()
    lq = p["lens"][rec["query_id"]]
    comp = rec["comp"] != 0
    rec["bb"][comp], rec["be"][comp] = (lq - p["records"]["be"])[comp], (lq - p["records"]["bb"])[comp]
    return rec


def _stored_frame_ends(p):
    rec = _stored_frame_records(p)
    return lambda: tc.record_ends(p["rs"], rec, p["sel"], p["sums"])


def _stored_frame_arcs(p):
    g = graph_model.graph(_stored_frame_records(p), p["lens"], sel=p["sel"], sums=p["sums"], clip=p["clip"])
    assert (g["arcs"]["flags"] == 0).any()
    return lambda: tc.arcs(p["rs"], g["arcs"], p["clip"], law=p["law"])


def _minus_heads_at_cb(p, monkeypatch):
    def head(rs, clip, v):
        return tc.genome_of(rs, v >> 1, int(clip[2 * (v >> 1)]))
    monkeypatch.setattr(tc, "head", head)
    return lambda: tc.arcs(p["rs"], p["arcs"], p["clip"], law=p["law"])


def narrowed_graph(p):
    """the graph of the block under tc.narrowed_clip: the coverage's own clip cuts no more than 3 bases off any read that keeps
    an arc on this block, so a len measured from the wrong begin could not show under it"""
    clip = tc.narrowed_clip(p["clip"])
    g = graph_model.graph(p["records"], p["lens"], sel=p["sel"], sums=p["sums"], clip=clip)
    return clip, g


def _len_from_the_unclipped_begin(p):
    clip, g = narrowed_graph(p)
    tc.arcs(p["rs"], g["arcs"], clip, law=p["law"])
    arcs = g["arcs"].copy()
    arcs["len"] += clip[2 * (arcs["u"] >> 1)]
    return lambda: tc.arcs(p["rs"], arcs, clip, law=p["law"])


def _flipped_vertex(p):
    u = p["utg"][3]
    lay = u["layout"].copy()
    lay["vertex"][len(lay) // 2] ^= 1
    return lambda: tc.layout(p["rs"], u["unitigs"], lay, u["places"], p["clip"], law=p["law"])


def _shifted_starts(p):
    u = p["utg"][3]
    lay = u["layout"].copy()
    for j in range(len(u["unitigs"])):
        at, n = int(u["unitigs"]["layout_at"][j]), int(u["unitigs"]["n_reads"][j])
        lay["start"][at + 4:at + n] += 300
    return lambda: tc.layout(p["rs"], u["unitigs"], lay, u["places"], p["clip"], law=p["law"])


def _minus_entries_not_complemented(p):
    u = p["utg"][3]
    seq = u["seq"].copy()
    swap = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        swap[a] = b
    for j in range(len(u["unitigs"])):
        at, n = int(u["unitigs"]["layout_at"][j]), int(u["unitigs"]["n_reads"][j])
        for e in u["layout"][at:at + n]:
            if e["vertex"] & 1:
                to = int(u["unitigs"]["seq_at"][j]) + int(e["start"])
                seq[to:to + int(e["take"])] = swap[seq[to:to + int(e["take"])]]        # complemented back: reversed only
    return lambda: tc.unitig_bases(p["rs"], u["unitigs"], u["layout"], seq, p["clip"])


def _raw_reads_as_corrected(p):
    rs = p["rs"]
    read_at = np.concatenate([[0], np.cumsum(p["lens"])]).astype(np.int64)
    return lambda: tc.corrected(rs, read_at, np.concatenate(rs.reads), range(rs.n))


CORRUPTIONS = {"ins_and_del_swapped/check1": _swap_ins_del, "complement_in_the_stored_frame/check1": _stored_frame_ends,
               "complement_in_the_stored_frame/check3": _stored_frame_arcs, "minus_heads_at_cb/check3": _minus_heads_at_cb,
               "len_plus_cb/check3": _len_from_the_unclipped_begin, "one_vertex_flipped/check4": _flipped_vertex,
               "starts_shifted_300/check4": _shifted_starts, "minus_entries_not_complemented/check5": _minus_entries_not_complemented,
               "raw_reads_as_corrected/check6": _raw_reads_as_corrected}


@pytest.mark.parametrize("name", sorted(CORRUPTIONS))
def test_a_shared_misreading_makes_the_named_check_raise(oracle, monkeypatch, name):
    p = reference_path(oracle, "A")
    make = CORRUPTIONS[name]
    check = make(p, monkeypatch) if make is _minus_heads_at_cb else make(p)
    with pytest.raises(AssertionError) as info:
        check()
    print("%s: %s" % (name, info.value))


# ---- block B: false hits

def block_b_figures(rs, law, false, records, sel, sums, clip, arcs, cleaned, utg, read_at, seq, which):
    """what must hold with false hits in the set, on the reference path and on the device alike: checks 1, 3 and 4 on the
    records, arcs and unitigs that no false hit made (false: tc.false_hits), check 6 as it stands, and no more wrong arcs after
    the cleaning than before it.  utg[k]: (unitigs, layout, places).  -> the counts, for printing"""
    hits, pairs = false
    chosen = [i for i in np.asarray(sel).tolist() if records["emitted"][i]]
    f1 = tc.record_ends(rs, records, sel, sums, false=hits)
    wrong = [tc.arcs(rs, a, clip, law=law, count_only=True) for a in (arcs, cleaned)]
    kept = [int((a["flags"] == 0).sum()) for a in (arcs, cleaned)]
    f3 = [tc.arcs(rs, a, clip, law=law, false=hits) for a in (arcs, cleaned)]
    f4 = {k: tc.layout(rs, utg[k][0], utg[k][1], utg[k][2], clip, law=law, false=tc.false_joins(arcs, hits)) for k in (0, 3)}
    f6 = tc.corrected(rs, read_at, seq, which)
    assert wrong[1] <= wrong[0], "%d wrong arcs after the cleaning, %d before it" % (wrong[1], wrong[0])
    return dict(selected=len(chosen), false_hits_selected=sum(i in hits for i in chosen),
                of_reads_with_disjoint_spans=sum(i in pairs for i in chosen), ends=f1, wrong_arcs="%d of %d" % (wrong[0], kept[0]),
                wrong_after_cleaning="%d of %d" % (wrong[1], kept[1]), true_arcs=f3, layout=f4,
                reads_per_unitig_at_3=sorted(utg[3][0]["n_reads"].tolist(), reverse=True)[:4], corrected=f6)


def test_block_b_false_hits_what_must_hold(oracle):
    """calling a selected pair false when the two reads' true spans are disjoint does not name every false hit: the synthesiser
    also draws them between reads that do overlap elsewhere (record 49 of this block: reads 3 and 7, the hit 3,697 genome bases
    off), and the pair selection keeps 6 of those beside the 31 of disjoint reads.  So a record is false by its own seed hit
    (tc.false_hits), which the simulator's truth decides before anything runs"""
    p = reference_path(oracle, "B")
    utg = {k: (p["utg"][k]["unitigs"], p["utg"][k]["layout"], p["utg"][k]["places"]) for k in (0, 3)}
    f = block_b_figures(p["rs"], p["law"], tc.false_hits(p["rs"], p["cands"], p["nf"]), p["records"], p["sel"], p["sums"], p["clip"],
                        p["arcs"], p["cleaned"], utg, p["read_at"], p["seq"], range(p["rs"].n))
    for k, v in f.items():
        print("block B, %s: %s" % (k, v))
    assert f["of_reads_with_disjoint_spans"] > 0, "block B holds no false pair"


# ---- checks 7, 8 and 10 on blocks A and B

def test_block_a_columns_depth_and_identity(oracle):
    p = reference_path(oracle, "A")
    rs, records, sel, sums = p["rs"], p["records"], p["sel"], p["sums"]
    f = tc.alignment_columns(rs, records, sel, sums, p["ops"])
    print("check 7, alignment columns:", f)
    assert f["records"] == int(records["emitted"][sel].sum()) and f["run_ends"] > 100 * f["records"]
    # REACH, taken here: twice the smallest multiple of 10 at which no position lies under the narrowed true depth
    depth = p["by_side"]["both"][1]
    misses = {r: tc.depth_misses(rs, records, sel, depth, reach=r, slack=s) for r, s in
              [(r, tc.END_SLACK) for r in range(10, 110, 10)] + [(tc.REACH, 5)]}
    print("check 8, positions (under, over) by reach:", misses)
    least = min(r for r in range(10, 110, 10) if misses[r][0] == 0)
    assert tc.REACH == 2 * least, "REACH is %d, the reference path needs %d" % (tc.REACH, least)
    f = tc.depth_of_sides(rs, records, sel, sums, p["by_side"], MIN_DEPTH)
    print("check 8, depth against true depth:", f)
    assert f["both"]["intervals"] == f["ref"]["intervals"] + f["query"]["intervals"] == 2 * int(records["emitted"][sel].sum())
    f = tc.identities(records, sel, sums)
    print("check 10, identities on block A:", f)
    assert f["false"][0] == 0


def _exchanged(ops):
    swap = {tc.OP_I: tc.OP_D, tc.OP_D: tc.OP_I}
    return [np.array([(int(w) & ~15) | swap.get(int(w) & 15, int(w) & 15) for w in o], dtype=np.uint32) for o in ops]


def _ins_and_del_exchanged_in_the_walk(p):
    ops = _exchanged(p["ops"])
    return lambda: tc.alignment_columns(p["rs"], p["records"], p["sel"], p["sums"], ops)


def _ins_and_del_exchanged_in_ops_and_summary(p):
    """... consistently: the walk still ends at (ae, be), from begins that are off by ins_bases - del_bases"""
    ops, sums = _exchanged(p["ops"]), p["sums"].copy()
    sums["ins_bases"], sums["del_bases"] = p["sums"]["del_bases"], p["sums"]["ins_bases"]
    return lambda: tc.alignment_columns(p["rs"], p["records"], p["sel"], sums, ops)


def _ops_reversed(p):
    ops = [o[::-1] for o in p["ops"]]
    return lambda: tc.alignment_columns(p["rs"], p["records"], p["sel"], p["sums"], ops)


def _stored_frame_columns(p):
    rec = _stored_frame_records(p)
    return lambda: tc.alignment_columns(p["rs"], rec, p["sel"], p["sums"], p["ops"])


def _ops_of_the_record_before(p):
    ops = p["ops"][-1:] + p["ops"][:-1]
    return lambda: tc.alignment_columns(p["rs"], p["records"], p["sel"], p["sums"], ops)


def _with_side(p, **sides):
    by_side = dict(p["by_side"])
    by_side.update(sides)
    return lambda: tc.depth_of_sides(p["rs"], p["records"], p["sel"], p["sums"], by_side, MIN_DEPTH)


def _query_unmirrored(p):
    """a complement record's [bb, be) put on the stored read as it stands: the records mirrored once, so that the model's own
    mirror undoes it"""
    rec = _stored_frame_records(p)
    got = {s: cover_model.cover(rec, p["lens"], sel=p["sel"], sums=p["sums"], sides=tc.SIDES.index(s) + 1, min_depth=MIN_DEPTH)
           for s in ("query", "both")}
    over = tc.depth_misses(p["rs"], p["records"], p["sel"], got["both"][1])[1]
    print("the query interval of complement records unmirrored: %d of %d positions over the widened true depth" % (
        over, len(got["both"][1])))
    return _with_side(p, **got)


def _target_and_query_exchanged(p):
    rec = p["records"].copy()
    rec["ref_id"], rec["query_id"] = p["records"]["query_id"], p["records"]["ref_id"]
    return _with_side(p, ref=cover_model.cover(rec, p["lens"], sel=p["sel"], sums=p["sums"], sides=cover_model.REF,
                                               min_depth=MIN_DEPTH))


def _depth_shifted_by_one_read(p):
    cover, depth = p["by_side"]["both"]
    n = int(p["lens"][-1])
    return _with_side(p, both=(cover, np.concatenate([depth[-n:], depth[:-n]])))


TEETH = {"ins_and_del_exchanged_in_the_walk/check7": (_ins_and_del_exchanged_in_the_walk, "the walk of its ops"),
         "ins_and_del_exchanged_in_ops_and_summary/check7": (_ins_and_del_exchanged_in_ops_and_summary,
                                                             "alignment column|leaves its reads"),
         "ops_reversed/check7": (_ops_reversed, "alignment column"),
         "complement_query_in_the_stored_frame/check7": (_stored_frame_columns, "alignment column"),
         "ops_of_the_record_before/check7": (_ops_of_the_record_before, "the walk of its ops"),
         "complement_query_unmirrored/check8": (_query_unmirrored, "sides query: .* over the true depth"),
         "target_and_query_exchanged/check8": (_target_and_query_exchanged, "sides ref: .* the true depth"),
         "depth_shifted_by_one_read/check8": (_depth_shifted_by_one_read, "sides both: .* the true depth")}


@pytest.mark.parametrize("name", sorted(TEETH))
def test_a_misreading_of_columns_or_depth_makes_the_named_check_raise(oracle, name):
    p = reference_path(oracle, "A")
    make, message = TEETH[name]
    with pytest.raises(AssertionError, match=message) as info:
        make(p)()
    print("%s: %s" % (name, info.value))


def test_block_b_identity_tells_false_records_from_true_ones(oracle):
    p = reference_path(oracle, "B")
    hits, _ = tc.false_hits(p["rs"], p["cands"], p["nf"])
    f = tc.identities(p["records"], p["sel"], p["sums"], false=hits)
    print("check 10, identities on block B:", f)
    assert f["false"][0] == sum(1 for i in p["sel"].tolist() if i in hits and p["records"]["emitted"][i]) > 0
    f7 = tc.alignment_columns(p["rs"], p["records"], p["sel"], p["sums"], p["ops"], false=hits)
    print("check 7, the alignment columns of block B's true records:", f7)
    assert f7["records"] == f["true"][0]
    with pytest.raises(AssertionError, match="identity does not tell"):
        tc.identities(p["records"], p["sel"], p["sums"], false=set(p["sel"][::2].tolist()))


# ---- block P: the reads placed on contigs, with a decoy

CONTIG, DECOY, DECOY_RATE, MIN_SHARE, P_SEED = 10000, (12000, 16000), 0.05, 300, 20261021
_P = {}


def block_p():
    """the `tiny` reads against the genome cut into four contigs and a fifth, genome[12000:16000] with 5 % of its bases
    substituted; one candidate, from truth, for every read and every contig that share 300 genome bases, the forward ones
    first.  -> dict(rs, contigs (begin, end), decoy, seqs, cands, nf)"""
    if "block" not in _P:
        from gact_amd import engine, synth
        rs = block("A")[0]
        rng = np.random.default_rng(P_SEED)
        contigs = [(b, b + CONTIG) for b in range(0, len(rs.genome), CONTIG)] + [DECOY]
        seqs = [rs.genome[b:e].copy() for b, e in contigs]
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        at = rng.choice(len(seqs[-1]), int(DECOY_RATE * len(seqs[-1])), replace=False)
        seqs[-1][at] = acgt[(np.searchsorted(acgt, seqs[-1][at]) + rng.integers(1, 4, len(at))) % 4]
        hits = {0: [], 1: []}
        for i in range(rs.n):
            for c, (b, e) in enumerate(contigs):
                lo, hi = max(b, int(rs.start[i])), min(e, int(rs.start[i] + rs.span[i]))
                if hi - lo >= MIN_SHARE:
                    g, comp = int(rng.integers(lo, hi)), int(rs.strand[i])
                    hits[comp].append((c, i, g - b, synth._read_coord(rs, i, g, comp)))
        _P["block"] = dict(rs=rs, contigs=contigs, decoy=len(contigs) - 1, seqs=seqs, nf=len(hits[0]),
                           cands=np.array(hits[0] + hits[1], dtype=engine.CAND_DTYPE))
    return _P["block"]


def reference_path_p(oracle):
    """the oracle's chain of every candidate of block P, its summary, and the model's placement; computed once"""
    if "path" not in _P:
        import place_model
        from gact_amd import engine
        from path_model import gact_path
        b = block_p()
        rs, cands, nf = b["rs"], b["cands"], b["nf"]
        records = np.zeros(len(cands), dtype=engine.OVERLAP_DTYPE)
        records["ref_id"], records["query_id"], records["comp"] = cands["ref_id"], cands["query_id"], np.arange(len(cands)) >= nf
        sums = np.zeros(len(cands), dtype=engine.SUMMARY_DTYPE)
        for k, c in enumerate(cands):
            q = int(c["query_id"])
            m = gact_path(oracle.align_with_bt, b["seqs"][int(c["ref_id"])], rs.rc(q) if k >= nf else rs.reads[q],
                          int(c["ref_pos"]), int(c["query_pos"]))
            for f in path_cases.RECORD_FIELDS:
                records[f][k] = m[f]
            sums[k] = engine.summarise(m["ops"])
        records["emitted"] = records["score"] > 0
        lens = np.array([len(r) for r in rs.reads], dtype=np.int32)
        place, table = place_model.place(records, lens, sums=sums)
        _P["path"] = dict(b, lens=lens, records=records, sums=sums, place=place, table=table)
    return _P["path"]


def test_block_p_placements(oracle):
    p = reference_path_p(oracle)
    f = tc.placements(p["rs"], p["contigs"], p["decoy"], p["records"], p["sums"], p["place"], p["table"])
    print("check 9, block P: %d chains, %d forward;" % (len(p["cands"]), p["nf"]), f)
    assert f["ends"] == 2 * int(p["records"]["emitted"].sum()) and f["kinds"][tc.PRIMARY] == p["rs"].n


def _decoy_and_home_exchanged(p):
    rec = p["records"].copy()
    k = int(np.flatnonzero((p["place"]["kind"] == tc.SECONDARY) & (rec["ref_id"] == p["decoy"]))[0])
    parent = int(p["place"]["parent"][k])
    rec["ref_id"][k], rec["ref_id"][parent] = p["records"]["ref_id"][parent], p["records"]["ref_id"][k]
    return dict(records=rec)


def _supplementary_and_secondary_exchanged(p):
    place = p["place"].copy()
    place["kind"][p["place"]["kind"] == tc.SUPPLEMENTARY] = tc.SECONDARY
    place["kind"][p["place"]["kind"] == tc.SECONDARY] = tc.SUPPLEMENTARY
    return dict(place=place)


def _comp_inverted_on_one_record(p):
    rec = p["records"].copy()
    rec["comp"][len(rec) // 2] ^= 1
    return dict(records=rec)


def _primary_at_the_lowest_score(p):
    table = p["table"].copy()
    many = int(np.argmax(table["n_records"]))
    mine = np.flatnonzero((p["records"]["query_id"] == many) & (p["records"]["emitted"] != 0))
    table["primary"][many] = mine[np.argmin(p["records"]["score"][mine])]
    assert table["primary"][many] != p["table"]["primary"][many]
    return dict(table=table)


P_TEETH = {"decoy_and_true_contig_exchanged": (_decoy_and_home_exchanged, "its primary is|on the decoy|apart"),
           "supplementary_and_secondary_exchanged": (_supplementary_and_secondary_exchanged, "not SUPPLEMENTARY|SECONDARY of"),
           "comp_inverted_on_one_record": (_comp_inverted_on_one_record, "apart|leaves its sequences|outside read"),
           "primary_at_the_lowest_score": (_primary_at_the_lowest_score, "its primary is")}


@pytest.mark.parametrize("name", sorted(P_TEETH))
def test_a_misplacement_makes_check_9_raise(oracle, name):
    p = dict(reference_path_p(oracle))
    make, message = P_TEETH[name]
    p.update(make(p))
    with pytest.raises(AssertionError, match=message) as info:
        tc.placements(p["rs"], p["contigs"], p["decoy"], p["records"], p["sums"], p["place"], p["table"])
    print("%s: %s" % (name, info.value))
