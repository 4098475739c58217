"""GPU suite: the device's passes behind a run held to the simulator's ground truth (tests/truth_checks.py), not to their models:
the records and summaries of a run of both strands, the pair selection, the coverage's clip, the overlap graph, the cleaning, the
unitigs with bases and the corrected reads of the pileup, the alignment paths column by column, the per-base depth of the
coverage per side and the identities, on the `tiny` block with true candidates only (block A) and with the synthesiser's share
of false hits (block B); and the placement of the same reads on contigs with a diverged decoy (block P).  What a kernel and its
model could both misread -- the frame of a complement record's bb / be, the end a minus vertex starts from, which read the
inserted and the deleted bases belong to, the direction of a path's ops, the mirror of a complement record's query interval,
which record is the primary -- fails here.
The model equalities are other files' (tests/test_gpu_unitigs.py and the passes' own); tests/test_truth_model.py runs the
reference path through the same checks and shows that every such misreading makes its check raise."""
import numpy as np
import pytest

import truth_checks as tc
from test_truth_model import INS_SLOTS, MIN_DEPTH, block, block_b_figures, block_p

pytestmark = pytest.mark.gpu


def device_path(name):
    """candidates_run_mixed -> select_overlaps("pair") -> candidates_summaries -> read_coverage -> overlap_graph(clip) ->
    clean_graph -> unitigs(seq) at tip_reads 0 and 3, then the pileup with two slots, the paths of the selected records and the
    coverage with its per-base depth, one call per side; the records are taken from the slot and fetched last.  One engine per
    block"""
    from path_cases import engine_with
    rs, cf, cr, law = block(name)
    e, n, nf = engine_with(rs, cf, cr)
    try:
        lens = np.array([len(r) for r in rs.reads], dtype=np.int32)
        e.candidates_run_mixed(n, nf)
        sel = e.select_overlaps(mode="pair")
        _, sums = e.candidates_summaries(sel=sel, rc_from=nf)
        cover = e.read_coverage(lens, sel=sel, sums=sums, min_depth=MIN_DEPTH)
        clip = np.stack([cover["span_begin"], cover["span_end"]], axis=1).astype(np.int32).reshape(-1)
        reads, arcs = e.overlap_graph(lens, sel=sel, sums=sums, clip=clip)
        clip2 = tc.narrowed_clip(clip)
        reads2, arcs2 = e.overlap_graph(lens, sel=sel, sums=sums, clip=clip2)
        arc_flags, _, _ = e.clean_graph(lens, reads, arcs, clip=clip)
        cleaned = arcs.copy()
        cleaned["flags"] = arc_flags
        utg = {0: e.unitigs(lens, reads, arcs, clip=clip, tip_reads=0, seq=True),
               3: e.unitigs(lens, reads, cleaned, clip=clip, tip_reads=3, seq=True)}
        e.pileup_begin(ins_slots=INS_SLOTS)
        e.pileup_add(sel=sel, rc_from=nf)
        table, read_at, seq, _ = e.pileup_corrected(min_depth=MIN_DEPTH, ins=True)
        _, paths, words = e.candidates_paths(sel=sel, rc_from=nf)
        by_side = {s: e.read_coverage(lens, sel=sel, sums=sums, sides=s, min_depth=MIN_DEPTH, depth=True) for s in tc.SIDES}
        records = e.candidates_fetch(n).copy()
    finally:
        e.close()
    ops = [words[int(p["op_offset"]):int(p["op_offset"]) + int(p["n_ops"])] for p in paths]
    return dict(rs=rs, law=law, cands=np.concatenate([cf, cr]), nf=nf, lens=lens, records=records, sel=sel, sums=sums, clip=clip,
                reads=reads, arcs=arcs, clip2=clip2, reads2=reads2, arcs2=arcs2, cleaned=cleaned, utg=utg, table=table,
                read_at=read_at, seq=seq, ops=ops, by_side=by_side, cover=cover)


@pytest.fixture(scope="module")
def run_a():
    return device_path("A")


def test_the_block_is_not_trivial(run_a):
    p = run_a
    lens, clip = p["lens"], p["clip"]
    assert ((clip[0::2] > 0) | (clip[1::2] < lens)).any(), "no clip is narrower than its read"
    assert (p["utg"][0][1]["vertex"] & 1).any() and (p["utg"][3][1]["vertex"] & 1).any(), "no layout vertex is odd"
    assert p["utg"][3][0]["n_reads"].max() >= 8, "no unitig at tip_reads 3 holds 8 reads"
    assert (p["reads"]["contained_by"] >= 0).any(), "no read is contained"
    comp = p["records"]["comp"][p["sel"]]
    assert comp.any() and not comp.all() and not tc.false_hits(p["rs"], p["cands"], p["nf"])[0]
    print("block A on the device: %d candidates, %d selected, %d arcs (%d kept, %d after the cleaning), reads per unitig %s / %s" % (
        len(p["cands"]), len(p["sel"]), len(p["arcs"]), int((p["arcs"]["flags"] == 0).sum()), int((p["cleaned"]["flags"] == 0).sum()),
        p["utg"][0][0]["n_reads"].tolist(), p["utg"][3][0]["n_reads"].tolist()))


def test_check_1_record_ends(run_a):
    p = run_a
    f = tc.record_ends(p["rs"], p["records"], p["sel"], p["sums"])
    print("check 1, record ends:", f)
    assert f["ends"] == 2 * int(p["records"]["emitted"][p["sel"]].sum()) > 1000


def test_check_2_containments(run_a):
    p = run_a
    f = tc.containments(p["rs"], p["reads"], p["records"], p["clip"])
    print("check 2, containments:", f)
    assert f["contained"] == int((p["reads"]["contained_by"] >= 0).sum()) > 0
    print("check 2 under the narrowed clip:", tc.containments(p["rs"], p["reads2"], p["records"], p["clip2"]))


def test_check_3_arcs(run_a):
    p = run_a
    for what, arcs in (("the graph's", p["arcs"]), ("the cleaned", p["cleaned"])):
        f = tc.arcs(p["rs"], arcs, p["clip"], law=p["law"])
        print("check 3, %s arcs:" % what, f)
        assert f["checked"] == f["kept"] > 0


def test_check_3_arcs_between_reads_whose_clips_begin_well_inside_them(run_a):
    """the coverage's clip cuts at most 3 bases off a read that keeps an arc on this block; under a clip 300 narrower at both
    ends a len that is not measured between the clipped reads' heads is off by 300"""
    p = run_a
    f = tc.arcs(p["rs"], p["arcs2"], p["clip2"], law=p["law"])
    print("check 3, the arcs under a clip 300 narrower at both ends:", f)
    kept = p["arcs2"][p["arcs2"]["flags"] == 0]
    assert f["kept"] > 0 and (p["clip2"][2 * (kept["u"] >> 1)] >= 300).all()


def test_check_4_layout(run_a):
    p = run_a
    for k in (0, 3):
        unitigs, layout, places, _ = p["utg"][k]
        f = tc.layout(p["rs"], unitigs, layout, places, p["clip"], law=p["law"])
        print("check 4, layout at tip_reads %d:" % k, f)
        assert f["checked"] == len(unitigs) > 0


def test_check_5_unitig_bases(run_a):
    p = run_a
    for k in (0, 3):
        unitigs, layout, _, bases = p["utg"][k]
        f = tc.unitig_bases(p["rs"], unitigs, layout, bases, p["clip"])
        print("check 5, bases at tip_reads %d:" % k, [(j, n, round(r, 4), round(o, 4)) for j, n, r, o in f["rates"] if n > 1])


def test_check_6_corrected_reads(run_a):
    p = run_a
    f = tc.corrected(p["rs"], p["read_at"], p["seq"], range(0, p["rs"].n, 4))
    print("check 6, corrected reads 0, 4, 8, ...:", f, "inserted %d" % int(p["table"]["inserted"].sum()))
    assert f["reads"] == (p["rs"].n + 3) // 4 and int(p["table"]["inserted"].sum()) > 0


def test_check_7_alignment_columns(run_a):
    """every = and X op of every selected record's path, at its first and its last column, against the genome: the direction of
    the ops, which of I and D moves which read, the frame of a complement record's query -- inside the record, not at its ends"""
    p = run_a
    f = tc.alignment_columns(p["rs"], p["records"], p["sel"], p["sums"], p["ops"])
    print("check 7, alignment columns:", f)
    assert f["records"] == int(p["records"]["emitted"][p["sel"]].sum()) and f["run_ends"] > 100 * f["records"]


def test_check_8_depth_against_true_depth(run_a):
    """the per-base depth of read_coverage between the true depth of the overlaps narrowed by REACH and widened by END_SLACK, per
    side and for both: the mirror that puts a complement record's query interval on the stored read, and which read gets which
    interval"""
    p = run_a
    f = tc.depth_of_sides(p["rs"], p["records"], p["sel"], p["sums"], p["by_side"], MIN_DEPTH)
    print("check 8, depth against true depth:", f)
    print("check 8, positions (under, over) at reach 70 and a widening of 5:",
          tc.depth_misses(p["rs"], p["records"], p["sel"], p["by_side"]["both"][1], reach=70, slack=5))
    assert f["both"]["intervals"] == 2 * int(p["records"]["emitted"][p["sel"]].sum())
    assert p["by_side"]["both"][0].tobytes() == p["cover"].tobytes()         # (the table is the same with and without the depth)
    comp = p["records"]["comp"][p["sel"]] != 0
    assert (np.asarray(p["rs"].strand)[p["records"]["query_id"][p["sel"]][comp]] == 1).any()


def test_check_10_identities_of_true_records(run_a):
    p = run_a
    f = tc.identities(p["records"], p["sel"], p["sums"])
    print("check 10, identities on block A:", f)
    assert f["true"][0] == int(p["records"]["emitted"][p["sel"]].sum()) and f["false"][0] == 0


def test_block_b_false_hits_what_must_hold():
    p = device_path("B")
    utg = {k: p["utg"][k][:3] for k in (0, 3)}
    false = tc.false_hits(p["rs"], p["cands"], p["nf"])
    f = block_b_figures(p["rs"], p["law"], false, p["records"], p["sel"], p["sums"], p["clip"],
                        p["arcs"], p["cleaned"], utg, p["read_at"], p["seq"], range(0, p["rs"].n, 4))
    for k, v in f.items():
        print("block B on the device, %s: %s" % (k, v))
    assert f["of_reads_with_disjoint_spans"] > 0, "block B holds no false pair"
    f10 = tc.identities(p["records"], p["sel"], p["sums"], false=false[0])
    print("check 10, identities on block B:", f10)
    assert f10["false"][0] == f["false_hits_selected"] > 0
    f7 = tc.alignment_columns(p["rs"], p["records"], p["sel"], p["sums"], p["ops"], false=false[0])
    print("check 7, the alignment columns of block B's true records:", f7)
    assert f7["records"] == f10["true"][0]


@pytest.fixture(scope="module")
def run_p():
    """block P on the device: the contigs as the reference set, the reads and their reverse complements as the queries, the
    truth candidates run on both strands, summarised and placed ahead of the fetch"""
    from gact_amd import engine, synth
    b = block_p()
    rs, n, nf = b["rs"], len(b["cands"]), b["nf"]
    e = engine.Engine()
    try:
        e.upload_seqs(engine.SET_REF, b["seqs"])
        e.upload_seqs(engine.SET_QUERY, rs.reads)
        e.upload_seqs(engine.SET_QUERY_RC, [synth.revcomp(r) for r in rs.reads])
        e.candidates_upload(b["cands"])
        e.candidates_run_mixed(n, rc_from=nf, same_file=False)
        _, sums = e.candidates_summaries(n=n, rc_from=nf, same_file=False)
        lens = np.array([len(r) for r in rs.reads], dtype=np.int32)
        place, table = e.place_reads(lens, sums=sums)
        records = e.candidates_fetch(n).copy()
    finally:
        e.close()
    return dict(b, lens=lens, records=records, sums=sums, place=place, table=table)


def test_check_9_placements_on_contigs_with_a_decoy(run_p):
    """the primary where the read came from, a supplementary for every piece a contig boundary cuts off, the diverged copy a
    secondary of the true locus with a lower MAPQ; and the device's placement is the model's on the same records"""
    import place_model
    p = run_p
    f = tc.placements(p["rs"], p["contigs"], p["decoy"], p["records"], p["sums"], p["place"], p["table"])
    print("check 9, block P on the device: %d chains, %d forward;" % (len(p["cands"]), p["nf"]), f)
    assert f["ends"] == 2 * int(p["records"]["emitted"].sum()) and f["kinds"][tc.PRIMARY] == p["rs"].n
    want = place_model.place(p["records"], p["lens"], sums=p["sums"])
    for got, model, what in zip((p["place"], p["table"]), want, ("place", "reads")):
        for name in got.dtype.names:
            bad = np.flatnonzero(got[name] != model[name])
            assert len(bad) == 0, (what, name, bad[:5].tolist(), got[bad[:5]].tolist(), model[bad[:5]].tolist())
