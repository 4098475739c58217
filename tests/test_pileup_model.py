"""CPU suite for the pileup rule (include/gact_hip.h gact_hip_pileup_*): tests/pileup_model.py against literals worked out by
hand on reads of about 12 bases, and the C-ABI of the four entry points as a C compiler and the built library see it."""
import ctypes
import os
import subprocess

import numpy as np

import pileup_model
from pileup_model import A, C, G, T, OTHER, DEL, INS, DEPTH, pileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

READS = [b"ACGTACGTACGT",      # 0: the target of most cases
         b"TTTT",              # 1: its reverse complement is AAAA
         b"ACGTGGGACGT",       # 2: read 0's first eight bases with GGG inserted behind the fourth
         b"ACGTACGTCC",        # 3: read 0's last eight bases and two more
         b"acNt",              # 4
         b"ACgTAC"]            # 5: a target with a lower-case base
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
RC = [r.translate(_COMP)[::-1] for r in READS]


def rec(ref_id, query_id, ae, be, comp=0, emitted=1):
    return dict(ref_id=ref_id, query_id=query_id, ae=ae, be=be, comp=comp, emitted=emitted)


def rows(n, **at):
    """n positions of zeros with the rows given as p<position>=(A, C, G, T, OTHER, DEL, INS, DEPTH)"""
    out = np.zeros((n, 8), dtype=np.uint32)
    for key, row in at.items():
        out[int(key[1:])] = row
    return out


def table_of(t):
    return [tuple(int(t[k][i]) for k in ("n_alignments", "max_depth", "called", "changed", "deleted", "ins_flagged")) for i in range(len(t))]


def test_an_insertion_run_of_three_counts_once():
    counts, cons, table = pileup(READS, RC, [rec(0, 2, ae=8, be=11)], ["4=3I4="], (0, 1), 1)
    want = rows(12, p0=(1, 0, 0, 0, 0, 0, 0, 1), p1=(0, 1, 0, 0, 0, 0, 0, 1), p2=(0, 0, 1, 0, 0, 0, 0, 1), p3=(0, 0, 0, 1, 0, 0, 0, 1),
                p4=(1, 0, 0, 0, 0, 0, 1, 1), p5=(0, 1, 0, 0, 0, 0, 0, 1), p6=(0, 0, 1, 0, 0, 0, 0, 1), p7=(0, 0, 0, 1, 0, 0, 0, 1))
    assert np.array_equal(counts, want)
    assert bytes(cons) == b"ACGTACGTACGT"
    assert table_of(table) == [(1, 1, 8, 0, 0, 1)]                 # position 4: 2 * 1 insertion run > depth 1
    # the same alignment as op words
    ops = np.array([(4 << 4) | 7, (3 << 4) | 1, (4 << 4) | 7], dtype=np.uint32)
    again = pileup(READS, RC, [rec(0, 2, ae=8, be=11)], [ops], (0, 1), 1)
    assert np.array_equal(again[0], want) and bytes(again[1]) == bytes(cons)


def test_an_insertion_run_at_the_alignments_end_is_clamped_to_the_last_position():
    counts, cons, table = pileup(READS, RC, [rec(0, 3, ae=12, be=10)], ["8=2I"], (0, 1), 1)
    want = rows(12, p4=(1, 0, 0, 0, 0, 0, 0, 1), p5=(0, 1, 0, 0, 0, 0, 0, 1), p6=(0, 0, 1, 0, 0, 0, 0, 1), p7=(0, 0, 0, 1, 0, 0, 0, 1),
                p8=(1, 0, 0, 0, 0, 0, 0, 1), p9=(0, 1, 0, 0, 0, 0, 0, 1), p10=(0, 0, 1, 0, 0, 0, 0, 1), p11=(0, 0, 0, 1, 0, 0, 1, 1))
    assert np.array_equal(counts, want)
    assert table_of(table) == [(1, 1, 8, 0, 0, 1)]
    # a run in front of the alignment's first column sits at its first position; one between two columns at the second one's
    counts, _, _ = pileup(READS, RC, [rec(0, 3, ae=8, be=9)], ["2I3=1I3="], (0, 1), 1)
    assert counts[:, INS].tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0] and counts[:, DEPTH].tolist() == [0, 0] + [1] * 6 + [0] * 4


def test_a_reverse_complement_record_reads_the_rc_set_and_complements_nothing():
    counts, cons, table = pileup(READS, RC, [rec(0, 1, ae=4, be=4, comp=1)], ["1=3X"], (0, 1), 1)
    assert np.array_equal(counts, rows(12, p0=(1, 0, 0, 0, 0, 0, 0, 1), p1=(1, 0, 0, 0, 0, 0, 0, 1), p2=(1, 0, 0, 0, 0, 0, 0, 1),
                                       p3=(1, 0, 0, 0, 0, 0, 0, 1)))
    assert bytes(cons) == b"AAAAACGTACGT"
    assert table_of(table) == [(1, 1, 4, 3, 0, 0)]
    forward, _, _ = pileup(READS, RC, [rec(0, 1, ae=4, be=4, comp=0)], ["4X"], (0, 1), 1)
    assert forward[:4, T].tolist() == [1, 1, 1, 1] and forward[:, A].sum() == 0


def test_n_and_lower_case_and_a_position_where_every_query_byte_is_other():
    counts, cons, table = pileup(READS, RC, [rec(0, 4, ae=4, be=4)], ["4X"], (0, 1), 1)
    assert np.array_equal(counts, rows(12, p0=(1, 0, 0, 0, 0, 0, 0, 1), p1=(0, 1, 0, 0, 0, 0, 0, 1), p2=(0, 0, 0, 0, 1, 0, 0, 1),
                                       p3=(0, 0, 0, 1, 0, 0, 0, 1)))
    assert bytes(cons) == b"ACGTACGTACGT"                          # position 2: depth 1, all five kinds zero: the read's own G
    assert table_of(table) == [(1, 1, 4, 0, 0, 0)]                 # ... which is called and not changed
    # a lower-case base of the target: upper case in the consensus where called, not changed; as it is where not called
    recs = [rec(5, 0, ae=6, be=6), rec(5, 0, ae=4, be=4)]
    counts, cons, table = pileup(READS, RC, recs, ["6=", "4="], (5, 1), 2)
    assert counts[:, DEPTH].tolist() == [2, 2, 2, 2, 1, 1] and counts[2].tolist() == [0, 0, 2, 0, 0, 0, 0, 2]
    assert bytes(cons) == b"ACGTAC" and table_of(table) == [(2, 2, 4, 0, 0, 0)]
    _, cons, table = pileup(READS, RC, recs, ["6=", "4="], (5, 1), 3)
    assert bytes(cons) == b"ACgTAC" and table_of(table) == [(2, 2, 0, 0, 0, 0)]


def test_every_tie_rule():
    def n(a=0, c=0, g=0, t=0, other=0, dele=0, ins=0):
        return np.array([a, c, g, t, other, dele, ins, a + c + g + t + other + dele], dtype=np.uint32)

    cases = [(n(c=2, g=2), b"G", b"G"),            # the read's own base is among the tied kinds
             (n(c=2, g=2), b"g", b"G"),            # ... case folded
             (n(a=2, c=2), b"G", b"A"),            # it is not: the order A C G T DEL
             (n(c=1, t=1, dele=1), b"A", b"C"),
             (n(t=1, dele=1), b"A", b"T"),
             (n(t=1, dele=1), b"N", b"T"),
             (n(a=1, dele=2), b"A", b"-"),         # no tie: a deletion wins
             (n(dele=1), b"C", b"-"),
             (n(a=1, other=3), b"C", b"A"),        # OTHER never wins
             (n(other=3), b"c", b"c"),             # all five zero: the read's own byte as it is
             (n(other=3), b"N", b"N"),
             (n(a=1, c=3, g=2, t=1), b"A", b"C")]
    for counts, own, want in cases:
        assert pileup_model.call(counts, own[0], 1) == want[0], (counts, own, want)
        assert pileup_model.call(counts, own[0], int(counts[DEPTH]) + 1) == own[0]
    stacked = np.stack([c for c, _, _ in cases])
    own = np.frombuffer(b"".join(o for _, o, _ in cases), dtype=np.uint8)
    assert bytes(pileup_model.consensus_of(stacked, own, 1)) == b"".join(w for _, _, w in cases)
    assert bytes(pileup_model.consensus_of(stacked, own, 8)) == bytes(own)
    # through the pileup: read 0's position 0 is one deep (under min_depth); position 1 (own C) sees one C and two T: T;
    # position 2 (own G) sees G, T and a deletion once each: the read's own; position 3 (own T) sees T and a deletion: its own
    recs = [rec(0, 0, ae=4, be=4), rec(0, 1, ae=3, be=2), rec(0, 1, ae=4, be=1)]
    counts, cons, table = pileup(READS, RC, recs, ["4=", "2X", "1X2D"], (0, 1), 2)
    assert counts[:4].tolist() == [[1, 0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 2, 0, 0, 0, 3], [0, 0, 1, 1, 0, 1, 0, 3], [0, 0, 0, 1, 0, 1, 0, 2]]
    assert bytes(cons[:4]) == b"ATGT" and table_of(table) == [(3, 3, 3, 1, 0, 0)]


def test_min_depth_on_both_sides_of_the_threshold():
    recs = [rec(0, 1, ae=4, be=4), rec(0, 1, ae=3, be=3)]                  # TTTT over ACGT, TTT over ACG
    for min_depth, want, table in ((1, b"TTTTACGTACGT", (2, 2, 4, 3, 0, 0)), (2, b"TTTTACGTACGT", (2, 2, 3, 3, 0, 0)),
                                   (3, b"ACGTACGTACGT", (2, 2, 0, 0, 0, 0))):
        counts, cons, t = pileup(READS, RC, recs, ["3X1=", "3X"], (0, 1), min_depth)
        assert counts[:, DEPTH].tolist() == [2, 2, 2, 1] + [0] * 8
        assert bytes(cons) == want and table_of(t) == [table], min_depth
    # a deletion at exactly min_depth is called, one short of it is the read's own byte
    recs = [rec(0, 1, ae=2, be=1), rec(0, 1, ae=2, be=1)]
    for min_depth, want, table in ((2, b"T-GT", (2, 2, 2, 1, 1, 0)), (3, b"ACGT", (2, 2, 0, 0, 0, 0))):
        _, cons, t = pileup(READS, RC, recs, ["1X1D", "1X1D"], (0, 1), min_depth)
        assert bytes(cons[:4]) == want and table_of(t) == [table]


def test_records_outside_the_window_not_emitted_or_without_columns_add_nothing():
    recs = [rec(0, 2, ae=8, be=11), rec(1, 0, ae=4, be=4), rec(1, 0, ae=4, be=4, emitted=0), rec(1, 0, ae=2, be=2), rec(2, 0, ae=4, be=4)]
    cigars = ["4=3I4=", "4X", "4X", "", "4="]
    counts, cons, table = pileup(READS, RC, recs, cigars, (1, 1), 1)
    assert counts.shape == (4, 8) and counts[:, A].tolist() == [1, 0, 0, 0] and counts[:, DEPTH].tolist() == [1, 1, 1, 1]
    assert bytes(cons) == b"ACGT" and table_of(table) == [(1, 1, 4, 3, 0, 0)]
    # the full window is the windows' results one after the other
    whole = pileup(READS, RC, recs, cigars, (0, len(READS)), 1)
    lens = np.cumsum([0] + [len(r) for r in READS])
    assert np.array_equal(whole[0][lens[1]:lens[2]], counts) and bytes(whole[1][lens[1]:lens[2]]) == bytes(cons)
    assert table_of(whole[2]) == [(1, 1, 8, 0, 0, 1), (1, 1, 4, 3, 0, 0), (1, 1, 4, 0, 0, 0), (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0),
                                  (0, 0, 0, 0, 0, 0)]
    empty = pileup(READS, RC, recs, cigars, (2, 0), 1)
    assert empty[0].shape == (0, 8) and len(empty[1]) == 0 and len(empty[2]) == 0
    assert OTHER == 4 and DEL == 5 and INS == 6 and (C, G, T) == (1, 2, 3)


def test_the_header_declares_the_two_records_and_the_library_exports_the_four_entry_points(hip_lib_path, tmp_path):
    from gact_amd import engine
    (tmp_path / "pileup.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\n"
        "int main(void) { printf(\"%zu %zu %zu %zu %d %d\\n\", sizeof(gact_pileup_col), sizeof(gact_read_pileup), "
        "offsetof(gact_read_pileup, ins_flagged), sizeof(gact_pileup_stats), GACT_PILEUP_INS, GACT_PILEUP_DEPTH); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "pileup"), str(tmp_path / "pileup.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "pileup")]).split()]
    assert got[:2] == [32, 32]
    assert got == [engine.PILEUP_COL_DTYPE.itemsize, engine.READ_PILEUP_DTYPE.itemsize, engine.READ_PILEUP_DTYPE.fields["ins_flagged"][1],
                   ctypes.sizeof(engine.PileupStats), engine.PILEUP_INS, engine.PILEUP_DEPTH]
    lib = ctypes.CDLL(hip_lib_path)
    for name in ("gact_hip_pileup_begin", "gact_hip_pileup_add", "gact_hip_pileup_finish", "gact_hip_last_pileup_stats"):
        assert hasattr(lib, name), name
    # and they refuse before anything touches a device
    lib.gact_hip_last_error.restype = ctypes.c_char_p
    assert lib.gact_hip_pileup_begin(None, 0, 0) == -1 and b"NULL" in lib.gact_hip_last_error()
    assert lib.gact_hip_pileup_add(None, 0, 0, None, 0, 1) == -1
    assert lib.gact_hip_pileup_finish(None, 1, None, None, None) == -1
    assert lib.gact_hip_last_pileup_stats(None, None) == -1
