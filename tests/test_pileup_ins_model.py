"""CPU suite for the inserted bases of the pileup (include/gact_hip.h gact_hip_pileup_begin_ins / gact_hip_pileup_corrected):
tests/pileup_ins_model.py against literals worked out by hand on reads of about 12 bases, the point of the feature against the
simulator's truth -- corrected reads lie closer to their genome spans with slots than without -- and the C-ABI of the three
entry points as a C compiler and the built library see it."""
import ctypes
import os
import subprocess

import numpy as np

import path_cases
from pileup_ins_model import pileup_ins, slot_calls
from pileup_model import pileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

READS = [b"ACGTACGTACGT",      # 0: the target
         b"TTTT",              # 1
         b"ACGTGGGACGT",       # 2: read 0's first eight bases with GGG inserted behind the fourth
         b"ACGTACGTCC",        # 3: read 0's last eight bases and two more
         b"ACGTGNGACGT",       # 4: read 2 with an N in the middle of the inserted run
         b"ACGTTACGT",         # 5: ... with one T inserted instead
         b"ACGTGGCGT",         # 6: GG inserted behind the fourth base, and the fifth (A) missing
         b"ACGTgtACGT"]        # 7: lower-case gt inserted
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
RC = [r.translate(_COMP)[::-1] for r in READS]


def rec(ref_id, query_id, ae, be, comp=0, emitted=1):
    return dict(ref_id=ref_id, query_id=query_id, ae=ae, be=be, comp=comp, emitted=emitted)


def run(records, cigars, min_depth, ins_slots, window=(0, 1)):
    return pileup_ins(READS, RC, records, cigars, window, min_depth, ins_slots)


def table_of(t):
    return [tuple(int(t[k][i]) for k in ("length", "inserted", "ins_sites", "deleted", "changed")) for i in range(len(t))]


def slots_at(ins, p):
    return ins[p].tolist()


def test_a_run_of_three_at_one_two_and_four_slots():
    one = [rec(0, 2, ae=8, be=11)], ["4=3I4="]
    G = [0, 0, 1, 0]
    for k, want, truncated in ((1, b"ACGTGACGTACGT", 1), (2, b"ACGTGGACGTACGT", 1), (4, b"ACGTGGGACGTACGT", 0)):
        ins, table, read_at, seq, runs_truncated = run(*one, 1, k)
        assert ins.shape == (12, k, 4) and int(ins.sum()) == min(k, 3)
        assert slots_at(ins, 4) == [G] * min(k, 3) + [[0] * 4] * (k - min(k, 3))        # in front of position 4, nowhere else
        assert seq == want and read_at.tolist() == [0, len(want)] and runs_truncated == truncated
        assert table_of(table) == [(len(want), min(k, 3), 1, 0, 0)]
    # no slots: the consensus with every '-' left out, no table
    ins, table, read_at, seq, runs_truncated = run(*one, 1, 0)
    assert ins.shape == (12, 0, 4) and seq == READS[0] and table_of(table) == [(12, 0, 0, 0, 0)] and runs_truncated == 1
    # position 4 is one deep: under min_depth 2 it is not called, and no slot of it is emitted
    ins, table, _, seq, _ = run(*one, 2, 4)
    assert int(ins.sum()) == 3 and seq == READS[0] and table_of(table) == [(12, 0, 0, 0, 0)]


def test_a_run_behind_the_reads_last_base_adds_nothing_to_the_slots():
    ins, table, read_at, seq, runs_truncated = run([rec(0, 3, ae=12, be=10)], ["8=2I"], 1, 1)
    assert not ins.any() and seq == READS[0] and runs_truncated == 1               # (two columns, one slot: truncated all the same)
    counts, _, _ = pileup(READS, RC, [rec(0, 3, ae=12, be=10)], ["8=2I"], (0, 1), 1)
    assert counts[11, 6] == 1                                                      # n[INS] as ever, clamped to the last position
    assert run([rec(0, 3, ae=12, be=10)], ["8=2I"], 1, 2)[4] == 0


def test_an_n_inside_a_run_and_a_slot_that_fails_in_front_of_one_that_would_pass():
    ins, table, read_at, seq, runs_truncated = run([rec(0, 4, ae=8, be=11)], ["4=3I4="], 1, 4)
    assert slots_at(ins, 4) == [[0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]          # the N keeps its slot and adds nothing
    emitted, byte = slot_calls(pileup(READS, RC, [rec(0, 4, ae=8, be=11)], ["4=3I4="], (0, 1), 1)[0], ins, 1)
    assert emitted[4].tolist() == [True, False, False, False]                      # slot 2 alone would pass: 2 * 1 > 1
    assert seq == b"ACGTGACGTACGT" and table_of(table) == [(13, 1, 1, 0, 0)] and runs_truncated == 0
    # lower-case inserted bases count as their upper-case ones and come out in upper case
    ins, _, _, seq, _ = run([rec(0, 7, ae=8, be=10)], ["4=2I4="], 1, 2)
    assert slots_at(ins, 4) == [[0, 0, 1, 0], [0, 0, 0, 1]] and seq == b"ACGTGTACGTACGT"


def test_a_tie_goes_to_the_first_of_a_c_g_t_and_half_the_depth_is_not_enough():
    recs, cigars = [rec(0, 5, ae=8, be=9), rec(0, 2, ae=8, be=11)], ["4=1I4=", "4=3I4="]              # T first, then GGG
    ins, table, _, seq, runs_truncated = run(recs, cigars, 1, 2)
    assert slots_at(ins, 4) == [[0, 0, 1, 1], [0, 0, 1, 0]]
    # slot 0: two of depth 2, G and T once each: G; slot 1: one of depth 2, 2 * 1 > 2 fails
    assert seq == b"ACGTGACGTACGT" and table_of(table) == [(13, 1, 1, 0, 0)] and runs_truncated == 1
    assert run(recs[::-1], cigars[::-1], 1, 2)[3] == seq
    # a third alignment without the insertion: slot 0 has two of depth 3 and still passes, with one it would not
    more = recs + [rec(0, 0, ae=12, be=12)]
    assert run(more, cigars + ["12="], 1, 2)[3] == b"ACGTGACGTACGT"
    assert run(more[1:], cigars[1:] + ["12="], 1, 2)[3] == READS[0]


def test_a_deleted_position_with_an_emitted_slot_in_front_of_it():
    ins, table, read_at, seq, _ = run([rec(0, 6, ae=8, be=9)], ["4=2I1D3="], 1, 2)
    assert slots_at(ins, 4) == [[0, 0, 1, 0], [0, 0, 1, 0]]
    assert seq == b"ACGTGGCGTACGT"                                                 # position 4: its two slots, its own byte left out
    assert table_of(table) == [(13, 2, 1, 1, 0)]


def test_windows_and_reads_back_to_back():
    recs = [rec(0, 2, ae=8, be=11), rec(2, 0, ae=4, be=4), rec(5, 2, ae=9, be=11)]
    cigars = ["4=3I4=", "4=", "4=1X2I4="]
    whole = pileup_ins(READS, RC, recs, cigars, (0, len(READS)), 1, 2)
    want = [b"ACGTGGACGTACGT", READS[1], READS[2], READS[3], READS[4], b"ACGTGGGACGT", READS[6], READS[7]]
    assert whole[3] == b"".join(want) and whole[2].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert table_of(whole[1])[5] == (11, 2, 1, 0, 1)
    part = pileup_ins(READS, RC, recs, cigars, (5, 2), 1, 2)
    assert part[3] == want[5] + want[6] and part[2].tolist() == [0, 11, 20] and part[0].shape == (18, 2, 4)
    assert part[1].tobytes() == whole[1][5:7].tobytes()
    empty = pileup_ins(READS, RC, recs, cigars, (3, 0), 1, 2)
    assert empty[0].shape == (0, 2, 4) and len(empty[1]) == 0 and empty[2].tolist() == [0] and empty[3] == b""


def _edit_distance(a, b):
    """the unit-cost edit distance of two uint8 arrays, row by row: the dependency inside a row is min.accumulate(row - j) + j"""
    j = np.arange(len(b) + 1, dtype=np.int64)
    row = j.copy()
    for i in range(1, len(a) + 1):
        t = np.empty_like(row)
        t[0] = i
        t[1:] = np.minimum(row[1:] + 1, row[:-1] + (b != a[i - 1]))
        row = np.minimum.accumulate(t - j) + j
    return int(row[-1])


def test_corrected_reads_lie_closer_to_the_genome_with_two_slots_than_with_none(oracle):
    """the point of the feature: the simulator leaves bases out of a read (30 % of its errors); without slots none of them can
    come back.  A handful of reads of the `tiny` block, every candidate on them aligned by the chain model, min_depth 3."""
    from gact_amd import engine, synth, workload
    blk = workload.make_block("tiny", candidates="synthetic")
    rs, nf = blk.rs, len(blk.cf)
    cands = np.concatenate([blk.cf, blk.cr])
    targets = (0, 1, 2, 3, 4, 5)
    sel = np.flatnonzero(np.isin(cands["ref_id"], targets) & (cands["ref_id"] != cands["query_id"]))
    assert len(sel) >= 4 * len(targets)
    exp = path_cases.expected(oracle, rs, cands, nf, sel)
    records = [dict(ref_id=int(cands[i]["ref_id"]), query_id=int(cands[i]["query_id"]), ae=e["ae"], be=e["be"], comp=int(i >= nf),
                    emitted=int(e["score"] > 0)) for i, e in zip(sel.tolist(), exp)]
    cigars = [e["cigar"] for e in exp]

    class Rc:
        def __getitem__(self, i):
            return rs.rc(i)

    total = {}
    for k in (0, 2):
        _, table, read_at, seq, _ = pileup_ins(rs.reads, Rc(), records, cigars, (0, len(targets)), 3, k)
        seq = np.frombuffer(seq, dtype=np.uint8)
        total[k] = 0
        for i in targets:
            truth = rs.genome[rs.start[i]:rs.start[i] + rs.span[i]]
            truth = synth.revcomp(truth) if rs.strand[i] else truth
            total[k] += _edit_distance(seq[read_at[i]:read_at[i + 1]], truth)
        if k:
            assert int(table["inserted"].sum()) > 0
    raw = sum(_edit_distance(rs.reads[i], synth.revcomp(rs.genome[rs.start[i]:rs.start[i] + rs.span[i]]) if rs.strand[i]
                             else rs.genome[rs.start[i]:rs.start[i] + rs.span[i]]) for i in targets)
    print("edit distance to the genome spans of %d reads (%d bases): raw %d, corrected without slots %d, with two slots %d"
          % (len(targets), sum(len(rs.reads[i]) for i in targets), raw, total[0], total[2]))
    assert total[2] < total[0]


def test_the_header_declares_the_records_and_the_library_exports_the_three_entry_points(hip_lib_path, tmp_path):
    from gact_amd import engine
    (tmp_path / "ins.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\n"
        "int main(void) { printf(\"%zu %zu %zu %zu %zu %d\\n\", sizeof(gact_pileup_ins), sizeof(gact_read_corrected), "
        "offsetof(gact_read_corrected, changed), sizeof(gact_pileup_ins_stats), offsetof(gact_pileup_ins_stats, emitted), "
        "GACT_PILEUP_MAX_INS_SLOTS); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "ins"), str(tmp_path / "ins.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "ins")]).split()]
    assert got[:2] == [16, 32]
    assert got == [engine.PILEUP_INS_DTYPE.itemsize, engine.READ_CORRECTED_DTYPE.itemsize, engine.READ_CORRECTED_DTYPE.fields["changed"][1],
                   ctypes.sizeof(engine.PileupInsStats), engine.PileupInsStats.emitted.offset, engine.PILEUP_MAX_INS_SLOTS]
    lib = ctypes.CDLL(hip_lib_path)
    for name in ("gact_hip_pileup_begin_ins", "gact_hip_pileup_corrected", "gact_hip_last_pileup_ins_stats"):
        assert hasattr(lib, name), name
    # and they refuse before anything touches a device
    lib.gact_hip_last_error.restype = ctypes.c_char_p
    assert lib.gact_hip_pileup_begin_ins(None, 0, 0, 1) == -1 and b"NULL" in lib.gact_hip_last_error()
    assert lib.gact_hip_pileup_corrected(None, 1, None, None, None, None, ctypes.c_int64(0), None) == -1
    assert lib.gact_hip_last_pileup_ins_stats(None, None) == -1
