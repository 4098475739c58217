"""CPU suite for the variants of the pileup (gact_hip_pileup_variants, gact_hip_format_vcf): tests/variant_model.py held to
records worked out by hand at every edge of the rule; gact_hip_format_vcf through ctypes against the restated formatter; the
planted cases of tests/variant_cases.py through the oracle's chains and tests/pileup_model.py, so that the CPU shows they give
the counts they were planted for before a GPU sees them (the longest left-out run the chain model carries at the default tile
and scoring is the 130 of variant_cases.LONGEST_RUN); and truth block V (tests/variant_truth.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import path_cases
import variant_cases
import variant_model
from pileup_ins_model import slot_counts
from pileup_model import pileup
from variant_model import DEL_KIND, INS_KIND, SNV_KIND, TRUNCATED, variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(min_depth=8, min_alt=4, min_permille=250, hom_permille=750)         # the defaults


def col(A=0, C=0, G=0, T=0, other=0, dele=0, ins=0):
    return [A, C, G, T, other, dele, ins, A + C + G + T + other + dele]


def call(cols, own, offsets=None, ins=None, seq_first=0, **params):
    counts = np.array(cols, dtype=np.uint32).reshape(-1, 8)
    own = np.frombuffer(own, dtype=np.uint8)
    offsets = [0, len(own)] if offsets is None else offsets
    ins = None if ins is None else np.array(ins, dtype=np.uint32).reshape(len(own), -1, 4)
    recs, table = variants(counts, ins, own, np.array(offsets, dtype=np.int64), seq_first=seq_first, **dict(P, **params))
    return [tuple(int(v) for v in r) for r in recs.tolist()], table


def rows(table):
    """the table's counted fields: (examined, n_ins, n_del, n_snv, first) per sequence"""
    assert not table["reserved"].any()
    return [tuple(int(t[k]) for k in ("examined", "n_ins", "n_del", "n_snv", "first")) for t in table]


def snv(seq, pos, base, alt, depth, gt):
    return (seq, pos, SNV_KIND, 1, ord(base), alt, depth, gt)


def test_defaults_are_the_headers():
    assert variant_model.DEFAULTS == P
    from gact_amd import engine
    assert engine.VARIANT_DEFAULTS == P


def test_min_alt_and_min_permille_at_their_edges():
    # a = min_alt - 1 and a = min_alt at a depth where the permille is no obstacle
    got, _ = call([col(A=9, C=3), col(A=8, C=4)], b"AA")
    assert got == [snv(0, 1, "C", 4, 12, 1)]
    # 1000 a == min_permille d exactly (4 of 16), and one read more depth (4 of 17: 4000 < 4250)
    got, _ = call([col(A=12, C=4), col(A=13, C=4)], b"AA")
    assert got == [snv(0, 0, "C", 4, 16, 1)]
    # the same edge with a parameter that does not divide: 7 of 27 at 260 (7000 < 7020), 7 of 26 at 270 (7000 < 7020), 7 of 25 at 280
    assert call([col(G=20, T=7)], b"G", min_permille=260)[0] == []
    assert call([col(G=19, T=7)], b"G", min_permille=270)[0] == []
    assert call([col(G=18, T=7)], b"G", min_permille=280)[0] == [snv(0, 0, "T", 7, 25, 1)]
    # min_permille 0: min_alt alone decides
    assert call([col(G=996, T=4)], b"G", min_permille=0)[0] == [snv(0, 0, "T", 4, 1000, 1)]


def test_the_hom_boundary():
    got, _ = call([col(A=2, C=6), col(A=3, C=5)], b"AA")
    assert got == [snv(0, 0, "C", 6, 8, 2), snv(0, 1, "C", 5, 8, 1)]               # 6000 >= 6000; 5000 < 6000
    got, _ = call([col(A=2, C=6)], b"A", hom_permille=751)
    assert got == [snv(0, 0, "C", 6, 8, 1)]                                        # 6000 < 6008
    got, _ = call([col(C=8)], b"A", hom_permille=1000)
    assert got == [snv(0, 0, "C", 8, 8, 2)]
    got, _ = call([col(A=4, C=4)], b"A", min_permille=500, hom_permille=500)
    assert got == [snv(0, 0, "C", 4, 8, 2)]


def test_min_depth_and_a_position_below_it_splits_a_run():
    gone = col(A=2, dele=6)
    got, table = call([gone, gone, col(dele=7), gone, gone], b"ACGTA")
    assert got == [(0, 0, DEL_KIND, 2, 0, 6, 8, 2), (0, 3, DEL_KIND, 2, 0, 6, 8, 2)]
    assert rows(table) == [(4, 0, 2, 0, 0)]
    # ... and one that is examined and not deleted splits it too; alt, depth and gt are the FIRST position's
    got, _ = call([col(A=4, dele=4), col(C=1, dele=9), col(G=6, dele=3), col(dele=8)], b"ACGT")
    assert got == [(0, 0, DEL_KIND, 2, 0, 4, 8, 1), (0, 3, DEL_KIND, 1, 0, 8, 8, 2)]
    # depth min_depth - 1 makes no record of any kind, min_depth does
    assert call([col(C=7)], b"A")[0] == [] and call([col(C=8)], b"A")[0] == [snv(0, 0, "C", 8, 8, 2)]
    assert call([col(C=1)], b"A", min_depth=1, min_alt=1)[0] == [snv(0, 0, "C", 1, 1, 2)]


def test_own_bytes_n_lower_case_and_two_alts_at_one_position():
    got, _ = call([col(A=4, C=4, T=4), col(A=4, C=4, T=4), col(A=4, C=4, T=4), col(A=4, C=4, G=4, T=4)], b"NatG")
    assert got == [snv(0, 1, "C", 4, 12, 1), snv(0, 1, "T", 4, 12, 1),             # own 'a': A is no alt; C then T
                   snv(0, 2, "A", 4, 12, 1), snv(0, 2, "C", 4, 12, 1),             # own 't'
                   snv(0, 3, "A", 4, 16, 1), snv(0, 3, "C", 4, 16, 1), snv(0, 3, "T", 4, 16, 1)]
    # an N still has its deletion and its insertion; OTHER counts into the depth and is never an alt
    got, _ = call([col(other=4, dele=4)], b"N", ins=[[4, 0, 0, 0]])
    assert got == [(0, 0, INS_KIND, 1, ord("A"), 4, 8, 1 | TRUNCATED), (0, 0, DEL_KIND, 1, 0, 4, 8, 1)]
    # an SNV inside a called deletion is reported on its own, behind the run's record at the run's first position
    got, _ = call([col(C=4, dele=4), col(A=4, dele=4)], b"AA")
    assert got == [(0, 0, DEL_KIND, 2, 0, 4, 8, 1), snv(0, 0, "C", 4, 8, 1)]


def test_insertions_their_length_their_bases_and_truncated():
    deep = col(A=8)
    got, _ = call([deep] * 5, b"AAAAA", ins=[[[2, 2, 0, 0], [0, 0, 1, 3]],         # both slots: len 2 == K, a tie goes to A
                                             [[0, 0, 0, 4], [1, 1, 1, 0]],         # slot 1 has 3 < min_alt: len 1
                                             [[1, 1, 1, 0], [0, 8, 0, 0]],         # slot 0 fails: no record, whatever slot 1 has
                                             [[0, 8, 0, 0], [0, 0, 0, 0]],
                                             [[0, 0, 0, 0], [0, 0, 0, 0]]])
    assert got == [(0, 0, INS_KIND, 2, ord("A") | ord("T") << 8, 4, 8, 1 | TRUNCATED), (0, 1, INS_KIND, 1, ord("T"), 4, 8, 1),
                   (0, 3, INS_KIND, 1, ord("C"), 8, 8, 2)]
    # one slot: every record is truncated; four slots; no slots: no record
    got, _ = call([deep], b"A", ins=[[[0, 0, 4, 0]]])
    assert got == [(0, 0, INS_KIND, 1, ord("G"), 4, 8, 1 | TRUNCATED)]
    got, _ = call([deep], b"A", ins=[[[4, 0, 0, 0], [0, 4, 0, 0], [0, 0, 4, 0], [0, 0, 0, 4]]])
    assert got == [(0, 0, INS_KIND, 4, int.from_bytes(b"ACGT", "little"), 4, 8, 1 | TRUNCATED)]
    assert call([deep], b"A")[0] == []
    # the three kinds at one position: INS, DEL, SNV
    got, _ = call([col(A=1, G=5, dele=6)], b"A", ins=[[[0, 0, 0, 6]]])
    assert [r[2] for r in got] == [INS_KIND, DEL_KIND, SNV_KIND] and got[0][3:] == (1, ord("T"), 6, 12, 1 | TRUNCATED)


def test_runs_never_cross_a_sequence_boundary_and_the_table():
    gone = col(dele=8)
    # sequence 5 ends deleted, sequence 6 is empty, sequence 7 starts deleted: two records
    got, table = call([col(A=8), gone, gone, gone, col(C=8)], b"AAAAC", offsets=[0, 3, 3, 5], seq_first=5)
    assert got == [(5, 1, DEL_KIND, 2, 0, 8, 8, 2), (7, 0, DEL_KIND, 1, 0, 8, 8, 2)]
    assert rows(table) == [(3, 0, 1, 0, 0), (0, 0, 0, 0, 1), (2, 0, 1, 0, 1)]
    got, table = call([], b"", offsets=[0, 0])
    assert got == [] and rows(table) == [(0, 0, 0, 0, 0)]
    assert call([], b"", offsets=[0])[1].shape == (0,)


@pytest.mark.parametrize("bad", [dict(min_depth=0), dict(min_alt=0), dict(min_permille=-1), dict(hom_permille=1001),
                                 dict(min_permille=800)])
def test_the_model_refuses_what_the_library_refuses(bad):
    assert not variant_model.check_params(**dict(P, **bad)) and variant_model.check_params(**P)


# ---- gact_hip_format_vcf

def _vcf(lib, v, name, seq, cap=4096):
    from gact_amd import engine
    v = np.array([v], dtype=engine.VARIANT_DTYPE)
    s = np.frombuffer(seq, dtype=np.uint8)
    buf = ctypes.create_string_buffer(b"\xff" * max(cap, 1), max(cap, 1))
    n = lib.gact_hip_format_vcf(v.ctypes.data, name, s.ctypes.data, len(s), buf if cap else None, cap)
    return n, buf.raw


VCF_SEQ = b"acgtNACGTTG"
VCF_RECORDS = [
    ((3, 0, SNV_KIND, 1, ord("T"), 5, 9, 1), "c1\t1\t.\tA\tT\t.\t.\tDP=9;AD=5\tGT\t0/1\n"),
    ((3, 4, SNV_KIND, 1, ord("C"), 9, 9, 2), "c1\t5\t.\tN\tC\t.\t.\tDP=9;AD=9\tGT\t1/1\n"),
    ((3, 10, SNV_KIND, 1, ord("A"), 4, 16, 1), "c1\t11\t.\tG\tA\t.\t.\tDP=16;AD=4\tGT\t0/1\n"),
    ((3, 2, DEL_KIND, 3, 0, 4, 8, 1), "c1\t2\t.\tCGTN\tC\t.\t.\tDP=8;AD=4\tGT\t0/1\n"),
    ((3, 9, DEL_KIND, 2, 0, 8, 8, 2), "c1\t9\t.\tTTG\tT\t.\t.\tDP=8;AD=8\tGT\t1/1\n"),
    ((3, 0, DEL_KIND, 2, 0, 4, 8, 1), "c1\t1\t.\tACG\tG\t.\t.\tDP=8;AD=4\tGT\t0/1\n"),
    ((3, 0, DEL_KIND, 10, 0, 4, 8, 1), "c1\t1\t.\tACGTNACGTTG\tG\t.\t.\tDP=8;AD=4\tGT\t0/1\n"),
    ((3, 0, DEL_KIND, 11, 0, 4, 8, 1), ""),
    ((3, 5, INS_KIND, 2, ord("G") | ord("T") << 8, 4, 8, 1 | TRUNCATED), "c1\t5\t.\tN\tNGT\t.\t.\tDP=8;AD=4\tGT\t0/1\n"),
    ((3, 1, INS_KIND, 1, ord("A"), 6, 8, 2), "c1\t1\t.\tA\tAA\t.\t.\tDP=8;AD=6\tGT\t1/1\n"),
    ((3, 0, INS_KIND, 3, int.from_bytes(b"CAT", "little"), 4, 8, 1), "c1\t1\t.\tA\tCATA\t.\t.\tDP=8;AD=4\tGT\t0/1\n"),
    ((3, 10, INS_KIND, 4, int.from_bytes(b"ACGT", "little"), 4, 8, 1 | TRUNCATED), "c1\t10\t.\tT\tTACGT\t.\t.\tDP=8;AD=4\tGT\t0/1\n"),
]


def test_format_vcf_every_kind_at_pos_0_and_behind_against_the_restated_formatter(hip_lib_path):
    from gact_amd import engine
    lib = engine.load()
    for rec, line in VCF_RECORDS:
        v = np.array([rec], dtype=engine.VARIANT_DTYPE)[0]
        assert variant_model.format_vcf(v, "c1", VCF_SEQ) == line, rec           # the restatement, to the lines written by hand
        n, raw = _vcf(lib, rec, b"c1", VCF_SEQ)
        assert n == len(line) and raw[:n + 1] == line.encode() + b"\0", (rec, raw[:n + 1])
        assert engine.format_vcf(v, "c1", VCF_SEQ) == line
        if line:
            # a short buffer: the length, nothing useful in buf, nothing written behind it
            for cap in (0, 1, len(line) - 1, len(line)):
                n, raw = _vcf(lib, rec, b"c1", VCF_SEQ, cap=cap)
                assert n == len(line) and raw[cap:] == b"\xff" * (len(raw) - cap) and (cap == 0 or raw[0] == 0), (rec, cap)
            n, raw = _vcf(lib, rec, b"c1", VCF_SEQ, cap=len(line) + 1)
            assert n == len(line) and raw == line.encode() + b"\0"


def test_format_vcf_refusals(hip_lib_path):
    from gact_amd import engine
    lib = engine.load()
    for rec, why in (((0, 0, 3, 1, ord("A"), 4, 8, 1), b"kind 3"), ((0, 0, SNV_KIND, 1, ord("A"), 4, 8, 0), b"gt 0"),
                     ((0, 0, SNV_KIND, 1, ord("A"), 4, 8, 3), b"gt 3"), ((0, 11, SNV_KIND, 1, ord("A"), 4, 8, 1), b"pos 11"),
                     ((0, -1, SNV_KIND, 1, ord("A"), 4, 8, 1), b"pos -1"), ((0, 2, SNV_KIND, 1, ord("a"), 4, 8, 1), b"SNV"),
                     ((0, 2, SNV_KIND, 2, ord("A"), 4, 8, 1), b"SNV"), ((0, 5, DEL_KIND, 7, 0, 4, 8, 1), b"ends behind"),
                     ((0, 5, DEL_KIND, 0, 0, 4, 8, 1), b"len 0"), ((0, 5, INS_KIND, 5, 0x41414141, 4, 8, 1), b"len 5"),
                     ((0, 5, INS_KIND, 2, ord("A"), 4, 8, 1), b"inserted byte 0"), ((0, 5, INS_KIND, 1, ord("N"), 4, 8, 1), b"inserted byte")):
        n, _ = _vcf(lib, rec, b"c1", VCF_SEQ)
        assert n == -1 and why in lib.gact_hip_last_error(), (rec, lib.gact_hip_last_error())
    v = np.array([VCF_RECORDS[0][0]], dtype=engine.VARIANT_DTYPE)
    s = np.frombuffer(VCF_SEQ, dtype=np.uint8)
    buf = ctypes.create_string_buffer(64)
    assert lib.gact_hip_format_vcf(None, b"c", s.ctypes.data, len(s), buf, 64) == -1
    assert lib.gact_hip_format_vcf(v.ctypes.data, None, s.ctypes.data, len(s), buf, 64) == -1
    assert lib.gact_hip_format_vcf(v.ctypes.data, b"c", None, len(s), buf, 64) == -1
    assert lib.gact_hip_format_vcf(v.ctypes.data, b"c", s.ctypes.data, len(s), None, 64) == -1


def test_the_header_declares_the_records_and_the_library_refuses_without_a_device(hip_lib_path, tmp_path):
    from gact_amd import engine
    (tmp_path / "v.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\n"
        "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d\\n\", sizeof(gact_variant), offsetof(gact_variant, bases), "
        "offsetof(gact_variant, flags), sizeof(gact_seq_variants), offsetof(gact_seq_variants, first), sizeof(gact_variant_stats), "
        "GACT_VARIANT_CHUNK, GACT_VARIANT_INS, GACT_VARIANT_DEL, GACT_VARIANT_SNV, GACT_VARIANT_TRUNCATED, GACT_VARIANT_DEFAULT_MIN_DEPTH, "
        "GACT_VARIANT_DEFAULT_MIN_ALT, GACT_VARIANT_DEFAULT_MIN_PERMILLE, GACT_VARIANT_DEFAULT_HOM_PERMILLE); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "v"), str(tmp_path / "v.c")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "v")]).split()]
    D = engine.VARIANT_DEFAULTS
    assert got == [engine.VARIANT_DTYPE.itemsize, engine.VARIANT_DTYPE.fields["bases"][1], engine.VARIANT_DTYPE.fields["flags"][1],
                   engine.SEQ_VARIANTS_DTYPE.itemsize, engine.SEQ_VARIANTS_DTYPE.fields["first"][1], ctypes.sizeof(engine.VariantStats),
                   engine.VARIANT_CHUNK, engine.VARIANT_INS, engine.VARIANT_DEL, engine.VARIANT_SNV, engine.VARIANT_TRUNCATED,
                   D["min_depth"], D["min_alt"], D["min_permille"], D["hom_permille"]]
    assert got[0] == 32 and got[3] == 32 and engine.VARIANT_CHUNK % 64 == 0
    assert (INS_KIND, DEL_KIND, SNV_KIND, TRUNCATED) == (engine.VARIANT_INS, engine.VARIANT_DEL, engine.VARIANT_SNV, engine.VARIANT_TRUNCATED)
    lib = ctypes.CDLL(hip_lib_path)
    lib.gact_hip_last_error.restype = ctypes.c_char_p
    assert lib.gact_hip_pileup_variants(None, None, None, ctypes.c_int64(0), None, None) == -1 and b"NULL" in lib.gact_hip_last_error()
    assert lib.gact_hip_last_variant_stats(None, None) == -1
    for name in ("gact_hip_pileup_variants", "gact_hip_last_variant_stats", "gact_hip_format_vcf"):
        assert name in engine.EXPORTS


# ---- the planted cases, through the oracle's chains

def chain_counts(oracle, case):
    """the window's counts and slot table as the chain model's alignments of the case's candidates make them"""
    nf = len(case.cands)
    exp = path_cases.expected(oracle, case.rs, case.cands, nf, threshold=variant_cases.THRESHOLD)
    recs = [dict(ref_id=int(c["ref_id"]), query_id=int(c["query_id"]), ae=e["ae"], be=e["be"], comp=0, emitted=int(e["score"] > 0))
            for c, e in zip(case.cands, exp)]
    cigars = [e["cigar"] for e in exp]
    counts, _, _ = pileup(case.rs.reads, None, recs, cigars, case.window, 1)
    ins = slot_counts(case.rs.reads, None, recs, cigars, case.window, case.ins_slots)[0] if case.ins_slots else None
    return counts, ins, cigars


@pytest.mark.parametrize("name", sorted(variant_cases.cases()))
def test_a_planted_case_gives_the_records_it_was_planted_for(oracle, name):
    case = variant_cases.cases()[name]
    counts, ins, cigars = chain_counts(oracle, case)
    own, offs = variant_cases.own_and_offsets(case)
    got, table = variants(counts, ins, own, offs, seq_first=case.window[0], **case.params)
    assert got.tolist() == case.want.tolist(), (name, cigars[0][:200])
    assert got.tobytes() == case.want.tobytes()
    # alt == a and depth == d exactly, at every record
    assert all(int(r["depth"]) == case.params["min_depth"] for r in got)
    assert variant_model.stats_of(table)["n_del"] == int((case.want["kind"] == DEL_KIND).sum())


def test_the_planted_cases_cover_what_they_aim_at():
    from gact_amd import engine
    cases = variant_cases.cases()
    CH = variant_cases.CHUNK
    assert CH == engine.VARIANT_CHUNK
    lengths = set()
    for c in cases.values():
        first, n = c.window
        lengths |= {len(c.rs.reads[first])}
        lengths |= {len(r) for r in c.rs.reads[first:first + n]} & {1}
    assert {1, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 200} <= lengths
    runs = np.concatenate([c.want[c.want["kind"] == DEL_KIND] for c in cases.values() if c.window[0] == 0])
    begin, end = runs["pos"].astype(np.int64), runs["pos"].astype(np.int64) + runs["len"]          # (window positions: one target)
    assert {1, 2, 64, 65, variant_cases.LONGEST_RUN} <= set(runs["len"].tolist()) and variant_cases.LONGEST_RUN >= 65
    assert np.any(begin % 64 == 63) and np.any((end - 1) % 64 == 0) and np.any((begin % 64 == 0) & (runs["len"] >= 64))
    assert np.any(begin // CH != (end - 1) // CH) and np.any(end - (begin // CH + 1) * CH > 64)     # across an edge; a peek of two steps
    assert np.any(end % CH == 0) and np.any(begin % CH == 0)
    snvs = np.concatenate([c.want[c.want["kind"] == SNV_KIND]["pos"] for n, c in cases.items() if n.startswith("snv-")])
    assert {4, 63, 64, CH - 1, CH} <= set(snvs.tolist())
    ins = cases["ins"].want[cases["ins"].want["kind"] == INS_KIND]
    assert sorted(ins["len"].tolist()) == [1, 1, 2, 2] and sorted((ins["flags"] & TRUNCATED).tolist()) == [0, 0, 4, 4]
    several = cases["several"]
    assert several.window[0] > 0 and several.ins_slots == variant_cases.K
    assert len(set(several.want["seq"].tolist())) >= 4 and {1, 2} <= set((several.want["flags"] & 3).tolist())


# ---- truth block V

def test_block_v_the_reference_path_finds_the_planted_variants(oracle):
    """Block V (tests/variant_truth.py) through the oracle's chains, pileup_model and variant_model, at 15 % read error, 30x and
    min_depth 8, min_alt 4, min_permille 250, hom_permille 600.  Measured: 65 of 70 planted SNVs found at the exact position with
    the exact base; 36 of the 37 het ones found and 27 of the 28 hom ones found have the planted genotype; 48 of 50 planted
    indels found within 3 bases with their kind and length; 0 SNV records unmatched on 20 kb of reference; 176 records in all,
    the rest insertions and deletions that no site was planted for (the simulator's errors are 60 % insertions)."""
    import variant_truth
    b = variant_truth.block_v()
    truth = b["truth"]
    assert len(truth) == 120 and len(b["seqs"]) == 2 and abs(len(b["h2"]) - len(b["h1"])) < 60
    sites = sorted(variant_truth.CONTIGS[c][0] + pos for c, pos, _, _, _, _ in truth)
    assert min(np.diff(sites)) >= variant_truth.APART
    assert all(variant_truth.FROM_ENDS <= pos < 10000 - variant_truth.FROM_ENDS for _, pos, _, _, _, _ in truth)
    f = variant_truth.reference_path(oracle)["figures"]
    print("block V, the CPU reference path:", f)
    variant_truth.check(f)
    assert f == dict(snv_planted=70, snv_found=65, het_found=37, het_right=36, hom_found=28, hom_right=27, indel_planted=50,
                     indel_found=48, snv_unmatched=0, records=176)


def test_simulate_reads_takes_a_genome_and_leaves_the_stream_alone_without_one():
    from gact_amd import synth
    kw = dict(n_reads=5, seed=7, mean_len=800, sd_len=100, min_len=300, max_len=1500)
    a, b = synth.simulate_reads(4000, **kw), synth.simulate_reads(4000, genome=None, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.reads, b.reads)) and a.genome.tobytes() == b.genome.tobytes()
    g = np.frombuffer(b"ACGT" * 1000, dtype=np.uint8)
    c = synth.simulate_reads(123, genome=g, error=0.0, **kw)
    assert c.genome.tobytes() == g.tobytes()
    for i, r in enumerate(c.reads):
        span = g[c.start[i]:c.start[i] + c.span[i]]
        assert r.tobytes() == (synth.revcomp(span) if c.strand[i] else span).tobytes()
