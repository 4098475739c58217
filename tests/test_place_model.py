"""CPU suite for the placement of reads (gact_hip_place_reads, gact_hip_format_sam): the model of tests/place_model.py held to
a second formulation (sorted(key=...) and an all-pairs mask matrix) on every crafted case and to hand-written expectations on
the small ones -- the condition that keeps tests/test_gpu_place.py from comparing the device with a wrong model -- the struct
layouts as a C compiler sees them, and the exact bytes of the SAM formatter, which needs no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cover_model
import place_model
from place_model import CASES, EXTRA, NONE, PRIMARY, SECONDARY, SUPPLEMENTARY, crafted, place

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def place_again(records, read_lens, read_first=0, sel=None, sums=None, mask_permille=500, mapq_cap=60):
    """the rule once more: the order by sorted(key=...), the masks of all pairs of a read at once, the walk over that matrix"""
    from gact_amd import engine
    chosen = np.arange(len(records)) if sel is None else np.asarray(sel, dtype=np.int64)
    mine = records[chosen]
    shifted = mine.copy()
    shifted["query_id"] = shifted["query_id"] - read_first
    emitted = mine["emitted"].astype(bool)
    # (cover_model's list is in chosen order with the empty intervals dropped: matched up again by walking both)
    inside = shifted[emitted]
    ivs = cover_model.intervals(inside, read_lens, None, None if sums is None else sums[emitted], cover_model.QUERY)
    b, e = np.zeros(len(chosen), dtype=np.int64), np.zeros(len(chosen), dtype=np.int64)
    at, nxt = np.flatnonzero(emitted), 0
    lens = np.asarray(read_lens, dtype=np.int64)
    for k in at:
        r = shifted[k]
        lo, hi = int(r["bb"]), int(r["be"])
        if sums is not None:
            lo = hi - int(sums[k]["n_eq"]) - int(sums[k]["n_x"]) - int(sums[k]["ins_bases"])
        if r["comp"]:
            lo, hi = int(lens[r["query_id"]]) - hi, int(lens[r["query_id"]]) - lo
        lo, hi = max(lo, 0), min(hi, int(lens[r["query_id"]]))
        if lo < hi:
            assert ivs[nxt] == (int(r["query_id"]), lo, hi)
            b[k], e[k], nxt = lo, hi, nxt + 1
    assert nxt == len(ivs)
    counted = b < e
    score = mine["score"].astype(np.int64)
    span = (mine["ae"].astype(np.int64) - mine["ab"]) + (mine["be"].astype(np.int64) - mine["bb"])
    out = np.zeros(len(chosen), dtype=engine.PLACE_DTYPE)
    out["parent"] = out["rank"] = -1
    reads = np.zeros(len(lens), dtype=engine.READ_PLACE_DTYPE)
    reads["primary"] = -1
    groups = {}
    for k in np.flatnonzero(counted).tolist():
        groups.setdefault(int(shifted["query_id"][k]), []).append(k)
    for read, members in groups.items():
        ks = sorted(members, key=lambda k: (-score[k], -span[k], k))
        bb, ee = b[ks], e[ks]
        ov = np.minimum(ee[:, None], ee[None, :]) - np.maximum(bb[:, None], bb[None, :])
        masks = (ov > 0) & (1000 * ov >= mask_permille * np.minimum((ee - bb)[:, None], (ee - bb)[None, :]))
        parents, kinds = [], []
        for t in range(len(ks)):
            by = [p for p in parents if masks[p, t]]
            if by:
                kinds.append((SECONDARY, by[0]))
            elif len(parents) < 64:
                kinds.append((SUPPLEMENTARY if parents else PRIMARY, t))
                parents.append(t)
            else:
                kinds.append((EXTRA, t))
        for t, (kind, parent) in enumerate(kinds):
            mapq = 0
            if kind in (PRIMARY, SUPPLEMENTARY):
                s1 = int(score[ks[t]])
                children = [int(score[ks[c]]) for c, (kc, pc) in enumerate(kinds) if kc == SECONDARY and pc == t]
                s2 = min(max(children + [0]), max(s1, 0))
                mapq = 0 if s1 <= 0 else mapq_cap * (s1 - s2) // s1
                if kind == PRIMARY:
                    n_of = lambda what: sum(1 for kc, _ in kinds if kc == what)
                    reads[read] = (len(ks), ks[t], n_of(SUPPLEMENTARY), n_of(SECONDARY), n_of(EXTRA), s1, s2, mapq)
            out[ks[t]] = (kind, mapq, ks[parent], t)
    return out, reads


@pytest.mark.parametrize("pattern", list(dict.fromkeys(p for p, _ in CASES)))
def test_the_model_agrees_with_a_second_formulation(pattern):
    for m in [m for p, m in CASES if p == pattern]:
        c = crafted(pattern, m)
        rec, lens = c.pop("records"), c.pop("read_lens")
        got, want = place(rec, lens, **c), place_again(rec, lens, **c)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), (pattern, m)


def _rows(rows, lens, **kw):
    out, reads = place(place_model.records_of(rows), np.array(lens, dtype=np.int32), **kw)
    return [tuple(int(v) for v in r) for r in out], [tuple(int(v) for v in r) for r in reads]


def test_hand_written_expectations():
    #        ref query comp ab  ae   bb   be  score emitted
    rows = [(0, 0, 0, 0, 100, 0, 100, 50, 1),          # 0: [0, 100) lies inside record 1's interval: its secondary, last in rank
            (1, 0, 0, 0, 200, 0, 200, 90, 1),          # 1: the primary
            (2, 0, 0, 0, 100, 250, 350, 70, 1),        # 2: disjoint: the supplementary, rank 1
            (3, 0, 1, 0, 100, 0, 100, 60, 1),          # 3: comp on a read of 400: [300, 400), overlaps 2 by 50 of 100: its secondary
            (4, 0, 0, 0, 100, 0, 100, 99, 0),          # 4: not emitted
            (5, 0, 0, 0, 100, 400, 500, 99, 1)]        # 5: wholly outside the read
    out, reads = _rows(rows, [400])
    assert out == [(SECONDARY, 0, 1, 3), (PRIMARY, 60 * (90 - 50) // 90, 1, 0), (SUPPLEMENTARY, 60 * (70 - 60) // 70, 2, 1),
                   (SECONDARY, 0, 2, 2), (NONE, 0, -1, -1), (NONE, 0, -1, -1)]
    assert reads == [(4, 1, 1, 2, 0, 90, 50, 26)]
    # one base shorter at that end and record 3 stands alone
    rows[3] = (3, 0, 1, 0, 100, 0, 99, 60, 1)          # [301, 400): 49 of 99, and 49000 < 49500
    out, reads = _rows(rows, [400])
    assert out[3] == (SUPPLEMENTARY, 60, 3, 2) and reads == [(4, 1, 2, 1, 0, 90, 50, 26)]
    # the shorter interval decides: one base of two is half of it, and not all of it
    rows[3] = (3, 0, 1, 0, 100, 49, 149, 60, 1)        # [251, 351)
    rows[2] = (2, 0, 0, 0, 100, 250, 252, 70, 1)       # [250, 252): one base of it under record 3
    out, _ = _rows(rows, [400], mask_permille=1000)
    assert out[3][0] == SUPPLEMENTARY
    out, _ = _rows(rows, [400], mask_permille=500)
    assert out[3] == (SECONDARY, 0, 2, 2)
    # abutting intervals never mask, whatever the threshold
    out, reads = _rows([(0, 0, 0, 0, 50, 0, 50, 9, 1), (1, 0, 0, 0, 50, 50, 100, 8, 1)], [100], mask_permille=0)
    assert out == [(PRIMARY, 60, 0, 0), (SUPPLEMENTARY, 60, 1, 1)] and reads == [(2, 0, 1, 0, 0, 9, 0, 60)]
    # ties: the lower k first; a sel that turns the records round turns the answer round, and a repeated index is two records
    rows = [(0, 0, 0, 0, 50, 0, 50, 7, 1), (1, 0, 0, 0, 50, 0, 50, 7, 1)]
    assert _rows(rows, [60])[0] == [(PRIMARY, 0, 0, 0), (SECONDARY, 0, 0, 1)]
    assert _rows(rows, [60], sel=[1, 0])[0] == [(PRIMARY, 0, 0, 0), (SECONDARY, 0, 0, 1)]
    assert _rows(rows, [60], sel=[1, 1, 0])[0] == [(PRIMARY, 0, 0, 0), (SECONDARY, 0, 0, 1), (SECONDARY, 0, 0, 2)]
    # the larger span goes first among equal scores
    rows = [(0, 0, 0, 0, 50, 0, 50, 7, 1), (1, 0, 0, 0, 51, 0, 50, 7, 1)]
    assert _rows(rows, [60])[0] == [(SECONDARY, 0, 1, 1), (PRIMARY, 0, 1, 0)]
    # a window: read_first moves the ids, and an emitted record outside it is refused, a sel index outside the records too
    rows = [(0, 7, 0, 0, 50, 0, 50, 7, 1), (1, 8, 0, 0, 50, 0, 50, 3, 1)]
    out, reads = _rows(rows, [60, 60], read_first=7)
    assert out == [(PRIMARY, 60, 0, 0), (PRIMARY, 60, 1, 0)] and [r[1] for r in reads] == [0, 1]
    with pytest.raises(ValueError):
        _rows(rows, [60], read_first=7)
    with pytest.raises(ValueError):
        _rows(rows, [60], read_first=8)
    with pytest.raises(IndexError):
        _rows(rows, [60, 60], read_first=7, sel=[0, 2])
    # the summary moves the begin: 30 query-consuming columns end at be
    sums = np.zeros(1, dtype=place_model.engine.SUMMARY_DTYPE)
    sums[0]["n_eq"], sums[0]["n_x"], sums[0]["ins_bases"], sums[0]["del_bases"] = 20, 4, 6, 9
    rows = [(0, 0, 0, 0, 50, 0, 50, 7, 1), (1, 0, 0, 0, 40, 0, 25, 9, 1)]
    assert _rows(rows, [60], sel=[0], sums=sums)[1] == [(1, 0, 0, 0, 0, 7, 0, 60)]
    iv = place_model.query_intervals(place_model.records_of(rows), [60], sel=[0], sums=sums)
    assert iv == {0: (0, 20, 50)}
    # an empty call
    out, reads = _rows([], [5, 6])
    assert out == [] and reads == [(0, -1, 0, 0, 0, 0, 0, 0)] * 2


def test_the_crafted_cases_reach_what_they_are_made_for():
    def of(pattern, m=None):
        c = crafted(pattern, m)
        rec, lens = c.pop("records"), c.pop("read_lens")
        return place(rec, lens, **c) + (rec, c)
    for m, extras in ((64, 0), (65, 1), (66, 2), (1000, 936)):
        out, reads, _, _ = of("chain", m)
        assert reads[0]["n_extra"] == extras and reads[0]["n_supplementary"] == 63 and (out["kind"] != SECONDARY).all()
        assert reads[0]["mapq"] == 60
    out, reads, rec, _ = of("stack", 129)
    assert reads[0]["n_secondary"] == 128 and reads[0]["score"] == rec["score"].max() and reads[1]["primary"] == -1
    assert reads[0]["second"] == np.sort(rec["score"])[-2]
    out, reads, rec, kw = of("ties_repeat", 65)
    assert len(set(kw["sel"].tolist())) < len(kw["sel"]) and len(out) == 68 and (out["kind"] != NONE).all()
    assert sorted(out["rank"].tolist()) == list(range(68)) and (np.diff(np.argsort(out["rank"])) > 0).all()      # the order is k's
    out, reads, _, kw = of("ties_perm", 65)
    assert (out["rank"] == np.arange(65)).all() and sorted(kw["sel"].tolist()) == list(range(65)) and kw["sel"].tolist() != list(range(65))
    for permille in place_model.PERMILLES:
        out, reads, rec, _ = of("threshold", permille)
        kinds = out["kind"].reshape(-1, 2)
        assert (kinds[:, 0] == PRIMARY).all() and set(kinds[:, 1].tolist()) == {SUPPLEMENTARY, SECONDARY}
    out, reads, _, _ = of("abut")
    assert (out["kind"] != SECONDARY).all() and reads["n_supplementary"].tolist() == [1, 2]
    out, reads, rec, _ = of("strand", 63)
    assert (rec["comp"] == 1).all() and [int(v) & 1 for v in crafted("strand", 63)["read_lens"][:2]] == [1, 0]
    out, reads, rec, _ = of("clip", 127)
    assert (out["kind"] == NONE).any() and (out["kind"] != NONE).any() and (rec["bb"] < 0).any() and (rec["be"] > 300).any()
    out, reads, rec, _ = of("not_emitted", 128)
    assert ((out["kind"] == NONE) == (rec["emitted"] == 0)).sum() > len(rec) // 2 and (rec["query_id"][rec["emitted"] == 0] == 99).any()
    out, reads, rec, kw = of("sums", 64)
    assert (out["kind"][len(kw["sel"]) // 2] == NONE) and rec["emitted"][kw["sel"][len(kw["sel"]) // 2]] == 1
    out, reads, _, _ = of("late_mask")
    assert out[64].tolist() == (SECONDARY, 0, 63, 64) and out[65].tolist() == (EXTRA, 0, 65, 65) and out[66].tolist() == (EXTRA, 0, 66, 66)
    assert out[63]["mapq"] == 60 * (4937 - 300) // 4937
    for cap in place_model.CAPS:
        out, reads, _, _ = of("mapq", cap)
        big = 2 ** 31 - 1
        assert reads["mapq"].tolist() == [0, 0, 0, cap, cap * (big - 1) // big, 0, cap * 300 // 1000, cap]
        assert reads["second"].tolist() == [0, 0, 40, 0, 1, big - 1, 700, 0] and out[15]["mapq"] == cap * 60 // 80
    out, reads, _, _ = of("one_read")
    assert reads[0]["n_records"] == 4097 and reads[0]["n_extra"] > 0 and reads[0]["n_supplementary"] == 63
    out, reads, _, _ = of("many_reads")
    assert len(reads) == 70001 and sorted(set(reads["n_records"].tolist())) == [0, 1, 2, 3]


def test_struct_layouts(tmp_path):
    from gact_amd import engine
    place_names, read_names = engine.PLACE_DTYPE.names, engine.READ_PLACE_DTYPE.names
    stat_names = [n for n, _ in engine.PlaceStats._fields_]
    (tmp_path / "abi.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\nint main(void) { "
        "printf(\"%zu %zu %zu %zu\", sizeof(gact_placement), sizeof(gact_read_place), sizeof(gact_place_params), sizeof(gact_place_stats)); "
        + " ".join('printf(" %%zu", offsetof(gact_placement, %s));' % n for n in place_names)
        + " ".join('printf(" %%zu", offsetof(gact_read_place, %s));' % n for n in read_names)
        + " ".join('printf(" %%zu", offsetof(gact_place_stats, %s));' % n for n in stat_names)
        + ' printf(" %d %d %d %d %d %d %d %d", GACT_PLACE_NONE, GACT_PLACE_PRIMARY, GACT_PLACE_SUPPLEMENTARY, GACT_PLACE_SECONDARY, '
          "GACT_PLACE_EXTRA, GACT_PLACE_MAX_PARENTS, GACT_PLACE_DEFAULT_MASK_PERMILLE, GACT_PLACE_DEFAULT_MAPQ_CAP); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "abi")]).split()]
    want = [16, 32, ctypes.sizeof(engine.PlaceParams), ctypes.sizeof(engine.PlaceStats)]
    want += [engine.PLACE_DTYPE.fields[n][1] for n in place_names] + [engine.READ_PLACE_DTYPE.fields[n][1] for n in read_names]
    want += [getattr(engine.PlaceStats, n).offset for n in stat_names]
    want += [engine.PLACE_NONE, engine.PLACE_PRIMARY, engine.PLACE_SUPPLEMENTARY, engine.PLACE_SECONDARY, engine.PLACE_EXTRA,
             engine.PLACE_MAX_PARENTS, engine.PLACE_DEFAULT_MASK_PERMILLE, engine.PLACE_DEFAULT_MAPQ_CAP]
    assert got == want and engine.PLACE_DTYPE.itemsize == 16 and engine.READ_PLACE_DTYPE.itemsize == 32
    assert (place_model.NONE, place_model.PRIMARY, place_model.SUPPLEMENTARY, place_model.SECONDARY, place_model.EXTRA,
            place_model.MAX_PARENTS) == (0, 1, 2, 3, 4, 64)


# ---- gact_hip_format_sam: no engine, no device

def _rec(**kw):
    from gact_amd import engine
    r = np.zeros((), dtype=engine.OVERLAP_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r


def _placed(kind, mapq=0, parent=0, rank=0):
    from gact_amd import engine
    p = np.zeros((), dtype=engine.PLACE_DTYPE)
    p["kind"], p["mapq"], p["parent"], p["rank"] = kind, mapq, parent, rank
    return p


def _ops(text):
    from gact_amd import engine
    code = {"I": engine.OP_I, "D": engine.OP_D, "=": engine.OP_EQ, "X": engine.OP_X}
    import re
    return np.array([int(n) << 4 | code[op] for n, op in re.findall(r"(\d+)([=XID])", text)], dtype=np.uint32)


READ = "ACGTTgcaNNACGTACGTAC"          # 20 bases
READ_RC = "GTACGTACGTNNtgcAACGT"


def test_format_sam_forward_and_reverse_primary(hip_lib_path):
    from gact_amd import engine
    # 6= 1X 2I 3D 4=: 14 ref columns, 13 query columns, NM 6; the alignment is [3, 16) of the read and ends at ref 114
    rec = _rec(ab=100, ae=114, bb=3, be=16, score=7, comp=0, emitted=1)
    line = engine.format_sam(rec, _ops("6=1X2I3D4="), _placed(PRIMARY, 37), "q1", READ, "ref_a")
    assert line == "q1\t0\tref_a\t101\t37\t3S6=1X2I3D4=4S\t*\t0\t0\t" + READ + "\t*\tAS:i:7\tNM:i:6\n"
    rec["comp"] = 1
    line = engine.format_sam(rec, _ops("6=1X2I3D4="), _placed(PRIMARY, 37), "q1", READ, "ref_a")
    assert line == "q1\t16\tref_a\t101\t37\t3S6=1X2I3D4=4S\t*\t0\t0\t" + READ_RC + "\t*\tAS:i:7\tNM:i:6\n"
    # lower case is kept, and the complement of what is no base is N
    rec = _rec(ab=0, ae=8, bb=0, be=8, score=8, comp=1, emitted=1)
    assert engine.format_sam(rec, _ops("8="), _placed(PRIMARY), "q", "acgtRyN-", "r").split("\t")[9] == "NNNNacgt"


def test_format_sam_supplementary_secondary_and_extra(hip_lib_path):
    from gact_amd import engine
    rec = _rec(ab=100, ae=114, bb=3, be=16, score=-7, comp=1, emitted=1)
    line = engine.format_sam(rec, _ops("6=1X2I3D4="), _placed(SUPPLEMENTARY, 60), "q1", READ, "ref_a")
    assert line == "q1\t2064\tref_a\t101\t60\t3H6=1X2I3D4=4H\t*\t0\t0\t" + READ_RC[3:16] + "\t*\tAS:i:-7\tNM:i:6\n"
    rec["comp"] = 0
    line = engine.format_sam(rec, _ops("6=1X2I3D4="), _placed(SUPPLEMENTARY, 60), "q1", READ, "ref_a")
    assert line.split("\t")[1] == "2048" and line.split("\t")[9] == READ[3:16]
    for kind in (SECONDARY, EXTRA):
        line = engine.format_sam(rec, _ops("6=1X2I3D4="), _placed(kind), "q1", READ, "ref_a")
        assert line == "q1\t256\tref_a\t101\t0\t3H6=1X2I3D4=4H\t*\t0\t0\t*\t*\tAS:i:-7\tNM:i:6\n"
    rec["comp"] = 1
    assert engine.format_sam(rec, _ops("13="), _placed(SECONDARY), "q1", READ, "ref_a").split("\t")[1] == "272"


def test_format_sam_omits_clips_of_length_zero(hip_lib_path):
    from gact_amd import engine
    rec = _rec(ab=0, ae=20, bb=0, be=20, score=20, comp=0, emitted=1)
    assert engine.format_sam(rec, _ops("20="), _placed(PRIMARY, 60), "q", READ, "r").split("\t")[3:6] == ["1", "60", "20="]
    rec["be"] = 18
    assert engine.format_sam(rec, _ops("18="), _placed(PRIMARY, 60), "q", READ, "r").split("\t")[5] == "18=2S"
    rec["be"] = 20
    assert engine.format_sam(rec, _ops("18="), _placed(SUPPLEMENTARY, 60), "q", READ, "r").split("\t")[5] == "2H18="


def test_format_sam_ops_shorter_than_the_record(hip_lib_path):
    """the left extension aligned nothing: ab / bb stay at the hit, and POS, the clip and NM come from the ops"""
    from gact_amd import engine
    rec = _rec(ab=500, ae=800, bb=2, be=19, score=9, comp=0, emitted=1)
    f = engine.format_sam(rec, _ops("5=2D1X3I4="), _placed(PRIMARY, 1), "q", READ, "r").split("\t")
    # 12 ref columns end at 800: POS 789; 13 query columns end at 19: a clip of 6, not of bb = 2
    assert f[3] == "789" and f[5] == "6S5=2D1X3I4=1S" and f[12] == "NM:i:6\n"


def test_format_sam_small_cap_refusals_and_the_unmapped_line(hip_lib_path):
    from gact_amd import engine
    L = engine.load()
    rec = _rec(ab=100, ae=114, bb=3, be=16, score=7, comp=0, emitted=1)
    ops, p = _ops("6=1X2I3D4="), _placed(PRIMARY, 37)
    seq = np.frombuffer(READ.encode(), dtype=np.uint8)
    want = engine.format_sam(rec, ops, p, "q1", READ, "ref_a")
    call = lambda buf, cap, n_ops=len(ops), pl=p: L.gact_hip_format_sam(rec.ctypes.data, ops.ctypes.data, n_ops, pl.ctypes.data, b"q1",
                                                                        seq.ctypes.data, len(seq), b"ref_a", buf, cap)
    # a cap too small: the length comes back, as from snprintf, and with that much room and one more the line does
    small = ctypes.create_string_buffer(b"#" * 16, 16)
    assert call(small, 16) == len(want) and call(None, 0) == len(want) and call(small, 0) == len(want)
    exact = ctypes.create_string_buffer(len(want))
    assert call(exact, len(want)) == len(want)
    room = ctypes.create_string_buffer(len(want) + 1)
    assert call(room, len(want) + 1) == len(want) and room.raw[:len(want)].decode() == want and room.raw[len(want)] == 0
    # refusals
    assert call(room, len(want) + 1, n_ops=0) == -1 and b"no ops" in L.gact_hip_last_error()
    assert call(room, len(want) + 1, pl=_placed(NONE)) == -1 and b"kind" in L.gact_hip_last_error()
    assert call(room, len(want) + 1, pl=_placed(5)) == -1
    with pytest.raises(engine.GactHipError, match="outside the read"):
        engine.format_sam(rec, _ops("17="), p, "q1", READ, "ref_a")               # begins in front of the read
    rec["be"] = 21
    with pytest.raises(engine.GactHipError, match="outside the read"):
        engine.format_sam(rec, ops, p, "q1", READ, "ref_a")                        # ends behind it
    with pytest.raises(engine.GactHipError, match="none of"):
        engine.format_sam(_rec(ae=5, be=5), np.array([5 << 4 | 3], dtype=np.uint32), p, "q1", READ, "ref_a")
    # a long read: the binding asks again with the room the first call named
    long_read = "ACGT" * 3000
    rec = _rec(ab=0, ae=12000, bb=0, be=12000, score=12000, comp=0, emitted=1)
    assert engine.format_sam(rec, _ops("12000="), p, "q", long_read, "r").split("\t")[9] == long_read
    # the unmapped line
    assert engine.format_sam_unmapped("q9", READ) == "q9\t4\t*\t0\t0\t*\t*\t0\t0\t" + READ + "\t*\n"
    assert engine.format_sam_unmapped("q9", long_read) == "q9\t4\t*\t0\t0\t*\t*\t0\t0\t" + long_read + "\t*\n"
    assert L.gact_hip_format_sam_unmapped(b"q9", seq.ctypes.data, len(seq), small, 16) == len("q9\t4\t*\t0\t0\t*\t*\t0\t0\t" + READ + "\t*\n")
