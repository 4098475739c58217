"""CPU suite for alignment summaries (gact_hip_candidates_summaries, gact_hip_format_paf): the struct layouts as a C
compiler sees them, engine.summarise on hand-written ops and on the model's alignments, the edges the crafted candidates and
the additions of tests/summary_cases.py reach on the model -- the condition that keeps tests/test_gpu_summaries.py from
passing vacuously -- and the exact bytes of the PAF formatter, which needs no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import path_cases
import summary_cases
from path_cases import AFFINE, LINEAR
from path_model import columns_to_ops, gact_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(64, 24), (320, 120)]


def _c_values(tmp_path, body):
    (tmp_path / "s.c").write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\nint main(void) { %s return 0; }\n" % body)
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c")])
    return [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]


def test_gact_path_summary_layout(tmp_path):
    from gact_amd import engine
    names = engine.SUMMARY_DTYPE.names
    assert names == ("n_eq", "n_x", "ins_bases", "del_bases", "eq_runs", "x_runs", "ins_runs", "del_runs")
    got = _c_values(tmp_path, "printf(\"%zu\", sizeof(gact_path_summary)); " +
                    " ".join("printf(\" %%zu\", offsetof(gact_path_summary, %s));" % n for n in names))
    assert got[0] == 32 == engine.SUMMARY_DTYPE.itemsize
    assert got[1:] == [engine.SUMMARY_DTYPE.fields[n][1] for n in names] == list(range(0, 32, 4))


def test_gact_summaries_stats_layout(tmp_path):
    from gact_amd import engine
    S = engine.SummariesStats
    got = _c_values(tmp_path, "printf(\"%zu %zu %zu %zu\\n\", sizeof(gact_summaries_stats), offsetof(gact_summaries_stats, device_ms), "
                              "offsetof(gact_summaries_stats, launches), offsetof(gact_summaries_stats, scratch_bytes));")
    assert got == [ctypes.sizeof(S), S.device_ms.offset, S.launches.offset, S.scratch_bytes.offset] == [16, 0, 4, 8]


def _fields(s):
    return tuple(int(s[f]) for f in s.dtype.names)


def test_summarise_on_hand_written_ops():
    from gact_amd import engine
    E, X, I, D = engine.OP_EQ, engine.OP_X, engine.OP_I, engine.OP_D
    s = engine.summarise(np.zeros(0, np.uint32))
    assert s.dtype == engine.SUMMARY_DTYPE and _fields(s) == (0,) * 8
    assert _fields(engine.summarise([])) == (0,) * 8
    assert _fields(engine.summarise([(700 << 4) | E])) == (700, 0, 0, 0, 1, 0, 0, 0)
    assert _fields(engine.summarise([(3 << 4) | D])) == (0, 0, 0, 3, 0, 0, 0, 1)
    # alternating kinds: 153=1X2I4=3D1=
    ops = columns_to_ops([E] * 153 + [X] + [I, I] + [E] * 4 + [D] * 3 + [E])
    assert _fields(engine.summarise(ops)) == (158, 1, 2, 3, 3, 1, 1, 1)
    # = X = X ..., then I D I D: every column its own op
    ops = columns_to_ops([E, X] * 10 + [I, D] * 4)
    assert _fields(engine.summarise(ops)) == (10, 10, 4, 4, 10, 10, 4, 4)
    # op words need not be merged to be counted: two adjacent words of one kind are two ops (summarise reduces, it does not merge)
    assert _fields(engine.summarise([(2 << 4) | I, (5 << 4) | I])) == (0, 0, 7, 0, 0, 0, 2, 0)
    assert summary_cases.ops_of_cigar("153=1X2I4=3D1=").tolist() == columns_to_ops([E] * 153 + [X] + [I, I] + [E] * 4 + [D] * 3 + [E]).tolist()


def _models(oracle, cr, tile_size, tile_overlap, scoring):
    cands, nf = np.concatenate([cr.cf, cr.cr]), len(cr.cf)
    out = []
    for idx in range(len(cands)):
        ref, query = path_cases.reads_of(cr.rs, cands, nf, idx)
        out.append(gact_path(oracle.align_with_bt, ref, query, int(cands[idx]["ref_pos"]), int(cands[idx]["query_pos"]),
                             tile_size=tile_size, tile_overlap=tile_overlap, scoring=scoring))
    return out


_REACH = {}


def _reach(oracle, scoring, config):
    """-> ({edge: count} of path_cases.crafted(raw=False), the same of summary_cases.additions()), on the model"""
    key = (scoring, config)
    if key not in _REACH:
        from gact_amd import engine
        counts = []
        for models in (_models(oracle, path_cases.crafted(raw=False), *config, scoring),
                       summary_cases.additions_models(oracle, *config, scoring)):
            cnt = dict.fromkeys(summary_cases.EDGES, 0)
            for m in models:
                # the defining rule on the model's own columns
                s = engine.summarise(columns_to_ops(m["cols"]))
                assert sum(int(s[f]) for f in ("eq_runs", "x_runs", "ins_runs", "del_runs")) == len(m["ops"])
                assert sum(int(s[f]) for f in ("n_eq", "n_x", "ins_bases", "del_bases")) == len(m["cols"])
                for k, v in summary_cases.edges(m).items():
                    cnt[k] += v
            counts.append(cnt)
        _REACH[key] = tuple(counts)
    return _REACH[key]


# what the model gives for path_cases.crafted(raw=False), 146 candidates: the affine scoring cuts no gap run and has no
# junction between different ops -- the gap summary_cases.additions() closes
CRAFTED_REACH = {
    (LINEAR, (64, 24)): dict(gap_cut=4, junction_same=64, junction_diff=0, left_empty=32, no_columns=20),
    (LINEAR, (320, 120)): dict(gap_cut=6, junction_same=64, junction_diff=2, left_empty=33, no_columns=16),
    (AFFINE, (64, 24)): dict(gap_cut=0, junction_same=72, junction_diff=0, left_empty=36, no_columns=6),
    (AFFINE, (320, 120)): dict(gap_cut=0, junction_same=72, junction_diff=0, left_empty=36, no_columns=6),
}


@pytest.mark.parametrize("scoring", [LINEAR, AFFINE], ids=["linear", "affine"])
@pytest.mark.parametrize("config", CONFIGS)
def test_edge_reach_of_the_crafted_candidates(oracle, scoring, config):
    """summarise(columns_to_ops(cols)) of every crafted candidate has run sum n_ops and column sum n_columns (in _reach), and
    the crafted set alone reaches what the table says"""
    crafted, _ = _reach(oracle, scoring, config)
    assert len(path_cases.crafted(raw=False).names) == 146
    assert crafted == CRAFTED_REACH[(scoring, config)]


@pytest.mark.parametrize("scoring", [LINEAR, AFFINE], ids=["linear", "affine"])
def test_crafted_plus_additions_reach_every_edge_of_the_counting_walk(oracle, scoring):
    """what tests/test_gpu_summaries.py counts on: at each scoring a gap run that goes on across a tile boundary (at 64/24 or
    320/120), a junction with the same op on both sides, an empty left part with a right part; at the linear scoring a
    junction between different ops; and a candidate without columns"""
    total = dict.fromkeys(summary_cases.EDGES, 0)
    for config in CONFIGS:
        for cnt in _reach(oracle, scoring, config):
            for k, v in cnt.items():
                total[k] += v
    assert total["gap_cut"] >= 1 and total["junction_same"] >= 1 and total["left_empty"] >= 1 and total["no_columns"] >= 1
    if scoring == LINEAR:
        assert total["junction_diff"] >= 1
    # the additions are what cuts a gap run at the affine scoring, at the small tile and at the default one
    for config in CONFIGS:
        assert _reach(oracle, scoring, config)[1]["gap_cut"] >= 1, config


def test_additions_and_the_combined_list():
    ad = summary_cases.additions()
    assert len(ad.cf) == len(ad.cr) == 6 and len(ad.names) == 12 == len(set(ad.names))
    base, deleted, inserted = ad.rs.reads[0], ad.rs.reads[1], ad.rs.reads[4]       # (pair(): ref, query, its reverse complement)
    assert len(base) == 1000 and len(deleted) == 1000 - 18 * 12 and len(inserted) == 1000 + 18 * 12
    assert all(set(bytes(r)) <= set(b"ACGT") for r in ad.rs.reads)
    for raw in (True, False):
        cr, cb = path_cases.crafted(raw), summary_cases.combined(raw)
        n, nf = len(cb.cf) + len(cb.cr), len(cb.cf)
        assert n == len(cr.names) + 12 == len(cb.names) == len(cb.origin) and len(set(cb.names)) == n
        cands = np.concatenate([cb.cf, cb.cr])
        sets = {"crafted": (cr, np.concatenate([cr.cf, cr.cr]), len(cr.cf)), "additions": (ad, np.concatenate([ad.cf, ad.cr]), 6)}
        for k, (where, idx) in enumerate(cb.origin):
            src, src_cands, src_nf = sets[where]
            assert (k >= nf) == (idx >= src_nf)
            a, b = path_cases.reads_of(cb.rs, cands, nf, k), path_cases.reads_of(src.rs, src_cands, src_nf, idx)
            assert bytes(a[0]) == bytes(b[0]) and bytes(a[1]) == bytes(b[1])
            assert (cands[k]["ref_pos"], cands[k]["query_pos"]) == (src_cands[idx]["ref_pos"], src_cands[idx]["query_pos"])


# ---- gact_hip_format_paf: no engine, no device

def _rec(**kw):
    from gact_amd import engine
    r = np.zeros((), dtype=engine.OVERLAP_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r


def _sum(*v):
    from gact_amd import engine
    return np.array(tuple(v), dtype=engine.SUMMARY_DTYPE)


def test_format_paf_forward_record(hip_lib_path):
    from gact_amd import engine
    # 90= 4X, two insertions of 3 + 2 query bases, one deletion of 6 ref bases: target 100 bases, query 99
    rec = _rec(ab=200, ae=300, bb=51, be=150, score=77, comp=0, emitted=1)
    line = engine.format_paf(rec, _sum(90, 4, 5, 6, 7, 4, 2, 1), "read_q", 5000, "read_t", 7000)
    de = 1 - 90 / (90 + 4 + 2 + 1)
    assert line == "read_q\t5000\t51\t150\t+\tread_t\t7000\t200\t300\t90\t105\t255\tAS:i:77\tNM:i:15\tde:f:%.4f\n" % de
    assert line.endswith("de:f:0.0722\n")


def test_format_paf_reverse_complement_record_flips_the_query_span(hip_lib_path):
    from gact_amd import engine
    rec = _rec(ab=0, ae=1000, bb=100, be=1100, score=1000, comp=1, emitted=1)
    line = engine.format_paf(rec, _sum(1000, 0, 0, 0, 1, 0, 0, 0), "q", 1500, "t", 1000)
    # the span [100, 1100) of the reverse-complemented read is [400, 1400) of the read
    assert line == "q\t1500\t400\t1400\t-\tt\t1000\t0\t1000\t1000\t1000\t255\tAS:i:1000\tNM:i:0\tde:f:0.0000\n"


def test_format_paf_path_shorter_than_the_record(hip_lib_path):
    """the left extension aligned nothing: ab / bb stay at the hit while the path starts at the right extension's arg-max"""
    from gact_amd import engine
    rec = _rec(ab=500, ae=800, bb=40, be=341, score=250, comp=0, emitted=1)
    line = engine.format_paf(rec, _sum(280, 5, 10, 3, 4, 3, 1, 1), "q", 400, "t", 900)
    used_t, used_q = 280 + 5 + 3, 280 + 5 + 10
    assert used_t < 800 - 500 and used_q < 341 - 40
    cols = line.split("\t")
    assert (int(cols[7]), int(cols[8])) == (800 - used_t, 800) and int(cols[7]) != 500
    assert (int(cols[2]), int(cols[3])) == (341 - used_q, 341)
    assert line == "q\t400\t46\t341\t+\tt\t900\t512\t800\t280\t298\t255\tAS:i:250\tNM:i:18\tde:f:%.4f\n" % (1 - 280 / 287)
    rec["comp"] = 1
    cols = engine.format_paf(rec, _sum(280, 5, 10, 3, 4, 3, 1, 1), "q", 400, "t", 900).split("\t")
    assert cols[2:5] == [str(400 - 341), str(400 - 46), "-"]


def test_format_paf_refuses_a_summary_without_columns_and_reports_a_small_cap(hip_lib_path):
    from gact_amd import engine
    L = engine.load()
    rec = _rec(ab=200, ae=300, bb=51, be=150, score=77, comp=0, emitted=1)
    with pytest.raises(engine.GactHipError, match="no columns"):
        engine.format_paf(rec, _sum(0, 0, 0, 0, 0, 0, 0, 0), "q", 10, "t", 10)
    # a cap too small: as gact_hip_format_overlap (snprintf): the length the line needs, the buffer cut and terminated
    s = _sum(90, 4, 5, 6, 7, 4, 2, 1)
    whole = engine.format_paf(rec, s, "read_q", 5000, "read_t", 7000)
    buf = ctypes.create_string_buffer(b"\xff" * 16, 16)
    n = L.gact_hip_format_paf(rec.ctypes.data, s.ctypes.data, b"read_q", 5000, b"read_t", 7000, buf, 16)
    assert n == len(whole) and buf.raw == whole.encode()[:15] + b"\0"
    over = ctypes.create_string_buffer(16)
    m = L.gact_hip_format_overlap(rec.ctypes.data, b"read_t", b"read_q", over, 16)
    assert m > 16 and over.raw[15:] == b"\0"
    assert L.gact_hip_format_paf(rec.ctypes.data, s.ctypes.data, b"read_q", 5000, b"read_t", 7000, buf, 0) < 0
    assert L.gact_hip_format_paf(None, s.ctypes.data, b"read_q", 5000, b"read_t", 7000, buf, 16) < 0
