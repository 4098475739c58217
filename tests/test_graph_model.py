"""CPU suite for the overlap graph (gact_hip_overlap_graph): the model of tests/graph_model.py against hand-written classes, arcs
and flags on its small crafted sets, the properties every arc set has (closed under complement with the same record, one arc per
key, ascending by (u, len, v), degrees that add up), what the crafted sets hold -- the condition that keeps
tests/test_gpu_graph.py from passing vacuously -- the rule against simulator truth, the new structs as a C compiler sees them,
the library's exports, and the driver's refusals of --gfa, which touch no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import graph_model
from graph_model import (DOVETAIL, DROPPED, INTERNAL, NONE, QUERY_CONTAINED, SELF, SHORT, TARGET_CONTAINED, crafted, graph)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MODEL = {}


def _model(pattern):
    if pattern not in _MODEL:
        rec, lens, kw = crafted(pattern)
        _MODEL[pattern] = (rec, lens, kw, graph(rec, lens, **kw))
    return _MODEL[pattern]


def _arcs(g, fields=("u", "v", "len", "record", "flags")):
    return [tuple(int(a[f]) for f in fields) for a in g["arcs"]]


def test_tiling_is_a_chain():
    rec, lens, kw, g = _model("tiling")
    assert g["classes"].tolist() == [DOVETAIL] * 18 and (g["reads"]["contained_by"] == -1).all()
    # strands 0 1 1 0 1 0: the walk to the right is 0 -> 3 -> 5 -> 6 -> 9 -> 10, the walk to the left its complement
    kept = [(u, v, ln) for u, v, ln, _, fl in _arcs(g) if fl == 0]
    right = [(0, 3), (3, 5), (5, 6), (6, 9), (9, 10)]
    assert sorted(kept) == sorted([(u, v, 2000) for u, v in right] + [(v ^ 1, u ^ 1, 2000) for u, v in right])
    # the next neighbours (1000 shared, 4000 apart) are explained by the two steps between them, on both strands
    skipped = [(0, 5), (3, 6), (5, 9), (6, 10)]
    assert sorted((u, v, ln) for u, v, ln, _, fl in _arcs(g) if fl) == sorted(
        [(u, v, 4000) for u, v in skipped] + [(v ^ 1, u ^ 1, 4000) for u, v in skipped])
    assert all(fl in (0, 3) for _, _, _, _, fl in _arcs(g))
    assert g["reads"]["n_hits"].tolist() == [4, 6, 8, 8, 6, 4] and g["reads"]["kept"].sum() == 10 and g["reads"]["deg"].sum() == 18
    assert g["counts"] == dict(reads=6, contained=0, by_class=[0, 0, 0, 0, 0, 0, 0, 18], proposed=36, arcs=18, transitive=8, kept=10)


def test_contained_reads_leave_the_graph():
    rec, lens, kw, g = _model("contained")
    # records in (t, q) order: (0,1) (0,2) (0,3) (1,0) (1,2)? -- only pairs that share a base are there
    pairs = list(zip(rec["ref_id"].tolist(), rec["query_id"].tolist()))
    want = {(0, 2): QUERY_CONTAINED, (2, 0): TARGET_CONTAINED, (1, 3): QUERY_CONTAINED, (3, 1): TARGET_CONTAINED}
    assert [int(c) for c in g["classes"]] == [want.get(p, DOVETAIL) for p in pairs]
    assert g["reads"]["contained_by"].tolist() == [-1, -1, pairs.index((0, 2)), pairs.index((1, 3)), -1]
    assert g["reads"]["n_contains"].tolist() == [2, 2, 0, 0, 0]
    # 0 (+) -> 1 (-, so vertex 3) -> 4 (+, vertex 8), and the complements; the contained reads' dovetails propose nothing
    assert [(u, v, ln, fl) for u, v, ln, _, fl in _arcs(g)] == [(0, 3, 5000, 0), (2, 1, 5000, 0), (3, 8, 5000, 0), (9, 2, 5000, 0)]
    assert g["counts"]["proposed"] == 8 and g["counts"]["by_class"][DOVETAIL] == 8


def test_mutual_containment_takes_the_shorter_read_then_the_higher_id():
    rec, lens, kw, g = _model("mutual")
    assert g["classes"].tolist() == [QUERY_CONTAINED, TARGET_CONTAINED, TARGET_CONTAINED, TARGET_CONTAINED, QUERY_CONTAINED]
    assert g["reads"]["contained_by"].tolist() == [-1, 0, 2, -1, -1, 3]
    assert g["reads"]["n_contains"].tolist() == [2, 0, 0, 1, 2, 0] and len(g["arcs"]) == 0


def test_internal_hits_make_no_arc_and_no_containment():
    rec, lens, kw, g = _model("internal")
    assert g["classes"].tolist() == [INTERNAL, INTERNAL, DOVETAIL]
    assert g["reads"]["n_internal"].tolist() == [1, 2, 1] and g["reads"]["n_hits"].tolist() == [2, 2, 2]
    assert [(u, v, ln, fl) for u, v, ln, _, fl in _arcs(g)] == [(0, 4, 3000, 0), (5, 1, 3000, 0)]


def test_every_threshold_at_its_value_and_one_off():
    rec, lens, kw, g = _model("thresholds")
    assert kw == {}
    assert g["classes"].tolist() == [DOVETAIL, DOVETAIL, INTERNAL,          # ext5 = max_hang on either side; max_hang + 1
                                     DOVETAIL, INTERNAL,                    # ext3 = max_hang; max_hang + 1
                                     DOVETAIL, INTERNAL,                    # 1000 sq = 800 (sq + ext); one under
                                     DOVETAIL, SHORT, DOVETAIL, SHORT,      # ov = min_ovlp, min_ovlp - 1 on both sides, on one side
                                     DOVETAIL, DOVETAIL, DOVETAIL, DOVETAIL, DOVETAIL, DOVETAIL]
    by_record = {}
    for u, v, ln, record, fl in _arcs(g):
        by_record.setdefault(record, []).append((u, v, ln, fl))
    # a -> b -> c, 3000 + 3000: equal to 5000 + fuzz, the long arc is flagged on both strands; against 4999 + fuzz it is kept
    assert [fl for _, _, _, fl in by_record[13]] == [3, 3] and [ln for _, _, ln, _ in by_record[13]] == [5000, 5000]
    assert [fl for _, _, _, fl in by_record[16]] == [0, 0] and [ln for _, _, ln, _ in by_record[16]] == [4999, 4999]
    assert all(fl == 0 for r in by_record for _, _, _, fl in by_record[r] if r != 13)
    # ov_u / ov_v of record 9: the query side is one base longer
    a = g["arcs"][g["arcs"]["record"] == 9]
    assert sorted((int(x["ov_u"]), int(x["ov_v"])) for x in a) == [(1000, 1001), (1001, 1000)]


def test_clip_moves_the_frame_and_empties_reads():
    rec, lens, kw, g = _model("clip")
    pairs = list(zip(rec["ref_id"].tolist(), rec["query_id"].tolist()))
    classes = dict(zip(pairs, g["classes"].tolist()))
    # read 6 has an empty clip: every record of it is dropped, it has no hits and no arcs
    assert all(c == DROPPED for p, c in classes.items() if 6 in p) and sum(6 in p for p in pairs) >= 6
    assert list(g["reads"][6].tolist()[:4]) == [0, 0, 0, -1]
    # read 7's clip [0, 1500) ends before its overlaps with reads 4 and 5 begin
    assert classes[(7, 5)] == DROPPED and classes[(5, 7)] == DROPPED
    # read 8, other strand, clip [100, 4100): with the clip mirrored into the record's frame it follows read 5; it contains read 7
    assert classes[(5, 8)] == DOVETAIL and classes[(8, 7)] == QUERY_CONTAINED and classes[(7, 8)] == TARGET_CONTAINED
    # (len is the distance between the clipped heads: read 5's at genome 10000, vertex 17's -- read 8 without the 900 -- at 13900)
    assert (10, 17, 3900) in [(u, v, ln) for u, v, ln, _, _ in _arcs(g)]
    # the six clipped reads still tile, 2000 from head to head as their genome starts are: both reads' ends move with the deeper clip
    assert sorted(ln for u, v, ln, _, fl in _arcs(g) if fl == 0 and max(u, v) < 12) == [2000] * 10
    assert sum(fl == 0 for _, _, _, _, fl in _arcs(g)) == 12 and g["counts"]["by_class"][DROPPED] == 18
    # without the clip nothing is dropped, and the adapter overhangs (300 on every end) stay under max_hang
    assert DROPPED not in graph(rec, lens)["classes"].tolist()


def test_summaries_move_the_begins():
    rec, lens, kw, g = _model("sums")
    t_rec, t_lens, _, tiling = _model("tiling")
    assert np.array_equal(lens, t_lens) and sorted(kw) == ["sel", "sums"] and sorted(kw["sel"].tolist()) == list(range(18))
    # with the summaries: the tiling's chain; the gaps in them move the begins by < 30, the flags stay
    assert [(u, v, fl) for u, v, _, _, fl in _arcs(g)] == [(u, v, fl) for u, v, _, _, fl in _arcs(tiling)]
    assert g["classes"].tolist() == [DOVETAIL] * 18
    # without them ab / bb are in the middle of the overlap: other classes
    assert graph(rec, lens, sel=kw["sel"])["classes"].tolist() != g["classes"].tolist()


def test_duplicates_the_higher_score_then_the_lower_index():
    rec, lens, kw, g = _model("duplicates")
    assert g["classes"].tolist() == [DOVETAIL] * 5 and g["counts"]["proposed"] == 10
    # records 0, 1, 2 share their keys with equal scores: record 0 wins both, with its own len; records 3, 4: the later is better
    assert [(u, v, record) for u, v, _, record, _ in _arcs(g)] == [(0, 3, 0), (2, 1, 0), (3, 4, 4), (5, 2, 4)]
    assert g["arcs"]["len"].tolist() == [3002, 3000, 3000, 3000] and g["arcs"]["score"].tolist() == [500, 500, 450, 450]


def test_both_strands_side_by_side():
    rec, lens, kw, g = _model("both_strands")
    assert [(u, v, ln, record) for u, v, ln, record, _ in _arcs(g)] == [(0, 2, 3000, 0), (0, 3, 3500, 1), (2, 1, 3500, 1), (3, 1, 3000, 0)]
    assert g["reads"]["deg"].tolist() == [[2, 0], [1, 1]] and (g["arcs"]["flags"] == 0).all()


def test_self_not_emitted_sel_disagree_empty():
    rec, lens, kw, g = _model("self")
    assert g["classes"].tolist() == [DOVETAIL, DOVETAIL, SELF, SELF] and g["reads"]["n_hits"].tolist() == [2, 2] and len(g["arcs"]) == 2
    rec, lens, kw, g = _model("not_emitted")
    assert (g["classes"] == NONE).tolist() == (rec["emitted"] == 0).tolist() and 0 < (g["classes"] == NONE).sum() < len(rec)
    rec, lens, kw, g = _model("sel")
    assert len(g["classes"]) == len(kw["sel"]) < len(rec) and sorted(kw["sel"].tolist()) != kw["sel"].tolist()
    assert (g["classes"] == NONE).tolist() == (rec["emitted"][kw["sel"]] == 0).tolist() and (g["classes"] == NONE).any()
    assert set(g["arcs"]["record"].tolist()) <= set(kw["sel"].tolist())
    rec, lens, kw, g = _model("disagree")
    assert g["classes"].tolist() == [QUERY_CONTAINED, QUERY_CONTAINED, DOVETAIL, DOVETAIL]
    assert g["reads"]["contained_by"].tolist() == [1, 0, -1] and len(g["arcs"]) == 0 and g["counts"]["proposed"] == 0
    rec, lens, kw, g = _model("empty")
    assert len(rec) > 100 and not g["classes"].any() and len(g["arcs"]) == 0 and (g["reads"]["contained_by"] == -1).all()
    with pytest.raises(IndexError):
        graph(rec, lens, sel=[0, len(rec)])
    rec, lens, kw, _ = _model("tiling")
    with pytest.raises(ValueError):
        graph(rec, lens[:5])


def test_what_the_large_patterns_hold():
    rec, lens, kw, g = _model("hub")
    assert g["reads"]["deg"][0].tolist() == [65, 0] and g["reads"]["deg"][1].tolist() == [129, 0]
    assert g["reads"]["kept"][0].tolist() == [1, 0] and g["reads"]["kept"][1].tolist() == [1, 0] and g["counts"]["transitive"] > 1000
    for pattern, want in (("blocks257", 257), ("blocks513", 513)):
        rec, lens, kw, g = _model(pattern)
        assert len(rec) == len(g["classes"]) == want and len(set(g["classes"].tolist())) >= 4 and g["counts"]["transitive"] > 0
    rec, lens, kw, g = _model("many_reads")
    assert len(lens) == 1500 > 2 * 256 and g["counts"]["kept"] == 2 * (len(lens) - 1) and g["counts"]["contained"] == 0
    # 128 reads: one chunk of the degree scan, full; 129: two vertices behind it, with arcs of their own
    for pattern, n in (("tiling128", 128), ("tiling129", 129)):
        rec, lens, kw, g = _model(pattern)
        assert len(lens) == n and len(rec) == 4 * n - 6 and g["classes"].tolist() == [DOVETAIL] * len(rec)
        assert g["counts"]["arcs"] == len(rec) and g["counts"]["kept"] == 2 * (n - 1) and g["counts"]["contained"] == 0
        assert g["reads"]["deg"].sum(axis=1).tolist() == [2, 3] + [4] * (n - 4) + [3, 2] and len(set(rec["comp"].tolist())) == 2
    rec, lens, kw, g = _model("random")
    assert len(rec) == 4000 and len(lens) == 300 and sorted(kw) == ["clip", "params"]
    assert all(n > 0 for n in g["counts"]["by_class"][INTERNAL:]) and g["counts"]["by_class"][NONE] > 0
    assert 0 < g["counts"]["contained"] < 300 and g["counts"]["kept"] > 0 and g["counts"]["transitive"] > 0
    assert g["counts"]["arcs"] < g["counts"]["proposed"]
    assert set(g["arcs"]["flags"].tolist()) >= {0, 3}


@pytest.mark.parametrize("pattern", graph_model.PATTERNS)
def test_properties_of_every_arc_set(pattern):
    rec, lens, kw, g = _model(pattern)
    arcs, reads = g["arcs"], g["reads"]
    rows = _arcs(g, ("u", "v", "len", "ov_u", "ov_v", "record", "score", "flags"))
    keys = [(u, v) for u, v, *_ in rows]
    assert len(set(keys)) == len(keys)
    assert [(u, ln, v) for u, v, ln, *_ in rows] == sorted((u, ln, v) for u, v, ln, *_ in rows)
    by_key = {(r[0], r[1]): r for r in rows}
    for u, v, ln, ov_u, ov_v, record, score, flags in rows:
        assert ln >= 1 and u >> 1 != v >> 1 and 0 <= u < 2 * len(lens) and 0 <= v < 2 * len(lens)
        c = by_key[(v ^ 1, u ^ 1)]                                  # closed under complement, with the same record
        assert c[5] == record and c[6] == score == rec["score"][record] and (c[3], c[4]) == (ov_v, ov_u)
        assert c[7] == (flags >> 1 | (flags & 1) << 1)              # bit 1 is the complement's bit 0
        assert reads["contained_by"][u >> 1] == -1 and reads["contained_by"][v >> 1] == -1
    deg = np.bincount(arcs["u"], minlength=2 * len(lens)).reshape(-1, 2) if len(lens) else np.zeros((0, 2))
    kept = np.bincount(arcs["u"][arcs["flags"] == 0], minlength=2 * len(lens)).reshape(-1, 2) if len(lens) else np.zeros((0, 2))
    assert np.array_equal(reads["deg"], deg) and np.array_equal(reads["kept"], kept)
    c = g["counts"]
    assert c["arcs"] == len(rows) == c["kept"] + c["transitive"] and sum(c["by_class"]) == len(g["classes"])
    assert c["contained"] == int((reads["contained_by"] >= 0).sum())
    counted = g["classes"][(g["classes"] != NONE) & (g["classes"] != SELF) & (g["classes"] != DROPPED)]
    assert reads["n_hits"].sum() == 2 * len(counted) and reads["n_internal"].sum() == 2 * int((counted == INTERNAL).sum())
    assert reads["n_contains"].sum() == int(((counted == QUERY_CONTAINED) | (counted == TARGET_CONTAINED)).sum())


@pytest.mark.parametrize("coverage,seed", [(8, 1), (12, 2), (20, 3)])
def test_the_rule_against_simulator_truth(coverage, seed):
    """exact overlaps from the simulator's own coordinates, every ordered pair that shares >= 1000 genome bases; min_ovlp 2000.
    After containment and reduction the kept arcs are the path through the non-contained reads in genome order, both strands"""
    from gact_amd import synth
    rs = synth.simulate_reads(60000, coverage=coverage, seed=seed, mean_len=6000, sd_len=1500, min_len=1500, max_len=12000)
    lens = np.array([len(r) for r in rs.reads], dtype=np.int32)

    def coords(i, lo, hi, flipped):
        """[lo, hi) of the genome on read i in genome orientation, or flipped"""
        g, n = rs.gmap[i], int(lens[i])
        b = int(g[lo - rs.start[i]])
        e = int(g[hi - rs.start[i]]) if hi < rs.start[i] + rs.span[i] else n
        return (n - e, n - b) if flipped else (b, e)

    rows = []
    for t in range(rs.n):
        for q in range(rs.n):
            lo, hi = max(rs.start[t], rs.start[q]), min(rs.start[t] + rs.span[t], rs.start[q] + rs.span[q])
            if t == q or hi - lo < 1000:
                continue
            flipped = bool(rs.strand[t])                 # the record's frame: read t as stored, read q on the matching strand
            ab, ae = coords(t, lo, hi, flipped)
            bb, be = coords(q, lo, hi, flipped)
            rows.append((t, q, int(rs.strand[t] != rs.strand[q]), ab, ae, bb, be, hi - lo, 1))
    g = graph(graph_model.records_of(rows), lens, params=dict(min_ovlp=2000))
    alive = [i for i in np.argsort(rs.start, kind="stable").tolist() if g["reads"]["contained_by"][i] < 0]
    arcs = g["arcs"]
    kept = arcs[arcs["flags"] == 0]
    print("%d reads, %d records, %d not contained, %d arcs, %d kept" % (rs.n, len(rows), len(alive), len(arcs), len(kept)))
    assert g["reads"]["kept"].max() <= 1
    place = {i: k for k, i in enumerate(alive)}
    for a in kept:
        assert abs(place[int(a["u"]) >> 1] - place[int(a["v"]) >> 1]) == 1
    assert len(kept) == 2 * (len(alive) - 1)
    assert set(arcs["flags"].tolist()) <= {0, 3}


def test_the_structs_are_what_a_c_compiler_sees(tmp_path):
    from gact_amd import engine
    arc = ("u", "v", "len", "ov_u", "ov_v", "record", "score", "flags")
    read = ("n_hits", "n_internal", "n_contains", "contained_by", "deg", "kept")
    stats = [n for n, _ in engine.GraphStats._fields_]
    params = [n for n, _ in engine.GraphParams._fields_]
    (tmp_path / "s.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\n"
        "int main(void) { printf(\"%zu %zu %zu %zu\", sizeof(gact_graph_arc), sizeof(gact_graph_read), sizeof(gact_graph_stats), "
        "sizeof(gact_graph_params));\n" +
        "".join("printf(\" %%zu\", offsetof(gact_graph_arc, %s));\n" % f for f in arc) +
        "".join("printf(\" %%zu\", offsetof(gact_graph_read, %s));\n" % f for f in read) +
        "".join("printf(\" %%zu\", offsetof(gact_graph_stats, %s));\n" % f for f in stats) +
        "".join("printf(\" %%zu\", offsetof(gact_graph_params, %s));\n" % f for f in params) +
        "printf(\" %d %d %d %d %d %d %d %d\", GACT_GRAPH_NONE, GACT_GRAPH_SELF, GACT_GRAPH_DROPPED, GACT_GRAPH_INTERNAL, "
        "GACT_GRAPH_QUERY_CONTAINED, GACT_GRAPH_TARGET_CONTAINED, GACT_GRAPH_SHORT, GACT_GRAPH_DOVETAIL);\n"
        "printf(\" %d %d %d %d\", GACT_GRAPH_DEFAULT_MAX_HANG, GACT_GRAPH_DEFAULT_INT_PERMILLE, GACT_GRAPH_DEFAULT_MIN_OVLP, "
        "GACT_GRAPH_DEFAULT_FUZZ);\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    A, R, S, P = engine.GRAPH_ARC_DTYPE, engine.GRAPH_READ_DTYPE, engine.GraphStats, engine.GraphParams
    assert got[:4] == [A.itemsize, R.itemsize, ctypes.sizeof(S), ctypes.sizeof(P)] == [32, 32, 128, 16]
    want = [A.fields[f][1] for f in arc] + [R.fields[f][1] for f in read] + [getattr(S, f).offset for f in stats] + \
        [getattr(P, f).offset for f in params]
    assert got[4:4 + len(want)] == want
    assert got[4 + len(want):] == [NONE, SELF, DROPPED, INTERNAL, QUERY_CONTAINED, TARGET_CONTAINED, SHORT, DOVETAIL] + \
        [graph_model.DEFAULTS[k] for k in ("max_hang", "int_permille", "min_ovlp", "fuzz")]
    d = engine.GraphParams()
    assert {k: getattr(d, k) for k in params} == graph_model.DEFAULTS
    assert [engine.GRAPH_NONE, engine.GRAPH_SELF, engine.GRAPH_DROPPED, engine.GRAPH_INTERNAL, engine.GRAPH_QUERY_CONTAINED,
            engine.GRAPH_TARGET_CONTAINED, engine.GRAPH_SHORT, engine.GRAPH_DOVETAIL] == list(range(8))


def test_the_library_exports_the_entries(hip_lib_path):
    from gact_amd import engine
    lib = ctypes.CDLL(hip_lib_path)
    for name in ("gact_hip_overlap_graph", "gact_hip_last_graph_stats"):
        assert name in engine.EXPORTS
        getattr(lib, name)
    assert hasattr(engine.Engine, "overlap_graph") and hasattr(engine.Engine, "last_graph_stats")


def test_the_driver_refuses_gfa_before_it_opens_a_device(tmp_path):
    from gact_amd import engine
    drv = engine.driver_path()
    for args, word in ((["reads.fasta", "reads.fasta", "1", "--gfa"], "--device-dsoft"),
                       (["reads.fasta", "reads.fasta", "1", "--device-dsoft", "--gfa", "--shard", "0/1"], "--shard"),
                       (["reads.fasta", "other.fasta", "1", "--device-dsoft", "--gfa"], "one input file")):
        out = subprocess.run([drv] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert out.returncode == 1 and "--gfa" in out.stderr and word in out.stderr, (args, out.stdout, out.stderr)
        assert not list(tmp_path.iterdir())
