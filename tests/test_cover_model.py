"""CPU suite for the per-read coverage (gact_hip_read_coverage): the model of tests/cover_model.py against a per-position
count, what its crafted sets hold -- the condition that keeps tests/test_gpu_cover.py from passing vacuously -- the new structs
as a C compiler sees them, the library's exports, and the driver's refusals of --coverage, which touch no device."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import cover_model
from cover_model import BOTH, QUERY, REF, cover, crafted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MODEL = {}


def _model(pattern, **over):
    key = (pattern, tuple(sorted(over.items())))
    if key not in _MODEL:
        rec, lens, kw = crafted(pattern)
        _MODEL[key] = cover(rec, lens, **dict(kw, **over))
    return _MODEL[key]


def test_the_model_agrees_with_a_count_per_position():
    rec, lens, kw = crafted("random")
    got, depth = _model("random")
    assert kw == {} and len(rec) == 5000 and len(lens) == 300 and lens.max() > 15000
    assert rec["comp"].any() and not rec["comp"].all()
    start = np.concatenate(([0], np.cumsum(lens.astype(np.int64))))
    count = np.zeros(int(start[-1]), dtype=np.int64)
    n_iv = np.zeros(len(lens), dtype=np.int64)
    for r in rec.tolist():
        ref_id, query_id, ab, ae, bb, be, _, comp = r[:8]
        if comp:
            bb, be = int(lens[query_id]) - be, int(lens[query_id]) - bb
        for read, b, e in ((ref_id, ab, ae), (query_id, bb, be)):
            b, e = max(b, 0), min(e, int(lens[read]))
            if e > b:
                count[start[read] + b:start[read] + e] += 1
                n_iv[read] += 1
    assert np.array_equal(depth, count) and depth.dtype == np.int32
    assert np.array_equal(got["n_intervals"], n_iv)
    for i in range(len(lens)):
        d = count[start[i]:start[i + 1]].tolist()
        runs, at = [], 0
        for deep, group in itertools.groupby(d, key=lambda v: v >= 3):
            size = len(list(group))
            if deep:
                runs.append((-size, at))
            at += size
        span = (min(runs)[1], min(runs)[1] - min(runs)[0]) if runs else (0, 0)
        assert (got[i]["span_begin"], got[i]["span_end"]) == span
        assert got[i]["max_depth"] == max(d) and got[i]["depth_sum"] == sum(d)
        assert got[i]["covered"] == sum(v >= 1 for v in d) and got[i]["well_covered"] == sum(v >= 3 for v in d)


@pytest.mark.parametrize("pattern", cover_model.PATTERNS)
def test_crafted_sets_are_seeded_and_consistent(pattern):
    rec, lens, kw = crafted(pattern)
    again = crafted(pattern)
    assert rec.tobytes() == again[0].tobytes() and lens.tobytes() == again[1].tobytes() and lens.dtype == np.int32
    got, depth = _model(pattern)
    assert len(got) == len(lens) and len(depth) == int(lens.astype(np.int64).sum())
    assert (got["covered"] >= got["well_covered"]).all() and (got["span_end"] - got["span_begin"] <= got["well_covered"]).all()
    assert (got["covered"] <= lens).all() and (got["depth_sum"] >= got["covered"]).all()
    assert int(got["depth_sum"].sum()) == int(depth.astype(np.int64).sum())


def test_what_the_crafted_sets_hold():
    """each pattern is what its name says"""
    # lengths
    got, depth = _model("lengths")
    lens = crafted("lengths")[1]
    assert tuple(lens.tolist()) == cover_model.LENGTHS
    assert got["n_intervals"].tolist() == [0] + [9] * (len(lens) - 1)
    assert got["span_begin"].tolist() == [0] * len(lens) and got["span_end"].tolist() == lens.tolist()
    assert got["max_depth"].tolist() == [0, 9, 6] + [6] * (len(lens) - 3)
    assert got["depth_sum"].tolist() == [0, 9, 12] + [3 * int(n) + 6 for n in lens[3:]]
    # chunk_edges
    got, depth = _model("chunk_edges")
    assert cover_model.CHUNK_RUNS == ((0, 63), (64, 128), (129, 130), (191, 321), (900, 1000))
    assert (got[0]["span_begin"], got[0]["span_end"]) == (191, 321)
    assert got[0]["well_covered"] == 63 + 64 + 1 + 130 + 100 and got[0]["covered"] == 1000 and got[0]["max_depth"] == 4
    assert depth[63] == depth[128] == depth[130] == depth[190] == depth[899] == 1 and depth[999] == 4
    assert got[1]["n_intervals"] == 0
    # ties: the leftmost of three equal runs, then the last one, a base longer
    got, _ = _model("ties")
    assert (got[0]["span_begin"], got[0]["span_end"]) == (10, 110) and (got[1]["span_begin"], got[1]["span_end"]) == (500, 601)
    assert got[0]["well_covered"] == 300 and got[1]["well_covered"] == 301
    # abut: no dip and no spike where one interval ends and the next begins
    got, depth = _model("abut")
    assert (depth == 3).all() and got["span_end"].tolist() == [500, 500, 64] and got["n_intervals"].tolist() == [6, 6, 6]
    # clip: exactly the intervals that should be dropped are
    rec, lens, kw = crafted("clip")
    got, depth = _model("clip")
    assert kw["sides"] == BOTH and (rec["ab"] < 0).any() and (rec["ae"] > 100).any() and (rec["ab"] > rec["ae"]).any()
    assert got["n_intervals"].tolist() == [5, 3, 2] and 2 * int(rec["emitted"].sum()) - 4 == 10
    assert got["covered"].tolist() == [40 + 40, 10 + 10 + 1, 30 + 5]
    assert depth[200 + 20] == 1 and depth[200 + 19] == 0 and depth[200 + 49] == 1 and depth[200 + 4] == 1 and depth[200 + 5] == 0
    # strand: both sides are the sum of each side, and the strand moves the query intervals
    rec, lens, kw = crafted("strand")
    assert int(rec["comp"].sum()) == len(rec) // 2
    d1, d2, d3 = (_model("strand", sides=s)[1] for s in (REF, QUERY, BOTH))
    assert np.array_equal(d1.astype(np.int64) + d2, d3) and d1.any() and d2.any()
    forward = rec.copy()
    forward["comp"] = 0
    assert not np.array_equal(cover(forward, lens, sides=QUERY)[1], d2)
    assert np.array_equal(cover(forward, lens, sides=REF)[1], d1)
    # stack
    got, depth = _model("stack")
    assert got[0]["max_depth"] == 70001 and got[0]["depth_sum"] == 70001 * 40000 > 2 ** 31 and got[0]["n_intervals"] == 70001
    assert (got[0]["span_begin"], got[0]["span_end"]) == (0, 40000)
    # many_reads
    got, _ = _model("many_reads")
    lens = crafted("many_reads")[1]
    assert len(got) == 70001 > 2 ** 16 and lens.max() == 130 and lens.min() == 1
    assert (got["n_intervals"] == 0).sum() > 100 and (got["span_end"] > 0).sum() > 1000
    assert (got["n_intervals"][2 ** 16:] > 0).any() and got["max_depth"].max() > 5
    # not_emitted
    rec, lens, kw = crafted("not_emitted")
    sel = crafted("not_emitted_sel")[2]["sel"]
    assert rec.tobytes() == crafted("not_emitted_sel")[0].tobytes() and "sel" not in kw
    assert rec["emitted"].sum() == 100 and 0 < rec["emitted"][sel].sum() < len(sel)
    everything = rec.copy()
    everything["emitted"] = 1
    plain, chosen = _model("not_emitted")[0], _model("not_emitted_sel")[0]
    assert plain["n_intervals"].sum() < cover(everything, lens, min_depth=2)[0]["n_intervals"].sum()
    assert 0 < chosen["n_intervals"].sum() < plain["n_intervals"].sum()
    assert chosen["n_intervals"].sum() < cover(everything, lens, sel=sel, min_depth=2)[0]["n_intervals"].sum()
    # sums: the begins move; the summary goes with the position in sel and not with the record's index
    rec, lens, kw = crafted("sums")
    got, depth = _model("sums")
    sel, sums = kw["sel"], kw["sums"]
    assert (np.diff(sel) < 0).any() and not np.array_equal(depth, cover(rec, lens, sel=sel, min_depth=2)[1])
    assert not np.array_equal(depth, cover(rec, lens, sel=np.sort(sel), sums=sums, min_depth=2)[1])
    assert not any(sums[7][f] for f in sums.dtype.names) and rec["emitted"][sel[7]]
    without = cover(rec, lens, sel=np.delete(sel, 7), sums=np.delete(sums, 7), min_depth=2)
    assert np.array_equal(without[1], depth) and without[0].tobytes() == got.tobytes()
    # random: a span on most reads at 1 and 3, none anywhere at 1,000
    for min_depth, some in ((1, True), (3, True), (1000, False)):
        got, _ = _model("random", min_depth=min_depth)
        assert (got["span_end"] > 0).any() == some and (got["well_covered"] > 0).any() == some
    got = _model("random")[0]
    assert ((got["span_end"] - got["span_begin"]) < got["well_covered"]).any()          # more than one run somewhere
    # empty
    rec, lens, _ = crafted("empty")
    got, depth = _model("empty")
    assert len(rec) == 100 and not rec["emitted"].any() and not depth.any() and got.tobytes() == bytes(32 * len(lens))


def test_refusals_of_the_model():
    rec, lens, _ = crafted("clip")
    with pytest.raises(IndexError):
        cover(rec, lens, sel=[0, len(rec)])
    with pytest.raises(ValueError):
        cover(rec, lens[:2])
    assert cover(rec, lens[:2], sides=REF)[0]["n_intervals"].tolist() == [5, 0]      # (only the requested side is looked at)


def test_gact_read_cover_and_stats_layout(tmp_path):
    from gact_amd import engine
    S, D = engine.CoverStats, engine.COVER_DTYPE
    cover_fields = ("n_intervals", "max_depth", "covered", "well_covered", "span_begin", "span_end", "depth_sum")
    stats_fields = ("device_ms", "reads", "intervals", "positions", "scratch_bytes")
    (tmp_path / "s.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\n"
        "int main(void) { printf(\"%zu %zu\", sizeof(gact_read_cover), sizeof(gact_cover_stats));\n" +
        "".join("printf(\" %%zu\", offsetof(gact_read_cover, %s));\n" % f for f in cover_fields) +
        "".join("printf(\" %%zu\", offsetof(gact_cover_stats, %s));\n" % f for f in stats_fields) +
        "printf(\" %d %d %d\\n\", GACT_COVER_REF, GACT_COVER_QUERY, GACT_COVER_BOTH); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got[:2] == [D.itemsize, ctypes.sizeof(S)] == [32, 32]
    assert got[2:9] == [D.fields[f][1] for f in cover_fields] == [0, 4, 8, 12, 16, 20, 24]
    assert D.names == cover_fields and D["depth_sum"] == np.dtype("<i8") and all(D[f] == np.dtype("<i4") for f in cover_fields[:6])
    assert got[9:14] == [getattr(S, f).offset for f in stats_fields] == [0, 4, 8, 16, 24]
    assert [f for f, _ in S._fields_] == list(stats_fields)
    assert got[14:] == [engine.COVER_REF, engine.COVER_QUERY, engine.COVER_BOTH] == [1, 2, 3] == [REF, QUERY, BOTH]


def test_the_library_exports_the_coverage(hip_lib_path):
    from gact_amd import engine
    lib = ctypes.CDLL(hip_lib_path)
    for name in ("gact_hip_read_coverage", "gact_hip_last_cover_stats"):
        assert name in engine.EXPORTS
        getattr(lib, name)
    assert hasattr(engine.Engine, "read_coverage") and hasattr(engine.Engine, "last_cover_stats")


@pytest.mark.parametrize("args", [["--coverage", "3"], ["--device-dsoft", "--coverage", "3", "--shard", "0/2"],
                                  ["--device-dsoft", "--coverage"], ["--device-dsoft", "--coverage", "0"],
                                  ["--device-dsoft", "--coverage", "3x"], ["--device-dsoft", "--coverage", "-2"],
                                  ["--device-dsoft", "--coverage", "2.5"]],
                         ids=["without-device-dsoft", "with-shard", "no-value", "zero", "not-a-number", "negative", "fraction"])
def test_the_driver_refuses_coverage_where_it_cannot_hold(tmp_path, args):
    """before any file is read and any device is opened: the FASTA files named here do not exist"""
    from gact_amd import engine
    out = subprocess.run([engine.driver_path(), "none.fasta", "none.fasta", "1"] + args, capture_output=True, text=True, cwd=tmp_path,
                         timeout=600)
    assert out.returncode not in (0, -6, -11) and out.returncode > 0, out.stdout + out.stderr
    assert "--coverage" in out.stderr and "cannot open" not in out.stderr and "unknown option" not in out.stderr
    assert not list(tmp_path.iterdir())
