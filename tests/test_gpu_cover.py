"""GPU suite for the per-read coverage (gact_hip_read_coverage, csrc/gact_cover.hpp): the result equals the model's
(tests/cover_model.py) field by field and the depth position by position -- on crafted host records of every pattern (no
alignment runs), three times over on two slots, on the device-resident records of a run of both strands with and without the
pair selection and its summaries, through the refusals, and through the driver's --coverage.  No tolerance anywhere."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cover_model
from cover_model import BOTH, QUERY, REF, cover, crafted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    """an engine that aligns nothing: two slots, workspaces for one block"""
    from gact_amd import engine
    e = engine.Engine(n_slots=2, max_blocks=1)
    yield e
    e.close()


_MODEL = {}


def _case(pattern, **over):
    """(records, read_lens, kwargs, model cover, model depth), computed once"""
    key = (pattern, tuple(sorted(over.items())))
    if key not in _MODEL:
        rec, lens, kw = crafted(pattern)
        kw = dict(kw, **over)
        _MODEL[key] = (rec, lens, kw) + cover(rec, lens, **kw)
    return _MODEL[key]


def _same(got, want, what):
    for f in want.dtype.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s: %s differs at read %d: device %s, model %s" % (what, f, bad[0], got[bad[0]], want[bad[0]])
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _same_depth(got, want, what):
    assert got.dtype == np.int32 and len(got) == len(want)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%s: depth differs at %d of %d positions, first at %d: device %d, model %d" % (
        what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def _variants(pattern):
    if pattern == "strand":
        return [dict(sides=s) for s in (REF, QUERY, BOTH)]
    if pattern == "random":
        return [dict(min_depth=d) for d in (1, 3, 1000)]
    return [{}]


@pytest.mark.parametrize("pattern", cover_model.PATTERNS)
def test_crafted_host_records_equal_the_model(eng, pattern):
    for over in _variants(pattern):
        rec, lens, kw, want, want_depth = _case(pattern, **over)
        before = [a.tobytes() for a in (rec, lens)] + [kw[k].tobytes() for k in ("sel", "sums") if k in kw]
        got, depth = eng.read_coverage(lens, records=rec, depth=True, **kw)
        _same(got, want, (pattern, over))
        _same_depth(depth, want_depth, (pattern, over))
        st = eng.last_cover_stats()
        assert st["reads"] == len(lens) and st["intervals"] == int(want["n_intervals"].sum())
        assert st["positions"] == int(lens.astype(np.int64).sum()) and st["device_ms"] > 0
        assert st["scratch_bytes"] >= 4 * (st["positions"] + st["reads"]) + 40 * st["reads"] > 0
        # without the per-base output: the same table
        _same(eng.read_coverage(lens, records=rec, **kw), want, (pattern, over, "no depth"))
        assert before == [a.tobytes() for a in (rec, lens)] + [kw[k].tobytes() for k in ("sel", "sums") if k in kw]


@pytest.mark.parametrize("pattern", ["stack", "many_reads", "random"])
def test_the_result_is_the_same_on_every_run_and_on_every_slot(eng, pattern):
    rec, lens, kw, want, want_depth = _case(pattern)
    runs = [eng.read_coverage(lens, records=rec, depth=True, slot=slot, **kw) for slot in (0, 0, 1)]
    for got, depth in runs:
        assert got.tobytes() == want.tobytes() and depth.tobytes() == want_depth.tobytes()
    # a small set after a large one on the same scratch, and the large one again
    s_rec, s_lens, s_kw, s_want, s_depth = _case("chunk_edges")
    got, depth = eng.read_coverage(s_lens, records=s_rec, depth=True, **s_kw)
    assert got.tobytes() == s_want.tobytes() and depth.tobytes() == s_depth.tobytes()
    got, depth = eng.read_coverage(lens, records=rec, depth=True, **kw)
    assert got.tobytes() == want.tobytes() and depth.tobytes() == want_depth.tobytes()
    # n < len(records): the first n only
    if pattern == "random":
        got = eng.read_coverage(lens, n=1000, records=rec, **kw)
        _same(got, cover(rec[:1000], lens, **kw)[0], "the first 1000")


@pytest.fixture(scope="module")
def small_run():
    """ecoli10x_small, both strands, run on slot 0; every coverage is taken BEFORE the records are fetched"""
    from conftest import workload_block
    from path_cases import engine_with
    blk = workload_block("ecoli10x_small")
    e, n, nf = engine_with(blk.rs, blk.cf, blk.cr, n_slots=2)
    lens = np.array([len(r) for r in blk.rs.reads], dtype=np.int32)
    e.candidates_run_mixed(n, nf)
    run_stats = e.last_run_stats()
    got = {"all": e.read_coverage(lens, depth=True)}
    sel = e.select_overlaps(mode="pair")
    got["pair"] = e.read_coverage(lens, sel=sel, depth=True)
    _, sums = e.candidates_summaries(sel=sel, rc_from=nf)
    got["pair+sums"] = e.read_coverage(lens, sel=sel, sums=sums, depth=True)
    stats = e.last_cover_stats()
    records = e.candidates_fetch(n).copy()
    yield dict(eng=e, n=n, nf=nf, lens=lens, got=got, sel=sel, sums=sums, stats=stats, records=records, run_stats=run_stats)
    e.close()


def test_device_records_of_a_run_of_both_strands_equal_the_model(small_run):
    r = small_run
    records, lens, sel, sums = r["records"], r["lens"], r["sel"], r["sums"]
    assert 0 < r["nf"] < r["n"] and (records["comp"][:r["nf"]] == 0).all() and (records["comp"][r["nf"]:] == 1).all()
    assert 0 < len(sel) < int(records["emitted"].sum()) < r["n"]
    want = {"all": cover(records, lens), "pair": cover(records, lens, sel=sel), "pair+sums": cover(records, lens, sel=sel, sums=sums)}
    for name in want:
        _same(r["got"][name][0], want[name][0], name)
        _same_depth(r["got"][name][1], want[name][1], name)
    # not trivially so: every read has a span at min_depth 3, and some reads' spans are not the whole read
    table = want["all"][0]
    with_span = int((table["span_end"] > table["span_begin"]).sum())
    partial = int(((table["span_begin"] > 0) | (table["span_end"] < lens)).sum())
    print("reads %d, with a span %d, span not the whole read %d; intervals %d (all) %d (pair)" % (
        len(lens), with_span, partial, table["n_intervals"].sum(), want["pair"][0]["n_intervals"].sum()))
    assert with_span == len(lens) == 232 and 0 < partial < len(lens)
    assert want["pair"][0]["n_intervals"].sum() < table["n_intervals"].sum()
    moved = int((want["pair+sums"][0] != want["pair"][0]).sum())
    print("reads whose table the summaries change: %d" % moved)
    assert moved > 0                                       # some left extension aligned nothing: the summaries are looked at
    assert r["stats"]["intervals"] == int(want["pair+sums"][0]["n_intervals"].sum()) and r["stats"]["reads"] == len(lens)
    # an explicit n: the first n records only; the ref side alone
    e = r["eng"]
    _same(e.read_coverage(lens, n=r["nf"], sides="ref", min_depth=2), cover(records[:r["nf"]], lens, sides=REF, min_depth=2)[0], "n = nf")


def test_what_a_coverage_leaves_on_its_slot(small_run):
    r = small_run
    e, n, nf, lens = r["eng"], r["n"], r["nf"], r["lens"]
    some = np.arange(0, n, 9, dtype=np.int32)
    e.candidates_paths(sel=some, rc_from=nf)
    e.candidates_summaries(sel=some, rc_from=nf)
    e.select_overlaps(mode="exact")
    before = (e.last_paths_stats(), e.last_summaries_stats(), e.last_select_stats())
    got, depth = e.read_coverage(lens, depth=True)
    assert got.tobytes() == r["got"]["all"][0].tobytes() and depth.tobytes() == r["got"]["all"][1].tobytes()
    mine = e.last_cover_stats()
    # host records on the same slot leave the slot's own records alone; the other slot's call leaves this one's figures
    rec, c_lens, kw, want, _ = _case("clip")
    _same(e.read_coverage(c_lens, records=rec, **kw), want, "clip on the run's slot")
    assert e.last_cover_stats()["reads"] == 3 != mine["reads"]
    mine = e.last_cover_stats()
    _same(e.read_coverage(c_lens, records=rec, slot=1, **kw), want, "clip on slot 1")
    assert e.last_cover_stats() == mine
    assert e.candidates_fetch(n).tobytes() == r["records"].tobytes()
    assert e.last_run_stats() == r["run_stats"]            # (times included: a run's times are read once and kept)
    assert (e.last_paths_stats(), e.last_summaries_stats(), e.last_select_stats()) == before
    assert e.select_overlaps(mode="pair").tolist() == r["sel"].tolist()


def test_refusals(small_run):
    from gact_amd import engine
    r = small_run
    e, n = r["eng"], r["n"]
    L = e.L
    rec, lens, kw, want, want_depth = _case("clip")
    cov = np.full(len(lens), -5, dtype=engine.COVER_DTYPE)
    depth = np.full(int(lens.sum()), -5, dtype=np.int32)
    sel = np.array([0, 1, 2], dtype=np.int32)

    def call(slot=0, n=len(rec), records=rec, n_sel=0, sel=None, sides=BOTH, min_depth=1, n_reads=len(lens), read_lens=lens):
        ptr = lambda a: a.ctypes.data if a is not None else None
        return L.gact_hip_read_coverage(e.h, slot, n, ptr(records), n_sel, ptr(sel), None, sides, min_depth, n_reads, ptr(read_lens),
                                        cov.ctypes.data, depth.ctypes.data)

    for bad, word in ((dict(min_depth=0), b"min_depth"), (dict(min_depth=-3), b"min_depth"), (dict(sides=0), b"sides"),
                      (dict(sides=4), b"sides"), (dict(n=-1), b"n = -1"), (dict(n_reads=-1), b"n_reads = -1"),
                      (dict(read_lens=np.array([100, -1, 50], dtype=np.int32)), b"negative"),
                      (dict(records=None, slot=1), b"no records"), (dict(records=None, n=n + 1), b"beyond"),
                      (dict(sel=np.array([0, len(rec)], dtype=np.int32), n_sel=2), b"sel"),
                      (dict(sel=np.array([-1], dtype=np.int32), n_sel=1), b"sel"), (dict(sel=sel, n_sel=-1), b"n_sel")):
        assert call(**bad) == -1, bad
        assert word in L.gact_hip_last_error(), (bad, L.gact_hip_last_error())
    # a read id outside the reads on a requested side: ERANGE; on the side that is not requested it does not matter
    two = lens[:2].copy()
    assert call(n_reads=2, read_lens=two) == -4 and b"outside" in L.gact_hip_last_error()
    assert call(n_reads=2, read_lens=two, sides=QUERY) == -4
    low = rec.copy()
    low["ref_id"][1] = -1
    assert call(records=low) == -4
    assert call(slot=2) < 0 and b"slot" in L.gact_hip_last_error()
    assert (cov["n_intervals"] == -5).all() and (cov["depth_sum"] == -5).all() and (depth == -5).all()
    with pytest.raises(engine.GactHipError, match="sides"):
        e.read_coverage(lens, records=rec, sides="neither")
    assert call(n_reads=2, read_lens=two, sides=REF) == 0
    assert cov["n_intervals"].tolist() == [5, 0, -5] and (depth[200:] == -5).all() and (depth[:200] >= 0).all()
    # the whole call works after the refusals, with a record that is out of range but not emitted
    low["emitted"][1] = 0
    assert call(records=low) == 0
    _same(cov, cover(low, lens, **kw)[0], "a record that does not count is not looked at")
    # n_reads == 0 returns 0 and writes nothing; n == 0 returns 0 with every cover zero, records or not, fresh slot or not
    cov[:], depth[:] = -5, -5
    assert call(n_reads=0, read_lens=None) == 0 and call(n_reads=0) == 0
    assert (cov["n_intervals"] == -5).all() and (depth == -5).all()
    assert call(n=0) == 0 and cov.tobytes() == bytes(32 * len(lens)) and not depth.any()
    cov[:], depth[:] = -5, -5
    assert call(n=0, records=None, slot=1) == 0 and cov.tobytes() == bytes(32 * len(lens)) and not depth.any()
    # a read of length 0 gets all zeros
    got = e.read_coverage(np.array([100, 0, 50], dtype=np.int32), records=rec[:3], min_depth=1, sides="ref")
    assert got[1].tobytes() == bytes(32) and got[0]["n_intervals"] == 2
    with pytest.raises(engine.GactHipError, match="no coverage"):
        fresh = engine.Engine(max_blocks=1)
        try:
            fresh.last_cover_stats()
        finally:
            fresh.close()


def _tsv(path):
    out = []
    for line in open(path).read().splitlines():
        f = line.split("\t")
        assert len(f) == 9 and re.fullmatch(r"\d+\.\d{3}", f[8]), line
        out.append((f[0],) + tuple(int(v) for v in f[1:8]) + (f[8],))
    return out


def test_driver_coverage(tmp_path):
    from gact_amd import engine, workload
    from conftest import workload_block
    rs = workload_block("tiny").rs
    rs.write_fasta(str(tmp_path / "reads.fasta"))
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()
    ids = {name: i for i, name in enumerate(rs.names)}
    lens = np.array([len(r) for r in rs.reads], dtype=np.int32)
    assert len(ids) == len(lens) == 60

    def run(name, *extra):
        d = tmp_path / name
        d.mkdir()
        os.symlink(tmp_path / "reads.fasta", d / "reads.fasta")
        os.symlink(tmp_path / "params.cfg", d / "params.cfg")
        out = subprocess.run([drv, "reads.fasta", "reads.fasta", "2", "--device-dsoft"] + list(extra), capture_output=True, text=True,
                             cwd=d, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        files = {p.name: p.read_bytes() for p in d.iterdir() if p.name.startswith("darwin.")}
        return d, files

    def expected(files, paf):
        rows = []
        if paf:
            # columns 3, 4 and 8, 9 of a PAF line: the spans on the read and on the reference, forward strand, half-open
            for t in range(2):
                for line in files["darwin.%d.paf" % t].decode().splitlines():
                    f = line.split("\t")
                    rows.append((ids[f[5]], ids[f[0]], 0, int(f[7]), int(f[8]), int(f[2]), int(f[3]), 1))
        else:
            pat = re.compile(r"ref_id: (\w+), query_id: (\w+), ab: (-?\d+), ae: (-?\d+), bb: (-?\d+), be: (-?\d+), score: -?\d+, comp: (\d)")
            for t in range(2):
                for line in files["darwin.%d.out" % t].decode().splitlines():
                    m = pat.fullmatch(line)
                    rows.append((ids[m.group(1)], ids[m.group(2)], int(m.group(7))) + tuple(int(m.group(k)) for k in (3, 4, 5, 6)) + (1,))
        assert len(rows) > 10
        table = cover(cover_model.records_of(rows), lens, sides=BOTH, min_depth=3)[0]
        return [(name, int(lens[i]), int(c["n_intervals"]), int(c["max_depth"]), int(c["covered"]), int(c["well_covered"]),
                 int(c["span_begin"]), int(c["span_end"]), "%.3f" % (int(c["depth_sum"]) / int(lens[i])))
                for i, (name, c) in enumerate(zip(rs.names, table))]

    for name, extra, paf in (("plain", (), False), ("pair", ("--unique", "pair"), False), ("paf", ("--unique", "pair", "--paf"), True)):
        _, without = run(name, *extra)
        d, files = run(name + "_cover", *(extra + ("--coverage", "3")))
        assert "darwin.cover.tsv" not in without and sorted(files) == sorted(list(without) + ["darwin.cover.tsv"])
        for f in without:
            assert files[f] == without[f], f
        got, want = _tsv(d / "darwin.cover.tsv"), expected(files, paf)
        assert [g[:8] for g in got] == [w[:8] for w in want]
        assert [g[8] for g in got] == [w[8] for w in want]
        print("%s: %d reads, %d with a span" % (name, len(got), sum(g[7] > g[6] for g in got)))
        assert sum(g[7] > g[6] for g in got) > 30
