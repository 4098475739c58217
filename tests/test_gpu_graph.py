"""GPU suite for the overlap graph (gact_hip_overlap_graph, csrc/gact_graph.hpp): reads, arcs, classes and the statistics' counts
equal the model's (tests/graph_model.py) byte for byte -- on crafted host records of every pattern (no alignment runs), three times
over on two slots, on the device-resident records of a run of both strands with and without the pair selection, its summaries
and the clip of read_coverage, through the arcs_cap protocol and the refusals, and through the driver's --gfa.  No tolerance."""
import os
import re
import subprocess

import numpy as np
import pytest

import graph_model
from graph_model import crafted, graph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("reads", "contained", "by_class", "proposed", "arcs", "transitive", "kept")


@pytest.fixture(scope="module")
def eng():
    """an engine that aligns nothing: two slots, workspaces for one block"""
    from gact_amd import engine
    e = engine.Engine(n_slots=2, max_blocks=1)
    yield e
    e.close()


_MODEL = {}


def _case(pattern):
    """(records, read_lens, kwargs, the model's result), computed once"""
    if pattern not in _MODEL:
        rec, lens, kw = crafted(pattern)
        _MODEL[pattern] = (rec, lens, kw, graph(rec, lens, **kw))
    return _MODEL[pattern]


def _same(got, want, what):
    """got: (reads, arcs, classes) of the device; want: the model's dict"""
    for name, g in zip(("reads", "arcs", "classes"), got):
        w = want[name]
        assert g.dtype == w.dtype and len(g) == len(w), "%s: %d %s, the model has %d" % (what, len(g), name, len(w))
        if g.tobytes() != w.tobytes():
            bad = int(np.flatnonzero(g != w)[0])
            raise AssertionError("%s: %s differ at %d: device %s, model %s" % (what, name, bad, g[bad], w[bad]))


def _same_counts(st, want, what):
    for name in COUNTS:
        assert st[name] == want["counts"][name], "%s: statistics' %s: device %s, model %s" % (what, name, st[name], want["counts"][name])


@pytest.mark.parametrize("pattern", graph_model.PATTERNS)
def test_crafted_host_records_equal_the_model(eng, pattern):
    rec, lens, kw, want = _case(pattern)
    held = [rec, lens] + [np.asarray(kw[k]) for k in ("sel", "sums", "clip") if k in kw]
    before = [a.tobytes() for a in held]
    got = eng.overlap_graph(lens, records=rec, classes=True, **kw)
    _same(got, want, pattern)
    st = eng.last_graph_stats()
    _same_counts(st, want, pattern)
    n_chosen = len(want["classes"])
    assert st["device_ms"] > 0 and st["table_slots"] >= 4 * n_chosen and st["table_slots"] & (st["table_slots"] - 1) == 0
    assert st["scratch_bytes"] >= 4 * st["table_slots"] + 137 * n_chosen + 52 * len(lens)
    # without the classes: the same reads and arcs
    reads, arcs = eng.overlap_graph(lens, records=rec, **kw)
    assert reads.tobytes() == want["reads"].tobytes() and arcs.tobytes() == want["arcs"].tobytes()
    assert before == [a.tobytes() for a in held]


@pytest.mark.parametrize("pattern", ["hub", "many_reads", "random"])
def test_the_result_is_the_same_on_every_run_and_on_every_slot(eng, pattern):
    rec, lens, kw, want = _case(pattern)
    for slot in (0, 0, 1):
        _same(eng.overlap_graph(lens, records=rec, classes=True, slot=slot, **kw), want, (pattern, slot))
    # a small set after a large one on the same scratch, and the large one again
    s_rec, s_lens, s_kw, s_want = _case("tiling")
    _same(eng.overlap_graph(s_lens, records=s_rec, classes=True, **s_kw), s_want, "tiling after " + pattern)
    _same(eng.overlap_graph(lens, records=rec, classes=True, **kw), want, pattern + " again")
    # n < len(records): the first n only
    if pattern == "many_reads":
        _same(eng.overlap_graph(lens, n=3000, records=rec, classes=True, **kw), graph(rec[:3000], lens, **kw), "the first 3000")


def test_arcs_cap_protocol(eng):
    from gact_amd import engine
    import ctypes as C
    rec, lens, kw, want = _case("tiling")
    n_arcs = len(want["arcs"])
    assert n_arcs == 18
    reads = np.zeros(len(lens), dtype=engine.GRAPH_READ_DTYPE)
    classes = np.zeros(len(rec), dtype=np.uint8)
    arcs = np.full(n_arcs, -5, dtype=engine.GRAPH_ARC_DTYPE)

    def call(arcs_ptr, cap):
        count = C.c_int64(-1)
        rc = eng.L.gact_hip_overlap_graph(eng.h, 0, len(rec), rec.ctypes.data, 0, None, None, len(lens), lens.ctypes.data, None, None,
                                          reads.ctypes.data, classes.ctypes.data, arcs_ptr, cap, C.byref(count))
        return rc, count.value

    for arcs_ptr, cap in ((arcs.ctypes.data, n_arcs - 1), (None, 1000), (arcs.ctypes.data, 0)):
        reads[:], classes[:] = 0, 0
        assert call(arcs_ptr, cap) == (-1, n_arcs) and b"room" in eng.L.gact_hip_last_error()
        assert (arcs["u"] == -5).all() and (arcs["flags"] == -5).all()
        assert reads.tobytes() == want["reads"].tobytes() and classes.tobytes() == want["classes"].tobytes()
        _same_counts(eng.last_graph_stats(), want, "a call without room")
    assert call(arcs.ctypes.data, n_arcs) == (0, n_arcs) and arcs.tobytes() == want["arcs"].tobytes()
    # the binding retries once: more arcs than chosen records
    rec, lens, kw, want = _case("both_strands")
    assert len(want["arcs"]) > len(rec)
    _same(eng.overlap_graph(lens, records=rec, classes=True, **kw), want, "both_strands")


@pytest.fixture(scope="module")
def small_run():
    """ecoli10x_small, both strands, run on slot 0; every graph is taken BEFORE the records are fetched"""
    from conftest import workload_block
    from path_cases import engine_with
    blk = workload_block("ecoli10x_small")
    e, n, nf = engine_with(blk.rs, blk.cf, blk.cr, n_slots=2)
    lens = np.array([len(r) for r in blk.rs.reads], dtype=np.int32)
    e.candidates_run_mixed(n, nf)
    run_stats = e.last_run_stats()
    got = {"all": e.overlap_graph(lens, classes=True)}
    sel = e.select_overlaps(mode="pair")
    _, sums = e.candidates_summaries(sel=sel, rc_from=nf)
    got["pair+sums"] = e.overlap_graph(lens, sel=sel, sums=sums, classes=True)
    cover = e.read_coverage(lens, sel=sel, sums=sums, min_depth=3)
    clip = np.stack([cover["span_begin"], cover["span_end"]], axis=1).astype(np.int32)
    got["pair+sums+clip"] = e.overlap_graph(lens, sel=sel, sums=sums, clip=clip, classes=True)
    stats = e.last_graph_stats()
    others = (e.last_summaries_stats(), e.last_select_stats(), e.last_cover_stats())
    records = e.candidates_fetch(n).copy()
    yield dict(eng=e, n=n, nf=nf, lens=lens, got=got, sel=sel, sums=sums, clip=clip, stats=stats, records=records, run_stats=run_stats,
               others=others)
    e.close()


def test_device_records_of_a_run_of_both_strands_equal_the_model(small_run):
    r = small_run
    records, lens, sel, sums, clip = r["records"], r["lens"], r["sel"], r["sums"], r["clip"]
    assert 0 < r["nf"] < r["n"] and 0 < len(sel) < int(records["emitted"].sum()) < r["n"]
    want = {"all": graph(records, lens), "pair+sums": graph(records, lens, sel=sel, sums=sums),
            "pair+sums+clip": graph(records, lens, sel=sel, sums=sums, clip=clip)}
    for name in want:
        _same(r["got"][name], want[name], name)
        print(name, want[name]["counts"])
    _same_counts(r["stats"], want["pair+sums+clip"], "pair+sums+clip")
    # not trivially so: arcs of both kinds, contained reads, and a clip that is not every whole read
    c = want["pair+sums+clip"]["counts"]
    assert c["kept"] > 0 and c["transitive"] > 0 and c["contained"] > 0 and c["by_class"][graph_model.DOVETAIL] > 0
    assert ((clip[:, 0] > 0) | (clip[:, 1] < lens)).any()
    assert want["all"]["arcs"].tobytes() != want["pair+sums"]["arcs"].tobytes() or \
        want["all"]["classes"].tobytes() != want["pair+sums"]["classes"].tobytes()
    # the slot's records, its run statistics and the other calls' statistics are what they were
    e = r["eng"]
    assert e.last_run_stats() == r["run_stats"]
    assert (e.last_summaries_stats(), e.last_select_stats(), e.last_cover_stats()) == r["others"]
    assert e.candidates_fetch(r["n"]).tobytes() == records.tobytes()
    _same(e.overlap_graph(lens, classes=True), want["all"], "all, after the fetch")
    assert e.last_run_stats() == r["run_stats"]
    assert e.select_overlaps(mode="pair").tolist() == sel.tolist()


def test_refusals(small_run):
    import ctypes as C
    from gact_amd import engine
    r = small_run
    e, n = r["eng"], r["n"]
    L = e.L
    rec, lens, kw, want = _case("tiling")
    reads = np.full(len(lens), -5, dtype=engine.GRAPH_READ_DTYPE)
    classes = np.full(len(rec), 99, dtype=np.uint8)
    arcs = np.full(2 * len(rec), -5, dtype=engine.GRAPH_ARC_DTYPE)
    count = C.c_int64()
    whole = np.stack([np.zeros_like(lens), lens], axis=1).astype(np.int32)

    def call(slot=0, n=len(rec), records=rec, n_sel=0, sel=None, n_reads=len(lens), read_lens=lens, clip=None, params=None):
        ptr = lambda a: a.ctypes.data if a is not None else None
        par = engine.GraphParams(**params) if params else None
        return L.gact_hip_overlap_graph(e.h, slot, n, ptr(records), n_sel, ptr(sel), None, n_reads, ptr(read_lens), ptr(clip),
                                        C.byref(par) if par else None, reads.ctypes.data, classes.ctypes.data, arcs.ctypes.data,
                                        len(arcs), C.byref(count))

    def clipped(i, b, end):
        c = whole.copy()
        c[i] = (b, end)
        return c.reshape(-1)

    for bad, word in ((dict(n=-1), b"n = -1"), (dict(n_reads=-1), b"n_reads = -1"),
                      (dict(read_lens=np.array([5000, -1, 5000, 5000, 5000, 5000], dtype=np.int32)), b"negative"),
                      (dict(clip=clipped(2, -1, 5000)), b"clip"), (dict(clip=clipped(2, 3000, 2999)), b"clip"),
                      (dict(clip=clipped(5, 0, 5001)), b"clip"),
                      (dict(params=dict(max_hang=-1)), b"parameter"), (dict(params=dict(int_permille=1001)), b"parameter"),
                      (dict(params=dict(int_permille=-1)), b"parameter"), (dict(params=dict(min_ovlp=-1)), b"parameter"),
                      (dict(params=dict(fuzz=-1)), b"parameter"),
                      (dict(records=None, slot=1), b"no records"), (dict(records=None, n=n + 1), b"beyond"),
                      (dict(sel=np.array([0, len(rec)], dtype=np.int32), n_sel=2), b"sel"),
                      (dict(sel=np.array([-1], dtype=np.int32), n_sel=1), b"sel"),
                      (dict(sel=np.array([0, 1], dtype=np.int32), n_sel=-1), b"n_sel")):
        assert call(**bad) == -1, bad
        assert word in L.gact_hip_last_error(), (bad, L.gact_hip_last_error())
    # a read id outside the reads: ERANGE
    assert call(n_reads=5, read_lens=lens[:5].copy()) == -4 and b"outside" in L.gact_hip_last_error()
    low = rec.copy()
    low["query_id"][1] = -1
    assert call(records=low) == -4
    assert call(slot=2) < 0 and b"slot" in L.gact_hip_last_error()
    assert (reads["n_hits"] == -5).all() and (reads["kept"] == -5).all() and (classes == 99).all() and (arcs["u"] == -5).all()
    # the whole call works after the refusals, with a record that is out of range but not emitted, and a clip of whole reads
    low["emitted"][1] = 0
    assert call(records=low, clip=whole.reshape(-1)) == 0
    _same((reads, arcs[:count.value], classes), graph(low, lens), "a record that does not count is not looked at")
    # n_reads == 0 returns 0 and writes nothing; n == 0 returns 0 with zeros and contained_by -1, records or not
    reads[:], classes[:], arcs[:] = -5, 99, -5
    assert call(n_reads=0, read_lens=None) == 0 and call(n_reads=0) == 0 and count.value == 0
    assert (reads["n_hits"] == -5).all() and (classes == 99).all() and (arcs["u"] == -5).all()
    nothing = np.zeros(len(lens), dtype=engine.GRAPH_READ_DTYPE)
    nothing["contained_by"] = -1
    for kwargs in (dict(n=0), dict(n=0, records=None, slot=1)):
        reads[:] = -5
        assert call(**kwargs) == 0 and count.value == 0 and reads.tobytes() == nothing.tobytes(), kwargs
    assert (classes == 99).all() and (arcs["u"] == -5).all()
    with pytest.raises(engine.GactHipError, match="no overlap graph"):
        fresh = engine.Engine(max_blocks=1)
        try:
            fresh.last_graph_stats()
        finally:
            fresh.close()


def _gfa(path):
    """-> (segments [(name, bases, LN)], links [(u name, +|-, v name, +|-, overlap, L1)])"""
    lines = open(path).read().splitlines()
    assert lines[0] == "H\tVN:Z:1.0"
    seg, links = [], []
    for line in lines[1:]:
        f = line.split("\t")
        if f[0] == "S":
            assert len(f) == 4 and f[3] == "LN:i:%d" % len(f[2]) and not links, line
            seg.append((f[1], f[2]))
        else:
            m = re.fullmatch(r"L\t(\w+)\t([+-])\t(\w+)\t([+-])\t(\d+)M\tL1:i:(\d+)", line)
            assert m, line
            links.append((m.group(1), m.group(2), m.group(3), m.group(4), int(m.group(5)), int(m.group(6))))
    return seg, links


def test_driver_gfa(tmp_path):
    from gact_amd import engine, workload
    from conftest import workload_block
    rs = workload_block("tiny").rs
    rs.write_fasta(str(tmp_path / "reads.fasta"))
    rs.write_fasta(str(tmp_path / "other.fasta"))
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()
    ids = {name: i for i, name in enumerate(rs.names)}
    lens = np.array([len(r) for r in rs.reads], dtype=np.int32)

    def run(name, *extra):
        d = tmp_path / name
        d.mkdir()
        for f in ("reads.fasta", "params.cfg"):
            os.symlink(tmp_path / f, d / f)
        out = subprocess.run([drv, "reads.fasta", "reads.fasta", "2", "--device-dsoft"] + list(extra), capture_output=True, text=True,
                             cwd=d, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        return d, {p.name: p.read_bytes() for p in d.iterdir() if p.name.startswith("darwin.")}

    pat = re.compile(r"ref_id: (\w+), query_id: (\w+), ab: (-?\d+), ae: (-?\d+), bb: (-?\d+), be: (-?\d+), score: (-?\d+), comp: (\d)")

    def expected(d, files, paf, cover):
        """the model on the records of the .out files (with --paf: begins as the .paf lines' spans give them, through sums)"""
        rows = []
        for t in range(2):
            for line in files["darwin.%d.out" % t].decode().splitlines():
                m = pat.fullmatch(line)
                rows.append((ids[m.group(1)], ids[m.group(2)], int(m.group(8))) + tuple(int(m.group(k)) for k in (3, 4, 5, 6, 7)) + (1,))
        rec = graph_model.records_of(rows)
        kw = {}
        if paf:
            # a PAF line's spans are the alignment's: [7], [8] on the target, [2], [3] on the query, forward strand of the read
            at = {}
            for t in range(2):
                for line in files["darwin.%d.paf" % t].decode().splitlines():
                    f = line.split("\t")
                    at.setdefault((ids[f[5]], ids[f[0]], f[4] == "-", int(f[8])), []).append((int(f[7]), int(f[8]), int(f[2]), int(f[3])))
            for k in range(len(rec)):
                key = (int(rec["ref_id"][k]), int(rec["query_id"][k]), bool(rec["comp"][k]), int(rec["ae"][k]))
                spans = at.get(key)
                if spans:
                    tb, te, qb, qe = spans.pop(0)
                    rec["ab"][k] = tb
                    rec["bb"][k] = int(rec["be"][k]) - (qe - qb)
                else:                                        # no alignment: no PAF line, a summary without columns
                    rec["ab"][k], rec["bb"][k] = rec["ae"][k], rec["be"][k]
        if cover:
            tsv = [line.split("\t") for line in files["darwin.cover.tsv"].decode().splitlines()]
            kw["clip"] = np.array([(int(f[6]), int(f[7])) for f in tsv], dtype=np.int32).reshape(-1)
        return graph(rec, lens, **kw), kw.get("clip")

    for name, extra, paf, cover in (("plain", (), False, False), ("full", ("--unique", "pair", "--paf", "--coverage", "3"), True, True)):
        _, without = run(name, *extra)
        d, files = run(name + "_gfa", *(extra + ("--gfa",)))
        assert "darwin.gfa" not in without and sorted(files) == sorted(list(without) + ["darwin.gfa"])
        for f in without:
            assert files[f] == without[f], f
        want, clip = expected(d, files, paf, cover)
        seg, links = _gfa(d / "darwin.gfa")
        want_seg = []
        for i, name_i in enumerate(rs.names):
            b, end = (0, int(lens[i])) if clip is None else (int(clip[2 * i]), int(clip[2 * i + 1]))
            if want["reads"]["contained_by"][i] < 0 and end > b:
                want_seg.append((name_i, rs.reads[i][b:end].tobytes().decode()))
        assert seg == want_seg
        kept = want["arcs"][want["arcs"]["flags"] == 0]
        want_links = [(rs.names[a["u"] >> 1], "+-"[a["u"] & 1], rs.names[a["v"] >> 1], "+-"[a["v"] & 1], int(min(a["ov_u"], a["ov_v"])),
                       int(a["len"])) for a in kept]
        assert links == want_links
        print("%s: %d segments, %d links" % (name, len(seg), len(links)))
        assert len(seg) > 5 and len(links) > 5
    # the refusals, before any device is opened
    for args, word in ((["reads.fasta", "reads.fasta", "1", "--gfa"], "--device-dsoft"),
                       (["reads.fasta", "reads.fasta", "1", "--device-dsoft", "--gfa", "--shard", "0/1"], "--shard"),
                       (["reads.fasta", "other.fasta", "1", "--device-dsoft", "--gfa"], "one input")):
        out = subprocess.run([drv] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60,
                             env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
        assert out.returncode == 1 and "--gfa" in out.stderr and word in out.stderr, (args, out.stdout, out.stderr)
