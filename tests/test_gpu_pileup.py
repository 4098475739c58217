"""GPU suite for the per-base pileup and consensus (gact_hip_pileup_begin / _add / _finish): counts, consensus bytes and the
per-read table equal tests/pileup_model.py's -- fed with the chain model's CIGARs on the crafted candidates of
tests/path_cases.py, with the path run's own ops at both tile geometries and both scorings -- and the depth equals
gact_hip_read_coverage's; one selection added in five ways gives the same bytes; windows, what a slot keeps, the figures of
all six passes behind one run on one slot, the refusals, and the driver's --pileup.  Exact equality everywhere: integers and bytes are equal or the test fails."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import path_cases
from path_cases import engine_with, expected, ops_of
from pileup_model import DEL, DEPTH, INS, pileup

pytestmark = pytest.mark.gpu


class _Rc:
    """rc[i]: read i's reverse complement, made when asked for"""

    def __init__(self, rs):
        self.rs, self.made = rs, {}

    def __getitem__(self, i):
        if i not in self.made:
            self.made[i] = self.rs.rc(i)
        return self.made[i]


def _model(rs, records, paths, ops, window=None, min_depth=1):
    window = (0, len(rs.reads)) if window is None else window
    return pileup(rs.reads, _Rc(rs), records, [ops_of(paths, ops, k) for k in range(len(records))], window, min_depth)


def _same(got, want, what=""):
    """got: Engine.pileup_finish's (reads, counts, consensus); want: the model's (counts, consensus, table)"""
    reads, counts, cons = got
    assert counts.shape == want[0].shape and cons.shape == want[1].shape and reads.shape == want[2].shape, what
    if not np.array_equal(counts, want[0]):
        p, k = [int(v[0]) for v in np.nonzero(counts != want[0])]
        raise AssertionError("%s: counts differ first at position %d kind %d: %s, model %s" % (what, p, k, counts[p], want[0][p]))
    assert cons.tobytes() == want[1].tobytes(), (what, int(np.flatnonzero(cons != want[1])[0]))
    assert reads.tobytes() == want[2].tobytes(), (what, [(i, reads[i], want[2][i]) for i in np.flatnonzero(reads != want[2])[:3]])


def _equal(a, b):
    """two pileup_finish results, byte for byte"""
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("raw", [True, False], ids=["raw-bytes", "acgt"])
def test_crafted_candidates_equal_the_model_fed_with_the_chain_models_cigars(oracle, raw):
    from gact_amd import engine
    cr = path_cases.crafted(raw)
    cands = np.concatenate([cr.cf, cr.cr])
    eng, n, nf = engine_with(cr.rs, cr.cf, cr.cr)
    eng.candidates_run_mixed(n, nf)
    normal = eng.candidates_fetch(n).copy()
    eng.pileup_begin()
    eng.pileup_add(n=n, rc_from=nf)
    got = {d: eng.pileup_finish(min_depth=d) for d in (1, 2)}
    st = eng.last_pileup_stats()
    eng.close()
    exp = expected(oracle, cr.rs, cands, nf)
    records = np.zeros(n, dtype=engine.OVERLAP_DTYPE)
    for k, e in enumerate(exp):
        same_read = cands[k]["ref_id"] == cands[k]["query_id"]
        records[k] = (cands[k]["ref_id"], cands[k]["query_id"], e["ab"], e["ae"], e["bb"], e["be"], e["score"], int(k >= nf),
                      int(not same_read and e["score"] > 0), e["first_tile_score"], e["n_tiles"], 0, 0)      # (emitted: gact.cpp:213)
    assert np.array_equal(records["emitted"], normal["emitted"]) and np.array_equal(records["ae"], normal["ae"])
    cigars = [e["cigar"] for e in exp]
    want = {d: pileup(cr.rs.reads, _Rc(cr.rs), records, cigars, (0, len(cr.rs.reads)), d) for d in (1, 2)}
    # what the families are there for shows in the model's own output
    counts = want[1][0]
    start = np.concatenate([[0], np.cumsum([len(r) for r in cr.rs.reads])])
    seen = set()
    for k, name in enumerate(cr.names):
        family = name.split("/")[0]
        if not records["emitted"][k] or not cigars[k] or family not in ("gaps", "inside", "edge"):
            continue
        mine = counts[start[cands[k]["ref_id"]]:start[cands[k]["ref_id"] + 1]]
        assert (mine[:, DEPTH] > 0).any(), name
        if family == "gaps":
            assert mine[:, DEL].sum() > 0 and mine[:, INS].sum() > 0, name
            seen.add(family)
        elif (mine[:, DEPTH] == 0).any():                              # (a short read inside a long one: the long one as the target)
            seen.add(family)
    assert seen == {"gaps", "inside", "edge"}
    assert (counts[:, DEPTH] >= 2).any() and (want[2][1] != want[1][1]).any()
    if raw:
        assert counts[:, 4].sum() > 0                                  # N against N: OTHER
    for d in (1, 2):
        _same(got[d], want[d], "min_depth %d" % d)
    assert np.array_equal(got[1][1], got[2][1])
    with_columns = [k for k in range(n) if records["emitted"][k] and cigars[k]]
    assert st["alignments"] == len(with_columns) == int(want[1][2]["n_alignments"].sum()) and st["adds"] == 1
    assert st["columns"] == sum(exp[k]["n_columns"] for k in with_columns) and st["positions"] == len(counts) and st["device_ms"] > 0


_SMALL = {}


def _small(want=150):
    """a sample of both strands of ecoli10x_small, in a shuffled order"""
    from conftest import workload_block
    if want not in _SMALL:
        blk = workload_block("ecoli10x_small")
        nf = len(blk.cf)
        sel = path_cases.sample(nf, len(blk.cr), want, seed=20261018)
        assert (sel < nf).sum() >= want // 4 and (sel >= nf).sum() >= want // 4 and np.any(np.diff(sel) < 0)
        _SMALL[want] = (blk, nf, sel)
    return _SMALL[want]


@pytest.mark.parametrize("scoring", [(1, -1, -1, -1), (2, -3, -5, -2)])
@pytest.mark.parametrize("tile_size,tile_overlap", [(320, 120), (512, 192), (64, 24)])
def test_both_tile_geometries_and_scorings_equal_the_model_and_the_coverage_depth(scoring, tile_size, tile_overlap):
    blk, nf, sel = _small(60)
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, tile_size=tile_size, tile_overlap=tile_overlap, scoring=scoring)
    records, paths, ops = eng.candidates_paths(sel=sel, rc_from=nf)
    eng.pileup_begin()
    eng.pileup_add(sel=sel, rc_from=nf)
    got = eng.pileup_finish(min_depth=2)
    rec2, sums = eng.candidates_summaries(sel=sel, rc_from=nf)
    lens = np.array([len(r) for r in blk.rs.reads], dtype=np.int32)
    _, depth = eng.read_coverage(lens, records=rec2, sums=sums, sides="ref", min_depth=2, depth=True)
    eng.close()
    assert rec2.tobytes() == records.tobytes()
    want = _model(blk.rs, records, paths, ops, min_depth=2)
    assert (records["emitted"] == 1).sum() > len(sel) // 2 and want[0][:, DEL].sum() > 0 and want[0][:, INS].sum() > 0
    _same(got, want)
    assert np.array_equal(got[1][:, DEPTH], depth.astype(np.uint32))


_REFERENCE = {}


def _reference():
    """the 150-candidate sample on the default engine: the path run's (records, paths, ops), the pileup of one add at
    min_depth 3, its statistics, and the model's answer -- made once, left unchanged"""
    if not _REFERENCE:
        blk, nf, sel = _small()
        eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
        path = eng.candidates_paths(sel=sel, rc_from=nf)
        eng.pileup_begin()
        eng.pileup_add(sel=sel, rc_from=nf)
        one = eng.pileup_finish()
        st = eng.last_pileup_stats()
        eng.close()
        want = _model(blk.rs, *path, min_depth=3)
        _same(one, want, "one add")
        _REFERENCE.update(path=path, one=one, stats=st, model=want)
    return _REFERENCE


def test_one_selection_added_in_five_ways_gives_the_same_bytes(monkeypatch):
    blk, nf, sel = _small()
    ref = _reference()
    one, st_one = ref["one"], ref["stats"]
    assert st_one["adds"] == 1 and st_one["chunks"] == 1 and st_one["alignments"] == int(one[0]["n_alignments"].sum()) > 50
    thirds = np.array_split(sel, 3)
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, slots=(0, 1), n_slots=2)
    eng.pileup_begin()
    for part in thirds:
        eng.pileup_add(sel=part, rc_from=nf)
    _equal(eng.pileup_finish(), one)
    assert eng.last_pileup_stats()["adds"] == 3
    eng.pileup_begin()
    for k, part in enumerate(thirds):
        eng.pileup_add(sel=part, rc_from=nf, slot=k % 2)
    _equal(eng.pileup_finish(), one)
    eng.pileup_begin()
    errors = []

    def feeder(slot, part):
        try:
            for piece in np.array_split(part, 3):
                eng.pileup_add(sel=piece, rc_from=nf, slot=slot)
        except Exception as e:                       # (shown by the assertion below)
            errors.append(e)

    halves = np.array_split(sel, 2)
    threads = [threading.Thread(target=feeder, args=(slot, halves[slot])) for slot in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    _equal(eng.pileup_finish(), one)
    st = eng.last_pileup_stats()
    assert st["adds"] == 6 and st["alignments"] == st_one["alignments"] and st["columns"] == st_one["columns"]
    eng.close()
    monkeypatch.setenv("GACT_HIP_PATH_BUDGET_MB", "1")                   # read at create: a fresh engine
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    eng.pileup_begin()
    eng.pileup_add(sel=sel, rc_from=nf)
    _equal(eng.pileup_finish(), one)
    st = eng.last_pileup_stats()
    eng.close()
    assert st["chunks"] > 1 and st["adds"] == 1 and st["columns"] == st_one["columns"]


def test_finish_twice_more_adds_after_a_finish_and_a_second_begin():
    from gact_amd import engine
    blk, nf, sel = _small()
    ref = _reference()
    more = np.setdiff1d(path_cases.sample(nf, len(blk.cr), 40, seed=3), sel).astype(np.int32)
    assert len(more) >= 10
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    eng.pileup_begin()
    eng.pileup_add(sel=sel, rc_from=nf)
    first = eng.pileup_finish()
    _equal(first, ref["one"])
    _equal(eng.pileup_finish(), first)
    other_depth = eng.pileup_finish(min_depth=1)
    assert np.array_equal(other_depth[1], first[1]) and (other_depth[2] != first[2]).any()
    only = eng.pileup_finish(min_depth=3, counts=False, consensus=False)
    assert only[1] is None and only[2] is None and only[0].tobytes() == first[0].tobytes()
    eng.pileup_add(sel=more, rc_from=nf)
    union = eng.pileup_finish()
    extra = eng.candidates_paths(sel=more, rc_from=nf)
    path = ref["path"]
    both = (np.concatenate([path[0], extra[0]]), np.concatenate([path[1], extra[1]]), None)
    both[1]["op_offset"][len(sel):] += len(path[2])
    _same(union, _model(blk.rs, both[0], both[1], np.concatenate([path[2], extra[2]]), min_depth=3), "the union")
    assert union[1].sum() > first[1].sum()
    eng.pileup_begin()
    zero = eng.pileup_finish(min_depth=1)
    assert not zero[1].any() and zero[0].tobytes() == bytes(32 * len(blk.rs.reads))
    assert zero[2].tobytes() == blk.rs.concat()[0].tobytes()
    assert eng.last_pileup_stats()["adds"] == 0
    eng.close()


def test_a_window_gives_the_full_windows_slice():
    blk, nf, sel = _small()
    ref = _reference()
    reads, counts, cons = ref["one"]
    n_all = len(blk.rs.reads)
    first, n_reads = n_all // 3, n_all // 2
    start = np.concatenate([[0], np.cumsum([len(r) for r in blk.rs.reads])])
    part = slice(int(start[first]), int(start[first + n_reads]))
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    eng.pileup_begin(first, n_reads)
    eng.pileup_add(sel=sel, rc_from=nf)
    got = eng.pileup_finish()
    st = eng.last_pileup_stats()
    _equal(got, (reads[first:first + n_reads], counts[part], cons[part]))
    inside = int(reads["n_alignments"][first:first + n_reads].sum())
    assert 0 < inside < int(reads["n_alignments"].sum()) and st["alignments"] == inside
    assert st["positions"] == part.stop - part.start and st["scratch_bytes"] >= 33 * st["positions"]
    # to the set's end; an empty window; an empty selection
    eng.pileup_begin(n_all - 2)
    eng.pileup_add(sel=sel, rc_from=nf)
    _equal(eng.pileup_finish(), (reads[-2:], counts[start[-3]:], cons[start[-3]:]))
    eng.pileup_begin(5, 0)
    eng.pileup_add(sel=sel, rc_from=nf)
    empty = eng.pileup_finish()
    assert [len(x) for x in empty] == [0, 0, 0] and eng.last_pileup_stats()["alignments"] == 0
    eng.pileup_begin()
    eng.pileup_add(n=0)
    eng.pileup_add(sel=np.zeros(0, dtype=np.int32), rc_from=nf)
    assert not eng.pileup_finish()[1].any()
    eng.close()


def test_an_add_leaves_the_slots_records_and_statistics_as_they_were():
    blk, nf, sel = _small()
    ref = _reference()
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    eng.candidates_run_mixed(n, nf)
    records = eng.candidates_fetch(n).copy()
    path = eng.candidates_paths(sel=sel[:40], rc_from=nf)
    run_stats, paths_stats = eng.last_run_stats(), eng.last_paths_stats()
    eng.pileup_begin()
    eng.pileup_add(sel=sel, rc_from=nf)
    assert eng.candidates_fetch(n).tobytes() == records.tobytes()
    assert eng.last_run_stats() == run_stats and eng.last_paths_stats() == paths_stats
    again = eng.candidates_paths(sel=sel[:40], rc_from=nf)
    for a, b in zip(path, again):
        assert a.tobytes() == b.tobytes()
    _equal(eng.pileup_finish(), ref["one"])
    eng.close()


def test_every_pass_of_one_slot_keeps_its_own_figures():
    """all six passes behind one run on ONE slot: each one's last_*_stats, read again after every other pass has run, is what
    it was directly after its own call (device_ms included: a call's time is read once and kept), and each result is its model's"""
    from gact_amd import engine
    from conftest import workload_block
    from cover_model import cover
    from graph_model import graph
    from select_model import select
    blk = workload_block("ecoli10x_small")
    lens = np.array([len(r) for r in blk.rs.reads], dtype=np.int32)
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    eng.candidates_run_mixed(n, nf)
    first, got = {}, {}
    got["select"] = eng.select_overlaps(mode="pair")
    first["select"] = eng.last_select_stats()
    sel = got["select"][:40].copy()
    assert len(sel) == 40 and 0 < nf < n
    got["summaries"] = eng.candidates_summaries(sel=sel, rc_from=nf)
    first["summaries"] = eng.last_summaries_stats()
    got["paths"] = eng.candidates_paths(sel=sel, rc_from=nf)
    first["paths"] = eng.last_paths_stats()
    sums = got["summaries"][1]
    got["cover"] = eng.read_coverage(lens, sel=sel, sums=sums, min_depth=2, depth=True)
    first["cover"] = eng.last_cover_stats()
    got["graph"] = eng.overlap_graph(lens, sel=sel, sums=sums, classes=True)
    first["graph"] = eng.last_graph_stats()
    eng.pileup_begin()
    eng.pileup_add(sel=sel, rc_from=nf)
    got["pileup"] = eng.pileup_finish(min_depth=2)
    first["pileup"] = eng.last_pileup_stats()
    again = dict(select=eng.last_select_stats(), summaries=eng.last_summaries_stats(), paths=eng.last_paths_stats(),
                 cover=eng.last_cover_stats(), graph=eng.last_graph_stats(), pileup=eng.last_pileup_stats())
    records = eng.candidates_fetch(n).copy()
    eng.close()
    for name in first:
        assert again[name] == first[name], (name, first[name], again[name])
        assert first[name]["device_ms"] > 0, name
    # every pass counted its own input, not a neighbour's
    assert first["select"]["selected"] == len(got["select"]) and first["select"]["emitted"] == int(records["emitted"].sum())
    assert first["summaries"]["launches"] == 1 and first["paths"]["chunks"] == 1 and first["paths"]["ops"] == len(got["paths"][2])
    assert first["cover"]["reads"] == first["graph"]["reads"] == len(lens) and first["pileup"]["adds"] == 1
    # ... and every result is its model's
    assert got["select"].tolist() == select(records, "pair").tolist()
    rec_s, _ = got["summaries"]
    rec_p, paths, ops = got["paths"]
    assert rec_s.tobytes() == rec_p.tobytes() == records[sel].tobytes()
    for k in range(len(sel)):
        assert sums[k].tobytes() == engine.summarise(ops_of(paths, ops, k)).tobytes(), (k, sums[k])
    want_cover, want_depth = cover(records, lens, sel=sel, sums=sums, min_depth=2)
    assert got["cover"][0].tobytes() == want_cover.tobytes() and np.array_equal(got["cover"][1], want_depth)
    assert first["cover"]["intervals"] == int(want_cover["n_intervals"].sum())
    want_graph = graph(records, lens, sel=sel, sums=sums)
    for name, g in zip(("reads", "arcs", "classes"), got["graph"]):
        assert g.tobytes() == want_graph[name].tobytes(), name
    for name, count in want_graph["counts"].items():
        assert first["graph"][name] == count, name
    want_pileup = _model(blk.rs, rec_p, paths, ops, min_depth=2)
    _same(got["pileup"], want_pileup, "the 40 selected")
    assert first["pileup"]["alignments"] == int(want_pileup[2]["n_alignments"].sum()) > 0


def test_refusals():
    from gact_amd import engine
    from conftest import workload_block
    blk = workload_block("tiny")
    n_reads = len(blk.rs.reads)
    eng = engine.Engine()
    with pytest.raises(engine.GactHipError, match="error -1: pileup_begin: GACT_SET_REF not uploaded"):
        eng.pileup_begin(0, 0)
    with pytest.raises(engine.GactHipError, match="error -1: pileup_add: no window is open"):
        eng.pileup_add(n=1)
    with pytest.raises(engine.GactHipError, match="error -1: pileup_finish: no window is open"):
        eng.pileup_finish()
    with pytest.raises(engine.GactHipError, match="error -1: last_pileup_stats: no window is open"):
        eng.last_pileup_stats()
    eng.close()
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, slots=(0,), n_slots=2)
    for first, count in ((-1, 1), (0, n_reads + 1), (n_reads, 1), (n_reads + 1, 0), (0, -1)):
        with pytest.raises(engine.GactHipError, match="error -1: pileup_begin: the window .* lies outside"):
            eng.pileup_begin(first, count)
    with pytest.raises(engine.GactHipError, match="no window is open"):            # (a refused begin opens none)
        eng.pileup_add(n=n, rc_from=nf)
    eng.pileup_begin()
    for kw, word in ((dict(sel=[0, n]), "error -1: pileup_add: sel.* outside"), (dict(sel=[-1]), "error -1: pileup_add: sel.* outside"),
                     (dict(n=-1), "error -1: pileup_add: bad arguments"), (dict(n=1, slot=1), "error -1: pileup_add: slot 1 holds no candidates"),
                     (dict(n=1, slot=2), "error -1: slot 2 out of range")):
        with pytest.raises(engine.GactHipError, match=word):
            eng.pileup_add(rc_from=nf, **kw)
    for depth in (0, -2):
        with pytest.raises(engine.GactHipError, match="error -1: pileup_finish: min_depth = %d, at least 1" % depth):
            eng.pileup_finish(min_depth=depth)
    st = eng.last_pileup_stats()
    assert st["adds"] == 0 and st["chunks"] == 0 and st["alignments"] == 0 and st["device_ms"] == 0
    assert not eng.pileup_finish(min_depth=1)[1].any()                              # nothing was counted
    # a refused begin closes the window an earlier begin opened: nothing can be finished into arrays sized for another one
    with pytest.raises(engine.GactHipError, match="error -1: pileup_begin: the window .* lies outside"):
        eng.pileup_begin(1, n_reads)
    with pytest.raises(engine.GactHipError, match="error -1: pileup_finish: no window is open"):
        eng.pileup_finish()
    with pytest.raises(engine.GactHipError, match="error -1: pileup_add: no window is open"):
        eng.pileup_add(n=n, rc_from=nf)
    small = np.zeros(4, dtype=np.uint8)
    assert eng.L.gact_hip_pileup_finish(eng.h, 1, None, small.ctypes.data, None) == -1 and not small.any()
    assert b"no window is open" in eng.L.gact_hip_last_error()
    eng.pileup_begin()
    assert not eng.pileup_finish(min_depth=1)[1].any()
    # GACT_SET_REF uploaded again: the window described the earlier one
    cat, offs = blk.rs.concat()
    eng.upload(engine.SET_REF, cat, offs)
    with pytest.raises(engine.GactHipError, match="error -1: pileup_add: GACT_SET_REF was uploaded after"):
        eng.pileup_add(n=n, rc_from=nf)
    eng.close()
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, tile_size=1024, tile_overlap=256)
    with pytest.raises(engine.GactHipError, match="error -1: pileup_begin: tile_size 1024 > GACT_HIP_FAST_TILE"):
        eng.pileup_begin()
    with pytest.raises(engine.GactHipError, match="error -1: pileup_add: tile_size 1024 > GACT_HIP_FAST_TILE"):
        eng.pileup_add(n=n, rc_from=nf)
    eng.close()


def test_driver_pileup(tmp_path):
    from gact_amd import engine, workload
    from conftest import workload_block
    rs = workload_block("tiny").rs
    rs.write_fasta(str(tmp_path / "reads.fasta"))
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()

    def run(name, *extra, ok=True):
        d = tmp_path / name
        d.mkdir()
        os.symlink(tmp_path / "reads.fasta", d / "reads.fasta")
        os.symlink(tmp_path / "params.cfg", d / "params.cfg")
        out = subprocess.run([drv, "reads.fasta", "reads.fasta", "2"] + list(extra), capture_output=True, text=True, cwd=d, timeout=600)
        assert (out.returncode == 0) == ok, out.stdout + out.stderr
        return out, {p.name: p.read_bytes() for p in d.iterdir() if p.name.startswith("darwin.")}

    _, without = run("pair", "--device-dsoft", "--unique", "pair")
    _, files = run("pileup", "--device-dsoft", "--unique", "pair", "--pileup", "2")
    assert sorted(files) == sorted(list(without) + ["darwin.cons.fa"])
    for f in without:
        assert files[f] == without[f], f
    # the same reads, parameters and selection through Engine, feeder by feeder, and the model
    n_reads = len(rs.reads)
    per_thread = -(-n_reads // 2)
    eng, _, _ = engine_with(rs, np.zeros(0, dtype=engine.CAND_DTYPE), np.zeros(0, dtype=engine.CAND_DTYPE), slots=())
    eng.dsoft_build()
    recs, paths, ops, n_ops = [], [], [], 0
    for t in range(2):
        lo = min(n_reads, t * per_thread)
        nf, nr, _ = eng.dsoft_query(lo, min(n_reads, lo + per_thread) - lo)
        eng.candidates_run_mixed(nf + nr, nf)
        sel = eng.select_overlaps(n=nf + nr, mode="pair")
        r, p, o = eng.candidates_paths(sel=sel, rc_from=nf)
        assert r["emitted"].all() and len(sel) > 5
        p["op_offset"] += n_ops
        n_ops += len(o)
        recs.append(r), paths.append(p), ops.append(o)
    eng.close()
    counts, cons, table = _model(rs, np.concatenate(recs), np.concatenate(paths), np.concatenate(ops), min_depth=2)
    start = np.concatenate([[0], np.cumsum([len(r) for r in rs.reads])])
    want = []
    for i, name in enumerate(rs.names):
        t = table[i]
        want.append(">%s called=%d changed=%d deleted=%d ins_flagged=%d" % (re.split(r"[^A-Za-z0-9_]+", name)[0], t["called"], t["changed"],
                                                                              t["deleted"], t["ins_flagged"]))
        want.append(bytes(cons[start[i]:start[i + 1]]).replace(b"-", b"").decode())
    got = files["darwin.cons.fa"].decode().splitlines()
    assert len(got) == 2 * n_reads and got[0::2] == want[0::2]
    assert got == want
    assert int(table["called"].sum()) > 1000 and int(table["changed"].sum()) > 0
    print("driver: %d called, %d changed, %d deleted" % tuple(int(table[k].sum()) for k in ("called", "changed", "deleted")))
    for extra in (("--pileup", "2"), ("--device-dsoft", "--pileup", "2", "--shard", "0/2"), ("--device-dsoft", "--pileup", "0")):
        out, _ = run("refused_" + "_".join(extra).replace("/", "-").replace("--", ""), *extra, ok=False)
        assert "--pileup" in out.stderr
