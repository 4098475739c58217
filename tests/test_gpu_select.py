"""GPU suite for the selection of overlaps (gact_hip_select_overlaps, csrc/gact_select.hpp): the selected indices equal the
model's (tests/select_model.py) in both modes -- on crafted host records of every pattern and size (no alignment runs), on the
device-resident records of a run of both strands, chained into the summaries call, through the refusals, and through the
driver's --unique.  No tolerance anywhere: the lists are compared element by element."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import select_model
from select_model import MODES, crafted, select

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 70001


@pytest.fixture(scope="module")
def eng():
    """an engine that aligns nothing: two slots, workspaces for one block"""
    from gact_amd import engine
    e = engine.Engine(n_slots=2, max_blocks=1)
    yield e
    e.close()


_MODEL = {}


def _model(pattern, n, mode):
    if (pattern, n, mode) not in _MODEL:
        _MODEL[(pattern, n, mode)] = select(crafted(pattern, n), mode)
    return _MODEL[(pattern, n, mode)]


@pytest.mark.parametrize("pattern", select_model.PATTERNS)
def test_crafted_host_records_equal_the_model_at_every_size(eng, pattern):
    assert select_model.SIZES == (0, 1, 63, 64, 65, 255, 256, 257, 1000, BIG)
    for n in select_model.SIZES:
        rec = crafted(pattern, n)
        before = rec.tobytes()
        for mode in MODES:
            want = _model(pattern, n, mode)
            got = eng.select_overlaps(records=rec, mode=mode)
            assert got.dtype == np.int32 and got.tolist() == want.tolist(), (pattern, n, mode)
            if n:
                st = eng.last_select_stats()
                slots = st["table_slots"]
                assert st["emitted"] == int(rec["emitted"].astype(bool).sum()) and st["selected"] == len(want)
                assert slots >= 2 * n and slots & (slots - 1) == 0 and slots < 4 * n + 2
                assert 0 < st["scratch_bytes"] and st["device_ms"] > 0
        assert rec.tobytes() == before


@pytest.mark.parametrize("pattern", ["mixed", "one_pair", "straddle"])
def test_the_list_is_the_same_on_every_run_and_on_every_slot(eng, pattern):
    rec = crafted(pattern, BIG)
    for mode in MODES:
        want = _model(pattern, BIG, mode).tolist()
        first = eng.select_overlaps(records=rec, mode=mode, slot=0)
        second = eng.select_overlaps(records=rec, mode=mode, slot=0)
        other = eng.select_overlaps(records=rec, mode=mode, slot=1)
        assert first.tolist() == second.tolist() == other.tolist() == want
    # a smaller selection after a larger one on the same scratch, and the larger one again
    small = crafted(pattern, 257)
    assert eng.select_overlaps(records=small, mode="pair").tolist() == _model(pattern, 257, "pair").tolist()
    assert eng.select_overlaps(records=rec, mode="pair").tolist() == _model(pattern, BIG, "pair").tolist()
    # n < len(records): the first n only
    assert eng.select_overlaps(n=1000, records=rec, mode="exact").tolist() == select(rec[:1000], "exact").tolist()


@pytest.fixture(scope="module")
def small_run():
    """ecoli10x_small, both strands, run on slot 0; the selections are made BEFORE the records are fetched"""
    from conftest import workload_block
    from path_cases import engine_with
    blk = workload_block("ecoli10x_small")
    e, n, nf = engine_with(blk.rs, blk.cf, blk.cr, n_slots=2)
    e.candidates_run_mixed(n, nf)
    run_stats = e.last_run_stats()
    got = {mode: e.select_overlaps(mode=mode) for mode in MODES}
    stats = e.last_select_stats()
    records = e.candidates_fetch(n).copy()
    yield dict(eng=e, n=n, nf=nf, got=got, stats=stats, records=records, run_stats=run_stats)
    e.close()


def test_device_records_of_a_run_of_both_strands_equal_the_model(small_run):
    r = small_run
    records, n, nf = r["records"], r["n"], r["nf"]
    assert 0 < nf < n and (records["comp"][:nf] == 0).all() and (records["comp"][nf:] == 1).all()
    want = {mode: select(records, mode) for mode in MODES}
    for mode in MODES:
        assert r["got"][mode].tolist() == want[mode].tolist(), mode
    emitted = int(records["emitted"].sum())
    exact, pair = len(want["exact"]), len(want["pair"])
    print("candidates %d, emitted %d, exact %d, pair %d" % (n, emitted, exact, pair))
    assert 0 < pair < exact < emitted
    assert emitted - pair >= emitted // 20
    slots = r["stats"]["table_slots"]
    assert r["stats"]["emitted"] == emitted and r["stats"]["selected"] == pair              # (pair was the last call)
    assert slots >= 2 * n and slots & (slots - 1) == 0
    # an explicit n: the first n records only
    assert r["eng"].select_overlaps(n=nf, mode="pair").tolist() == select(records[:nf], "pair").tolist()


def test_what_a_selection_leaves_on_its_slot(small_run):
    r = small_run
    e, n, nf = r["eng"], r["n"], r["nf"]
    some = np.arange(0, n, 9, dtype=np.int32)
    e.candidates_paths(sel=some, rc_from=nf)
    e.candidates_summaries(sel=some, rc_from=nf)
    paths_stats, sums_stats, select_stats = e.last_paths_stats(), e.last_summaries_stats(), e.last_select_stats()
    for mode in MODES:
        assert e.select_overlaps(mode=mode).tolist() == r["got"][mode].tolist()
    assert e.candidates_fetch(n).tobytes() == r["records"].tobytes()
    assert e.last_run_stats() == r["run_stats"]            # (times included: a run's times are read once and kept)
    assert e.last_paths_stats() == paths_stats and e.last_summaries_stats() == sums_stats
    # host records on the same slot leave the slot's own records alone, and the other slot's selection leaves this one's figures
    e.select_overlaps(records=crafted("mixed", 1000), mode="pair")
    assert e.candidates_fetch(n).tobytes() == r["records"].tobytes()
    mine = e.last_select_stats()
    assert mine["emitted"] != select_stats["emitted"]
    e.select_overlaps(records=crafted("mixed", 257), mode="exact", slot=1)
    assert e.last_select_stats() == mine
    assert e.last_run_stats() == r["run_stats"]            # (times included: a run's times are read once and kept)


def test_the_pair_selection_chained_into_the_summaries_call(small_run):
    r = small_run
    e, n, nf, records = r["eng"], r["n"], r["nf"], r["records"]
    sel = e.select_overlaps(mode="pair")
    st = e.last_select_stats()
    want = select(records, "pair")
    assert sel.tolist() == want.tolist() and len(sel) > 0
    assert st["emitted"] == int(records["emitted"].sum()) and st["selected"] == len(want)
    assert st["table_slots"] >= 2 * n and st["table_slots"] & (st["table_slots"] - 1) == 0
    all_records, all_sums = e.candidates_summaries(n=n, rc_from=nf)
    got_records, got_sums = e.candidates_summaries(sel=sel, rc_from=nf)
    assert len(got_sums) == len(got_records) == len(sel)
    assert got_sums.tobytes() == all_sums[sel].tobytes()
    assert got_records.tobytes() == all_records[sel].tobytes() == records[sel].tobytes()
    assert (got_records["emitted"] == 1).all()


def test_refusals(small_run):
    from gact_amd import engine
    r = small_run
    e, n = r["eng"], r["n"]
    L = e.L
    rec = crafted("mixed", 1000)
    want = select(rec, "pair")
    sel = np.full(1000, -5, dtype=np.int32)
    n_sel = ctypes.c_int32(-1)
    # bad mode
    for mode in (2, -1):
        assert L.gact_hip_select_overlaps(e.h, 0, 1000, rec.ctypes.data, mode, sel.ctypes.data, 1000, ctypes.byref(n_sel)) == -1
        assert b"mode" in L.gact_hip_last_error() and n_sel.value == 0
    with pytest.raises(engine.GactHipError, match="mode"):
        e.select_overlaps(records=rec, mode="best")
    # n < 0
    assert L.gact_hip_select_overlaps(e.h, 0, -1, rec.ctypes.data, 1, sel.ctypes.data, 1000, ctypes.byref(n_sel)) == -1
    # records == NULL on a slot without records (slot 1 never held candidates), and n beyond the slot's array
    with pytest.raises(engine.GactHipError, match="no records"):
        e.select_overlaps(n=1, mode="pair", slot=1)
    with pytest.raises(engine.GactHipError, match="beyond"):
        e.select_overlaps(n=n + 1, mode="pair", slot=0)
    with pytest.raises(engine.GactHipError, match="slot"):
        e.select_overlaps(records=rec, slot=2)
    assert (sel == -5).all()
    # n == 0 is no error, records or not, fresh slot or not
    assert L.gact_hip_select_overlaps(e.h, 1, 0, None, 1, None, 0, ctypes.byref(n_sel)) == 0 and n_sel.value == 0
    assert len(e.select_overlaps(records=rec[:0])) == 0
    # too little room: EINVAL with n_sel set, nothing written; the retry with that much room succeeds
    n_sel.value = -1
    assert L.gact_hip_select_overlaps(e.h, 0, 1000, rec.ctypes.data, 1, sel.ctypes.data, len(want) - 1, ctypes.byref(n_sel)) == -1
    assert n_sel.value == len(want) and (sel == -5).all() and b"room" in L.gact_hip_last_error()
    assert L.gact_hip_select_overlaps(e.h, 0, 1000, rec.ctypes.data, 1, None, 1000, ctypes.byref(n_sel)) == -1
    assert n_sel.value == len(want)
    assert L.gact_hip_select_overlaps(e.h, 0, 1000, rec.ctypes.data, 1, sel.ctypes.data, n_sel.value, ctypes.byref(n_sel)) == 0
    assert sel[:n_sel.value].tolist() == want.tolist() and (sel[n_sel.value:] == -5).all()
    with pytest.raises(engine.GactHipError, match="no selection"):
        fresh = engine.Engine(max_blocks=1)
        try:
            fresh.last_select_stats()
        finally:
            fresh.close()


def test_driver_unique(tmp_path):
    from gact_amd import engine, workload
    from conftest import workload_block
    rs = workload_block("tiny").rs
    rs.write_fasta(str(tmp_path / "reads.fasta"))
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()

    def run(name, *extra):
        d = tmp_path / name
        d.mkdir()
        os.symlink(tmp_path / "reads.fasta", d / "reads.fasta")
        os.symlink(tmp_path / "params.cfg", d / "params.cfg")
        out = subprocess.run([drv, "reads.fasta", "reads.fasta", "2", "--device-dsoft"] + list(extra), capture_output=True, text=True,
                             cwd=d, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        read = lambda ext: [open(d / ("darwin.%d.%s" % (t, ext))).read().splitlines() if os.path.exists(d / ("darwin.%d.%s" % (t, ext)))
                            else None for t in range(2)]
        return read("out"), read("paf")

    plain, _ = run("plain")
    exact, no_paf = run("exact", "--unique", "exact")
    assert no_paf == [None, None]
    for t in range(2):
        # each feeder's file: every line of the plain file once, in the plain file's order
        first_seen = list(dict.fromkeys(plain[t]))
        assert exact[t] == first_seen
    lines = plain[0] + plain[1]
    assert sorted(exact[0] + exact[1]) == sorted(set(lines)) and len(lines) > 10
    print("driver: %d lines, %d distinct" % (len(lines), len(set(lines))))
    pair_out, pair_paf = run("pair", "--unique", "pair", "--paf")
    seen = set()
    for t in range(2):
        assert set(pair_out[t]) <= set(exact[t]) and len(pair_paf[t]) == len(pair_out[t]) > 0
        for line in pair_paf[t]:
            f = line.split("\t")
            assert (f[0], f[5], f[4]) not in seen, line
            seen.add((f[0], f[5], f[4]))
    # one line per (ref, query, strand) of the plain output
    keys = lambda ls: {(l.split(",")[0], l.split(",")[1], l.rsplit(",", 1)[1]) for l in ls}
    assert len(pair_out[0] + pair_out[1]) == len(keys(lines)) == len(seen)
