"""GPU suite for the inserted bases of the pileup and the corrected reads (gact_hip_pileup_begin_ins / gact_hip_pileup_corrected):
the slot table, the per-read table, read_at and the bytes equal tests/pileup_ins_model.py's fed with the path run's own ops --
on reads crafted so that insertion runs straddle a 64-column step, a tile boundary and the junction of the two extensions, on
the crafted candidates of tests/path_cases.py and on a sample of ecoli10x_small at both tile geometries and both scorings;
one selection added in five ways gives the same bytes; windows; the refusals and the seq_cap protocol; the driver's
--ins-slots.  Exact equality everywhere: integers and bytes are equal or the test fails."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import path_cases
from path_cases import engine_with, ops_of
from path_model import gact_path
from pileup_ins_model import pileup_ins
from pileup_model import columns

pytestmark = pytest.mark.gpu


class _Rc:
    """rc[i]: read i's reverse complement, made when asked for"""

    def __init__(self, rs):
        self.rs, self.made = rs, {}

    def __getitem__(self, i):
        if i not in self.made:
            self.made[i] = self.rs.rc(i)
        return self.made[i]


def _model(rs, records, paths, ops, ins_slots, window=None, min_depth=1):
    window = (0, len(rs.reads)) if window is None else window
    return pileup_ins(rs.reads, _Rc(rs), records, [ops_of(paths, ops, k) for k in range(len(records))], window, min_depth, ins_slots)


def _same(got, want, what=""):
    """got: Engine.pileup_corrected(ins=True)'s (reads, read_at, seq, ins); want: the model's (ins, table, read_at, seq, ...)"""
    reads, read_at, seq, ins = got
    assert ins.shape == want[0].shape and reads.shape == want[1].shape and read_at.shape == want[2].shape, what
    if not np.array_equal(ins, want[0]):
        p, j, k = [int(v[0]) for v in np.nonzero(ins != want[0])]
        raise AssertionError("%s: slots differ first at position %d slot %d: %s, model %s" % (what, p, j, ins[p, j], want[0][p, j]))
    assert reads.tobytes() == want[1].tobytes(), (what, [(i, reads[i], want[1][i]) for i in np.flatnonzero(reads != want[1])[:3]])
    assert np.array_equal(read_at, want[2]), what
    assert seq == want[3], (what, len(seq), len(want[3]))


def _equal(a, b):
    """two pileup_corrected(ins=True) or pileup_finish results, byte for byte"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, bytes):
            assert x == y
        else:
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


RUN_TILE = (64, 24)
RUN_SPACING = 61                                        # columns from one inserted block's first to the next one's: coprime with 64
RUN_BLOCKS = (1, 2, 3, 6)


def crafted_runs():
    """-> (rs, cf, cr, junction): read 1 is read 0 with blocks of 1, 2, 3, 6, 1, ... random bases put in, block k's first column
    61 (k + 1) columns behind the alignment's first; read 2 is read 1's reverse complement.  Candidates: read 0 against read 1
    seeded in the middle of a stretch, against read 2's reverse complement likewise, and (`junction`, its index) seeded at the
    first base behind a stretch, where a block of 6 follows: the left extension ends there and the right one begins with the run"""
    from gact_amd import engine, synth
    rng = np.random.default_rng(20261020)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    target = acgt[rng.integers(0, 4, 4000)]
    parts, at, column, where = [], 0, 0, []            # where[k]: (target position, query position) of block k's first base
    k = 0
    while True:
        p = RUN_SPACING * (k + 1) - column + at         # the target position in front of which block k goes
        if p >= len(target) - 40:
            break
        parts.append(target[at:p])
        column += p - at
        block = acgt[rng.integers(0, 4, RUN_BLOCKS[k % 4])]
        where.append((p, column))
        parts.append(block)
        column += len(block)
        at = p
        k += 1
    parts.append(target[at:])
    query = np.concatenate(parts)
    rs = synth.ReadSet()
    for seq in (target, query, synth.revcomp(query)):
        rs.reads.append(np.ascontiguousarray(seq, dtype=np.uint8))
        rs.names.append("R%d" % len(rs.reads))
    six = [w for k, w in enumerate(where) if RUN_BLOCKS[k % 4] == 6]
    mid, at_six = where[len(where) // 2], six[len(six) // 2]
    cf = np.array([(0, 1, mid[0] - 30, mid[1] - 30), (0, 1, at_six[0], at_six[1])], dtype=engine.CAND_DTYPE)
    cr = np.array([(0, 2, mid[0] + 20, mid[1] + RUN_BLOCKS[(len(where) // 2) % 4] + 20)], dtype=engine.CAND_DTYPE)
    return rs, cf, cr, 1


def run_shapes(cols, n_left, tile_ends):
    """what the runs of 'I' of one alignment's columns do: the set of "step" (a run goes on across a multiple of 64 columns),
    "tile" (across the end of a tile's columns), "junction" (the right extension's first column is an 'I') and "long:<n>" """
    seen = set()
    for c in range(1, len(cols)):
        if cols[c] == "I" and cols[c - 1] == "I":
            if c % 64 == 0:
                seen.add("step")
            if c in tile_ends:
                seen.add("tile")
    if 0 < n_left < len(cols) and cols[n_left] == "I":
        seen.add("junction")
    for m in re.finditer("I+", cols):
        seen.add("long:%d" % len(m.group()))
    return seen


def model_tiles(oracle, rs, cands, nf, k, tile=RUN_TILE):
    """the chain model's alignment of candidate k: (CIGAR, columns of the left extension, the column indices at which a tile's
    columns end)"""
    ref, query = path_cases.reads_of(rs, cands, nf, k)
    m = gact_path(oracle.align_with_bt, ref, query, int(cands[k]["ref_pos"]), int(cands[k]["query_pos"]), tile_size=tile[0],
                  tile_overlap=tile[1])
    from gact_amd import engine
    left = [t[9] for t in m["tiles"] if not t[4]]
    right = [t[9] for t in m["tiles"] if t[4]]
    n_left = sum(left)
    ends = set((n_left - np.cumsum(left)).tolist()) | set((n_left + np.cumsum(right)).tolist())
    return engine.cigar_string(m["ops"]), n_left, ends - {0, len(m["cols"])}


def test_crafted_runs_across_steps_tiles_and_the_junction_equal_the_model(oracle):
    rs, cf, cr, junction = crafted_runs()
    cands = np.concatenate([cf, cr])
    eng, n, nf = engine_with(rs, cf, cr, tile_size=RUN_TILE[0], tile_overlap=RUN_TILE[1])
    records, paths, ops = eng.candidates_paths(n=n, rc_from=nf)
    assert records["emitted"].all()
    # the inputs do what they were made for, by the chain model's own account
    seen = []
    for k in range(n):
        cigar, n_left, tile_ends = model_tiles(oracle, rs, cands, nf, k)
        from gact_amd import engine
        assert engine.cigar_string(ops_of(paths, ops, k)) == cigar, k
        seen.append(run_shapes(columns(cigar), n_left, tile_ends))
    assert "junction" in seen[junction], seen[junction]
    for k in range(n):
        assert {"step", "tile", "long:1", "long:2", "long:3", "long:6"} <= seen[k], (k, seen[k])
    eng.pileup_begin()
    eng.pileup_add(n=n, rc_from=nf)
    plain = eng.pileup_finish(min_depth=1)
    truncated = {}
    for k in (1, 2, 4):
        want = _model(rs, records, paths, ops, k)
        truncated[k] = want[4]
        assert want[1]["inserted"][0] > 20 * min(k, 3) and want[4] > 0, (k, want[1], want[4])      # (at 4 slots: the runs of 6)
        eng.pileup_begin(ins_slots=k)
        eng.pileup_add(n=n, rc_from=nf)
        _same(eng.pileup_corrected(min_depth=1, ins=True), want, "%d slots" % k)
        st = eng.last_pileup_ins_stats()
        assert st["ins_slots"] == k and st["runs_truncated"] == want[4] and st["slot_adds"] == int(want[0].sum())
        assert st["emitted"] == int(want[1]["inserted"].sum()) and st["table_bytes"] == want[0].nbytes and st["device_ms"] > 0
        _equal(eng.pileup_finish(min_depth=1), plain)
    eng.close()
    assert truncated[1] > truncated[2] > truncated[4]


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


def _inputs(name):
    if name == "small60":
        blk, nf, sel = _small(60)
        return blk.rs, blk.cf, blk.cr, sel
    cr = path_cases.crafted(name == "crafted-raw")
    return cr.rs, cr.cf, cr.cr, np.arange(len(cr.cf) + len(cr.cr), dtype=np.int32)


@pytest.mark.parametrize("scoring", [(1, -1, -1, -1), (2, -3, -5, -2)])
@pytest.mark.parametrize("tile_size,tile_overlap", [(320, 120), (64, 24)])
@pytest.mark.parametrize("name", ["crafted-raw", "crafted-acgt", "small60"])
def test_both_tile_geometries_and_scorings_equal_the_model(name, tile_size, tile_overlap, scoring):
    rs, cf, cr, sel = _inputs(name)
    eng, n, nf = engine_with(rs, cf, cr, tile_size=tile_size, tile_overlap=tile_overlap, scoring=scoring)
    records, paths, ops = eng.candidates_paths(sel=sel, rc_from=nf)
    eng.pileup_begin(ins_slots=2)
    eng.pileup_add(sel=sel, rc_from=nf)
    got = eng.pileup_corrected(min_depth=2, ins=True)
    st = eng.last_pileup_ins_stats()
    eng.close()
    want = _model(rs, records, paths, ops, 2, min_depth=2)
    assert int(want[1]["inserted"].sum()) > 0 and int(want[1]["deleted"].sum()) > 0 and want[4] > 0
    _same(got, want)
    assert st["runs_truncated"] == want[4] and st["slot_adds"] == int(want[0].sum()) and st["emitted"] == int(want[1]["inserted"].sum())


_REFERENCE = {}


def _reference():
    """the 150-candidate sample on the default engine with two slots: the path run, the corrected reads of one add at min_depth 3,
    the statistics, the plain finish -- made once, left unchanged, and held to the model here"""
    if not _REFERENCE:
        blk, nf, sel = _small()
        eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
        path = eng.candidates_paths(sel=sel, rc_from=nf)
        eng.pileup_begin(ins_slots=2)
        eng.pileup_add(sel=sel, rc_from=nf)
        one = eng.pileup_corrected(ins=True)
        st = eng.last_pileup_ins_stats()
        finish = eng.pileup_finish()
        eng.close()
        _same(one, _model(blk.rs, *path, 2, min_depth=3), "one add")
        assert st["emitted"] > 0
        _REFERENCE.update(path=path, one=one, stats=st, finish=finish)
    return _REFERENCE


def _counted(st):
    return {k: st[k] for k in ("ins_slots", "slot_adds", "runs_truncated", "emitted", "table_bytes")}


def test_one_selection_added_in_five_ways_gives_the_same_bytes(monkeypatch):
    blk, nf, sel = _small()
    ref = _reference()
    one, st_one = ref["one"], _counted(ref["stats"])
    thirds = np.array_split(sel, 3)
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, slots=(0, 1), n_slots=2)
    eng.pileup_begin(ins_slots=2)
    for part in thirds:
        eng.pileup_add(sel=part, rc_from=nf)
    _equal(eng.pileup_corrected(ins=True), one)
    assert _counted(eng.last_pileup_ins_stats()) == st_one
    eng.pileup_begin(ins_slots=2)
    for k, part in enumerate(thirds):
        eng.pileup_add(sel=part, rc_from=nf, slot=k % 2)
    _equal(eng.pileup_corrected(ins=True), one)
    _equal(eng.pileup_corrected(ins=True), one)                          # ... and again: the counts stay
    eng.pileup_begin(ins_slots=2)
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
    _equal(eng.pileup_corrected(ins=True), one)
    assert _counted(eng.last_pileup_ins_stats()) == st_one
    _equal(eng.pileup_finish(), ref["finish"])
    eng.close()
    monkeypatch.setenv("GACT_HIP_PATH_BUDGET_MB", "1")                   # read at create: a fresh engine
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    eng.pileup_begin(ins_slots=2)
    eng.pileup_add(sel=sel, rc_from=nf)
    _equal(eng.pileup_corrected(ins=True), one)
    assert eng.last_pileup_stats()["chunks"] > 1 and _counted(eng.last_pileup_ins_stats()) == st_one
    eng.close()


def test_a_window_gives_the_full_windows_slice():
    blk, nf, sel = _small()
    ref = _reference()
    reads, read_at, seq, ins = ref["one"]
    n_all = len(blk.rs.reads)
    first, n_reads = n_all // 3, n_all // 2
    start = np.concatenate([[0], np.cumsum([len(r) for r in blk.rs.reads])])

    def part_of(a, b):
        return (reads[a:b], read_at[a:b + 1] - read_at[a], seq[read_at[a]:read_at[b]], ins[start[a]:start[b]])

    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    eng.pileup_begin(first, n_reads, ins_slots=2)
    eng.pileup_add(sel=sel, rc_from=nf)
    got = eng.pileup_corrected(ins=True)
    _equal(got, part_of(first, first + n_reads))
    assert 0 < int(got[0]["inserted"].sum()) < int(reads["inserted"].sum())
    st = eng.last_pileup_stats()
    assert st["scratch_bytes"] >= (32 + 2 * 16 + 1) * st["positions"]
    # to the set's end; an empty window; an empty selection
    eng.pileup_begin(n_all - 2, ins_slots=2)
    eng.pileup_add(sel=sel, rc_from=nf)
    _equal(eng.pileup_corrected(ins=True), part_of(n_all - 2, n_all))
    eng.pileup_begin(5, 0, ins_slots=2)
    eng.pileup_add(sel=sel, rc_from=nf)
    empty = eng.pileup_corrected(ins=True)
    assert len(empty[0]) == 0 and empty[1].tolist() == [0] and empty[2] == b"" and empty[3].shape == (0, 2, 4)
    eng.pileup_begin(ins_slots=2)
    eng.pileup_add(n=0)
    eng.pileup_add(sel=np.zeros(0, dtype=np.int32), rc_from=nf)
    nothing = eng.pileup_corrected(min_depth=1, ins=True)
    assert not nothing[3].any() and nothing[2] == blk.rs.concat()[0].tobytes() and np.array_equal(nothing[1], start)
    assert not nothing[0]["inserted"].any() and np.array_equal(nothing[0]["length"], np.diff(start))
    eng.close()


FILLERS = 260                                           # reads in front of the aligned ones: more than one chunk of pileup_scan_kernel (256)


def _fillers(n, seed=20261021):
    """n reads of 64 to 100 random bases"""
    from gact_amd import synth
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rs = synth.ReadSet()
    for k in range(n):
        rs.reads.append(acgt[rng.integers(0, 4, int(rng.integers(64, 101)))])
        rs.names.append("F%d" % k)
    return rs


def test_aligned_reads_behind_a_chunk_of_unaligned_ones_equal_the_model():
    """pileup_scan_kernel takes 256 reads a chunk and carries the bases and the inserted bases on: here every read with an
    alignment lies in the second chunk, behind 260 short reads that nothing aligns to"""
    from conftest import workload_block
    blk = workload_block("tiny")
    rs = _fillers(FILLERS)
    rs.reads += list(blk.rs.reads)
    rs.names += list(blk.rs.names)
    cf, cr = blk.cf.copy(), blk.cr.copy()
    for c in (cf, cr):
        c["ref_id"] += FILLERS
        c["query_id"] += FILLERS
    assert 256 < FILLERS < len(rs.reads) <= 512 and len(cf) > 0 and len(cr) > 0
    eng, n, nf = engine_with(rs, cf, cr)
    records, paths, ops = eng.candidates_paths(n=n, rc_from=nf)
    eng.pileup_begin(ins_slots=2)
    eng.pileup_add(n=n, rc_from=nf)
    got = eng.pileup_corrected(min_depth=2, ins=True)
    st = eng.last_pileup_ins_stats()
    eng.close()
    want = _model(rs, records, paths, ops, 2, min_depth=2)
    table, read_at = want[1], want[2]
    assert int(table["inserted"][FILLERS:].sum()) > 0 and not table["inserted"][:FILLERS].any() and read_at[256] > 0
    _same(got, want)
    assert st["emitted"] == int(table["inserted"].sum())


def test_a_window_of_513_reads_with_no_add_gives_the_reads_back():
    """two full chunks of the scan and one read in a third"""
    from gact_amd import engine
    rs = _fillers(513, seed=20261022)
    none = np.zeros(0, dtype=engine.CAND_DTYPE)
    eng, _, _ = engine_with(rs, none, none, slots=())
    eng.pileup_begin(ins_slots=2)
    reads, read_at, seq, ins = eng.pileup_corrected(min_depth=1, ins=True)
    st = eng.last_pileup_ins_stats()
    eng.close()
    cat, offs = rs.concat()
    assert len(read_at) == 514 and np.array_equal(read_at, offs) and seq == cat.tobytes()
    assert np.array_equal(reads["length"], np.diff(offs)) and not reads["inserted"].any() and not ins.any() and st["emitted"] == 0


def test_no_slots_the_room_protocol_and_the_refusals():
    import ctypes
    from gact_amd import engine
    blk, nf, sel = _small()
    ref = _reference()
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    # without slots: the consensus with every '-' left out
    eng.pileup_begin()
    eng.pileup_add(sel=sel, rc_from=nf)
    _equal(eng.pileup_finish(), ref["finish"])
    table, _, cons = ref["finish"]
    reads, read_at, seq = eng.pileup_corrected()
    assert int(table["deleted"].sum()) > 0 and seq == cons.tobytes().replace(b"-", b"") and read_at[-1] == len(seq)
    assert not reads["inserted"].any() and not reads["ins_sites"].any()
    assert np.array_equal(reads["deleted"], table["deleted"]) and np.array_equal(reads["changed"], table["changed"])
    st = eng.last_pileup_ins_stats()
    assert _counted(st) == dict(ins_slots=0, slot_adds=0, runs_truncated=0, emitted=0, table_bytes=0) and st["device_ms"] > 0
    with pytest.raises(engine.GactHipError, match="error -1: pileup_corrected: the window was opened without slots"):
        eng.pileup_corrected(ins=True)
    # gact_hip_pileup_begin_ins with no slots is gact_hip_pileup_begin
    assert eng.L.gact_hip_pileup_begin_ins(eng.h, 0, len(blk.rs.reads), 0) == 0
    eng.pileup_add(sel=sel, rc_from=nf)
    _equal(eng.pileup_finish(), ref["finish"])
    # room: too little is refused with everything else filled in, and the length it names is enough
    want = ref["one"]
    eng.candidates_run_mixed(n, nf)
    records = eng.candidates_fetch(n).copy()
    before = dict(run=eng.last_run_stats())
    eng.pileup_begin(ins_slots=2)
    eng.pileup_add(sel=sel, rc_from=nf)
    before["pileup"] = eng.last_pileup_stats()
    n_reads = len(blk.rs.reads)
    reads = np.zeros(n_reads, dtype=engine.READ_CORRECTED_DTYPE)
    read_at = np.zeros(n_reads + 1, dtype=np.int64)
    seq_len = ctypes.c_int64()
    small = np.zeros(len(want[2]) - 1, dtype=np.uint8)
    rc = eng.L.gact_hip_pileup_corrected(eng.h, 3, None, reads.ctypes.data, read_at.ctypes.data, small.ctypes.data, len(small),
                                         ctypes.byref(seq_len))
    assert rc == -1 and re.search(r"pileup_corrected: %d bases, room for %d: call again" % (len(want[2]), len(small)),
                                  eng.L.gact_hip_last_error().decode())
    assert seq_len.value == len(want[2]) and not small.any()
    assert reads.tobytes() == want[0].tobytes() and np.array_equal(read_at, want[1])
    exact = np.zeros(seq_len.value, dtype=np.uint8)
    assert eng.L.gact_hip_pileup_corrected(eng.h, 3, None, None, None, exact.ctypes.data, len(exact), ctypes.byref(seq_len)) == 0
    assert exact.tobytes() == want[2]
    assert eng.L.gact_hip_pileup_corrected(eng.h, 3, None, None, None, None, 0, ctypes.byref(seq_len)) == 0       # only the length
    assert seq_len.value == len(want[2])
    _equal(eng.pileup_corrected(ins=True), want)
    # the slot's records and every other pass's figures stay as they were
    assert eng.candidates_fetch(n).tobytes() == records.tobytes()
    assert eng.last_run_stats() == before["run"] and eng.last_pileup_stats() == before["pileup"]
    # refusals
    for depth in (0, -2):
        with pytest.raises(engine.GactHipError, match="error -1: pileup_corrected: min_depth = %d, at least 1" % depth):
            eng.pileup_corrected(min_depth=depth)
    assert eng.L.gact_hip_pileup_corrected(eng.h, 3, None, None, None, exact.ctypes.data, -1, ctypes.byref(seq_len)) == -1
    assert b"pileup_corrected: seq_cap = -1" in eng.L.gact_hip_last_error()
    for slots in (-1, 5):
        with pytest.raises(engine.GactHipError, match=r"error -1: pileup_begin: ins_slots = %d outside \[0, 4\]" % slots):
            eng.pileup_begin(ins_slots=slots)
        with pytest.raises(engine.GactHipError, match="error -1: pileup_corrected: no window is open"):        # (a refused begin opens none)
            eng.pileup_corrected()
        assert eng.L.gact_hip_pileup_corrected(eng.h, 3, None, None, None, None, 0, ctypes.byref(seq_len)) == -1
        assert b"pileup_corrected: no window is open" in eng.L.gact_hip_last_error()
        with pytest.raises(engine.GactHipError, match="error -1: last_pileup_ins_stats: no window is open"):
            eng.last_pileup_ins_stats()
    eng.pileup_begin(ins_slots=4)
    cat, offs = blk.rs.concat()
    eng.upload(engine.SET_REF, cat, offs)
    with pytest.raises(engine.GactHipError, match="error -1: pileup_corrected: GACT_SET_REF was uploaded after"):
        eng.pileup_corrected()
    eng.close()
    eng = engine.Engine()
    with pytest.raises(engine.GactHipError, match="error -1: pileup_begin: GACT_SET_REF not uploaded"):
        eng.pileup_begin(0, 0, ins_slots=1)
    with pytest.raises(engine.GactHipError, match="error -1: pileup_corrected: no window is open"):
        eng.pileup_corrected()
    eng.close()


def test_driver_ins_slots(tmp_path):
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

    _, without = run("plain", "--device-dsoft", "--unique", "pair", "--pileup", "2")
    _, files = run("slots", "--device-dsoft", "--unique", "pair", "--pileup", "2", "--ins-slots", "2")
    assert sorted(files) == sorted(without)
    for f in without:
        assert (files[f] == without[f]) == (f != "darwin.cons.fa"), f
    # the same reads, parameters and selection through Engine, feeder by feeder, and the two models
    from pileup_model import pileup
    n_reads = len(rs.reads)
    per_thread = -(-n_reads // 2)
    eng, _, _ = engine_with(rs, np.zeros(0, dtype=engine.CAND_DTYPE), np.zeros(0, dtype=engine.CAND_DTYPE), slots=())
    eng.dsoft_build()
    recs, cigars = [], []
    for t in range(2):
        lo = min(n_reads, t * per_thread)
        nf, nr, _ = eng.dsoft_query(lo, min(n_reads, lo + per_thread) - lo)
        eng.candidates_run_mixed(nf + nr, nf)
        sel = eng.select_overlaps(n=nf + nr, mode="pair")
        r, p, o = eng.candidates_paths(sel=sel, rc_from=nf)
        recs.append(r)
        cigars += [ops_of(p, o, k) for k in range(len(r))]
    eng.close()
    records = np.concatenate(recs)
    _, _, table = pileup(rs.reads, _Rc(rs), records, cigars, (0, n_reads), 2)
    ins, corrected, read_at, seq, _ = pileup_ins(rs.reads, _Rc(rs), records, cigars, (0, n_reads), 2, 2)
    want, plain = [], []
    for i, name in enumerate(rs.names):
        t = table[i]
        head = ">%s called=%d changed=%d deleted=%d ins_flagged=%d" % (re.split(r"[^A-Za-z0-9_]+", name)[0], t["called"], t["changed"],
                                                                        t["deleted"], t["ins_flagged"])
        plain.append(head)
        want += [head + " inserted=%d" % corrected["inserted"][i], seq[read_at[i]:read_at[i + 1]].decode()]
    got = files["darwin.cons.fa"].decode().splitlines()
    assert len(got) == 2 * n_reads and got[0::2] == want[0::2]
    assert got == want
    assert without["darwin.cons.fa"].decode().splitlines()[0::2] == plain                  # without the flag: the line as it was
    assert int(corrected["inserted"].sum()) > 100
    for extra in (("--device-dsoft", "--ins-slots", "2"), ("--device-dsoft", "--pileup", "2", "--ins-slots", "0"),
                  ("--device-dsoft", "--pileup", "2", "--ins-slots", "5"), ("--device-dsoft", "--pileup", "2", "--ins-slots", "x")):
        out, left = run("refused_" + "_".join(extra).replace("--", ""), *extra, ok=False)
        assert "--ins-slots" in out.stderr and not left
