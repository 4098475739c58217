"""GPU suite for the filter of an overlap set (gact_hip_filter_overlaps, csrc/gact_filter.hpp): the reasons, the two kept lists
and the per-read table equal the model's (tests/filter_model.py) on the hand-made cases and on crafted host records at the wave
and block edges of the ballot and the write, beyond one block of block counts, with and without sel, on every side and with
every record on one read (no alignment runs); the same bytes on every run and on two slots; every refusal with the outputs
untouched, the capacity protocol, the empty inputs and the struct sizes; truth blocks B and P behind a run, where the false
hits and the decoy's records go and what is left is block A's graph; and the driver's --min-identity.  Every comparison is an
integer equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import filter_model as fm
import truth_checks as tc
from test_filter_model import P_MAX_DROP, kept_arcs
from test_truth_model import MIN_DEPTH, block, block_p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -4


@pytest.fixture(scope="module")
def eng():
    """an engine that aligns nothing: two slots, workspaces for one block"""
    from gact_amd import engine
    e = engine.Engine(n_slots=2, max_blocks=1)
    yield e
    e.close()


_MODEL = {}


def _random(n, **kw):
    """(records, sums, kwargs, the model's result) of a crafted random set, computed once"""
    key = (n, tuple(sorted(kw.items())))
    if key not in _MODEL:
        rec, sums, args = fm.random_case(n, **kw)
        _MODEL[key] = (rec, sums, args, fm.filter_overlaps(rec, sums, **args))
    return _MODEL[key]


def _device(e, rec, sums, kw, slot=0):
    """the engine's call for the model's arguments -> dict(why, kept_sel, kept_sums, reads)"""
    n_reads = kw.get("n_reads", 0)
    sel2, sums2, table, why = e.filter_overlaps(
        sums, records=rec, sel=kw.get("sel"), min_identity=kw.get("min_identity", 650), min_span=kw.get("min_span", 0),
        max_drop=kw.get("max_drop", 1000), sides=kw.get("sides", fm.BOTH), read_lens_or_n_reads=n_reads if n_reads else None,
        read_first=kw.get("read_first", 0), table=True, why=True, slot=slot)
    return dict(why=why, kept_sel=sel2, kept_sums=sums2, reads=table)


def _same(got, want, sums, what):
    bad = np.flatnonzero(got["why"] != want["why"])
    assert len(bad) == 0, "%s: why differs at %d chosen records, first at %d: device %d, model %d" % (
        what, len(bad), bad[0], got["why"][bad[0]], want["why"][bad[0]])
    assert got["kept_sel"].dtype == np.int32 and got["kept_sel"].tolist() == want["kept_sel"].tolist(), what
    assert got["kept_sums"].tobytes() == sums[want["kept_at"]].tobytes(), what
    for f in want["reads"].dtype.names:
        bad = np.flatnonzero(got["reads"][f] != want["reads"][f])
        assert len(bad) == 0, "%s: %s differs at read %d: device %s, model %s" % (what, f, bad[0], got["reads"][bad[0]], want["reads"][bad[0]])
    assert got["reads"].tobytes() == want["reads"].tobytes()


def _stats_agree(st, want, n_reads):
    why = want["why"]
    assert st["chosen"] == len(why) and st["kept"] == len(want["kept_at"]) and st["reads"] == n_reads and st["device_ms"] > 0
    assert st["counted"] == int(((why != fm.NOT_EMITTED) & (why != fm.EMPTY)).sum())
    for name, reason in (("not_emitted", fm.NOT_EMITTED), ("empty", fm.EMPTY), ("identity", fm.IDENTITY), ("span", fm.SPAN),
                         ("relative", fm.RELATIVE)):
        assert st[name] == int((why == reason).sum()), name
    assert st["scratch_bytes"] >= 16 * len(why) + 32 * n_reads


def test_struct_sizes_and_no_stats_before_a_call(tmp_path):
    """sizes as a C compiler sees include/gact_hip.h == what the ctypes / numpy side declares"""
    from gact_amd import engine
    (tmp_path / "abi.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\n"
        "int main(void) { printf(\"%zu %zu %zu %zu %zu\\n\", sizeof(gact_filter_params), sizeof(gact_read_filter), "
        "offsetof(gact_read_filter, eq_sum), sizeof(gact_filter_stats), offsetof(gact_filter_stats, chosen)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "abi")]).split()]
    assert got == [12, 32, 16, ctypes.sizeof(engine.FilterStats), engine.FilterStats.chosen.offset]
    assert ctypes.sizeof(engine.FilterParams) == 12 and engine.FILTER_READ_DTYPE.itemsize == 32
    assert engine.FILTER_READ_DTYPE.fields["eq_sum"][1] == 16
    assert (engine.FILTER_KEPT, engine.FILTER_NOT_EMITTED, engine.FILTER_EMPTY, engine.FILTER_IDENTITY, engine.FILTER_SPAN,
            engine.FILTER_RELATIVE) == (0, 1, 2, 3, 4, 5) == (fm.KEPT, fm.NOT_EMITTED, fm.EMPTY, fm.IDENTITY, fm.SPAN, fm.RELATIVE)
    assert engine.FILTER_DEFAULTS == dict(min_identity=650, min_span=0, max_drop=1000)
    fresh = engine.Engine(max_blocks=1)
    try:
        with pytest.raises(engine.GactHipError, match="filtered nothing"):
            fresh.last_filter_stats()
    finally:
        fresh.close()


@pytest.mark.parametrize("name", sorted(fm.hand_cases()))
def test_hand_made_cases_equal_the_model_and_what_is_written_beside_them(eng, name):
    rec, sums, kw, why, rows = fm.hand_cases()[name]
    want = fm.filter_overlaps(rec, sums, **kw)
    got = _device(eng, rec, sums, kw)
    assert got["why"].tolist() == why
    for x, row in rows.items():
        assert tuple(got["reads"][x].tolist()) == row
    _same(got, want, sums, name)
    _stats_agree(eng.last_filter_stats(), want, kw.get("n_reads", 0))


@pytest.mark.parametrize("n", fm.SIZES)
def test_crafted_sets_at_the_wave_and_block_edges(eng, n):
    for with_sel in (True, False):
        rec, sums, kw, want = _random(n, with_sel=with_sel)
        before = rec.tobytes() + sums.tobytes()
        _same(_device(eng, rec, sums, kw), want, sums, (n, with_sel))
        _stats_agree(eng.last_filter_stats(), want, kw["n_reads"])
        assert before == rec.tobytes() + sums.tobytes()
    # every chosen record kept, and none: the write's first and last lane of every wave
    rec, sums, kw, _ = _random(n, with_sel=False)
    rec = rec.copy()
    rec["emitted"] = 1
    for identity, span in ((0, 0), (1000, 0)):
        args = dict(kw, min_identity=identity, min_span=span, max_drop=1000)
        _same(_device(eng, rec, sums, args), fm.filter_overlaps(rec, sums, **args), sums, (n, identity))


@pytest.mark.parametrize("sides", [fm.REF, fm.QUERY, fm.BOTH])
def test_every_side(eng, sides):
    rec, sums, kw, want = _random(1025, sides=sides)
    _same(_device(eng, rec, sums, kw), want, sums, sides)
    assert (want["why"] == fm.RELATIVE).any() and (want["why"] == fm.KEPT).any()


def test_beyond_one_block_of_block_counts_and_many_records_on_one_read(eng):
    rec, sums, kw, want = _random(fm.BIG)
    assert (fm.BIG + 255) // 256 > 256
    _same(_device(eng, rec, sums, kw), want, sums, "big")
    _stats_agree(eng.last_filter_stats(), want, kw["n_reads"])
    # every record names read 0 on its query side: 5000 records on one table row
    rec, sums, kw, want = _random(5000, one_read=True, sides=fm.QUERY, n_reads=1)
    assert rec["query_id"].min() == rec["query_id"].max() and want["reads"]["n_records"][0] > 3000
    _same(_device(eng, rec, sums, kw), want, sums, "one read")
    rec, sums, kw, want = _random(5000, one_read=True, sides=fm.BOTH, n_reads=40)
    _same(_device(eng, rec, sums, kw), want, sums, "one read, both sides")


def test_the_same_bytes_on_every_run_and_on_both_slots(eng):
    big = _random(fm.BIG)
    small = _random(257)
    first = None
    for slot in (0, 0, 1):
        got = _device(eng, big[0], big[1], big[2], slot=slot)
        these = [got[k].tobytes() for k in ("why", "kept_sel", "kept_sums", "reads")]
        first = first or these
        assert these == first
    # a small set after a large one on the same scratch, and the large one again
    _same(_device(eng, small[0], small[1], small[2]), small[3], small[1], "small after big")
    _same(_device(eng, big[0], big[1], big[2]), big[3], big[1], "big again")
    # n < len(records): the first n only
    rec, sums, kw, _ = _random(1025, with_sel=False)
    got = eng.filter_overlaps(sums[:1000], n=1000, records=rec, min_identity=650, read_lens_or_n_reads=kw["n_reads"],
                              read_first=kw["read_first"], table=True, why=True)
    want = fm.filter_overlaps(rec[:1000], sums[:1000], min_identity=650, n_reads=kw["n_reads"], read_first=kw["read_first"])
    _same(dict(kept_sel=got[0], kept_sums=got[1], reads=got[2], why=got[3]), want, sums[:1000], "the first 1000")


def test_refusals_capacity_and_empty_inputs(eng):
    from gact_amd import engine
    L = eng.L
    rec, sums, kw, _, _ = fm.hand_cases()["relative_chain"]
    want = fm.filter_overlaps(rec, sums, **kw)
    why = np.full(4, -5, dtype=np.int32)
    kept_at, kept_sel = np.full(4, -5, dtype=np.int32), np.full(4, -5, dtype=np.int32)
    table = np.full(4, -5, dtype=engine.FILTER_READ_DTYPE)
    n_kept = ctypes.c_int32(-5)
    ptr = lambda a: a.ctypes.data if a is not None else None

    def call(slot=0, n=4, records=rec, n_sel=0, sel=None, sums=sums, sides=fm.BOTH, read_first=0, n_reads=4, min_identity=0, min_span=0,
             max_drop=50, cap=4, lists=True):
        params = engine.FilterParams(min_identity, min_span, max_drop)
        return L.gact_hip_filter_overlaps(eng.h, slot, n, ptr(records), n_sel, ptr(sel), ptr(sums), sides, read_first, n_reads,
                                          ctypes.byref(params), why.ctypes.data, kept_at.ctypes.data if lists else None,
                                          kept_sel.ctypes.data if lists else None, cap, ctypes.byref(n_kept), table.ctypes.data)

    untouched = lambda: all((a == -5).all() for a in (why, kept_at, kept_sel, table["n_records"], table["col_sum"]))
    # a refused call, on the host or by the device's check, leaves the figures of the call before it
    eng.filter_overlaps(sums, records=rec, min_identity=0, max_drop=50, read_lens_or_n_reads=4)
    figures = eng.last_filter_stats()
    assert figures["kept"] == 1 and figures["relative"] == 3
    with pytest.raises(engine.GactHipError, match="3 summaries for 4"):
        eng.filter_overlaps(sums[:3], records=rec)
    for bad, word in ((dict(sums=None), b"sums"), (dict(min_identity=-1), b"min_identity"), (dict(min_identity=1001), b"min_identity"),
                      (dict(min_span=-1), b"min_span"), (dict(max_drop=-1), b"max_drop"), (dict(max_drop=1001), b"max_drop"),
                      (dict(sides=0), b"sides"), (dict(sides=4), b"sides"), (dict(n=-1), b"n = -1"), (dict(n=(1 << 30) + 1), b"at most"),
                      (dict(sel=np.arange(4, dtype=np.int32), n_sel=-1), b"n_sel"),
                      (dict(sel=np.arange(4, dtype=np.int32), n_sel=(1 << 30) + 1), b"n_sel"),
                      (dict(sel=np.array([0, 1, 2, 4], dtype=np.int32), n_sel=4), b"sel"),
                      (dict(sel=np.array([0, -1, 2, 3], dtype=np.int32), n_sel=4), b"sel"), (dict(n_reads=-1), b"n_reads"),
                      (dict(n_reads=0), b"n_reads"), (dict(records=None, slot=1), b"no records"), (dict(cap=-1), b"cap")):
        n_kept.value = -5
        assert call(**bad) == EINVAL, bad
        assert word in L.gact_hip_last_error(), (bad, L.gact_hip_last_error())
        assert untouched() and n_kept.value == 0, bad
    # a counted record that names a read outside the window on a requested side: ERANGE; not counted, or on the other side: fine
    for bad in (dict(n_reads=3), dict(read_first=1), dict(read_first=-2, n_reads=5)):
        assert call(**bad) == ERANGE and b"outside" in L.gact_hip_last_error(), bad
        assert untouched() and n_kept.value == 0
    assert call(slot=2) < 0 and b"slot" in L.gact_hip_last_error() and untouched()
    assert eng.last_filter_stats() == figures
    with pytest.raises(engine.GactHipError, match="sides"):
        eng.filter_overlaps(sums, records=rec, sides="neither")
    far = rec.copy()
    far["ref_id"][1], far["emitted"][1] = 99, 0
    assert call(records=far) == 0 and why.tolist() == fm.filter_overlaps(far, sums, **kw)["why"].tolist()
    far["emitted"][1] = 1
    assert call(records=far) == ERANGE and call(records=far, sides=fm.QUERY, max_drop=1000) == 0
    # the capacity protocol: too little room refuses with *n_kept filled in and the lists untouched; no list at all needs no room
    rec8, sums8, kw8, want8 = _random(257, with_sel=False)
    k = len(want8["kept_at"])
    assert k > 4
    kept_at[:], kept_sel[:] = -5, -5
    big_why, big_table = np.zeros(257, dtype=np.int32), np.zeros(kw8["n_reads"], dtype=engine.FILTER_READ_DTYPE)
    params = engine.FilterParams(kw8["min_identity"], kw8["min_span"], kw8["max_drop"])
    args = (eng.h, 0, 257, rec8.ctypes.data, 0, None, sums8.ctypes.data, kw8["sides"], kw8["read_first"], kw8["n_reads"], ctypes.byref(params))
    assert L.gact_hip_filter_overlaps(*args, big_why.ctypes.data, kept_at.ctypes.data, kept_sel.ctypes.data, 4, ctypes.byref(n_kept),
                                      big_table.ctypes.data) == EINVAL
    assert b"room" in L.gact_hip_last_error() and n_kept.value == k and (kept_at == -5).all() and (kept_sel == -5).all()
    assert big_why.tolist() == want8["why"].tolist() and eng.last_filter_stats()["kept"] == k
    n_kept.value = -5
    assert L.gact_hip_filter_overlaps(*args, None, None, None, 0, ctypes.byref(n_kept), None) == 0 and n_kept.value == k
    room = np.full(k + 1, -5, dtype=np.int32)
    assert L.gact_hip_filter_overlaps(*args, None, room.ctypes.data, None, k, ctypes.byref(n_kept), None) == 0
    assert room[:k].tolist() == want8["kept_at"].tolist() and room[k] == -5
    # the whole call works after the refusals
    assert call() == 0 and n_kept.value == 1 and why.tolist() == want["why"].tolist() and table.tobytes() == want["reads"].tobytes()
    assert kept_at.tolist()[:1] == [0] and kept_sel.tolist()[:1] == [0]
    # n == 0 and an empty selection: 0 kept and a zeroed table, records or not, fresh slot or not; n_reads == 0 writes no table
    for empty in (dict(n=0), dict(n=0, records=None, slot=1), dict(sel=np.zeros(1, dtype=np.int32), n_sel=0)):
        table[:], why[:], n_kept.value = -5, -5, -5
        assert call(**empty) == 0 and n_kept.value == 0 and table.tobytes() == bytes(32 * 4) and (why == -5).all(), empty
    table[:] = -5
    assert call(n_reads=0, max_drop=1000) == 0 and n_kept.value == 4 and (table["n_records"] == -5).all()


# ---- behind a run: truth blocks A, B and P

def _graph_of(e, lens, sel, sums):
    cover = e.read_coverage(lens, sel=sel, sums=sums, min_depth=MIN_DEPTH)
    clip = np.stack([cover["span_begin"], cover["span_end"]], axis=1).astype(np.int32).reshape(-1)
    reads, arcs = e.overlap_graph(lens, sel=sel, sums=sums, clip=clip)
    arc_flags, _, _ = e.clean_graph(lens, reads, arcs, clip=clip)
    cleaned = arcs.copy()
    cleaned["flags"] = arc_flags
    utg = e.unitigs(lens, reads, cleaned, clip=clip, tip_reads=3)
    return dict(clip=clip, arcs=arcs, cleaned=cleaned, utg=utg)


def _n_beyond_the_slots_records_is_refused(e, n, sel, sums):
    """records == NULL with n one beyond the n records the slot holds: EINVAL, the outputs untouched, *n_kept 0, and the
    figures of the call before it left as they were"""
    from gact_amd import engine
    why, kept_at, kept_sel = (np.full(len(sel), -5, dtype=np.int32) for _ in range(3))
    table = np.full(4, -5, dtype=engine.FILTER_READ_DTYPE)
    n_kept = ctypes.c_int32(-5)
    params = engine.FilterParams(650, 0, 1000)
    before = e.last_filter_stats()

    def call(n_records):
        return e.L.gact_hip_filter_overlaps(e.h, 0, n_records, None, len(sel), sel.ctypes.data, sums.ctypes.data, fm.BOTH, 0, 4,
                                            ctypes.byref(params), why.ctypes.data, kept_at.ctypes.data, kept_sel.ctypes.data, len(sel),
                                            ctypes.byref(n_kept), table.ctypes.data)

    assert call(n + 1) == EINVAL and b"beyond" in e.L.gact_hip_last_error(), e.L.gact_hip_last_error()
    assert n_kept.value == 0 and all((a == -5).all() for a in (why, kept_at, kept_sel, table["n_records"], table["col_sum"]))
    assert e.last_filter_stats() == before
    # ... and with n the slot's own count the same call gets to the device: the window of four reads is too small for it
    assert call(n) == ERANGE and n_kept.value == 0 and (why == -5).all() and e.last_filter_stats() == before


def _run_block(name, filtered):
    """candidates_run_mixed -> select_overlaps("pair") -> candidates_summaries [-> filter_overlaps(650)] -> read_coverage ->
    overlap_graph -> clean_graph -> unitigs; the records are fetched last"""
    from path_cases import engine_with
    rs, cf, cr, law = block(name)
    e, n, nf = engine_with(rs, cf, cr)
    try:
        lens = np.array([len(r) for r in rs.reads], dtype=np.int32)
        e.candidates_run_mixed(n, nf)
        sel = e.select_overlaps(mode="pair")
        _, sums = e.candidates_summaries(sel=sel, rc_from=nf)
        out = dict(rs=rs, law=law, cands=np.concatenate([cf, cr]), nf=nf, lens=lens, sel=sel, sums=sums)
        if filtered:
            before = (e.last_run_stats(), e.last_select_stats(), e.last_summaries_stats())
            sel2, sums2, table, why = e.filter_overlaps(sums, sel=sel, min_identity=650, read_lens_or_n_reads=lens, table=True, why=True)
            assert (e.last_run_stats(), e.last_select_stats(), e.last_summaries_stats()) == before
            out.update(sel2=sel2, sums2=sums2, table=table, why=why, stats=e.last_filter_stats())
            _n_beyond_the_slots_records_is_refused(e, n, sel, sums)
            sel, sums = sel2, sums2
        out.update(_graph_of(e, lens, sel, sums), records=e.candidates_fetch(n).copy())
    finally:
        e.close()
    return out


def test_block_b_filtered_on_the_device_is_block_a():
    a, b = _run_block("A", False), _run_block("B", True)
    want = fm.filter_overlaps(b["records"], b["sums"], sel=b["sel"], min_identity=650, n_reads=b["rs"].n)
    _same(dict(why=b["why"], kept_sel=b["sel2"], kept_sums=b["sums2"], reads=b["table"]), want, b["sums"], "block B")
    hits, _ = tc.false_hits(b["rs"], b["cands"], b["nf"])
    selected_false = sum(i in hits for i in b["sel"].tolist() if b["records"]["emitted"][i])
    wrong = [tc.arcs(b["rs"], arcs, b["clip"], law=b["law"], count_only=True) for arcs in (b["arcs"], b["cleaned"])]
    print("block B on the device: %d selected, %d of them false; kept at 650: %d; dropped by identity %d; kept arcs %d, wrong %s; "
          "reads per unitig %s, block A's %s" % (len(b["sel"]), selected_false, len(b["sel2"]), b["stats"]["identity"],
                                                 int((b["arcs"]["flags"] == 0).sum()), wrong, b["utg"][0]["n_reads"].tolist(),
                                                 a["utg"][0]["n_reads"].tolist()))
    assert selected_false > 0 and not any(i in hits for i in b["sel2"].tolist()), "a false hit was kept"
    assert len(b["sel2"]) == int(b["records"]["emitted"][b["sel"]].sum()) - selected_false
    assert wrong == [0, 0]
    assert kept_arcs(b["arcs"]) == kept_arcs(a["arcs"]), "the filtered block B's kept arcs are not block A's device arcs"
    assert sorted(b["utg"][0]["n_reads"].tolist()) == sorted(a["utg"][0]["n_reads"].tolist())


def test_block_p_the_decoy_goes_on_the_device():
    from gact_amd import engine, synth
    p = block_p()
    rs, n, nf = p["rs"], len(p["cands"]), p["nf"]
    e = engine.Engine()
    try:
        e.upload_seqs(engine.SET_REF, p["seqs"])
        e.upload_seqs(engine.SET_QUERY, rs.reads)
        e.upload_seqs(engine.SET_QUERY_RC, [synth.revcomp(r) for r in rs.reads])
        e.candidates_upload(p["cands"])
        e.candidates_run_mixed(n, rc_from=nf, same_file=False)
        _, sums = e.candidates_summaries(n=n, rc_from=nf, same_file=False)
        got = {d: e.filter_overlaps(sums, min_identity=0, max_drop=d, sides="query", read_lens_or_n_reads=rs.n, table=True, why=True)
               for d in (P_MAX_DROP, 1000)}
        records = e.candidates_fetch(n).copy()
    finally:
        e.close()
    for d, (sel2, sums2, table, why) in got.items():
        want = fm.filter_overlaps(records, sums, min_identity=0, max_drop=d, sides=fm.QUERY, n_reads=rs.n)
        _same(dict(why=why, kept_sel=sel2, kept_sums=sums2, reads=table), want, sums, ("block P", d))
    on_decoy = records["ref_id"] == p["decoy"]
    why = got[P_MAX_DROP][3]
    under = got[P_MAX_DROP][2]["best_permille"][records["query_id"]] - fm.filter_overlaps(records, sums, min_identity=0)["ident"]
    print("block P on the device: %d records on the decoy, at least %d under their read's best; %d others, at most %d under" % (
        int(on_decoy.sum()), under[on_decoy].min(), int((~on_decoy).sum()), under[~on_decoy].max()))
    assert on_decoy.any() and (why[on_decoy] == fm.RELATIVE).all(), "a record on the decoy was kept"
    assert (why[~on_decoy] == fm.KEPT).all() and (got[1000][3] == fm.KEPT).all()
    assert not on_decoy[got[P_MAX_DROP][0]].any() and len(got[P_MAX_DROP][0]) == int((~on_decoy).sum())


# ---- the driver

def test_driver_min_identity(tmp_path):
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
        files = {p.name: p.read_bytes() for p in d.iterdir() if p.name.startswith("darwin.")}
        return files, out.stdout

    def lines(files, t, ext):
        return files["darwin.%d.%s" % (t, ext)].decode().splitlines()

    def identity(paf_line):
        f = paf_line.split("\t")
        return 1000 * int(f[9]) // int(f[10])

    plain, stdout = run("plain", "--paf")
    assert "Filter (thread" not in stdout
    for t in range(2):
        assert len(lines(plain, t, "paf")) == len(lines(plain, t, "out")) > 0          # a PAF line for every .out line
    every = sorted(identity(l) for t in range(2) for l in lines(plain, t, "paf"))
    p = every[len(every) // 2] + 1
    filtered, stdout = run("filtered", "--paf", "--min-identity", str(p))
    assert sorted(filtered) == sorted(plain) and stdout.count("Filter (thread") == 2
    gone = 0
    for t in range(2):
        passes = [identity(l) >= p for l in lines(plain, t, "paf")]
        for ext in ("paf", "out"):
            assert lines(filtered, t, ext) == [l for l, ok in zip(lines(plain, t, ext), passes) if ok], (t, ext)
        gone += passes.count(False)
    stay = len(every) - gone
    print("driver: %d lines, identity %d to %d; --min-identity %d: %d go, %d stay" % (len(every), every[0], every[-1], p, gone, stay))
    assert gone > 0 and stay > 0
    zero, _ = run("zero", "--paf", "--min-identity", "0")
    assert zero == plain
    # with a D: no kept line of a query lies more than D under that query's best kept line
    drop = 20
    relative, _ = run("relative", "--paf", "--min-identity", "0:0:%d" % drop)
    fewer = 0
    for t in range(2):
        all_lines, kept = lines(plain, t, "paf"), lines(relative, t, "paf")
        best = {}
        for l in all_lines:
            best[l.split("\t")[0]] = max(best.get(l.split("\t")[0], 0), identity(l))
        assert kept == [l for l in all_lines if best[l.split("\t")[0]] - identity(l) <= drop]
        best_kept = {}
        for l in kept:
            best_kept[l.split("\t")[0]] = max(best_kept.get(l.split("\t")[0], 0), identity(l))
        assert all(best_kept[l.split("\t")[0]] - identity(l) <= drop for l in kept)
        fewer += len(all_lines) - len(kept)
    print("driver: --min-identity 0:0:%d drops %d lines" % (drop, fewer))
    assert fewer > 0
    bad = subprocess.run([drv, "nowhere.fasta", "nowhere.fasta", "2", "--device-dsoft", "--min-identity", "650:"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--min-identity wants" in bad.stderr
