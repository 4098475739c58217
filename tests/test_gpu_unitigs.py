"""GPU suite for the unitigs (gact_hip_unitigs, csrc/gact_unitig.hpp): unitigs, layout, places, bases and the statistics' counts
equal the model's (tests/unitig_model.py) byte for byte -- on hand-made chains, tips and cycles with the read ids shuffled along
them (an in-place ranking update passes with ordered ids), on lengths past 2^31, on random graphs, three times over on two
slots, through the seq_cap protocol and the refusals, behind a real run of both strands, and through the driver's --unitigs.
No tolerance."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import graph_model
import unitig_model
from unitig_model import hand_made, unitigs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    """an engine that aligns nothing: two slots, workspaces for one block"""
    from gact_amd import engine
    e = engine.Engine(n_slots=2, max_blocks=1)
    yield e
    e.close()


_GRAPHS, _MODEL = {}, {}


def _graph_of(name):
    """(read_lens, reads, arcs, clip) of a named graph, made once"""
    if name not in _GRAPHS:
        if name == "chain6":
            rec, lens, kw = graph_model.crafted("tiling")
            g = graph_model.graph(rec, lens, **kw)
            _GRAPHS[name] = (lens, g["reads"], g["arcs"], None)
        elif name.startswith("random"):
            n, seed = name[6:].split("_")
            _GRAPHS[name] = unitig_model.random_graph(int(n), int(seed))
        elif name == "large":
            # three reads of 2^30 bases joined with len 2^30 - 2000: length, start and seq_at pass 2^31; and a second unitig behind
            lens = np.array([1 << 30, 1 << 30, 1 << 30, 7000], dtype=np.int32)
            arcs = unitig_model.make_arcs([(0, 2, (1 << 30) - 2000), (2, 5, (1 << 30) - 2000)])
            _GRAPHS[name] = (lens, unitig_model.plain_reads(4), arcs, None)
        else:
            _GRAPHS[name] = hand_made(name)
    return _GRAPHS[name]


def _case(name, tip_reads):
    """(the graph, the model's result), computed once"""
    if (name, tip_reads) not in _MODEL:
        lens, reads, arcs, clip = _graph_of(name)
        _MODEL[(name, tip_reads)] = unitigs(lens, reads, arcs, clip=clip, tip_reads=tip_reads)
    return _graph_of(name), _MODEL[(name, tip_reads)]


def _same(got, want, what):
    """got: (unitigs, layout, places[, bases]) of the device; want: the model's dict"""
    for name, g in zip(("unitigs", "layout", "places"), got):
        w = want[name]
        assert g.dtype == w.dtype and len(g) == len(w), "%s: %d %s, the model has %d" % (what, len(g), name, len(w))
        if g.tobytes() != w.tobytes():
            bad = int(np.flatnonzero(g != w)[0])
            raise AssertionError("%s: %s differ at %d: device %s, model %s" % (what, name, bad, g[bad], w[bad]))
    if len(got) > 3:
        assert got[3] == want["seq"].tobytes(), "%s: the bases differ" % (what,)


def _same_counts(st, want, what, n_reads):
    for name in unitig_model.COUNTS:
        assert st[name] == want["counts"][name], "%s: statistics' %s: device %s, model %s" % (what, name, st[name], want["counts"][name])
    rounds = max(1, int(2 * n_reads - 1).bit_length())
    assert st["device_ms"] > 0 and st["rank_launches"] == 3 * rounds and st["scratch_bytes"] >= 250 * n_reads


def _check(eng, name, tip_reads, slot=0):
    (lens, reads, arcs, clip), want = _case(name, tip_reads)
    held = [lens, reads, arcs] + ([clip] if clip is not None else [])
    before = [a.tobytes() for a in held]
    _same(eng.unitigs(lens, reads, arcs, clip=clip, tip_reads=tip_reads, slot=slot), want, (name, tip_reads, slot))
    _same_counts(eng.last_unitig_stats(slot), want, (name, tip_reads), len(lens))
    assert before == [a.tobytes() for a in held]
    return want


@pytest.mark.parametrize("tip_reads", [0, 3])
@pytest.mark.parametrize("name", ["chain6", "chain1", "chain64", "chain65", "chain257", "chain5000", "minus64"])
def test_chains_with_shuffled_ids(eng, name, tip_reads):
    want = _check(eng, name, tip_reads)
    n = len(_graph_of(name)[0])
    if n > 3:
        u = want["unitigs"]
        assert len(u) == 1 and u["n_reads"][0] == n and not u["circular"][0]
        if name != "chain6":                              # neighbours along the chain sit in different waves and blocks
            assert np.abs(np.diff(want["layout"]["vertex"])).max() > min(n, 512) // 2
    if name == "minus64":
        assert (want["places"]["orient"] == 0).all() and (_graph_of(name)[2]["u"][::2] & 1).any()    # emitted: the complement


@pytest.mark.parametrize("tip_reads", [0, 3])
@pytest.mark.parametrize("name", ["tiling128", "tiling129"])
def test_tilings_that_end_with_the_scans_chunk_and_one_read_behind_it(eng, name, tip_reads):
    """256 vertices: the last full chunk of unitig_scan_kernel; 258: the first carry, read by the head of read 128's unitig"""
    want = _check(eng, name, tip_reads)
    n = len(_graph_of(name)[0])
    u = want["unitigs"]
    assert len(u) == (25 if tip_reads else n - 102) and want["counts"]["cut"] == (n - 125 if tip_reads else 0)
    if (n, tip_reads) == (129, 0):
        assert u["first"][-1] == 256 and u["layout_at"][-1] == 128 and u["seq_at"][-1] == u["length"][:-1].sum() > 0


@pytest.mark.parametrize("tip_reads", [0, 1, 3])
@pytest.mark.parametrize("name", ["fork", "two_tips", "tip_lengths", "reverse_tip", "isolated", "no_arcs", "chain1"])
def test_tips(eng, name, tip_reads):
    want = _check(eng, name, tip_reads)
    cut = np.flatnonzero(want["places"]["state"] == unitig_model.TIP).tolist()
    expect = {("fork", 3): [10, 11], ("two_tips", 1): [5, 6], ("two_tips", 3): [5, 6], ("tip_lengths", 1): [23],
              ("tip_lengths", 3): [16, 17, 18, 23], ("reverse_tip", 3): [8, 9], ("isolated", 3): [0, 1, 2], ("no_arcs", 1): [0, 1, 2],
              ("no_arcs", 3): [0, 1, 2], ("chain1", 1): [0], ("chain1", 3): [0]}
    assert cut == expect.get((name, tip_reads), [])
    if (name, tip_reads) == ("fork", 3):
        assert want["unitigs"]["n_reads"].tolist() == [10]             # the two halves merged through the junction


def test_a_tip_of_tip_reads_plus_one_stays(eng):
    assert np.flatnonzero(_check(eng, "tip_lengths", 4)["places"]["state"] == unitig_model.TIP).tolist() == [0, 1, 2, 3] + list(range(16, 24))
    assert np.flatnonzero(_check(eng, "tip_lengths", 2)["places"]["state"] == unitig_model.TIP).tolist() == [23]


@pytest.mark.parametrize("tip_reads", [0, 3])
@pytest.mark.parametrize("name", ["cycle2", "cycle3", "cycle300", "cycle_minus", "cycle_beside", "cycle_tip"])
def test_cycles(eng, name, tip_reads):
    want = _check(eng, name, tip_reads)
    u = want["unitigs"]
    if name == "cycle_tip":
        assert u["circular"].tolist() == ([1] if tip_reads == 3 else [0, 0])
    else:
        assert u["circular"].sum() == 1 and want["counts"]["circular"] == 1
        c = u[u["circular"] == 1][0]
        assert c["first"] % 2 == 0 and c["first"] == want["layout"]["vertex"][int(c["layout_at"]):int(c["layout_at"] + c["n_reads"])].min() & ~1
    if name == "cycle_minus":
        assert want["layout"]["vertex"].tolist() == [0, 9, 3, 6, 5]


def test_lengths_past_two_to_the_31(eng):
    want = _check(eng, "large", 0)
    u, lay = want["unitigs"], want["layout"]
    assert u["length"][0] == 3 * (1 << 30) - 4000 > 1 << 31 and lay["start"][2] == (1 << 31) - 4000 and u["seq_at"][1] == u["length"][0]
    assert want["counts"]["longest_bases"] == u["length"][0]


@pytest.mark.parametrize("tip_reads", [0, 3])
def test_skipped_inputs(eng, tip_reads):
    want = _check(eng, "skipped", tip_reads)
    assert want["places"]["state"].tolist() == [0] * 6 + [unitig_model.CONTAINED, unitig_model.EMPTY]
    assert (_graph_of("skipped")[2]["flags"] != 0).sum() == 4


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n", [400, 3000])
def test_random_graphs(eng, n, seed):
    for tip_reads in (0, 3):
        want = _check(eng, "random%d_%d" % (n, seed), tip_reads)
    c = want["counts"]
    assert c["cut"] > 0 and c["links"] > 0 and c["unitigs"] > 10 and c["contained"] > 0 and c["longest_reads"] > 10


def test_the_result_is_the_same_on_every_run_and_on_every_slot(eng):
    for slot in (0, 0, 1):
        _check(eng, "random3000_1", 3, slot=slot)
        _check(eng, "cycle_beside", 3, slot=slot)
    # a small graph after a large one on the same scratch, and the large one again
    _check(eng, "chain5000", 0)
    _check(eng, "cycle3", 0)
    _check(eng, "fork", 3)
    _check(eng, "chain5000", 0)


# ---- bases

@pytest.fixture(scope="module")
def based(eng):
    """100 reads of the random-graph kind with bytes of their own -- a few N, lower case, one foreign byte -- as SET_REF"""
    from gact_amd import engine
    lens, reads, arcs, clip = unitig_model.random_graph(100, 7)
    rng = np.random.default_rng(20261023)
    seqs = [np.frombuffer(b"ACGTACGTACGTACGTacgtNn", dtype=np.uint8)[rng.integers(0, 22, int(ln))] for ln in lens]
    res0 = unitigs(lens, reads, arcs, clip=clip, tip_reads=0)
    rc = [int(e["vertex"]) >> 1 for e in res0["layout"] if e["vertex"] & 1 and e["take"] > 50]
    assert rc
    seqs[rc[0]] = seqs[rc[0]].copy()
    seqs[rc[0]][int(clip[2 * rc[0] + 1]) - 20] = ord("*")                   # inside the take of a reverse entry
    eng.upload_seqs(engine.SET_REF, seqs)
    return lens, reads, arcs, clip, seqs


@pytest.mark.parametrize("tip_reads", [0, 3])
def test_bases_equal_the_model(eng, based, tip_reads):
    lens, reads, arcs, clip, seqs = based
    want = unitigs(lens, reads, arcs, clip=clip, tip_reads=tip_reads, seqs=seqs)
    assert ((clip[0::2] > 0) | (clip[1::2] < lens)).any() and (want["layout"]["vertex"] & 1).any() and len(want["unitigs"]) > 1
    if tip_reads == 0:
        assert b"N" in want["seq"].tobytes() and b"n" in want["seq"].tobytes() and b"*" not in want["seq"].tobytes()
    for slot in (0, 1):
        _same(eng.unitigs(lens, reads, arcs, clip=clip, tip_reads=tip_reads, seq=True, slot=slot), want, ("bases", tip_reads, slot))
    _same_counts(eng.last_unitig_stats(1), want, "bases", len(lens))


def test_seq_cap_protocol(eng, based):
    from gact_amd import engine
    lens, reads, arcs, clip, seqs = based
    want = unitigs(lens, reads, arcs, clip=clip, tip_reads=3, seqs=seqs)
    total = len(want["seq"])
    n = len(lens)
    utg = np.zeros(n, dtype=engine.UNITIG_DTYPE)
    layout = np.zeros(n, dtype=engine.UNITIG_ENTRY_DTYPE)
    places = np.zeros(n, dtype=engine.UNITIG_PLACE_DTYPE)
    bases = np.full(total, 7, dtype=np.uint8)
    par = engine.UnitigParams(3)

    def call(seq_ptr, cap):
        count, seq_len = C.c_int32(-1), C.c_int64(-1)
        rc = eng.L.gact_hip_unitigs(eng.h, 0, n, lens.ctypes.data, clip.ctypes.data, reads.ctypes.data, len(arcs), arcs.ctypes.data,
                                    C.byref(par), utg.ctypes.data, C.byref(count), layout.ctypes.data, places.ctypes.data, seq_ptr, cap,
                                    C.byref(seq_len))
        return rc, count.value, seq_len.value

    for seq_ptr, cap, rc in ((bases.ctypes.data, total - 1, -1), (bases.ctypes.data, 0, -1), (None, 1000, 0)):
        utg[:], layout[:], places[:] = 0, 0, 0
        assert call(seq_ptr, cap) == (rc, len(want["unitigs"]), total)
        assert rc == 0 or b"room" in eng.L.gact_hip_last_error()
        assert (bases == 7).all()
        _same((utg[:len(want["unitigs"])], layout[:len(want["layout"])], places), want, "a call without room")
        _same_counts(eng.last_unitig_stats(), want, "a call without room", n)
    assert call(bases.ctypes.data, total) == (0, len(want["unitigs"]), total) and bases.tobytes() == want["seq"].tobytes()
    # the binding retries once: a cap of half the reads' bases is too small for whole reads that do not overlap
    eng.upload_seqs(engine.SET_REF, seqs[:3])
    got = eng.unitigs(lens[:3], unitig_model.plain_reads(3), arcs[:0], tip_reads=0, seq=True)
    assert got[3] == b"".join(s.tobytes() for s in seqs[:3]) and len(got[0]) == 3


# ---- behind a real run

@pytest.fixture(scope="module")
def small_run():
    """ecoli10x_small, both strands, run on slot 0: pair selection -> summaries -> coverage clip -> graph -> unitigs with bases,
    all BEFORE the records are fetched"""
    from conftest import workload_block
    from path_cases import engine_with
    blk = workload_block("ecoli10x_small")
    e, n, nf = engine_with(blk.rs, blk.cf, blk.cr, n_slots=2)
    lens = np.array([len(r) for r in blk.rs.reads], dtype=np.int32)
    e.candidates_run_mixed(n, nf)
    sel = e.select_overlaps(mode="pair")
    _, sums = e.candidates_summaries(sel=sel, rc_from=nf)
    cover = e.read_coverage(lens, sel=sel, sums=sums, min_depth=3)
    clip = np.stack([cover["span_begin"], cover["span_end"]], axis=1).astype(np.int32)
    reads, arcs = e.overlap_graph(lens, sel=sel, sums=sums, clip=clip)
    others = (e.last_run_stats(), e.last_summaries_stats(), e.last_select_stats(), e.last_cover_stats(), e.last_graph_stats())
    got = {k: e.unitigs(lens, reads, arcs, clip=clip, tip_reads=k, seq=True) for k in (0, 3)}
    stats = e.last_unitig_stats()
    after = (e.last_run_stats(), e.last_summaries_stats(), e.last_select_stats(), e.last_cover_stats(), e.last_graph_stats())
    records = e.candidates_fetch(n).copy()
    yield dict(eng=e, n=n, nf=nf, lens=lens, sel=sel, sums=sums, clip=clip, reads=reads, arcs=arcs, got=got, stats=stats, others=others,
               after=after, records=records, seqs=blk.rs.reads)
    e.close()


def test_behind_a_run_of_both_strands(small_run):
    r = small_run
    lens, clip = r["lens"], r["clip"]
    g = graph_model.graph(r["records"], lens, sel=r["sel"], sums=r["sums"], clip=clip)
    assert g["reads"].tobytes() == r["reads"].tobytes() and g["arcs"].tobytes() == r["arcs"].tobytes()
    for k in (0, 3):
        want = unitigs(lens, g["reads"], g["arcs"], clip=clip, tip_reads=k, seqs=r["seqs"])
        _same(r["got"][k], want, "ecoli10x_small, tip_reads %d" % k)
        print(k, want["counts"])
    _same_counts(r["stats"], want, "ecoli10x_small", len(lens))
    # not trivially so, as far as the model says: a unitig of two reads or more, and a read spelled from its other strand
    assert want["unitigs"]["n_reads"].max() >= 2 and (want["layout"]["vertex"] & 1).any() and len(want["seq"]) > 0
    # the slot's records, its run statistics and the other calls' statistics are what they were
    e = r["eng"]
    assert r["after"] == r["others"]
    assert (e.last_run_stats(), e.last_summaries_stats(), e.last_select_stats(), e.last_cover_stats(), e.last_graph_stats()) == r["others"]
    _same(e.unitigs(lens, r["reads"], r["arcs"], clip=clip, tip_reads=3, seq=True, slot=1), want, "on the other slot, after the fetch")
    assert e.candidates_fetch(r["n"]).tobytes() == r["records"].tobytes()
    assert e.select_overlaps(mode="pair").tolist() == r["sel"].tolist()


def test_refusals(eng):
    from gact_amd import engine
    L = eng.L
    lens, reads, arcs, clip = _graph_of("fork")
    n = len(lens)
    utg = np.full(n, -5, dtype=engine.UNITIG_DTYPE)
    layout = np.full(n, -5, dtype=engine.UNITIG_ENTRY_DTYPE)
    places = np.full(n, -5, dtype=engine.UNITIG_PLACE_DTYPE)
    bases = np.full(int(lens.sum()), 7, dtype=np.uint8)
    count, seq_len = C.c_int32(-9), C.c_int64(-9)
    whole = np.stack([np.zeros_like(lens), lens], axis=1).astype(np.int32)
    ptr = lambda a: a.ctypes.data if a is not None else None

    def call(slot=0, n_reads=n, read_lens=lens, clip=None, reads=reads, n_arcs=None, arcs=arcs, tip_reads=3, utg=utg, count=count,
             layout=layout, places=places, seq=None, cap=0):
        par = engine.UnitigParams(tip_reads)
        return L.gact_hip_unitigs(eng.h, slot, n_reads, ptr(read_lens), ptr(clip), ptr(reads), len(arcs) if n_arcs is None else n_arcs,
                                  ptr(arcs), C.byref(par), ptr(utg), C.byref(count) if count is not None else None, ptr(layout),
                                  ptr(places), ptr(seq), cap, C.byref(seq_len))

    def clipped(i, b, end):
        c = whole.copy()
        c[i] = (b, end)
        return c.reshape(-1)

    def changed(field, k, value):
        a = arcs.copy()
        a[field][k] = value
        return a

    contained = reads.copy()
    contained["contained_by"][5] = 3
    neg = lens.copy()
    neg[1] = -1
    eng.upload_seqs(engine.SET_REF, [np.full(5000, ord("A"), dtype=np.uint8)] * n)
    long_arc = changed("len", len(arcs) - 1, 5001)
    cases = [(dict(read_lens=None), b"NULL"), (dict(reads=None), b"NULL"), (dict(count=None), b"NULL"), (dict(places=None), b"NULL"),
             (dict(utg=None), b"NULL"), (dict(layout=None), b"NULL"),
             (dict(n_reads=-1), b"n_reads = -1"), (dict(n_reads=(1 << 30) + 1), b"n_reads"), (dict(n_arcs=-1), b"n_arcs = -1"),
             (dict(n_arcs=(1 << 29) + 1), b"n_arcs"), (dict(tip_reads=-1), b"tip_reads"), (dict(read_lens=neg), b"negative"),
             (dict(clip=clipped(2, -1, 5000)), b"clip"), (dict(clip=clipped(2, 3000, 2999)), b"clip"), (dict(clip=clipped(5, 0, 5001)), b"clip"),
             (dict(arcs=changed("v", 0, 2 * n)), b"outside"), (dict(arcs=changed("v", 0, -1)), b"outside"),
             (dict(arcs=changed("u", len(arcs) - 1, 2 * n)), b"outside"),
             (dict(arcs=changed("v", 0, int(arcs["u"][0]) ^ 1)), b"one read"), (dict(arcs=changed("len", 0, 0)), b"len < 1"),
             (dict(arcs=arcs[::-1].copy()), b"ascending"), (dict(arcs=np.concatenate([arcs[:1], arcs])), b"ascending"),
             (dict(reads=contained), b"not live"), (dict(clip=clipped(5, 2000, 2000)), b"not live"),
             (dict(arcs=arcs[1:].copy()), b"complement"), (dict(arcs=changed("flags", 0, 1)), b"complement"),
             (dict(seq=bases, cap=len(bases), arcs=long_arc), b"longer"),
             (dict(seq=bases, cap=len(bases), n_reads=n - 2, read_lens=lens[:n - 2].copy(), reads=reads[:n - 2].copy(), arcs=arcs[:0]), b"sequences"),
             (dict(seq=bases, cap=len(bases), read_lens=np.full(n, 4999, dtype=np.int32)), b"length")]
    for bad, word in cases:
        assert call(**bad) == -1, bad
        assert word in L.gact_hip_last_error(), (bad, L.gact_hip_last_error())
    assert call(slot=2) < 0 and b"slot" in L.gact_hip_last_error()
    fresh = engine.Engine(max_blocks=1)
    try:
        with pytest.raises(engine.GactHipError, match="no unitigs"):
            fresh.last_unitig_stats()
        # bases without a read set
        rc = fresh.L.gact_hip_unitigs(fresh.h, 0, n, ptr(lens), None, ptr(reads), len(arcs), ptr(arcs), None, ptr(utg), C.byref(count),
                                      ptr(layout), ptr(places), ptr(bases), len(bases), C.byref(seq_len))
        assert rc == -1 and b"not uploaded" in fresh.L.gact_hip_last_error()
    finally:
        fresh.close()
    assert (utg["first"] == -5).all() and (layout["take"] == -5).all() and (places["state"] == -5).all() and (bases == 7).all()
    assert count.value == -9 and seq_len.value == -9
    # the call works after the refusals: with bases, a clip of whole reads, and the long arc when no bases are asked for
    want = unitigs(lens, reads, arcs, tip_reads=3, seqs=[np.full(5000, ord("A"), dtype=np.uint8)] * n)
    assert call(seq=bases, cap=len(bases), clip=whole.reshape(-1)) == 0 and count.value == 1 and seq_len.value == len(want["seq"])
    _same((utg[:1], layout[:10], places), want, "after the refusals")
    assert bases[:seq_len.value].tobytes() == want["seq"].tobytes()
    assert call(arcs=long_arc) == 0
    _same((utg[:count.value], layout[:10], places), unitigs(lens, reads, long_arc, tip_reads=3), "a long arc without bases")
    # n_reads == 0 returns 0 and writes nothing but the two counts
    utg[:], layout[:], places[:] = -5, -5, -5
    assert call(n_reads=0, arcs=arcs[:0]) == 0 and count.value == 0 and seq_len.value == 0
    assert (utg["first"] == -5).all() and (places["state"] == -5).all()


# ---- the driver

def _utg_gfa(path):
    """-> (segments [(name, bases)], entries per segment [[(start, read, b, e, sign, take)]], links [(utg, sign, utg, sign, overlap)])"""
    lines = open(path).read().splitlines()
    assert lines[0] == "H\tVN:Z:1.0"
    seg, entries, links = [], [], []
    for line in lines[1:]:
        f = line.split("\t")
        if f[0] == "S":
            assert len(f) == 4 and f[3] == "LN:i:%d" % len(f[2]) and not links, line
            seg.append((f[1], f[2]))
            entries.append([])
        elif f[0] == "a":
            m = re.fullmatch(r"a\t(\w+)\t(\d+)\t(\w+):(\d+)-(\d+)\t([+-])\t(\d+)", line)
            assert m and m.group(1) == seg[-1][0] and not links, line
            entries[-1].append((int(m.group(2)), m.group(3), int(m.group(4)), int(m.group(5)), m.group(6), int(m.group(7))))
        else:
            m = re.fullmatch(r"L\t(\w+)\t([+-])\t(\w+)\t([+-])\t(\d+)M", line)
            assert m, line
            links.append((m.group(1), m.group(2), m.group(3), m.group(4), int(m.group(5))))
    return seg, entries, links


def test_driver_unitigs(tmp_path):
    from gact_amd import engine, workload
    from conftest import workload_block
    rs = workload_block("tiny").rs
    rs.write_fasta(str(tmp_path / "reads.fasta"))
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()
    ids = {name: i for i, name in enumerate(rs.names)}
    lens = np.array([len(r) for r in rs.reads], dtype=np.int32)
    extra = ("--unique", "pair", "--coverage", "3", "--gfa")

    def run(name, *more):
        d = tmp_path / name
        d.mkdir()
        for f in ("reads.fasta", "params.cfg"):
            os.symlink(tmp_path / f, d / f)
        out = subprocess.run([drv, "reads.fasta", "reads.fasta", "2", "--device-dsoft"] + list(extra + more), capture_output=True,
                             text=True, cwd=d, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        return {p.name: p.read_bytes() for p in d.iterdir() if p.name.startswith("darwin.")}

    without = run("gfa")
    # the graph's inputs as tests/test_gpu_graph.py reconstructs them: the records of the .out files, the clip of the table
    pat = re.compile(r"ref_id: (\w+), query_id: (\w+), ab: (-?\d+), ae: (-?\d+), bb: (-?\d+), be: (-?\d+), score: (-?\d+), comp: (\d)")
    rows = []
    for t in range(2):
        for line in without["darwin.%d.out" % t].decode().splitlines():
            m = pat.fullmatch(line)
            rows.append((ids[m.group(1)], ids[m.group(2)], int(m.group(8))) + tuple(int(m.group(k)) for k in (3, 4, 5, 6, 7)) + (1,))
    tsv = [line.split("\t") for line in without["darwin.cover.tsv"].decode().splitlines()]
    clip = np.array([(int(f[6]), int(f[7])) for f in tsv], dtype=np.int32).reshape(-1)
    g = graph_model.graph(graph_model.records_of(rows), lens, clip=clip)
    for k in (0, 3):
        files = run("utg%d" % k, "--unitigs", str(k))
        assert sorted(files) == sorted(list(without) + ["darwin.utg.gfa"])
        for f in without:
            assert files[f] == without[f], f
        want = unitigs(lens, g["reads"], g["arcs"], clip=clip, tip_reads=k, seqs=rs.reads)
        seg, entries, links = _utg_gfa(tmp_path / ("utg%d" % k) / "darwin.utg.gfa")
        names = ["utg%06d%s" % (j + 1, "c" if u["circular"] else "l") for j, u in enumerate(want["unitigs"])]
        assert seg == [(names[j], want["seq"][int(u["seq_at"]):int(u["seq_at"] + u["length"])].tobytes().decode())
                       for j, u in enumerate(want["unitigs"])]
        for j, u in enumerate(want["unitigs"]):
            lay = want["layout"][int(u["layout_at"]):int(u["layout_at"] + u["n_reads"])]
            assert entries[j] == [(int(e["start"]), rs.names[e["vertex"] >> 1], int(clip[2 * (e["vertex"] >> 1)]),
                                   int(clip[2 * (e["vertex"] >> 1) + 1]), "+-"[e["vertex"] & 1], int(e["take"])) for e in lay]
        assert links == [(names[a], sa, names[b], sb, ov) for a, sa, b, sb, ov in want["links"]]
        print("--unitigs %d: %s" % (k, want["counts"]))
        # (the tiny workload gives chains: were it not so, ecoli10x_small would have to stand in here)
        assert want["unitigs"]["n_reads"].max() >= 2
    # refused without --gfa, before any device is opened
    out = subprocess.run([drv, "reads.fasta", "reads.fasta", "1", "--device-dsoft", "--unitigs", "3"], capture_output=True, text=True,
                         cwd=tmp_path, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert out.returncode == 1 and "--unitigs" in out.stderr and "--gfa" in out.stderr, (out.stdout, out.stderr)
