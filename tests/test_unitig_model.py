"""CPU suite for the unitigs: the model (tests/unitig_model.py) against truth it does not compute itself -- a genome the reads were
cut from, the simulator's own coordinates -- its invariants on every hand-made and random graph, what each hand-made graph is
there to show, the new structs as a C compiler sees them, the library's exports, and the driver's refusal of --unitigs without
--gfa, which touches no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import graph_model
import unitig_model
from graph_model import graph
from unitig_model import CONTAINED, EMPTY, PLACED, TIP, hand_made, unitigs, vertex_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _revcomp(a):
    return unitig_model.oriented(a, 0, len(a), 1)


@pytest.mark.parametrize("clipped", [False, True])
def test_bases_against_the_genome_the_reads_were_cut_from(clipped):
    """200 reads, exact substrings of a random genome on mixed strands; tip_reads = 0.  Every unitig spells the genome from its
    first read's begin to its last read's end, or the reverse complement of that.  Once without a clip and once with the clip of
    whole reads written out (the graph clamps each end of an overlap to the clips on its own, so with a clip that cuts bases an
    arc's len is no longer the distance of two genome positions, and no such truth exists)"""
    rng = np.random.default_rng(20261021 + clipped)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 150000)]
    layout = [(int(rng.integers(0, 150000 - 7000)), int(rng.integers(3000, 7000)), int(rng.integers(0, 2))) for _ in range(200)]
    seqs = [genome[s:s + ln] if sd == 0 else _revcomp(genome[s:s + ln]) for s, ln, sd in layout]
    lens = np.array([ln for _, ln, _ in layout], dtype=np.int32)
    clip = None
    if clipped:
        clip = np.array([(0, ln) for _, ln, _ in layout], dtype=np.int32).reshape(-1)
    g = graph(graph_model.records_of(graph_model.layout_records(layout)), lens, clip=clip)
    res = unitigs(lens, g["reads"], g["arcs"], clip=clip, tip_reads=0, seqs=seqs)

    def span(i):
        """what read i covers of the genome after its clip"""
        s, ln, sd = layout[i]
        cb, ce = (0, ln) if clip is None else (int(clip[2 * i]), int(clip[2 * i + 1]))
        return (s + cb, s + ce) if sd == 0 else (s + ln - ce, s + ln - cb)

    live = [i for i in range(200) if g["reads"]["contained_by"][i] < 0]
    assert sorted(v >> 1 for vs in vertex_lists(res) for v in vs) == live and len(live) > 20
    assert [i for i in range(200) if res["places"]["state"][i] == PLACED] == live
    several = 0
    for u, vs in zip(res["unitigs"], vertex_lists(res)):
        first, last = span(vs[0] >> 1), span(vs[-1] >> 1)
        lo, hi = min(first[0], last[0]), max(first[1], last[1])
        assert u["length"] == hi - lo and not u["circular"]
        got = res["seq"][int(u["seq_at"]):int(u["seq_at"] + u["length"])]
        forward = (layout[vs[0] >> 1][2] == 0) == (vs[0] & 1 == 0)          # the first vertex reads along the genome
        assert len(vs) == 1 or (first[0] == lo) == forward
        want = genome[lo:hi] if forward else _revcomp(genome[lo:hi])
        assert got.tobytes() == want.tobytes()
        several += len(vs) > 1
    assert several >= 1 and len(res["seq"]) == int(res["unitigs"]["length"].sum())
    print("%d live reads in %d unitigs, the longest of %d reads" % (len(live), len(res["unitigs"]), res["counts"]["longest_reads"]))


@pytest.mark.parametrize("coverage,seed", [(8, 1), (12, 2), (20, 3)])
def test_one_unitig_on_the_simulators_truth(coverage, seed):
    """the exact overlaps of tests/test_graph_model.py's truth test (the simulator's own coordinates, layout only): the kept arcs
    are one path over the reads that are not contained, so there is exactly one unitig that holds all of them in genome order,
    with tip_reads = 0 and with 3"""
    from gact_amd import synth
    rs = synth.simulate_reads(60000, coverage=coverage, seed=seed, mean_len=6000, sd_len=1500, min_len=1500, max_len=12000)
    lens = np.array([len(r) for r in rs.reads], dtype=np.int32)

    def coords(i, lo, hi, flipped):
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
            flipped = bool(rs.strand[t])
            ab, ae = coords(t, lo, hi, flipped)
            bb, be = coords(q, lo, hi, flipped)
            rows.append((t, q, int(rs.strand[t] != rs.strand[q]), ab, ae, bb, be, hi - lo, 1))
    g = graph(graph_model.records_of(rows), lens, params=dict(min_ovlp=2000))
    alive = [i for i in np.argsort(rs.start, kind="stable").tolist() if g["reads"]["contained_by"][i] < 0]
    for tip_reads in (0, 3):
        res = unitigs(lens, g["reads"], g["arcs"], tip_reads=tip_reads)
        assert len(res["unitigs"]) == 1 and res["counts"]["cut"] == 0 and res["counts"]["links"] == 0
        order = [v >> 1 for v in vertex_lists(res)[0]]
        assert order in (alive, alive[::-1])
        u = res["unitigs"][0]
        assert (u["n_reads"], u["circular"], u["layout_at"], u["seq_at"]) == (len(alive), 0, 0, 0)
        # every vertex reads along the genome, or every one against it
        along = set((v & 1) == int(rs.strand[v >> 1]) for v in vertex_lists(res)[0])
        assert len(along) == 1
    print("%d reads, %d not contained, one unitig of %d bases" % (rs.n, len(alive), u["length"]))


# ---- the invariants, on every graph

_GRAPHS = {}


def _graph_of(name):
    if name not in _GRAPHS:
        if name.startswith("random"):
            _GRAPHS[name] = unitig_model.random_graph(150, int(name[6:]))
        elif name.startswith("crafted:"):
            rec, lens, kw = graph_model.crafted(name[8:])
            g = graph(rec, lens, **kw)
            _GRAPHS[name] = (lens, g["reads"], g["arcs"], kw.get("clip"))
        else:
            _GRAPHS[name] = hand_made(name)
    return _GRAPHS[name]


ALL_GRAPHS = tuple(unitig_model.HAND_MADE) + ("random1", "random2", "random3") + \
    tuple("crafted:" + p for p in ("tiling", "contained", "clip", "both_strands", "hub", "many_reads", "random"))


def _complemented(lens, reads, arcs, clip):
    """every read stored the other way round: vertex x becomes x ^ 1, the clip is counted from the other end"""
    out = arcs.copy()
    out["u"] ^= 1
    out["v"] ^= 1
    out = out[np.lexsort((out["v"], out["len"], out["u"]))]
    if clip is not None:
        c = np.asarray(clip).reshape(-1, 2)
        clip = np.stack([lens - c[:, 1], lens - c[:, 0]], axis=1).astype(np.int32).reshape(-1)
    return lens, reads, out, clip


def _canonical(vs, circular):
    """a vertex list up to complement (and, for a cycle, rotation)"""
    forms = [list(vs), [v ^ 1 for v in reversed(vs)]]
    if circular:
        forms = [f[k:] + f[:k] for f in forms for k in range(len(f))]
    return tuple(min(forms))


@pytest.mark.parametrize("tip_reads", [0, 1, 3])
@pytest.mark.parametrize("name", ALL_GRAPHS)
def test_invariants(name, tip_reads):
    lens, reads, arcs, clip = _graph_of(name)
    n = len(lens)
    res = unitigs(lens, reads, arcs, clip=clip, tip_reads=tip_reads)
    utg, layout, places, c = res["unitigs"], res["layout"], res["places"], res["counts"]
    cl = lens.astype(np.int64) if clip is None else np.diff(np.asarray(clip).reshape(-1, 2).astype(np.int64), axis=1)[:, 0]
    # states
    for i in range(n):
        want = CONTAINED if reads["contained_by"][i] >= 0 else EMPTY if cl[i] == 0 else None
        assert want is None and places["state"][i] in (PLACED, TIP) or places["state"][i] == want
    assert tip_reads > 0 or not (places["state"] == TIP).any()
    # places and layout are inverse to each other, no read twice
    assert len(layout) == c["placed"] == int((places["state"] == PLACED).sum()) == int(utg["n_reads"].sum())
    assert len(set((layout["vertex"] >> 1).tolist())) == len(layout)
    at = 0
    for j, u in enumerate(utg):
        assert u["layout_at"] == at and u["n_reads"] >= 1
        for r in range(int(u["n_reads"])):
            e = layout[at + r]
            assert tuple(places[e["vertex"] >> 1]) == (j, r, e["vertex"] & 1, PLACED)
        at += int(u["n_reads"])
    for i in np.flatnonzero(places["state"] != PLACED):
        assert tuple(places[i])[:3] == (-1, -1, 0)
    # takes sum to the length, starts and seq_at are running sums, the numbering ascends by first
    seq_at = 0
    for u, vs in zip(utg, vertex_lists(res)):
        e = layout[int(u["layout_at"]):int(u["layout_at"] + u["n_reads"])]
        assert (e["take"] >= 1).all() and e["take"].sum() == u["length"] and u["seq_at"] == seq_at
        assert e["start"].tolist() == (np.cumsum(e["take"]) - e["take"]).tolist()
        assert (u["first"], u["last"]) == (vs[0], vs[-1])
        if u["circular"]:
            assert u["first"] == min(min(vs), min(v ^ 1 for v in vs)) and u["first"] % 2 == 0
        else:
            assert u["first"] < u["last"] ^ 1 and e["take"][-1] == cl[vs[-1] >> 1]
        seq_at += int(u["length"])
    assert (np.diff(utg["first"]) > 0).all()
    assert c["links"] == c["e1_arcs"] - c["joins"] + 2 * c["circular"] and c["reads"] == n
    assert c["placed"] + c["cut"] + c["contained"] + int((places["state"] == EMPTY).sum()) == n
    # the same unitigs from the complemented input
    other = unitigs(*_complemented(lens, reads, arcs, clip)[:3], clip=_complemented(lens, reads, arcs, clip)[3], tip_reads=tip_reads)
    mine = sorted(_canonical(vs, u["circular"]) for u, vs in zip(utg, vertex_lists(res)))
    theirs = sorted(_canonical([v ^ 1 for v in vs], u["circular"]) for u, vs in zip(other["unitigs"], vertex_lists(other)))
    assert mine == theirs and other["places"]["state"].tolist() == places["state"].tolist()
    # the survivors again: the same unitigs with nothing to cut, and with the same tip_reads when it finds no new tip
    gone = places["state"] == TIP
    s_reads = reads.copy()
    s_reads["contained_by"][gone] = 0
    s_arcs = arcs[~(gone[arcs["u"] >> 1] | gone[arcs["v"] >> 1])]
    for again in (0, tip_reads):
        second = unitigs(lens, s_reads, s_arcs, clip=clip, tip_reads=again)
        if not (second["places"]["state"] == TIP).any():
            assert second["unitigs"].tobytes() == utg.tobytes() and second["layout"].tobytes() == layout.tobytes()
        else:
            assert again > 0


# ---- what each hand-made graph is there to show

def _reads_of(res):
    return [[v >> 1 for v in vs] for vs in vertex_lists(res)]


def _run(name, tip_reads):
    lens, reads, arcs, clip = _graph_of(name)
    return unitigs(lens, reads, arcs, clip=clip, tip_reads=tip_reads)


def test_chains_come_out_whole_in_the_orientation_with_the_smaller_head():
    for name, n in (("chain64", 64), ("chain65", 65), ("chain257", 257), ("minus64", 64)):
        res = _run(name, 3)
        u = res["unitigs"]
        assert len(u) == 1 and u["n_reads"][0] == n and not u["circular"][0] and u["first"][0] < u["last"][0] ^ 1
        assert u["length"][0] == sum(1000 + k for k in range(n - 1)) + 5000
    res = _run("minus64", 0)
    assert res["unitigs"]["first"][0] == 0 and (res["places"]["orient"] == 0).all()      # every read on its plus strand: the complement
    assert _reads_of(_run("chain1", 0)) == [[0]] and _run("chain1", 0)["unitigs"]["first"][0] == 0
    assert _run("chain1", 1)["places"]["state"].tolist() == [TIP]
    ordered = sorted(_graph_of("chain257")[2]["u"].tolist())
    assert np.abs(np.diff(vertex_lists(_run("chain257", 0))[0])).max() > 128 and ordered         # neighbours far apart in id


def test_the_tilings_end_with_the_scans_chunk_and_one_read_behind_it():
    for name, n in (("tiling128", 128), ("tiling129", 129)):
        lens, reads, arcs, clip = _graph_of(name)
        assert len(lens) == n and set((arcs["u"] & 1).tolist()) == {0, 1}
        pieces = [list(range(a, min(a + 5, 128))) for a in range(0, 128, 5)] + [[128]] * (n - 128)
        res = _run(name, 0)
        u = res["unitigs"]
        assert _reads_of(res) == pieces and not u["circular"].any()
        assert (u["first"] >> 1).tolist() == [p[0] for p in pieces] and u["layout_at"].tolist() == list(range(0, 126, 5)) + [128] * (n - 128)
        if n == 129:                                     # the head behind the chunk: its number, layout_at and seq_at are all carries
            assert u["first"][-1] == 256 and u["seq_at"][-1] == u["length"][:-1].sum() > 0 and len(u) - 1 == 26
        res = _run(name, 3)
        assert _reads_of(res) == pieces[:25] and np.flatnonzero(res["places"]["state"] == TIP).tolist() == list(range(125, n))


def test_tips():
    assert _reads_of(_run("fork", 1)) == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11]]
    assert _reads_of(_run("fork", 3)) == [list(range(10))] and _run("fork", 3)["counts"]["cut"] == 2
    for tip_reads, want in ((0, [[0, 1, 2, 3, 4], [5], [6]]), (1, [[0, 1, 2, 3, 4]]), (3, [[0, 1, 2, 3, 4]])):
        assert _reads_of(_run("two_tips", tip_reads)) == want
    # dead ends of 3, 4 and 1 reads: at 3 the one of 4 stays, at 1 only the one of 1 goes
    cut = lambda t: np.flatnonzero(_run("tip_lengths", t)["places"]["state"] == TIP).tolist()
    assert cut(0) == [] and cut(1) == [23] and cut(3) == [16, 17, 18, 23]
    assert _reads_of(_run("tip_lengths", 3))[0] == list(range(8))        # merged through read 3, up to read 7 where the long one hangs
    assert cut(4) == [0, 1, 2, 3] + list(range(16, 24))                   # ... and at 4 the backbone's first stretch is a dead end too
    cut = lambda t: np.flatnonzero(_run("reverse_tip", t)["places"]["state"] == TIP).tolist()
    assert cut(1) == [] and cut(3) == [8, 9] and _reads_of(_run("reverse_tip", 3)) == [list(range(8))]
    assert len(_run("isolated", 0)["unitigs"]) == 2 and _reads_of(_run("isolated", 3)) == [[3, 4, 5, 6]]
    assert len(_run("no_arcs", 0)["unitigs"]) == 3 and _run("no_arcs", 1)["places"]["state"].tolist() == [TIP] * 3


def test_cycles():
    for name, n in (("cycle2", 2), ("cycle3", 3), ("cycle300", 300), ("cycle_minus", 5)):
        for tip_reads in (0, 3):
            res = _run(name, tip_reads)
            u = res["unitigs"]
            assert len(u) == 1 and (u["n_reads"][0], u["circular"][0], u["first"][0]) == (n, 1, 0) and res["counts"]["links"] == 2
            assert res["links"] == [(0, "+", 0, "+", res["links"][0][4]), (0, "-", 0, "-", res["links"][1][4])] or \
                res["links"] == [(0, "-", 0, "-", res["links"][0][4]), (0, "+", 0, "+", res["links"][1][4])]
    # the stored cycle 1 4 7 2 8 holds read 0 on its minus strand: emitted is 0 -> 9 -> 3 -> 6 -> 5
    assert vertex_lists(_run("cycle_minus", 0)) == [[0, 9, 3, 6, 5]]
    res = _run("cycle_beside", 3)
    assert sorted(res["unitigs"]["n_reads"].tolist()) == [9, 12, 19] and res["unitigs"]["circular"].sum() == 1
    # a dead end of 2 hangs off the cycle: it holds the cycle open until it is cut
    assert sorted(_run("cycle_tip", 1)["unitigs"]["n_reads"].tolist()) == [2, 6] and _run("cycle_tip", 1)["unitigs"]["circular"].sum() == 0
    res = _run("cycle_tip", 3)
    assert res["unitigs"]["n_reads"].tolist() == [6] and res["unitigs"]["circular"].tolist() == [1] and res["counts"]["cut"] == 2


def test_skipped_inputs_and_refusals():
    res = _run("skipped", 0)
    assert res["places"]["state"].tolist() == [PLACED] * 6 + [CONTAINED, EMPTY] and _reads_of(res) == [[0, 1, 2, 3, 4, 5]]
    assert res["unitigs"]["length"][0] == sum(1000 + k for k in range(5)) + 4800 and res["counts"]["e0_arcs"] == 10
    lens, reads, arcs, clip = _graph_of("fork")
    bad = []
    a = arcs.copy(); a["v"][0] = 2 * len(lens); bad.append((a, reads, "range"))
    a = arcs.copy(); a["v"][0] = a["u"][0] ^ 1; bad.append((a, reads, "range"))
    a = arcs.copy(); a["len"][0] = 0; bad.append((a, reads, "range"))
    a = arcs[::-1].copy(); bad.append((a, reads, "ascending"))
    a = np.concatenate([arcs[:1], arcs]); bad.append((a, reads, "ascending"))
    r = reads.copy(); r["contained_by"][5] = 3; bad.append((arcs, r, "live"))
    a = arcs[1:].copy(); bad.append((a, reads, "complement"))
    a = arcs.copy(); a["flags"][0] = 1; bad.append((a, reads, "complement"))
    for a, r, word in bad:
        with pytest.raises(ValueError, match=word):
            unitigs(lens, r, a, tip_reads=3)
    with pytest.raises(ValueError, match="tip_reads"):
        unitigs(lens, reads, arcs, tip_reads=-1)
    with pytest.raises(ValueError, match="longer"):
        a = arcs.copy(); a["len"][-1] = 5001
        unitigs(lens, reads, a, seqs=[np.zeros(5000, dtype=np.uint8)] * len(lens))
    empty = unitigs(np.zeros(0, dtype=np.int32), unitig_model.plain_reads(0), arcs[:0])
    assert len(empty["unitigs"]) == 0 and empty["counts"]["placed"] == 0


def test_large_lengths_stay_exact():
    lens = np.full(3, 1 << 30, dtype=np.int32)
    arcs = unitig_model.make_arcs([(0, 2, (1 << 30) - 2000), (2, 5, (1 << 30) - 2000)])
    res = unitigs(lens, unitig_model.plain_reads(3), arcs, tip_reads=0)
    assert res["unitigs"]["length"].tolist() == [3 * (1 << 30) - 4000] and res["layout"]["start"].tolist() == [0, (1 << 30) - 2000, (1 << 31) - 4000]


# ---- the structs, the exports, the driver's refusal

def test_the_structs_are_what_a_c_compiler_sees(tmp_path):
    from gact_amd import engine
    fields = {"gact_unitig": (engine.UNITIG_DTYPE, ("first", "last", "n_reads", "circular", "layout_at", "seq_at", "length")),
              "gact_unitig_entry": (engine.UNITIG_ENTRY_DTYPE, ("vertex", "take", "start")),
              "gact_unitig_place": (engine.UNITIG_PLACE_DTYPE, ("unitig", "rank", "orient", "state"))}
    stats = [n for n, _ in engine.UnitigStats._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\nint main(void) {\n"
    for name, (_, names) in fields.items():
        src += "printf(\"%%zu \", sizeof(%s));\n" % name + "".join("printf(\"%%zu \", offsetof(%s, %s));\n" % (name, f) for f in names)
    src += "printf(\"%zu \", sizeof(gact_unitig_stats));\n" + "".join("printf(\"%%zu \", offsetof(gact_unitig_stats, %s));\n" % f for f in stats)
    src += "printf(\"%zu %d %d %d %d %d\", sizeof(gact_unitig_params), GACT_UNITIG_DEFAULT_TIP_READS, GACT_UNITIG_PLACED, " \
           "GACT_UNITIG_CONTAINED, GACT_UNITIG_EMPTY, GACT_UNITIG_TIP);\nreturn 0; }\n"
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    want = []
    for name, (dt, names) in fields.items():
        want += [dt.itemsize] + [dt.fields[f][1] for f in names]
        assert tuple(dt.names) == names
    want += [ctypes.sizeof(engine.UnitigStats)] + [getattr(engine.UnitigStats, f).offset for f in stats]
    want += [ctypes.sizeof(engine.UnitigParams), engine.UnitigParams().tip_reads, PLACED, CONTAINED, EMPTY, TIP]
    assert got == want
    assert [fields[k][0].itemsize for k in fields] == [40, 16, 16] and engine.UNITIG_DEFAULT_TIP_READS == 3
    assert [engine.UNITIG_PLACED, engine.UNITIG_CONTAINED, engine.UNITIG_EMPTY, engine.UNITIG_TIP] == [0, 1, 2, 3]


def test_the_library_exports_the_entries(hip_lib_path):
    from gact_amd import engine
    lib = ctypes.CDLL(hip_lib_path)
    for name in ("gact_hip_unitigs", "gact_hip_last_unitig_stats"):
        assert name in engine.EXPORTS
        getattr(lib, name)
    assert hasattr(engine.Engine, "unitigs") and hasattr(engine.Engine, "last_unitig_stats")


def test_the_driver_refuses_unitigs_without_gfa_before_it_opens_a_device(tmp_path):
    from gact_amd import engine
    drv = engine.driver_path()
    for args, word in ((["reads.fasta", "reads.fasta", "1", "--device-dsoft", "--unitigs", "3"], "--gfa"),
                       (["reads.fasta", "reads.fasta", "1", "--device-dsoft", "--gfa", "--unitigs", "-1"], "integer"),
                       (["reads.fasta", "reads.fasta", "1", "--device-dsoft", "--gfa", "--unitigs"], "integer")):
        out = subprocess.run([drv] + args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert out.returncode == 1 and "--unitigs" in out.stderr and word in out.stderr, (args, out.stdout, out.stderr)
        assert not list(tmp_path.iterdir())
