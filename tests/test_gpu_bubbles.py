"""GPU suite for the bubble popping (gact_hip_pop_bubbles, csrc/gact_bubble.hpp): bubbles, read_bubble, arc_flags and the
statistics' counts equal the model's (tests/bubble_model.py) byte for byte -- on every hand-made case, on random graphs with and
without the tips skipped, three times over on two slots, through the bubbles_cap protocol and the refusals, composed with the
unitig call, and through the driver's --bubbles.  No tolerance: everything is integer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bubble_model
import graph_model
import unitig_model
from bubble_model import hand_made, pop_bubbles

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
    """(read_lens, reads, arcs, clip, tips) of a named graph, made once; tips: the reads unitig_model cuts at tip_reads = 3"""
    if name not in _GRAPHS:
        if name.startswith("random"):
            n, seed = name[6:].split("_")
            g = unitig_model.random_graph(int(n), int(seed))
        elif name in bubble_model.HAND_MADE:
            g = hand_made(name)[:4]
        else:
            g = unitig_model.hand_made(name)
        tips = unitig_model.unitigs(g[0], g[1], g[2], clip=g[3], tip_reads=3)["places"]["state"] == unitig_model.TIP
        _GRAPHS[name] = tuple(g) + (tips.astype(np.uint8),)
    return _GRAPHS[name]


def _case(name, skip=None, **kw):
    """(the graph, the skip array, the model's result), computed once.  skip: None, "tips", or a tuple of read ids"""
    key = (name, skip, tuple(sorted(kw.items())))
    lens, reads, arcs, clip, tips = _graph_of(name)
    sk = None
    if skip == "tips":
        sk = tips
    elif skip is not None:
        sk = np.zeros(len(lens), dtype=np.uint8)
        sk[list(skip)] = 1
    if key not in _MODEL:
        _MODEL[key] = pop_bubbles(lens, reads, arcs, clip=clip, skip=sk, **kw)
        bubble_model.check(reads, arcs, _MODEL[key], skip=sk)
    return (lens, reads, arcs, clip), sk, _MODEL[key]


def _same(got, want, what):
    for name, g in zip(("bubbles", "read_bubble", "arc_flags"), got):
        w = want[name]
        assert g.dtype == w.dtype and len(g) == len(w), "%s: %d %s, the model has %d" % (what, len(g), name, len(w))
        if g.tobytes() != w.tobytes():
            bad = int(np.flatnonzero(g != w)[0])
            raise AssertionError("%s: %s differ at %d: device %s, model %s" % (what, name, bad, g[bad], w[bad]))


def _same_counts(st, want, what, n_arcs):
    for name in bubble_model.COUNTS:
        assert st[name] == want["counts"][name], "%s: statistics' %s: device %s, model %s" % (what, name, st[name], want["counts"][name])
    assert st["device_ms"] > 0 and st["scratch_bytes"] >= 36 * n_arcs


def _check(eng, name, skip=None, slot=0, **kw):
    (lens, reads, arcs, clip), sk, want = _case(name, skip, **kw)
    held = [a for a in (lens, reads, arcs, clip, sk) if a is not None]
    before = [a.tobytes() for a in held]
    _same(eng.pop_bubbles(lens, reads, arcs, clip=clip, skip=sk, slot=slot, **kw), want, (name, skip, kw, slot))
    _same_counts(eng.last_bubble_stats(slot), want, (name, skip, kw), len(arcs))
    assert before == [a.tobytes() for a in held]
    return want


@pytest.mark.parametrize("name", bubble_model.HAND_MADE)
def test_hand_made(eng, name):
    kw = dict(max_dist=1 << 30) if name == "long_lens" else {}
    want = _check(eng, name, **kw)
    c = want["counts"]
    found = dict(simple=2, tie=2, more_reads=2, minus=2, beads=6, nested_in=4, nested_out=4, fan62=2, deep=2, long_lens=1).get(name, 0)
    assert c["found"] == found and c["popped"] == (found + 1) // 2 - (name.startswith("nested"))
    if name == "long_lens":
        assert want["bubbles"]["path_len"][0] > 1 << 31
    if name == "flagged":
        assert c["sources"] == 0
    if name in ("fan62", "deep"):
        assert want["bubbles"]["n_vertices"][0] == (64 if name == "fan62" else 62)


def test_limits_of_distance_and_vertices(eng):
    many = bubble_model.FAILS.index("many")
    dist = bubble_model.FAILS.index("dist")
    assert _check(eng, "simple", max_vertices=3)["counts"]["by_fail"][many] == 2
    assert _check(eng, "simple", max_vertices=4)["counts"]["popped"] == 1
    assert _check(eng, "fan62", max_vertices=63)["counts"]["by_fail"][many] == 2
    assert _check(eng, "fan63")["counts"]["by_fail"][many] == 2
    assert _check(eng, "simple", max_dist=2200)["counts"]["popped"] == 1
    assert _check(eng, "simple", max_dist=2199)["counts"]["by_fail"][dist] == 2


def test_skip_takes_a_reads_arcs_out(eng):
    assert _check(eng, "dead")["counts"]["found"] == 0
    extra = hand_made("dead")[4]["extra"][0] >> 1
    want = _check(eng, "dead", skip=(extra,))
    assert want["counts"]["popped"] == 1 and want["counts"]["working_arcs"] == len(_graph_of("dead")[2]) - 2


@pytest.mark.parametrize("name", ["chain64", "no_arcs"])
def test_graphs_without_a_branch(eng, name):
    want = _check(eng, name)
    assert want["counts"]["sources"] == 0 and len(want["bubbles"]) == 0


@pytest.mark.parametrize("skip", [None, "tips"])
@pytest.mark.parametrize("name,at_least", [("random300_3", 5), ("random300_2", 5), ("random3000_1", 50)])
def test_random_graphs(eng, name, at_least, skip):
    want = _check(eng, name, skip=skip)
    print(name, skip, want["counts"])
    assert want["counts"]["popped"] >= at_least
    if skip and name == "random3000_1":                     # (the small graphs have no tip that keeps an arc)
        assert _graph_of(name)[4].any() and want["counts"]["working_arcs"] < _case(name)[2]["counts"]["working_arcs"]


def test_the_result_is_the_same_on_every_run_and_on_every_slot(eng):
    for slot in (0, 0, 1):
        _check(eng, "random3000_1", skip="tips", slot=slot)
        _check(eng, "beads", slot=slot)
    # a small graph after a large one on the same scratch, and the large one again
    _check(eng, "simple")
    _check(eng, "random3000_1")


def _raw_call(eng, lens, reads, arcs, clip=None, skip=None, slot=0, n_reads=None, n_arcs=None, max_dist=50000, max_vertices=64,
              bubbles=None, cap=0, count="own", read_bubble=None, arc_flags=None):
    from gact_amd import engine
    ptr = lambda a: a.ctypes.data if a is not None else None
    par = engine.BubbleParams(max_dist, max_vertices)
    n_bubbles = C.c_int64(-9)
    rc = eng.L.gact_hip_pop_bubbles(eng.h, slot, len(lens) if n_reads is None else n_reads, ptr(lens), ptr(clip), ptr(reads),
                                    len(arcs) if n_arcs is None else n_arcs, ptr(arcs), ptr(skip), C.byref(par), ptr(bubbles), cap,
                                    C.byref(n_bubbles) if count == "own" else None, ptr(read_bubble), ptr(arc_flags))
    return rc, n_bubbles.value


def test_bubbles_cap_protocol(eng):
    from gact_amd import engine
    (lens, reads, arcs, clip), sk, want = _case("beads")
    need = len(want["bubbles"])
    assert need == 6
    bubbles = np.full(need, -5, dtype=engine.BUBBLE_DTYPE)
    for room, ptr_given in ((need - 1, True), (0, True), (need, False)):
        read_bubble, arc_flags = np.full(len(lens), -7, dtype=np.int32), np.full(len(arcs), -7, dtype=np.int32)
        rc, n = _raw_call(eng, lens, reads, arcs, bubbles=bubbles if ptr_given else None, cap=room, read_bubble=read_bubble,
                          arc_flags=arc_flags)
        assert (rc, n) == (-1, need) and b"room" in eng.L.gact_hip_last_error()
        assert (bubbles["source"] == -5).all()
        _same((want["bubbles"], read_bubble, arc_flags), want, "a call without room")
        _same_counts(eng.last_bubble_stats(), want, "a call without room", len(arcs))
    read_bubble, arc_flags = np.full(len(lens), -7, dtype=np.int32), np.full(len(arcs), -7, dtype=np.int32)
    assert _raw_call(eng, lens, reads, arcs, bubbles=bubbles, cap=need, read_bubble=read_bubble, arc_flags=arc_flags) == (0, need)
    _same((bubbles, read_bubble, arc_flags), want, "a call with room")
    # the binding calls once more: the large random graph has more bubbles than its first room
    assert len(_case("random3000_1")[2]["bubbles"]) > 64
    _check(eng, "random3000_1")


def test_refusals(eng):
    from gact_amd import engine
    lens, reads, arcs, clip, tips = _graph_of("simple")
    n = len(lens)
    bubbles = np.full(8, -5, dtype=engine.BUBBLE_DTYPE)
    read_bubble, arc_flags = np.full(n, -7, dtype=np.int32), np.full(len(arcs), -7, dtype=np.int32)
    base = dict(lens=lens, reads=reads, arcs=arcs, n_reads=n, bubbles=bubbles, cap=8, read_bubble=read_bubble, arc_flags=arc_flags)

    def call(**over):
        kw = dict(base)
        kw.update(over)
        return _raw_call(eng, kw.pop("lens"), kw.pop("reads"), kw.pop("arcs"), **kw)

    def changed(field, k, value):
        a = arcs.copy()
        a[field][k] = value
        return a

    contained = reads.copy()
    contained["contained_by"][int(arcs["u"][0]) >> 1] = 3
    neg = lens.copy()
    neg[1] = -1
    whole = np.stack([np.zeros_like(lens), lens], axis=1).astype(np.int32)
    bad_clip = whole.copy()
    bad_clip[2] = (3000, 2999)
    cases = [(dict(max_dist=0), b"max_dist"), (dict(max_dist=(1 << 30) + 1), b"max_dist"), (dict(max_vertices=2), b"max_vertices"),
             (dict(max_vertices=65), b"max_vertices"), (dict(count=None), b"NULL"), (dict(read_bubble=None), b"NULL"),
             (dict(arc_flags=None), b"NULL"), (dict(cap=-1), b"bubbles_cap = -1"), (dict(n_reads=-1), b"n_reads = -1"),
             (dict(n_arcs=-1), b"n_arcs = -1"), (dict(lens=None), b"NULL"), (dict(reads=None), b"NULL"), (dict(lens=neg), b"negative"),
             (dict(clip=bad_clip.reshape(-1)), b"clip"),
             # the arc refusals shared with the unitig call, one of each kind
             (dict(arcs=changed("v", 0, 2 * n)), b"outside"), (dict(arcs=arcs[::-1].copy()), b"ascending"),
             (dict(reads=contained), b"not live"), (dict(arcs=arcs[1:].copy()), b"complement")]
    for bad, word in cases:
        rc, count = call(**bad)
        assert rc == -1 and count == -9, bad
        assert word in eng.L.gact_hip_last_error(), (bad, eng.L.gact_hip_last_error())
    rc, count = call(slot=2)
    assert rc < 0 and b"slot" in eng.L.gact_hip_last_error()
    assert (bubbles["source"] == -5).all() and (read_bubble == -7).all() and (arc_flags == -7).all()
    fresh = engine.Engine(max_blocks=1)
    try:
        with pytest.raises(engine.GactHipError, match="no bubbles"):
            fresh.last_bubble_stats()
    finally:
        fresh.close()
    # the call works after the refusals, with a clip of whole reads; and n_reads == 0 returns 0 and writes the count alone
    want = _case("simple")[2]
    assert call(clip=whole.reshape(-1)) == (0, 2)
    _same((bubbles[:2], read_bubble, arc_flags), want, "after the refusals")
    read_bubble[:], arc_flags[:] = -7, -7
    assert call(lens=lens[:0], reads=reads[:0], arcs=arcs[:0], n_reads=0) == (0, 0)
    assert (read_bubble == -7).all() and (arc_flags == -7).all()
    got = eng.pop_bubbles(lens[:0], reads[:0], arcs[:0])
    assert [len(a) for a in got] == [0, 0, 0]


@pytest.mark.parametrize("name", ["simple", "beads", "random300_1"])
def test_unitigs_of_the_cleaned_arcs(eng, name):
    (lens, reads, arcs, clip), sk, want = _case(name, skip="tips" if name.startswith("random") else None)
    got = eng.pop_bubbles(lens, reads, arcs, clip=clip, skip=sk)
    _same(got, want, name)
    cleaned = bubble_model.cleaned(arcs, got[2])
    model = unitig_model.unitigs(lens, reads, cleaned, clip=clip, tip_reads=3)
    dev = eng.unitigs(lens, reads, cleaned, clip=clip, tip_reads=3)
    for part, g in zip(("unitigs", "layout", "places"), dev):
        assert g.tobytes() == model[part].tobytes(), (name, part)
    before = unitig_model.unitigs(lens, reads, arcs, clip=clip, tip_reads=3)
    assert len(model["unitigs"]) < len(before["unitigs"])
    if not name.startswith("random"):
        assert len(before["unitigs"]) >= 4 and len(model["unitigs"]) == 1


# ---- the driver

def test_driver_bubbles(tmp_path):
    import re
    from gact_amd import engine, synth, workload
    from test_gpu_unitigs import _utg_gfa
    # the reads of ecoli10x_small (232 of them: the tiny workload of the unitig driver test has no bubble); the driver filters them itself
    cfg = dict(workload.CONFIGS["ecoli10x_small"])
    rs = synth.simulate_reads(seed=cfg.pop("seed"), **cfg)
    rs.write_fasta(str(tmp_path / "reads.fasta"))
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()
    ids = {name: i for i, name in enumerate(rs.names)}
    lens = np.array([len(r) for r in rs.reads], dtype=np.int32)
    extra = ("--unique", "pair", "--coverage", "3", "--gfa", "--unitigs", "3")

    def run(name, *more):
        d = tmp_path / name
        d.mkdir()
        for f in ("reads.fasta", "params.cfg"):
            os.symlink(tmp_path / f, d / f)
        out = subprocess.run([drv, "reads.fasta", "reads.fasta", "2", "--device-dsoft"] + list(extra + more), capture_output=True,
                             text=True, cwd=d, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        return {p.name: p.read_bytes() for p in d.iterdir() if p.name.startswith("darwin.")}

    without = run("utg")
    files = run("bubbles", "--bubbles", "50000")
    assert sorted(files) == sorted(list(without) + ["darwin.bubbles.tsv"])
    for f in without:
        if f != "darwin.utg.gfa":
            assert files[f] == without[f], f
    # the graph's inputs as tests/test_gpu_unitigs.py reconstructs them: the records of the .out files, the clip of the table
    pat = re.compile(r"ref_id: (\w+), query_id: (\w+), ab: (-?\d+), ae: (-?\d+), bb: (-?\d+), be: (-?\d+), score: (-?\d+), comp: (\d)")
    rows = []
    for t in range(2):
        for line in without["darwin.%d.out" % t].decode().splitlines():
            m = pat.fullmatch(line)
            rows.append((ids[m.group(1)], ids[m.group(2)], int(m.group(8))) + tuple(int(m.group(k)) for k in (3, 4, 5, 6, 7)) + (1,))
    tsv = [line.split("\t") for line in without["darwin.cover.tsv"].decode().splitlines()]
    clip = np.array([(int(f[6]), int(f[7])) for f in tsv], dtype=np.int32).reshape(-1)
    g = graph_model.graph(graph_model.records_of(rows), lens, clip=clip)
    # the model chain: graph -> unitigs (tips) -> bubbles -> unitigs
    tips = unitig_model.unitigs(lens, g["reads"], g["arcs"], clip=clip, tip_reads=3)["places"]["state"] == unitig_model.TIP
    popped = pop_bubbles(lens, g["reads"], g["arcs"], clip=clip, skip=tips, max_dist=50000)
    print("--bubbles 50000:", popped["counts"])
    want_tsv = "".join("%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % tuple(int(b[k]) for k in ("source", "sink", "state", "n_vertices", "n_path",
                                                                                   "n_removed", "path_len")) for b in popped["bubbles"])
    assert files["darwin.bubbles.tsv"].decode() == want_tsv
    want = unitig_model.unitigs(lens, g["reads"], bubble_model.cleaned(g["arcs"], popped["arc_flags"]), clip=clip, tip_reads=3, seqs=rs.reads)
    seg, entries, links = _utg_gfa(tmp_path / "bubbles" / "darwin.utg.gfa")
    names = ["utg%06d%s" % (j + 1, "c" if u["circular"] else "l") for j, u in enumerate(want["unitigs"])]
    assert seg == [(names[j], want["seq"][int(u["seq_at"]):int(u["seq_at"] + u["length"])].tobytes().decode())
                   for j, u in enumerate(want["unitigs"])]
    for j, u in enumerate(want["unitigs"]):
        lay = want["layout"][int(u["layout_at"]):int(u["layout_at"] + u["n_reads"])]
        assert entries[j] == [(int(e["start"]), rs.names[e["vertex"] >> 1], int(clip[2 * (e["vertex"] >> 1)]),
                               int(clip[2 * (e["vertex"] >> 1) + 1]), "+-"[e["vertex"] & 1], int(e["take"])) for e in lay]
    assert links == [(names[a], sa, names[b], sb, ov) for a, sa, b, sb, ov in want["links"]]
    # not trivially so: bubbles pop, reads go, and the unitigs are fewer for it
    assert popped["counts"]["popped"] >= 2 and popped["counts"]["lost"] >= 2 and popped["counts"]["reads_removed"] >= 2
    assert files["darwin.utg.gfa"] != without["darwin.utg.gfa"] and len(seg) < len(_utg_gfa(tmp_path / "utg" / "darwin.utg.gfa")[0])
    # refused before any file is read or any device is opened
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    for args in (("--gfa", "--bubbles", "50000"), ("--gfa", "--unitigs", "0", "--bubbles", "50000"), ("--unitigs", "3", "--bubbles", "50000"),
                 ("--gfa", "--unitigs", "3", "--bubbles", "0"), ("--gfa", "--unitigs", "3", "--bubbles", str((1 << 30) + 1)),
                 ("--gfa", "--unitigs", "3", "--bubbles", "5k")):
        out = subprocess.run([drv, "missing.fasta", "missing.fasta", "1", "--device-dsoft"] + list(args), capture_output=True, text=True,
                             cwd=tmp_path, timeout=60, env=env)
        assert out.returncode == 1 and "--bubbles" in out.stderr, (args, out.stdout, out.stderr)
