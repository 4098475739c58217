"""GPU suite for the weak-arc rule and the cleaning rounds (gact_hip_prune_overlaps, gact_hip_clean_graph, csrc/gact_clean.hpp):
arc_flags, vertex_best, read_state, the step log and the statistics' counts equal the model's (tests/clean_model.py) byte for
byte -- on every hand-made case, at the ratios' ends, on generated graphs with and without repeats and with and without the
tips skipped, three times over on two slots, through the steps_cap protocol and the refusals, composed with the unitig call, against the
same rounds made from the stand-alone calls, in the one wording the four calls on an arc graph share for a fault, and through the
driver's --clean.  No tolerance: everything is integer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bubble_model
import clean_model
import graph_model
import unitig_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    """an engine that aligns nothing: two slots, workspaces for one block"""
    from gact_amd import engine
    e = engine.Engine(n_slots=2, max_blocks=1)
    yield e
    e.close()


_GRAPHS, _MODEL = {}, {}
_BUBBLE_GRAPHS = ("simple", "beads", "nested_in", "nested_out")


def _graph_of(name):
    """(read_lens, reads, arcs, clip, skip of the case or None, tips) of a named graph, made once"""
    if name not in _GRAPHS:
        skip = None
        if name.startswith("random") or name.startswith("repeat"):
            n, seed = name[6:].split("_")
            g = (unitig_model.random_graph if name.startswith("random") else clean_model.repeat_graph)(int(n), int(seed))[:4]
        elif name in clean_model.HAND_MADE:
            g = clean_model.hand_made(name)
            skip = g[4]["skip"]
            g = g[:4]
        else:
            g = bubble_model.hand_made(name)[:4]
        tips = unitig_model.unitigs(g[0], g[1], g[2], clip=g[3], tip_reads=3)["places"]["state"] == unitig_model.TIP
        _GRAPHS[name] = tuple(g) + (skip, tips.astype(np.uint8))
    return _GRAPHS[name]


def _prune_case(name, skip="own", ratio=500):
    lens, reads, arcs, clip, own, tips = _graph_of(name)
    sk = own if skip == "own" else tips if skip == "tips" else None
    key = ("prune", name, skip, ratio)
    if key not in _MODEL:
        _MODEL[key] = clean_model.prune(lens, reads, arcs, clip=clip, skip=sk, ratio_permille=ratio)
        clean_model.check(reads, arcs, _MODEL[key]["arc_flags"])
    return (lens, reads, arcs, clip), sk, _MODEL[key]


def _clean_case(name, **kw):
    lens, reads, arcs, clip = _graph_of(name)[:4]
    key = ("clean", name, tuple(sorted(kw.items())))
    if key not in _MODEL:
        _MODEL[key] = clean_model.clean(lens, reads, arcs, clip=clip, **kw)
        clean_model.check(reads, arcs, _MODEL[key]["arc_flags"], _MODEL[key]["steps"], _MODEL[key]["read_state"])
    return (lens, reads, arcs, clip), _MODEL[key]


def _same(got, want, names, what):
    for name, g in zip(names, got):
        w = want[name]
        assert g.dtype == w.dtype and len(g) == len(w), "%s: %d %s, the model has %d" % (what, len(g), name, len(w))
        if g.tobytes() != w.tobytes():
            bad = int(np.flatnonzero(g != w)[0])
            raise AssertionError("%s: %s differ at %d: device %s, model %s" % (what, name, bad, g[bad], w[bad]))


def _same_counts(st, want, names, what, n_arcs):
    for name in names:
        assert st[name] == want["counts"][name], "%s: statistics' %s: device %s, model %s" % (what, name, st[name], want["counts"][name])
    assert st["device_ms"] > 0 and st["scratch_bytes"] >= 36 * n_arcs


def _check_prune(eng, name, skip="own", ratio=500, slot=0):
    (lens, reads, arcs, clip), sk, want = _prune_case(name, skip, ratio)
    held = [a for a in (lens, reads, arcs, clip, sk) if a is not None]
    before = [a.tobytes() for a in held]
    got = eng.prune_overlaps(lens, reads, arcs, clip=clip, skip=sk, ratio_permille=ratio, best=True, slot=slot)
    _same(got, want, ("arc_flags", "vertex_best"), (name, skip, ratio, slot))
    _same_counts(eng.last_prune_stats(slot), want, clean_model.PRUNE_COUNTS, (name, skip, ratio), len(arcs))
    assert before == [a.tobytes() for a in held]
    flags_only = eng.prune_overlaps(lens, reads, arcs, clip=clip, skip=sk, ratio_permille=ratio, slot=slot)
    _same((flags_only,), want, ("arc_flags",), (name, "without vertex_best"))
    return want


def _check_clean(eng, name, slot=0, **kw):
    (lens, reads, arcs, clip), want = _clean_case(name, **kw)
    held = [a for a in (lens, reads, arcs, clip) if a is not None]
    before = [a.tobytes() for a in held]
    got = eng.clean_graph(lens, reads, arcs, clip=clip, slot=slot, **kw)
    _same(got, want, ("arc_flags", "read_state", "steps"), (name, kw, slot))
    _same_counts(eng.last_clean_stats(slot), want, clean_model.CLEAN_COUNTS, (name, kw), len(arcs))
    assert before == [a.tobytes() for a in held]
    return want


# ---- prune

@pytest.mark.parametrize("name", clean_model.HAND_MADE)
def test_prune_hand_made(eng, name):
    want = _check_prune(eng, name)
    info = clean_model.hand_made(name)[4]
    c = want["counts"]
    assert c["weak"] == len(info["weak"]) and c["arcs_removed"] == 2 * c["weak"]
    assert c["examined"] == dict(single=0, no_arcs=0, mirror_only=2).get(name, 1)
    if name == "fan129":
        assert c["weak"] == 3 and c["bared"] == 3
    if name in ("flagged", "skipped"):
        assert want["vertex_best"][info["x"]] == 2000


@pytest.mark.parametrize("ratio", [500, 700])
def test_prune_threshold(eng, ratio):
    want = _check_prune(eng, "threshold", ratio=ratio)
    arcs = _graph_of("threshold")[2]
    assert sorted(int(arcs["ov_u"][k]) for k in want["weak"]) == ([999] if ratio == 500 else [999, 1000, 1399])


def test_prune_products_need_64_bits(eng):
    want = _check_prune(eng, "big_ov", ratio=1000)
    arcs = _graph_of("big_ov")[2]
    assert sorted(int(arcs["ov_u"][k]) for k in want["weak"]) == [clean_model.STRONG, 2 ** 31 - 2]


@pytest.mark.parametrize("name", ["fan65", "random300_1"])
def test_prune_ratios_at_their_ends(eng, name):
    none = _check_prune(eng, name, ratio=0)
    arcs = _graph_of(name)[2]
    assert none["counts"]["weak"] == 0 and none["counts"]["examined"] > 0 and (none["arc_flags"] == arcs["flags"]).all()
    most = _check_prune(eng, name, ratio=1000)
    # everything below the best goes, the ties of the best stay: every examined vertex keeps an arc unless a complement took it
    weak = set(most["weak"])
    for x in np.flatnonzero(most["vertex_best"] > 0).tolist():
        at = [k for k in np.flatnonzero(arcs["u"] == x).tolist() if arcs["flags"][k] == 0]
        assert [k for k in at if k not in weak] == [k for k in at if arcs["ov_u"][k] == most["vertex_best"][x]]
    assert most["counts"]["weak"] > none["counts"]["weak"]


@pytest.mark.parametrize("skip", [None, "tips"])
@pytest.mark.parametrize("ratio", [300, 500, 900])
@pytest.mark.parametrize("name", ["random300_1", "random300_2", "random3000_1", "repeat300_1", "repeat1000_1"])
def test_prune_generated_graphs(eng, name, ratio, skip):
    want = _check_prune(eng, name, skip=skip, ratio=ratio)
    if ratio == 900:
        assert want["counts"]["weak"] > 0 and want["counts"]["examined"] > 0
    if skip and name == "random3000_1":
        assert _graph_of(name)[5].any() and want["counts"]["working_arcs"] < _prune_case(name, None, ratio)[2]["counts"]["working_arcs"]


# ---- clean

@pytest.mark.parametrize("name", clean_model.HAND_MADE + _BUBBLE_GRAPHS)
def test_clean_hand_made(eng, name):
    want = _check_clean(eng, name)
    if name == "false_fork":
        assert want["counts"]["arcs_removed"] == [0, 0, 2]
    if name == "no_arcs":
        assert (want["read_state"]["state"] == clean_model.TIP).all() and (want["read_state"]["step"] == 0).all()
    if name in _BUBBLE_GRAPHS:
        assert want["counts"]["reads_bubble"] >= 1 and want["counts"]["arcs_removed"][clean_model.BUBBLES] >= 2


def test_clean_nested_bubbles_and_the_second_pass(eng):
    """nested_in needs the second pass: one pass leaves more arcs than four.  In nested_out the outer bubble owns the contested
    reads, pops in the first pass and takes the inner one's losing branch with it (the bubble rule, which does not change), so one
    pass leaves what four leave: 20 arcs either way in the model, and the device has to say the same"""
    one = _check_clean(eng, "nested_in", max_passes=1)
    four = _check_clean(eng, "nested_in")
    assert one["counts"]["arcs_left"] > four["counts"]["arcs_left"] and four["counts"]["passes"] >= 2
    one = _check_clean(eng, "nested_out", max_passes=1)
    four = _check_clean(eng, "nested_out")
    assert one["counts"]["arcs_left"] == four["counts"]["arcs_left"]


@pytest.mark.parametrize("name", ["repeat300_1", "repeat1000_1", "repeat3000_1", "random3000_1"])
def test_clean_generated_graphs(eng, name):
    want = _check_clean(eng, name)
    print(name, want["counts"])
    assert want["counts"]["passes"] >= 2
    if name.startswith("repeat"):
        assert want["counts"]["arcs_removed"][clean_model.PRUNE] > 0


@pytest.mark.parametrize("ratios", [(500, 700, 0), (500, 700, 1), (600, 600, 3), (0, 1000, 16)])
def test_clean_ratio_plans(eng, ratios):
    want = _check_clean(eng, "repeat300_1", ratios=ratios)
    kinds = want["steps"]["kind"]
    assert (kinds == clean_model.PRUNE).sum() == ratios[2]
    assert want["steps"]["param"][kinds == clean_model.PRUNE].tolist() == clean_model.ratios_of(*ratios)
    _check_clean(eng, "threshold", ratios=ratios, max_passes=2, tip_reads=1, max_dist=3000, max_vertices=8)


@pytest.mark.parametrize("name", ["false_fork", "nested_in", "repeat300_1", "repeat3000_1"])
def test_unitigs_of_the_cleaned_arcs(eng, name):
    (lens, reads, arcs, clip), want = _clean_case(name)
    got = eng.clean_graph(lens, reads, arcs, clip=clip)
    _same(got, want, ("arc_flags", "read_state", "steps"), name)
    cleaned = clean_model.cleaned(arcs, got[0])
    model = unitig_model.unitigs(lens, reads, cleaned, clip=clip, tip_reads=3)
    dev = eng.unitigs(lens, reads, cleaned, clip=clip, tip_reads=3, seq=False)
    for part, g in zip(("unitigs", "layout", "places"), dev):
        assert g.tobytes() == model[part].tobytes(), (name, part)
    before = unitig_model.unitigs(lens, reads, arcs, clip=clip, tip_reads=3)
    assert len(model["unitigs"]) < len(before["unitigs"])
    if name.startswith("repeat"):
        assert len(model["unitigs"]) == 1


# ---- protocols

def test_the_result_is_the_same_on_every_run_and_on_every_slot(eng):
    for slot in (0, 0, 1):
        _check_clean(eng, "repeat3000_1", slot=slot)
        _check_prune(eng, "repeat1000_1", skip="tips", ratio=900, slot=slot)
        _check_clean(eng, "beads", slot=slot)
        _check_prune(eng, "fan129", slot=slot)
    # a small graph after a large one on the same scratch, and the large one again
    _check_clean(eng, "false_fork")
    _check_clean(eng, "repeat3000_1")


def test_every_other_statistic_stays(eng):
    """the rounds launch the unitig and bubble kernels on a scratch of their own: those calls' figures stay as they were"""
    lens, reads, arcs, clip = _graph_of("beads")[:4]
    eng.unitigs(lens, reads, arcs, clip=clip)
    eng.pop_bubbles(lens, reads, arcs, clip=clip)
    held = eng.last_unitig_stats(), eng.last_bubble_stats()
    _check_prune(eng, "repeat300_1")
    _check_clean(eng, "repeat300_1")
    assert (eng.last_unitig_stats(), eng.last_bubble_stats()) == held
    prune_held = eng.last_prune_stats()
    _check_clean(eng, "beads")
    assert eng.last_prune_stats() == prune_held


def _raw_prune(eng, lens, reads, arcs, clip=None, skip=None, slot=0, n_reads=None, n_arcs=None, ratio=500, arc_flags=None, best=None):
    from gact_amd import engine
    ptr = lambda a: a.ctypes.data if a is not None else None
    par = engine.PruneParams(ratio)
    return eng.L.gact_hip_prune_overlaps(eng.h, slot, len(lens) if n_reads is None else n_reads, ptr(lens), ptr(clip), ptr(reads),
                                         len(arcs) if n_arcs is None else n_arcs, ptr(arcs), ptr(skip), C.byref(par), ptr(arc_flags),
                                         ptr(best))


def _raw_clean(eng, lens, reads, arcs, clip=None, slot=0, n_reads=None, n_arcs=None, params=None, arc_flags=None, read_state=None,
               steps=None, cap=0, count="own", **kw):
    from gact_amd import engine
    ptr = lambda a: a.ctypes.data if a is not None else None
    par = engine.CleanParams(**kw) if params is None else params
    n_steps = C.c_int64(-9)
    rc = eng.L.gact_hip_clean_graph(eng.h, slot, len(lens) if n_reads is None else n_reads, ptr(lens), ptr(clip), ptr(reads),
                                    len(arcs) if n_arcs is None else n_arcs, ptr(arcs), C.byref(par) if par != "null" else None,
                                    ptr(arc_flags), ptr(read_state), ptr(steps), cap, C.byref(n_steps) if count == "own" else None)
    return rc, n_steps.value


def test_steps_cap_protocol(eng):
    from gact_amd import engine
    (lens, reads, arcs, clip), want = _clean_case("repeat300_1")
    need = len(want["steps"])
    assert need == 13
    steps = np.full(need, -5, dtype=engine.CLEAN_STEP_DTYPE)
    for room, ptr_given in ((need - 1, True), (0, True), (need, False)):
        arc_flags, read_state = np.full(len(arcs), -7, dtype=np.int32), np.full(len(lens), -7, dtype=engine.CLEAN_READ_DTYPE)
        rc, n = _raw_clean(eng, lens, reads, arcs, clip=clip, steps=steps if ptr_given else None, cap=room, arc_flags=arc_flags,
                           read_state=read_state)
        assert (rc, n) == (-1, need) and b"room" in eng.L.gact_hip_last_error()
        assert (steps["kind"] == -5).all()
        _same((arc_flags, read_state), want, ("arc_flags", "read_state"), "a call without room")
        _same_counts(eng.last_clean_stats(), want, clean_model.CLEAN_COUNTS, "a call without room", len(arcs))
    arc_flags, read_state = np.full(len(arcs), -7, dtype=np.int32), np.full(len(lens), -7, dtype=engine.CLEAN_READ_DTYPE)
    assert _raw_clean(eng, lens, reads, arcs, clip=clip, steps=steps, cap=need, arc_flags=arc_flags, read_state=read_state) == (0, need)
    _same((arc_flags, read_state, steps), want, ("arc_flags", "read_state", "steps"), "a call with room")
    # NULL params are the defaults
    steps[:] = -5
    assert _raw_clean(eng, lens, reads, arcs, clip=clip, params="null", steps=steps, cap=need, arc_flags=arc_flags,
                      read_state=read_state) == (0, need)
    _same((arc_flags, read_state, steps), want, ("arc_flags", "read_state", "steps"), "NULL params")
    # the binding calls once more: sixteen ratios on a graph that keeps settling take more steps than its first room
    many = _check_clean(eng, "repeat300_1", ratios=(0, 1000, 16))
    assert len(many["steps"]) > 16


def _bad_inputs(lens, reads, arcs):
    n = len(lens)

    def changed(field, k, value):
        a = arcs.copy()
        a[field][k] = value
        return a

    contained = reads.copy()
    contained["contained_by"][int(arcs["u"][0]) >> 1] = 3
    neg = lens.copy()
    neg[1] = -1
    bad_clip = np.stack([np.zeros_like(lens), lens], axis=1).astype(np.int32)
    bad_clip[2] = (3000, 2999)
    return [(dict(n_reads=-1), b"n_reads = -1"), (dict(n_arcs=-1), b"n_arcs = -1"), (dict(lens=None), b"NULL"), (dict(reads=None), b"NULL"),
            (dict(arc_flags=None), b"NULL"), (dict(lens=neg), b"negative"), (dict(clip=bad_clip.reshape(-1)), b"clip"),
            # the arc refusals shared with the unitig and bubble calls, one of each kind: they come from the device
            (dict(arcs=changed("v", 0, 2 * n)), b"outside"), (dict(arcs=arcs[::-1].copy()), b"ascending"),
            (dict(reads=contained), b"not live"), (dict(arcs=arcs[1:].copy()), b"complement")]


def test_prune_refusals(eng):
    from gact_amd import engine
    lens, reads, arcs, clip = _graph_of("false_fork")[:4]
    n = len(lens)
    arc_flags, best = np.full(len(arcs), -7, dtype=np.int32), np.full(2 * n, -7, dtype=np.int32)
    base = dict(lens=lens, reads=reads, arcs=arcs, n_reads=n, arc_flags=arc_flags, best=best)

    def call(**over):
        kw = dict(base)
        kw.update(over)
        return _raw_prune(eng, kw.pop("lens"), kw.pop("reads"), kw.pop("arcs"), **kw)

    for bad, word in _bad_inputs(lens, reads, arcs) + [(dict(ratio=-1), b"ratio_permille"), (dict(ratio=1001), b"ratio_permille")]:
        assert call(**bad) == -1, bad
        assert word in eng.L.gact_hip_last_error(), (bad, eng.L.gact_hip_last_error())
    assert call(slot=2) < 0 and b"slot" in eng.L.gact_hip_last_error()
    assert (arc_flags == -7).all() and (best == -7).all()
    fresh = engine.Engine(max_blocks=1)
    try:
        with pytest.raises(engine.GactHipError, match="pruned no overlaps"):
            fresh.last_prune_stats()
        with pytest.raises(engine.GactHipError, match="cleaned no graph"):
            fresh.last_clean_stats()
    finally:
        fresh.close()
    # the call works after the refusals; n_reads == 0 returns 0 and writes nothing
    want = _prune_case("false_fork")[2]
    assert call() == 0
    _same((arc_flags, best), want, ("arc_flags", "vertex_best"), "after the refusals")
    arc_flags[:] = -7
    assert call(lens=lens[:0], reads=reads[:0], arcs=arcs[:0], n_reads=0) == 0 and (arc_flags == -7).all()
    got = eng.prune_overlaps(lens[:0], reads[:0], arcs[:0], best=True)
    assert [len(a) for a in got] == [0, 0]


def test_clean_refusals(eng):
    from gact_amd import engine
    lens, reads, arcs, clip = _graph_of("false_fork")[:4]
    n = len(lens)
    steps = np.full(64, -5, dtype=engine.CLEAN_STEP_DTYPE)
    arc_flags, read_state = np.full(len(arcs), -7, dtype=np.int32), np.full(n, -7, dtype=engine.CLEAN_READ_DTYPE)
    base = dict(lens=lens, reads=reads, arcs=arcs, n_reads=n, arc_flags=arc_flags, read_state=read_state, steps=steps, cap=64)

    def call(**over):
        kw = dict(base)
        kw.update(over)
        return _raw_clean(eng, kw.pop("lens"), kw.pop("reads"), kw.pop("arcs"), **kw)

    cases = _bad_inputs(lens, reads, arcs) + [
        (dict(read_state=None), b"NULL"), (dict(count=None), b"NULL"), (dict(cap=-1), b"steps_cap = -1"),
        (dict(tip_reads=0), b"tip_reads"), (dict(max_dist=0), b"max_dist"), (dict(max_dist=(1 << 30) + 1), b"max_dist"),
        (dict(max_vertices=2), b"max_vertices"), (dict(max_vertices=65), b"max_vertices"), (dict(ratio_lo_permille=-1), b"ratios"),
        (dict(ratio_hi_permille=1001), b"ratios"), (dict(ratio_lo_permille=800), b"ratios"), (dict(n_ratios=-1), b"n_ratios"),
        (dict(n_ratios=17), b"n_ratios"), (dict(max_passes=0), b"max_passes"), (dict(max_passes=17), b"max_passes")]
    for bad, word in cases:
        rc, count = call(**bad)
        assert rc == -1 and count == -9, bad
        assert word in eng.L.gact_hip_last_error(), (bad, eng.L.gact_hip_last_error())
    rc, count = call(slot=2)
    assert rc < 0 and b"slot" in eng.L.gact_hip_last_error()
    assert (steps["kind"] == -5).all() and (arc_flags == -7).all() and (read_state["state"] == -7).all()
    want = _clean_case("false_fork")[1]
    assert call() == (0, len(want["steps"]))
    _same((arc_flags, read_state, steps[:len(want["steps"])]), want, ("arc_flags", "read_state", "steps"), "after the refusals")
    arc_flags[:] = -7
    assert call(lens=lens[:0], reads=reads[:0], arcs=arcs[:0], n_reads=0) == (0, 0) and (arc_flags == -7).all()
    got = eng.clean_graph(lens[:0], reads[:0], arcs[:0])
    assert [len(a) for a in got] == [0, 0, 0]


# ---- the loop is the stand-alone calls' steps; the four calls on an arc graph refuse in one wording

def _rounds_of_the_calls(eng, lens, reads, arcs, clip, tip_reads=3, max_dist=50000, max_vertices=64, ratios=(500, 700, 3), max_passes=4):
    """the rounds made on the host out of the device's stand-alone calls, the way clean_model.clean composes the models:
    -> (arc_flags, read_state, steps) as clean_graph returns them"""
    from gact_amd import engine
    n = len(lens)
    work = arcs.copy()                                # (flags: F)
    touches = list(zip((arcs["u"] >> 1).tolist(), (arcs["v"] >> 1).tolist()))
    state, step_of, steps = [], [-1] * n, []

    def log(kind, param, removed_reads, examined, new_flags):
        had, left = int((work["flags"] == 0).sum()), int((new_flags == 0).sum())
        for i in removed_reads:
            state[i], step_of[i] = (clean_model.TIP if kind == clean_model.TIPS else clean_model.BUBBLE), len(steps)
        steps.append((kind, param, len(removed_reads), examined, had - left, left))
        work["flags"] = new_flags
        return had - left

    def tips():
        places = eng.unitigs(lens, reads, work, clip=clip, tip_reads=tip_reads)[2]
        if not state:                                 # (the first call says which reads are contained or empty)
            own = {unitig_model.CONTAINED: clean_model.CONTAINED, unitig_model.EMPTY: clean_model.EMPTY}
            state.extend(own.get(s, clean_model.KEPT) for s in places["state"].tolist())
        cut = (places["state"] == unitig_model.TIP).tolist()
        f = work["flags"].copy()
        for k, (a, b) in enumerate(touches):
            if f[k] == 0 and (cut[a] or cut[b]):
                f[k] = clean_model.TIP_BIT
        newly = [i for i in range(n) if cut[i] and state[i] == clean_model.KEPT]
        return log(clean_model.TIPS, tip_reads, newly, clean_model._tip_chains(lens, reads, work, clip), f)

    def bubbles():
        _, read_bubble, arc_flags = eng.pop_bubbles(lens, reads, work, clip=clip, max_dist=max_dist, max_vertices=max_vertices)
        return log(clean_model.BUBBLES, max_dist, np.flatnonzero(read_bubble >= 0).tolist(), eng.last_bubble_stats()["sources"], arc_flags)

    def settle():
        for _ in range(max_passes):
            if tips() + bubbles() == 0:
                break

    settle()
    for r in clean_model.ratios_of(*ratios):
        arc_flags = eng.prune_overlaps(lens, reads, work, clip=clip, ratio_permille=r)
        if log(clean_model.PRUNE, r, [], eng.last_prune_stats()["examined"], arc_flags):
            settle()
    read_state = np.zeros(n, dtype=engine.CLEAN_READ_DTYPE)
    read_state["state"], read_state["step"] = state, step_of
    return work["flags"].astype(np.int32), read_state, np.array(steps, dtype=engine.CLEAN_STEP_DTYPE).reshape(-1)


@pytest.mark.parametrize("plan", [dict(), dict(ratios=(500, 700, 0), max_passes=1), dict(ratios=(600, 600, 1))], ids=str)
@pytest.mark.parametrize("name", ["false_fork", "nested_in", "simple", "repeat300_1"])
def test_the_loop_is_its_steps(eng, name, plan):
    """clean_graph launches the step sequences of the unitig, bubble and prune calls on resident arcs: the same calls made one
    by one from the host, each on the flags the one in front left, end with the same bytes"""
    lens, reads, arcs, clip = _graph_of(name)[:4]
    want = _rounds_of_the_calls(eng, lens, reads, arcs, clip, **plan)
    got = eng.clean_graph(lens, reads, arcs, clip=clip, **plan)
    _same(got, dict(zip(("arc_flags", "read_state", "steps"), want)), ("arc_flags", "read_state", "steps"), (name, plan))
    kinds = got[2]["kind"].tolist()
    assert kinds[:2] == [clean_model.TIPS, clean_model.BUBBLES] and kinds.count(clean_model.PRUNE) == plan.get("ratios", (0, 0, 3))[2]
    # behind a prune that removed an arc the loop settles again, as the helper does; in false_fork one does, and makes new tips
    dropped = [j for j, k in enumerate(kinds) if k == clean_model.PRUNE and got[2]["arcs_removed"][j] > 0]
    assert all(kinds[j + 1] == clean_model.TIPS for j in dropped)
    if name == "false_fork" and not plan:
        assert dropped
    if name == "repeat300_1" and not plan:
        assert eng.last_clean_stats()["passes"] >= 2


def _raw_unitigs(eng, lens, reads, arcs, clip=None, slot=0, n_reads=None, n_arcs=None, utg=None, layout=None, places=None, seq=None):
    from gact_amd import engine
    ptr = lambda a: a.ctypes.data if a is not None else None
    par = engine.UnitigParams(3)
    count, seq_len = C.c_int32(-9), C.c_int64(-9)
    rc = eng.L.gact_hip_unitigs(eng.h, slot, len(lens) if n_reads is None else n_reads, ptr(lens), ptr(clip), ptr(reads),
                                len(arcs) if n_arcs is None else n_arcs, ptr(arcs), C.byref(par), ptr(utg), C.byref(count), ptr(layout),
                                ptr(places), ptr(seq), len(seq) if seq is not None else 0, C.byref(seq_len))
    return rc, count.value, seq_len.value


def test_one_wording_for_one_fault(eng):
    """the four calls on an arc graph refuse the same input with the same sentence behind their own names; an input wrong in two
    ways gets the sentence of the first check from all four; a refused call writes nothing"""
    from gact_amd import engine
    from test_gpu_bubbles import _raw_call as _raw_bubbles
    lens, reads, arcs, clip = _graph_of("false_fork")[:4]
    n = len(lens)
    out = dict(utg=np.full(n, -5, dtype=engine.UNITIG_DTYPE), layout=np.full(n, -5, dtype=engine.UNITIG_ENTRY_DTYPE),
               places=np.full(n, -5, dtype=engine.UNITIG_PLACE_DTYPE), bubbles=np.full(8, -5, dtype=engine.BUBBLE_DTYPE),
               read_bubble=np.full(n, -7, dtype=np.int32), arc_flags=np.full(len(arcs), -7, dtype=np.int32),
               best=np.full(2 * n, -7, dtype=np.int32), read_state=np.full(n, -7, dtype=engine.CLEAN_READ_DTYPE),
               steps=np.full(64, -5, dtype=engine.CLEAN_STEP_DTYPE), seq=np.full(int(lens.sum()), 7, dtype=np.uint8))
    held = {k: a.tobytes() for k, a in out.items()}
    entries = {
        "unitigs": (_raw_unitigs, dict(utg=out["utg"], layout=out["layout"], places=out["places"])),
        "pop_bubbles": (_raw_bubbles, dict(bubbles=out["bubbles"], cap=8, read_bubble=out["read_bubble"], arc_flags=out["arc_flags"])),
        "prune_overlaps": (_raw_prune, dict(arc_flags=out["arc_flags"], best=out["best"])),
        "clean_graph": (_raw_clean, dict(arc_flags=out["arc_flags"], read_state=out["read_state"], steps=out["steps"], cap=64))}

    def refused(who, **over):
        """the call of entry `who` on the graph with `over` laid over it -> the sentence behind the entry's name"""
        fn, kw = entries[who]
        kw = dict(dict(lens=lens, reads=reads, arcs=arcs, n_reads=n), **kw)
        kw.update(over)
        if who == "unitigs" and "arc_flags" in over:                    # (the unitig call has no arc_flags: its places)
            kw["places"] = kw.pop("arc_flags")
        res = fn(eng, kw.pop("lens"), kw.pop("reads"), kw.pop("arcs"), **kw)
        assert (res if isinstance(res, int) else res[0]) == -1, (who, over)
        assert isinstance(res, int) or all(v == -9 for v in res[1:]), (who, over, res)
        said = eng.L.gact_hip_last_error().decode()
        assert said.startswith(who + ": "), (who, over, said)
        return said[len(who) + 2:]

    tails = {b"outside": "an arc with u or v outside [0, %d), between the two vertices of one read, or with len < 1" % (2 * n),
             b"ascending": "the arcs are not ascending by (u, len, v)",
             b"not live": "an arc with flags == 0 names a read that is not live (contained, or clipped to nothing)",
             b"complement": "an arc with flags == 0 whose complement v^1 -> u^1 is not among the arcs with flags == 0",
             b"negative": "read 1 has the negative length -1",
             b"clip": "the clip [3000, 2999) of read 2 is not inside [0, %d]" % lens[2]}
    seen = set()
    for bad, word in _bad_inputs(lens, reads, arcs):
        for who in entries:
            tail = refused(who, **bad)
            assert word.decode() in tail, (who, bad, tail)
            if word in tails:
                assert tail == tails[word], (who, bad, tail)
                seen.add(word)
    assert seen == set(tails)
    # wrong in two ways: the arcs reversed, and the one arc the order check passes -- the first -- leaves a contained read
    contained = reads.copy()
    contained["contained_by"][int(arcs["u"][-1]) >> 1] = 3
    for who in entries:
        assert refused(who, arcs=arcs[::-1].copy(), reads=contained) == tails[b"ascending"], who
    # bases asked for, and an arc longer than its clipped read: the unitig call's own sentence, in front of the fallback
    eng.upload_seqs(engine.SET_REF, [np.full(int(ln), ord("A"), dtype=np.uint8) for ln in lens])
    long_arc = arcs.copy()
    assert long_arc["flags"][-1] == 0
    long_arc["len"][-1] = int(lens[int(arcs["u"][-1]) >> 1]) + 1
    assert refused("unitigs", arcs=long_arc, seq=out["seq"]) == "bases asked for and an arc with flags == 0 is longer than the clipped read it leaves"
    assert {k: a.tobytes() for k, a in out.items()} == held


# ---- the driver

def test_driver_clean(tmp_path):
    import re
    from gact_amd import engine, synth, workload
    from test_gpu_unitigs import _utg_gfa
    # the reads of ecoli10x_small, as the bubble driver test makes them; the driver filters them itself
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
    files = run("clean", "--clean", "500:700:3")
    assert sorted(files) == sorted(list(without) + ["darwin.clean.tsv"])
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
    # the model chain: graph -> the cleaning rounds -> unitigs
    res = clean_model.clean(lens, g["reads"], g["arcs"], clip=clip, tip_reads=3, max_dist=50000, ratios=(500, 700, 3))
    print("--clean 500:700:3:", res["counts"])
    want_tsv = "".join("%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % ((j, clean_model.KINDS[int(s["kind"])]) + tuple(
        int(s[k]) for k in ("param", "reads_removed", "examined", "arcs_removed", "arcs_left"))) for j, s in enumerate(res["steps"]))
    assert files["darwin.clean.tsv"].decode() == want_tsv
    want = unitig_model.unitigs(lens, g["reads"], clean_model.cleaned(g["arcs"], res["arc_flags"]), clip=clip, tip_reads=3, seqs=rs.reads)
    seg, entries, links = _utg_gfa(tmp_path / "clean" / "darwin.utg.gfa")
    names = ["utg%06d%s" % (j + 1, "c" if u["circular"] else "l") for j, u in enumerate(want["unitigs"])]
    assert seg == [(names[j], want["seq"][int(u["seq_at"]):int(u["seq_at"] + u["length"])].tobytes().decode())
                   for j, u in enumerate(want["unitigs"])]
    for j, u in enumerate(want["unitigs"]):
        lay = want["layout"][int(u["layout_at"]):int(u["layout_at"] + u["n_reads"])]
        assert entries[j] == [(int(e["start"]), rs.names[e["vertex"] >> 1], int(clip[2 * (e["vertex"] >> 1)]),
                               int(clip[2 * (e["vertex"] >> 1) + 1]), "+-"[e["vertex"] & 1], int(e["take"])) for e in lay]
    assert links == [(names[a], sa, names[b], sb, ov) for a, sa, b, sb, ov in want["links"]]
    # not trivially so: arcs go, and the unitigs are fewer for it
    assert sum(res["counts"]["arcs_removed"]) > 0
    assert files["darwin.utg.gfa"] != without["darwin.utg.gfa"] and len(seg) < len(_utg_gfa(tmp_path / "utg" / "darwin.utg.gfa")[0])
    # refused before any file is read or any device is opened
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    for args in (("--gfa", "--clean", "500:700:3"), ("--gfa", "--unitigs", "0", "--clean", "500:700:3"), ("--unitigs", "3", "--clean", "500:700:3"),
                 ("--gfa", "--unitigs", "3", "--clean", "500:700"), ("--gfa", "--unitigs", "3", "--clean", "700:500:3"),
                 ("--gfa", "--unitigs", "3", "--clean", "500:1001:3"), ("--gfa", "--unitigs", "3", "--clean", "500:700:17"),
                 ("--gfa", "--unitigs", "3", "--clean", "500:700:3x"), ("--gfa", "--unitigs", "3", "--clean", "-1:700:3"),
                 ("--gfa", "--unitigs", "3", "--clean")):
        out = subprocess.run([drv, "missing.fasta", "missing.fasta", "1", "--device-dsoft"] + list(args), capture_output=True, text=True,
                             cwd=tmp_path, timeout=60, env=env)
        assert out.returncode == 1 and "--clean" in out.stderr, (args, out.stdout, out.stderr)
