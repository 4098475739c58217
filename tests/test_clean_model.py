"""The model of the weak-arc rule and of the cleaning rounds (tests/clean_model.py) on its hand-made graphs and on generated graphs
with repeats: what the header promises holds on every graph, the hand-made cases say what they were made to say, and on the
graphs with repeats the prune steps take every arc a repeat made, no arc of a true overlap, and leave fewer unitigs than tips and
bubbles alone.  No device."""
import numpy as np
import pytest

import bubble_model
import clean_model
import unitig_model
from clean_model import SHORT_BIT, clean, hand_made, prune

_REPEATS = {}


def _repeat(n):
    if n not in _REPEATS:
        _REPEATS[n] = clean_model.repeat_graph(n, 1)
    return _REPEATS[n]


def _removed(arcs, result):
    rows = list(zip(arcs["u"].tolist(), arcs["v"].tolist()))
    return sorted(rows[k] for k in np.flatnonzero(result["arc_flags"] & SHORT_BIT).tolist())


@pytest.mark.parametrize("name", clean_model.HAND_MADE)
def test_hand_made_prune(name):
    lens, reads, arcs, clip, info = hand_made(name)
    res = prune(lens, reads, arcs, clip=clip, skip=info["skip"])
    clean_model.check(reads, arcs, res["arc_flags"])
    rows = list(zip(arcs["u"].tolist(), arcs["v"].tolist()))
    assert sorted(rows[k] for k in res["weak"]) == sorted(info["weak"])
    assert _removed(arcs, res) == sorted(set(info["weak"]) | set((v ^ 1, u ^ 1) for u, v in info["weak"]))
    c = res["counts"]
    assert c["weak"] == len(info["weak"]) and c["arcs_removed"] == 2 * c["weak"]
    assert c["examined"] == dict(single=0, no_arcs=0, mirror_only=2).get(name, 1)
    if info["x"] is not None:
        want_best = dict(threshold=2000, mirror_only=2000, big_ov=2 ** 31 - 1, flagged=2000, skipped=2000, false_fork=clean_model.STRONG)
        assert res["vertex_best"][info["x"]] == want_best.get(name, 4000)
    # the stretch of x holds what the case says: positions in array order
    if name.startswith("fan"):
        n = int(name[3:])
        at = np.flatnonzero(arcs["u"] == info["x"])
        assert len(at) == n and (np.diff(at) == 1).all()
        weak_at = [k - at[0] for k in res["weak"]]
        assert weak_at == [j for j in (0, 63, 64, 128) if j < n - 1] and arcs["ov_u"][at[-1]] == 4000
    if name in ("flagged", "skipped"):
        at = np.flatnonzero(arcs["u"] == info["x"])
        assert arcs["ov_u"][at].tolist() == [2000, 10 ** 9, 1200, 10 ** 9, 900] and c["working_arcs"] == len(arcs) - 4


def test_threshold_is_strict():
    lens, reads, arcs, clip, info = hand_made("threshold")
    x = info["x"]
    for ratio, gone in ((500, [999]), (700, [1399, 1000, 999]), (0, []), (1000, [1400, 1399, 1000, 999])):
        res = prune(lens, reads, arcs, ratio_permille=ratio)
        assert sorted(arcs["ov_u"][k] for k in res["weak"]) == sorted(gone), ratio
        assert res["vertex_best"][x] == 2000


def test_mirror_only_takes_the_best_arc_of_its_vertex():
    lens, reads, arcs, clip, info = hand_made("mirror_only")
    res = prune(lens, reads, arcs)
    x = info["x"]
    k = [k for k in np.flatnonzero(arcs["u"] == x).tolist() if arcs["ov_u"][k] == res["vertex_best"][x]]
    assert len(k) == 1 and k[0] not in res["weak"] and res["arc_flags"][k[0]] == SHORT_BIT


def test_ratio_1000_keeps_the_ties_of_the_best():
    lens, reads, arcs, clip, info = hand_made("big_ov")
    res = prune(lens, reads, arcs, ratio_permille=1000)
    at = np.flatnonzero(arcs["u"] == info["x"])
    assert [int(arcs["ov_u"][k]) for k in at if k not in res["weak"]] == [2 ** 31 - 1] * 2 and res["counts"]["weak"] == 2
    lens, reads, arcs, clip = unitig_model.random_graph(300, 1)
    none = prune(lens, reads, arcs, clip=clip, ratio_permille=0)
    assert none["counts"]["weak"] == 0 and (none["arc_flags"] == arcs["flags"]).all() and none["counts"]["examined"] > 0
    res = prune(lens, reads, arcs, clip=clip, ratio_permille=1000)
    assert res["counts"]["weak"] > 0
    clean_model.check(reads, arcs, res["arc_flags"])


def test_refusals():
    lens, reads, arcs, clip, info = hand_made("false_fork")
    for bad in (-1, 1001):
        with pytest.raises(ValueError):
            prune(lens, reads, arcs, ratio_permille=bad)
    for kw in (dict(tip_reads=0), dict(max_dist=0), dict(max_vertices=2), dict(ratios=(-1, 700, 3)), dict(ratios=(500, 1001, 3)),
               dict(ratios=(700, 500, 3)), dict(ratios=(500, 700, 17)), dict(ratios=(500, 700, -1)), dict(max_passes=0), dict(max_passes=17)):
        with pytest.raises(ValueError):
            clean(lens, reads, arcs, **kw)
    with pytest.raises(ValueError):
        prune(lens, reads, arcs[1:])
    with pytest.raises(ValueError):
        clean(lens, reads, arcs[::-1])


def test_ratios():
    assert clean_model.ratios_of(500, 700, 3) == [500, 600, 700] and clean_model.ratios_of(500, 700, 1) == [500]
    assert clean_model.ratios_of(500, 700, 0) == [] and clean_model.ratios_of(500, 701, 4) == [500, 567, 634, 701]


@pytest.mark.parametrize("name", clean_model.HAND_MADE + ("simple", "beads", "nested_in", "nested_out"))
def test_hand_made_clean(name):
    g = hand_made(name) if name in clean_model.HAND_MADE else bubble_model.hand_made(name)
    lens, reads, arcs, clip = g[:4]
    res = clean(lens, reads, arcs, clip=clip)
    clean_model.check(reads, arcs, res["arc_flags"], res["steps"], res["read_state"])
    steps = res["steps"]
    assert steps["kind"][:2].tolist() == [clean_model.TIPS, clean_model.BUBBLES] and len(steps) <= 4 * 9
    assert res["counts"]["steps"] == len(steps) and res["counts"]["arcs_left"] == steps["arcs_left"][-1]
    if name == "false_fork":
        # the weak arc is no tip and no bubble: only the prune step takes it, and one unitig more becomes whole
        alone = clean(lens, reads, arcs, ratios=(500, 700, 0))
        assert alone["counts"]["arcs_removed"] == [0, 0, 0] and res["counts"]["arcs_removed"] == [0, 0, 2]
        before = unitig_model.unitigs(lens, reads, arcs)["counts"]["unitigs"]
        after = unitig_model.unitigs(lens, reads, clean_model.cleaned(arcs, res["arc_flags"]))["counts"]["unitigs"]
        assert (before, after) == (3, 2)
    if name.startswith("nested"):
        # nested_in: the inner bubble owns the contested reads and the outer one waits for the second pass.  nested_out: the outer
        # bubble owns them, pops in the first pass and takes the inner one's losing branch with it (the bubble rule, which does
        # not change), so one pass leaves what four leave
        one = clean(lens, reads, arcs, max_passes=1)
        if name == "nested_in":
            assert one["counts"]["arcs_left"] > res["counts"]["arcs_left"] and res["counts"]["passes"] >= 2
        else:
            assert one["counts"]["arcs_left"] == res["counts"]["arcs_left"]
        assert unitig_model.unitigs(lens, reads, clean_model.cleaned(arcs, res["arc_flags"]))["counts"]["unitigs"] == 1


def test_steps_fit_the_promised_room():
    lens, reads, arcs, clip, info = hand_made("threshold")
    for ratios, passes in (((500, 700, 3), 4), ((0, 1000, 16), 1), ((500, 500, 2), 2)):
        res = clean(lens, reads, arcs, ratios=ratios, max_passes=passes)
        assert len(res["steps"]) <= (ratios[2] + 1) * (2 * passes + 1)
        clean_model.check(reads, arcs, res["arc_flags"], res["steps"], res["read_state"])


@pytest.mark.parametrize("n", [300, 1000, 3000])
def test_repeats_are_resolved_by_the_prune_steps(n):
    lens, reads, arcs, clip, repeat_records = _repeat(n)
    res = clean(lens, reads, arcs, clip=clip)
    clean_model.check(reads, arcs, res["arc_flags"], res["steps"], res["read_state"])
    of_repeat = np.isin(arcs["record"], sorted(repeat_records))
    assert (of_repeat & (arcs["flags"] == 0)).any()
    assert not (of_repeat & (res["arc_flags"] == 0)).any(), "an arc of a repeat-only record is left"
    assert not (~of_repeat & ((res["arc_flags"] & SHORT_BIT) != 0)).any(), "an arc of a true overlap is marked short"
    alone = clean(lens, reads, arcs, clip=clip, ratios=(500, 700, 0))
    with_prune = unitig_model.unitigs(lens, reads, clean_model.cleaned(arcs, res["arc_flags"]), clip=clip)["counts"]
    without = unitig_model.unitigs(lens, reads, clean_model.cleaned(arcs, alone["arc_flags"]), clip=clip)["counts"]
    raw = unitig_model.unitigs(lens, reads, arcs, clip=clip)["counts"]
    print(n, "unitigs / longest: raw %d / %d, tips + bubbles %d / %d, with the prune steps %d / %d" %
          (raw["unitigs"], raw["longest_bases"], without["unitigs"], without["longest_bases"], with_prune["unitigs"],
           with_prune["longest_bases"]), res["counts"])
    assert with_prune["unitigs"] < without["unitigs"]


def test_rounds_alone_help_a_graph_without_repeats():
    lens, reads, arcs, clip = unitig_model.random_graph(3000, 1)
    res = clean(lens, reads, arcs, clip=clip)
    clean_model.check(reads, arcs, res["arc_flags"], res["steps"], res["read_state"])
    before = unitig_model.unitigs(lens, reads, arcs, clip=clip)["counts"]["unitigs"]
    after = unitig_model.unitigs(lens, reads, clean_model.cleaned(arcs, res["arc_flags"]), clip=clip)["counts"]["unitigs"]
    print("random_graph(3000, 1): %d unitigs, %d behind the rounds" % (before, after), res["counts"])
    assert after < before


def test_exports_and_dtypes():
    from gact_amd import engine
    for name in ("gact_hip_prune_overlaps", "gact_hip_last_prune_stats", "gact_hip_clean_graph", "gact_hip_last_clean_stats"):
        assert name in engine.EXPORTS
    assert engine.CLEAN_STEP_DTYPE.itemsize == 32 and engine.CLEAN_READ_DTYPE.itemsize == 8
    assert (engine.GRAPH_ARC_TIP, engine.GRAPH_ARC_SHORT) == (clean_model.TIP_BIT, clean_model.SHORT_BIT)
    assert engine.CLEAN_KINDS == clean_model.KINDS
