"""CPU suite for the bubble model (tests/bubble_model.py): the hand-made cases give what the rule in include/gact_hip.h says they
give, the checker of the rule's consequences passes on every case, the random graphs are not vacuous, and the unitigs of the
cleaned arcs run through every popped bubble.  The declarations of the header, the binding and a C compiler agree."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bubble_model
import unitig_model
from bubble_model import POPPED, LOST, FAILS, hand_made, pop_bubbles, check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FAIL = {name: i for i, name in enumerate(FAILS)}


def _run(name, skip=None, **kw):
    lens, reads, arcs, clip, info = hand_made(name)
    r = pop_bubbles(lens, reads, arcs, clip=clip, skip=skip, **kw)
    check(reads, arcs, r, skip=skip)
    c = r["counts"]
    assert c["sources"] == c["found"] + sum(c["by_fail"]) and c["found"] == c["popped"] + c["lost"] == len(r["bubbles"])
    assert c["reads_removed"] == int((r["read_bubble"] >= 0).sum()) and c["arcs_removed"] == int((r["arc_flags"] & 4).astype(bool).sum())
    return r, info, arcs


def _removed(r):
    return np.flatnonzero(r["read_bubble"] >= 0).tolist()


def _states(r):
    return {int(b["source"]): int(b["state"]) for b in r["bubbles"]}


def test_simple():
    r, info, arcs = _run("simple")
    s, t = info["s"], info["t"]
    assert _states(r) == {min(s, t ^ 1): POPPED, max(s, t ^ 1): LOST}
    # c's path is 100 bases shorter at the same arc count: b goes, with its four arcs
    assert _removed(r) == [info["b"] >> 1] and r["counts"]["arcs_removed"] == 4
    b = r["bubbles"][0]
    assert (b["n_vertices"], b["n_path"], b["n_removed"], b["path_len"]) == (4, 1, 1, 2100)
    assert b["sink"] == (t if b["source"] == s else s ^ 1)


def test_tie_the_lower_arc_wins():
    r, info, arcs = _run("tie")
    # b -> t is the lower arc, and b reaches t second: it replaces c's equal record
    assert info["b"] < info["c"] and _states(r)[info["s"]] == POPPED and _removed(r) == [info["c"] >> 1]


def test_more_reads_keeps_the_path_of_more_arcs_and_rule_b_takes_the_direct_arc():
    r, info, arcs = _run("more_reads")
    assert _removed(r) == [info["c"] >> 1]
    b = r["bubbles"][r["bubbles"]["state"] == POPPED][0]
    assert (b["n_vertices"], b["n_path"], b["n_removed"], b["path_len"]) == (5, 2, 1, 3000)
    s, t = info["s"], info["t"]
    gone = {(int(a["u"]), int(a["v"])) for a, f in zip(arcs, r["arc_flags"]) if f & 4}
    assert (s, t) in gone and (t ^ 1, s ^ 1) in gone and len(gone) == 6       # c's four arcs, the direct arc and its complement


def test_minus_pops_from_the_other_side():
    r, info, arcs = _run("minus")
    s, t = info["s"], info["t"]
    assert s & 1 and t & 1 and t ^ 1 < s
    assert _states(r) == {t ^ 1: POPPED, s: LOST} and r["bubbles"]["sink"][0] == s ^ 1


def test_beads_all_three_pop():
    r, info, arcs = _run("beads")
    c = r["counts"]
    assert (c["found"], c["popped"], c["lost"], c["reads_removed"]) == (6, 3, 3, 3)
    ends = {info["s"], info["m1"], info["m2"], info["t"]}
    for b in r["bubbles"]:
        assert {int(b["source"]) & ~1, int(b["sink"]) & ~1} <= {x & ~1 for x in ends}


@pytest.mark.parametrize("name", ["nested_in", "nested_out"])
def test_nested_the_owner_of_the_contested_reads_pops(name):
    r, info, arcs = _run(name)
    c = r["counts"]
    assert (c["found"], c["popped"], c["lost"]) == (4, 1, 3)
    b = r["bubbles"][0]
    assert b["source"] == 0 and b["state"] == POPPED
    if name == "nested_in":
        assert info["x0"] == 0 and b["n_vertices"] == 4 and len(_removed(r)) == 1 and _removed(r)[0] in (info["p"] >> 1, info["q"] >> 1)
    else:
        # the outer one keeps the branch with the inner bubble (four arcs against two): y goes, and one of p, q
        assert info["s"] == 0 and (b["n_vertices"], b["n_path"], b["n_removed"]) == (7, 3, 2) and info["y"] >> 1 in _removed(r)


def test_fans_at_the_limit_of_one_wave():
    r, info, arcs = _run("fan62")
    b = r["bubbles"]
    assert b["n_vertices"].tolist() == [64, 64] and b["state"].tolist() == [POPPED, LOST] and r["counts"]["reads_removed"] == 61
    r, info, arcs = _run("fan63")
    assert r["counts"]["found"] == 0 and r["counts"]["by_fail"][_FAIL["many"]] == 2
    r, info, arcs = _run("fan62", max_vertices=63)
    assert r["counts"]["found"] == 0 and r["counts"]["by_fail"][_FAIL["many"]] == 2
    r, info, arcs = _run("simple", max_vertices=3)
    assert r["counts"]["found"] == 0 and r["counts"]["by_fail"][_FAIL["many"]] == 2
    assert _run("simple", max_vertices=4)[0]["counts"]["popped"] == 1


def test_deep():
    r, info, arcs = _run("deep")
    b = r["bubbles"][0]
    assert (b["n_vertices"], b["n_path"], b["n_removed"], b["state"]) == (62, 30, 30, POPPED) and len(_removed(r)) == 30


def test_dist_at_and_over():
    # b's path reaches t at 2200: the longer of the two
    at = _run("simple", max_dist=2200)[0]
    assert at["counts"]["popped"] == 1 and at["counts"]["by_fail"] == [0] * 5
    over = _run("simple", max_dist=2199)[0]
    assert over["counts"]["found"] == 0 and over["counts"]["by_fail"][_FAIL["dist"]] == 2


def test_dead():
    r, info, arcs = _run("dead")
    # from s the dead end is popped; from t^1 the dead end's complement enters b^1 from outside; and b is a source itself
    assert r["counts"]["found"] == 0 and r["counts"]["by_fail"] == [1, 2, 0, 0, 0]
    skip = np.zeros(len(r["read_bubble"]), dtype=np.uint8)
    skip[info["extra"][0] >> 1] = 1
    r, info, arcs = _run("dead", skip=skip)
    assert r["counts"]["popped"] == 1 and _removed(r) == [info["b"] >> 1] and r["counts"]["working_arcs"] == len(arcs) - 2


def test_open():
    # as the model gives them: from s the arc from outside keeps b waiting (open), from t^1 its complement is a dead end, which
    # is b^1's second arc, so b^1 is a source too (dead)
    r, info, arcs = _run("open_in")
    assert r["counts"]["found"] == 0 and r["counts"]["by_fail"] == [1, 2, 0, 0, 0]
    r, info, arcs = _run("open_out")
    assert r["counts"]["found"] == 0 and r["counts"]["by_fail"] == [1, 2, 0, 0, 0]


def test_twice():
    r, info, arcs = _run("twice_cycle")
    assert r["counts"]["found"] == 0 and r["counts"]["by_fail"][_FAIL["twice"]] == 1 and r["counts"]["by_fail"] == [2, 1, 1, 0, 0]
    r, info, arcs = _run("twice_inversion")
    assert r["counts"]["found"] == 0 and r["counts"]["by_fail"][_FAIL["twice"]] == 1 and r["counts"]["by_fail"] == [3, 0, 1, 0, 0]


def test_flagged_arcs_are_not_of_the_working_set():
    r, info, arcs = _run("flagged")
    assert r["counts"]["sources"] == 0 and r["counts"]["working_arcs"] == len(arcs) - 4 and (r["arc_flags"] == arcs["flags"]).all()


def test_long_lens_path_len_past_two_to_the_31():
    r, info, arcs = _run("long_lens", max_dist=1 << 30)
    b = r["bubbles"]
    assert len(b) == 1 and b["state"][0] == POPPED and b["path_len"][0] == 3 * (1 << 30) - 5 > 1 << 31
    assert (b["n_vertices"][0], b["n_path"][0]) == (6, 3) and _removed(r) == [info["c"] >> 1]
    assert r["counts"]["arcs_removed"] == 8                 # c's four arcs, the short arcs s -> b2, s -> b3 and their complements


@pytest.mark.parametrize("name", ["chain64", "no_arcs"])
def test_graphs_without_a_branch(name):
    lens, reads, arcs, clip = unitig_model.hand_made(name)
    r = pop_bubbles(lens, reads, arcs, clip=clip)
    check(reads, arcs, r)
    assert r["counts"]["sources"] == 0 and len(r["bubbles"]) == 0 and (r["read_bubble"] == -1).all()
    assert r["arc_flags"].tolist() == arcs["flags"].tolist()


def test_no_reads():
    r = pop_bubbles(np.zeros(0, dtype=np.int32), unitig_model.plain_reads(0), unitig_model.make_arcs([]))
    assert len(r["bubbles"]) == 0 and len(r["read_bubble"]) == 0 and len(r["arc_flags"]) == 0 and r["counts"]["sources"] == 0


def test_refusals():
    lens, reads, arcs, clip, info = hand_made("simple")
    for kw in (dict(max_dist=0), dict(max_dist=(1 << 30) + 1), dict(max_vertices=2), dict(max_vertices=65)):
        with pytest.raises(ValueError):
            pop_bubbles(lens, reads, arcs, **kw)
    with pytest.raises(ValueError):
        pop_bubbles(lens, reads, arcs[1:])
    with pytest.raises(ValueError):
        pop_bubbles(lens, reads, arcs[::-1])


_RANDOM = {}


def _random(n, seed):
    if (n, seed) not in _RANDOM:
        lens, reads, arcs, clip = unitig_model.random_graph(n, seed)
        before = unitig_model.unitigs(lens, reads, arcs, clip=clip, tip_reads=3)
        _RANDOM[(n, seed)] = (lens, reads, arcs, clip, before)
    return _RANDOM[(n, seed)]


@pytest.mark.parametrize("n,seed,at_least,popped,with_skip", [(300, 3, 5, 5, 5), (300, 2, 5, 5, 5), (3000, 1, 50, 59, 58)])
def test_random_graphs(n, seed, at_least, popped, with_skip):
    lens, reads, arcs, clip, before = _random(n, seed)
    tips = before["places"]["state"] == unitig_model.TIP
    for skip, want in ((None, popped), (tips, with_skip)):
        r = pop_bubbles(lens, reads, arcs, clip=clip, skip=skip)
        check(reads, arcs, r, skip=skip)
        c = r["counts"]
        print(n, seed, skip is not None, c)
        assert c["popped"] >= at_least and c["popped"] == want and c["sources"] == c["found"] + sum(c["by_fail"])
    if (n, seed) == (3000, 1):
        c = pop_bubbles(lens, reads, arcs, clip=clip)["counts"]
        assert (c["found"], c["reads_removed"], c["arcs_removed"], c["working_arcs"]) == (118, 62, 252, 2336)


@pytest.mark.parametrize("name", ["simple", "beads"])
def test_unitigs_run_through_a_popped_bubble(name):
    r, info, arcs = _run(name)
    lens, reads = hand_made(name)[:2]
    before = unitig_model.unitigs(lens, reads, arcs, tip_reads=3)
    after = unitig_model.unitigs(lens, reads, bubble_model.cleaned(arcs, r["arc_flags"]), tip_reads=3)
    assert len(before["unitigs"]) >= 4 and len(after["unitigs"]) == 1
    assert after["unitigs"]["n_reads"][0] == len(lens) - r["counts"]["reads_removed"]
    assert np.flatnonzero(after["places"]["state"] == unitig_model.TIP).tolist() == _removed(r)
    chain = set(unitig_model.vertex_lists(after)[0])
    assert ({info["s"], info["t"]} <= chain) or ({info["s"] ^ 1, info["t"] ^ 1} <= chain)


def test_fewer_unitigs_on_the_large_random_graph():
    lens, reads, arcs, clip, before = _random(3000, 1)
    r = pop_bubbles(lens, reads, arcs, clip=clip, skip=before["places"]["state"] == unitig_model.TIP)
    after = unitig_model.unitigs(lens, reads, bubble_model.cleaned(arcs, r["arc_flags"]), clip=clip, tip_reads=3)
    print(len(before["unitigs"]), "->", len(after["unitigs"]))
    assert len(after["unitigs"]) < len(before["unitigs"])


# ---- the declarations: the header as a C compiler sees it, the binding, the model

def test_declarations_agree(tmp_path):
    from gact_amd import engine
    names = [n for n, _ in engine.BubbleStats._fields_]
    (tmp_path / "abi.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\nint main(void) { printf(\"%zu %zu %zu %zu\", sizeof(gact_bubble), "
        "offsetof(gact_bubble, path_len), sizeof(gact_bubble_params), sizeof(gact_bubble_stats));\n"
        + " ".join('printf(" %%zu", offsetof(gact_bubble_stats, %s));' % n for n in names)
        + ' printf(" %d %d %d %d %d\\n", GACT_GRAPH_ARC_BUBBLE, GACT_BUBBLE_DEFAULT_MAX_DIST, GACT_BUBBLE_MAX_VERTICES, '
        "GACT_BUBBLE_POPPED, GACT_BUBBLE_LOST); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "abi")]).split()]
    want = [32, engine.BUBBLE_DTYPE.fields["path_len"][1], ctypes.sizeof(engine.BubbleParams), ctypes.sizeof(engine.BubbleStats)] + \
        [getattr(engine.BubbleStats, n).offset for n in names] + \
        [engine.GRAPH_ARC_BUBBLE, engine.BUBBLE_DEFAULT_MAX_DIST, engine.BUBBLE_MAX_VERTICES, engine.BUBBLE_POPPED, engine.BUBBLE_LOST]
    assert got == want and engine.BUBBLE_DTYPE.itemsize == 32
    assert (engine.BUBBLE_POPPED, engine.BUBBLE_LOST, engine.GRAPH_ARC_BUBBLE) == (POPPED, LOST, bubble_model.BUBBLE_BIT)
    assert [n for n in engine.BUBBLE_DTYPE.names] == ["source", "sink", "n_vertices", "n_path", "n_removed", "state", "path_len"]
    # the statistics' fields are the model's counts, and the header declares them in the binding's order
    assert set(bubble_model.COUNTS) == set(names) - {"device_ms", "scratch_bytes"}
    txt = open(os.path.join(ROOT, "include", "gact_hip.h")).read()
    decl = re.search(r"typedef struct \{([^}]*)\} gact_bubble_stats;", txt).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", decl) == names
    assert "gact_hip_pop_bubbles" in engine.EXPORTS and "gact_hip_last_bubble_stats" in engine.EXPORTS
    assert callable(engine.Engine.pop_bubbles) and callable(engine.Engine.last_bubble_stats)
