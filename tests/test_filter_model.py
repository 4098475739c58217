"""CPU suite: the filter of an overlap set by identity, span and each read's best (tests/filter_model.py, written from the rule
in include/gact_hip.h) on hand-made records for every edge of the rule, on truth block B (the false hits go, and what is left
is block A's graph) and on truth block P (the decoy's records go by the relative rule alone), and the teeth: four misreadings
a kernel and a model could share each make a named assertion fail.  tests/test_gpu_filter.py holds the device to the model."""
import numpy as np
import pytest

import filter_model as fm
import test_truth_model as ttm
import truth_checks as tc


def check_hand_cases():
    """every hand-made case against the reasons and the table rows written beside it"""
    for name, (rec, sums, kw, why, rows) in fm.hand_cases().items():
        out = fm.filter_overlaps(rec, sums, **kw)
        assert out["why"].tolist() == why, "%s: the reasons are %s, not %s" % (name, out["why"].tolist(), why)
        for x, row in rows.items():
            assert tuple(out["reads"][x].tolist()) == row, "%s: the table's row %d is %s, not %s" % (name, x, out["reads"][x], row)
        sel = kw.get("sel")
        kept = [k for k, w in enumerate(why) if w == fm.KEPT]
        assert out["kept_at"].tolist() == kept and out["kept_sel"].tolist() == [int(sel[k]) if sel is not None else k for k in kept], name
    rec, sums, kw, _, _ = fm.hand_cases()["span"]
    out = fm.filter_overlaps(rec, sums, **kw)
    assert out["t_span"].tolist() == [90, 110, 100, 100], "span: the target's span counts the deleted bases, not the inserted ones"
    assert out["q_span"].tolist() == [110, 90, 100, 110], "span: the query's span counts the inserted bases, not the deleted ones"


def test_hand_made_edges():
    check_hand_cases()
    names = set(fm.hand_cases())
    assert {"threshold", "empty_and_not_emitted", "span", "relative_at", "relative_chain", "best_of_passed", "side_ref", "side_query",
            "side_both", "self"} <= names


def test_refusals_and_empty_inputs():
    rec, sums, kw, _, _ = fm.hand_cases()["relative_chain"]
    for bad, code in ((dict(min_identity=-1), "EINVAL"), (dict(min_identity=1001), "EINVAL"), (dict(min_span=-1), "EINVAL"),
                      (dict(max_drop=-1), "EINVAL"), (dict(max_drop=1001), "EINVAL"), (dict(sides=0), "EINVAL"), (dict(sides=4), "EINVAL"),
                      (dict(n_reads=-1), "EINVAL"), (dict(n_reads=0), "EINVAL"), (dict(sel=np.array([0, 4, 1, 2])), "EINVAL"),
                      (dict(sel=np.array([0, -1, 1, 2])), "EINVAL"), (dict(n_reads=3), "ERANGE"), (dict(read_first=1), "ERANGE")):
        with pytest.raises(fm.Refused) as info:
            fm.filter_overlaps(rec, sums, **dict(kw, **bad))
        assert info.value.code == code, bad
    with pytest.raises(fm.Refused):
        fm.filter_overlaps(rec, None, **kw)
    # a record that is not counted may name any read
    far = rec.copy()
    far["ref_id"][1], far["emitted"][1] = 99, 0
    assert fm.filter_overlaps(far, sums, **kw)["why"].tolist()[1] == fm.NOT_EMITTED
    # without a window nothing is looked up, and an empty selection keeps nothing
    out = fm.filter_overlaps(rec, sums, min_identity=800, max_drop=1000)
    assert out["why"].tolist() == [fm.KEPT, fm.KEPT, fm.IDENTITY, fm.KEPT] and len(out["reads"]) == 0
    out = fm.filter_overlaps(rec, sums[:0], sel=np.zeros(0, dtype=np.int32), n_reads=4)
    assert len(out["kept_at"]) == 0 and not out["reads"].view(np.int32).any()


def test_random_sets_hold_every_reason():
    """the crafted random sets the device is compared on are about something: every reason occurs in them"""
    seen = set()
    for n in fm.SIZES:
        rec, sums, kw = fm.random_case(n)
        out = fm.filter_overlaps(rec, sums, **kw)
        seen |= set(out["why"].tolist())
        assert len(out["why"]) == n and int(out["reads"]["n_kept"].sum()) == 2 * len(out["kept_at"])
    assert seen == set(range(6))


def _identity_of_the_aligned_pairs(n_eq, n_x, ins, dele):
    return 1000 * n_eq // (n_eq + n_x) if n_eq + n_x else 0


TEETH = {"identity_over_matches_and_mismatches_only": ("identity", _identity_of_the_aligned_pairs, "threshold: the reasons"),
         "ins_and_del_exchanged_in_the_spans": ("spans", lambda n_eq, n_x, ins, dele: (n_eq + n_x + ins, n_eq + n_x + dele),
                                                "the target's span counts the deleted bases"),
         "best_over_all_counted_records": ("towards_best", lambda why: why not in (fm.NOT_EMITTED, fm.EMPTY), "best_of_passed: the reasons"),
         "relative_on_the_ref_side_only_under_both": ("relative_sides", lambda sides: fm.REF if sides == fm.BOTH else sides,
                                                      "relative_chain: the reasons"),
         "relative_on_the_query_side_only_under_both": ("relative_sides", lambda sides: fm.QUERY if sides == fm.BOTH else sides,
                                                        "relative_chain: the reasons")}


@pytest.mark.parametrize("name", sorted(TEETH))
def test_a_misreading_makes_the_named_assertion_fail(monkeypatch, name):
    what, wrong, message = TEETH[name]
    monkeypatch.setattr(fm, what, wrong)
    with pytest.raises(AssertionError, match=message):
        check_hand_cases()


# ---- truth block B: the false hits go, and what is left is block A's graph

_B = {}


def filtered_block_b(oracle):
    """block B's reference path, its selection filtered at 650, and the stages behind it again; computed once"""
    if "b" not in _B:
        p = ttm.reference_path(oracle, "B")
        out = fm.filter_overlaps(p["records"], p["sums"], sel=p["sel"], min_identity=650, sides=fm.BOTH, n_reads=p["rs"].n)
        sel2, sums2 = out["kept_sel"], p["sums"][out["kept_at"]]
        _B["b"] = dict(p=p, out=out, sel=sel2, sums=sums2, stages=ttm.graph_stages(p["rs"], p["records"], sel2, sums2))
    return _B["b"]


def kept_arcs(arcs):
    """the kept arcs as the sorted multiset of (u, v, len)"""
    kept = arcs[arcs["flags"] == 0]
    return sorted(zip(kept["u"].tolist(), kept["v"].tolist(), kept["len"].tolist()))


def test_block_b_filtered_is_block_a(oracle):
    b, a = filtered_block_b(oracle), ttm.reference_path(oracle, "A")
    p, out, g = b["p"], b["out"], b["stages"]
    hits, _ = tc.false_hits(p["rs"], p["cands"], p["nf"])
    emitted = [i for i in p["sel"].tolist() if p["records"]["emitted"][i]]
    n_false = sum(i in hits for i in emitted)
    ident = out["ident"][[k for k, i in enumerate(p["sel"].tolist()) if p["records"]["emitted"][i]]]
    is_false = np.array([i in hits for i in emitted])
    print("block B: %d selected and emitted, %d false (identity %d to %d), %d true (%d to %d); kept at 650: %d" % (
        len(emitted), n_false, ident[is_false].min(), ident[is_false].max(), len(emitted) - n_false, ident[~is_false].min(),
        ident[~is_false].max(), len(b["sel"])))
    assert n_false > 0, "block B holds no false record"
    assert len(b["sel"]) == len(emitted) - n_false == 578
    assert not any(i in hits for i in b["sel"].tolist()), "a false hit was kept"
    for t in (600, 700):
        other = fm.filter_overlaps(p["records"], p["sums"], sel=p["sel"], min_identity=t)
        assert other["kept_sel"].tolist() == b["sel"].tolist(), "the kept set at %d is not the one at 650" % t
    for what, arcs in (("the graph's", g["arcs"]), ("the cleaned", g["cleaned"])):
        wrong = tc.arcs(p["rs"], arcs, g["clip"], law=p["law"], count_only=True)
        print("block B filtered, %s arcs: %d kept, %d wrong" % (what, int((arcs["flags"] == 0).sum()), wrong))
        assert wrong == 0
    assert kept_arcs(g["arcs"]) == kept_arcs(a["arcs"]), "the filtered block B's kept arcs are not block A's"
    for k in (0, 3):
        print("block B filtered, reads per unitig at tip_reads %d:" % k, g["utg"][k]["unitigs"]["n_reads"].tolist(),
              "block A's:", a["utg"][k]["unitigs"]["n_reads"].tolist())
    assert sorted(g["utg"][3]["unitigs"]["n_reads"].tolist()) == sorted(a["utg"][3]["unitigs"]["n_reads"].tolist())


# ---- truth block P: the decoy's records go by the relative rule alone

P_MAX_DROP = 26


def block_p_filtered(p, **kw):
    return fm.filter_overlaps(p["records"], p["sums"], min_identity=0, sides=fm.QUERY, n_reads=p["rs"].n, **kw)


def test_block_p_the_decoy_goes_by_the_relative_rule(oracle):
    p = ttm.reference_path_p(oracle)
    on_decoy = p["records"]["ref_id"] == p["decoy"]
    out = block_p_filtered(p, max_drop=P_MAX_DROP)
    under = out["reads"]["best_permille"][p["records"]["query_id"]] - out["ident"]
    counted = out["why"] != fm.NOT_EMITTED
    print("block P: %d records on the decoy (identity %d to %d, at least %d under their read's best), %d others (%d to %d, at most %d "
          "under)" % (int(on_decoy.sum()), out["ident"][on_decoy].min(), out["ident"][on_decoy].max(), under[on_decoy].min(),
                      int((~on_decoy).sum()), out["ident"][~on_decoy & counted].min(), out["ident"][~on_decoy & counted].max(),
                      under[~on_decoy & counted].max()))
    assert counted.all() and (out["why"] != fm.EMPTY).all(), "block P holds a record that is not counted"
    assert on_decoy.sum() == 15 and (~on_decoy).sum() == 76
    assert (out["why"][on_decoy] == fm.RELATIVE).all(), "a record on the decoy was kept"
    assert (out["why"][~on_decoy] == fm.KEPT).all(), "a record on a true contig was dropped"
    assert under[~on_decoy].max() <= P_MAX_DROP < under[on_decoy].min()
    assert (block_p_filtered(p, max_drop=1000)["why"] == fm.KEPT).all()
