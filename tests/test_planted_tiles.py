"""The planted-tile builder (tests/planted_tiles.py) does what it is for, under every configuration that
tests/test_gpu_planted_tiles.py runs: the CPU oracle's trace of a candidate holds the planted tile, the walks inside the planted
tiles are of every class a pass can get wrong, some leave the default band, and the rectangular shapes alone reach every shape of
the split pass's pointer phase.  These are conditions on the lists, asserted here so that the GPU file can rely on them."""
import numpy as np
import pytest

import planted_tiles as P

_IDS = ["%d/%d-%s" % (t, o, sc if isinstance(sc, str) else "%d,%d,%d,%d" % sc) for t, o, sc, _ in P.CONFIGS]


def _lists(oracle, tile, overlap, scoring, raw=False):
    return P.planted_lists(oracle, tile, overlap, P.resolve(scoring), raw)


def test_the_structural_sizes_are_those_of_the_lin_files():
    import test_gpu_lin_code_groups, test_gpu_lin_col_drift, test_gpu_lin_level_window, test_gpu_lin_rows
    union = set()
    for mod in (test_gpu_lin_rows, test_gpu_lin_code_groups, test_gpu_lin_col_drift, test_gpu_lin_level_window):
        union |= set(mod.SIZES)
    assert set(P.lin_sizes()) == union
    for x in (1, 17, 64, 120, 200, 208, 232, 304, 320):                # the generalised pass shape is the lin files' on squares
        assert P.pass_shape(x, x) == test_gpu_lin_code_groups.pass_shape(x)


def test_the_edge_sets_follow_the_rule():
    assert len(P.EDGE_320) == 36 and P.edge_set(320, 120) == P.EDGE_320
    for tile, overlap in sorted({(t, o) for t, o, _, _ in P.CONFIGS}):
        es = set(P.edge_set(tile, overlap))
        want = {1, 2, tile - 1, tile}
        for m in (overlap, tile - overlap):
            want |= {m - 1, m, m + 1}
        if P.has_split(tile, overlap) and P.W2 < tile:
            want |= {P.W2 - 1, P.W2, P.W2 + 1}
        assert want <= es and min(es) == 1 and max(es) == tile, (tile, overlap, sorted(want - es))


@pytest.mark.parametrize("raw", (False, True), ids=("clean", "raw"))
def test_lengths_are_exact_and_both_strands_hold_the_same_bases(raw):
    from gact_amd import synth
    pl = P.planted(320, 120, raw)
    assert len(pl.cf) == len(pl.cr) == len(pl.meta)
    n_raw = 0
    for k in range(len(pl.cf)):
        c, r, m = pl.cf[k], pl.cr[k], pl.meta[k]
        ref, query, qrc = (pl.rs.reads[int(i)] for i in (c["ref_id"], c["query_id"], r["query_id"]))
        assert (c["ref_id"], c["ref_pos"], c["query_pos"]) == (r["ref_id"], r["ref_pos"], r["query_pos"])
        assert np.array_equal(synth.revcomp(qrc), query)
        a, b, roff, qoff = P._planted_bytes(pl, k)
        assert (len(a), len(b)) == (m["R"], m["Q"])
        s = pl.anchors[1 - m["reverse"]]
        assert len(ref) == m["R"] + s and len(query) == m["Q"] + s
        anchor = ref[:s] if m["reverse"] else ref[m["R"]:]
        assert np.array_equal(anchor, query[:s] if m["reverse"] else query[m["Q"]:]) and set(anchor.tobytes()) <= set(b"ACGT")
        n_raw += bool(set(a + b) - set(b"ACGT"))
    if raw:
        assert n_raw == len(pl.cf)                                        # every planted tile holds N or lower-case bases
        assert any(set(P._planted_bytes(pl, k)[0]) & set(b"acgt") for k in range(len(pl.cf)))
    else:
        assert n_raw == 0


def _check_list(pl, kept, share, tile, overlap, all_present):
    for d in (0, 1):
        assert share[d] >= (1.0 if all_present else 0.95), (d, share)
        es = set(P.edge_set(tile, overlap))
        sel = kept.meta[kept.meta["reverse"] == d]
        assert es <= set(sel["R"].tolist()) and es <= set(sel["Q"].tolist()), d
    assert 2000 <= len(kept.cf) + len(kept.cr) <= 15000, len(kept.cf) + len(kept.cr)
    # every shape of the edge set's cross product, with at least two kinds
    kinds = {}
    for m in pl.meta:
        kinds.setdefault((int(m["reverse"]), int(m["R"]), int(m["Q"])), set()).add(str(m["kind"]))
    return kinds


@pytest.mark.parametrize("tile,overlap,scoring", [c[:3] for c in P.CONFIGS], ids=_IDS)
def test_the_planted_tile_is_in_the_oracles_trace(oracle, tile, overlap, scoring):
    pl = P.planted(tile, overlap)
    kept, walks, share = _lists(oracle, tile, overlap, scoring)
    assert all(w.present for w in walks) and len(walks) == len(kept.cf)
    kinds = _check_list(pl, kept, share, tile, overlap, all_present=(tile, overlap, scoring) == (320, 120, P.PLAIN))
    es = P.edge_set(tile, overlap)
    for d in (0, 1):
        few = [(r, q) for r in es for q in es if len(kinds.get((d, r, q), ())) < 2]
        assert not few, few[:10]


@pytest.mark.parametrize("tile,overlap,scoring", P.RAW_CONFIGS, ids=("plain", "affine"))
def test_the_raw_byte_lists(oracle, tile, overlap, scoring):
    kept, walks, share = _lists(oracle, tile, overlap, scoring, raw=True)
    _check_list(P.planted(tile, overlap, True), kept, share, tile, overlap, all_present=scoring == P.PLAIN)


@pytest.mark.parametrize("tile,overlap", [(t, o) for t, o, sc, _ in P.CONFIGS if sc == P.PLAIN], ids=lambda v: str(v))
def test_walks_of_every_class(oracle, tile, overlap):
    """under +1/-1/-1/-1: walks with both gap kinds, walks that end on a ZERO inside the tile, on a border, at the early-termination
    limit, and walks that never start (H = 0 at (R, Q)) -- each at least one planted tile in twenty"""
    kept, walks, _ = _lists(oracle, tile, overlap, P.PLAIN)
    n = float(len(walks))
    share = {"I and D": sum(w.n_i > 0 and w.n_d > 0 for w in walks) / n,
             "ZERO inside": sum(w.end == "zero" for w in walks) / n,
             "border": sum(w.end == "border" for w in walks) / n,
             "early termination": sum(w.end == "early" for w in walks) / n,
             "pos_score == 0": sum(w.pos_zero for w in walks) / n}
    print(tile, overlap, {k: round(v, 3) for k, v in share.items()})
    assert all(v >= 0.05 for v in share.values()), share


def test_walks_leave_the_default_band(oracle):
    kept, walks, _ = _lists(oracle, 320, 120, P.PLAIN)
    out = np.array([w.band > 48 for w in walks])
    assert out.mean() >= 0.01, out.mean()
    full = (kept.meta["R"] == 320) & (kept.meta["Q"] == 320)
    for d in (0, 1):
        assert (out & full & (kept.meta["reverse"] == d)).any(), d


def _linear(scoring):
    """open == extend == mismatch: the scorings the linear-gap pass takes (every such configuration here is within its guard)"""
    return isinstance(scoring, str) or scoring[1] == scoring[2] == scoring[3]


_LINEAR = [(i, c[:3]) for i, c in zip(_IDS, P.CONFIGS) if _linear(c[2]) and P.has_split(c[0], c[1])]


@pytest.mark.parametrize("tile,overlap,scoring", [c for _, c in _LINEAR], ids=[i for i, _ in _LINEAR])
def test_which_linear_gap_lists_leave_the_band(oracle, tile, overlap, scoring):
    """every list that the linear-gap pass runs holds walks that leave the default band -- but for the largest |g|: a walk
    more than 48 off the diagonal has made 49 gap moves more of one kind than of the other, which cost 49 |g|, and no path inside a
    tile scores more than match * tile"""
    sc = P.resolve(scoring)
    _, walks, _ = _lists(oracle, tile, overlap, scoring)
    can = 49 * -sc[3] < sc[0] * tile
    assert can == (scoring != "max-gap")
    assert any(w.band > 48 for w in walks) == can


def test_rectangles_alone_reach_every_shape_of_the_pointer_phase(oracle):
    kept, _, _ = _lists(oracle, 320, 120, P.PLAIN)
    for d in (0, 1):
        sel = kept.meta[(kept.meta["reverse"] == d) & (kept.meta["R"] != kept.meta["Q"])]
        rq = sorted(set(zip(sel["R"].tolist(), sel["Q"].tolist())))
        shapes = [P.pass_shape(r, q) for r, q in rq]
        # (the assertions of tests/test_gpu_lin_code_groups.py and tests/test_gpu_lin_level_window.py, which squares meet there)
        assert {n % 8 for n, _, _, _, _ in shapes} == set(range(8))
        assert {rem for _, _, _, _, rem in shapes} == set(range(8))
        assert any(off <= 0 for _, off, _, _, _ in shapes) and any(off > 0 for _, off, _, _, _ in shapes)
        assert any(both > 1 and r2 > 0 for _, _, both, r2, _ in shapes)              # whole blocks of both kinds
        assert any(both == 0 and r2 > 0 for _, _, both, r2, _ in shapes)             # only region-2 blocks
        assert any(both == 0 and r2 == 0 and n > 0 for n, _, both, r2, _ in shapes)  # no whole block at all
        assert {both + r2 for _, _, both, r2, _ in shapes} >= set(range(2, 9)) | {16, 17, 18}
        # and a rectangle is not a square in disguise: the pointer phase's length changes with Q at one R and with R at one Q
        for axis in (0, 1):
            steps = {}
            for sh, shape in zip(rq, shapes):
                steps.setdefault(sh[axis], set()).add(shape[0])
            assert sum(len(v) > 1 for v in steps.values()) >= 10, axis
