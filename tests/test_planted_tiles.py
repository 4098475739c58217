"""The planted-tile builder (tests/planted_tiles.py) does what it is for, under every configuration that
tests/test_gpu_planted_tiles.py runs: the CPU oracle's trace of a candidate holds the planted tile, the walks inside the planted
tiles are of every class a pass can get wrong, some leave the default band, and the rectangular shapes alone reach every shape of
the split pass's pointer phase.  The geometry table (planted_tiles.GEOMETRIES) is held to the engine's plans, to the window starts
it is there to cover and to the same conditions on its lists.  These are conditions on the lists, asserted here so that the GPU
file can rely on them."""
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


@pytest.mark.parametrize("tile,overlap,scoring", P.RAW_CONFIGS, ids=("plain", "affine", "317/119-plain"))
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


# ---------------------------------------------------------------------------------------------------------------------
# the geometry table (planted_tiles.GEOMETRIES)
_GEO_IDS = ["%d/%d" % (g.tile, g.overlap) for g in P.GEOMETRIES]
# sha256 of cf, cr and the concatenated reads of the lists that were there before the table: the geometry-aware threshold and the
# unpadded shapes of the table's rows leave the older lists as they were, byte for byte
_UNCHANGED = {
    (320, 120, False): ("9febfb742dd43d4026b420866bd4a71bbebc61333f5167e3094038535de976cd",
                        "53fd020a7d848a5fd96b0e945c3ba840eec42f11c451feff714dfcdfbab9986b",
                        "df00f5470f0974ec3a6515c53bbc0cd84570f78f3618b940c6da1ec352243e75"),
    (64, 8, False): ("8b63c76dc30e4784f60d03d4ab1d6259ed218a0c4d01662f21f2dc00c3b562f5",
                     "b9bf41f91689fe8aaf327c0b4342a58965857ce7fc09195d0bb8d7017e48543a",
                     "c05adf782c8793e1858e969f13a6585cba706675fbe2211a1afcb7ed8e26a24e"),
    (128, 32, False): ("a0fe385b941cdd4475c0c456f4a49fff9ea124b9520b345cdf334ac3bfdd6aba",
                       "a4ab3015b359acd389d297eaccbf2e4a54580ae0980c0d7c1a071c3ac88c9c0c",
                       "5b88e72e42f952b9281682f1ba31491bb6b9455e919a11bfd812553a65cab15f"),
    (320, 100, False): ("9b5972f7cf7c910fc59bdb2ceb02fa6479404eb121a8c9aa3ed8fc11549c6889",
                        "4a372fc9eb6af99e1677620e123096b88cb73ccc16eb1fc3e37f502b26f29f1f",
                        "5f66af2055223056e8956bbebe858fe11034177f78925c9b56c20b79e8fd38cd"),
    (512, 128, False): ("bac9ac21ed06267aa40d044aa149aa6870585c3584d144d634f8120baea5658c",
                        "e1c205b133ab903a3a30d5abd2a2302b7f6c70be24f28cb3a7d66987a4cbc938",
                        "e12901c3ada1b061dfaf2883d3da92224dae7625a2678c0426c5f118f6e2033e"),
    (320, 120, True): ("6c0ad49681e35931a5ad3c695595450892423e5968c533a5a7c33e4e7b1f2469",
                       "4b0313bc36c244b3b327c72ca32e4768dfe167c55999105349ddfbd98a932afa",
                       "efaf9bbdebdc91366446441fa1c23c4f183fc9dc968a9882d3c11a98db412014"),
}


def test_the_older_lists_are_unchanged():
    import hashlib
    assert {k[:2] for k in _UNCHANGED} == {c[:2] for c in P.CONFIGS}
    for (tile, overlap, raw), want in _UNCHANGED.items():
        pl = P.planted(tile, overlap, raw)
        got = tuple(hashlib.sha256(x).hexdigest() for x in (pl.cf.tobytes(), pl.cr.tobytes(), np.concatenate(pl.rs.reads).tobytes()))
        assert got == want, (tile, overlap, raw)
    for tile, overlap, scoring, _ in P.CONFIGS:                          # every one of them has an anchor of 56 bases or more
        assert P.default_threshold(P.resolve(scoring), tile, overlap) == 35 * max(P.resolve(scoring)[0], 1)
    assert P.default_threshold(P.AFFINE, 320, 307) == 26 and P.default_threshold(P.PLAIN, 1, 0) == 1


def test_the_geometry_table_is_the_one_agreed():
    """the rows, and what the engine's geometry conditions (derive_kernel_flags) make of them, restated"""
    geo = [(g.tile, g.overlap) for g in P.GEOMETRIES]
    assert len(geo) == len(set(geo)) == 27 and not set(geo) & {c[:2] for c in P.CONFIGS}
    for g in P.GEOMETRIES:
        assert 1 <= g.tile <= 512 and 0 <= g.overlap < g.tile
        split = g.tile <= 320 and g.tile - g.overlap <= 208
        assert P.has_split(g.tile, g.overlap) == split
        assert (g.plain, g.affine) == ((P.LIN, P.AFF) if split else (P.UNI, P.UNI)), g
    # both sides of each boundary
    for a, b in (((320, 112), (320, 111)), ((208, 0), (209, 0)), ((320, 112), (321, 113)), ((320, 125), (321, 121))):
        assert a in geo and b in geo and P.has_split(*a) and not P.has_split(*b)
    assert any(t % 8 for t, _ in geo) and min(t for t, _ in geo) == 1 and any(t < P.C2 for t, _ in geo)


@pytest.mark.parametrize("g", P.GEOMETRIES, ids=_GEO_IDS)
def test_the_plan_of_every_geometry(g):
    """engine.plan (no device): the main kernel of a large list is the row's, under both scorings; a short list gets the wide
    layout wherever the tile is at most 320"""
    from gact_amd import engine
    for scoring, main, wide in ((P.PLAIN, g.plain, P.WIDE_LIN), (P.AFFINE, g.affine, P.WIDE_TAG)):
        kw = dict(tile_size=g.tile, tile_overlap=g.overlap, scoring=scoring, threshold=P.default_threshold(scoring, g.tile, g.overlap))
        assert engine.plan(50000, **kw)["main_kernel"] == main, (g, scoring)
        assert engine.plan(100, **kw)["main_kernel"] == (wide if g.tile <= 320 else P.UNI), (g, scoring)


def test_the_split_rows_cover_the_window_starts():
    """the lane and the column of region 2 at which the pointer window begins follow from tile - overlap alone (209 - early), so
    only the table's rows move them: a lane's first, second and last column, the lanes 12 to 15"""
    split = [g for g in P.GEOMETRIES if P.has_split(g.tile, g.overlap)]
    starts = {P.window_start(g.tile, g.overlap) for g in split}
    assert set(P.WINDOW_STARTS) <= starts, sorted(set(P.WINDOW_STARTS) - starts)
    assert {(0, 0), (0, 12), (1, 0)} <= starts and any(lane >= 12 for lane, _ in starts)
    for g in split:
        early = g.tile - g.overlap
        es = P.edge_set(g.tile, g.overlap)
        for R in es:
            for Q in es:
                step, lane, col = P.split_first_pointer_step(R, Q, early)
                # (pass_shape restates the same step: its second value is the first pointer step minus (T_end - LAG))
                assert step - (R + (P.K_GROUP - 1) + P.K_GROUP - P.LAG) == P.pass_shape(R, Q, g.tile, g.overlap)[1]
                if Q > early:                                    # R and Q do not move the window's start ...
                    assert (lane, col) == P.window_start(g.tile, g.overlap) and step == max(1, R - early + 1) + lane + P.K_GROUP
                else:                                            # ... a tile narrower than the window starts on its own first column
                    assert (lane, col) == ((P.W2 - Q) // P.C2, (P.W2 - Q) % P.C2)
    for tile, overlap in ((320, 120), (320, 200), (128, 32), (64, 8)):   # the four starts there were: none of the above
        assert P.window_start(tile, overlap) not in P.WINDOW_STARTS


def _left_floor(g):
    """share of the left phase's candidates whose planted tile the oracle's trace must hold.  The left phase's anchor is
    tile - overlap bases long, and the first tile's maximum is its corner only if the anchor scores more than the planted tile's
    own best cell loses on the way to (R, Q): under a full tile, an anchor of a lane's 13 bases or fewer wears thin.  Measured
    (PLAIN, AFFINE): 320/294 0.989, 0.958; 320/307 0.968, 0.949; 320/308 0.965, 0.932; 320/319 0.655, 0.491; every other row 1.0"""
    return {(320, 307): 0.90, (320, 308): 0.90, (320, 319): 0.45}.get((g.tile, g.overlap), 0.95)


@pytest.mark.parametrize("g", P.GEOMETRIES, ids=_GEO_IDS)
def test_the_planted_tile_is_in_the_oracles_trace_at_every_geometry(oracle, g):
    pl = P.planted(g.tile, g.overlap)
    es = P.edge_set(g.tile, g.overlap)
    assert 4 <= len(pl.cf) <= 5200 and len(pl.cf) == len(pl.cr) and (len(pl.cf) >= 4 * len(es) ** 2)
    for scoring in (P.PLAIN, P.AFFINE):
        kept, walks, share = P.planted_lists(oracle, g.tile, g.overlap, scoring)
        print("%d/%d %s: left phase %.3f, right phase %.3f of %d" % (g.tile, g.overlap, scoring, share[0], share[1], len(pl.cf) // 2))
        assert all(w.present for w in walks) and len(walks) == len(kept.cf)
        assert share[1] == 1.0 and share[0] >= _left_floor(g), (g, scoring, share)
        for d in (0, 1):                                         # every size of the edge set, as rows and as columns, both ways
            sel = kept.meta[kept.meta["reverse"] == d]
            assert set(es) <= set(sel["R"].tolist()) and set(es) <= set(sel["Q"].tolist()), (g, scoring, d)
    kinds = {}
    for m in pl.meta:
        kinds.setdefault((int(m["reverse"]), int(m["R"]), int(m["Q"])), set()).add(str(m["kind"]))
    assert all(len(kinds.get((d, r, q), ())) >= 2 for d in (0, 1) for r in es for q in es)


_WALK_ROWS = [g for g in P.GEOMETRIES if g.tile - g.overlap >= 26 and g.tile >= 100]


@pytest.mark.parametrize("g", _WALK_ROWS, ids=["%d/%d" % (g.tile, g.overlap) for g in _WALK_ROWS])
def test_walks_of_every_class_at_every_geometry(oracle, g):
    """test_walks_of_every_class's one in twenty for walks that end on a ZERO inside the tile, on a border, and at the
    early-termination limit -- but where tile - overlap is the whole tile: no walk is longer than its tile"""
    _, walks, _ = P.planted_lists(oracle, g.tile, g.overlap, P.PLAIN)
    n = float(len(walks))
    share = {end: sum(w.end == end for w in walks) / n for end in ("zero", "border", "early")}
    print(g.tile, g.overlap, {k: round(v, 3) for k, v in share.items()})
    assert share["zero"] >= 0.05 and share["border"] >= 0.05, share
    if g.overlap == 0:
        assert share["early"] == 0, share
    else:
        assert share["early"] >= 0.05, share


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
