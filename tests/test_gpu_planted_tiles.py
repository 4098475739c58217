"""GPU: every packed int16 pass on arbitrary R x Q tiles, through planted tiles (tests/planted_tiles.py).

tests/test_gpu_tiles.py gives tiles of any shape and content to the int32 pass only; the packed passes run inside chains, and the
chain tests reach the structural tile sizes with square exact copies, whose walk is the main diagonal.  A planted tile is a non-first
tile of a chosen R x Q and content inside a chain: rectangles (the split pass's schedule depends on R and Q separately), clamped
cells on the walk and where it ends (zero levels), I and D codes and ties at the block hand-overs (pointer codes), walks that
leave the band, and lane partners of like and unlike size.  tests/test_planted_tiles.py holds the lists to that on the CPU.

Every configuration of planted_tiles.CONFIGS runs the geometry's list through each of its layouts and compares every record field
with the oracle (oracle.gact_many); every run asserts from last_run_stats() that the pass meant is the one that ran.  Every row of
planted_tiles.GEOMETRIES does the same with its own list: the tile geometries at which the kernel family, the split pass's pointer
window or the fill of the last lane change."""
import numpy as np
import pytest

import planted_tiles as P
from test_gpu_int16_edges import LAYOUTS, _SWITCHES, _check_stats, _kind
from test_gpu_lin_code_groups import _same          # (it compares every field of FIELDS)

pytestmark = pytest.mark.gpu

_CASES = [(t, o, sc, lay) for t, o, sc, lays in P.CONFIGS for lay in lays]
_IDS = ["%d/%d-%s-%s" % (t, o, sc if isinstance(sc, str) else "%d,%d,%d,%d" % sc, lay) for t, o, sc, lay in _CASES]


def _expected_stats(tile, overlap, scoring, layout):
    """what last_run_stats() must say (tests/test_gpu_int16_edges.py's _expected_stats, from the engine's plan of a large list)"""
    from gact_amd import engine
    main = engine.plan(50000, tile_size=tile, tile_overlap=overlap, scoring=scoring,
                       threshold=P.default_threshold(scoring, tile, overlap))["main_kernel"]
    kind = "plain" if layout == "plain" else _kind(main)
    uniform = main.startswith("Uniform") or layout == "uniform"
    lin = kind == "lin" and not uniform
    return {"packed16": True,
            "layout": "packed16-wide" if layout == "wide" else "packed16-uniform" if uniform else "packed16-split",
            "tagged_pointers": kind in ("lin", "aff", "tag"),
            "linear_gap": lin,
            "lin_row_drift": lin and scoring[0] - 2 * scoring[3] > 63,          # lin_col_drift_ok, csrc/gact_lin.hpp 12.
            "affine_drift": kind == "aff" and layout == "split",
            "coop_walks": layout == "coop"}


_SEQS, _WANT = {}, {}


def _seqs(pl):
    key = id(pl.rs)
    if key not in _SEQS:
        _SEQS[key] = pl.rs.concat() + pl.rs.concat(rc=True)
    return _SEQS[key]


def _records(oracle, pl, tile, overlap, scoring, raw=False):
    """the oracle's records of a list under one scoring, forward candidates then reverse-complement ones: computed once, shared by
    every layout"""
    key = (tile, overlap, scoring, raw)
    if key not in _WANT:
        cat, offs, rcat, roffs = _seqs(pl)
        kw = dict(same_file=True, tile_size=tile, tile_overlap=overlap, threshold=P.default_threshold(scoring, tile, overlap),
                  scoring=scoring, n_threads=8)
        wf, _ = oracle.gact_many(cat, offs, cat, offs, pl.cf, complement=False, **kw)
        wr, _ = oracle.gact_many(cat, offs, rcat, roffs, pl.cr, complement=True, **kw)
        _WANT[key] = np.concatenate([wf, wr])
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _run(monkeypatch, pl, scoring, layout, band=None, orders=(None,)):
    """one engine, one launch per order (a permutation of the forward and one of the reverse-complement candidates, or None);
    returns the fetched records and stats of every launch"""
    from gact_amd import engine
    for var in _SWITCHES + ("GACT_HIP_BAND",):
        monkeypatch.delenv(var, raising=False)
    for var, val in LAYOUTS[layout].items():
        monkeypatch.setenv(var, val)
    if band is not None:
        monkeypatch.setenv("GACT_HIP_BAND", str(band))
    cat, offs, rcat, roffs = _seqs(pl)
    eng = engine.Engine(tile_size=pl.tile, tile_overlap=pl.overlap, scoring=scoring,
                        threshold=P.default_threshold(scoring, pl.tile, pl.overlap))
    out = []
    try:
        eng.upload(engine.SET_REF, cat, offs); eng.upload(engine.SET_QUERY, cat, offs); eng.upload(engine.SET_QUERY_RC, rcat, roffs)
        for order in orders:
            cf, cr = (pl.cf, pl.cr) if order is None else (pl.cf[order[0]], pl.cr[order[1]])
            cands = np.concatenate([cf, cr])
            eng.candidates_upload(cands)
            eng.candidates_run_mixed(len(cands), rc_from=len(cf))
            out.append((eng.candidates_fetch(len(cands)).copy(), eng.last_run_stats()))
    finally:
        eng.close()
    return out


def _reaches_the_tiles(got, pl):
    """the chains really ran their planted tiles: all pass the first tile's threshold and go on behind it"""
    assert (got["n_tiles"] >= 2).all() and len(got) == 2 * len(pl.cf)


@pytest.mark.parametrize("tile,overlap,scoring,layout", _CASES, ids=_IDS)
def test_planted_tiles_match_the_oracle(monkeypatch, oracle, tile, overlap, scoring, layout):
    scoring = P.resolve(scoring)
    pl, walks, _ = P.planted_lists(oracle, tile, overlap, scoring)
    (got, st), = _run(monkeypatch, pl, scoring, layout)
    tag = "%d/%d %s %s" % (tile, overlap, (scoring,), layout)
    want_stats = _expected_stats(tile, overlap, scoring, layout)
    print(tag, len(got), "candidates, band_redos", st["band_redos"], "main_ms %.1f" % st["main_ms"])
    _check_stats(st, want_stats, tag)
    if want_stats["linear_gap"] and any(w.band > 48 for w in walks):
        # default band: the walks that leave it give up and their tiles run again with every block stored.  (Only under the
        # largest |g| no walk can: 49 gap moves cost more than a tile of 320 rows can score, tests/test_planted_tiles.py)
        assert st["band_redos"] > 0, (tag, st)
    _same(got, _records(oracle, pl, tile, overlap, scoring), tag)
    _reaches_the_tiles(got, pl)


_GEO_CASES = [(g, sc, lay) for g in P.GEOMETRIES for sc, lay in P.geometry_layouts(g)]
_GEO_IDS = ["%d/%d-%s-%s" % (g.tile, g.overlap, "plain" if sc == P.PLAIN else "affine", lay) for g, sc, lay in _GEO_CASES]


@pytest.mark.parametrize("g,scoring,layout", _GEO_CASES, ids=_GEO_IDS)
def test_planted_tiles_match_the_oracle_at_every_geometry(monkeypatch, oracle, g, scoring, layout):
    """planted_tiles.GEOMETRIES: where the split pass's pointer window begins (tile - overlap alone sets its lane and column), which
    kernel family runs, and tiles that fill no whole lane or lane group -- what no R x Q at 320/120 moves.  The same comparison
    as above, on the row's own edge set crossed with itself"""
    tile, overlap = g.tile, g.overlap
    pl, walks, _ = P.planted_lists(oracle, tile, overlap, scoring)
    (got, st), = _run(monkeypatch, pl, scoring, layout)
    tag = "%d/%d %s %s" % (tile, overlap, (scoring,), layout)
    want_stats = _expected_stats(tile, overlap, scoring, layout)
    assert (want_stats["layout"] == "packed16-uniform") == (g.plain == P.UNI or layout == "uniform"), (tag, want_stats)
    print(tag, len(got), "candidates, band_redos", st["band_redos"], "main_ms %.1f" % st["main_ms"])
    _check_stats(st, want_stats, tag)
    if want_stats["linear_gap"] and any(w.band > 48 for w in walks):
        assert st["band_redos"] > 0, (tag, st)
    _same(got, _records(oracle, pl, tile, overlap, scoring), tag)
    _reaches_the_tiles(got, pl)


@pytest.mark.parametrize("layout", ("split", "coop"))
def test_narrow_band(monkeypatch, oracle, layout):
    """GACT_HIP_BAND=24: many more walks leave the stored band; the records do not change"""
    pl, _, _ = P.planted_lists(oracle, 320, 120, P.PLAIN)
    (got, st), = _run(monkeypatch, pl, P.PLAIN, layout, band=24)
    _check_stats(st, _expected_stats(320, 120, P.PLAIN, layout), "band 24 " + layout)
    assert st["band_redos"] > 0, st
    _same(got, _records(oracle, pl, 320, 120, P.PLAIN), "band 24 " + layout)


@pytest.mark.parametrize("layout", ("split", "coop"))
def test_lane_partners_like_and_unlike(monkeypatch, oracle, layout):
    """two tiles share a lane's half-words and both are delayed to end on the wave's last step: sorted by (|a|, |b|) a planted tile
    runs beside one of its own size, in a shuffled list beside any other.  Both orders give the oracle's records, and each other's"""
    pl, _, _ = P.planted_lists(oracle, 320, 120, P.PLAIN)
    n = len(pl.cf)
    by_size = np.lexsort((pl.meta["Q"], pl.meta["R"]))
    rng = np.random.default_rng(4242)
    orders = ((by_size, by_size), (rng.permutation(n), rng.permutation(n)))
    want = _records(oracle, pl, 320, 120, P.PLAIN)
    runs = _run(monkeypatch, pl, P.PLAIN, layout, orders=orders)
    back = []
    for name, (of, orc), (got, st) in zip(("sorted", "shuffled"), orders, runs):
        tag = "%s %s" % (layout, name)
        _check_stats(st, _expected_stats(320, 120, P.PLAIN, layout), tag)
        perm = np.concatenate([of, n + orc])
        _same(got, want[perm], tag)
        undone = np.empty_like(got)
        undone[perm] = got
        back.append(undone)
    _same(back[0], back[1], "%s: sorted against shuffled" % layout)


@pytest.mark.parametrize("tile,overlap,scoring", P.RAW_CONFIGS, ids=("plain", "affine", "317/119-plain"))
def test_raw_bytes(monkeypatch, oracle, tile, overlap, scoring):
    """N and lower-case bases inside the planted tiles: the raw-byte kernels of the split layout"""
    pl, _, _ = P.planted_lists(oracle, tile, overlap, scoring, raw=True)
    (got, st), = _run(monkeypatch, pl, scoring, "split")
    assert st["raw_candidates"] > 0 and st["packed16"] and st["layout"] == "packed16-split", st
    _same(got, _records(oracle, pl, tile, overlap, scoring, raw=True), "raw %s" % (scoring,))
    _reaches_the_tiles(got, pl)

