"""GPU: the walk batch of the cooperative launch (coop_walk_batch, csrc/gact_coop.hpp) on lists made for what its
straight-line moves can get wrong.

The batch walks up to 64 tiles in lock step, eight moves per trip with no branch inside a move: a lane whose walk has
ended rides along to the end of the batch with every update of its state masked, the stop tests fall on any of a trip's
eight moves, and the walk's column is kept relative to the lane a trip began in.  tests/test_gpu_roles.py and the coop
cases of tests/test_gpu_planted_tiles.py hold the kernel to the oracle at the pass's edges; the list here is a few hundred
planted tiles (tests/planted_tiles.py) at tile 320 / overlap 120, shuffled and run on a grid of ONE block
(GACT_HIP_LIN_BLOCKS=1), so that every batch of that block mixes them:

  * walks of every length 8n ... 8n + 7 (exact copies of R = Q = 193 ... 200 and 57 ... 64 end at the tile's border after
    R moves), so that every move of a trip is a stop point;
  * walks of 17 ... 24 moves beside walks of 200 and more, so that finished lanes ride through 20 and more trips;
  * every ending of planted_tiles.Walk.end -- zero, border, early --, the early limit reached by rows first behind a long
    insertion run and by columns first behind a long deletion run;
  * a deletion run of at least 14 columns (more than a lane of region 2 holds), and tiles of Q <= 13 and of R <= 2;
  * both values of `reverse`;
  * and the same list under GACT_HIP_BAND=24, where walks leave the stored band and their tiles run again.

What the lists hold is read off the oracle's own traceback of every planted tile: a case that is missing fails the test.
Every record field is compared with the oracle's."""
import numpy as np
import pytest

import planted_tiles as P
from test_gpu_int16_edges import _check_stats
from test_gpu_lin_code_groups import _same          # (it compares every field of FIELDS)
from test_gpu_planted_tiles import _expected_stats, _run

pytestmark = pytest.mark.gpu

TILE, OVERLAP, SCORING = 320, 120, P.PLAIN
EARLY = TILE - OVERLAP


def _shapes():
    out = []
    for n in list(range(193, 201)) + list(range(57, 65)) + list(range(17, 25)):
        out.append((n, n, "copy0"))
    out += [(320, 320, "copy0")] * 2 + [(320, 320, "copy5")] * 4 + [(320, 320, "copy15")] * 8 + [(320, 320, "copy30")] * 2
    out += [(320, 320, "burst")] * 14 + [(289, 320, "burst"), (320, 289, "burst"), (304, 304, "burst"), (232, 320, "burst")]
    out += [(64, 64, "unrelated"), (200, 200, "unrelated"), (320, 320, "unrelated"), (33, 320, "unrelated"), (320, 33, "unrelated"),
            (320, 320, "flood"), (320, 320, "flood"), (200, 320, "flood")]
    for q in (1, 2, 5, 12, 13):
        for r in (1, 2, 16, 200, 320):
            out.append((r, q, "copy0"))
            out.append((r, q, "copy15"))
    for r in (1, 2):
        for q in (14, 26, 27, 200, 320):
            out.append((r, q, "copy0"))
            out.append((r, q, "unrelated"))
    return out


_LIST = {}


def _states(oracle, pl, k):
    """the oracle's traceback of candidate k's planted tile, as planted_tiles.describe asks for it: 3 diagonal, 2 insertion
    (a row alone), 1 deletion (a column alone)"""
    a, b, _, _ = P._planted_bytes(pl, k)
    bt = oracle.align_with_bt(a, b, SCORING, bool(pl.meta[k]["reverse"]), False, EARLY)
    return list(bt[1:])


def _longest_run(states, what):
    best = run = 0
    for s in states:
        run = run + 1 if s == what else 0
        best = max(best, run)
    return best


def _list(oracle):
    """(Planted of the candidates whose planted tile the oracle's trace holds, shuffled; their Walk; their tracebacks; the
    oracle's records, forward candidates then reverse-complement ones) -- built once"""
    if not _LIST:
        pl = P.plant(TILE, OVERLAP, SCORING, P.default_threshold(SCORING), _shapes(), P.KINDS, seed=131313)
        walks = P.describe(oracle, pl, SCORING, P.default_threshold(SCORING))
        keep = np.flatnonzero([w.present for w in walks])
        keep = keep[np.random.default_rng(77).permutation(len(keep))]
        kept = pl._replace(cf=pl.cf[keep], cr=pl.cr[keep], meta=pl.meta[keep])
        cat, offs = kept.rs.concat()
        rcat, roffs = kept.rs.concat(rc=True)
        kw = dict(same_file=True, tile_size=TILE, tile_overlap=OVERLAP, threshold=P.default_threshold(SCORING), scoring=SCORING, n_threads=8)
        wf, _ = oracle.gact_many(cat, offs, cat, offs, kept.cf, complement=False, **kw)
        wr, _ = oracle.gact_many(cat, offs, rcat, roffs, kept.cr, complement=True, **kw)
        want = np.concatenate([wf, wr])
        for arr in (kept.cf, kept.cr, kept.meta, want):
            arr.setflags(write=False)
        _LIST["v"] = (kept, [walks[k] for k in keep], [_states(oracle, kept, k) for k in range(len(keep))], want)
    return _LIST["v"]


def _holds_every_case(pl, walks, states):
    n = len(pl.cf)
    assert 150 <= n and 2 * n <= 800, n
    lengths = np.array([len(s) for s in states])
    rev = pl.meta["reverse"]
    for d in (0, 1):
        here = lengths[rev == d]
        assert len(here) >= 60, (d, len(here))
        # every move of a trip is a stop point, among the long walks and among the short ones
        for lo, hi in ((185, 10 ** 6), (40, 80)):
            part = here[(here >= lo) & (here <= hi)]
            assert set(part % 8) == set(range(8)), (d, lo, sorted(set(part % 8)))
        # finished lanes ride along: walks a tenth as long beside walks of 200 moves and more
        assert ((here >= 10) & (here <= 25)).sum() >= 8 and (here >= 200).sum() >= 20, (d, np.sort(here))
    ends = {w.end for w in walks}
    assert ends == {"zero", "border", "early"}, ends
    # the early limit by rows first behind an insertion run, by columns first behind a deletion run; a deletion run that
    # no lane of region 2 (13 columns) holds
    rows_first = [k for k, w in enumerate(walks) if w.end == "early" and w.n_i > w.n_d and _longest_run(states[k], 2) >= 14]
    cols_first = [k for k, w in enumerate(walks) if w.end == "early" and w.n_d > w.n_i and _longest_run(states[k], 1) >= 14]
    assert rows_first and cols_first, (len(rows_first), len(cols_first))
    assert {int(rev[k]) for k in rows_first} == {0, 1} and {int(rev[k]) for k in cols_first} == {0, 1}
    assert max(_longest_run(s, 1) for s in states) >= 14
    # the clamps: tiles of at most one lane's columns, of at most two rows -- with a walk to speak of
    narrow = [k for k in range(n) if pl.meta["Q"][k] <= 13 and lengths[k] >= 1]
    flat = [k for k in range(n) if pl.meta["R"][k] <= 2 and lengths[k] >= 1]
    assert len(narrow) >= 10 and len(flat) >= 10, (len(narrow), len(flat))
    assert any(w.band > 24 for w in walks) and any(w.band > 48 for w in walks)


def test_the_list_holds_every_case(oracle):
    pl, walks, states, _ = _list(oracle)
    _holds_every_case(pl, walks, states)


@pytest.mark.parametrize("band", (None, 24), ids=("default-band", "band-24"))
def test_walk_batches_match_the_oracle(monkeypatch, oracle, band):
    pl, walks, states, want = _list(oracle)
    _holds_every_case(pl, walks, states)
    monkeypatch.setenv("GACT_HIP_LIN_BLOCKS", "1")
    (got, st), = _run(monkeypatch, pl, SCORING, "coop", band=band)
    tag = "coop walk batch, band %s" % band
    print(tag, len(got), "candidates, band_redos", st["band_redos"], "main_ms %.1f" % st["main_ms"])
    _check_stats(st, _expected_stats(TILE, OVERLAP, SCORING, "coop"), tag)
    assert st["coop_walks"], st
    assert st["band_redos"] > 0, st            # (walks wider than the band are in the list: _holds_every_case)
    _same(got, want, tag)
    assert (got["n_tiles"] >= 2).all() and len(got) == 2 * len(pl.cf)
