"""GPU: the per-row plumbing of the linear-gap passes (csrc/gact_lin.hpp) at the edges of a pass.

Round 6 took the look-up word of a row out of a table in LDS (the stream byte is the table offset, a pad row has an entry
of its own), made the eight steps of a flush block straight-line code and the score-only steps two per trip.  None of it
is the recurrence; what can go wrong is a row's word at the first and last steps of a pass, the hand-over between the
kinds of step (region 1 alone, both regions, pointer phase, region 2 alone), the flush block that is not full, and the pad
rows in front of row 1 and behind row R.  So the lists here are made of short reads whose last tiles take every size that
moves one of those edges, in both extension directions and on both strands, and they run through every launch that holds
the pass: the split launch, the cooperative launch, the wide launch and the seed launch in front of them, with the default
band and a narrow one, under +1/-1/-1/-1 and under the linear scoring with the largest match - mismatch the guard admits.

Every record field is compared with the oracle (oracle.gact_many), as tests/test_gpu_roles.py does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("ref_id", "query_id", "ab", "ae", "bb", "be", "score", "comp", "emitted", "first_tile_score", "n_tiles", "cells")
TILE, OVERLAP = 320, 120
# last-tile sizes: the LAG boundaries, the region boundary 7 x 16, and the sizes around them that move the first pointer step
SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 111, 112, 113, 119, 120, 121, 199, 200, 201, 207, 208, 209, 319, 320)
PLAIN = (1, -1, -1, -1)
LEN = 700


def _max_linear_scoring():
    """the linear scoring (mismatch == gap_open == gap_extend) with the largest match - mismatch for which the engine still
    plans the linear-gap pass at this tile size (p16_lin_ok, csrc/gact_lin.hpp, asked through engine.plan)"""
    from gact_amd import engine
    best = None
    for g in range(0, -40, -1):
        for match in range(64, -1, -1):
            sc = (match, g, g, g)
            if engine.plan(50000, tile_size=TILE, tile_overlap=OVERLAP, scoring=sc)["linear"]:
                if best is None or match - g > best[0] - best[1]:
                    best = sc
                break
    return best


def _sized_reads(rng):
    """exact copies of one 700-base segment, whole and cut at either end, on both strands: a candidate on the diagonal at ref
    position p has LEN - p bases to its right and p to its left, and every tile of an exact copy advances TILE - OVERLAP"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    g = acgt[rng.integers(0, 4, size=LEN)]
    # (query id offset within the block, first base, last base + 1)
    return g, ((0, LEN), (0, LEN - 50), (40, LEN))


@pytest.fixture(scope="module")
def lists(oracle):
    """reads, forward and reverse-complement candidates, and the check that the sized candidates do what they are for"""
    from gact_amd import synth
    rs = synth.simulate_reads(9000, n_reads=70, seed=601, mean_len=500, sd_len=120, min_len=300, max_len=700)
    cf, cr = synth.synth_candidates(rs, seed=602, min_overlap=120, false_frac=0.1)
    rng = np.random.default_rng(603)
    g, cuts = _sized_reads(rng)
    base = rs.n
    rs.reads.append(g.copy()); rs.names.append("sized_ref")
    for k, (a, b) in enumerate(cuts):
        rs.reads.append(g[a:b].copy()); rs.names.append("sized_q%d" % k)
    for k, (a, b) in enumerate(cuts):
        rs.reads.append(synth.revcomp(g[a:b])); rs.names.append("sized_qrc%d" % k)
    adv = TILE - OVERLAP
    # right phase: one tile of x rows from the seed position to the read's end; left phase: the first tile advances `adv`, the
    # tile after it has x rows left
    positions = sorted({LEN - x for x in SIZES} | {adv + x for x in SIZES})
    sf, sr = [], []
    for k, (a, b) in enumerate(cuts):
        for p in positions:
            if a <= p < b:
                sf.append((base, base + 1 + k, p, p - a))
                sr.append((base, base + 1 + len(cuts) + k, p, p - a))
    sf = np.array(sf, dtype=synth.CAND_DTYPE); sr = np.array(sr, dtype=synth.CAND_DTYPE)
    # what the sized candidates are for: in each direction, a non-first tile of x rows and x columns for every x of SIZES
    seen = set()
    ref = rs.reads[base].tobytes()
    for c in sf[sf["query_id"] == base + 1]:
        _, traces = oracle.gact(ref, rs.reads[base + 1].tobytes(), int(c["ref_pos"]), int(c["query_pos"]), tile_size=TILE,
                                tile_overlap=OVERLAP, ref_id=0, query_id=1, trace_cap=16)
        seen |= {(t.reverse, t.ref_len) for t in traces if not t.first and t.ref_len == t.query_len}
    missing = [(d, x) for d in (0, 1) for x in SIZES if (d, x) not in seen]
    assert not missing, "no non-first tile of these (direction, size): %s" % missing
    cf = np.concatenate([cf, sf]); cr = np.concatenate([cr, sr])
    assert 200 <= len(cf) + len(cr) <= 900
    return rs, cf, cr


_WANT = {}


def _records(oracle, lists, scoring, threshold):
    """the oracle's records of the lists under one scoring: computed once, shared by every test"""
    if scoring not in _WANT:
        rs, cf, cr = lists
        cat, offs = rs.concat(); rcat, roffs = rs.concat(rc=True)
        kw = dict(same_file=True, tile_size=TILE, tile_overlap=OVERLAP, threshold=threshold, scoring=scoring, n_threads=8)
        wf, _ = oracle.gact_many(cat, offs, cat, offs, cf, complement=False, **kw)
        wr, _ = oracle.gact_many(cat, offs, rcat, roffs, cr, complement=True, **kw)
        _WANT[scoring] = np.concatenate([wf, wr])
        _WANT[scoring].setflags(write=False)
    return _WANT[scoring]


def _same(got, want, what):
    for f in FIELDS:
        if not np.array_equal(got[f], want[f]):
            k = int(np.flatnonzero(got[f] != want[f])[0])
            raise AssertionError("%s: %s differs at candidate %d: hip %s, oracle %s" % (what, f, k, got[k], want[k]))


LAUNCHES = ("split", "coop", "wide")


def _run(monkeypatch, lists, launch, scoring, threshold, band=None):
    from gact_amd import engine
    rs, cf, cr = lists
    if launch != "wide":
        monkeypatch.setenv("GACT_HIP_NO_WIDE", "1")              # (lists this small take the wide layout)
    monkeypatch.setenv("GACT_HIP_COOP", "1" if launch == "coop" else "0")
    if band is not None:
        monkeypatch.setenv("GACT_HIP_BAND", str(band))
    eng = engine.Engine(tile_size=TILE, tile_overlap=OVERLAP, scoring=scoring, threshold=threshold)
    cat, offs = rs.concat(); rcat, roffs = rs.concat(rc=True)
    eng.upload(engine.SET_REF, cat, offs); eng.upload(engine.SET_QUERY, cat, offs); eng.upload(engine.SET_QUERY_RC, rcat, roffs)
    cands = np.concatenate([cf, cr])
    eng.candidates_upload(cands)
    eng.candidates_run_mixed(len(cands), rc_from=len(cf))
    got = eng.candidates_fetch(len(cands)).copy()
    st = eng.last_run_stats()
    eng.close()
    return got, st


def _check_launch(st, launch, scoring):
    from gact_amd import engine
    assert st["linear_gap"], st
    assert st["layout"] == ("packed16-wide" if launch == "wide" else "packed16-split"), st
    assert st["coop_walks"] == (launch == "coop") and not st["role_waves"], st
    # the seed launch in front: the packed linear-gap one wherever the plan says so
    lin_seed = engine.plan(50000, tile_size=TILE, tile_overlap=OVERLAP, scoring=scoring)["seed_kernel"] == "seed_p16<lin>"
    assert (st["seed_layout"] == "packed16") == lin_seed, st


@pytest.mark.parametrize("launch", LAUNCHES)
def test_every_last_tile_size_in_every_launch(monkeypatch, oracle, lists, launch):
    got, st = _run(monkeypatch, lists, launch, PLAIN, 35)
    _check_launch(st, launch, PLAIN)
    assert st["seed_layout"] == "packed16", st                   # +1/-1/-1/-1: the seed launch runs the uniform pass with AMAX
    _same(got, _records(oracle, lists, PLAIN, 35), "%s launch" % launch)


@pytest.mark.parametrize("launch", LAUNCHES)
def test_narrow_band_reruns_store_every_block(monkeypatch, oracle, lists, launch):
    """GACT_HIP_BAND=24: some walks leave the stored band and their tiles run again with every block stored"""
    got, st = _run(monkeypatch, lists, launch, PLAIN, 35, band=24)
    _check_launch(st, launch, PLAIN)
    assert st["band_redos"] > 0, st
    _same(got, _records(oracle, lists, PLAIN, 35), "%s launch, band 24" % launch)


@pytest.mark.parametrize("launch", LAUNCHES)
def test_largest_match_minus_mismatch(monkeypatch, oracle, lists, launch):
    """the scoring whose pointer-phase look-up bytes, 4 (match - mismatch) + 1, are the largest the guard admits"""
    sc = _max_linear_scoring()
    assert sc is not None and sc[0] - sc[1] >= 19, sc            # (18, -1, -1, -1) is admitted at 320 (tests/scoring_edges.py)
    threshold = 35 * max(sc[0], 1)
    got, st = _run(monkeypatch, lists, launch, sc, threshold)
    _check_launch(st, launch, sc)
    _same(got, _records(oracle, lists, sc, threshold), "%s launch, scoring %s" % (launch, (sc,)))
