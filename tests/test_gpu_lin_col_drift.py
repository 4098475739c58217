"""GPU: the column-drifted frame of the split linear-gap pass (csrc/gact_lin.hpp 2b.) where its zero levels and hand-overs
matter, and the launch's choice between it and the row-drifted pass (gact_lin.hpp 12.).

The pass keeps the cell of step t and column slot c as X + base + (t + c)|g|: H_left + g is the left neighbour as it stands, the
zero levels are wave-uniform and come out of scalar registers, and a value that crosses a lane is converted by a constant.
What can go wrong is a zero level of the wrong slot or step, a hand-over constant, the left pad columns (which must stay at
their zero level), and the j = 0 border, which only a full-width tile reaches.  So the lists give a non-first tile, in both
extension directions and on both strands, every size 1..16 (region 2's last lanes alone), 200..216 (the first lanes of region
1 come into use) and 300..320 (the pad columns shrink to none), and run through the split and the cooperative launch under
+1/-1/-1/-1, a g = 0 scoring, and the largest |g| and the largest match - g for which the engine still plans the linear-gap
pass.  Its look-up byte needs match + 2|g| <= 63 where the guard admits match + |g| <= 63; a scoring beyond that takes the same
kernels on the row-drifted pass.  That happens at small tiles only, so the last scoring on either side of the rule runs at
tile 64 on the adversarial reads of tests/scoring_edges.py.

The row-drifted frame is reachable at such tiles only, so every shape of the pointer phase that tile 64 / overlap 8 can give it
(pass_shape of tests/test_gpu_lin_code_groups.py: whole blocks of both regions, of region 2 alone, none, every remainder, a
first pointer step on either side of T_end - LAG) runs there too, under (62, -1, -1, -1), on last tiles of every size 1..64
of exact copies and on copies with errors.

Every record field is compared with the oracle (oracle.gact_many), as tests/test_gpu_lin_code_groups.py does; its helpers
build and run the lists."""
import numpy as np
import pytest

from test_gpu_lin_code_groups import (LEN, OVERLAP, PLAIN, TILE, _check_launch, _max_linear_scoring, _run, _same, _sized_reads,
                                      pass_shape)

pytestmark = pytest.mark.gpu

SIZES = tuple(range(1, 17)) + tuple(range(200, 217)) + tuple(range(300, 321))
ZERO_GAP = (2, 0, 0, 0)
LAUNCHES = ("split", "coop")


def _max_gap_scoring():
    """the linear scoring with the largest |g| (match 1) for which the engine still plans the linear-gap pass at this tile size"""
    from gact_amd import engine
    for g in range(-40, 0):
        sc = (1, g, g, g)
        if engine.plan(50000, tile_size=TILE, tile_overlap=OVERLAP, scoring=sc)["linear"]:
            return sc
    return None


@pytest.fixture(scope="module")
def lists(oracle):
    """reads, forward and reverse-complement candidates: a few simulated overlaps and the sized candidates, with the check that
    the sized ones give a non-first tile of every size in each direction"""
    from gact_amd import synth
    rs = synth.simulate_reads(6000, n_reads=24, seed=901, mean_len=500, sd_len=120, min_len=300, max_len=700)
    cf, cr = synth.synth_candidates(rs, seed=902, min_overlap=120, false_frac=0.1)
    rng = np.random.default_rng(903)
    g, cuts = _sized_reads(rng)
    base = rs.n
    rs.reads.append(g.copy()); rs.names.append("sized_ref")
    for k, (a, b) in enumerate(cuts):
        rs.reads.append(g[a:b].copy()); rs.names.append("sized_q%d" % k)
    for k, (a, b) in enumerate(cuts):
        rs.reads.append(synth.revcomp(g[a:b])); rs.names.append("sized_qrc%d" % k)
    adv = TILE - OVERLAP
    # right phase: the first tile advances `adv` (or ends the read), the tile after it has x rows left; left phase the same
    positions = sorted({LEN - x for x in SIZES} | {LEN - adv - x for x in SIZES} | {adv + x for x in SIZES} | {x for x in SIZES})
    sf, sr = [], []
    for k, (a, b) in enumerate(cuts):
        for p in positions:
            if a <= p < b:
                sf.append((base, base + 1 + k, p, p - a))
                sr.append((base, base + 1 + len(cuts) + k, p, p - a))
    sf = np.array(sf, dtype=synth.CAND_DTYPE); sr = np.array(sr, dtype=synth.CAND_DTYPE)
    seen = set()
    ref = rs.reads[base].tobytes()
    for c in sf[sf["query_id"] == base + 1]:
        _, traces = oracle.gact(ref, rs.reads[base + 1].tobytes(), int(c["ref_pos"]), int(c["query_pos"]), tile_size=TILE,
                                tile_overlap=OVERLAP, ref_id=0, query_id=1, trace_cap=16)
        seen |= {(t.reverse, t.ref_len) for t in traces if not t.first and t.ref_len == t.query_len}
    missing = [(d, x) for d in (0, 1) for x in SIZES if (d, x) not in seen]
    assert not missing, "no non-first tile of these (direction, size): %s" % missing
    cf = np.concatenate([cf, sf]); cr = np.concatenate([cr, sr])
    assert 400 <= len(cf) + len(cr) <= 1500, len(cf) + len(cr)
    return rs, cf, cr


_WANT = {}


def _records(oracle, lists, scoring, threshold):
    """the oracle's records of the lists under one scoring: computed once, shared by both launches"""
    if scoring not in _WANT:
        rs, cf, cr = lists
        cat, offs = rs.concat(); rcat, roffs = rs.concat(rc=True)
        kw = dict(same_file=True, tile_size=TILE, tile_overlap=OVERLAP, threshold=threshold, scoring=scoring, n_threads=8)
        wf, _ = oracle.gact_many(cat, offs, cat, offs, cf, complement=False, **kw)
        wr, _ = oracle.gact_many(cat, offs, rcat, roffs, cr, complement=True, **kw)
        _WANT[scoring] = np.concatenate([wf, wr])
        _WANT[scoring].setflags(write=False)
    return _WANT[scoring]


def _scoring(name):
    if name == "plain":
        return PLAIN
    if name == "zero-gap":
        return ZERO_GAP
    if name == "max-gap":
        sc = _max_gap_scoring()
        assert sc is not None and sc[1] <= -12, sc               # (1, -12, -12, -12) is admitted at 320 (tests/scoring_edges.py)
        return sc
    sc = _max_linear_scoring()
    assert sc is not None and sc[0] - sc[1] >= 19, sc            # (18, -1, -1, -1) is admitted at 320 (tests/scoring_edges.py)
    return sc


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("name", ("plain", "zero-gap", "max-gap", "max-match"))
def test_column_drift_at_every_edge(monkeypatch, oracle, lists, name, launch):
    sc = _scoring(name)
    threshold = 35 * max(sc[0], 1)
    got, st = _run(monkeypatch, lists, launch, sc, threshold)
    _check_launch(st, launch)
    assert not st["lin_row_drift"], st                           # every scoring admitted at this tile takes the column-drifted pass
    _same(got, _records(oracle, lists, sc, threshold), "%s launch, scoring %s" % (launch, (sc,)))


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("scoring", ((61, -1, -1, -1), (62, -1, -1, -1)), ids=("last-column-drifted", "first-row-drifted"))
def test_either_side_of_the_byte_rule_at_tile_64(monkeypatch, oracle, scoring, launch):
    """match + 2|g| = 63: the largest pointer byte the column-drifted pass makes (253); 64: the row-drifted pass.  Both are
    admitted by the guard at tile 64 (the `lin-match-64` edge) and both must give the reference's records"""
    from scoring_edges import EDGES
    from test_gpu_chain import _compare
    from test_gpu_int16_edges import LAYOUTS, _engine, _reads, _runs, _want
    edge = next(e for e in EDGES if e.name == "lin-match-64")
    er = _reads(edge)
    eng = _engine(monkeypatch, edge, scoring, LAYOUTS[launch], er)
    try:
        for name, comp, cands, qcat, qoffs in _runs(er)[:2]:
            tag = "tile 64 %s %s %s" % ((scoring,), launch, name)
            got = eng.extend(cands, complement=comp, same_file=True)
            st = eng.last_run_stats()
            assert st["linear_gap"] and st["layout"] == "packed16-split" and st["coop_walks"] == (launch == "coop"), (tag, st)
            assert st["lin_row_drift"] == (scoring[0] - 2 * scoring[3] > 63), (tag, st)        # the pass meant is the one that ran
            _compare(got, _want(oracle, edge, scoring, er, name, comp, cands, qcat, qoffs, True), tag)
    finally:
        eng.close()


ROW_TILE, ROW_OVERLAP, ROW_LEN, ROW_SCORING = 64, 8, 200, (62, -1, -1, -1)
ROW_SIZES = tuple(range(1, ROW_TILE + 1))


@pytest.fixture(scope="module")
def row_lists(oracle):
    """exact copies of one 200-base segment, whole and cut at either end, with candidates that leave a last tile of every size
    1..64 in each direction, and two copies with 4 % and 10 % errors seeded at the same positions; the oracle's records of
    both strands under (62, -1, -1, -1); and the check that the exact copies' tiles give the pass every shape of its pointer
    phase that this tile size can"""
    from gact_amd import synth
    from scoring_edges import EDGES, threshold
    edge = next(e for e in EDGES if e.name == "lin-match-64")
    assert (edge.tile, edge.overlap) == (ROW_TILE, ROW_OVERLAP)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    g = acgt[np.random.default_rng(911).integers(0, 4, size=ROW_LEN)]
    cuts = ((0, ROW_LEN), (0, ROW_LEN - 30), (25, ROW_LEN))
    rs = synth.ReadSet()
    rs.reads = [g.copy()] + [g[a:b].copy() for a, b in cuts] + [synth.revcomp(g[a:b]) for a, b in cuts]
    rs.names = ["sized_ref"] + ["sized_q%d" % k for k in range(3)] + ["sized_qrc%d" % k for k in range(3)]
    # two copies with errors, so that the same last tiles also leave the diagonal: the left neighbour's and the upper
    # neighbour's terms and the hand-overs decide values here, not only shapes (exact copies never take them)
    rng = np.random.default_rng(912)
    noisy = []
    for rate in (0.04, 0.10):
        out = []
        for base in g:
            r = rng.random()
            if r < rate / 3:
                continue                                                 # deletion
            if r < 2 * rate / 3:
                out.append(acgt[rng.integers(0, 4)])                     # insertion in front of the base
            out.append(acgt[rng.integers(0, 4)] if r > 1 - rate / 3 else base)   # substitution (a quarter of them silent)
        noisy.append(np.array(out, dtype=np.uint8))
    first_noisy = len(rs.reads)
    rs.reads += noisy + [synth.revcomp(q) for q in noisy]
    rs.names += ["noisy_q%d" % k for k in range(2)] + ["noisy_qrc%d" % k for k in range(2)]
    adv = ROW_TILE - ROW_OVERLAP
    positions = sorted({ROW_LEN - x for x in ROW_SIZES} | {ROW_LEN - adv - x for x in ROW_SIZES} |
                       {adv + x for x in ROW_SIZES} | set(ROW_SIZES))
    sf = [(0, 1 + k, p, p - a) for k, (a, b) in enumerate(cuts) for p in positions if a <= p < b]
    sr = [(0, 4 + k, p, p - a) for k, (a, b) in enumerate(cuts) for p in positions if a <= p < b]
    for k, q in enumerate(noisy):
        pos = [p for p in positions if 20 <= p < min(ROW_LEN, len(q)) - 20][::3]
        sf += [(0, first_noisy + k, p, p) for p in pos]
        sr += [(0, first_noisy + 2 + k, p, p) for p in pos]
    sf = np.array(sf, dtype=synth.CAND_DTYPE); sr = np.array(sr, dtype=synth.CAND_DTYPE)
    seen = set()
    for c in sf[sf["query_id"] == 1]:
        _, traces = oracle.gact(rs.reads[0].tobytes(), rs.reads[1].tobytes(), int(c["ref_pos"]), int(c["query_pos"]),
                                tile_size=ROW_TILE, tile_overlap=ROW_OVERLAP, ref_id=0, query_id=1, trace_cap=16)
        seen |= {(t.reverse, t.ref_len) for t in traces if not t.first and t.ref_len == t.query_len}
    missing = [(d, x) for d in (0, 1) for x in ROW_SIZES if (d, x) not in seen]
    assert not missing, "no non-first tile of these (direction, size): %s" % missing
    for d in (0, 1):
        shapes = [pass_shape(x, ROW_TILE, ROW_OVERLAP) for dd, x in seen if dd == d and x in ROW_SIZES]
        assert {rem for _, _, _, _, rem in shapes} == set(range(8))                  # the remainders 0..7
        assert any(off <= 0 for _, off, _, _, _ in shapes) and any(off > 0 for _, off, _, _, _ in shapes)
        assert any(both > 1 and r2 > 0 for _, _, both, r2, _ in shapes)              # whole blocks of both kinds
        assert any(both == 0 and r2 > 0 for _, _, both, r2, _ in shapes)             # only region-2 blocks
        assert any(both == 0 and r2 == 0 and n > 0 for n, _, both, r2, _ in shapes)  # no whole block at all
    assert len(sf) + len(sr) <= 1500, len(sf) + len(sr)
    cat, offs = rs.concat(); rcat, roffs = rs.concat(rc=True)
    th = threshold(edge, ROW_SCORING)
    kw = dict(same_file=True, tile_size=ROW_TILE, tile_overlap=ROW_OVERLAP, threshold=th, scoring=ROW_SCORING, n_threads=8)
    want = (oracle.gact_many(cat, offs, cat, offs, sf, complement=False, **kw)[0],
            oracle.gact_many(cat, offs, rcat, roffs, sr, complement=True, **kw)[0])
    for w in want:
        w.setflags(write=False)
    return (cat, offs, rcat, roffs), (sf, sr), want, th


@pytest.mark.parametrize("launch", LAUNCHES)
def test_row_drift_at_every_shape_of_the_pointer_phase(monkeypatch, row_lists, launch):
    from gact_amd import engine
    from test_gpu_int16_edges import LAYOUTS
    (cat, offs, rcat, roffs), cands, want, th = row_lists
    for var, val in LAYOUTS[launch].items():
        monkeypatch.setenv(var, val)
    if launch != "coop":
        monkeypatch.setenv("GACT_HIP_COOP", "0")
    eng = engine.Engine(tile_size=ROW_TILE, tile_overlap=ROW_OVERLAP, scoring=ROW_SCORING, threshold=th)
    try:
        eng.upload(engine.SET_REF, cat, offs); eng.upload(engine.SET_QUERY, cat, offs); eng.upload(engine.SET_QUERY_RC, rcat, roffs)
        for comp in (False, True):
            got = eng.extend(cands[comp], complement=comp, same_file=True)
            st = eng.last_run_stats()
            _check_launch(st, launch)
            assert st["lin_row_drift"], st                       # the row-drifted pass is the one that ran
            _same(got, want[comp], "tile 64 %s, row drift, %s" % (launch, "rc" if comp else "fwd"))
    finally:
        eng.close()
