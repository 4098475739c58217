"""GPU: the byte groups of the split linear-gap pass (csrc/gact_lin.hpp 9.) at every shape of its pointer phase.

Inside a whole flush block of eight steps the pass files the op codes of two columns at once, four steps to a byte, and
the flush re-pairs them; the steps behind the last whole block keep the half-word scheme on registers that must still be
zero.  What can go wrong is the hand-over between the two schemes and between the two kinds of block (both regions,
region 2 alone), so the lists here give a non-first tile every last-tile size 1..24 and 193..216 in both extension
directions and on both strands.  Taken by itself such a tile has x + 15 - (208 - x) // 13 pointer steps up to x = 200 and
215 above: every residue mod 8 and mod 4, a first pointer step on either side of T_end - LAG, and so passes with whole
blocks of both kinds, with blocks of region 2 alone, and with no whole block at all.  They run through the split launch and
the cooperative launch, with the default band and a narrow one (second runs that store every block), under +1/-1/-1/-1
and under the widest linear scoring the guard admits.  The uniform pass (wide launch, seed launch) is as it was.

Every record field is compared with the oracle (oracle.gact_many), as tests/test_gpu_lin_rows.py does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("ref_id", "query_id", "ab", "ae", "bb", "be", "score", "comp", "emitted", "first_tile_score", "n_tiles", "cells")
TILE, OVERLAP = 320, 120
SIZES = tuple(range(1, 25)) + tuple(range(193, 217))
PLAIN = (1, -1, -1, -1)
LEN = 700
K_GROUP, C2, LAG = 16, 13, 16


def _max_linear_scoring():
    """the linear scoring with the largest match - mismatch for which the engine still plans the linear-gap pass at this tile
    size (p16_lin_ok, csrc/gact_lin.hpp, asked through engine.plan): found as tests/test_gpu_lin_rows.py finds it"""
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


def pass_shape(x, tile=TILE, overlap=OVERLAP):
    """a pass over one non-first tile of x rows and x columns (split_last_step, split_first_pointer_step in csrc/gact_p16s.hpp,
    the loops of dp_pass_lin_split, the same in dp_pass_lin_split_col): pointer steps, first pointer step minus (T_end - LAG), whole
    blocks of step_tagged, whole blocks of step_tagged_r2, steps behind the last whole block"""
    early = tile - overlap
    first = max(1, x - early + 1)
    jj = first + (C2 * K_GROUP - x)
    t = tB = first + (jj - 1) // C2 + K_GROUP
    T_end = x + (K_GROUP - 1) + K_GROUP
    both = r2 = 0
    while t + 7 <= T_end and t <= T_end - LAG:
        t += 8; both += 1
    while t + 7 <= T_end:
        t += 8; r2 += 1
    return T_end - tB + 1, tB - (T_end - LAG), both, r2, T_end - t + 1


def _sized_reads(rng):
    """exact copies of one 700-base segment, whole and cut at either end (tests/test_gpu_lin_rows.py)"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    g = acgt[rng.integers(0, 4, size=LEN)]
    return g, ((0, LEN), (0, LEN - 50), (40, LEN))


@pytest.fixture(scope="module")
def lists(oracle):
    """reads, forward and reverse-complement candidates, and the check that the sized candidates do what they are for"""
    from gact_amd import synth
    rs = synth.simulate_reads(6000, n_reads=40, seed=701, mean_len=500, sd_len=120, min_len=300, max_len=700)
    cf, cr = synth.synth_candidates(rs, seed=702, min_overlap=120, false_frac=0.1)
    rng = np.random.default_rng(703)
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
    # what the sized candidates are for: in each direction a non-first tile of x rows and x columns for every x of SIZES ...
    seen = set()
    ref = rs.reads[base].tobytes()
    for c in sf[sf["query_id"] == base + 1]:
        _, traces = oracle.gact(ref, rs.reads[base + 1].tobytes(), int(c["ref_pos"]), int(c["query_pos"]), tile_size=TILE,
                                tile_overlap=OVERLAP, ref_id=0, query_id=1, trace_cap=16)
        seen |= {(t.reverse, t.ref_len) for t in traces if not t.first and t.ref_len == t.query_len}
    missing = [(d, x) for d in (0, 1) for x in SIZES if (d, x) not in seen]
    assert not missing, "no non-first tile of these (direction, size): %s" % missing
    # ... and, from those sizes, every shape of the pointer phase, in each direction
    for d in (0, 1):
        shapes = [pass_shape(x) for dd, x in seen if dd == d and x in SIZES]
        assert {n % 8 for n, _, _, _, _ in shapes} == set(range(8))
        assert {n % 4 for n, _, _, _, _ in shapes} == set(range(4))
        assert {rem for _, _, _, _, rem in shapes} == set(range(8))
        assert any(off <= 0 for _, off, _, _, _ in shapes) and any(off > 0 for _, off, _, _, _ in shapes)
        assert any(both > 1 and r2 > 0 for _, _, both, r2, _ in shapes)              # whole blocks of both kinds
        assert any(both == 0 and r2 > 0 for _, _, both, r2, _ in shapes)             # only region-2 blocks
        assert any(both == 0 and r2 == 0 and n > 0 for n, _, both, r2, _ in shapes)  # no whole block at all
    cf = np.concatenate([cf, sf]); cr = np.concatenate([cr, sr])
    assert 400 <= len(cf) + len(cr) <= 1500
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


LAUNCHES = ("split", "coop")


def _run(monkeypatch, lists, launch, scoring, threshold, band=None):
    from gact_amd import engine
    rs, cf, cr = lists
    monkeypatch.setenv("GACT_HIP_NO_WIDE", "1")                  # (lists this small take the wide layout)
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


def _check_launch(st, launch):
    assert st["linear_gap"], st
    assert st["layout"] == "packed16-split", st
    assert st["coop_walks"] == (launch == "coop") and not st["role_waves"], st


@pytest.mark.parametrize("launch", LAUNCHES)
def test_every_shape_of_the_pointer_phase(monkeypatch, oracle, lists, launch):
    got, st = _run(monkeypatch, lists, launch, PLAIN, 35)
    _check_launch(st, launch)
    _same(got, _records(oracle, lists, PLAIN, 35), "%s launch" % launch)


@pytest.mark.parametrize("launch", LAUNCHES)
def test_narrow_band_reruns_store_every_block(monkeypatch, oracle, lists, launch):
    """GACT_HIP_BAND=24: some walks leave the stored band and their tiles run again with every block stored"""
    got, st = _run(monkeypatch, lists, launch, PLAIN, 35, band=24)
    _check_launch(st, launch)
    assert st["band_redos"] > 0, st
    _same(got, _records(oracle, lists, PLAIN, 35), "%s launch, band 24" % launch)


@pytest.mark.parametrize("launch", LAUNCHES)
def test_widest_linear_scoring(monkeypatch, oracle, lists, launch):
    """the scoring whose tagged scores are the largest the guard admits: the gathered low bytes carry the most above the tags"""
    sc = _max_linear_scoring()
    assert sc is not None and sc[0] - sc[1] >= 19, sc            # (18, -1, -1, -1) is admitted at 320 (tests/scoring_edges.py)
    threshold = 35 * max(sc[0], 1)
    got, st = _run(monkeypatch, lists, launch, sc, threshold)
    _check_launch(st, launch)
    _same(got, _records(oracle, lists, sc, threshold), "%s launch, scoring %s" % (launch, (sc,)))
