"""GPU: the sliding zero levels of the column-drifted split linear-gap pass (csrc/gact_lin.hpp 13.) at the tile sizes where
the block structure of a pass changes.

Inside whole blocks of eight steps the pass reads its zero levels out of a strip that moves once per block; the steps outside
whole blocks move a window per step.  What can go wrong is an entry off by one at a hand-over between the two forms: where the
plain steps' trips of eight end, where the pointer phase begins, behind its last whole block, and where it begins with fewer
than eight steps left.  tests/test_gpu_lin_code_groups.py and tests/test_gpu_lin_col_drift.py give tiles of 1..24, 193..216
and 300..320; the lists here give, as a non-first tile in both extension directions and on both strands, the sizes they leave
out and at which that structure changes.  Taken by itself such a tile has, behind region 1's 16 steps alone:
17..64: 14..11 plain steps (one trip of eight, 6..3 left over), then 2..8 whole pointer blocks and every length 0..7 behind them;
120..136: 6 or 5 plain steps (no whole trip), 16..18 whole pointer blocks, every length 0..7 behind them;
217..232 and 289..304: 17..32 and 89..104 plain steps -- 2..4 and 11..13 trips of eight, every length 0..7 left over -- and a
pointer phase of 215 steps.
Both launches (split, cooperative), +1/-1/-1/-1 and the largest |g| the engine still plans the linear-gap pass for, every
record field against the oracle (oracle.gact_many).

The helpers are those of tests/test_gpu_lin_code_groups.py, the lists are built as tests/test_gpu_lin_col_drift.py builds them."""
import numpy as np
import pytest

from test_gpu_lin_code_groups import K_GROUP, LAG, LEN, OVERLAP, PLAIN, TILE, _check_launch, _run, _same, _sized_reads, pass_shape
from test_gpu_lin_col_drift import _max_gap_scoring

pytestmark = pytest.mark.gpu

SIZES = tuple(range(17, 65)) + tuple(range(120, 137)) + tuple(range(217, 233)) + tuple(range(289, 305))
LAUNCHES = ("split", "coop")


@pytest.fixture(scope="module")
def lists(oracle):
    """reads, forward and reverse-complement candidates: a few simulated overlaps and the sized candidates, with the check that
    the oracle's traces really hold a non-first tile of every size in each direction"""
    from gact_amd import synth
    rs = synth.simulate_reads(6000, n_reads=16, seed=1001, mean_len=500, sd_len=120, min_len=300, max_len=700)
    cf, cr = synth.synth_candidates(rs, seed=1002, min_overlap=120, false_frac=0.1)
    rng = np.random.default_rng(1003)
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
    # what the sizes are for (pass_shape; plain steps: those between region 1's LAG steps alone and the first pointer step)
    shapes = [pass_shape(x) for x in SIZES]
    assert {both + r2 for _, _, both, r2, _ in shapes} >= set(range(2, 9)) | {16, 17, 18}
    assert {rem for _, _, _, _, rem in shapes} == set(range(8))
    plain = [x + 2 * K_GROUP - 1 - n - LAG for x, (n, _, _, _, _) in zip(SIZES, shapes)]
    assert {p % 8 for p in plain} == set(range(8)) and {p // 8 for p in plain} >= {0, 1, 2, 3, 4, 11, 12, 13}, plain
    cf = np.concatenate([cf, sf]); cr = np.concatenate([cr, sr])
    print("level-window lists: %d candidates" % (len(cf) + len(cr)))
    assert 400 <= len(cf) + len(cr) <= 3000, len(cf) + len(cr)
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
    sc = _max_gap_scoring()
    assert sc is not None and sc[1] <= -12, sc                   # (1, -12, -12, -12) is admitted at 320 (tests/scoring_edges.py)
    return sc


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("name", ("plain", "max-gap"))
def test_levels_where_the_block_structure_changes(monkeypatch, oracle, lists, name, launch):
    sc = _scoring(name)
    threshold = 35 * max(sc[0], 1)
    got, st = _run(monkeypatch, lists, launch, sc, threshold)
    _check_launch(st, launch)
    assert not st["lin_row_drift"], st                           # the column-drifted pass is the one that ran
    _same(got, _records(oracle, lists, sc, threshold), "%s launch, scoring %s" % (launch, (sc,)))
