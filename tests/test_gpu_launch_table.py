"""GPU: every launch sequence and every form of the split linear-gap main kernels (csrc/gact_launch_table.hpp: plain /
row-drifted x one set / two sets of queues), at list sizes of a few hundred chains.

What a pass runs as is decided by the number of candidates per resident tile slot of the narrow layouts (csrc/gact_policy.hpp
plan_pass: S = lin_grid_blocks x kNarrowTilesPerBlock).  On the whole machine S is 24,576 and the sequences beyond "all wide"
are reached by workload-sized lists only; an engine made with max_blocks = 6 has every persistent grid capped at six blocks,
S = 6 x 32 = 192, and plans on an idle engine
    n <= S                all wide                                           (count <= narrow_slots)
    S < n < 1.5 S         seed, split launch + critical lane                 (count < narrow_slots0 + narrow_slots0 / 2)
    1.5 S <= n <= 4 S     ordered, overlapped seeding: the two-set kernels   (count <= 4 * narrow_slots0)
    4 S < n < 6 S         seed, one split launch
    n >= 6 S              the same in the cooperative layout                 (coop_auto: count >= 6 * narrow_slots0)
"coop" 1 / "roles" 1 put the two-set cooperative / role kernel into the overlapped sequence, "runs_in_flight" 1 (the launch
shares the machine) takes the plain sequence and from 1.5 S on the one-set cooperative kernel.  The role grid of such an engine
is two blocks (6 x 4 / 12 waves), one for each of the two main launches of the overlapped sequence.

Each case runs both sides of its threshold, so a threshold derived wrongly here fails its case instead of running another plan:
the plan is asked of gact_policy.hpp itself (engine.plan at two compute units: 3 x 2 = 6 blocks, no device needed) and
last_run_stats must name the same plan for the run that was made.  Every record field is compared with the oracle's
(oracle.gact_many, once per scoring); the list is permuted anew within each strand for every case, so a candidate a launch left
out shows whatever another case left at its index.

Both drift frames of the linear-gap pass run everything: tile 64 / overlap 8 under (61, -1, -1, -1), the last column-drifted
scoring, and (62, -1, -1, -1), the first row-drifted one (tests/test_gpu_lin_col_drift.py, tests/planted_tiles.py CONFIGS).
Their arg-max keys do not fit the packed seed kernel (p16_argmax_ok: match x (tile + 2) < 2047), and plan_pass orders and
overlaps packed seed launches only: with the int32 seed launch 1.5 S ... 4 S is seed + one launch, of the split, the
cooperative ("coop") or the role kernel ("roles"), and these two frames reach the one-set forms alone.  So the same cases
also run under (28, -18, -18, -18) at 64 / 8 -- row-drifted by the smallest margin (match + 2|g| = 64) with a packed seed
launch -- and under the default geometry and scoring (column-drifted, packed seed launch): these reach the two-set forms of
both frames.  "lone_lane" is never set here: on a capped engine that plan does not bound its workspace."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("ref_id", "query_id", "ab", "ae", "bb", "be", "score", "comp", "emitted", "first_tile_score", "n_tiles", "cells")
BLOCKS = 6
S = BLOCKS * 32                                    # gact_policy.hpp kNarrowTilesPerBlock = 4 waves x 4 groups x 2 slots
# name: tile, overlap, scoring, first-tile threshold (tile 64: scoring_edges.threshold of the `lin-match-64` edge, match x 64 / 4),
# row-drifted (gact_lin.hpp lin_col_drift_ok fails: match + 2|g| > 63), packed seed launch (gact_p16.hpp p16_argmax_ok)
FRAMES = {"column-drifted": (64, 8, (61, -1, -1, -1), 61 * 64 // 4, False, False),
          "row-drifted": (64, 8, (62, -1, -1, -1), 62 * 64 // 4, True, False),
          "row-drifted-packed-seed": (64, 8, (28, -18, -18, -18), 28 * 64 // 4, True, True),
          "default": (320, 120, (1, -1, -1, -1), 35, False, True)}
# plan: (sequence of gact_policy::name(Seq), main kernel of name(MainK), layout, overlapped, critical lane, coop, roles)
WIDE = ("seed+main", "WideLayoutLin", "packed16-wide", False, False, False, False)
CRIT = ("seed+main+critical-lane", "SplitLayoutLin", "packed16-split", False, True, False, False)
OVERLAPPED = ("overlapped-seeding", "SplitLayoutLin", "packed16-split", True, False, False, False)
OVERLAPPED_COOP = ("overlapped-seeding", "coop<SplitLayoutLin>", "packed16-split", True, False, True, False)
OVERLAPPED_ROLES = ("overlapped-seeding", "roles<SplitLayoutLin>", "packed16-split", True, False, False, True)
SPLIT = ("seed+main", "SplitLayoutLin", "packed16-split", False, False, False, False)
COOP = ("seed+main", "coop<SplitLayoutLin>", "packed16-split", False, False, True, False)
ROLES = ("seed+main", "roles<SplitLayoutLin>", "packed16-split", False, False, False, True)
INT32_SEED = {OVERLAPPED: SPLIT, OVERLAPPED_COOP: COOP, OVERLAPPED_ROLES: ROLES}        # what a frame without the packed seed launch plans instead
ALL = -1                                           # the whole list
# switch: (engine.plan flags, [(n, plan)]): both sides of every threshold
CASES = {
    None: (0, [(1, WIDE), (S, WIDE), (S + 1, CRIT), (3 * S // 2 - 1, CRIT), (3 * S // 2, OVERLAPPED), (4 * S, OVERLAPPED),
               (4 * S + 1, SPLIT), (6 * S - 1, SPLIT), (6 * S, COOP), (ALL, COOP)]),
    "coop": (8, [(3 * S // 2, OVERLAPPED_COOP), (4 * S, OVERLAPPED_COOP)]),
    "roles": (4, [(3 * S // 2, OVERLAPPED_ROLES), (4 * S, OVERLAPPED_ROLES)]),
    "runs_in_flight": (2, [(3 * S // 2 - 1, SPLIT), (3 * S // 2, COOP), (ALL, COOP)]),
}
PARAMS = [pytest.param(frame, switch, n, plan if FRAMES[frame][5] else INT32_SEED.get(plan, plan),
                       id="%s-%s-%s" % (frame, switch or "policy", "all" if n == ALL else n))
          for frame in FRAMES for switch, (_, cases) in CASES.items() for n, plan in cases]


@pytest.fixture(scope="module")
def lists():
    from gact_amd import synth
    rs = synth.simulate_reads(40000, n_reads=100, seed=141, mean_len=2200, sd_len=600, min_len=600, max_len=4000)
    cf, cr = synth.synth_candidates(rs, seed=142, min_overlap=200, false_frac=0.1)
    assert 6 * S + 32 <= len(cf) + len(cr) <= 1500 and len(cf) > 2 * S and len(cr) > 2 * S, (len(cf), len(cr))
    return rs, cf, cr


_WANT = {}


def _records(oracle, lists, frame):
    """the oracle's records of the list in one frame: computed once, left unchanged"""
    if frame not in _WANT:
        rs, cf, cr = lists
        tile, overlap, scoring, threshold = FRAMES[frame][:4]
        cat, offs = rs.concat(); rcat, roffs = rs.concat(rc=True)
        kw = dict(same_file=True, tile_size=tile, tile_overlap=overlap, threshold=threshold, scoring=scoring, n_threads=8)
        wf, _ = oracle.gact_many(cat, offs, cat, offs, cf, complement=False, **kw)
        wr, _ = oracle.gact_many(cat, offs, rcat, roffs, cr, complement=True, **kw)
        for w in (wf, wr):
            w.setflags(write=False)
        _WANT[frame] = (wf, wr)
    return _WANT[frame]


@pytest.mark.parametrize("frame,switch,n,plan", PARAMS)
def test_the_plan_meant_runs_and_gives_the_oracles_records(oracle, lists, frame, switch, n, plan):
    from gact_amd import engine
    rs, cf, cr = lists
    wf, wr = _records(oracle, lists, frame)
    tile, overlap, scoring, threshold, row_drift, packed_seed = FRAMES[frame]
    assert row_drift == (scoring[0] - 2 * scoring[3] > 63) and packed_seed == (scoring[0] * (tile + 2) * 8 + 7 < 16384)
    total = len(cf) + len(cr)
    n = total if n == ALL else n
    sequence, main_kernel, layout, overlapped, lane, coop, roles = plan
    # the policy's own answer for a pass of n candidates on six blocks
    p = engine.plan(n, flags=CASES[switch][0], compute_units=BLOCKS // 3, tile_size=tile, tile_overlap=overlap, scoring=scoring,
                    threshold=threshold)
    assert (p["sequence"], p["main_kernel"], p["critical_lane"], p["coop"], p["roles"], p["linear"]) == \
           (sequence, main_kernel, lane, coop, roles, True), p
    # the list in this case's own order within each strand
    rng = np.random.default_rng([n, sorted(FRAMES).index(frame), sorted(CASES, key=str).index(switch)])
    pf, pr = rng.permutation(len(cf)), rng.permutation(len(cr))
    cands = np.concatenate([cf[pf], cr[pr]])
    want = np.concatenate([wf[pf], wr[pr]])
    first = 0 if n == total else min(max(0, len(cf) - n // 2), total - n)          # a range across the strand boundary
    eng = engine.Engine(tile_size=tile, tile_overlap=overlap, scoring=scoring, threshold=threshold, max_blocks=BLOCKS)
    try:
        if switch:
            eng.set_option(switch, 1)
        cat, offs = rs.concat(); rcat, roffs = rs.concat(rc=True)
        eng.upload(engine.SET_REF, cat, offs); eng.upload(engine.SET_QUERY, cat, offs); eng.upload(engine.SET_QUERY_RC, rcat, roffs)
        eng.candidates_upload(cands)
        eng.candidates_run_mixed(n, rc_from=len(cf), first=first)
        got = eng.candidates_fetch(total)[first:first + n].copy()
        st = eng.last_run_stats()
    finally:
        eng.close()
    ran = (st["layout"], st["overlapped_seeding"], st["critical_lane"], st["coop_walks"], st["role_waves"], st["linear_gap"],
           st["lin_row_drift"], st["seed_layout"])
    assert ran == (layout, overlapped, lane, coop, roles, True, row_drift and layout == "packed16-split",
                   "packed16" if packed_seed else "int32"), (ran, st)
    assert len(got) == n
    for f in FIELDS:
        if not np.array_equal(got[f], want[first:first + n][f]):
            k = int(np.flatnonzero(got[f] != want[first:first + n][f])[0])
            raise AssertionError("%s, %s, %d candidates from %d: %s differs at candidate %d: hip %s, oracle %s" %
                                 (frame, switch or "policy", n, first, f, first + k, got[k], want[first + k]))
