"""GPU suite that holds the path run (gact_hip_candidates_paths) to the chain model at every configuration and edge: the
CIGAR string, n_columns, n_ops and the record of every compared candidate equal tests/path_model.py's on the oracle's
AlignWithBT, the records equal the normal run's byte for byte, and check_path holds with the model's left_aligned.  A
sample of both strands of ecoli10x_small at both scorings and three tile geometries (chain_kernel<20, ColumnSink> and <32, ...>), raw-byte
reads, the crafted candidates of tests/path_cases.py, one block walking everything, what a slot keeps between runs, and
the device filter's own list.  No tolerance anywhere: integers, bytes and strings are equal or the test fails."""
import numpy as np
import pytest

import path_cases
from path_cases import AFFINE, LINEAR, assert_equals_model, engine_with, expected, ops_of

pytestmark = pytest.mark.gpu

SAMPLE = 200                     # candidates per cell of the matrix, both strands; a floor, not a measurement
SCORINGS = [LINEAR, AFFINE]


def _small():
    from conftest import workload_block
    blk = workload_block("ecoli10x_small")
    cands = np.concatenate([blk.cf, blk.cr])
    nf = len(blk.cf)
    sel = path_cases.sample(nf, len(blk.cr), SAMPLE, seed=20261016)
    assert len(sel) >= 200 and (sel < nf).sum() >= 50 and (sel >= nf).sum() >= 50 and np.any(np.diff(sel) < 0)
    return blk, cands, nf, sel


def _normal(eng, n, nf, same_file=True, slot=0):
    eng.candidates_run_mixed(n, nf, same_file=same_file, slot=slot)
    return eng.candidates_fetch(n, slot=slot).copy()


def _same(a, b):
    """two (records, paths, ops) results, byte for byte"""
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("tile_size,tile_overlap", [(320, 120), (512, 192), (64, 24)])
def test_a_sample_of_both_strands_equals_the_model(oracle, scoring, tile_size, tile_overlap):
    blk, cands, nf, sel = _small()
    kw = dict(tile_size=tile_size, tile_overlap=tile_overlap, scoring=scoring)
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, **kw)
    normal = _normal(eng, n, nf)
    got = eng.candidates_paths(sel=sel, rc_from=nf)
    eng.close()
    exp = expected(oracle, blk.rs, cands, nf, sel, **kw)
    assert sum(e["n_columns"] > 0 for e in exp) > len(sel) // 2
    assert_equals_model(exp, blk.rs, cands, nf, sel, normal, *got, scoring)


@pytest.mark.parametrize("scoring", SCORINGS)
def test_raw_byte_reads_equal_the_model(oracle, scoring):
    """reads with N and lower case take the raw-byte kernels: = / X by raw byte equality (case matters, N == N,
    align.cpp:134), every candidate"""
    from conftest import workload_block
    blk = workload_block("tiny")
    rs = path_cases.n_and_lower_case(blk.rs)
    cands = np.concatenate([blk.cf, blk.cr])
    eng, n, nf = engine_with(rs, blk.cf, blk.cr, scoring=scoring)
    normal = _normal(eng, n, nf)
    got = eng.candidates_paths(n=n, rc_from=nf)
    eng.close()
    assert nf > 0 and n > nf
    assert_equals_model(expected(oracle, rs, cands, nf, scoring=scoring), rs, cands, nf, None, normal, *got, scoring)


@pytest.mark.parametrize("raw", [True, False], ids=["raw-bytes", "acgt"])
@pytest.mark.parametrize("scoring", SCORINGS)
# (320/125: the pointer window begins on a lane's first column; 317/119: a tile that fills no whole lane; 321/121: the first tile
# size on 32 columns per lane -- tests/planted_tiles.py GEOMETRIES)
@pytest.mark.parametrize("tile_size,tile_overlap", [(320, 120), (64, 24), (320, 125), (317, 119), (321, 121)])
def test_crafted_candidates_equal_the_model(oracle, tile_size, tile_overlap, scoring, raw):
    """in order (sel = None), as a reversed selection, and with same_file off (the same ops; `emitted` as the normal run
    with same_file off says)"""
    cr = path_cases.crafted(raw)
    cands = np.concatenate([cr.cf, cr.cr])
    kw = dict(tile_size=tile_size, tile_overlap=tile_overlap, scoring=scoring)
    eng, n, nf = engine_with(cr.rs, cr.cf, cr.cr, **kw)
    normal = _normal(eng, n, nf)
    in_order = eng.candidates_paths(n=n, rc_from=nf)
    rev = np.arange(n, dtype=np.int32)[::-1].copy()
    backwards = eng.candidates_paths(sel=rev, rc_from=nf)
    normal_two_files = _normal(eng, n, nf, same_file=False)
    two_files = eng.candidates_paths(n=n, rc_from=nf, same_file=False)
    eng.close()
    exp = expected(oracle, cr.rs, cands, nf, **kw)
    assert_equals_model(exp, cr.rs, cands, nf, None, normal, *in_order, scoring, names=cr.names)
    assert_equals_model(exp[::-1], cr.rs, cands, nf, rev, normal, *backwards, scoring, names=cr.names)
    assert_equals_model(exp, cr.rs, cands, nf, None, normal_two_files, *two_files, scoring, names=cr.names)
    assert two_files[1].tobytes() == in_order[1].tobytes() and two_files[2].tobytes() == in_order[2].tobytes()
    # a read against itself: nothing to emit within one file, and its path is there all the same
    own = np.flatnonzero(cands["ref_id"] == cands["query_id"])
    assert len(own) >= 6 and not in_order[0]["emitted"][own].any() and (in_order[1]["n_columns"][own] > 0).all()
    assert normal_two_files["emitted"][own].any()


def test_one_block_walking_every_candidate_gives_what_the_default_grid_gives(oracle):
    """max_blocks = 1: every group pops many candidates one after another (n_left / n_right start again at each)"""
    blk, cands, nf, sel = _small()
    # (the sampled candidates alone, forward ones first: a normal run of the whole workload on one block takes minutes)
    order = np.concatenate([np.sort(sel[sel < nf]), np.sort(sel[sel >= nf])])
    cf, cr = cands[order[order < nf]], cands[order[order >= nf]]
    mine = np.searchsorted(order, sel).astype(np.int32)               # sel's candidates, in sel's order, in the short list
    short = np.concatenate([cf, cr])
    assert short[mine].tobytes() == cands[sel].tobytes()
    got = {}
    for max_blocks in (0, 1):
        eng, n, n_f = engine_with(blk.rs, cf, cr, max_blocks=max_blocks)
        if max_blocks == 0:
            normal = _normal(eng, n, n_f)
        got[max_blocks] = eng.candidates_paths(sel=mine, rc_from=n_f)
        eng.close()
    _same(got[0], got[1])
    assert_equals_model(expected(oracle, blk.rs, short, len(cf), mine), blk.rs, short, len(cf), mine, normal, *got[1], LINEAR)


def test_what_a_slot_keeps_between_runs_does_not_show(oracle):
    """a shorter path run after a longer one (column bytes and counts of the longer one are still on the device), a normal
    run after path runs (they share the slot's workspace), the first path run once more; and slot 1 of a two-slot engine"""
    blk, cands, nf, sel = _small()
    exp = expected(oracle, blk.rs, cands, nf, sel)
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    normal = _normal(eng, n, nf)
    whole = eng.candidates_paths(sel=sel, rc_from=nf)
    seven = eng.candidates_paths(sel=sel[:7], rc_from=nf)
    normal_again = _normal(eng, n, nf)
    whole_again = eng.candidates_paths(sel=sel, rc_from=nf)
    eng.close()
    assert_equals_model(exp, blk.rs, cands, nf, sel, normal, *whole, scoring=LINEAR)
    assert_equals_model(exp[:7], blk.rs, cands, nf, sel[:7], normal, *seven, scoring=LINEAR)
    n_ops = int(whole[1]["n_ops"][:7].sum())
    assert seven[0].tobytes() == whole[0][:7].tobytes() and seven[1].tobytes() == whole[1][:7].tobytes()
    assert len(seven[2]) == n_ops and seven[2].tobytes() == whole[2][:n_ops].tobytes()
    assert normal_again.tobytes() == normal.tobytes()
    _same(whole, whole_again)
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, slots=(0, 1), n_slots=2)
    slot1 = eng.candidates_paths(sel=sel, rc_from=nf, slot=1)
    slot0 = eng.candidates_paths(sel=sel, rc_from=nf, slot=0)
    eng.close()
    _same(whole, slot1)
    _same(whole, slot0)


def test_paths_of_the_device_filters_own_list(oracle):
    """dsoft_query leaves the candidates on the device and the host holds no copy: the path run copies the list back.  The
    same list uploaded to a fresh engine gives the same bytes, and a sample equals the model."""
    from gact_amd import engine
    from conftest import workload_block
    blk = workload_block("tiny")
    eng, _, _ = engine_with(blk.rs, blk.cf[:0], blk.cr[:0], slots=())
    eng.dsoft_build()
    nf, nr, _ = eng.dsoft_query(0, len(blk.rs.reads))
    n = nf + nr
    assert nf > 0 and nr > 0
    filtered = eng.candidates_paths(n=n, rc_from=nf)                     # (before any normal run on this engine)
    normal_filtered = _normal(eng, n, nf)
    cands = eng.candidates_download(n)
    eng.close()
    fresh, n2, nf2 = engine_with(blk.rs, cands[:nf], cands[nf:])
    assert (n2, nf2) == (n, nf)
    normal = _normal(fresh, n, nf)
    uploaded = fresh.candidates_paths(n=n, rc_from=nf)
    fresh.close()
    _same(filtered, uploaded)
    assert normal_filtered.tobytes() == normal.tobytes() == filtered[0].tobytes()
    sel = path_cases.sample(nf, nr, 50, seed=7)
    records, paths, ops = uploaded
    picked_ops = np.concatenate([ops_of(paths, ops, k) for k in sel.tolist()])
    picked = paths[sel].copy()
    picked["op_offset"] = np.cumsum(np.concatenate([[0], picked["n_ops"][:-1]]))
    assert len(sel) == 50
    assert_equals_model(expected(oracle, blk.rs, cands, nf, sel), blk.rs, cands, nf, sel, normal, records[sel], picked,
                        picked_ops, LINEAR)
