"""GPU suite of the D-SOFT filter's edge cases (tests/dsoft_cases.py; tests/test_dsoft_model.py proves on the CPU that
each case reaches its path): the device list (dsoft_build + dsoft_query + candidates_download, strand-major) equals,
element by element and in order, the reference's own list (`reflib`: its recorded answers where oracle/_ref is not
built), and the model's (tests/dsoft_model.py) for the strands the reference does not define; the places are listed in
tests/test_dsoft_model.py.  Then the engine's state between calls: sub-ranges, repeats, a second build, two slots, the
re-sized staging area, and the hand-over to GACT."""
import numpy as np
import pytest

import dsoft_cases

pytestmark = pytest.mark.gpu


def as_arrays(seqs):
    return [np.frombuffer(s, dtype=np.uint8) for s in seqs]


def upload(eng, c):
    from gact_amd import engine
    eng.upload_seqs(engine.SET_REF, as_arrays(c.reads))
    eng.upload_seqs(engine.SET_QUERY, as_arrays(c.reads))
    eng.upload_seqs(engine.SET_QUERY_RC, as_arrays(c.rc))


def build(eng, c):
    from gact_amd import engine
    upload(eng, c)
    return eng.dsoft_build(engine.DsoftParams(**c.params))


def query(eng, first, n, slot=0):
    nf, nr, _ = eng.dsoft_query(first, n, slot=slot)
    return listed(eng.candidates_download(nf + nr, slot=slot), nf)


def listed(cands, nf):
    return [(int(x["ref_id"]), int(x["query_id"]), int(x["ref_pos"]), int(x["query_pos"]), int(k >= nf))
            for k, x in enumerate(cands)]


def sub_list(want, first, n):
    return [x for x in want if first <= x[1] < first + n]


@pytest.mark.parametrize("name", dsoft_cases.NAMES)
def test_device_equals_reference(reflib, name):
    from gact_amd import engine
    c = dsoft_cases.case(name)
    want = dsoft_cases.expected(reflib, c)
    eng = engine.Engine()
    info = build(eng, c)
    got = query(eng, 0, len(c.reads))
    assert len(want) > 0 and got == want
    assert info["ref_length"] == c.ref_len() and info["max_occurrence"] == c.max_occ()
    # a sub-range of the queries gives the matching sub-list; the same range again gives the same list
    first, n = 1, max(1, len(c.reads) - 2)
    assert query(eng, first, n) == sub_list(want, first, n)
    assert query(eng, first, n) == sub_list(want, first, n)
    assert query(eng, 0, len(c.reads)) == want
    eng.close()


def test_threshold_plus_seed_size_of_256_is_refused():
    from gact_amd import engine
    c = dsoft_cases.case("full_counter")
    eng = engine.Engine()
    upload(eng, c)
    with pytest.raises(engine.GactHipError):
        eng.dsoft_build(engine.DsoftParams(**dict(c.params, threshold=c.params["threshold"] + 1)))
    eng.close()


@pytest.mark.parametrize("names", [("seed_cut_0", "many_hits_bin64"), ("many_hits_bin64", "seed_cut_0"),
                                   ("low_threshold_1", "padding"), ("full_counter", "seed_cut_1")])
def test_second_build_with_other_parameters_on_one_engine(reflib, names):
    """the band table and the staging area of a wave are sized from the parameters at the first query after a build:
    the smaller table first, and the larger first"""
    from gact_amd import engine
    a, b = (dsoft_cases.case(n) for n in names)
    assert a.band_slots() != b.band_slots()
    eng = engine.Engine()
    for c in (a, b, a):
        build(eng, c)
        assert query(eng, 0, len(c.reads)) == dsoft_cases.expected(reflib, c), c.name
    eng.close()


def test_two_slots_give_the_same_list_and_leave_each_other_alone(reflib):
    from gact_amd import engine
    c = dsoft_cases.case("many_hits_bin4096")
    want = dsoft_cases.expected(reflib, c)
    eng = engine.Engine(n_slots=2)
    build(eng, c)
    n = len(c.reads)
    assert query(eng, 0, n, slot=1) == want
    assert query(eng, 0, n, slot=0) == want
    part = query(eng, 1, 3, slot=1)
    assert part == sub_list(want, 1, 3) and len(part) < len(want)
    nf0 = sum(1 for x in want if x[4] == 0)
    assert listed(eng.candidates_download(len(want), slot=0), nf0) == want        # slot 0 still holds its own
    part0 = query(eng, 2, 2, slot=0)
    nf1 = sum(1 for x in part if x[4] == 0)
    assert listed(eng.candidates_download(len(part), slot=1), nf1) == part
    assert part0 == sub_list(want, 2, 2)
    eng.close()


@pytest.mark.parametrize("name", ["many_hits_bin64", "many_hits_bin4096"])
def test_many_hits_through_the_resized_staging_area(reflib, monkeypatch, name):
    """GACT_HIP_DSOFT_TEMP_CAP=8: the candidates do not fit, the area is sized from the exact counts, the filter runs again"""
    from gact_amd import engine
    c = dsoft_cases.case(name)
    monkeypatch.setenv("GACT_HIP_DSOFT_TEMP_CAP", "8")
    eng = engine.Engine()
    build(eng, c)
    assert query(eng, 0, len(c.reads)) == dsoft_cases.expected(reflib, c)
    eng.close()


def test_many_hits_from_the_device_list_straight_into_gact(oracle):
    from gact_amd import engine
    c = dsoft_cases.case("many_hits_bin64")
    cat = np.frombuffer(b"".join(c.reads), dtype=np.uint8)
    rcat = np.frombuffer(b"".join(c.rc), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in c.reads])]).astype(np.int64)
    eng = engine.Engine()
    eng.upload(engine.SET_REF, cat, offs)
    eng.upload(engine.SET_QUERY, cat, offs)
    eng.upload(engine.SET_QUERY_RC, rcat, offs)
    eng.dsoft_build(engine.DsoftParams(**c.params))
    nf, nr, _ = eng.dsoft_query(0, len(c.reads))
    assert nf > 0 and nr > 0
    eng.candidates_run_mixed(nf + nr, rc_from=nf, same_file=True)
    rec = eng.candidates_fetch(nf + nr)
    cands = eng.candidates_download(nf + nr)
    assert listed(cands, nf) == c.model()[0]
    for comp, sl, qcat in ((False, slice(0, nf), cat), (True, slice(nf, nf + nr), rcat)):
        want, _ = oracle.gact_many(cat, offs, qcat, offs, cands[sl], complement=comp, same_file=True, n_threads=8)
        for field in ("ab", "ae", "bb", "be", "score", "emitted", "n_tiles", "cells"):
            assert np.array_equal(rec[sl][field], want[field]), field
    eng.close()
