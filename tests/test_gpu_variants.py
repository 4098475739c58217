"""GPU suite for the variants of the pileup (gact_hip_pileup_variants): on every planted case of tests/variant_cases.py the
device's records, table and statistics equal tests/variant_model.py's on the device's own counts, field by field, and the
records are the ones the case was planted for; the capacity protocol; every refusal, with the outputs untouched; the call again
with other parameters after one more add; two slots adding from two threads; a window without slots; truth block V and the
driver's --vcf (tests/variant_truth.py).  Exact equality everywhere: integers are equal or the test fails."""
import ctypes
import threading

import numpy as np
import pytest

import variant_cases
import variant_model
from path_cases import engine_with
from variant_model import DEL_KIND, INS_KIND, SNV_KIND

pytestmark = pytest.mark.gpu

CASES = variant_cases.cases()


def _engine(case, **kw):
    from gact_amd import engine
    none = np.zeros(0, dtype=engine.CAND_DTYPE)
    eng, n, nf = engine_with(case.rs, case.cands, none, threshold=variant_cases.THRESHOLD, **kw)
    assert n == nf == len(case.cands)
    return eng, n


def _begin_and_add(eng, case, n, ins_slots=None):
    eng.pileup_begin(case.window[0], case.window[1], ins_slots=case.ins_slots if ins_slots is None else ins_slots)
    eng.pileup_add(n=n, rc_from=n)


def _model(eng, case, slots=None, **params):
    """the model on the counts and the slot table the device holds"""
    _, counts, _ = eng.pileup_finish(min_depth=1)
    slots = case.ins_slots if slots is None else slots
    ins = eng.pileup_corrected(min_depth=1, ins=True)[3] if slots else None
    own, offs = variant_cases.own_and_offsets(case)
    return variant_model.variants(counts, ins, own, offs, seq_first=case.window[0], **params)


def _same(got, want, what=""):
    (recs, table), (m_recs, m_table) = got, want
    assert recs.dtype == m_recs.dtype and table.dtype == m_table.dtype
    assert recs.tolist() == m_recs.tolist(), what
    assert recs.tobytes() == m_recs.tobytes() and table.tobytes() == m_table.tobytes(), (what, table, m_table)


def _check_stats(st, table, positions):
    want = variant_model.stats_of(table)
    assert {k: st[k] for k in want} == want
    assert st["chunks"] == -(-positions // variant_cases.CHUNK) and st["device_ms"] > 0
    assert st["scratch_bytes"] >= positions + 8 * st["chunks"] + 32 * len(table) + 32 * (want["n_ins"] + want["n_del"] + want["n_snv"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_planted_case_equals_the_model_and_what_it_was_planted_for(name):
    case = CASES[name]
    eng, n = _engine(case)
    _begin_and_add(eng, case, n)
    got = eng.pileup_variants(table=True, **case.params)
    st = eng.last_variant_stats()
    again = eng.pileup_variants(table=True, **case.params)                       # the counts stay, and so does the answer
    want = _model(eng, case, **case.params)
    eng.close()
    _same(got, want, name)
    _same(again, want, name + ", again")
    assert got[0].tolist() == case.want.tolist(), name
    _check_stats(st, want[1], len(variant_cases.own_and_offsets(case)[0]))


def test_the_capacity_protocol_and_the_counts_stay():
    from gact_amd import engine
    case = CASES["several"]
    eng, n = _engine(case)
    _begin_and_add(eng, case, n)
    before = eng.pileup_finish(min_depth=1)
    want, table = eng.pileup_variants(table=True, **case.params)
    assert len(want) == len(case.want) > 4
    p = engine.VariantParams(*(case.params[k] for k in ("min_depth", "min_alt", "min_permille", "hom_permille")))
    L, count = eng.L, ctypes.c_int64(-1)
    # only the number
    assert L.gact_hip_pileup_variants(eng.h, ctypes.byref(p), None, 0, ctypes.byref(count), None) == 0 and count.value == len(want)
    # too little room: refused, with the number and the table filled in and the records' room untouched
    small = np.full(len(want) - 1, 0x55, dtype=np.uint8).repeat(32).view(engine.VARIANT_DTYPE)
    seqs = np.zeros(case.window[1], dtype=engine.SEQ_VARIANTS_DTYPE)
    count.value = -1
    rc = L.gact_hip_pileup_variants(eng.h, ctypes.byref(p), small.ctypes.data, len(small), ctypes.byref(count), seqs.ctypes.data)
    assert rc == -1 and ("pileup_variants: %d records, room for %d: call again" % (len(want), len(small))).encode() in L.gact_hip_last_error()
    assert count.value == len(want) and seqs.tobytes() == table.tobytes() and (small.view(np.uint8) == 0x55).all()
    # exact room; more room than records leaves the rest alone
    exact = np.zeros(count.value, dtype=engine.VARIANT_DTYPE)
    assert L.gact_hip_pileup_variants(eng.h, ctypes.byref(p), exact.ctypes.data, len(exact), None, None) == 0
    assert exact.tobytes() == want.tobytes()
    wide = np.full((len(want) + 3) * 32, 0x55, dtype=np.uint8).view(engine.VARIANT_DTYPE)
    assert L.gact_hip_pileup_variants(eng.h, ctypes.byref(p), wide.ctypes.data, len(wide), ctypes.byref(count), None) == 0
    assert wide[:len(want)].tobytes() == want.tobytes() and (wide[len(want):].view(np.uint8) == 0x55).all()
    # NULL parameters are the defaults
    assert L.gact_hip_pileup_variants(eng.h, None, None, 0, ctypes.byref(count), None) == 0
    assert count.value == len(eng.pileup_variants())
    # the window's counts, consensus and table are as they were
    after = eng.pileup_finish(min_depth=1)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    # an empty window; a window of the one-base target alone
    eng.pileup_begin(case.window[0], 0)
    recs, tab = eng.pileup_variants(table=True)
    assert len(recs) == 0 and tab.shape == (0,) and eng.last_variant_stats()["chunks"] == 0
    eng.pileup_begin(case.window[0], 1)
    eng.pileup_add(n=n, rc_from=n)
    recs, tab = eng.pileup_variants(table=True, min_depth=4, min_alt=2)
    assert len(recs) == 0 and tab["examined"].tolist() == [1] and tab["first"].tolist() == [0]
    eng.close()


def test_every_refusal_leaves_the_outputs_untouched():
    from gact_amd import engine
    case = CASES["hom"]
    eng, n = _engine(case)
    L = eng.L
    room = np.full(8 * 32, 0x55, dtype=np.uint8).view(engine.VARIANT_DTYPE)
    seqs = np.full(case.window[1] * 32, 0x55, dtype=np.uint8).view(engine.SEQ_VARIANTS_DTYPE)
    count = ctypes.c_int64(-7)

    def refused(params, why, cap=8):
        p = None if params is None else ctypes.byref(engine.VariantParams(*params))
        assert L.gact_hip_pileup_variants(eng.h, p, room.ctypes.data, cap, ctypes.byref(count), seqs.ctypes.data) == -1
        assert why in L.gact_hip_last_error(), L.gact_hip_last_error()
        assert count.value == -7 and (room.view(np.uint8) == 0x55).all() and (seqs.view(np.uint8) == 0x55).all()

    refused(None, b"pileup_variants: no window is open")
    with pytest.raises(engine.GactHipError, match="error -1: pileup_variants: no window is open"):
        eng.pileup_variants()
    with pytest.raises(engine.GactHipError, match="error -1: last_variant_stats: no gact_hip_pileup_variants call has run"):
        eng.last_variant_stats()
    _begin_and_add(eng, case, n)
    refused((0, 4, 250, 750), b"min_depth = 0, at least 1")
    refused((8, 0, 250, 750), b"min_alt = 0, at least 1")
    refused((8, 4, -1, 750), b"min_permille = -1")
    refused((8, 4, 751, 750), b"min_permille = 751, hom_permille = 750")
    refused((8, 4, 250, 1001), b"hom_permille = 1001")
    refused(None, b"pileup_variants: cap = -1", cap=-1)
    for bad in (dict(min_depth=0), dict(min_alt=-3), dict(min_permille=600, hom_permille=500)):
        with pytest.raises(engine.GactHipError, match="error -1: pileup_variants: min_"):
            eng.pileup_variants(**bad)
    # the edges of what is allowed are allowed
    assert len(eng.pileup_variants(min_depth=1, min_alt=1, min_permille=0, hom_permille=0)) >= len(case.want)
    assert len(eng.pileup_variants(min_depth=4, min_alt=4, min_permille=1000, hom_permille=1000)) == len(case.want)
    cat, offs = case.rs.concat()
    eng.upload(engine.SET_REF, cat, offs)
    refused(None, b"pileup_variants: GACT_SET_REF was uploaded after")
    eng.close()


def test_again_with_other_parameters_after_one_more_add():
    case = CASES["ins"]
    eng, n = _engine(case)
    _begin_and_add(eng, case, n)
    first = eng.pileup_variants(table=True, **case.params)
    _same(first, _model(eng, case, **case.params), "one add")
    eng.pileup_add(n=n, rc_from=n)                                              # every alignment once more: twice the counts
    d, a = case.params["min_depth"], case.params["min_alt"]
    for params in (dict(min_depth=2 * d, min_alt=2 * a, min_permille=250, hom_permille=750), dict(min_depth=2 * d, min_alt=2 * a + 1),
                   dict(min_depth=1, min_alt=1, min_permille=0, hom_permille=500), dict(min_depth=2 * d + 1)):
        got = eng.pileup_variants(table=True, **params)
        _same(got, _model(eng, case, **params), str(params))
        _check_stats(eng.last_variant_stats(), got[1], len(variant_cases.own_and_offsets(case)[0]))
    twice = eng.pileup_variants(min_depth=2 * d, min_alt=2 * a)
    assert len(twice) == len(first[0]) and np.array_equal(twice["alt"], 2 * first[0]["alt"]) and np.array_equal(twice["depth"], 2 * first[0]["depth"])
    for k in ("seq", "pos", "kind", "len", "bases", "flags"):
        assert np.array_equal(twice[k], first[0][k]), k
    assert len(eng.pileup_variants(min_depth=2 * d, min_alt=2 * a + 1)) == 0 and len(eng.pileup_variants(min_depth=2 * d + 1)) == 0
    eng.close()


def test_two_slots_adding_from_two_threads_give_the_same_bytes_as_one():
    case = CASES["several"]
    eng, n = _engine(case, slots=(0, 1), n_slots=2)
    _begin_and_add(eng, case, n)
    one = eng.pileup_variants(table=True, **case.params)
    eng.pileup_begin(case.window[0], case.window[1], ins_slots=case.ins_slots)
    errors = []

    def feeder(slot):
        try:
            for piece in np.array_split(np.arange(slot, n, 2, dtype=np.int32), 3):
                eng.pileup_add(sel=piece, rc_from=n, slot=slot)
        except Exception as e:                       # (shown by the assertion below)
            errors.append(e)

    threads = [threading.Thread(target=feeder, args=(slot,)) for slot in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    two = eng.pileup_variants(table=True, **case.params)
    eng.close()
    _same(two, one)
    assert one[0].tolist() == case.want.tolist()


@pytest.mark.parametrize("name", ["ins", "several"])
def test_a_window_without_slots_makes_no_ins_records_and_the_other_records_the_same(name):
    case = CASES[name]
    eng, n = _engine(case)
    _begin_and_add(eng, case, n)
    with_slots, t_slots = eng.pileup_variants(table=True, **case.params)
    _begin_and_add(eng, case, n, ins_slots=0)
    without, t_none = eng.pileup_variants(table=True, **case.params)
    _same((without, t_none), _model(eng, case, slots=0, **case.params))
    eng.close()
    assert (with_slots["kind"] == INS_KIND).sum() >= 2 and not (without["kind"] == INS_KIND).any()
    assert without.tobytes() == with_slots[with_slots["kind"] != INS_KIND].tobytes()
    assert not t_none["n_ins"].any() and np.array_equal(t_none["n_del"], t_slots["n_del"]) and np.array_equal(t_none["n_snv"], t_slots["n_snv"])
    assert np.array_equal(t_none["examined"], t_slots["examined"]) and {DEL_KIND, SNV_KIND} <= set(without["kind"].tolist())


# ---- truth block V (tests/variant_truth.py) and the driver's --vcf

def _engine_v(n_slots=1, candidates=True):
    from gact_amd import engine
    import variant_truth
    b = variant_truth.block_v()
    eng = engine.Engine(n_slots=n_slots)
    eng.upload_seqs(engine.SET_REF, b["seqs"])
    eng.upload_seqs(engine.SET_QUERY, b["reads"])
    eng.upload_seqs(engine.SET_QUERY_RC, b["rc"])
    if candidates:
        eng.candidates_upload(b["cands"])
    return eng, b


def test_block_v_the_devices_records_equal_the_model_and_find_what_the_reference_path_finds(oracle):
    import variant_truth
    eng, b = _engine_v()
    n, nf = len(b["cands"]), b["nf"]
    eng.pileup_begin(ins_slots=variant_truth.K)
    eng.pileup_add(n=n, rc_from=nf, same_file=False)
    got = eng.pileup_variants(table=True, **variant_truth.PARAMS)
    st = eng.last_variant_stats()
    _, counts, _ = eng.pileup_finish(min_depth=1)
    ins = eng.pileup_corrected(min_depth=1, ins=True)[3]
    # every base any alignment disagrees in: more records than the binding's first call has room for, and than the pass held
    loose = dict(min_depth=1, min_alt=1, min_permille=0, hom_permille=1000)
    many = eng.pileup_variants(table=True, **loose)
    st_many = eng.last_variant_stats()
    eng.close()
    own, offs = variant_truth.own_and_offsets()
    _same(got, variant_model.variants(counts, ins, own, offs, **variant_truth.PARAMS), "block V")
    assert len(many[0]) > 4096
    _same(many, variant_model.variants(counts, ins, own, offs, **loose), "block V, every disagreement")
    _check_stats(st_many, many[1], len(own))
    _check_stats(st, got[1], len(own))
    ref = variant_truth.reference_path(oracle)
    f = variant_truth.figures(got[0])
    print("block V, the device:", f)
    assert f == ref["figures"]                          # integer work on bit-exact records: no margin
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(ins, ref["ins"]) and got[0].tobytes() == ref["records"].tobytes()
    variant_truth.check(f)


def _feeders(eng, b, n_threads, parents_only):
    """what the driver's feeders add, through the binding: reads [lo, hi) per feeder, filtered, extended, the emitted records
    stacked -- with parents_only the ones gact_hip_place_reads makes primary or supplementary"""
    from gact_amd import engine
    n_reads = len(b["reads"])
    lens = np.array([len(r) for r in b["reads"]], dtype=np.int32)
    per_thread = -(-n_reads // n_threads)
    for t in range(n_threads):
        lo = min(n_reads, t * per_thread)
        hi = min(n_reads, lo + per_thread)
        nf, nr, _ = eng.dsoft_query(lo, hi - lo)
        n = nf + nr
        eng.candidates_run_mixed(n, rc_from=nf, same_file=False)
        records = eng.candidates_fetch(n).copy()
        sel = np.flatnonzero(records["emitted"] != 0).astype(np.int32)
        if parents_only:
            _, sums = eng.candidates_summaries(sel=sel, rc_from=nf, same_file=False)
            place, _ = eng.place_reads(lens[lo:hi], read_first=lo, n=n, sel=sel, sums=sums)
            sel = sel[(place["kind"] == engine.PLACE_PRIMARY) | (place["kind"] == engine.PLACE_SUPPLEMENTARY)]
        eng.pileup_add(sel=sel, rc_from=nf, same_file=False)


def test_driver_vcf(tmp_path):
    import os
    import subprocess
    from gact_amd import engine, workload
    import variant_truth
    b = variant_truth.block_v()
    variant_truth.write_fasta(str(tmp_path / "ref.fa"), b["names"], b["seqs"])
    variant_truth.write_fasta(str(tmp_path / "reads.fa"), b["read_names"], b["reads"])
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()
    P = variant_truth.PARAMS
    depth, vcf = str(P["min_depth"]), "%d:%d:%d" % (P["min_alt"], P["min_permille"], P["hom_permille"])

    def run(name, *extra, ok=True):
        d = tmp_path / name
        d.mkdir()
        for f in ("ref.fa", "reads.fa", "params.cfg"):
            os.symlink(tmp_path / f, d / f)
        out = subprocess.run([drv, "ref.fa", "reads.fa", "2", "--device-dsoft"] + list(extra), capture_output=True, text=True, cwd=d, timeout=600)
        assert (out.returncode == 0) == ok, out.stdout + out.stderr
        return out, {p.name: p.read_bytes() for p in d.iterdir() if p.name.startswith("darwin.")}

    header = ["##fileformat=VCFv4.2"] + ["##contig=<ID=%s,length=%d>" % (nm, len(s)) for nm, s in zip(b["names"], b["seqs"])]
    for name, extra in (("plain", ()), ("sam", ("--sam", "primary"))):
        _, without = run(name + "_without", "--pileup", depth, "--ins-slots", str(variant_truth.K), *extra)
        _, files = run(name, "--pileup", depth, "--ins-slots", str(variant_truth.K), "--vcf", vcf, *extra)
        assert sorted(files) == sorted(list(without) + ["darwin.vcf"])
        if not extra:                                   # (with --sam the adds take the placed parents only: another consensus)
            assert all(files[f] == without[f] for f in without)
        else:
            assert all(files[f] == without[f] for f in without if f != "darwin.cons.fa")
        lines = files["darwin.vcf"].decode().splitlines(keepends=True)
        head = [l.rstrip("\n") for l in lines if l.startswith("#")]
        assert head[:len(header)] == header and head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tdarwin"
        assert [l[:13] for l in head[len(header):-1]] == ["##INFO=<ID=DP", "##INFO=<ID=AD", "##FORMAT=<ID="] and "ID=GT" in head[-2]
        body = [l for l in lines if not l.startswith("#")]
        # the same reads, parameters and selection through Engine, feeder by feeder
        eng, _ = _engine_v(candidates=False)
        eng.dsoft_build()
        eng.pileup_begin(ins_slots=variant_truth.K)
        _feeders(eng, b, 2, parents_only=bool(extra))
        recs = eng.pileup_variants(**P)
        eng.close()
        assert body == [variant_model.format_vcf(r, b["names"][int(r["seq"])], b["seqs"][int(r["seq"])]) for r in recs], name
        assert body == [engine.format_vcf(r, b["names"][int(r["seq"])], b["seqs"][int(r["seq"])]) for r in recs]
        pos = {}
        for l in body:
            f = l.split("\t")
            assert pos.get(f[0], 0) <= int(f[1]), l   # POS never decreases inside a contig
            pos[f[0]] = int(f[1])
        f = variant_truth.figures(recs)
        print("block V through the driver's own candidates, %s:" % name, f)
        assert f["snv_found"] > 0 and f["indel_found"] > 0
    # refused without --pileup and with a malformed argument, with nothing written
    for extra in (("--vcf", vcf), ("--pileup", depth, "--vcf", "4:250"), ("--pileup", depth, "--vcf", "0:250:750"),
                  ("--pileup", depth, "--vcf", "4:800:750"), ("--pileup", depth, "--vcf", "4:250:1001"), ("--pileup", depth, "--vcf", "4:250:750x")):
        out, left = run("refused_%d" % len(os.listdir(tmp_path)), *extra, ok=False)
        assert "--vcf" in out.stderr and not left
