"""GPU suite for the placement of reads (gact_hip_place_reads, csrc/gact_place.hpp): the per-record places and the per-read
table equal the model's (tests/place_model.py) field by field -- on crafted host records of every pattern and size (no
alignment runs), on the device-resident records of a run of both strands ahead of the fetch, on chimeric reads against a
reference set (two files), through the refusals, and through the driver's --sam.  No tolerance anywhere."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import place_model
from place_model import CASES, crafted, place, stats_of

pytestmark = pytest.mark.gpu

STAT_KEYS = ("reads", "max_records", "counted", "parents", "secondaries", "extras")


@pytest.fixture(scope="module")
def eng():
    """an engine that aligns nothing: two slots, workspaces for one block"""
    from gact_amd import engine
    e = engine.Engine(n_slots=2, max_blocks=1)
    yield e
    e.close()


_MODEL = {}


def _case(pattern, m):
    """(records, read_lens, the call's keyword arguments, the model's (place, reads)) of a crafted case, made once"""
    if (pattern, m) not in _MODEL:
        c = crafted(pattern, m)
        rec, lens = c.pop("records"), c.pop("read_lens")
        _MODEL[(pattern, m)] = (rec, lens, c, place(rec, lens, **c))
    return _MODEL[(pattern, m)]


def _equal(got, want, what):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and len(a) == len(b), what
        for name in a.dtype.names:
            bad = np.flatnonzero(a[name] != b[name])
            assert len(bad) == 0, (what, name, bad[:5].tolist(), a[bad[:5]].tolist(), b[bad[:5]].tolist())


@pytest.mark.parametrize("pattern", list(dict.fromkeys(p for p, _ in CASES)))
def test_crafted_host_records_equal_the_model_at_every_size(eng, pattern):
    sizes = [m for p, m in CASES if p == pattern]
    assert sizes
    for m in sizes:
        rec, lens, kw, want = _case(pattern, m)
        before = rec.tobytes()
        got = eng.place_reads(lens, records=rec, **kw)
        _equal(got, want, (pattern, m))
        if len(want[0]):
            st = eng.last_place_stats()
            assert {k: st[k] for k in STAT_KEYS} == stats_of(*want), (pattern, m)
            assert st["scratch_bytes"] > 0 and st["device_ms"] > 0
        assert rec.tobytes() == before


def test_the_sized_patterns_hold_what_they_are_made_for():
    """(the model's own answers: the GPU is not asked)"""
    for m, extras in ((63, 0), (64, 0), (65, 1), (66, 2)):
        out, reads = _case("chain", m)[3]
        assert reads[0]["n_extra"] == extras and reads[0]["n_supplementary"] == min(m, 64) - 1 and reads[0]["n_secondary"] == 0
    out, reads = _case("stack", 1000)[3]
    assert reads[0]["n_secondary"] == 999 and reads[0]["n_supplementary"] == 0 and reads[1]["primary"] == -1
    out, reads = _case("late_mask", None)[3]
    assert out[64].tolist() == (place_model.SECONDARY, 0, 63, 64) and out[65]["kind"] == out[66]["kind"] == place_model.EXTRA
    assert _case("one_read", None)[3][1][0]["n_records"] == 4097
    assert _case("many_reads", None)[3][1]["n_records"].max() == 3 and len(_case("many_reads", None)[1]) == 70001


def test_the_result_is_the_same_on_every_call_and_on_every_slot(eng):
    for pattern, m, small in (("many_reads", None, ("random", 65)), ("one_read", None, ("chain", 66))):
        rec, lens, kw, want = _case(pattern, m)
        for slot in (0, 0, 1):
            _equal(eng.place_reads(lens, records=rec, slot=slot, **kw), want, (pattern, slot))
        # a smaller call after a larger one on the same scratch, and the larger one again
        s_rec, s_lens, s_kw, s_want = _case(*small)
        _equal(eng.place_reads(s_lens, records=s_rec, **s_kw), s_want, small)
        _equal(eng.place_reads(lens, records=rec, **kw), want, pattern)
    # n < len(records): the first n only
    rec, lens, kw, _ = _case("random", 129)
    _equal(eng.place_reads(lens, n=100, records=rec, **kw), place(rec[:100], lens, **kw), "first n")


def _call(e, slot, n, rec, n_sel, sel, sums, read_first, lens, params, out_place, out_reads, n_reads=None):
    ptr = lambda a: a.ctypes.data if a is not None else None
    return e.L.gact_hip_place_reads(e.h, slot, n, ptr(rec), n_sel, ptr(sel), ptr(sums), read_first, len(lens) if n_reads is None else n_reads,
                                    ptr(lens), ctypes.byref(params) if params is not None else None, ptr(out_place), ptr(out_reads))


def test_refusals_leave_the_outputs_untouched(eng):
    from gact_amd import engine
    e = eng
    rec, lens, kw, want = _case("random", 65)
    read_first = kw["read_first"]
    n = len(rec)
    out_place = np.full(n, -7, dtype=np.int32).repeat(4).view(engine.PLACE_DTYPE)
    out_reads = np.full(len(lens) * 8, -7, dtype=np.int32).view(engine.READ_PLACE_DTYPE)
    untouched = lambda: (out_place.view(np.int32) == -7).all() and (out_reads.view(np.int32) == -7).all()
    P = engine.PlaceParams
    # the parameters
    for params in (P(-1, 60), P(1001, 60), P(500, -1), P(500, 256)):
        assert _call(e, 0, n, rec, 0, None, None, read_first, lens, params, out_place, out_reads) == -1
        assert b"parameters" in e.L.gact_hip_last_error() and untouched()
    # negative n, n_sel, n_reads, read_first
    sel = np.arange(4, dtype=np.int32)
    assert _call(e, 0, -1, rec, 0, None, None, read_first, lens, None, out_place, out_reads) == -1
    assert _call(e, 0, n, rec, -1, sel, None, read_first, lens, None, out_place, out_reads) == -1
    assert _call(e, 0, n, rec, 0, None, None, read_first, lens, None, out_place, out_reads, n_reads=-1) == -1
    assert _call(e, 0, n, rec, 0, None, None, -1, lens, None, out_place, out_reads) == -1
    assert untouched()
    # a negative length
    bad_lens = lens.copy()
    bad_lens[3] = -1
    assert _call(e, 0, n, rec, 0, None, None, read_first, bad_lens, None, out_place, out_reads) == -1
    assert b"negative length" in e.L.gact_hip_last_error() and untouched()
    # a slot without records (slot 1 never held candidates), a slot that is none
    with pytest.raises(engine.GactHipError, match="no records"):
        e.place_reads(lens, n=1, slot=1)
    with pytest.raises(engine.GactHipError, match="slot"):
        e.place_reads(lens, records=rec, slot=2)
    # a sel index outside [0, n), at either end
    for bad in (-1, n):
        sel = np.array([0, 1, bad, 2], dtype=np.int32)
        assert _call(e, 0, n, rec, 4, sel, None, read_first, lens, None, out_place, out_reads) == -1
        assert b"outside [0," in e.L.gact_hip_last_error() and untouched()
    # ERANGE: a counted record's query_id one outside each end of a window with read_first > 0
    assert read_first > 0
    k = int(np.flatnonzero(want[0]["kind"] != place_model.NONE)[0])
    for qid in (read_first - 1, read_first + len(lens)):
        moved = rec.copy()
        moved["query_id"][k] = qid
        assert _call(e, 0, n, moved, 0, None, None, read_first, lens, None, out_place, out_reads) == -4
        assert b"window" in e.L.gact_hip_last_error() and untouched()
        with pytest.raises(ValueError):
            place(moved, lens, **kw)
        # ... and not emitted, it is never looked at
        moved["emitted"][k] = 0
        _equal(e.place_reads(lens, records=moved, **kw), place(moved, lens, **kw), "not emitted outside")
    # zero sizes: no reads writes nothing; no chosen record makes every read empty
    assert _call(e, 0, n, rec, 0, None, None, read_first, lens, None, out_place, out_reads, n_reads=0) == 0 and untouched()
    assert _call(e, 0, n, rec, 0, sel[:0], None, read_first, lens, None, out_place, out_reads) == 0
    assert (out_place.view(np.int32) == -7).all()
    assert (out_reads["primary"] == -1).all() and all((out_reads[f] == 0).all() for f in out_reads.dtype.names if f != "primary")
    # either output may be NULL
    got = np.zeros(n, dtype=engine.PLACE_DTYPE)
    assert _call(e, 0, n, rec, 0, None, None, read_first, lens, None, got, None) == 0
    _equal((got,), want[:1], "place alone")
    got = np.zeros(len(lens), dtype=engine.READ_PLACE_DTYPE)
    assert _call(e, 0, n, rec, 0, None, None, read_first, lens, None, None, got) == 0
    _equal((got,), want[1:], "reads alone")
    with pytest.raises(engine.GactHipError, match="placed no reads"):
        fresh = engine.Engine(max_blocks=1)
        try:
            fresh.last_place_stats()
        finally:
            fresh.close()


@pytest.fixture(scope="module")
def small_run():
    """ecoli10x_small, both strands, run on slot 0: select pair -> summaries -> place, all BEFORE the records are fetched"""
    from conftest import workload_block
    from path_cases import engine_with
    blk = workload_block("ecoli10x_small")
    e, n, nf = engine_with(blk.rs, blk.cf, blk.cr, n_slots=2)
    lens = np.array([len(r) for r in blk.rs.reads], dtype=np.int32)
    e.candidates_run_mixed(n, nf)
    sel = e.select_overlaps(mode="pair")
    _, sums = e.candidates_summaries(sel=sel, rc_from=nf)
    before = dict(run=e.last_run_stats(), select=e.last_select_stats(), summaries=e.last_summaries_stats())
    got = e.place_reads(lens, sel=sel, sums=sums)
    stats = e.last_place_stats()
    after = dict(run=e.last_run_stats(), select=e.last_select_stats(), summaries=e.last_summaries_stats())
    records = e.candidates_fetch(n).copy()
    yield dict(eng=e, n=n, nf=nf, lens=lens, sel=sel, sums=sums, got=got, stats=stats, before=before, after=after, records=records)
    e.close()


def test_device_records_of_a_run_of_both_strands_equal_the_model(small_run):
    r = small_run
    e, records, lens, sel, sums = r["eng"], r["records"], r["lens"], r["sel"], r["sums"]
    want = place(records, lens, sel=sel, sums=sums)
    _equal(r["got"], want, "run")
    assert {k: r["stats"][k] for k in STAT_KEYS} == stats_of(*want)
    assert r["before"] == r["after"]                      # (times included: they are read once and kept)
    kinds = np.bincount(want[0]["kind"], minlength=5)
    print("ecoli10x_small: %d records chosen of %d, %d reads; kinds %s; place %.3f ms, select %.3f ms" %
          (len(sel), r["n"], len(lens), kinds.tolist(), r["stats"]["device_ms"], r["after"]["select"]["device_ms"]))
    assert kinds[place_model.PRIMARY] > len(lens) // 2 and kinds[place_model.SUPPLEMENTARY] > 0 and kinds[place_model.SECONDARY] > 0
    assert e.candidates_fetch(r["n"]).tobytes() == records.tobytes()
    # n beyond the slot's records is refused
    from gact_amd import engine
    with pytest.raises(engine.GactHipError, match="beyond"):
        e.place_reads(lens, n=r["n"] + 1)
    # a second window: the upper half of the reads, and sel restricted to those reads' records
    first = len(lens) // 2
    mine = records["query_id"][sel] >= first
    half = e.place_reads(lens[first:], read_first=first, sel=sel[mine], sums=sums[mine])
    _equal(half, place(records, lens[first:], read_first=first, sel=sel[mine], sums=sums[mine]), "window")
    # ... equals the corresponding slice: kinds, MAPQs and ranks as they are, parents and primaries as positions in the shorter list
    at = np.cumsum(mine) - 1
    whole = want[0][mine].copy()
    whole["parent"] = np.where(whole["parent"] >= 0, at[np.maximum(whole["parent"], 0)], -1)
    table = want[1][first:].copy()
    table["primary"] = np.where(table["primary"] >= 0, at[np.maximum(table["primary"], 0)], -1)
    _equal(half, (whole, table), "slice")


def _revcomp(seq):
    from gact_amd import synth
    return synth.revcomp(seq)


# Piece lengths and seed are chosen on the CPU, on the reference path alone (the host filter's candidates of the two files, the
# oracle's chains, the model): a chain runs on over a junction into the unrelated piece, by several hundred bases and up to
# about a thousand, from both sides, so with a 2,500-base second piece the two records overlap by more than half of the
# shorter one for some of the twelve at every seed tried (eight), and the second piece is a secondary.  With 3,500 bases all
# twelve have their primary on A and a supplementary on B at seven seeds of eight, this one among them.
CHIMERA_SEED, CHIMERA_A, CHIMERA_B, CHIMERAS = 20261020, 4000, 3500, 12


def chimeras(rs, seed=CHIMERA_SEED, len_a=CHIMERA_A, len_b=CHIMERA_B):
    """-> [(query uint8, A, B)]: a verbatim len_a-base piece of the middle of read A, then the reverse complement of a
    verbatim len_b-base piece of the middle of read B"""
    rng = np.random.default_rng(seed)
    long_a = [i for i, r in enumerate(rs.reads) if len(r) >= len_a + 200]
    long_b = [i for i, r in enumerate(rs.reads) if len(r) >= len_b + 200]
    out = []
    while len(out) < CHIMERAS:
        a, b = int(rng.choice(long_a)), int(rng.choice(long_b))
        # different reads from different places of the genome: neither piece aligns to the other's read
        if a == b or abs(int(rs.start[a]) - int(rs.start[b])) < 12000 or any(a == x[1] for x in out):
            continue
        ra, rb = rs.reads[a], rs.reads[b]
        pa, pb = (len(ra) - len_a) // 2, (len(rb) - len_b) // 2
        out.append((np.concatenate([ra[pa:pa + len_a], _revcomp(rb[pb:pb + len_b])]), a, b))
    return out


@pytest.fixture(scope="module")
def chimera_run():
    from conftest import workload_block
    from gact_amd import engine
    rs = workload_block("tiny").rs
    qs = chimeras(rs)
    e = engine.Engine()
    e.upload_seqs(engine.SET_REF, rs.reads)
    e.upload_seqs(engine.SET_QUERY, [q for q, _, _ in qs])
    e.upload_seqs(engine.SET_QUERY_RC, [_revcomp(q) for q, _, _ in qs])
    e.dsoft_build()
    nf, nr, _ = e.dsoft_query(0, len(qs))
    n = nf + nr
    e.candidates_run_mixed(n, rc_from=nf, same_file=False)
    sel = e.select_overlaps(mode="pair")
    _, sums = e.candidates_summaries(sel=sel, rc_from=nf, same_file=False)
    lens = np.array([len(q) for q, _, _ in qs], dtype=np.int32)
    got = e.place_reads(lens, sel=sel, sums=sums)
    records = e.candidates_fetch(n).copy()
    yield dict(rs=rs, qs=qs, lens=lens, sel=sel, sums=sums, got=got, records=records)
    e.close()


def test_chimeras_against_a_reference_set(chimera_run):
    r = chimera_run
    records, sel, got = r["records"], r["sel"], r["got"]
    _equal(got, place(records, r["lens"], sel=sel, sums=r["sums"]), "chimeras")
    out, table = got
    for q, (_, a, b) in enumerate(r["qs"]):
        assert table[q]["primary"] >= 0, q
        prim = records[sel[table[q]["primary"]]]
        assert (prim["query_id"], prim["ref_id"], prim["comp"]) == (q, a, 0), (q, a, b, prim)
        sup = records[sel[np.flatnonzero(out["kind"] == place_model.SUPPLEMENTARY)]]
        assert ((sup["query_id"] == q) & (sup["ref_id"] == b) & (sup["comp"] == 1)).any(), (q, a, b)
    print("chimeras: kinds %s, MAPQ of the primaries %s" % (np.bincount(out["kind"], minlength=5).tolist(), table["mapq"].tolist()))


_CIGAR = re.compile(r"(\d+)([=XIDSH])")


def _check_sam(path, refs, queries, every_read):
    """the file's body lines, each checked against the sequences: {read name: [fields]}"""
    names = list(refs)
    lines = open(path).read().splitlines()
    header = [l for l in lines if l.startswith("@")]
    assert header[0] == "@HD\tVN:1.6\tSO:unsorted" and header[-1].startswith("@PG\tID:darwin_hip")
    assert header[1:-1] == ["@SQ\tSN:%s\tLN:%d" % (nm, len(refs[nm])) for nm in names]
    assert lines[:len(header)] == header
    by_read = {}
    for line in lines[len(header):]:
        f = line.split("\t")
        by_read.setdefault(f[0], []).append(f)
        flag, read = int(f[1]), queries[f[0]]
        if flag & 4:
            assert f[1:9] == ["4", "*", "0", "0", "*", "*", "0", "0"] and f[9] == read and f[10] == "*"
            continue
        ops = [(int(n), op) for n, op in _CIGAR.findall(f[5])]
        assert "".join("%d%s" % o for o in ops) == f[5]
        clip = "S" if not flag & 0x900 else "H"
        assert all(op != ("H" if clip == "S" else "S") for _, op in ops)
        on_query = sum(n for n, op in ops if op in "=XI")
        assert sum(n for n, op in ops if op == clip) + on_query == len(read)
        tags = dict(t.split(":", 1) for t in f[11:])
        assert tags["NM"] == "i:%d" % sum(n for n, op in ops if op in "XID")
        if f[9] == "*":
            assert flag & 256
            continue
        assert not flag & 256
        seq, ref, at, pos = f[9], refs[f[2]], 0, int(f[3]) - 1
        assert len(seq) == (len(read) if clip == "S" else on_query)
        for n, op in ops:
            if op == "S":
                at += n
            elif op == "I":
                at += n
            elif op == "D":
                pos += n
            elif op in "=X":
                same = [seq[at + i].upper() == ref[pos + i].upper() for i in range(n)]
                assert all(same) if op == "=" else not any(same), (f[0], f[5], op, n)
                at, pos = at + n, pos + n
    for name in every_read:
        assert sum(1 for f in by_read.get(name, []) if not int(f[1]) & 0x900) == 1, name
    return by_read


def test_driver_sam(tmp_path, chimera_run):
    from gact_amd import engine, workload
    rs, qs = chimera_run["rs"], chimera_run["qs"]
    rs.write_fasta(str(tmp_path / "ref.fa"))
    with open(tmp_path / "reads.fa", "wb") as f:
        for i, (q, _, _) in enumerate(qs):
            f.write(b">chimera%d\n" % i + q.tobytes() + b"\n")
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    refs = {name: r.tobytes().decode() for name, r in zip(rs.names, rs.reads)}
    queries = {"chimera%d" % i: q.tobytes().decode() for i, (q, _, _) in enumerate(qs)}
    drv = engine.driver_path()

    def run(name, *extra, ok=True):
        d = tmp_path / name
        d.mkdir()
        for f in ("ref.fa", "reads.fa", "params.cfg"):
            os.symlink(tmp_path / f, d / f)
        out = subprocess.run([drv, "ref.fa", "reads.fa", "2"] + list(extra), capture_output=True, text=True, cwd=d, timeout=600)
        assert (out.returncode == 0) == ok, out.stdout + out.stderr
        return d, out

    plain, _ = run("plain", "--device-dsoft")
    sams = {}
    for mode in ("primary", "all"):
        d, _ = run(mode, "--device-dsoft", "--sam", mode)
        sams[mode] = []
        seen = set()
        for t in range(2):
            assert open(d / ("darwin.%d.out" % t), "rb").read() == open(plain / ("darwin.%d.out" % t), "rb").read()
            by_read = _check_sam(d / ("darwin.%d.sam" % t), refs, queries, ())
            assert not seen & set(by_read)
            seen |= set(by_read)
            for name, fs in by_read.items():
                assert sum(1 for f in fs if not int(f[1]) & 0x900) == 1, name
                if mode == "primary":
                    assert not any(int(f[1]) & 256 for f in fs)
                sams[mode] += ["\t".join(f) for f in fs]
        assert seen == set(queries)
    assert set(sams["primary"]) <= set(sams["all"]) and len(sams["primary"]) < len(sams["all"])
    # the truth once more, from the files: the primary on A's strand +, a supplementary on B's strand -
    for i, (_, a, b) in enumerate(qs):
        mine = [l.split("\t") for l in sams["primary"] if l.startswith("chimera%d\t" % i)]
        assert [f[2] for f in mine if int(f[1]) == 0] == [rs.names[a]]
        assert any(f[2] == rs.names[b] and int(f[1]) == 2048 + 16 for f in mine)
    # the combinations that are refused, with nothing written
    for extra in (("--sam", "primary"), ("--device-dsoft", "--sam", "best"), ("--device-dsoft", "--shard", "0/2", "--sam", "all")):
        d, out = run("bad%d" % len(os.listdir(tmp_path)), *extra, ok=False)
        assert "--sam" in out.stderr and sorted(os.listdir(d)) == ["params.cfg", "reads.fa", "ref.fa"]
