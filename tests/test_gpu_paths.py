"""GPU suite for alignment paths (gact_hip_candidates_paths): the CIGAR of every candidate of a small workload equals the
model's (tests/path_model.py, on the oracle's AlignWithBT); on larger sets, every candidate's path is consistent with its
record and its two reads, and its record equals the normal run's byte for byte; chunking, the ops_cap retry, the refusals,
and the driver's --cigar lines.  tests/test_gpu_paths_exact.py compares with the model at every other configuration."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import path_cases
from path_model import check_path, gact_path

pytestmark = pytest.mark.gpu


def _engine_with(rs, cf, cr, **kw):
    from gact_amd import engine
    eng = engine.Engine(**kw)
    cat, offs = rs.concat()
    rcat, _ = rs.concat(rc=True)
    eng.upload(engine.SET_REF, cat, offs)
    eng.upload(engine.SET_QUERY, cat, offs)
    eng.upload(engine.SET_QUERY_RC, rcat, offs)
    cands = np.concatenate([cf, cr]).astype(engine.CAND_DTYPE)
    eng.candidates_upload(cands)
    return eng, len(cands), len(cf)


def _normal_and_paths(eng, n, nf, sel=None):
    eng.candidates_run_mixed(n, nf)
    normal = eng.candidates_fetch(n).copy()
    records, paths, ops = eng.candidates_paths(sel=sel, n=None if sel is not None else n, rc_from=nf)
    return normal, records, paths, ops


def _check_all(rs, cands, nf, normal, records, paths, ops, scoring, sel=None, left_aligned=None):
    """left_aligned: per selected candidate, from the model where one is at hand: whether the path must span the record"""
    sel = np.arange(len(cands)) if sel is None else np.asarray(sel)
    assert records.tobytes() == normal[sel].tobytes(), "path records differ from the normal run's"
    exact = 0
    for k, idx in enumerate(sel.tolist()):
        c = cands[idx]
        q = rs.rc(int(c["query_id"])) if idx >= nf else rs.reads[int(c["query_id"])]
        p = paths[k]
        mine = ops[p["op_offset"]:p["op_offset"] + p["n_ops"]]
        exact += check_path(records[k], mine, int(p["n_columns"]), rs.reads[int(c["ref_id"])], q, scoring,
                            left_aligned=None if left_aligned is None else left_aligned[k])
    if left_aligned is None:
        assert exact >= len(sel) // 2              # (most paths span [ab, ae) exactly; see check_path)
    else:
        assert exact >= sum(bool(x) for x in left_aligned)
    assert paths["n_columns"].sum() > 0


def test_paths_equal_the_model_on_tiny(oracle):
    from gact_amd import engine
    from conftest import workload_block
    blk = workload_block("tiny")
    eng, n, nf = _engine_with(blk.rs, blk.cf, blk.cr)
    cands = np.concatenate([blk.cf, blk.cr])
    normal, records, paths, ops = _normal_and_paths(eng, n, nf)
    eng.close()
    assert nf > 0 and n > nf
    models = []
    for k in range(n):
        c = cands[k]
        q = blk.rs.rc(int(c["query_id"])) if k >= nf else blk.rs.reads[int(c["query_id"])]
        models.append(gact_path(oracle.align_with_bt, blk.rs.reads[int(c["ref_id"])], q, int(c["ref_pos"]), int(c["query_pos"])))
    _check_all(blk.rs, cands, nf, normal, records, paths, ops, (1, -1, -1, -1))
    _check_all(blk.rs, cands, nf, normal, records, paths, ops, (1, -1, -1, -1), left_aligned=[m["left_aligned"] for m in models])
    for k, m in enumerate(models):
        p = paths[k]
        got = engine.cigar_string(ops[p["op_offset"]:p["op_offset"] + p["n_ops"]])
        assert got == engine.cigar_string(m["ops"]), (k, got[:80], engine.cigar_string(m["ops"])[:80])
        assert p["n_columns"] == len(m["cols"])


@pytest.mark.parametrize("scoring", [(1, -1, -1, -1), (2, -3, -5, -2)])
@pytest.mark.parametrize("tile_size,tile_overlap", [(320, 120), (512, 192), (64, 24)])
def test_path_invariants_on_ecoli10x_small(scoring, tile_size, tile_overlap):
    from conftest import workload_block
    blk = workload_block("ecoli10x_small")
    eng, n, nf = _engine_with(blk.rs, blk.cf, blk.cr, tile_size=tile_size, tile_overlap=tile_overlap, scoring=scoring)
    normal, records, paths, ops = _normal_and_paths(eng, n, nf)
    eng.close()
    _check_all(blk.rs, np.concatenate([blk.cf, blk.cr]), nf, normal, records, paths, ops, scoring)


def test_path_invariants_with_n_and_lower_case_reads():
    """raw-byte sets: = / X by raw byte equality (case matters, N == N, align.cpp:134)"""
    from conftest import workload_block
    blk = workload_block("tiny")
    rs = path_cases.n_and_lower_case(blk.rs, seed=5)
    assert any(b"N" in bytes(r) for r in rs.reads) and any(bytes(r) != bytes(r).upper() for r in rs.reads)
    eng, n, nf = _engine_with(rs, blk.cf, blk.cr)
    normal, records, paths, ops = _normal_and_paths(eng, n, nf)
    eng.close()
    _check_all(rs, np.concatenate([blk.cf, blk.cr]), nf, normal, records, paths, ops, (1, -1, -1, -1))


def test_a_selection_of_many_chunks_equals_one_chunk(monkeypatch):
    from conftest import workload_block
    blk = workload_block("ecoli10x_small")
    n_all = len(blk.cf) + len(blk.cr)
    sel = np.arange(0, n_all, 3, dtype=np.int32)[::-1].copy()          # (any order, both strands)
    eng, n, nf = _engine_with(blk.rs, blk.cf, blk.cr)
    one = eng.candidates_paths(sel=sel, rc_from=nf)
    st_one = eng.last_paths_stats()
    eng.candidates_run_mixed(n, nf)
    normal = eng.candidates_fetch(n).copy()
    eng.close()
    assert (sel < nf).any() and (sel >= nf).any() and np.any(np.diff(sel) < 0)
    monkeypatch.setenv("GACT_HIP_PATH_BUDGET_MB", "1")                   # read at create: a fresh engine
    eng, n, nf = _engine_with(blk.rs, blk.cf, blk.cr)
    many = eng.candidates_paths(sel=sel, rc_from=nf)
    st_many = eng.last_paths_stats()
    eng.close()
    cands = np.concatenate([blk.cf, blk.cr])
    column_bytes = sum(len(blk.rs.reads[int(cands[k]["ref_id"])]) + len(blk.rs.reads[int(cands[k]["query_id"])]) for k in sel)
    assert st_one["chunks"] == 1 and st_one["column_bytes"] == column_bytes
    assert st_many["chunks"] >= column_bytes // (1 << 20) > 3 and st_many["column_bytes"] <= 1 << 20
    for st in (st_one, st_many):
        assert st["device_ms"] > 0 and st["ops"] == len(one[2]) and st["columns"] == int(one[1]["n_columns"].sum())
    for a, b in zip(one, many):
        assert a.tobytes() == b.tobytes()
    # the selection against the normal run and the reads: sel[k] on its own strand, in its own column buffer
    assert one[0].tobytes() == normal[sel].tobytes()
    _check_all(blk.rs, cands, nf, normal, *one, (1, -1, -1, -1), sel=sel)


def test_ops_cap_too_small_says_how_much_and_the_retry_succeeds():
    from gact_amd import engine
    from conftest import workload_block
    blk = workload_block("tiny")
    eng, n, nf = _engine_with(blk.rs, blk.cf, blk.cr)
    rec_a, paths_a, ops_a = eng.candidates_paths(n=n, rc_from=nf)
    records = np.zeros(n, dtype=engine.OVERLAP_DTYPE)
    paths = np.zeros(n, dtype=engine.PATH_DTYPE)
    needed = ctypes.c_int64()
    small = np.zeros(8, dtype=np.uint32)
    rc = eng.L.gact_hip_candidates_paths(eng.h, 0, n, None, nf, 1, records.ctypes.data, paths.ctypes.data, small.ctypes.data,
                                         len(small), ctypes.byref(needed))
    assert rc == -1 and needed.value == len(ops_a) > 8
    assert b"ops_cap" in eng.L.gact_hip_last_error()
    assert paths.tobytes() == paths_a.tobytes() and records.tobytes() == rec_a.tobytes()
    rc = eng.L.gact_hip_candidates_paths(eng.h, 0, n, None, nf, 1, records.ctypes.data, paths.ctypes.data, None, 0,
                                         ctypes.byref(needed))
    assert rc == -1 and needed.value == len(ops_a)
    room = np.zeros(needed.value, dtype=np.uint32)
    rc = eng.L.gact_hip_candidates_paths(eng.h, 0, n, None, nf, 1, records.ctypes.data, paths.ctypes.data, room.ctypes.data,
                                         len(room), ctypes.byref(needed))
    assert rc == 0 and np.array_equal(room, ops_a)
    eng.close()


def test_refusals():
    from gact_amd import engine
    from conftest import workload_block
    blk = workload_block("tiny")
    eng = engine.Engine()
    with pytest.raises(engine.GactHipError, match="no candidates"):
        eng.candidates_paths(n=1)
    records, paths, ops = eng.candidates_paths(n=0)          # (nothing asked for is no error, candidates or not)
    assert len(records) == len(paths) == len(ops) == 0
    with pytest.raises(engine.GactHipError, match="no path run"):
        eng.last_paths_stats()
    eng.close()
    eng, n, nf = _engine_with(blk.rs, blk.cf, blk.cr)
    with pytest.raises(engine.GactHipError, match="outside"):
        eng.candidates_paths(sel=[0, n], rc_from=nf)
    with pytest.raises(engine.GactHipError, match="outside"):
        eng.candidates_paths(sel=[-1], rc_from=nf)
    eng.close()
    eng, n, nf = _engine_with(blk.rs, blk.cf, blk.cr, tile_size=1024, tile_overlap=256)
    with pytest.raises(engine.GactHipError, match="GACT_HIP_FAST_TILE"):
        eng.candidates_paths(n=n, rc_from=nf)
    eng.close()


_LINE = re.compile(r"^ref_id: (\S+), query_id: (\S+), ab: (\d+), ae: (\d+), bb: (\d+), be: (\d+), score: (-?\d+), comp: (\d)$")


def test_driver_cigar_lines(tmp_path):
    from gact_amd import engine, synth, workload
    from conftest import workload_block
    rs = workload_block("tiny").rs
    rs.write_fasta(str(tmp_path / "reads.fasta"))
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()

    def run(d, *extra):
        d.mkdir()
        os.symlink(tmp_path / "reads.fasta", d / "reads.fasta")
        os.symlink(tmp_path / "params.cfg", d / "params.cfg")
        out = subprocess.run([drv, "reads.fasta", "reads.fasta", "2", "--device-dsoft"] + list(extra), capture_output=True,
                             text=True, cwd=d, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        return [open(d / ("darwin.%d.out" % t)).read() for t in range(2)]

    plain = run(tmp_path / "plain")
    cig = run(tmp_path / "cigar", "--cigar")
    names = {nm.split()[0]: k for k, nm in enumerate(rs.names)}
    n_lines = 0
    for a, b in zip(plain, cig):
        stripped = "".join(re.sub(r", cigar: [0-9=XID]*$", "", line) + "\n" for line in b.splitlines())
        assert stripped == a
        for line in b.splitlines():
            head, cigar = line.rsplit(", cigar: ", 1)
            m = _LINE.match(head)
            assert m, head
            ref_name, query_name, ab, ae, bb, be, score, comp = m.groups()
            rec = dict(ab=int(ab), ae=int(ae), bb=int(bb), be=int(be), score=int(score))
            ops = np.array([(int(x) << 4) | {"I": 1, "D": 2, "=": 7, "X": 8}[o] for x, o in re.findall(r"(\d+)([=XID])", cigar)],
                           dtype=np.uint32)
            assert engine.cigar_string(ops) == cigar
            qi = names[query_name]
            q = synth.revcomp(rs.reads[qi]) if comp == "1" else rs.reads[qi]
            check_path(rec, ops, int((ops >> 4).sum()), rs.reads[names[ref_name]], q, (1, -1, -1, -1))
            n_lines += 1
    assert n_lines > 0
    out = subprocess.run([drv, "reads.fasta", "reads.fasta", "1", "--cigar"], capture_output=True, text=True, cwd=tmp_path / "plain",
                         timeout=600)
    assert out.returncode != 0 and "--cigar" in out.stderr


def test_driver_cigar_with_feeders_that_have_no_reads_or_no_candidates(tmp_path):
    """more feeder threads than reads (empty read ranges) and a shard whose range is empty: --cigar writes what plain
    --device-dsoft writes, plus the CIGARs, and finishes"""
    from gact_amd import engine, synth, workload
    from conftest import workload_block
    full = workload_block("tiny").rs
    rs = synth.ReadSet()
    rs.reads, rs.names = full.reads[:10], full.names[:10]
    rs.write_fasta(str(tmp_path / "reads.fasta"))
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()
    for extra, files in ((["8"], ["darwin.%d.out" % t for t in range(8)]),
                         (["2", "--shard", "3/4"], ["darwin.3.%d.out" % t for t in range(2)])):
        got = {}
        for mode in ("plain", "cigar"):
            d = tmp_path / ("%s_%s" % (mode, "_".join(extra).replace("/", "-")))
            d.mkdir()
            os.symlink(tmp_path / "reads.fasta", d / "reads.fasta")
            os.symlink(tmp_path / "params.cfg", d / "params.cfg")
            args = [drv, "reads.fasta", "reads.fasta"] + extra + ["--device-dsoft"] + (["--cigar"] if mode == "cigar" else [])
            out = subprocess.run(args, capture_output=True, text=True, cwd=d, timeout=600)
            assert out.returncode == 0, out.stdout + out.stderr
            got[mode] = [open(d / f).read() for f in files]
        for a, b in zip(got["plain"], got["cigar"]):
            assert "".join(re.sub(r", cigar: [0-9=XID]*$", "", line) + "\n" for line in b.splitlines()) == a
            assert all(", cigar: " in line for line in b.splitlines())
