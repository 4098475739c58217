"""GPU suite for alignment summaries (gact_hip_candidates_summaries): sums[k] is what reducing candidate k's ops of
gact_hip_candidates_paths gives, field by field, and what the chain model gives (tests/path_model.py on the oracle's
AlignWithBT); its records equal the normal run's byte for byte.  The crafted candidates plus the additions of
tests/summary_cases.py (tests/test_summaries_model.py asserts which edges of the counting walk they reach), a shuffled
sample of both strands at three tile geometries (chain_kernel<20, CountSink> and <32, ...>), raw-byte reads, one block walking everything,
independence from the path budget, what a slot keeps, the refusals, and the driver's --paf.  No tolerance anywhere."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import path_cases
import summary_cases
from path_cases import AFFINE, LINEAR, engine_with, expected
from summary_cases import assert_summaries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = 200


def _small():
    from conftest import workload_block
    blk = workload_block("ecoli10x_small")
    cands = np.concatenate([blk.cf, blk.cr])
    nf = len(blk.cf)
    sel = path_cases.sample(nf, len(blk.cr), SAMPLE, seed=20261016)
    assert len(sel) >= 200 and (sel < nf).sum() >= 50 and (sel >= nf).sum() >= 50 and np.any(np.diff(sel) < 0)
    return blk, cands, nf, sel


def _normal(eng, n, nf, slot=0):
    eng.candidates_run_mixed(n, nf, slot=slot)
    return eng.candidates_fetch(n, slot=slot).copy()


def _model_of(exp):
    from gact_amd import engine
    out = np.zeros(len(exp), dtype=engine.SUMMARY_DTYPE)
    for k, e in enumerate(exp):
        out[k] = engine.summarise(summary_cases.ops_of_cigar(e["cigar"]))
    return out


@pytest.mark.parametrize("raw", [True, False], ids=["raw-bytes", "acgt"])
@pytest.mark.parametrize("scoring", [LINEAR, AFFINE], ids=["linear", "affine"])
@pytest.mark.parametrize("tile_size,tile_overlap", [(320, 120), (64, 24), (320, 125), (317, 119), (321, 121)])   # (planted_tiles.GEOMETRIES)
def test_crafted_candidates_and_additions_equal_the_paths_and_the_model(oracle, tile_size, tile_overlap, scoring, raw):
    cb = summary_cases.combined(raw)
    kw = dict(tile_size=tile_size, tile_overlap=tile_overlap, scoring=scoring)
    eng, n, nf = engine_with(cb.rs, cb.cf, cb.cr, **kw)
    normal = _normal(eng, n, nf)
    _, paths, ops = eng.candidates_paths(n=n, rc_from=nf)
    records, sums = eng.candidates_summaries(n=n, rc_from=nf)
    eng.close()
    model = summary_cases.model_summaries(oracle, raw, tile_size, tile_overlap, scoring)
    assert_summaries(sums, records, normal, paths, ops, model, cb.names)
    cols = sums["n_eq"] + sums["n_x"] + sums["ins_bases"] + sums["del_bases"]
    assert (cols == 0).sum() >= 5 and (cols > 0).sum() > n // 2
    assert all(sums[f][cols == 0].sum() == 0 for f in sums.dtype.names)


@pytest.mark.parametrize("tile_size,tile_overlap", [(320, 120), (512, 192), (64, 24)])
def test_a_shuffled_sample_of_both_strands_equals_the_paths_and_the_model(oracle, tile_size, tile_overlap):
    blk, cands, nf, sel = _small()
    kw = dict(tile_size=tile_size, tile_overlap=tile_overlap)
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, **kw)
    normal = _normal(eng, n, nf)
    _, paths, ops = eng.candidates_paths(sel=sel, rc_from=nf)
    records, sums = eng.candidates_summaries(sel=sel, rc_from=nf)
    st = eng.last_summaries_stats()
    eng.close()
    model = _model_of(expected(oracle, blk.rs, cands, nf, sel, **kw))
    assert_summaries(sums, records, normal, paths, ops, model, None, sel=sel)
    assert st["launches"] == 1 and st["device_ms"] > 0 and 0 < st["scratch_bytes"] <= 128 * len(sel) + 4096
    assert (sums["ins_runs"] > 0).sum() > len(sel) // 2 and (sums["del_runs"] > 0).sum() > len(sel) // 2


def test_reads_with_n_and_lower_case(oracle):
    """raw-byte comparison: N == N counts as '=', an upper-case base against its lower-case one as 'X'"""
    from conftest import workload_block
    blk = workload_block("tiny")
    rs = path_cases.n_and_lower_case(blk.rs)
    cands = np.concatenate([blk.cf, blk.cr])
    eng, n, nf = engine_with(rs, blk.cf, blk.cr)
    normal = _normal(eng, n, nf)
    _, paths, ops = eng.candidates_paths(n=n, rc_from=nf)
    records, sums = eng.candidates_summaries(n=n, rc_from=nf)
    eng.close()
    assert nf > 0 and n > nf
    assert_summaries(sums, records, normal, paths, ops, None, None)                    # every candidate against its ops,
    sel = path_cases.sample(nf, n - nf, 40, seed=11)                                    # a sample of both strands against the model
    picked = paths[sel].copy()
    picked["op_offset"] = np.cumsum(np.concatenate([[0], picked["n_ops"][:-1]]))
    picked_ops = np.concatenate([path_cases.ops_of(paths, ops, k) for k in sel.tolist()])
    assert_summaries(sums[sel], records[sel], normal, picked, picked_ops, _model_of(expected(oracle, rs, cands, nf, sel)), None, sel=sel)
    # N against N is '=', an upper-case base against its lower-case one 'X': both kinds of column are there
    assert sums["n_x"].sum() > 0 and sums["n_eq"].sum() > sums["n_x"].sum()


def test_one_block_walking_every_candidate_gives_what_the_default_grid_gives():
    """max_blocks = 1: every group pops many candidates one after another (the counters start again at each)"""
    blk, cands, nf, sel = _small()
    order = np.concatenate([np.sort(sel[sel < nf]), np.sort(sel[sel >= nf])])
    cf, cr = cands[order[order < nf]], cands[order[order >= nf]]
    mine = np.searchsorted(order, sel).astype(np.int32)
    got = {}
    for max_blocks in (0, 1):
        eng, n, n_f = engine_with(blk.rs, cf, cr, max_blocks=max_blocks)
        if max_blocks == 0:
            normal = _normal(eng, n, n_f)
            _, paths, ops = eng.candidates_paths(sel=mine, rc_from=n_f)
        got[max_blocks] = eng.candidates_summaries(sel=mine, rc_from=n_f)
        eng.close()
    for a, b in zip(got[0], got[1]):
        assert a.tobytes() == b.tobytes()
    assert_summaries(got[1][1], got[1][0], normal, paths, ops, None, None, sel=mine)


_BUDGET_CHILD = """
import json, os, sys
root, out = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests"), os.path.join(root, "darwin-gpu_amd"), root]
import numpy as np
from conftest import workload_block
from path_cases import engine_with
blk = workload_block("ecoli10x_small")
sel = np.load(os.path.join(out, "sel.npy"))
eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
eng.candidates_paths(sel=sel, rc_from=nf)
chunks = eng.last_paths_stats()["chunks"]
records, sums = eng.candidates_summaries(sel=sel, rc_from=nf)
st = eng.last_summaries_stats()
eng.close()
np.save(os.path.join(out, "records.npy"), records)
np.save(os.path.join(out, "sums.npy"), sums)
print(json.dumps(dict(chunks=chunks, launches=st["launches"], scratch_bytes=st["scratch_bytes"])))
"""


def test_summaries_do_not_depend_on_the_path_budget(tmp_path, monkeypatch):
    """GACT_HIP_PATH_BUDGET_MB=1 in a fresh child process: the paths call runs in several chunks, the summaries call in one
    launch with memory proportional to the selection, and gives what a run without the variable gives (here, in this process)"""
    from conftest import workload_block
    monkeypatch.delenv("GACT_HIP_PATH_BUDGET_MB", raising=False)
    blk = workload_block("ecoli10x_small")
    n_all = len(blk.cf) + len(blk.cr)
    sel = np.arange(0, n_all, 3, dtype=np.int32)[::-1].copy()          # (any order, both strands)
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    eng.candidates_paths(sel=sel, rc_from=nf)
    assert eng.last_paths_stats()["chunks"] == 1
    records, sums = eng.candidates_summaries(sel=sel, rc_from=nf)
    st = eng.last_summaries_stats()
    eng.close()
    assert (sel < nf).any() and (sel >= nf).any() and len(sel) > 100 and sums["n_eq"].sum() > 0
    assert st["launches"] == 1 and 0 < st["scratch_bytes"] <= 128 * len(sel) + 4096
    np.save(tmp_path / "sel.npy", sel)
    env = dict(os.environ, GACT_HIP_PATH_BUDGET_MB="1")
    out = subprocess.run([sys.executable, "-c", _BUDGET_CHILD, ROOT, str(tmp_path)], capture_output=True, text=True, env=env,
                         timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert child["chunks"] > 3                                           # the paths call took several chunks ...
    assert child["launches"] == 1 and 0 < child["scratch_bytes"] <= 128 * len(sel) + 4096
    assert np.load(tmp_path / "sums.npy").tobytes() == sums.tobytes()
    assert np.load(tmp_path / "records.npy").tobytes() == records.tobytes()


def _same_run_stats(a, b):
    """two readings of gact_hip_last_run_stats of one run.  Every field is equal; the three times are not stored but made
    from the run's HIP events by the runtime at every reading (hipEventElapsedTime, a float), and two readings of the same
    events have been seen two float32 ulps apart.  4 ulps (4 * 2^-23, relative) allows that rounding and nothing else:
    events recorded again by another launch would move a time of milliseconds by microseconds at the least, 10^-4 of it."""
    assert a.keys() == b.keys()
    for k in a:
        if k.endswith("_ms"):
            assert abs(a[k] - b[k]) <= 4 * 2.0 ** -23 * abs(a[k]), (k, a[k], b[k])
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def test_what_a_summaries_call_leaves_on_its_slot():
    from gact_amd import engine
    blk, cands, nf, sel = _small()
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, slots=(0, 1), n_slots=2)
    normal = _normal(eng, n, nf)
    run_stats = eng.last_run_stats()
    paths = eng.candidates_paths(sel=sel, rc_from=nf)
    paths_stats = eng.last_paths_stats()
    whole = eng.candidates_summaries(sel=sel, rc_from=nf)
    # the slot's records, run statistics and paths statistics are what they were
    assert eng.candidates_fetch(n).tobytes() == normal.tobytes()
    _same_run_stats(eng.last_run_stats(), run_stats)
    assert eng.last_paths_stats() == paths_stats
    # a second call with another selection is not influenced by the first (a shorter one: the longer one's summaries are
    # still on the device), nor the first one repeated by the second
    seven = eng.candidates_summaries(sel=sel[7:14], rc_from=nf)
    again = eng.candidates_summaries(sel=sel, rc_from=nf)
    assert seven[0].tobytes() == whole[0][7:14].tobytes() and seven[1].tobytes() == whole[1][7:14].tobytes()
    assert again[0].tobytes() == whole[0].tobytes() and again[1].tobytes() == whole[1].tobytes()
    # slot 1 leaves slot 0 alone
    stats0 = eng.last_summaries_stats(slot=0)
    with pytest.raises(engine.GactHipError, match="no summary run"):
        eng.last_summaries_stats(slot=1)
    other = eng.candidates_summaries(sel=sel[::-1].copy(), rc_from=nf, slot=1)
    assert other[1].tobytes() == whole[1][::-1].tobytes()
    assert eng.last_summaries_stats(slot=0) == stats0 and eng.last_paths_stats(slot=0) == paths_stats
    _same_run_stats(eng.last_run_stats(slot=0), run_stats)
    assert eng.candidates_fetch(n, slot=0).tobytes() == normal.tobytes()
    # a normal run and a path run after summaries calls (they share the slot's workspace)
    assert _normal(eng, n, nf).tobytes() == normal.tobytes()
    for a, b in zip(eng.candidates_paths(sel=sel, rc_from=nf), paths):
        assert a.tobytes() == b.tobytes()
    eng.close()
    assert_summaries(whole[1], whole[0], normal, paths[1], paths[2], None, None, sel=sel)


def test_nothing_selected_and_the_device_filters_own_list():
    from gact_amd import engine
    from conftest import workload_block
    blk = workload_block("tiny")
    eng, _, _ = engine_with(blk.rs, blk.cf[:0], blk.cr[:0], slots=())
    records, sums = eng.candidates_summaries(n=0)                   # (nothing asked for is no error, candidates or not)
    assert len(records) == len(sums) == 0
    assert eng.L.gact_hip_candidates_summaries(eng.h, 0, 0, None, 0, 1, None, None) == 0
    eng.dsoft_build()
    nf, nr, _ = eng.dsoft_query(0, len(blk.rs.reads))
    n = nf + nr
    assert nf > 0 and nr > 0
    records, sums = eng.candidates_summaries(n=n, rc_from=nf)         # (before any normal run: the list is copied back)
    normal = _normal(eng, n, nf)
    _, paths, ops = eng.candidates_paths(n=n, rc_from=nf)
    eng.close()
    assert_summaries(sums, records, normal, paths, ops, None, None)
    assert (sums["n_eq"] > 0).sum() > n // 4


def test_refusals():
    from gact_amd import engine
    from conftest import workload_block
    blk = workload_block("tiny")
    eng = engine.Engine()
    with pytest.raises(engine.GactHipError, match="no candidates"):
        eng.candidates_summaries(n=1)
    with pytest.raises(engine.GactHipError, match="no summary run"):
        eng.last_summaries_stats()
    eng.close()
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr)
    with pytest.raises(engine.GactHipError, match="outside"):
        eng.candidates_summaries(sel=[0, n], rc_from=nf)
    with pytest.raises(engine.GactHipError, match="outside"):
        eng.candidates_summaries(sel=[-1], rc_from=nf)
    records = np.zeros(n, dtype=engine.OVERLAP_DTYPE)
    sums = np.zeros(n, dtype=engine.SUMMARY_DTYPE)
    assert eng.L.gact_hip_candidates_summaries(eng.h, 0, n, None, nf, 1, None, sums.ctypes.data) == -1
    assert eng.L.gact_hip_candidates_summaries(eng.h, 0, n, None, nf, 1, records.ctypes.data, None) == -1
    assert b"bad arguments" in eng.L.gact_hip_last_error()
    assert eng.L.gact_hip_candidates_summaries(eng.h, 0, -1, None, nf, 1, records.ctypes.data, sums.ctypes.data) == -1
    assert not records.view(np.uint8).any() and not sums.view(np.uint8).any()
    eng.close()
    eng, n, nf = engine_with(blk.rs, blk.cf, blk.cr, tile_size=513, tile_overlap=120)
    with pytest.raises(engine.GactHipError, match="GACT_HIP_FAST_TILE"):
        eng.candidates_summaries(n=n, rc_from=nf)
    eng.close()


_OUT = re.compile(r"^ref_id: (\S+), query_id: (\S+), ab: (\d+), ae: (\d+), bb: (\d+), be: (\d+), score: (-?\d+), comp: (\d)"
                  r"(?:, cigar: ([0-9=XID]*))?$")


def test_driver_paf_lines(tmp_path):
    from gact_amd import engine, workload
    from conftest import workload_block
    rs = workload_block("tiny").rs
    rs.write_fasta(str(tmp_path / "reads.fasta"))
    (tmp_path / "params.cfg").write_text(workload.PARAMS_CFG)
    drv = engine.driver_path()
    lengths = {nm.split()[0]: len(r) for nm, r in zip(rs.names, rs.reads)}

    def run(d, *extra, dsoft=True, ok=True):
        d.mkdir()
        os.symlink(tmp_path / "reads.fasta", d / "reads.fasta")
        os.symlink(tmp_path / "params.cfg", d / "params.cfg")
        out = subprocess.run([drv, "reads.fasta", "reads.fasta", "2"] + (["--device-dsoft"] if dsoft else []) + list(extra),
                             capture_output=True, text=True, cwd=d, timeout=600)
        if not ok:
            return out
        assert out.returncode == 0, out.stdout + out.stderr
        return ([open(d / ("darwin.%d.out" % t)).read() for t in range(2)],
                [open(d / ("darwin.%d.paf" % t)).read() if os.path.exists(d / ("darwin.%d.paf" % t)) else None for t in range(2)])

    cigar_out, no_paf = run(tmp_path / "cigar", "--cigar")
    both_out, both_paf = run(tmp_path / "both", "--paf", "--cigar")
    plain_out, _ = run(tmp_path / "plain")
    alone_out, alone_paf = run(tmp_path / "alone", "--paf")
    assert no_paf == [None, None]
    assert both_out == cigar_out and alone_out == plain_out           # the .out files are what they are without --paf
    n_lines = n_minus = 0
    for out_text, paf_text, alone_text in zip(both_out, both_paf, alone_paf):
        with_cigar = [m for m in (_OUT.match(line) for line in out_text.splitlines()) if m.group(9)]
        assert all(_OUT.match(line) for line in out_text.splitlines())
        paf = paf_text.splitlines()
        assert len(paf) == len(with_cigar) and paf_text.endswith("\n")
        # --paf alone: the same lines without cg
        assert alone_text == "".join(re.sub(r"\tcg:Z:[0-9=XID]+$", "", line) + "\n" for line in paf)
        for m, line in zip(with_cigar, paf):
            ref_name, query_name, ab, ae, bb, be, score, comp, cigar = m.groups()
            ab, ae, bb, be = int(ab), int(ae), int(bb), int(be)
            f = line.split("\t")
            assert len(f) == 16 and f[11] == "255", line
            assert (f[0], f[5]) == (query_name, ref_name) and (int(f[1]), int(f[6])) == (lengths[query_name], lengths[ref_name])
            assert f[12] == "AS:i:" + score and f[15] == "cg:Z:" + cigar
            s = engine.summarise(summary_cases.ops_of_cigar(cigar))
            n_eq, n_x, ins, dele = int(s["n_eq"]), int(s["n_x"]), int(s["ins_bases"]), int(s["del_bases"])
            qstart, qend, tstart, tend, nmatch, block = (int(f[k]) for k in (2, 3, 7, 8, 9, 10))
            assert nmatch == n_eq and block == n_eq + n_x + ins + dele
            assert tend - tstart == n_eq + n_x + dele and qend - qstart == n_eq + n_x + ins
            assert f[13] == "NM:i:%d" % (n_x + ins + dele)
            assert f[14] == "de:f:%.4f" % (1 - n_eq / (n_eq + n_x + int(s["ins_runs"]) + int(s["del_runs"])))
            # the span rule against the .out line's coordinates
            assert tend == ae and ab <= tstart
            start, end = be - (qend - qstart), be
            assert bb <= start
            if comp == "1":
                assert f[4] == "-" and (qstart, qend) == (lengths[query_name] - end, lengths[query_name] - start)
                n_minus += 1
            else:
                assert f[4] == "+" and (qstart, qend) == (start, end)
            n_lines += 1
    assert n_lines > 10 and n_minus > 0 and n_lines > n_minus
    for extra, dsoft in ((["--paf"], False), (["--paf", "--rccl-gather", "id"], True)):
        out = run(tmp_path / ("refused%d" % dsoft), *extra, dsoft=dsoft, ok=False)
        assert out.returncode == 1 and "--paf" in out.stderr
