"""CPU suite for alignment paths (gact_hip_candidates_paths): the Python restatement of GACT's tile chain that keeps the
alignment (tests/path_model.py) is pinned against the oracle -- record and tile sequence -- and, on small cases, against the
reference's own AlignWithBT; the crafted candidates of tests/path_cases.py reach, on the model, the edges the GPU suite
counts on them to reach; the CIGAR helpers of gact_amd.engine; the gact_path layout as a C compiler sees it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import path_cases
from path_model import columns_to_ops, gact_path, check_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_FIELDS = ("ref_off", "query_off", "ref_len", "query_len", "reverse", "first", "tile_score", "max_i", "max_j",
                "n_states", "i_steps", "j_steps")


def _cases(n, seed, **kw):
    from gact_amd import synth
    rs = synth.simulate_reads(60_000, coverage=4, seed=seed, mean_len=2500, sd_len=800, min_len=300, max_len=5000)
    cf, cr = synth.synth_candidates(rs, seed=seed + 1, min_overlap=200)
    out = []
    for comp, cands in ((False, cf), (True, cr)):
        for c in cands[: n // 2]:
            q = rs.rc(int(c["query_id"])) if comp else rs.reads[int(c["query_id"])]
            out.append((rs.reads[int(c["ref_id"])], q, int(c["ref_pos"]), int(c["query_pos"])))
    return out


@pytest.mark.parametrize("tile_size,tile_overlap,scoring", [(320, 120, (1, -1, -1, -1)), (64, 16, (2, -3, -5, -2))])
def test_model_matches_the_oracle_record_and_tile_sequence(oracle, tile_size, tile_overlap, scoring):
    cases = _cases(300, seed=17 if tile_size == 320 else 23)
    assert len(cases) >= 200
    with_cols = 0
    for ref, query, rp, qp in cases:
        m = gact_path(oracle.align_with_bt, ref, query, rp, qp, tile_size=tile_size, tile_overlap=tile_overlap,
                      scoring=scoring)
        ov, traces = oracle.gact(bytes(ref), bytes(query), rp, qp, tile_size=tile_size, tile_overlap=tile_overlap,
                                 scoring=scoring, trace_cap=4096)
        for f in ("ab", "ae", "bb", "be", "score", "first_tile_score", "n_tiles"):
            assert m[f] == getattr(ov, f), (f, m[f], getattr(ov, f), rp, qp)
        assert m["tiles"] == [tuple(getattr(t, f) for f in TRACE_FIELDS) for t in traces]
        rec = {f: m[f] for f in ("ab", "ae", "bb", "be", "score")}
        check_path(rec, m["ops"], len(m["cols"]), np.frombuffer(bytes(ref), np.uint8), np.frombuffer(bytes(query), np.uint8),
                   scoring, left_aligned=m["left_aligned"])
        with_cols += len(m["cols"]) > 0
    assert with_cols > len(cases) // 2


def test_model_on_the_references_own_alignwithbt(reflib, oracle):
    """a handful of small chains: the model driven by the reference's AlignWithBT gives the oracle-driven CIGAR"""
    from gact_amd import engine
    for ref, query, rp, qp in _cases(12, seed=31)[:6]:
        ref, query = bytes(ref[:1200]), bytes(query[:1200])
        rp, qp = min(rp, len(ref)), min(qp, len(query))
        a = gact_path(oracle.align_with_bt, ref, query, rp, qp, tile_size=128, tile_overlap=32)
        b = gact_path(reflib.align_with_bt, ref, query, rp, qp, tile_size=128, tile_overlap=32)
        assert engine.cigar_string(a["ops"]) == engine.cigar_string(b["ops"])
        assert (a["ab"], a["ae"], a["bb"], a["be"], a["score"]) == (b["ab"], b["ae"], b["bb"], b["be"], b["score"])


@pytest.mark.parametrize("scoring", [path_cases.LINEAR, path_cases.AFFINE])
def test_crafted_cases_reach_the_edges_they_are_made_for(oracle, scoring):
    """asserted on the model's output at tile 320 / 120, so that a change of the helper or the simulator cannot quietly
    empty tests/test_gpu_paths_exact.py: path_ops_kernel works in steps of 64 columns and carries the open run between them"""
    cr = path_cases.crafted()
    cands, nf = np.concatenate([cr.cf, cr.cr]), len(cr.cf)
    assert len(cr.names) == len(cands) == len(set(cr.names))
    exp = path_cases.expected(oracle, cr.rs, cands, nf, scoring=scoring)
    starts = set()
    for e in exp:
        lens = [int(n) for n in re.findall(r"(\d+)[=XID]", e["cigar"])]
        assert sum(lens) == e["n_columns"] and len(lens) == e["n_ops"]
        starts |= {int(c) % 64 for c in np.cumsum(lens)[:-1]}          # (every run but a path's first, which starts at 0)
    assert {0, 1, 62, 63} <= starts
    assert any(e["n_columns"] > 0 and e["n_columns"] % 64 == 0 for e in exp)
    assert any(e["n_ops"] == 1 and e["n_columns"] > 128 for e in exp)
    assert sum(e["n_columns"] == 0 for e in exp) >= 5
    assert all(e["n_ops"] == 0 and e["score"] == 0 for e in exp if e["n_columns"] == 0)
    assert sum(e["n_columns"] > 0 and not e["left_aligned"] for e in exp) >= 5
    for op in "IDX":
        assert any(op in e["cigar"] for e in exp), op
    for strand, names in (("forward", cr.names[:nf]), ("reverse-complement", cr.names[nf:])):
        assert {nm.split("/")[0] for nm in names} == set(path_cases.FAMILIES), strand
    # the two read sets differ in the raw family's stretches only, and only one of them has a byte outside ACGT
    plain = path_cases.crafted(raw=False)
    assert plain.names == cr.names and np.array_equal(plain.cf, cr.cf) and np.array_equal(plain.cr, cr.cr)
    assert all(set(bytes(r)) <= set(b"ACGT") for r in plain.rs.reads)
    assert any(b"N" in bytes(r) for r in cr.rs.reads) and any(bytes(r) != bytes(r).upper() for r in cr.rs.reads)
    # a read against itself, on both strands
    assert sum(c["ref_id"] == c["query_id"] for c in cr.cf) >= 1 and sum(c["ref_id"] == c["query_id"] for c in cr.cr) >= 1


def test_sample_draws_both_strands_unsorted_and_is_fixed_by_its_seed():
    sel = path_cases.sample(1000, 700, 200, seed=3)
    assert sel.dtype == np.int32 and len(sel) == len(set(sel.tolist())) == 200
    assert (sel < 1000).sum() == (sel >= 1000).sum() == 100 and sel.max() < 1700
    assert np.any(np.diff(sel) < 0) and np.array_equal(sel, path_cases.sample(1000, 700, 200, seed=3))
    assert not np.array_equal(sel, path_cases.sample(1000, 700, 200, seed=4))
    assert (path_cases.sample(1000, 30, 200, seed=3) >= 1000).sum() == 30          # a short strand gives all it has
    assert sorted(path_cases.sample(5, 3, 200, seed=3).tolist()) == list(range(8))


@pytest.mark.parametrize("scoring", [path_cases.LINEAR, path_cases.AFFINE])
def test_crafted_cases_on_the_references_own_alignwithbt(reflib, oracle, scoring):
    """every crafted pair of reads of at most 1,000 bases, at tile 128 / 32: the model driven by the reference's AlignWithBT
    gives the oracle-driven CIGAR and record"""
    cr = path_cases.crafted()
    cands, nf = np.concatenate([cr.cf, cr.cr]), len(cr.cf)
    small = np.array([k for k in range(len(cands))
                      if max(len(r) for r in path_cases.reads_of(cr.rs, cands, nf, k)) <= 1000], dtype=np.int32)
    assert len(small) > 100 and {cr.names[k].split("/")[0] for k in small} >= set(path_cases.FAMILIES) - {"inside", "edge", "unrelated"}
    kw = dict(tile_size=128, tile_overlap=32, scoring=scoring)
    a = path_cases.expected(oracle, cr.rs, cands, nf, small, **kw)
    b = path_cases.expected(oracle, cr.rs, cands, nf, small, align=reflib.align_with_bt, **kw)
    for k, x, y in zip(small.tolist(), a, b):
        assert x == y, (cr.names[k], x, y)


def test_cigar_string_and_rescore():
    from gact_amd import engine
    E, X, I, D = engine.OP_EQ, engine.OP_X, engine.OP_I, engine.OP_D
    ops = columns_to_ops([E] * 153 + [X] + [I, I] + [E] * 4 + [D] * 3 + [E])
    assert engine.cigar_string(ops) == "153=1X2I4=3D1="
    assert engine.rescore(ops, (1, -1, -1, -1)) == 153 - 1 - 2 + 4 - 3 + 1
    assert engine.rescore(ops, (2, -3, -5, -2)) == 306 - 3 + (-5 - 2) + 8 + (-5 - 2 - 2) + 2
    # one `open` flag for both gap kinds (gact.cpp:198-205): an I run right behind a D run goes on with the gap
    ops = columns_to_ops([E, E, D, D, I, E])
    assert engine.cigar_string(ops) == "2=2D1I1="
    assert engine.rescore(ops, (2, -3, -5, -2)) == 4 + (-5 - 2) + (-2) + 2
    # a gap at the very start is opened
    assert engine.rescore(columns_to_ops([I, E]), (1, -1, -4, -1)) == -4 + 1
    assert engine.cigar_string([]) == "" and engine.rescore([], (1, -1, -1, -1)) == 0


def test_gact_paths_stats_layout(tmp_path):
    from gact_amd import engine
    S = engine.PathsStats
    (tmp_path / "s.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\n"
        "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu\\n\", sizeof(gact_paths_stats), offsetof(gact_paths_stats, device_ms), "
        "offsetof(gact_paths_stats, chunks), offsetof(gact_paths_stats, column_bytes), offsetof(gact_paths_stats, columns), "
        "offsetof(gact_paths_stats, ops)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got == [ctypes.sizeof(S), S.device_ms.offset, S.chunks.offset, S.column_bytes.offset, S.columns.offset, S.ops.offset]


def test_gact_path_layout(tmp_path):
    from gact_amd import engine
    assert engine.PATH_DTYPE.itemsize == 16
    (tmp_path / "p.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\n"
        "int main(void) { printf(\"%zu %zu %zu %zu %d %d %d %d\\n\", sizeof(gact_path), offsetof(gact_path, op_offset), "
        "offsetof(gact_path, n_ops), offsetof(gact_path, n_columns), GACT_PATH_OP_I, GACT_PATH_OP_D, GACT_PATH_OP_EQ, "
        "GACT_PATH_OP_X); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "p"), str(tmp_path / "p.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "p")]).split()]
    f = engine.PATH_DTYPE.fields
    assert got == [engine.PATH_DTYPE.itemsize, f["op_offset"][1], f["n_ops"][1], f["n_columns"][1],
                   engine.OP_I, engine.OP_D, engine.OP_EQ, engine.OP_X]
