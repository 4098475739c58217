"""CPU suite for alignment paths (gact_hip_candidates_paths): the Python restatement of GACT's tile chain that keeps the
alignment (tests/path_model.py) is pinned against the oracle -- record and tile sequence -- and, on small cases, against the
reference's own AlignWithBT; the CIGAR helpers of gact_amd.engine; the gact_path layout as a C compiler sees it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

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
