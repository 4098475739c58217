"""CPU suite for the selection of overlaps (gact_hip_select_overlaps): the model of tests/select_model.py on hand-written
cases, what its crafted record sets hold -- the condition that keeps tests/test_gpu_select.py from passing vacuously -- the
new struct as a C compiler sees it, the library's exports, and the driver's refusals of --unique, which touch no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import select_model
from select_model import crafted, records_of, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(rows):
    rec = records_of(rows)
    return select(rec, "exact").tolist(), select(rec, "pair").tolist()


#        ref query comp   ab    ae   bb    be  score emitted
def test_a_score_tie_is_broken_by_span():
    rows = [(1, 2, 0, 100, 1100, 50, 1050, 900, 1),      # 0  span 2000
            (1, 2, 0, 100, 1300, 50, 1250, 900, 1),      # 1  span 2400: the same score, longer
            (1, 2, 0, 100, 9000, 50, 9000, 899, 1),      # 2  much longer, one point less
            (1, 2, 1, 100, 1100, 50, 1050, 10, 1)]       # 3  the other strand: a pair of its own
    exact, pair = _both(rows)
    assert exact == [0, 1, 2, 3]
    assert pair == [1, 3]


def test_a_span_tie_is_broken_by_index():
    rows = [(5, 9, 0, 0, 500, 0, 480, 300, 1),           # 0  span 980, score 300
            (5, 9, 0, 10, 700, 0, 510, 400, 1),          # 1  span 1200, score 400
            (5, 9, 0, 0, 600, 20, 620, 400, 1),          # 2  span 1200 made differently, score 400: ties with 1
            (5, 9, 0, 10, 700, 0, 510, 400, 1),          # 3  a copy of 1
            (9, 5, 0, 10, 700, 0, 510, 400, 1)]          # 4  (b, a) is not (a, b)
    exact, pair = _both(rows)
    assert exact == [0, 1, 2, 4]
    assert pair == [1, 4]


def test_a_record_that_was_not_emitted_is_never_selected_whatever_its_score():
    rows = [(4, 6, 0, 0, 100, 0, 100, 5000, 0),          # 0  the best score of its pair, not emitted
            (4, 6, 0, 0, 90, 0, 90, 80, 1),              # 1
            (4, 6, 0, 0, 100, 0, 100, 5000, 0),          # 2  a copy of 0
            (4, 6, 0, 0, 95, 0, 95, 85, 1),              # 3  the best emitted one
            (8, 6, 0, 0, 95, 0, 95, 85, 0),              # 4  alone in its pair, not emitted: the pair has no survivor
            (4, 6, 0, 0, 90, 0, 90, 80, 1)]              # 5  a copy of 1
    exact, pair = _both(rows)
    assert exact == [1, 3]
    assert pair == [3]
    assert _both([]) == ([], [])
    assert _both([(0, 0, 0, 0, 0, 0, 0, 0, 0)]) == ([], [])
    assert _both([(0, 0, 0, 0, 0, 0, 0, -7, 1)]) == ([0], [0])


def test_the_span_is_not_computed_in_32_bits():
    big = 2 ** 31 - 1
    rows = [(1, 1, 0, 0, big, 0, big, 10, 1),            # span 2^32 - 2: wraps to -2 in an int32
            (1, 1, 0, 0, 5, 0, 5, 10, 1)]
    assert _both(rows) == ([0, 1], [0])


@pytest.mark.parametrize("pattern", select_model.PATTERNS)
def test_crafted_sets_pair_selection_is_a_subset_of_the_exact_one(pattern):
    for n in select_model.SIZES:
        rec = crafted(pattern, n)
        assert len(rec) == n and crafted(pattern, n).tobytes() == rec.tobytes()        # seeded
        exact, pair = select(rec, "exact"), select(rec, "pair")
        emitted = np.flatnonzero(rec["emitted"])
        assert set(pair.tolist()) <= set(exact.tolist()) <= set(emitted.tolist())
        assert np.all(np.diff(exact) > 0) and np.all(np.diff(pair) > 0)
        assert len(set(zip(*(rec[f][pair].tolist() for f in select_model.PAIR_FIELDS)))) == len(pair)
        assert len(set(zip(*(rec[f][exact].tolist() for f in select_model.EXACT_FIELDS)))) == len(exact)


def test_what_the_crafted_sets_hold():
    """each pattern is what its name says, at the size where the scan spans many blocks and ends in a partial wave"""
    n = 70001
    assert n in select_model.SIZES and n % 64 != 0 and n > 256 * 256
    sel = {p: (select(crafted(p, n), "exact"), select(crafted(p, n), "pair")) for p in select_model.PATTERNS}
    assert sel["one_line"][0].tolist() == sel["one_line"][1].tolist() == [0]
    one_pair = crafted("one_pair", n)
    assert len(sel["one_pair"][1]) == 1 and 20 < len(sel["one_pair"][0]) <= 5 * 4 * 3
    top = one_pair[one_pair["score"] == one_pair["score"].max()]
    assert len(top) > 1000 and sel["one_pair"][1][0] > 0                              # ties at the top; not simply index 0
    assert len(sel["distinct"][0]) == len(sel["distinct"][1]) == n
    high = crafted("high_bits", n)
    assert not ((high["ref_id"] | high["query_id"]) & 0xffff).any() and len(sel["high_bits"][1]) == (n + 1) // 2
    assert len(sel["high_bits"][0]) == n
    second = crafted("every_second", n)
    assert second["emitted"].sum() == (n + 1) // 2 and not (sel["every_second"][0] & 1).any()
    assert len(sel["every_second"][1]) == len(np.unique(second["ref_id"]))
    assert len(sel["none_emitted"][0]) == len(sel["none_emitted"][1]) == 0
    straddle = crafted("straddle", n)
    for b in (64, 256, 65536):
        assert len({tuple(straddle[f][k] for f in select_model.EXACT_FIELDS) for k in range(b - 2, b + 3)}) == 1
        assert b - 2 in sel["straddle"][0] and not set(range(b - 1, b + 3)) & set(sel["straddle"][0].tolist())
    assert len(sel["straddle"][0]) == n - 4 * (n // 64)
    ties = crafted("ties", n)
    assert len(sel["ties"][1]) == n // 7 and sel["ties"][1].tolist() == list(range(n // 7))
    assert len(np.unique(ties["score"])) == 1 and len(sel["ties"][0]) > n - n // 100
    assert 0 < len(sel["mixed"][1]) < len(sel["mixed"][0]) < crafted("mixed", n)["emitted"].sum() < n


def test_gact_select_stats_layout(tmp_path):
    from gact_amd import engine
    S = engine.SelectStats
    (tmp_path / "s.c").write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"gact_hip.h\"\n"
        "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %d %d\\n\", sizeof(gact_select_stats), offsetof(gact_select_stats, device_ms), "
        "offsetof(gact_select_stats, emitted), offsetof(gact_select_stats, selected), offsetof(gact_select_stats, table_slots), "
        "offsetof(gact_select_stats, scratch_bytes), GACT_SELECT_EXACT, GACT_SELECT_PAIR); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.c")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got[:6] == [ctypes.sizeof(S), S.device_ms.offset, S.emitted.offset, S.selected.offset, S.table_slots.offset,
                       S.scratch_bytes.offset] == [32, 0, 4, 8, 16, 24]
    assert got[6:] == [engine.SELECT_EXACT, engine.SELECT_PAIR] == [0, 1]


def test_the_library_exports_the_selection(hip_lib_path):
    from gact_amd import engine
    lib = ctypes.CDLL(hip_lib_path)
    for name in ("gact_hip_select_overlaps", "gact_hip_last_select_stats"):
        assert name in engine.EXPORTS
        getattr(lib, name)
    assert hasattr(engine.Engine, "select_overlaps") and hasattr(engine.Engine, "last_select_stats")


@pytest.mark.parametrize("args", [["--unique", "pair"], ["--unique", "pair", "--device-dsoft", "--shard", "0/2"],
                                  ["--device-dsoft", "--unique", "sometimes"], ["--device-dsoft", "--unique"]],
                         ids=["without-device-dsoft", "with-shard", "unknown-value", "no-value"])
def test_the_driver_refuses_unique_where_it_cannot_hold(tmp_path, args):
    """before any file is read and any device is opened: the FASTA files named here do not exist"""
    from gact_amd import engine
    out = subprocess.run([engine.driver_path(), "none.fasta", "none.fasta", "1"] + args, capture_output=True, text=True, cwd=tmp_path,
                         timeout=600)
    assert out.returncode not in (0, -6, -11) and out.returncode > 0, out.stdout + out.stderr
    assert "--unique" in out.stderr and "cannot open" not in out.stderr
    assert not list(tmp_path.iterdir())
