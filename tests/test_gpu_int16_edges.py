"""GPU parity at the edges of the packed int16 kernels' scoring guards (tests/scoring_edges.py): at the last scoring each
guard admits, every layout that can take it runs the adversarial read sets and must match the oracle field by field,
having run the kernel it is meant to test and pushed the first tiles' scores to match * tile; one step past each guard
the engine must take the fallback the table names and stay bit-exact."""
import pytest

from scoring_edges import EDGES, edge_reads, threshold
from test_gpu_chain import _compare

pytestmark = pytest.mark.gpu

_SWITCHES = ("GACT_HIP_FORCE_INT32", "GACT_HIP_FORCE_UNIFORM", "GACT_HIP_FORCE_INT32_SEED", "GACT_HIP_FORCE_WIDE",
             "GACT_HIP_NO_WIDE", "GACT_HIP_NO_TAGGED", "GACT_HIP_NO_LIN", "GACT_HIP_NO_AFF", "GACT_HIP_COOP")
LAYOUTS = {
    "split": {"GACT_HIP_NO_WIDE": "1"},
    "wide": {"GACT_HIP_FORCE_WIDE": "1"},
    "coop": {"GACT_HIP_NO_WIDE": "1", "GACT_HIP_COOP": "1"},
    "uniform": {"GACT_HIP_NO_WIDE": "1", "GACT_HIP_FORCE_UNIFORM": "1"},
    "no-aff": {"GACT_HIP_NO_WIDE": "1", "GACT_HIP_NO_AFF": "1"},
    "plain": {"GACT_HIP_NO_WIDE": "1", "GACT_HIP_NO_TAGGED": "1"},
    "int32-seed": {"GACT_HIP_NO_WIDE": "1", "GACT_HIP_FORCE_INT32_SEED": "1"},
}


def _kind(main):
    """the int16 main kernel family a plan names"""
    return ("int32" if main == "-" else "lin" if "Lin" in main else "aff" if "Aff" in main else
            "tag" if ("<tag" in main or "Tagged" in main) else "plain")


def _layouts(edge):
    """every layout that can take the edge's last admitted scoring"""
    kind = _kind(edge.at_last.split)
    plain = ["plain"] if kind != "plain" else []
    if edge.at_last.split.startswith("Uniform"):           # the geometry allows no split layout
        return ["split", "int32-seed"] + (["wide"] if edge.tile <= 320 else []) + plain
    return (["split", "wide", "uniform", "int32-seed"] + (["coop"] if kind == "lin" else []) +
            (["no-aff"] if kind == "aff" else []) + plain)


def _expected_stats(edge, layout):
    kind = "plain" if layout == "plain" else _kind(edge.at_last.split)
    geo_uniform = edge.at_last.split.startswith("Uniform")
    uniform = geo_uniform or layout == "uniform"
    return {"packed16": True,
            "layout": "packed16-wide" if layout == "wide" else "packed16-uniform" if uniform else "packed16-split",
            "seed_layout": "packed16" if edge.at_last.seed.startswith("seed_p16") and layout != "int32-seed" else "int32",
            "tagged_pointers": kind in ("lin", "aff", "tag"),
            "linear_gap": kind == "lin" and not uniform,
            "affine_drift": kind == "aff" and layout in ("split", "int32-seed"),
            "coop_walks": layout == "coop"}


def _past_stats(edge):
    main, kind = edge.at_past.split, _kind(edge.at_past.split)
    if kind == "int32":
        return {"packed16": False, "layout": "int32"}
    return {"packed16": True, "layout": "packed16-uniform" if main.startswith("Uniform") else "packed16-split",
            "seed_layout": "packed16" if edge.at_past.seed.startswith("seed_p16") else "int32",
            "tagged_pointers": kind in ("lin", "aff", "tag"), "linear_gap": kind == "lin", "affine_drift": kind == "aff",
            "coop_walks": False}


_READS, _WANT = {}, {}


def _reads(edge):
    key = (edge.tile, edge.overlap)
    if key not in _READS:
        er = edge_reads(edge.tile, edge.overlap)
        er.cat, er.offs = er.rs.concat()
        er.rcat, er.roffs = er.rs.concat(rc=True)
        _READS[key] = er
    return _READS[key]


def _runs(er):
    """(name, complement, candidates, query set): both strands, clean and raw-byte lists"""
    return (("clean_f", False, er.clean_f, er.cat, er.offs), ("clean_r", True, er.clean_r, er.rcat, er.roffs),
            ("raw_f", False, er.raw_f, er.cat, er.offs), ("raw_r", True, er.raw_r, er.rcat, er.roffs))


def _want(oracle, edge, scoring, er, name, comp, cands, qcat, qoffs, same_file):
    """the oracle's records; with same_file False only a chain of a read with itself can differ (its emit flag), so the
    oracle reruns those alone"""
    key = (edge.tile, edge.overlap, scoring, name, same_file)
    if key not in _WANT:
        kw = dict(complement=comp, tile_size=edge.tile, tile_overlap=edge.overlap, threshold=threshold(edge, scoring),
                  scoring=scoring, n_threads=16)
        if same_file:
            _WANT[key] = oracle.gact_many(er.cat, er.offs, qcat, qoffs, cands, same_file=True, **kw)[0]
        else:
            w = _want(oracle, edge, scoring, er, name, comp, cands, qcat, qoffs, True).copy()
            self_ = cands["ref_id"] == cands["query_id"]
            w[self_] = oracle.gact_many(er.cat, er.offs, qcat, qoffs, cands[self_], same_file=False, **kw)[0]
            _WANT[key] = w
    return _WANT[key]


def _engine(monkeypatch, edge, scoring, env, er):
    from gact_amd import engine
    for var in _SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    eng = engine.Engine(tile_size=edge.tile, tile_overlap=edge.overlap, scoring=scoring, threshold=threshold(edge, scoring))
    eng.upload(engine.SET_REF, er.cat, er.offs)
    eng.upload(engine.SET_QUERY, er.cat, er.offs)
    eng.upload(engine.SET_QUERY_RC, er.rcat, er.roffs)
    return eng


def _check_stats(st, want, tag):
    got = {k: st[k] for k in want}
    assert got == want, "%s: ran %s, expected %s" % (tag, got, want)


@pytest.mark.parametrize("edge,layout", [(e, lay) for e in EDGES for lay in _layouts(e)],
                         ids=["%s-%s" % (e.name, lay) for e in EDGES for lay in _layouts(e)])
def test_int16_edge_bit_exact(oracle, monkeypatch, edge, layout):
    er = _reads(edge)
    sc = edge.last
    eng = _engine(monkeypatch, edge, sc, LAYOUTS[layout], er)
    want_stats = _expected_stats(edge, layout)
    try:
        for name, comp, cands, qcat, qoffs in _runs(er):
            for same_file in ((True, False) if name.startswith("clean") else (True,)):
                tag = "%s %s %s same_file=%d" % (edge.name, layout, name, same_file)
                got = eng.extend(cands, complement=comp, same_file=same_file)
                st = eng.last_run_stats()
                want = _want(oracle, edge, sc, er, name, comp, cands, qcat, qoffs, same_file)
                _compare(got, want, tag)
                if name.startswith("clean"):
                    _check_stats(st, want_stats, tag)
                    # the data reached the edge: full-score first tiles, chains of several tiles
                    exact = er.exact_f if not comp else er.exact_r
                    assert exact.sum() >= 20
                    assert got["first_tile_score"][exact].max() >= 0.95 * sc[0] * edge.tile, tag
                    assert (got["n_tiles"][exact] >= 3).mean() >= 0.9, tag
                    emitted = got["emitted"].astype(bool)
                    assert 0.2 < emitted.mean() < 0.9, tag              # the threshold splits the first tiles
                else:
                    assert st["raw_candidates"] > 0 and st["packed16"], tag
    finally:
        eng.close()


@pytest.mark.parametrize("edge", EDGES, ids=[e.name for e in EDGES])
def test_int16_edge_one_step_past(oracle, monkeypatch, edge):
    er = _reads(edge)
    sc = edge.past
    eng = _engine(monkeypatch, edge, sc, LAYOUTS["split"], er)
    try:
        for name, comp, cands, qcat, qoffs in _runs(er)[:2]:
            tag = "%s past %s" % (edge.name, name)
            got = eng.extend(cands, complement=comp, same_file=True)
            _check_stats(eng.last_run_stats(), _past_stats(edge), tag)
            _compare(got, _want(oracle, edge, sc, er, name, comp, cands, qcat, qoffs, True), tag)
            exact = er.exact_f if not comp else er.exact_r
            assert got["first_tile_score"][exact].max() >= 0.95 * sc[0] * edge.tile, tag
    finally:
        eng.close()
