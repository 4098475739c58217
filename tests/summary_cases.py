"""Cases and helpers for the summary run (gact_hip_candidates_summaries), shared by the CPU and GPU suites.

The summary walk counts a run where it starts and carries the last op from tile to tile of a phase and across the junction
of the left and the right part, so the candidates that can catch it out are those whose alignment has a run cut by a tile
boundary, the same / another op on the two sides of the junction, an empty left part, or no columns at all.  edges() says
which of these a model alignment (path_model.gact_path) has.  The crafted candidates of tests/path_cases.py reach all of
them at linear scoring but no cut gap run at the affine one (tests/test_summaries_model.py has the counts); additions()
closes that gap with periodic 12-base gaps: at tile 64 / 24 a walk stops after 40 ref or query steps, so its stopping
points drift across the gaps.  combined() is the one list the GPU suite runs: crafted + additions."""
import re
from collections import namedtuple

import numpy as np

from gact_amd import engine, synth
import path_cases
from path_cases import Crafted, _Builder

PERIOD, GAP = 53, 12
EDGES = ("gap_cut", "junction_same", "junction_diff", "left_empty", "no_columns")

_ADDITIONS = []


def additions():
    """-> Crafted: a 1,000-base read against a copy with a 12-base deletion every 53 bases, and against a copy with a 12-base
    insertion every 53 bases; hits in the middle and at both ends, both strands"""
    if _ADDITIONS:
        return _ADDITIONS[0]
    b = _Builder(20261017)
    base = b.rnd(1000)
    blocks = [base[a:a + PERIOD] for a in range(0, len(base), PERIOD)]
    deleted = np.concatenate([blk[:PERIOD - GAP] if len(blk) == PERIOD else blk for blk in blocks])
    inserted = np.concatenate([np.concatenate([blk, b.rnd(GAP)]) if len(blk) == PERIOD else blk for blk in blocks])
    mid = 9 * PERIOD                                                    # a block's first base: the same base in all three
    hits = [(mid, mid - 9 * GAP), (0, 0), (len(base), len(deleted))]
    b.pair("periodic/deletions", base, deleted, hits, hits)
    hits = [(mid, mid + 9 * GAP), (0, 0), (len(base), len(inserted))]
    b.pair("periodic/insertions", base, inserted, hits, hits)
    cf = np.array([c[:4] for c in b.fwd], dtype=engine.CAND_DTYPE)
    cr = np.array([c[:4] for c in b.rev], dtype=engine.CAND_DTYPE)
    _ADDITIONS.append(Crafted(b.rs, cf, cr, [c[4] for c in b.fwd + b.rev]))
    return _ADDITIONS[0]


# origin[k]: ("crafted" | "additions", index into that set's np.concatenate([cf, cr])) of candidate k of this set's
Combined = namedtuple("Combined", "rs cf cr names origin")

_COMBINED = {}


def combined(raw):
    """path_cases.crafted(raw) and additions() as one read set and one candidate list (forward ones first)"""
    if raw in _COMBINED:
        return _COMBINED[raw]
    a, b = path_cases.crafted(raw), additions()
    rs = synth.ReadSet()
    rs.reads = list(a.rs.reads) + list(b.rs.reads)
    rs.names = list(a.rs.names) + ["A%d" % k for k in range(len(b.rs.reads))]
    shift = len(a.rs.reads)

    def moved(c):
        c = c.copy()
        c["ref_id"] += shift
        c["query_id"] += shift
        return c

    cf = np.concatenate([a.cf, moved(b.cf)])
    cr = np.concatenate([a.cr, moved(b.cr)])
    naf, nbf = len(a.cf), len(b.cf)
    names = a.names[:naf] + b.names[:nbf] + a.names[naf:] + b.names[nbf:]
    origin = ([("crafted", k) for k in range(naf)] + [("additions", k) for k in range(nbf)] +
              [("crafted", naf + k) for k in range(len(a.cr))] + [("additions", nbf + k) for k in range(len(b.cr))])
    _COMBINED[raw] = Combined(rs, cf, cr, names, origin)
    return _COMBINED[raw]


_OPS = {"I": engine.OP_I, "D": engine.OP_D, "=": engine.OP_EQ, "X": engine.OP_X}


def ops_of_cigar(cigar):
    return np.array([(int(n) << 4) | _OPS[o] for n, o in re.findall(r"(\d+)([=XID])", cigar)], dtype=np.uint32)


_MODELS = {}


def additions_models(oracle, tile_size, tile_overlap, scoring, threshold=35):
    """path_model.gact_path of every candidate of additions(), kept for the session"""
    from path_model import gact_path
    key = (tile_size, tile_overlap, tuple(scoring), threshold)
    if key not in _MODELS:
        ad = additions()
        cands, nf = np.concatenate([ad.cf, ad.cr]), len(ad.cf)
        out = []
        for idx in range(len(cands)):
            ref, query = path_cases.reads_of(ad.rs, cands, nf, idx)
            out.append(gact_path(oracle.align_with_bt, ref, query, int(cands[idx]["ref_pos"]), int(cands[idx]["query_pos"]),
                                 tile_size=tile_size, tile_overlap=tile_overlap, threshold=threshold, scoring=tuple(scoring)))
        _MODELS[key] = out
    return _MODELS[key]


def model_summaries(oracle, raw, tile_size, tile_overlap, scoring):
    """the model's summary of every candidate of combined(raw): path_cases.expected for the crafted ones, gact_path for the
    additions -> SUMMARY_DTYPE array"""
    cr, cb = path_cases.crafted(raw), combined(raw)
    exp = path_cases.expected(oracle, cr.rs, np.concatenate([cr.cf, cr.cr]), len(cr.cf), tile_size=tile_size,
                              tile_overlap=tile_overlap, scoring=scoring)
    add = additions_models(oracle, tile_size, tile_overlap, scoring)
    out = np.zeros(len(cb.origin), dtype=engine.SUMMARY_DTYPE)
    for k, (where, idx) in enumerate(cb.origin):
        out[k] = engine.summarise(ops_of_cigar(exp[idx]["cigar"]) if where == "crafted" else add[idx]["ops"])
    return out


def edges(m):
    """which of EDGES the model alignment m (path_model.gact_path) has -> dict of bools.  A tile's columns are its n_states
    (tiles[t][9]); the left phase's tiles come first and emit right to left."""
    cols = m["cols"]
    lt = [t[9] for t in m["tiles"] if t[4] == 0]
    rt = [t[9] for t in m["tiles"] if t[4] == 1]
    nl, nr = sum(lt), sum(rt)
    assert nl + nr == len(cols)
    left, right = cols[:nl][::-1], cols[nl:]                            # both in emission order
    out = dict.fromkeys(EDGES, False)
    out["no_columns"] = not cols
    for part, per_tile in ((left, lt), (right, rt)):
        at = 0
        for n in per_tile[:-1]:
            at += n
            if 0 < at < len(part) and part[at - 1] == part[at] and part[at] in (engine.OP_I, engine.OP_D):
                out["gap_cut"] = True
    if nl and nr:
        out["junction_same" if left[0] == right[0] else "junction_diff"] = True
    out["left_empty"] = bool(not nl and nr)
    return out


def assert_summaries(sums, records, normal, paths, ops, model, names, sel=None):
    """the comparison every GPU test makes: records byte-equal to the normal run's; sums[k] == summarise(candidate k's ops of
    the path run) field by field, run sum == n_ops and column sum == n_columns; and, where a model is given, == model[k]"""
    sel = np.arange(len(sums)) if sel is None else np.asarray(sel)
    assert len(sums) == len(records) == len(paths) == len(sel)
    assert records.tobytes() == normal[sel].tobytes(), "summary records differ from the normal run's"
    for k, idx in enumerate(sel.tolist()):
        who = (k, idx, names[idx] if names else None)
        want = engine.summarise(path_cases.ops_of(paths, ops, k))
        for f in engine.SUMMARY_DTYPE.names:
            assert int(sums[k][f]) == int(want[f]), (who, f, sums[k], want)
        assert sum(int(sums[k][f]) for f in ("eq_runs", "x_runs", "ins_runs", "del_runs")) == int(paths[k]["n_ops"]), who
        assert sum(int(sums[k][f]) for f in ("n_eq", "n_x", "ins_bases", "del_bases")) == int(paths[k]["n_columns"]), who
        if model is not None:
            assert sums[k].tobytes() == model[k].tobytes(), (who, sums[k], model[k])
