"""Crafted candidates, the sampler and the model's expectations for the path run (gact_hip_candidates_paths), shared by the
CPU and GPU suites.

crafted() builds read pairs whose alignment is known in advance and whose CIGARs hit the edges path_ops_kernel and the
chain walk have: runs that start in the first and the last lanes of a 64-column step, paths of whole steps, paths of one
op, empty paths, hits at position 0 and at a read's end, left extensions that align nothing, reads shorter than a tile, a
read against itself, reads with N and lower case, and all of it on both strands.  sample() draws an unsorted selection
of both strands from a workload's candidates.  expected() is what the GPU must give for a selection: tests/path_model.py
on the oracle's AlignWithBT, computed once per session and configuration.  assert_equals_model() is the comparison every
exact test makes."""
from collections import namedtuple

import numpy as np

from gact_amd import engine, synth
from path_model import check_path, gact_path

LINEAR, AFFINE = (1, -1, -1, -1), (2, -3, -5, -2)
RECORD_FIELDS = ("ab", "ae", "bb", "be", "score", "first_tile_score", "n_tiles")
FAMILIES = ("identical", "mismatch700", "six1000", "gaps", "inside", "edge", "unrelated", "self", "raw")

# names[k]: "family/detail" of candidate k of np.concatenate([cf, cr]); reads: one set for ref and query (rs.rc(i) is the
# reverse-complement strand's query i)
Crafted = namedtuple("Crafted", "rs cf cr names")

_SWAP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _SWAP[_a] = _b


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rs = synth.ReadSet()
        self.fwd, self.rev = [], []                # (ref_id, query_id, ref_pos, query_pos, name)

    def rnd(self, n):
        return np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, n)].copy()

    def read(self, seq):
        self.rs.reads.append(np.ascontiguousarray(seq, dtype=np.uint8))
        self.rs.names.append("C%d" % len(self.rs.reads))
        return len(self.rs.reads) - 1

    def pair(self, name, ref, query, hits, rc_hits=()):
        """ref against query at every hit on the forward strand; at every rc_hit against a read whose reverse
        complement is query"""
        r = self.read(ref)
        q = self.read(query)
        for rp, qp in hits:
            self.fwd.append((r, q, rp, qp, "%s/%d,%d" % (name, rp, qp)))
        if len(rc_hits):
            c = self.read(synth.revcomp(query))
            for rp, qp in rc_hits:
                self.rev.append((r, c, rp, qp, "%s/%d,%d/rc" % (name, rp, qp)))
        return r, q


def _mutate(seq, positions):
    out = seq.copy()
    out[list(positions)] = _SWAP[out[list(positions)]]
    return out


def _lower(seq, a, b):
    seq[a:b] = np.frombuffer(bytes(seq[a:b]).lower(), np.uint8)


MISMATCH_AT = tuple(range(58, 72)) + tuple(range(122, 134)) + (0, 1, 698, 699)
SIX = (63, 64, 127, 128, 129, 500)

_CRAFTED = {}


def crafted(raw=True):
    """-> Crafted.  raw=False: the same reads and candidates without the N and lower-case stretches of the "raw" family,
    so that the whole set stays on the 2-bit kernels (one read with another byte routes a run to the raw-byte ones)"""
    if raw in _CRAFTED:
        return _CRAFTED[raw]
    b = _Builder(20261016)
    for L in (34, 35, 36, 63, 64, 65, 128, 320, 321, 640):
        s = b.rnd(L)
        hits = [(0, 0), (L // 2, L // 2), (L, L)]
        b.pair("identical/L%d" % L, s, s.copy(), hits, hits)
    s = b.rnd(700)
    for p in MISMATCH_AT:
        b.pair("mismatch700/p%d" % p, s, _mutate(s, [p]), [(350, 350)], [(350, 350)] if p in (0, 63, 64, 699) else ())
    base = b.rnd(1000)
    hits = [(400, 400), (0, 0), (1, 1), (999, 999), (1000, 1000)]
    b.pair("six1000", base, _mutate(base, SIX), hits, hits)
    gapped = np.concatenate([base[:300], base[310:700], b.rnd(5), base[700:]])       # a 10-base deletion, a 5-base insertion
    b.pair("gaps", base, gapped, [(500, 490)], [(500, 490)])
    long_ = b.rnd(3000)
    short = long_[1000:1100].copy()
    b.pair("inside/short-query", long_, short, [(1050, 50)], [(1050, 50)])
    b.pair("inside/short-ref", short, long_, [(50, 1050)], [(50, 1050)])
    g = b.rnd(2000)
    left, right = g[:1500], g[500:]                                # left[500:] == right[:1000]
    hits = [(500, 0), (1500, 1000), (1000, 500)]                   # query_pos 0; the ref's end only; the middle
    b.pair("edge/query-at-0", left, right, hits, hits)
    hits = [(0, 500), (1000, 1500), (500, 1000)]                   # ref_pos 0; the query's end only; the middle
    b.pair("edge/ref-at-0", right, left, hits, hits)
    b.pair("unrelated", b.rnd(2000), b.rnd(2000), [(1000, 1000), (0, 0), (2000, 2000)], [(1000, 1000)])
    s = b.read(b.rnd(500))
    for p in (0, 250, 500):
        b.fwd.append((s, s, p, p, "self/%d,%d" % (p, p)))
    half = b.rnd(250)
    s = b.read(np.concatenate([half, synth.revcomp(half)]))        # its own reverse complement
    for p in (0, 250, 500):
        b.rev.append((s, s, p, p, "self/%d,%d/rc" % (p, p)))
    # ---- three of the above with N and lower case: N == N is '=', an upper-case base against its lower-case one is 'X'
    ref, query = base.copy(), _mutate(base, SIX)
    if raw:
        ref[200:240] = ord("N")
        query[200:240] = ord("N")
        query[300:305] = ord("N")
        _lower(ref, 700, 760)
        _lower(query, 700, 760)
        _lower(ref, 800, 820)
    hits = [(400, 400), (0, 0), (1000, 1000)]
    b.pair("raw/six1000", ref, query, hits, hits)
    ref, query = base.copy(), gapped.copy()
    if raw:
        ref[100:120] = ord("N")
        query[100:120] = ord("N")
        _lower(query, 600, 650)
    b.pair("raw/gaps", ref, query, [(500, 490)], [(500, 490)])
    s = b.rnd(640)
    if raw:
        _lower(s, 100, 200)
        s[300:310] = ord("N")
    hits = [(0, 0), (320, 320), (640, 640)]
    b.pair("raw/identical640", s, s.copy(), hits, hits)
    cf = np.array([c[:4] for c in b.fwd], dtype=engine.CAND_DTYPE)
    cr = np.array([c[:4] for c in b.rev], dtype=engine.CAND_DTYPE)
    _CRAFTED[raw] = Crafted(b.rs, cf, cr, [c[4] for c in b.fwd + b.rev])
    return _CRAFTED[raw]


def n_and_lower_case(rs, seed=5):
    """a copy of a read set with 40 N in every third read and 500 lower-case bases in every fourth"""
    out = synth.ReadSet()
    rng = np.random.default_rng(seed)
    for k, r in enumerate(rs.reads):
        r = r.copy()
        if k % 3 == 0:
            r[rng.integers(0, len(r), 40)] = ord("N")
        if k % 4 == 1:
            a = int(rng.integers(0, max(1, len(r) - 500)))
            _lower(r, a, a + 500)
        out.reads.append(r)
        out.names.append(rs.names[k])
    return out


def sample(n_f, n_r, want, seed):
    """`want` distinct indices into the n_f forward candidates followed by the n_r reverse-complement ones, half from each
    strand where both have enough, in a shuffled order (int32)"""
    rng = np.random.default_rng(seed)
    want = min(want, n_f + n_r)
    take_r = min(want // 2, n_r)
    take_f = min(want - take_r, n_f)
    take_r = min(want - take_f, n_r)
    sel = np.sort(np.concatenate([rng.choice(n_f, take_f, replace=False), n_f + rng.choice(n_r, take_r, replace=False)]))
    return rng.permutation(sel).astype(np.int32)


def reads_of(rs, cands, nf, idx):
    """(ref, query) of candidate idx: the query on the strand the index says"""
    c = cands[idx]
    return rs.reads[int(c["ref_id"])], rs.rc(int(c["query_id"])) if idx >= nf else rs.reads[int(c["query_id"])]


_EXPECTED = {}


def expected(oracle, rs, cands, nf, sel=None, tile_size=320, tile_overlap=120, threshold=35, scoring=LINEAR, align=None):
    """the model's answer for every selected candidate, in the selection's order: a list of dicts with cigar, n_columns,
    n_ops, RECORD_FIELDS and left_aligned.  Kept for the session (the model takes about 0.05 s per 10 kb candidate); align:
    another AlignWithBT than the oracle's (not kept)"""
    sel = np.arange(len(cands)) if sel is None else np.asarray(sel)
    key = (id(rs), cands[sel].tobytes(), (sel >= nf).tobytes(), tile_size, tile_overlap, threshold, tuple(scoring))
    if align is None and key in _EXPECTED:
        return _EXPECTED[key][1]
    out = []
    for idx in sel.tolist():
        ref, query = reads_of(rs, cands, nf, idx)
        m = gact_path(align or oracle.align_with_bt, ref, query, int(cands[idx]["ref_pos"]), int(cands[idx]["query_pos"]),
                      tile_size=tile_size, tile_overlap=tile_overlap, threshold=threshold, scoring=tuple(scoring))
        e = {f: m[f] for f in RECORD_FIELDS}
        e.update(cigar=engine.cigar_string(m["ops"]), n_columns=len(m["cols"]), n_ops=len(m["ops"]),
                 left_aligned=m["left_aligned"])
        out.append(e)
    if align is None:
        _EXPECTED[key] = (rs, out)                 # (rs: its id stays its own for as long as the entry lives)
    return out


def ops_of(paths, ops, k):
    return ops[paths[k]["op_offset"]:paths[k]["op_offset"] + paths[k]["n_ops"]]


def assert_equals_model(exp, rs, cands, nf, sel, normal, records, paths, ops, scoring, names=None):
    """the exact comparison: records byte-equal to the normal run's, then per candidate the CIGAR string, n_columns, n_ops
    and the record's RECORD_FIELDS equal to the model's, and check_path with the model's left_aligned"""
    sel = np.arange(len(cands)) if sel is None else np.asarray(sel)
    assert len(exp) == len(sel) == len(records) == len(paths)
    assert records.tobytes() == normal[sel].tobytes(), "path records differ from the normal run's"
    assert int(paths["n_ops"].sum()) == len(ops)
    for k, idx in enumerate(sel.tolist()):
        who = (k, idx, names[idx] if names else None)
        e, p = exp[k], paths[k]
        mine = ops_of(paths, ops, k)
        got = engine.cigar_string(mine)
        assert got == e["cigar"], (who, got[:120], e["cigar"][:120])
        assert (int(p["n_columns"]), int(p["n_ops"])) == (e["n_columns"], e["n_ops"]), who
        for f in RECORD_FIELDS:
            assert int(records[k][f]) == e[f], (who, f, int(records[k][f]), e[f])
        ref, query = reads_of(rs, cands, nf, idx)
        check_path(records[k], mine, int(p["n_columns"]), ref, query, scoring, left_aligned=e["left_aligned"])


def engine_with(rs, cf, cr, slots=(0,), **kw):
    """an engine with rs as ref, query and reverse-complement query, and the candidates on every slot of `slots`:
    -> (engine, n, n_forward)"""
    eng = engine.Engine(**kw)
    cat, offs = rs.concat()
    rcat, _ = rs.concat(rc=True)
    eng.upload(engine.SET_REF, cat, offs)
    eng.upload(engine.SET_QUERY, cat, offs)
    eng.upload(engine.SET_QUERY_RC, rcat, offs)
    cands = np.concatenate([cf, cr]).astype(engine.CAND_DTYPE)
    for slot in slots:
        eng.candidates_upload(cands, slot=slot)
    return eng, len(cands), len(cf)
