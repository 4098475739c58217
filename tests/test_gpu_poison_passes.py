"""GPU parity of the passes behind a run under poisoned scratch (GACT_HIP_POISON_SCRATCH=<seed>, gact_engine.hip::ScratchPoison).

Every pass keeps a device allocation between its calls and lays a ladder of regions over it whose offsets move with n, n_reads
and n_arcs.  A region that a call reads without having copied, zeroed or wholly written it -- the flag word of a wave whose lanes
are all past n, a block count behind nb, a table slot, the consensus byte of a read nothing aligned to -- normally holds what
an earlier, similar call left at nearly the same place, or a fresh allocation's zeros, and the read goes unnoticed.  With the
switch set the whole allocation (not this call's layout of it) is refilled with seeded garbage in front of the call's first
write, with other words at every fill, and such a read shows as a result that differs from the model's or changes with the seed.

Each test makes its own two-slot engine with the switch unset, set to one seed and set to another, and walks its pass in the
order that makes leftovers matter: the largest case first, then the smallest, some in between, the largest again, and the same
on slot 1.  Every result equals the model's exactly -- they are integers -- and so equals the other seeds'.  After every call
the fill counter (gact_hip_scratch_fills) has risen by at least the bytes the pass holds; unset, it stays at 0.  The inputs, the
models and the comparisons are the ones of the passes' own files."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = (None, 20261021, 0xC0FFEE)
seeded = pytest.mark.parametrize("seed", SEEDS, ids=["unset", "seed-a", "seed-b"])


class _Engine(object):
    """an engine made after the switch is set (or unset), and the fill counter's last reading"""

    def __init__(self, monkeypatch, seed, **kw):
        from gact_amd import engine
        monkeypatch.delenv("GACT_HIP_POISON_SCRATCH", raising=False)
        if seed is not None:
            monkeypatch.setenv("GACT_HIP_POISON_SCRATCH", str(seed))
        self.seed = seed
        make = kw.pop("make", None)             # (the switch is read when the engine is made)
        self.e = make() if make else engine.Engine(**dict(dict(n_slots=2, max_blocks=1), **kw))
        self.seen = self.e.scratch_fills()
        assert self.seen == (0, 0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()

    def filled(self, at_least, what, fills=1):
        """since the last reading: unset, nothing; set, at least `fills` fills over at least `at_least` bytes"""
        now = self.e.scratch_fills()
        if self.seed is None:
            assert now == (0, 0), what
        else:
            assert now[0] - self.seen[0] >= fills and now[1] - self.seen[1] >= at_least > 0, (what, self.seen, now, at_least)
        self.seen = now

    def filled_exactly(self, fills, nbytes, what):
        """since the last reading: unset, nothing; set, exactly that many fills over exactly that many bytes"""
        now = self.e.scratch_fills()
        if self.seed is None:
            assert now == (0, 0), what
        else:
            assert (now[0] - self.seen[0], now[1] - self.seen[1]) == (fills, nbytes), (what, self.seen, now, fills, nbytes)
        self.seen = now

    def quiet(self, what):
        """since the last reading: no fill at all"""
        assert self.e.scratch_fills() == self.seen, what


def _ladder(cases):
    """largest first, the smaller ones, the largest again; then the same on slot 1"""
    return [(slot, case) for slot in (0, 1) for case in list(cases) + [cases[0]]]


# ---- the passes over host records

@seeded
def test_select(monkeypatch, seed):
    import select_model
    from test_gpu_select import _model
    with _Engine(monkeypatch, seed) as p:
        for pattern in select_model.PATTERNS:
            for slot, n in _ladder([1000, 1, 257, 64, 65]):
                rec = select_model.crafted(pattern, n)
                for mode in select_model.MODES:
                    got = p.e.select_overlaps(records=rec, mode=mode, slot=slot)
                    assert got.dtype == np.int32 and got.tolist() == _model(pattern, n, mode).tolist(), (pattern, n, mode, slot, seed)
                    p.filled(p.e.last_select_stats(slot)["scratch_bytes"], (pattern, n, mode, slot))


@seeded
def test_filter(monkeypatch, seed):
    import filter_model as fm
    from test_gpu_filter import _device, _random, _same
    hand = fm.hand_cases()
    with _Engine(monkeypatch, seed) as p:
        # beyond one block of block counts first; sel names twice as many records in no order; then the wave and block edges
        sized = [(fm.BIG, True), (1, True), (257, False), (64, True), (65, False), (1025, True), (256, False)]
        for slot, (n, with_sel) in _ladder(sized):
            rec, sums, kw, want = _random(n, with_sel=with_sel)
            _same(_device(p.e, rec, sums, kw, slot=slot), want, sums, (n, with_sel, slot, seed))
            p.filled(p.e.last_filter_stats(slot)["scratch_bytes"], (n, with_sel, slot))
        for slot in (0, 1):
            for name in sorted(hand):
                rec, sums, kw, why, rows = hand[name]
                got = _device(p.e, rec, sums, kw, slot=slot)
                assert got["why"].tolist() == why, (name, seed)
                _same(got, fm.filter_overlaps(rec, sums, **kw), sums, (name, slot, seed))
                p.filled(p.e.last_filter_stats(slot)["scratch_bytes"], name)
            # every record on one table row, one side and both
            for kw1 in (dict(sides=fm.QUERY, n_reads=1), dict(sides=fm.REF, n_reads=40)):
                rec, sums, kw, want = _random(5000, one_read=True, **kw1)
                _same(_device(p.e, rec, sums, kw, slot=slot), want, sums, ("one read", kw1, slot, seed))
                p.filled(p.e.last_filter_stats(slot)["scratch_bytes"], "one read")


@seeded
def test_cover(monkeypatch, seed):
    from cover_model import QUERY, REF
    from test_gpu_cover import _case, _same, _same_depth
    cases = [("random", {}), ("empty", {}), ("lengths", {}), ("strand", dict(sides=REF)), ("strand", dict(sides=QUERY)),
             ("chunk_edges", {}), ("sums", {}), ("not_emitted_sel", {}), ("stack", {})]
    assert (_case("empty")[3]["n_intervals"] == 0).all()          # reads that no record names
    assert (_case("lengths")[3]["n_intervals"] == 0).any() and 0 in _case("lengths")[1].tolist()
    with _Engine(monkeypatch, seed) as p:
        for slot, (pattern, over) in _ladder(cases):
            rec, lens, kw, want, want_depth = _case(pattern, **over)
            for depth in (True, False):
                got = p.e.read_coverage(lens, records=rec, depth=depth, slot=slot, **kw)
                _same(got[0] if depth else got, want, (pattern, over, slot, seed))
                if depth:
                    _same_depth(got[1], want_depth, (pattern, over, slot, seed))
                p.filled(p.e.last_cover_stats(slot)["scratch_bytes"], (pattern, over, slot))


@seeded
def test_place(monkeypatch, seed):
    from test_gpu_place import _case, _equal
    with _Engine(monkeypatch, seed) as p:
        for slot, (pattern, m) in _ladder([("many_reads", None), ("chain", 66), ("random", 65), ("stack", 1000)]):
            rec, lens, kw, want = _case(pattern, m)
            _equal(p.e.place_reads(lens, records=rec, slot=slot, **kw), want, (pattern, m, slot, seed))
            p.filled(p.e.last_place_stats(slot)["scratch_bytes"], (pattern, m, slot))


@seeded
def test_graph(monkeypatch, seed):
    from test_gpu_graph import _case, _same, _same_counts
    cases = ["many_reads", "tiling", "contained", "sel", "sums", "clip", "blocks257", "empty", "tiling129", "random", "hub"]
    assert _case("contained")[3]["counts"]["contained"] > 0 and _case("random")[3]["counts"]["contained"] > 0
    assert "sel" in _case("sel")[2] and "sums" in _case("sums")[2]
    with _Engine(monkeypatch, seed) as p:
        for slot, pattern in _ladder(cases):
            rec, lens, kw, want = _case(pattern)
            _same(p.e.overlap_graph(lens, records=rec, classes=True, slot=slot, **kw), want, (pattern, slot, seed))
            _same_counts(p.e.last_graph_stats(slot), want, pattern)
            p.filled(p.e.last_graph_stats(slot)["scratch_bytes"], (pattern, slot))


# ---- the passes over an arc graph

def _all_flagged(g):
    """the graph with no arc of flags == 0"""
    arcs = g[2].copy()
    arcs["flags"] = 1
    return g[0], g[1], arcs, g[3]


@seeded
def test_unitigs(monkeypatch, seed):
    import test_gpu_unitigs as tu
    import unitig_model
    from gact_amd import engine
    flagged = _all_flagged(tu._graph_of("chain65"))             # (this file's own: not put into the other file's cache)
    flagged_want = unitig_model.unitigs(flagged[0], flagged[1], flagged[2], clip=flagged[3], tip_reads=3)
    assert (flagged[2]["flags"] != 0).all()
    # a chain over many blocks, no arcs at all, a cycle, a cut tip, skipped inputs, no arc left, the scan's first carry
    cases = [("random3000_1", 3), ("no_arcs", 3), ("cycle300", 0), ("fork", 3), ("skipped", 3), ("all_flagged", 3), ("tiling129", 0),
             ("chain1", 0), ("cycle_tip", 3), ("chain257", 0)]
    assert tu._case("cycle300", 0)[1]["counts"]["circular"] == 1 and tu._case("fork", 3)[1]["counts"]["cut"] == 2
    # ... and one with bases: reads of the random-graph kind with bytes of their own as GACT_SET_REF
    lens, reads, arcs, clip = unitig_model.random_graph(100, 7)
    rng = np.random.default_rng(20261023)
    seqs = [np.frombuffer(b"ACGTACGTACGTACGTacgtNn", dtype=np.uint8)[rng.integers(0, 22, int(ln))] for ln in lens]
    based = unitig_model.unitigs(lens, reads, arcs, clip=clip, tip_reads=3, seqs=seqs)
    assert len(based["seq"]) > 0
    with _Engine(monkeypatch, seed) as p:
        p.e.upload_seqs(engine.SET_REF, seqs)
        for slot, (name, tip_reads) in _ladder(cases):
            if name == "all_flagged":
                got = p.e.unitigs(flagged[0], flagged[1], flagged[2], clip=flagged[3], tip_reads=tip_reads, slot=slot)
                tu._same(got, flagged_want, (name, slot, seed))
                tu._same_counts(p.e.last_unitig_stats(slot), flagged_want, name, len(flagged[0]))
            else:
                tu._check(p.e, name, tip_reads, slot=slot)
            p.filled(p.e.last_unitig_stats(slot)["scratch_bytes"], (name, tip_reads, slot))
            if name in ("no_arcs", "chain257"):                 # the bases after a small graph and after a large one
                tu._same(p.e.unitigs(lens, reads, arcs, clip=clip, tip_reads=3, seq=True, slot=slot), based, ("bases", slot, seed))
                p.filled(p.e.last_unitig_stats(slot)["scratch_bytes"], ("bases", slot))


@seeded
def test_bubbles(monkeypatch, seed):
    import test_gpu_bubbles as tb
    cases = [("random3000_1", "tips", {}), ("no_arcs", None, {}), ("beads", None, {}), ("flagged", None, {}), ("simple", None, dict(max_vertices=3)),
             ("fan62", None, {}), ("dead", (tb.hand_made("dead")[4]["extra"][0] >> 1,), {}), ("nested_in", None, {}), ("cycle300", None, {}),
             ("random300_2", None, {}), ("fork", "tips", {}), ("random3000_1", None, {})]
    assert tb._case("flagged")[2]["counts"]["sources"] == 0 and tb._graph_of("fork")[4].any()
    with _Engine(monkeypatch, seed) as p:
        for slot, (name, skip, kw) in _ladder(cases):
            tb._check(p.e, name, skip=skip, slot=slot, **kw)
            p.filled(p.e.last_bubble_stats(slot)["scratch_bytes"], (name, skip, slot))


@seeded
def test_prune(monkeypatch, seed):
    import test_gpu_clean as tc
    cases = [("random3000_1", "tips", 900), ("no_arcs", "own", 500), ("fan129", "own", 500), ("flagged", "own", 500), ("skipped", "own", 500),
             ("single", "own", 500), ("fan64", "own", 500), ("fan65", None, 1000), ("repeat1000_1", "tips", 900), ("twice_cycle", None, 500),
             ("big_ov", "own", 1000), ("random3000_1", None, 300)]
    with _Engine(monkeypatch, seed) as p:
        for slot, (name, skip, ratio) in _ladder(cases):
            tc._check_prune(p.e, name, skip=skip, ratio=ratio, slot=slot)         # (with vertex_best and without: two calls)
            p.filled(2 * p.e.last_prune_stats(slot)["scratch_bytes"], (name, skip, ratio, slot), fills=2)


@seeded
def test_clean(monkeypatch, seed):
    import clean_model
    import test_gpu_clean as tc
    cases = [("repeat3000_1", {}), ("no_arcs", {}), ("false_fork", {}), ("flagged", {}), ("nested_in", dict(max_passes=1)), ("beads", {}),
             ("repeat300_1", dict(ratios=(0, 1000, 16))), ("twice_cycle", {}), ("skipped", {}), ("random3000_1", {}),
             ("threshold", dict(ratios=(600, 600, 3), max_passes=2, tip_reads=1, max_dist=3000, max_vertices=8))]
    kinds = set(tc._clean_case("repeat3000_1")[1]["steps"]["kind"].tolist())
    assert kinds >= {clean_model.PRUNE, clean_model.BUBBLES} and len(kinds) >= 3         # a plan with every kind of step
    with _Engine(monkeypatch, seed) as p:
        for slot, (name, kw) in _ladder(cases):
            tc._check_clean(p.e, name, slot=slot, **kw)
            p.filled(p.e.last_clean_stats(slot)["scratch_bytes"], (name, kw, slot))


# ---- the passes that walk the alignments again

CHUNKED = 130                    # candidates of ecoli10x_small (about 20 kB of columns each) that a budget of 1 MiB cuts into three chunks


class _PathBufs(object):
    """The sizes of a slot's path buffers (Slot::PathBufs), restated from the host code: a DevBuf grows to max(n, 1024) elements
    when a chunk needs more than it has and never shrinks; a chunk is as many candidates as the budget's column bytes hold, at
    least one (path_chunk_end); a chunk of n candidates and b column bytes needs n candidates, records, op offsets and op counts,
    n + 1 column offsets, 2 n column counts and b + 64 column bytes; a path run reserves per chunk, a pileup add reserves the
    largest chunk's before its first.  Under the switch every chunk fills all seven arrays over all of their elements, and a
    chunk that writes ops fills all of the ops' words: -> (fills, bytes) that a call must have added to the counter, exactly"""
    SIZES = dict(cands=16, records=56, col_off=8, op_off=8, n_cols=4, n_ops=4, cols=1, ops=4)
    SEVEN = ("cands", "records", "col_off", "op_off", "n_cols", "n_ops", "cols")

    def __init__(self, budget_mb=1024):
        self.budget = budget_mb << 20
        self.cap = dict.fromkeys(self.SIZES, 0)

    def _reserve(self, name, n):
        if n > self.cap[name]:
            self.cap[name] = max(n, 1024)

    def _reserve_chunk(self, n, nbytes):
        for name, want in (("cands", n), ("records", n), ("col_off", n + 1), ("op_off", n), ("n_cols", 2 * n), ("n_ops", n),
                           ("cols", nbytes + 64)):
            self._reserve(name, want)

    def chunks(self, col_caps):
        """[(first, end, column bytes)]"""
        out, first = [], 0
        while first < len(col_caps):
            end, nbytes = first, 0
            while end < len(col_caps) and (end == first or nbytes + col_caps[end] <= self.budget):
                nbytes += col_caps[end]
                end += 1
            out.append((first, end, nbytes))
            first = end
        return out

    def _seven(self):
        return sum(self.cap[name] * self.SIZES[name] for name in self.SEVEN)

    def paths(self, col_caps, n_ops=None):
        """gact_hip_candidates_paths; n_ops: the candidates' op counts where the call has room for the ops, else None"""
        fills = nbytes = 0
        for first, end, b in self.chunks(col_caps):
            self._reserve_chunk(end - first, b)
            fills, nbytes = fills + 7, nbytes + self._seven()
            chunk_ops = int(sum(n_ops[first:end])) if n_ops is not None else 0
            if chunk_ops > 0:
                self._reserve("ops", chunk_ops)
                fills, nbytes = fills + 1, nbytes + self.cap["ops"] * self.SIZES["ops"]
        return fills, nbytes

    def add(self, col_caps):
        """gact_hip_pileup_add of the candidates inside the window"""
        chunks = self.chunks(col_caps)
        if chunks:
            self._reserve_chunk(max(end - first for first, end, _ in chunks), max(b for _, _, b in chunks))
        return 7 * len(chunks), len(chunks) * self._seven()


def _col_caps(rs, cands, sel=None):
    """the column bytes a path run sets aside for each selected candidate: every column consumes a base of one of its two reads"""
    sel = range(len(cands)) if sel is None else sel
    return [len(rs.reads[int(cands[k]["ref_id"])]) + len(rs.reads[int(cands[k]["query_id"])]) for k in sel]


def _paths_ops_null_then_room(p, bufs, caps, sel, nf, slot):
    """gact_hip_candidates_paths with ops == NULL (refused once the counts are known, records and paths written), then with room;
    bufs: the slot's _PathBufs, caps: _col_caps of the selection.  Each call fills every chunk's arrays whole, and only those"""
    import ctypes
    from gact_amd import engine
    e = p.e
    records, paths = np.zeros(len(sel), dtype=engine.OVERLAP_DTYPE), np.zeros(len(sel), dtype=engine.PATH_DTYPE)
    needed = ctypes.c_int64(-1)
    rc = e.L.gact_hip_candidates_paths(e.h, slot, len(sel), sel.ctypes.data, nf, 1, records.ctypes.data, paths.ctypes.data, None, 0,
                                       ctypes.byref(needed))
    assert needed.value > 0 and rc == -1 and b"ops_cap" in e.L.gact_hip_last_error()
    assert e.last_paths_stats(slot)["chunks"] == len(bufs.chunks(caps))
    p.filled_exactly(*bufs.paths(caps), what=("ops == NULL", len(sel), slot))
    got = e.candidates_paths(sel=sel, rc_from=nf, slot=slot, ops_cap=needed.value)
    p.filled_exactly(*bufs.paths(caps, got[1]["n_ops"].tolist()), what=("with room", len(sel), slot))
    assert got[0].tobytes() == records.tobytes() and got[1].tobytes() == paths.tobytes() and len(got[2]) == needed.value
    return got


@seeded
def test_paths_and_summaries_in_chunks(oracle, monkeypatch, seed):
    """the sample of both strands of ecoli10x_small that test_gpu_paths_exact.py holds to the chain model, under a path budget
    that cuts it into several chunks: the second chunk's columns, counts and offsets lie where the first one's were"""
    import path_cases
    from test_gpu_paths_exact import _small
    from test_gpu_summaries import _model_of
    blk, cands, nf, sel = _small()
    exp = path_cases.expected(oracle, blk.rs, cands, nf, sel)[:CHUNKED]          # (kept for the session under the whole sample's key)
    sel = sel[:CHUNKED].copy()
    model = _model_of(exp)
    assert (sel < nf).any() and (sel >= nf).any()
    monkeypatch.setenv("GACT_HIP_PATH_BUDGET_MB", "1")
    n, nf = len(cands), len(blk.cf)
    with _Engine(monkeypatch, seed, make=lambda: path_cases.engine_with(blk.rs, blk.cf, blk.cr, slots=(0, 1), n_slots=2)[0]) as p:
        e = p.e
        caps = _col_caps(blk.rs, cands, sel.tolist())
        for slot in (0, 1):
            e.candidates_run_mixed(n, nf, slot=slot)
            normal = e.candidates_fetch(n, slot=slot).copy()
            p.quiet("a run fills nothing")
            whole, bufs = None, _PathBufs(budget_mb=1)
            for k in (len(sel), 1, 65, len(sel)):
                # (k = 1 and k = 65 behind the whole selection: their chunks fill the arrays the larger chunks left, about 1 MiB each)
                got = _paths_ops_null_then_room(p, bufs, caps[:k], sel[:k], nf, slot)
                st = e.last_paths_stats(slot)
                assert st["chunks"] == (3 if k == len(sel) else 2 if k == 65 else 1), (k, st)
                if whole is None:                   # every candidate against the chain model on the oracle
                    path_cases.assert_equals_model(exp, blk.rs, cands, nf, sel, normal, *got, path_cases.LINEAR)
                    whole = got
                # ... and its first k as a selection of their own, the whole selection again: the same bytes
                n_ops = int(whole[1]["n_ops"][:k].sum())
                assert got[0].tobytes() == whole[0][:k].tobytes() and got[1].tobytes() == whole[1][:k].tobytes(), (k, slot, seed)
                assert got[2].tobytes() == whole[2][:n_ops].tobytes(), (k, slot, seed)
                records, sums = e.candidates_summaries(sel=sel[:k], rc_from=nf, slot=slot)
                p.filled(e.last_summaries_stats(slot)["scratch_bytes"], ("summaries", k, slot))
                assert records.tobytes() == normal[sel[:k]].tobytes() and sums.tobytes() == model[:k].tobytes(), (k, slot, seed)
    monkeypatch.delenv("GACT_HIP_PATH_BUDGET_MB")


@seeded
def test_paths_and_summaries_of_the_crafted_candidates(oracle, monkeypatch, seed):
    """tests/path_cases.py's crafted candidates, both strands, raw bytes: in order, a reversed selection, one candidate"""
    import path_cases
    from test_gpu_summaries import _model_of
    from summary_cases import assert_summaries
    cr = path_cases.crafted(True)
    cands = np.concatenate([cr.cf, cr.cr])
    exp = path_cases.expected(oracle, cr.rs, cands, len(cr.cf))
    model = _model_of(exp)
    n, nf = len(cands), len(cr.cf)
    everything = np.arange(n, dtype=np.int32)
    with _Engine(monkeypatch, seed, make=lambda: path_cases.engine_with(cr.rs, cr.cf, cr.cr, slots=(0, 1), n_slots=2)[0]) as p:
        e = p.e
        for slot in (0, 1):
            e.candidates_run_mixed(n, nf, slot=slot)
            normal = e.candidates_fetch(n, slot=slot).copy()
            bufs = _PathBufs()
            for sel in (everything, everything[n - 1:], everything[::-1][:65].copy(), everything[::-1].copy(), everything):
                got = _paths_ops_null_then_room(p, bufs, _col_caps(cr.rs, cands, sel.tolist()), sel, nf, slot)
                want = [exp[k] for k in sel.tolist()]
                path_cases.assert_equals_model(want, cr.rs, cands, nf, sel, normal, *got, path_cases.LINEAR, names=cr.names)
                records, sums = e.candidates_summaries(sel=sel, rc_from=nf, slot=slot)
                p.filled(e.last_summaries_stats(slot)["scratch_bytes"], ("summaries", len(sel), slot))
                assert_summaries(sums, records, normal, got[1], got[2], model[sel], cr.names, sel=sel)


def _load(e, case, slot):
    """a planted case's reads as the three sets and its candidates (forward only) on `slot`"""
    from gact_amd import engine
    cat, offs = case.rs.concat()
    rcat, _ = case.rs.concat(rc=True)
    e.upload(engine.SET_REF, cat, offs)
    e.upload(engine.SET_QUERY, cat, offs)
    e.upload(engine.SET_QUERY_RC, rcat, offs)
    e.candidates_upload(case.cands.astype(engine.CAND_DTYPE), slot=slot)
    return len(case.cands)


_ACROSS_SEEDS = {}


def _same_as_the_other_seeds(key, *arrays):
    blob = [a if isinstance(a, bytes) else a.tobytes() for a in arrays]
    assert _ACROSS_SEEDS.setdefault(key, blob) == blob, key


class _VariantRoom(object):
    """The allocation of gact_hip_pileup_variants, restated from the host code: position bytes | chunk_at | totals | the
    sequences' table | records, each part 16-byte aligned; the records' room is what the allocation holds beyond the rest; a
    call that has room from the caller for more records than that grows the allocation to exactly those and counts again (the
    second reserve).  Every call fills the allocation in begin(), and the new one again when it has grown"""

    def __init__(self):
        self.bytes = 0

    def call(self, positions, n_seqs, cap, total):
        """one call of the C entry -> (fills, bytes filled, whether the second reserve ran)"""
        up16 = lambda v: (v + 15) & ~15
        chunks = -(-positions // 4096)
        at_rec = up16(up16(up16(positions) + (chunks + 1) * 8 + 40) + n_seqs * 32)
        room = (self.bytes - at_rec) // 32 if self.bytes > at_rec else 0
        self.bytes = max(self.bytes, at_rec + room * 32)
        fills, filled, regrown = 1, self.bytes, False
        if positions > 0 and cap >= total > room:
            self.bytes = at_rec + total * 32
            fills, filled, regrown = 2, filled + self.bytes, True
        return fills, filled, regrown

    def binding(self, positions, n_seqs, total):
        """Engine.pileup_variants: room for 1024 records, and once more with room for all where there are more"""
        fills, filled, regrown = self.call(positions, n_seqs, 1024, total)
        if total > 1024:
            more = self.call(positions, n_seqs, total, total)
            fills, filled, regrown = fills + more[0], filled + more[1], regrown or more[2]
        return fills, filled, regrown


_BLOCK_V_MODEL = {}


@seeded
def test_pileup_corrected_reads_and_variants(monkeypatch, seed):
    """the planted windows of tests/variant_cases.py on one engine: the largest, the one with a target nothing aligns to and a
    target of one base, the one with insertions, the largest again; a window of the one-base target alone behind each; counts,
    consensus and read table against pileup_model, slots and corrected reads against pileup_ins_model, the records against
    variant_model on the models' counts and against what was planted; then truth block V with thresholds that let every
    disagreement through: more records than the room the pass held, so the second reserve runs.  Every fill is accounted for:
    the window's in begin alone, the path buffers' whole per chunk of an add, the corrected reads' bytes, the variants' block"""
    import test_gpu_pileup as tp
    import test_gpu_pileup_ins as ti
    import variant_cases
    import variant_model
    import variant_truth
    from gact_amd import engine
    from test_gpu_variants import _same
    cases = variant_cases.cases()
    loose = dict(min_depth=1, min_alt=1, min_permille=0, hom_permille=1000)
    with _Engine(monkeypatch, seed, threshold=variant_cases.THRESHOLD, max_blocks=0) as p:
        e = p.e
        bufs, room, seq_cap = {0: _PathBufs(), 1: _PathBufs()}, _VariantRoom(), 0

        def variants(positions, n_seqs, what, **params):
            """a call of the binding, its fills and the pass's bytes as _VariantRoom says -> (records, table), regrown"""
            got = e.pileup_variants(table=True, **params)
            fills, filled, regrown = room.binding(positions, n_seqs, len(got[0]))
            p.filled_exactly(fills, filled, what + ("variants", str(params)))
            assert e.last_variant_stats()["scratch_bytes"] == room.bytes, what
            return got, regrown

        first_call = True
        for slot, name in _ladder(["runs-at-edges", "several", "ins"]):
            case = cases[name]
            n = _load(e, case, slot)
            caps = _col_caps(case.rs, case.cands)
            records, paths, ops = e.candidates_paths(n=n, rc_from=n, slot=slot)
            p.filled_exactly(*bufs[slot].paths(caps, paths["n_ops"].tolist()), what=(name, "paths"))
            K = case.ins_slots
            # (the whole case; then, where that is another window, its first target alone: a small window after a large one)
            for window in dict.fromkeys((tuple(case.window), (case.window[0], 1))):
                what = (name, window, slot, seed)
                e.pileup_begin(window[0], window[1], ins_slots=K)
                p.filled_exactly(1, e.last_pileup_stats()["scratch_bytes"], what + ("begin",))
                e.pileup_add(n=n, rc_from=n, slot=slot)
                st = e.last_pileup_stats()
                inside = [c for c, t in zip(caps, case.cands["ref_id"].tolist()) if window[0] <= t < window[0] + window[1]]
                assert st["chunks"] == 1 and st["alignments"] >= 1 and inside, what
                p.filled_exactly(*bufs[slot].add(inside), what=what + ("add",))
                want = {d: tp._model(case.rs, records, paths, ops, window=window, min_depth=d) for d in (1, 2)}
                for d in (1, 2):
                    got = e.pileup_finish(min_depth=d)
                    tp._same(got, want[d], what + (d,))
                p.quiet(what + ("finish fills nothing",))
                first = e.pileup_finish(min_depth=1)
                seqs = case.rs.reads[window[0]:window[0] + window[1]]
                own = np.concatenate([np.asarray(r) for r in seqs])
                offs = np.concatenate([[0], np.cumsum([len(r) for r in seqs])]).astype(np.int64)
                ins_model = ti._model(case.rs, records, paths, ops, K, window=window, min_depth=1)
                if K:
                    corrected = e.pileup_corrected(min_depth=1, ins=True)
                    ti._same(corrected, ins_model, what)
                    ins = ins_model[0]
                else:
                    reads, read_at, seq = e.pileup_corrected(min_depth=1)
                    assert reads.tobytes() == ins_model[1].tobytes() and np.array_equal(read_at, ins_model[2]) and seq == ins_model[3], what
                    corrected, ins = (reads, read_at, seq), None
                # the corrected reads' bytes: one allocation of the engine's that grows to the most bases spelled so far
                seq_cap = max(seq_cap, len(corrected[2]))
                p.filled_exactly(1 if corrected[2] else 0, seq_cap if corrected[2] else 0, what + ("corrected",))
                for params in (case.params, loose, case.params):
                    got, regrown = variants(len(own), window[1], what, **params)
                    _same(got, variant_model.variants(want[1][0], ins, own, offs, seq_first=window[0], **params), what + (str(params),))
                    if window == tuple(case.window) and params is case.params:
                        assert got[0].tolist() == case.want.tolist(), what
                    assert regrown == (first_call and len(got[0]) > 0), what      # (a fresh engine holds no room; later these few fit)
                    first_call = False
                    _same_as_the_other_seeds((name, window, slot, str(params)), *got)
                # the window is kept state: nothing since the adds has touched it
                for x, y in zip(first, e.pileup_finish(min_depth=1)):
                    assert x.tobytes() == y.tobytes(), what
                p.quiet(what + ("the window is not filled again",))
                _same_as_the_other_seeds((name, window, slot), *(first + tuple(corrected)))
        # truth block V: more than 4096 records under the loose thresholds, against the few hundred bytes of room held so far
        b = variant_truth.block_v()
        e.upload_seqs(engine.SET_REF, b["seqs"])
        e.upload_seqs(engine.SET_QUERY, b["reads"])
        e.upload_seqs(engine.SET_QUERY_RC, b["rc"])
        e.candidates_upload(b["cands"])
        n, nf, what = len(b["cands"]), b["nf"], ("block V", seed)
        e.pileup_begin(ins_slots=variant_truth.K)
        p.filled_exactly(1, e.last_pileup_stats()["scratch_bytes"], what + ("begin",))
        e.pileup_add(n=n, rc_from=nf, same_file=False)
        caps = [len(b["seqs"][int(c["ref_id"])]) + len(b["reads"][int(c["query_id"])]) for c in b["cands"]]
        p.filled_exactly(*bufs[0].add(caps), what=what + ("add",))
        own, offs = variant_truth.own_and_offsets()
        strict, regrown = variants(len(own), len(b["seqs"]), what, **variant_truth.PARAMS)
        held = e.last_variant_stats()["scratch_bytes"]
        many, regrown = variants(len(own), len(b["seqs"]), what, **loose)
        assert len(many[0]) > 4096 and regrown and e.last_variant_stats()["scratch_bytes"] > held + 32 * 4096, (len(many[0]), regrown, held)
        _, counts, _ = e.pileup_finish(min_depth=1)
        ins = e.pileup_corrected(min_depth=1, ins=True)[3]
        key = counts.tobytes() + ins.tobytes()
        if key not in _BLOCK_V_MODEL:
            _BLOCK_V_MODEL.clear()
            _BLOCK_V_MODEL[key] = [variant_model.variants(counts, ins, own, offs, **params) for params in (variant_truth.PARAMS, loose)]
        _same(strict, _BLOCK_V_MODEL[key][0], "block V")
        _same(many, _BLOCK_V_MODEL[key][1], "block V, every disagreement")
        _same_as_the_other_seeds("block V", counts, ins, *(strict + many))


# ---- the passes one behind the other

_CHAIN = {}


def _device_chain(e, n, nf, lens, fills=None):
    """run -> summaries -> filter -> select -> cover -> graph -> clean -> unitigs on slot 0, every pass on the sel / sums of the one
    before (the selection takes records, not a sel: the kept records go in, and its answer indexes the filter's lists);
    fills: called with the pass's name and its last figures after every pass"""
    import clean_model
    fills = fills or (lambda name, st: None)
    out = {}
    e.candidates_run_mixed(n, nf)
    _, out["sums_all"] = e.candidates_summaries(n=n, rc_from=nf)
    fills("summaries", e.last_summaries_stats())
    out["sel_f"], out["sums_f"], out["table"], out["why"] = e.filter_overlaps(out["sums_all"], max_drop=300, read_lens_or_n_reads=len(lens),
                                                                             table=True, why=True)
    fills("filter", e.last_filter_stats())
    out["records"] = e.candidates_fetch(n).copy()
    out["picked"] = e.select_overlaps(records=out["records"][out["sel_f"]], mode="pair")
    fills("select", e.last_select_stats())
    sel, sums = out["sel_f"][out["picked"]], out["sums_f"][out["picked"]]
    out["cover"] = e.read_coverage(lens, sel=sel, sums=sums, min_depth=3)
    fills("cover", e.last_cover_stats())
    clip = np.stack([out["cover"]["span_begin"], out["cover"]["span_end"]], axis=1).astype(np.int32).reshape(-1)
    out["reads"], out["arcs"] = e.overlap_graph(lens, sel=sel, sums=sums, clip=clip)
    fills("graph", e.last_graph_stats())
    out["arc_flags"], out["read_state"], out["steps"] = e.clean_graph(lens, out["reads"], out["arcs"], clip=clip)
    fills("clean", e.last_clean_stats())
    cleaned = clean_model.cleaned(out["arcs"], out["arc_flags"])
    out["unitigs"], out["layout"], out["places"], out["bases"] = e.unitigs(lens, out["reads"], cleaned, clip=clip, tip_reads=3, seq=True)
    fills("unitigs", e.last_unitig_stats())
    return out


def _model_chain(rs, lens, records, sums_all):
    """the same chain on the models, from the run's records and summaries"""
    import clean_model
    import cover_model
    import filter_model
    import graph_model
    import select_model
    import unitig_model
    out = {}
    f = filter_model.filter_overlaps(records, sums_all, max_drop=300, n_reads=len(lens))
    out["sel_f"], out["sums_f"], out["table"], out["why"] = f["kept_sel"], sums_all[f["kept_at"]], f["reads"], f["why"]
    out["picked"] = select_model.select(records[out["sel_f"]], "pair")
    sel, sums = out["sel_f"][out["picked"]], out["sums_f"][out["picked"]]
    out["cover"] = cover_model.cover(records, lens, sel=sel, sums=sums, min_depth=3)[0]
    clip = np.stack([out["cover"]["span_begin"], out["cover"]["span_end"]], axis=1).astype(np.int32).reshape(-1)
    g = graph_model.graph(records, lens, sel=sel, sums=sums, clip=clip)
    out["reads"], out["arcs"] = g["reads"], g["arcs"]
    c = clean_model.clean(lens, g["reads"], g["arcs"], clip=clip)
    out["arc_flags"], out["read_state"], out["steps"] = c["arc_flags"], c["read_state"], c["steps"]
    u = unitig_model.unitigs(lens, g["reads"], clean_model.cleaned(g["arcs"], c["arc_flags"]), clip=clip, tip_reads=3, seqs=rs.reads)
    out["unitigs"], out["layout"], out["places"], out["bases"] = u["unitigs"], u["layout"], u["places"], u["seq"].tobytes()
    return out


def _blob(x):
    return x if isinstance(x, bytes) else x.tobytes()


@pytest.mark.parametrize("seed", SEEDS[1:], ids=["seed-a", "seed-b"])
def test_the_chain_of_passes_behind_a_run_of_ecoli10x_small(oracle, monkeypatch, seed):
    """every pass on what the pass before it left, under both seeds: each output equals the models' chain on the run's records and
    summaries, and the chain of an engine with the switch unset; the summaries of test_gpu_paths_exact.py's sample equal the chain
    model's on the oracle"""
    import path_cases
    from conftest import workload_block
    from test_gpu_paths_exact import _small
    from test_gpu_summaries import _model_of
    blk = workload_block("ecoli10x_small")
    lens = np.array([len(r) for r in blk.rs.reads], dtype=np.int32)
    if not _CHAIN:
        monkeypatch.delenv("GACT_HIP_POISON_SCRATCH", raising=False)
        e, n, nf = path_cases.engine_with(blk.rs, blk.cf, blk.cr)
        try:
            _CHAIN["plain"] = _device_chain(e, n, nf, lens)
            assert e.scratch_fills() == (0, 0)
        finally:
            e.close()
        _CHAIN["model"] = _model_chain(blk.rs, lens, _CHAIN["plain"]["records"], _CHAIN["plain"]["sums_all"])
    n, nf = len(blk.cf) + len(blk.cr), len(blk.cf)
    seen = []
    with _Engine(monkeypatch, seed, make=lambda: path_cases.engine_with(blk.rs, blk.cf, blk.cr)[0]) as p:

        def fills(name, st):
            p.filled(st["scratch_bytes"], (name, seed))
            seen.append(name)

        got = _device_chain(p.e, n, nf, lens, fills)
    assert seen == ["summaries", "filter", "select", "cover", "graph", "clean", "unitigs"]
    plain, model = _CHAIN["plain"], _CHAIN["model"]
    for name in plain:
        assert _blob(got[name]) == _blob(plain[name]), "%s differs from the engine's without the switch" % name
    for name in model:
        assert isinstance(got[name], bytes) or got[name].dtype == model[name].dtype, name
        assert _blob(got[name]) == _blob(model[name]), "%s differs from the model's" % name
    _, cands, _, sample = _small()
    assert got["sums_all"][sample].tobytes() == _model_of(path_cases.expected(oracle, blk.rs, cands, nf, sample)).tobytes()
    assert len(got["sel_f"]) > len(got["picked"]) > 1000 and len(got["unitigs"]) >= 1 and len(got["bases"]) > 10000
    assert (got["why"] != 0).any() and (got["arc_flags"] != got["arcs"]["flags"]).any()
