"""Planted tiles: chains built so that one non-first tile has exactly the rows, columns and content one wants.

The packed int16 passes are reached through whole chains only, and a chain over ordinary reads gives its non-first tiles
whatever size and content the reads happen to have.  Here every candidate is made to contain one tile of a chosen R x Q
holding two chosen byte strings (a, b).  S is an exact random ACGT segment that both reads share:

  right phase   ref = S + a, query = S + b, candidate (|S|, |S|): the first tile runs over S alone, its maximum is its corner and
                it walks back to the reads' starts; the next tile is the non-first reverse = 1 tile of |a| rows and |b| columns.
  left phase    ref = a + S, query = b + S with |S| = tile - overlap, candidate (|a| + |S|, |b| + |S|): the first tile's maximum
                is its corner again and it walks back |S| steps, where the early-termination limit stops it; the next tile is
                the non-first reverse = 0 tile over a and b.

plant() builds reads and candidates, describe() asks the oracle what became of every one of them (tests/test_planted_tiles.py
holds it to what it is for), planted_lists() is what tests/test_gpu_planted_tiles.py runs: the candidates whose planted tile the
oracle's trace really holds.  Nothing here needs a device."""
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from gact_amd import synth

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
K_GROUP, C1, C2, LAG = 16, 7, 13, 16            # the split layout (csrc/gact_p16s.hpp): lanes, slots of region 1 / region 2 per lane
W2 = K_GROUP * C2                               # region 2's columns: a tile wider than this has columns in region 1

NOISY = ("copy0", "copy5", "copy15", "copy30")
KINDS = NOISY + ("unrelated", "homopolymer", "acac", "burst", "flood")
BURSTS = (49, 64, 100)                          # all wider than the default band of 48
# the sizes next to which the kernels at 320/120 change what they do: the first and last lane of either region (13 and 16 columns
# or rows wide), the uniform pass's lanes (8 = 128 / 16 is the other geometry's, 32 a whole wave row pair), overlap and
# tile - overlap, region 2's width, the structural sizes of tests/test_gpu_lin_level_window.py, tile - 1 and tile
EDGE_320 = (1, 2, 7, 8, 9, 12, 13, 14, 15, 16, 17, 26, 31, 32, 33, 64, 111, 112, 113, 119, 120, 121, 136, 199, 200, 201, 207,
            208, 209, 217, 224, 232, 289, 304, 319, 320)

META_DTYPE = np.dtype([("reverse", "<i4"), ("R", "<i4"), ("Q", "<i4"), ("kind", "U12")])
Planted = namedtuple("Planted", "tile overlap rs cf cr meta anchors")
Walk = namedtuple("Walk", "present n_i n_d end pos_zero band")          # end: "zero", "border" or "early"


def lane_width(tile, overlap):
    """columns per lane of the pass that takes non-first tiles at this geometry: region 2's 13 where the split layout exists
    (tile <= 320 and tile - overlap <= 208, gact_engine.hip derive_kernel_flags), else the uniform layout's 20 or 32"""
    if tile <= 20 * K_GROUP:
        return C2 if tile - overlap <= W2 else 20
    return 32


def has_split(tile, overlap):
    return tile <= 20 * K_GROUP and tile - overlap <= W2


def edge_set(tile, overlap):
    """the sizes at which a pass over a tile of this geometry can change what it does: 1 and 2, the lane boundaries at either end
    of the tile (the lane's columns and the wave's 16 rows), tile - overlap, overlap, the boundary between the two regions where the
    split layout exists and the tile reaches it, tile - 1 and tile -- each with its neighbours"""
    if (tile, overlap) == (320, 120):
        return EDGE_320
    w = lane_width(tile, overlap)
    mids = [w, K_GROUP, tile - w, tile - K_GROUP, tile - overlap, overlap]
    if has_split(tile, overlap):
        mids.append(W2)
    out = {1, 2, tile - 1, tile}
    for m in mids:
        out |= {m - 1, m, m + 1}
    return tuple(sorted(x for x in out if 1 <= x <= tile))


def pass_shape(R, Q, tile=320, overlap=120):
    """tests/test_gpu_lin_code_groups.py's pass_shape for a non-first tile of R rows and Q columns (split_last_step,
    split_first_pointer_step in csrc/gact_p16s.hpp, the loops of dp_pass_lin_split): pointer steps, first pointer step minus
    (T_end - LAG), whole blocks of both regions, whole blocks of region 2 alone, steps behind the last whole block"""
    early = tile - overlap
    r_first = max(1, R - early + 1)
    j_first = max(1, Q - early + 1)
    jj = j_first + (C2 * K_GROUP - Q)
    t = tB = r_first + (jj - 1) // C2 + K_GROUP
    T_end = R + (K_GROUP - 1) + K_GROUP
    both = r2 = 0
    while t + 7 <= T_end and t <= T_end - LAG:
        t += 8; both += 1
    while t + 7 <= T_end:
        t += 8; r2 += 1
    return T_end - tB + 1, tB - (T_end - LAG), both, r2, T_end - t + 1


def split_first_pointer_step(R, Q, early):
    """split_first_pointer_step<13> of csrc/gact_p16s.hpp: (the first step whose pointers the traceback can reach, region 2's
    lane in which the pointer window begins, its column within that lane).  Where Q > early, jj = 209 - early whatever R and Q
    are: the lane and the column are set by the geometry alone"""
    r_first = max(1, R - early + 1)
    j_first = max(1, Q - early + 1)
    jj = j_first + (C2 * K_GROUP - Q)                                   # 1-based index inside region 2
    return r_first + (jj - 1) // C2 + K_GROUP, (jj - 1) // C2, (jj - 1) % C2


def window_start(tile, overlap):
    """(lane, column) of region 2 at which the pointer window of a tile wider than tile - overlap begins"""
    early = tile - overlap
    return (W2 - early) // C2, (W2 - early) % C2


# ---------------------------------------------------------------------------------------------------------------------
def _random(rng, n):
    return ACGT[rng.integers(0, 4, size=n)]


def _noisy(rng, t, err, split=(10, 60, 30)):
    """a copy of t under the error model of synth.simulate_reads: substitutions, one-base insertions and deletions 10:60:30"""
    if err == 0:
        return t.copy()
    tot = float(sum(split))
    p_sub, p_ins, p_del = (err * s / tot for s in split)
    L = len(t)
    u = rng.random(L)
    deleted = u < p_del
    subbed = (u >= p_del) & (u < p_del + p_sub)
    base = t.copy()
    if subbed.any():
        idx = np.searchsorted(ACGT, base[subbed])
        base[subbed] = ACGT[(idx + rng.integers(1, 4, size=int(subbed.sum()))) % 4]
    ins = rng.random(L) < p_ins
    emit = (~deleted).astype(np.int64) + ins.astype(np.int64)
    ends = np.cumsum(emit)
    out = np.empty(int(ends[-1]) if L else 0, dtype=np.uint8)
    begin = ends - emit
    out[begin[ins]] = _random(rng, int(ins.sum()))
    out[(begin + ins.astype(np.int64))[~deleted]] = base[~deleted]
    return out


def _noisy_exact(rng, t, err, n):
    """n bases of a noisy copy of t, exactly: t is long enough for any error rate used here, and that is checked"""
    out = _noisy(rng, t, err)
    assert len(out) >= n, (len(out), n)
    return out[:n]


def walk_pair(rng, R, Q, kind):
    """(a, b) of exactly R and Q bases in walk order: index 0 is the cell (R, Q) the traceback starts from"""
    L = 2 * max(R, Q) + 200
    if kind in NOISY:
        err = int(kind[4:]) / 100.0
        t = _random(rng, L)
        return _noisy_exact(rng, t, err, R), _noisy_exact(rng, t, err, Q)
    if kind == "unrelated":
        return _random(rng, R), _random(rng, Q)
    if kind == "homopolymer":
        base = ACGT[int(rng.integers(0, 4))]
        return np.full(R, base, dtype=np.uint8), np.full(Q, base, dtype=np.uint8)
    if kind == "acac":
        return np.frombuffer((b"AC" * R)[:R], dtype=np.uint8).copy(), np.frombuffer((b"CA" * Q)[:Q], dtype=np.uint8).copy()
    if kind == "burst":
        # an exact copy but for one run of n bases that only one of the two has.  The run is of a base that occurs nowhere else
        # in either (under a scoring with a large match a walk would otherwise rather thread many short gaps through chance
        # matches than cross one long one); `near` bases lie between the walk's start and the run, few enough that the walk reaches
        # it before the early-termination limit, and what lies behind it scores more than the run costs wherever there is room
        x = int(rng.integers(0, 4))
        t = np.delete(ACGT, x)[rng.integers(0, 3, size=L)]
        m = min(R, Q)
        fits = [n for n in BURSTS if m >= 2 * n + 8] or [BURSTS[0]]
        n = int(fits[int(rng.integers(0, len(fits)))])
        near = int(rng.integers(4, max(5, min(91, m - 2 * n))))
        grown = np.concatenate([t[:near], np.full(n, ACGT[x], dtype=np.uint8), t[near:]])
        return (t[:R].copy(), grown[:Q].copy()) if rng.random() < 0.5 else (grown[:R].copy(), t[:Q].copy())
    if kind == "flood":
        t = _random(rng, L)
        a, b = t[:R].copy(), t[:Q].copy()
        b[:Q // 3] = _random(rng, Q // 3)
        if rng.random() < 0.5:
            a[:R // 3] = _random(rng, R // 3)
        return a, b
    raise ValueError(kind)


def _raw_bytes(rng, s):
    """s with a few N and lower-case bases (tests/tilecases.py does the same to single tiles)"""
    s = s.copy()
    for _ in range(1 + len(s) // 40):
        k = int(rng.integers(0, len(s)))
        s[k] = ord("N") if rng.random() < 0.7 else ord(chr(s[k]).lower())
    return s


def anchors(tile, overlap, scoring, threshold):
    """(|S| of the right phase, |S| of the left phase): threshold / match <= |S| <= tile - overlap on the right, where a short
    first tile leaves the planted tile its own row in the launch; exactly tile - overlap on the left"""
    early = tile - overlap
    need = -(-threshold // max(scoring[0], 1))
    assert need <= early, "no exact segment of at most tile - overlap bases reaches the threshold"
    return min(early, max(need, 64)), early


def plant(tile, overlap, scoring, threshold, shapes, kinds, seed, raw=False):
    """shapes: (R, Q) or (R, Q, kind); a shape without a kind gets two different ones of `kinds`, drawn from the seed.  Every
    (shape, kind) is planted once in each direction.  Returns Planted: rs (synth.ReadSet; per candidate a ref, a query and the
    query's reverse complement), cf / cr (forward and reverse-complement candidates, the same coordinates), meta (one row per
    forward candidate = per reverse-complement candidate) and the two anchor lengths"""
    rng = np.random.default_rng(seed)
    s_right, s_left = anchors(tile, overlap, scoring, threshold)
    todo = []
    for sh in shapes:
        if len(sh) == 3:
            todo.append(tuple(sh))
        else:
            for k in rng.choice(len(kinds), size=min(2, len(kinds)), replace=False):
                todo.append((sh[0], sh[1], kinds[int(k)]))
    rs = synth.ReadSet()
    cf, cr, meta = [], [], []
    for R, Q, kind in todo:
        assert 1 <= R <= tile and 1 <= Q <= tile, (R, Q)
        for reverse in (1, 0):
            a, b = walk_pair(rng, R, Q, kind)
            if raw:
                a, b = _raw_bytes(rng, a), _raw_bytes(rng, b)
            assert len(a) == R and len(b) == Q
            if reverse:                 # right phase: the tile is read back to front, the walk starts at a[0], b[0]
                S = _random(rng, s_right)
                ref, query, pos = np.concatenate([S, a]), np.concatenate([S, b]), (s_right, s_right)
            else:                       # left phase: the walk starts at the last bases of a and b
                S = _random(rng, s_left)
                ref, query, pos = np.concatenate([a[::-1], S]), np.concatenate([b[::-1], S]), (R + s_left, Q + s_left)
            base = rs.n
            tag = "%s%d_%dx%d_%s" % ("lr"[reverse], len(meta), R, Q, kind)
            for name, seq in (("ref", ref), ("q", query), ("qrc", synth.revcomp(query))):
                rs.reads.append(np.ascontiguousarray(seq)); rs.names.append("%s_%s" % (tag, name))
            cf.append((base, base + 1) + pos)
            cr.append((base, base + 2) + pos)
            meta.append((reverse, R, Q, kind))
    return Planted(tile, overlap, rs, np.array(cf, dtype=synth.CAND_DTYPE), np.array(cr, dtype=synth.CAND_DTYPE),
                   np.array(meta, dtype=META_DTYPE), (s_right, s_left))


# ---------------------------------------------------------------------------------------------------------------------
def _planted_bytes(pl, k):
    """(a, b) of candidate k as the tile holds them, and the tile's offsets in ref and query"""
    c, m = pl.cf[k], pl.meta[k]
    ref, query = pl.rs.reads[int(c["ref_id"])], pl.rs.reads[int(c["query_id"])]
    R, Q = int(m["R"]), int(m["Q"])
    if m["reverse"]:
        return ref[pl.anchors[0]:].tobytes(), query[pl.anchors[0]:].tobytes(), pl.anchors[0], pl.anchors[0]
    return ref[:R].tobytes(), query[:Q].tobytes(), 0, 0


def _walk(states, R, Q, early, pos_score):
    n_i = n_d = di = dj = band = 0
    for s in states:
        if s == 3:
            di += 1; dj += 1
        elif s == 2:
            di += 1; n_i += 1
        else:
            dj += 1; n_d += 1
        band = max(band, abs(di - dj))
    end = "border" if di == R or dj == Q else "early" if di >= early or dj >= early else "zero"
    return n_i, n_d, end, pos_score == 0, band


def describe(oracle, pl, scoring, threshold, n_threads=8):
    """what the oracle makes of every forward candidate: a list of Walk.  present: the chain's trace holds the planted tile as
    (first = 0, reverse = d, ref_len = |a|, query_len = |b|) at the place of a and b; the rest describes that tile's walk,
    from oracle.align_with_bt on a and b themselves"""
    early = pl.tile - pl.overlap

    def one(k):
        c, m = pl.cf[k], pl.meta[k]
        ref, query = pl.rs.reads[int(c["ref_id"])].tobytes(), pl.rs.reads[int(c["query_id"])].tobytes()
        a, b, roff, qoff = _planted_bytes(pl, k)
        _, traces = oracle.gact(ref, query, int(c["ref_pos"]), int(c["query_pos"]), tile_size=pl.tile, tile_overlap=pl.overlap,
                                threshold=threshold, ref_id=0, query_id=1, scoring=scoring, trace_cap=16)
        present = any(not t.first and t.reverse == m["reverse"] and t.ref_len == m["R"] and t.query_len == m["Q"] and
                      t.ref_off == roff and t.query_off == qoff for t in traces)
        bt = oracle.align_with_bt(a, b, scoring, bool(m["reverse"]), False, early)
        return Walk(present, *_walk(bt[1:], len(a), len(b), early, bt[0]))

    with ThreadPoolExecutor(n_threads) as pool:
        return list(pool.map(one, range(len(pl.cf))))


# ---------------------------------------------------------------------------------------------------------------------
def lin_sizes():
    """the union of the SIZES of the four lin files (tests/test_gpu_lin_*.py); written out so that this module needs no device
    file: tests/test_planted_tiles.py checks it against them"""
    return tuple(range(1, 65)) + (111, 112, 113, 119) + tuple(range(120, 137)) + tuple(range(193, 233)) + tuple(range(289, 321))


def shapes(tile, overlap, pad=True):
    """the clean list's shapes at a geometry: the cross product of the edge set, each with two kinds; at 320/120 also every
    structural size of the lin files against itself and against the full tile, with 15 % noise, and bursts on the largest tiles
    (walks that leave the default band need room for a run of 49 and for what pays for it).  pad: a small edge set's shapes are
    repeated until the list holds 600 candidates (the geometries of CONFIGS; those of GEOMETRIES are many and stay as they are)"""
    es = edge_set(tile, overlap)
    out = [(r, q) for r in es for q in es]
    if (tile, overlap) == (320, 120):
        for x in lin_sizes():
            out += [(x, 320, "copy15"), (320, x, "copy15"), (x, x, "copy15")]
            out.append((x, x, "unrelated"))                           # clamped cells everywhere, at every structural size
            if x <= 64:                                               # walks that start on H = 0 need a short side
                out += [(x, 320, "unrelated"), (320, x, "unrelated"), (x, 200, "unrelated"), (200, x, "unrelated")]
        big = (224, 232, 289, 304, 319, 320)
        out += [(r, q, "burst") for r in big for q in big] + [(320, 320, "burst")] * 4
    else:
        if tile - overlap >= BURSTS[0]:
            # (below that the band is the whole pointer window, which no walk can leave; and the left phase's anchor of
            # tile - overlap bases scores less than crossing a run costs, so the first tile would end in front of the run)
            big = ([x for x in es if x >= 2 * BURSTS[0] + 8] or list(es))[-4:]
            out += [(r, q, "burst") for r in big for q in big] * 2
        if not pad and 0 < overlap < C2:
            # an overlap this small: only a walk from the corner of a full tile is long enough to end at the early-termination
            # limit, tile - overlap steps on, in front of the border -- and the edge set's cross product holds that shape once
            out += [(tile, tile, k) for k in NOISY] * 8
        while pad and len(out) * 2 < 600:                            # small edge sets: more kinds per shape
            out += [(r, q) for r in es for q in es]
    return out


def raw_shapes(tile, overlap):
    es = edge_set(tile, overlap)
    return [(r, q, "copy15") for r in es for q in es]


PLAIN, ZERO_GAP, AFFINE, MAX_AFFINE = (1, -1, -1, -1), (2, 0, 0, 0), (2, -3, -5, -2), (1, -11, -13, -11)
# (tile, overlap, scoring, layouts of tests/test_gpu_int16_edges.py's LAYOUTS): what tests/test_gpu_planted_tiles.py runs.
# "max-gap" / "max-linear": the largest |g| / the largest match - g for which the engine plans the linear-gap pass at 320
CONFIGS = (
    (320, 120, PLAIN, ("split", "coop", "wide", "uniform")),      # column-drifted split lin, wide lin, tagged uniform
    (320, 120, ZERO_GAP, ("split", "coop")),                      # column-drifted split lin at its value extremes
    (320, 120, "max-gap", ("split", "coop")),
    (320, 120, "max-linear", ("split", "coop")),
    (320, 120, AFFINE, ("split", "no-aff", "wide", "uniform", "plain")),      # drifted affine; tagged split / wide / uniform; untagged
    (320, 120, MAX_AFFINE, ("split",)),                           # drifted affine at its largest drift
    (320, 100, AFFINE, ("split",)),                               # tagged uniform: the geometry allows no split
    (128, 32, PLAIN, ("split", "coop")),                          # the same passes where most of the lanes hold pads
    (128, 32, AFFINE, ("split",)),
    (64, 8, (61, -1, -1, -1), ("split", "coop")),                 # the last column-drifted scoring ...
    (64, 8, (62, -1, -1, -1), ("split", "coop")),                 # ... and the first row-drifted one
    (512, 128, PLAIN, ("split",)),                                # uniform, 32 columns per lane
)
RAW_CONFIGS = ((320, 120, PLAIN), (320, 120, AFFINE), (317, 119, PLAIN))       # 317: N and lower case where the tile fills no whole lane

# Tile geometries: R and Q leave unchanged where in region 2 the split pass's pointer window begins (window_start: tile - overlap
# alone sets it), which of the three kernel families runs (derive_kernel_flags: tile <= 320, tile - overlap <= 208, tile > 512)
# and how much of the last lane and lane group a full tile fills.  (tile, overlap, what the row is for, the main kernel that
# engine.plan names for 50,000 candidates under PLAIN, the same under AFFINE)
LIN, AFF, UNI = "SplitLayoutLin", "SplitLayoutAff<cbneg>", "UniformLayout<tag>"
WIDE_LIN, WIDE_TAG = "WideLayoutLin", "WideLayoutTagged"                   # what 100 candidates get where tile <= 320
Geometry = namedtuple("Geometry", "tile overlap what plain affine")
GEOMETRIES = tuple(Geometry(*g) for g in (
    (320, 112, "largest split early (208): the window begins on region 2's first column, lane 0 column 0", LIN, AFF),
    (320, 113, "lane 0, column 1", LIN, AFF),
    (320, 124, "last column of lane 0", LIN, AFF),
    (320, 125, "first column of lane 1", LIN, AFF),
    (320, 216, "first column of lane 8", LIN, AFF),
    (320, 294, "first column of lane 14", LIN, AFF),
    (320, 307, "first column of the last lane", LIN, AFF),
    (320, 308, "inside the last lane: early less than a lane", LIN, AFF),
    (320, 319, "one step per tile, 320 tiles a chain", LIN, AFF),
    (320, 111, "early 209: the first past the split layout", UNI, UNI),
    (209, 0, "the same boundary with early == tile", UNI, UNI),
    (208, 0, "no region 1 at all, early == tile", LIN, AFF),
    (209, 1, "one column in region 1", LIN, AFF),
    (317, 119, "tile no multiple of 16, 13, 8 or 7", LIN, AFF),
    (300, 100, "region 1 of 92 columns, no multiple of 7", LIN, AFF),
    (250, 90, "tile no multiple of 16", LIN, AFF),
    (100, 37, "both odd", LIN, AFF),
    (33, 7, "two lane groups and one column", LIN, AFF),
    (17, 3, "one lane group and one column", LIN, AFF),
    (16, 8, "one lane group", LIN, AFF),
    (15, 0, "less than one lane group", LIN, AFF),
    (2, 1, "the smallest tile with an overlap", LIN, AFF),
    (1, 0, "the smallest tile the engine accepts", LIN, AFF),
    (321, 121, "first tile size on 32 columns per lane", UNI, UNI),
    (321, 113, "early 208 would allow the split, the tile size does not", UNI, UNI),
    (333, 0, "32 columns per lane, overlap 0", UNI, UNI),
    (511, 200, "the last size below 512, odd", UNI, UNI),
))
# the window starts the split rows must cover: a lane's first column (lanes 0, 1, 8, 14, 15), its second, its last, the last lane
WINDOW_STARTS = ((0, 0), (0, 1), (0, 12), (1, 0), (8, 0), (14, 0), (15, 0), (15, 1))


def geometry_layouts(g):
    """[(scoring, layout of tests/test_gpu_int16_edges.py's LAYOUTS)] that tests/test_gpu_planted_tiles.py runs a row through"""
    if g.plain == UNI:
        return [(PLAIN, "split"), (AFFINE, "split")]                  # (it resolves to the uniform kernel, as 320/100 does)
    out = [(PLAIN, "split"), (AFFINE, "split"), (PLAIN, "coop"), (PLAIN, "wide")]
    if (g.tile, g.overlap) in ((320, 125), (317, 119)):
        out += [(PLAIN, "uniform"), (PLAIN, "plain")]
    return out


def resolve(scoring):
    """a scoring of CONFIGS as four numbers (the named ones are asked of the engine's plan: no device needed)"""
    if scoring == "max-gap":
        from test_gpu_lin_col_drift import _max_gap_scoring
        scoring = _max_gap_scoring()
        assert scoring is not None and scoring[1] <= -12, scoring
    elif scoring == "max-linear":
        from test_gpu_lin_code_groups import _max_linear_scoring
        scoring = _max_linear_scoring()
        assert scoring is not None and scoring[0] - scoring[1] >= 19, scoring
    return tuple(scoring)


def default_threshold(scoring, tile=320, overlap=120):
    """the first tile's threshold: 35 matches, or as many as the exact segment of tile - overlap bases has"""
    return min(35, tile - overlap) * max(scoring[0], 1)


_PLANTED, _LISTS = {}, {}


def planted(tile, overlap, raw=False):
    """the reads and candidates of one geometry, built once: the anchors hold for every scoring used with default_threshold
    (min(35, tile - overlap) matches), so every scoring of a geometry shares them"""
    key = (tile, overlap, raw)
    if key not in _PLANTED:
        pad = any((tile, overlap) == c[:2] for c in CONFIGS)
        _PLANTED[key] = plant(tile, overlap, (1, -1, -1, -1), min(35, tile - overlap),
                              raw_shapes(tile, overlap) if raw else shapes(tile, overlap, pad),
                              (KINDS[2],) if raw else KINDS, seed=4000 + tile * 3 + overlap + (7 if raw else 0), raw=raw)
    return _PLANTED[key]


def planted_lists(oracle, tile, overlap, scoring, raw=False):
    """(Planted with the failing candidates dropped from cf, cr and meta, the list of Walk of those kept, share of candidates
    kept per direction {0: .., 1: ..}) under one scoring"""
    key = (tile, overlap, scoring, raw)
    if key not in _LISTS:
        pl = planted(tile, overlap, raw)
        walks = describe(oracle, pl, scoring, default_threshold(scoring, tile, overlap))
        keep = np.array([w.present for w in walks], dtype=bool)
        share = {d: float(keep[pl.meta["reverse"] == d].mean()) for d in (0, 1)}
        kept = pl._replace(cf=pl.cf[keep], cr=pl.cr[keep], meta=pl.meta[keep])
        for arr in (kept.cf, kept.cr, kept.meta):
            arr.setflags(write=False)
        _LISTS[key] = (kept, [w for w in walks if w.present], share)
    return _LISTS[key]
