"""The column-drifted frame of the split linear-gap pass (csrc/gact_lin.hpp 2b., dp_pass_lin_split_col), modelled in numpy at
lane level, and the rule by which the launch takes the row-drifted pass instead (lin_col_drift_ok, gact_lin.hpp 12.).

The pass keeps the cell a lane computes at step t in column slot c as X + base + (t + c)|g|.  H_left + g is then the left
neighbour as it stands and H_up + g the upper one; the diagonal lies two gaps below, which the look-up words carry
(lin_lut_fill_col, csrc/gact_p16.hpp); the zero level of (t, c) is the same number in every lane, a window of scalars moved
once per step; and a value that crosses a lane is converted by a constant: (C1 - 1)|g| inside region 1 and from region 1
into region 2, (C2 - 1)|g| inside region 2.

The model runs the pass as the kernel does: 16 lanes, regions of 7 and 13 slots, region 2 LAG = 16 steps behind, two tiles in
the half-words of a uint32 with 32-bit additions and subtractions (a carry or borrow between the halves would show), tiles
right-aligned with pad columns on the left and pad rows in front of a delayed tile and behind every tile, the steps of region
1 alone, of both regions, and the pointer phase entered at any step tB (scores times four, tags M 3 / up 2 / left 1, stored
form (H'' & ~3) | 2, left retag - 1).  It is held to the plain recurrence: H of every cell, the op of every cell of the
pointer phase, and H[R][Q] as the pass returns it.  It also holds, over every scoring the guard admits at tiles 1 .. 320,
that the rule is exact for the pointer phase's byte -- it fits where the rule says column-drifted, it does not where it says
row-drifted, and at tiles 305..320 it always fits -- and that every value of the frame is a normal positive half."""
import numpy as np
import pytest

from test_lin_lut_table import K_LIN_FLOOR, ONES, admitted, p16_lin_ok

LANES, C1, C2, LAG = 16, 7, 13, 16
CT, TILE_MAX = C1 + C2, (C1 + C2) * 16
LIN_PAD = 32
LO, HI = 0x0400, 0x7BFF                    # every value: a normal, finite, positive half-precision number
M32 = 0xFFFFFFFF
def lin_col_drift_ok(match, ext):
    """csrc/gact_lin.hpp lin_col_drift_ok, restated"""
    return match - 2 * ext <= 63


def lin_base(g):
    return K_LIN_FLOOR + 40 * (-g) + 8


def pk2(v):
    return (v & 0xFFFF) | ((v & 0xFFFF) << 16)


def table(match, g):
    """lin_lut_fill_col: a real row's bytes gain |g| on plain scores and 4|g| in the pointer phase; the pad row's do not"""
    d, a = match - g, -g
    words = []
    for tid in range(10):
        b = 8 * (tid >> 1)
        base = ((4 * d if tid & 1 else d) << 24) & M32
        gap = ((4 * a if tid & 1 else a) & 0xFF) * ONES
        words.append((((base >> b) + gap if b < LIN_PAD else 0) + (ONES if tid & 1 else 0)) & M32)
    return words


def reference(ref, qry, match, g):
    """the plain recurrence (csrc/gact_lin.hpp 1.): H and op (M 3 wins a tie, then up 2, then left 1; H == 0 reads as 3)"""
    R, Q = len(ref), len(qry)
    H = [[0] * (Q + 1) for _ in range(R + 1)]
    op = [[0] * (Q + 1) for _ in range(R + 1)]
    for i in range(1, R + 1):
        Hi, Hu, ri = H[i], H[i - 1], ref[i - 1]
        for j in range(1, Q + 1):
            m = max(Hu[j - 1] + (match if ri == qry[j - 1] else g), 0)
            u, l = Hu[j] + g, Hi[j - 1] + g
            h = max(m, u, l)
            Hi[j] = h
            op[i][j] = 3 if h == m else 2 if h == u else 1
    return H, op


def reference_rows(ref, qry, match, g):
    """the same H and op a row at a time: H[i][j] = max over k <= j of b[k] + (j - k) g with b = max(M, H_up + g), a running
    maximum of b[k] - k g.  Only for speed on the large shapes; the test holds it to reference() on the small ones"""
    R, Q = len(ref), len(qry)
    ref, qry = np.asarray(ref), np.asarray(qry)
    H = np.zeros((R + 1, Q + 1), dtype=np.int64)
    op = np.zeros((R + 1, Q + 1), dtype=np.int64)
    j = np.arange(1, Q + 1)
    for i in range(1, R + 1):
        m = np.maximum(H[i - 1, :-1] + np.where(qry == ref[i - 1], match, g), 0)
        u = H[i - 1, 1:] + g
        H[i, 1:] = np.maximum.accumulate(np.maximum(m, u) - j * g) + j * g
        op[i, 1:] = np.where(H[i, 1:] == m, 3, np.where(H[i, 1:] == u, 2, 1))
    return H, op


class Range:
    lo, hi = 1 << 20, 0

    def see(self, *arrays):
        for a in arrays:
            a = np.asarray(a, dtype=np.uint32)
            self.lo = min(self.lo, int((a & 0xFFFF).min()), int((a >> 16).min()))
            self.hi = max(self.hi, int((a & 0xFFFF).max()), int((a >> 16).max()))


def pk_max(a, b):
    """v_pk_max_i16 / v_pk_maximum3_f16 on values in [LO, HI]: the larger half-word, each half by itself"""
    lo = np.maximum(a & 0xFFFF, b & 0xFFFF)
    hi = np.maximum(a >> 16, b >> 16)
    return (lo | (hi << 16)).astype(np.uint32)


def model(tiles, match, g, tB):
    """tiles: two (ref, qry) pairs of 2-bit codes.  Returns, per tile, H[i][j] of every real cell, op[i][j] of every real cell
    of the pointer phase (-1 elsewhere), H[R][Q] as returned, and the range of every value that went through a maximum"""
    a = -g
    R = [len(t[0]) for t in tiles]
    Q = [len(t[1]) for t in tiles]
    T_end = max(r + (LANES - 1) + LAG for r in R)
    shift = [T_end - (r + (LANES - 1) + LAG) for r in R]          # every tile's last row on the wave's last step
    words = table(match, g)
    rng = Range()
    u32 = lambda x: (np.asarray(x, dtype=np.int64) & M32).astype(np.uint32)
    add = lambda x, y: u32(x.astype(np.int64) + np.asarray(y, dtype=np.int64))     # v_add_u32
    sub = lambda x, y: u32(x.astype(np.int64) - np.asarray(y, dtype=np.int64))     # v_sub_u32
    lanes = np.arange(LANES)

    # column map: the tile right-aligned in 16 x 7 + 16 x 13 slots; code of the column or -1 for a pad column
    def col_of(h, region, lane, c):
        s = lane * C1 + c if region == 1 else LANES * C1 + lane * C2 + c
        return s - (TILE_MAX - Q[h])                                               # 0-based column, < 0: pad

    qcode = np.full((2, CT, LANES), -1)
    jcol = np.full((2, CT, LANES), -1)
    for h in range(2):
        for c in range(CT):
            for l in range(LANES):
                j = col_of(h, 1, l, c) if c < C1 else col_of(h, 2, l, c - C1)
                jcol[h, c, l] = j
                if j >= 0:
                    qcode[h, c, l] = tiles[h][1][j]

    def row_of(h, region, t):
        return t - lanes - shift[h] - (LAG if region == 2 else 0)                  # per lane; outside 1..R: a pad row

    # the stream: a row's byte is 24 - 8 * code, the pad row's kLinPadRow, and IS the byte offset of its pair of words
    wtab = np.array(words, dtype=np.uint32)
    stream = [np.concatenate([[LIN_PAD], 24 - 8 * np.asarray(tiles[h][0], dtype=np.int64), [LIN_PAD]]) for h in range(2)]

    def row_words(region, t, phase):
        """per lane the look-up words of tile A and tile B for the row of this step"""
        out = []
        for h in range(2):
            i = row_of(h, region, t)
            byte = stream[h][np.clip(i, 0, R[h] + 1)]
            out.append(wtab[byte // 4 + phase])
        return out

    def shr1(v, lane0):
        out = np.empty(LANES, dtype=np.uint32)
        out[1:] = v[:-1]
        out[0] = lane0
        return out

    NWIN = C2 + 1
    g2, g42 = pk2(a), pk2(4 * a)
    W = [pk2(lin_base(g) + (k - 1) * a) for k in range(NWIN)]                      # before step 1: Zw(k - 1)
    T = [0] * C2
    k1, k2, k24, k12 = pk2((C1 - 1) * a), pk2((C2 - 1) * a), pk2((C2 - 1) * 4 * a), pk2(2 - 4 * (C1 - 1) * a)
    full = lambda s: np.full(LANES, s, dtype=np.uint32)
    G = np.stack([full(W[(c if c < C1 else c - C1) + 1]) for c in range(CT)])      # H of the previous step, [slot][lane]
    H1, H2 = full(W[C1]), full(W[C2])
    Hd1, Hd2 = full(W[0]), full(W[0])
    Hcells = [np.full((R[h] + 1, Q[h] + 1), -1 << 20, dtype=np.int64) for h in range(2)]      # [i][j]; -2^20: not computed
    ops = [np.full((R[h] + 1, Q[h] + 1), -1, dtype=np.int64) for h in range(2)]

    slot_of = np.array([c if c < C1 else c - C1 for c in range(CT)])
    region_of = np.array([1 if c < C1 else 2 for c in range(CT)])

    def record(t, cs, vals, tagged):
        """true H (and op) of the real cells a step has just computed in the slots cs, frame taken off"""
        for h in range(2):
            for region in (1, 2):
                sel = [k for k, c in enumerate(cs) if region_of[c] == region]
                if not sel:
                    continue
                c = np.asarray(cs)[sel]
                i = np.broadcast_to(row_of(h, region, t), (len(c), LANES))
                v = ((vals[sel] >> (16 * h)) & 0xFFFF).astype(np.int64)
                real = (i >= 1) & (i <= R[h]) & (jcol[h, c] >= 0)
                ii, jj = i[real], jcol[h, c][real] + 1
                frame = np.broadcast_to((lin_base(g) + (t + slot_of[c]) * a)[:, None], real.shape)[real]
                assert (Hcells[h][ii, jj] == -1 << 20).all()                       # every cell is computed once
                Hcells[h][ii, jj] = ((v[real] >> 2) if tagged else v[real]) - frame
                if tagged:
                    ops[h][ii, jj] = v[real] & 3

    def mad4(v, c):
        """v_pk_mad_u16 v, 4, c: each half times four plus its constant, wrapping in the half"""
        lo = ((v & 0xFFFF).astype(np.int64) * 4 + (c & 0xFFFF)) & 0xFFFF
        hi = ((v >> 16).astype(np.int64) * 4 + (c >> 16)) & 0xFFFF
        return (lo | (hi << 16)).astype(np.uint32)

    def advance(nW, tagged_too):
        for k in range(nW):
            W[k] = (W[k] + g2) & M32                                               # s_add_u32 on both half-words at once
        if tagged_too:
            for c in range(C2):
                T[c] = (T[c] + g42) & M32

    qsel = np.maximum(qcode, 0).astype(np.uint32) * 8
    qreal = qcode >= 0

    def upper(t, cs, tag2):
        """the stage off the column chain, all slots of cs at once: v_perm_b32, v_add_u32, v_pk_maximum3_f16"""
        cs = np.asarray(cs)
        wA, wB = np.empty((len(cs), LANES), dtype=np.uint32), np.empty((len(cs), LANES), dtype=np.uint32)
        for region in (1, 2):
            m = region_of[cs] == region
            if m.any():
                wa, wb = row_words(region, t, 1 if (tag2 and region == 2) else 0)
                wA[m], wB[m] = wa, wb
        # v_perm_b32: byte 0 = tile A's byte of the column's code, byte 2 = tile B's, a pad column the constant 0
        P = (np.where(qreal[0, cs], (wA >> qsel[0, cs]) & 0xFF, 0) | (np.where(qreal[1, cs], (wB >> qsel[1, cs]) & 0xFF, 0) << 16)).astype(np.uint32)
        diag = np.stack([Hd1 if c == 0 else Hd2 if c == C1 else G[c - 1] for c in cs])
        Z = np.array([W[c + 1] if c < C1 else T[c - C1] if tag2 else W[c - C1 + 1] for c in cs], dtype=np.uint32)[:, None]
        u = add(diag, P)
        rng.see(u, Z, G[cs])
        return pk_max(pk_max(u, np.broadcast_to(Z, u.shape)), G[cs])

    def step(t, regions, tag2):
        nonlocal H1, H2, Hd1, Hd2
        advance(NWIN if (regions == (1, 2) and not tag2) else C1 + 1 if 1 in regions else 0, tag2)
        if 1 in regions:
            Hl1 = shr1(sub(H1, k1), W[0])                                          # lane 0: the j = 0 border, Zw(t - 1)
        if 2 in regions:
            if tag2:
                # lane 15's region-1 column enters region 2 scaled, its frame constant and tag 2 in the addend
                Hl2 = shr1(sub(H2, k24), mad4(H1, k12)[LANES - 1])
            else:
                Hl2 = shr1(sub(H2, k2), sub(H1, k1)[LANES - 1])
        cs = [c for c in range(CT) if region_of[c] in regions]
        U = dict(zip(cs, upper(t, cs, tag2)))
        if 1 in regions:
            Hd1 = Hl1
            Ha = Hl1
            for c in range(C1):
                G[c] = pk_max(U[c], Ha)                                            # H_left + g: the neighbour as it stands
                Ha = G[c]
            H1 = Ha.copy()
            rng.see(Hl1)
            record(t, list(range(C1)), G[:C1], False)
        if 2 in regions:
            Hd2 = Hl2
            Hb = Hl2
            rng.see(Hl2)
            Hp = np.empty((C2, LANES), dtype=np.uint32)
            for c in range(C2):
                if tag2:
                    Hp[c] = pk_max(U[C1 + c], sub(Hb, 0x00010001))                 # G'' tagged 2 -> D'' tagged 1
                    G[C1 + c] = (Hp[c] & np.uint32(0xFFFCFFFC)) | np.uint32(0x00020002)
                else:
                    Hp[c] = G[C1 + c] = pk_max(U[C1 + c], Hb)
                Hb = G[C1 + c]
            H2 = Hb.copy()
            record(t, list(range(C1, CT)), Hp, tag2)

    t = 1
    tP = min(LAG, tB - 1, T_end)
    while t <= tP:
        step(t, (1,), False)
        t += 1
    if t > 1:
        for k in range(C1 + 1, NWIN):
            W[k] = (W[k - 1] + g2) & M32
        for c in range(C1, CT):
            G[c] = full(W[c - C1 + 1])
        H2, Hd2 = full(W[C2]), full(W[0])
    tU = min(tB - 1, T_end)
    while t <= tU:
        step(t, (1, 2), False)
        t += 1
    tagged = t <= T_end
    if tagged:
        for c in range(C1, CT):
            G[c] = mad4(G[c], 0x00020002)
        H2, Hd2 = mad4(H2, 0x00020002), mad4(Hd2, 0x00020002)
        for c in range(C2):
            T[c] = ((W[c + 1] << 2) + 0x00030003) & M32
    while t <= T_end - LAG:
        step(t, (1, 2), True)
        t += 1
    while t <= T_end:
        step(t, (2,), True)
        t += 1
    if tagged:
        fin = int(H2[LANES - 1]) | 0x00030003                                      # v_pk_sub_i16, v_pk_ashrrev_i16
        ret = [((((fin >> (16 * h)) & 0xFFFF) - ((T[C2 - 1] >> (16 * h)) & 0xFFFF)) & 0xFFFF) >> 2 for h in range(2)]
    else:
        ret = [(((int(H2[LANES - 1]) >> (16 * h)) & 0xFFFF) - ((W[C2] >> (16 * h)) & 0xFFFF)) & 0xFFFF for h in range(2)]
    return Hcells, ops, ret, rng, T_end


def _reads(rng, R, Q):
    """a reference of R codes and a query of Q: the query a copy with point errors and a short indel, so that all three moves occur"""
    n = max(R, Q) + 8
    ref = rng.integers(0, 4, size=n)
    qry = ref.copy()
    flip = rng.random(n) < 0.12
    qry[flip] = rng.integers(0, 4, size=int(flip.sum()))
    if n > 12:
        cut = int(rng.integers(3, n - 6))
        qry = np.concatenate([qry[:cut], qry[cut + 2:], rng.integers(0, 4, size=2)])
    return [int(x) for x in ref[:R]], [int(x) for x in qry[:Q]]


def _scorings():
    adm = admitted(320)
    max_gap = min(g for _, g in adm)
    widest = max(adm, key=lambda mg: (mg[0] - mg[1], mg[0]))
    out = [(1, -1), (2, 0), (max(m for m, g in adm if g == max_gap), max_gap), widest, (18, -1), (1, -12)]
    assert all(p16_lin_ok(320, m, g, g, g) for m, g in out)
    return list(dict.fromkeys(out))


SMALL = (((1, 1), (2, 7)), ((7, 2), (8, 8)), ((13, 14), (14, 13)), ((16, 17), (17, 16)), ((17, 1), (1, 17)), ((8, 16), (13, 7)))
BIG = (((207, 207), (209, 208)), ((208, 209), (207, 320)), ((319, 319), (320, 320)), ((320, 319), (16, 320)), ((320, 320), (209, 1)))


def _check(pair, match, g, tB_of, seed):
    rng = np.random.default_rng(seed)
    tiles = [_reads(rng, *pair[0]), _reads(rng, *pair[1])]
    T_end = max(len(t[0]) for t in tiles) + 31
    tB = tB_of(T_end)
    Hc, ops, ret, seen, _ = model(tiles, match, g, tB)
    assert LO <= seen.lo and seen.hi <= HI, (pair, match, g, tB, seen.lo, seen.hi)
    for h, (ref, qry) in enumerate(tiles):
        R, Q = len(ref), len(qry)
        H, op = reference_rows(ref, qry, match, g)
        if R * Q <= 17 * 17:
            Hp, opp = reference(ref, qry, match, g)
            assert np.array_equal(H, np.array(Hp)) and np.array_equal(op, np.array(opp))
        bad = np.argwhere(Hc[h][1:, 1:] != H[1:, 1:])                              # (a cell never computed differs too)
        assert len(bad) == 0, (pair, (match, g), tB, "tile %d H[%d][%d]" % (h, bad[0][0] + 1, bad[0][1] + 1))
        made = ops[h] >= 0
        bad = np.argwhere(made & (ops[h] != op))
        assert len(bad) == 0, (pair, (match, g), tB, "tile %d op[%d][%d]" % (h, bad[0][0], bad[0][1]))
        assert ret[h] == H[R][Q], (pair, (match, g), tB, h, ret[h], H[R][Q])
        if tB == 1:
            # pointers from the first step on: every real cell of region 2 has its op
            assert made.sum() == R * min(Q, C2 * LANES), (pair, h, int(made.sum()))
    return tB


TB_KINDS = {
    "from-step-1": lambda T_end: 1,
    "inside-region-1-alone": lambda T_end: min(9, T_end),
    "before-T_end-LAG": lambda T_end: max(2, T_end - LAG - 5),
    "at-T_end-LAG": lambda T_end: max(1, T_end - LAG),
    "after-T_end-LAG": lambda T_end: T_end - LAG + 3,
    "last-step": lambda T_end: T_end,
    "never": lambda T_end: T_end + 1,
}


@pytest.mark.parametrize("kind", sorted(TB_KINDS))
def test_small_tiles_every_scoring_every_entry(kind):
    for n, pair in enumerate(SMALL):
        for k, (match, g) in enumerate(_scorings()):
            _check(pair, match, g, TB_KINDS[kind], 100 * n + k)


@pytest.mark.parametrize("pair", BIG, ids=lambda p: "%dx%d+%dx%d" % (p[0] + p[1]))
def test_region_1_and_the_border_come_into_use(pair):
    """207..209 columns: the first slots of region 1 hold real columns; 319, 320: the pad columns shrink to none and lane 0 of
    region 1 meets the j = 0 border.  Every scoring, the entry into the pointer phase rotating through its kinds"""
    kinds = sorted(TB_KINDS)
    for k, (match, g) in enumerate(_scorings()):
        _check(pair, match, g, TB_KINDS[kinds[(k + BIG.index(pair)) % len(kinds)]], 7000 + k)


def test_bounds_over_everything_the_guard_admits():
    """every tile 1..320 (the layout holds 320 columns and runs every smaller tile right-aligned) and every scoring the guard
    admits there.  Where the launch gives it the column-drifted pass, the pointer phase's byte 4 (match + 2|g|) + 1 fits and every
    value of the frame -- from the diagonal of the first step, one gap below base, to the largest tagged score at the last slot of
    the last step -- is a normal positive half; where it does not, the byte would not fit (the rule is exact), the row-drifted
    pass's does, and the tile is below 305.

    The range also follows from the guard without enumerating.  With a = |g|, the largest value is
    4 (match tile + lin_base + (T_end + C2 - 1) a) + 3 with lin_base = 1024 + 40 a + 8 and T_end = tile + 31, that is
    4 (match tile + a (tile + 83) + 1032) + 3; p16_lin_ok holds 4 (match (tile + 2) + a (tile + 176) + 1024) + 3 <= 30000, and
    a (tile + 83) + 8 <= a (tile + 176) + 2 match + 8, so the largest value is at most 30000 + 32 < 0x7BFF.  The smallest is
    lin_base - a = 1032 + 39 a >= 0x0400"""
    n = 0
    g = -np.arange(0, 64)[:, None]                                       # (the guard's match - ext <= 63 bounds both)
    m = np.arange(0, 128)[None, :]
    a = -g
    row_tiles = set()
    for tile in range(1, 321):
        steps = tile + 4 * 16 + 64 + 48
        ok = ((m * (tile + 2) <= 7900) & (m - g <= 63) & (g >= -1000) &
              (4 * (m * (tile + 2) + a * steps + K_LIN_FLOOR) + 3 <= 30000))            # p16_lin_ok with p16_tagged_ok, restated
        if tile in (64, 128, 200, 305, 320):
            assert {(int(mm), int(gg)) for gg, mm in zip(*np.nonzero(ok))} == {(mm, -gg) for mm, gg in admitted(tile)}, tile
        col = ok & (m - 2 * g <= 63)                                                      # lin_col_drift_ok
        row = ok & ~col
        byte = 4 * (m + 2 * a) + 1
        assert (byte[col] <= 255).all() and (byte[row] > 255).all(), tile
        assert ((4 * (m - g) + 1)[row] <= 255).all(), tile
        if row.any():
            row_tiles.add(tile)
        T_end = tile + (LANES - 1) + LAG
        base = K_LIN_FLOOR + 40 * a + 8
        lowest = np.broadcast_to(base - a, ok.shape)                                      # Zw(-1): the hand-over value of "step 0"
        highest = 4 * (m * tile + base + (T_end + C2 - 1) * a) + 3
        assert (lowest[col] >= LO).all() and (highest[col] <= HI).all(), tile
        n += int(col.sum())
    assert n > 50000 and row_tiles and max(row_tiles) < 305
    # the table as the kernel fills it, at the two ends of what the column-drifted pass is given: no byte wraps
    for match, gg in ((61, -1), (0, -13), (20, 0), (1, -12)):
        assert max((w >> (8 * k)) & 0xFF for w in table(match, gg) for k in range(4)) == 4 * (match + 2 * -gg) + 1


def test_the_rule_sends_the_lin_match_64_edge_to_the_row_drifted_pass():
    """(62, -1, -1, -1) at tile 64 -- the `lin-match-64` edge of tests/scoring_edges.py, which tests/test_gpu_int16_edges.py
    runs -- is admitted by the guard and its byte would be 257; (61, -1, -1, -1) is the last that fits"""
    from scoring_edges import EDGES
    edge = next(e for e in EDGES if e.name == "lin-match-64")
    match, g = edge.last[0], edge.last[1]
    assert p16_lin_ok(edge.tile, *edge.last) and not lin_col_drift_ok(match, g) and 4 * (match + 2 * -g) + 1 == 257
    assert p16_lin_ok(edge.tile, 61, -1, -1, -1) and lin_col_drift_ok(61, -1) and 4 * (61 + 2) + 1 == 253
