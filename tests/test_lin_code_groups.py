"""The byte groups of the split linear-gap pass (csrc/gact_lin.hpp 9.), modelled in numpy.

Inside a whole flush block the pass files the 2-bit op codes of two adjacent region-2 columns at once: a v_perm_b32 gathers
the low bytes of the pair's two H'' (tile A in the low half-word, tile B in the high one), a v_and_b32 keeps the four tags,
and a register takes four steps, a byte per (column, tile), with v_pk_mad_u16 x 4 on its half-words.  The flush builds
the stored words with one v_perm_b32 per pair and tile.  Whatever the codes, the words must be those of the scheme the
remainder steps still use and LinWords documents: a half-word holds eight steps of one column with the first step on top,
a dword two adjacent columns with the even one low; the 13th column keeps that scheme and has the dword to itself."""
import numpy as np

C2, STEPS = 13, 8
PAIR_SEL, PAIR_MASK = 0x06020400, 0x03030303          # kLinPairSel, kLinPairMask
FLUSH_SEL_A, FLUSH_SEL_B = 0x05010400, 0x07030602     # kLinFlushSelA, kLinFlushSelB
HALF_SEL_A, HALF_SEL_B = 0x05040100, 0x07060302       # lin_flush's selectors (the unpaired column, and the present scheme)
M32 = 0xffffffff


def v_perm(s0, s1, sel):
    """v_perm_b32 / __builtin_amdgcn_perm(s0, s1, sel): selector bytes 0-3 take bytes of s1, 4-7 bytes of s0"""
    src = [(s1 >> (8 * k)) & 0xff for k in range(4)] + [(s0 >> (8 * k)) & 0xff for k in range(4)]
    out = 0
    for k in range(4):
        s = (sel >> (8 * k)) & 0xff
        assert s < 8                                   # (the constant and sign selectors are not used)
        out |= src[s] << (8 * k)
    return out


def pk_mad4(a, c):
    """v_pk_mad_u16 a, 4, c: each half-word a * 4 + c, wrapping"""
    lo = ((a & 0xffff) * 4 + (c & 0xffff)) & 0xffff
    hi = ((a >> 16) * 4 + (c >> 16)) & 0xffff
    return lo | (hi << 16)


def tagged_scores(rng, codes):
    """H'' of one step as the pass holds it: tile A's 4 H + op in the low half-word, tile B's in the high one"""
    h = rng.integers(0x0400, 0x1d00, size=codes.shape[:1] + (2,)) * 4 + codes
    return [int(a) | (int(b) << 16) for a, b in h]


def present_words(codes):
    """the words of the half-word scheme: codes[step][column][tile] -> (tile A's dwords, tile B's dwords)"""
    acc = [0] * (C2 + 1)
    for s in range(STEPS):
        for c in range(C2):
            acc[c] = pk_mad4(acc[c], int(codes[s, c, 0]) | (int(codes[s, c, 1]) << 16))
    nw = (C2 + 1) // 2
    return ([v_perm(acc[2 * n + 1], acc[2 * n], HALF_SEL_A) for n in range(nw)],
            [v_perm(acc[2 * n + 1], acc[2 * n], HALF_SEL_B) for n in range(nw)])


def group_words(rng, codes):
    """the same words from the byte groups, instruction by instruction"""
    npair = C2 // 2
    grp = [None] * (2 * npair)                          # nothing may read a group before its first step has written it
    odd = None
    for s in range(STEPS):
        hp = tagged_scores(rng, codes[s])
        for p in range(npair):
            x = v_perm(hp[2 * p + 1], hp[2 * p], PAIR_SEL) & PAIR_MASK
            r = 2 * p + (s >> 2)
            grp[r] = x if s & 3 == 0 else pk_mad4(grp[r], x)
        t = hp[C2 - 1] & 0x00030003
        odd = t if s == 0 else pk_mad4(odd, t)
    wa = [v_perm(grp[2 * p], grp[2 * p + 1], FLUSH_SEL_A) for p in range(npair)] + [v_perm(0, odd, HALF_SEL_A)]
    wb = [v_perm(grp[2 * p], grp[2 * p + 1], FLUSH_SEL_B) for p in range(npair)] + [v_perm(0, odd, HALF_SEL_B)]
    return wa, wb


def documented_words(codes, tile):
    """LinWords, restated without either scheme: half-word = eight steps of a column, first on top; dword = two columns, even low"""
    words = []
    for n in range((C2 + 1) // 2):
        w = 0
        for half, c in enumerate((2 * n, 2 * n + 1)):
            if c < C2:
                hw = 0
                for s in range(STEPS):
                    hw |= int(codes[s, c, tile]) << (2 * (STEPS - 1 - s))
                w |= hw << (16 * half)
        words.append(w)
    return words


def test_group_words_equal_the_present_scheme():
    rng = np.random.default_rng(7)
    for _ in range(400):
        codes = rng.integers(0, 4, size=(STEPS, C2, 2))
        wa, wb = group_words(rng, codes)
        pa, pb = present_words(codes)
        assert wa == pa and wb == pb
        assert wa == documented_words(codes, 0) and wb == documented_words(codes, 1)


def test_extreme_codes_do_not_cross_bytes():
    """all threes in one (column, tile) and zeros beside it, and the other way round: a byte never reaches its neighbour"""
    rng = np.random.default_rng(8)
    for c in range(C2):
        for tile in range(2):
            for fill in (0, 3):
                codes = np.full((STEPS, C2, 2), fill)
                codes[:, c, tile] = 3 - fill
                wa, wb = group_words(rng, codes)
                assert wa == documented_words(codes, 0) and wb == documented_words(codes, 1)


def test_a_single_code_lands_at_its_place():
    """one code 1, 2 or 3 at one (step, column, tile), zeros elsewhere"""
    rng = np.random.default_rng(9)
    for s in range(STEPS):
        for c in range(C2):
            for tile in range(2):
                codes = np.zeros((STEPS, C2, 2), dtype=np.int64)
                codes[s, c, tile] = 1 + (s + c) % 3
                w = group_words(rng, codes)
                want = [0] * ((C2 + 1) // 2)
                want[c // 2] = int(codes[s, c, tile]) << (16 * (c & 1) + 2 * (STEPS - 1 - s))
                assert w[tile] == want and w[1 - tile] == [0] * len(want)
