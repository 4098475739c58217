"""The look-up words of the split linear-gap pass (csrc/gact_lin.hpp 8., lin_lut_fill in csrc/gact_p16.hpp), modelled in numpy.

The pass used to make a row's word with a shift by the row's stream byte a: dsub >> (a & 31) on plain scores and
(dsub4 >> (a & 31)) + 0x01010101 in the pointer phase.  It now reads the word from a table whose byte offset is the stream
byte.  For every linear scoring the guard admits and every byte the loader writes, the table must hold what the shifts
gave.

One-instruction forms of the pointer phase's word that do not work, kept here because the first of them is the obvious
one: a 64-bit window {0x01010101, dsub4 + 0x01010101} >> (a & 31) (v_alignbit_b32) is right for the four real rows and
gives 0x02020202 for a pad row at any pad byte -- the five rows would need five byte-aligned windows and 32 bits hold
four."""
import numpy as np

TILES = (64, 128, 200, 320)
K_GROUP, K_LIN_FLOOR = 16, 1024
REAL_ROWS = (0, 8, 16, 24)                 # 24 - 8 * code, the loader's byte of a row inside the tile
OLD_PAD, LIN_PAD = 31, 32                  # kLutPadRow (every other pass), kLinPadRow (the split linear-gap pass)
ONES = 0x01010101


def p16_lin_ok(tile, match, mismatch, gap_open, ext):
    """csrc/gact_lin.hpp p16_lin_ok and csrc/gact_p16.hpp p16_tagged_ok, restated"""
    steps = tile + 4 * K_GROUP + 64 + 48
    tagged = match * (tile + 2) <= 7900 and match - mismatch <= 63 and mismatch >= -1000 and gap_open >= -1000 and ext >= -1000
    return (gap_open == ext and mismatch == ext and ext <= 0 and match >= 0 and tagged and
            4 * (match * (tile + 2) + (-ext) * steps + K_LIN_FLOOR) + 3 <= 30000 and match - ext <= 63)


def admitted(tile):
    return [(m, g) for g in range(0, -64, -1) for m in range(0, 128) if p16_lin_ok(tile, m, g, g, g)]


def table(match, mismatch):
    """lin_lut_fill: word 2 k of the row with stream byte 8 k on plain scores, word 2 k + 1 in the pointer phase"""
    dsub = np.uint32((match - mismatch) << 24)
    dsub4 = np.uint32((4 * (match - mismatch)) << 24)
    words = np.zeros(10, dtype=np.uint32)
    for tid in range(10):
        b = 8 * (tid >> 1)
        base = dsub4 if tid & 1 else dsub
        words[tid] = (int(base) >> b if b < LIN_PAD else 0) + (ONES if tid & 1 else 0)
    return words


def word(words, stream_byte, pointer_phase):
    assert stream_byte % 4 == 0 and stream_byte + 4 * pointer_phase + 4 <= 4 * len(words)     # an aligned read inside the table
    return int(words[stream_byte // 4 + pointer_phase])


def test_guard_model_agrees_with_the_table_of_edges():
    from scoring_edges import EDGES
    for e in EDGES:
        if e.guard == "p16_lin_ok":
            assert p16_lin_ok(e.tile, *e.last) and not p16_lin_ok(e.tile, *e.past), e.name


def test_table_words_are_what_the_shifts_gave():
    n = 0
    for tile in TILES:
        for match, g in admitted(tile):
            d = match - g
            dsub, dsub4 = (d << 24) & 0xffffffff, ((4 * d) << 24) & 0xffffffff
            assert 4 * d + 1 <= 255                                      # the pointer phase's byte fits
            w = table(match, g)
            for a in REAL_ROWS:
                assert word(w, a, 0) == dsub >> (a & 31)
                assert word(w, a, 1) == ((dsub4 >> (a & 31)) + ONES) & 0xffffffff
                # one byte per row: match - mismatch (times four, plus one) at the code's place, 0 (1) elsewhere
                code = (24 - a) // 8
                assert [(word(w, a, 0) >> (8 * k)) & 0xff for k in range(4)] == [d if k == code else 0 for k in range(4)]
                assert [(word(w, a, 1) >> (8 * k)) & 0xff for k in range(4)] == [4 * d + 1 if k == code else 1 for k in range(4)]
            # a pad row: no bonus in any column.  The shift by 31 gave the same wherever bit 31 of dsub4 is clear -- at
            # every scoring admitted at tile 320 -- and a stray 1 in byte 0 above that
            assert word(w, LIN_PAD, 0) == 0 == dsub >> OLD_PAD
            assert word(w, LIN_PAD, 1) == ONES
            if 4 * d < 128:
                assert word(w, LIN_PAD, 1) == (dsub4 >> OLD_PAD) + ONES
            n += 1
    assert n > 1000
    assert all(4 * (m - g) < 128 for m, g in admitted(320))


def test_no_64_bit_window_serves_the_pad_row():
    """the v_alignbit_b32 form: right for the real rows, 2 in every byte of a pad row"""
    for match, g in ((1, -1), (18, -1), (20, 0)):
        d4 = 4 * (match - g)
        lo, hi = ((d4 << 24) + ONES) & 0xffffffff, ONES
        window = lambda a: (((hi << 32) | lo) >> (a & 31)) & 0xffffffff
        for a in REAL_ROWS:
            assert window(a) == (((d4 << 24) & 0xffffffff) >> a) + ONES
        assert window(OLD_PAD) & 0xfefefefe == 0x02020202
