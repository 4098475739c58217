"""A Python restatement of GACT's tile chain (gact.cpp:82-195) that keeps what the reference builds and throws away: the
alignment, one column per state, as the CIGAR ops gact_hip_candidates_paths returns.  `align` is any AlignWithBT with the
signature of oracle_py.Oracle.align_with_bt (the oracle's, or the reference's own through oracle_py.RefLib)."""
import numpy as np

from gact_amd import engine

STATE_D, STATE_I, STATE_M = 1, 2, 3          # align.h:23


def columns_to_ops(cols):
    """column codes (engine.OP_*) -> op words len << 4 | op"""
    ops = []
    for c in cols:
        if ops and (ops[-1] & 15) == c:
            ops[-1] += 1 << 4
        else:
            ops.append((1 << 4) | c)
    return np.array(ops, dtype=np.uint32)


def gact_path(align, ref, query, ref_pos, query_pos, tile_size=320, tile_overlap=120, threshold=35,
              scoring=(1, -1, -1, -1)):
    """-> dict(ab, ae, bb, be, score, first_tile_score, n_tiles, cols, ops, tiles); tiles: one tuple per AlignWithBT call,
    (ref_off, query_off, ref_len, query_len, reverse, first, tile_score, max_i, max_j, n_states, i_steps, j_steps) as
    oracle_py.TileTrace records it"""
    ref, query = bytes(ref), bytes(query)
    early = tile_size - tile_overlap
    left, right, tiles = [], [], []            # left: columns right to left
    rev_ref_pos, rev_query_pos = ref_pos, query_pos
    i = j = 0
    first_tile, first_tile_score = True, 0

    def consume(q, k, out, r_at, q_at):
        nonlocal i, j, first_tile
        for st in q[k:]:
            first_tile = False
            if st == STATE_M:
                out.append(engine.OP_EQ if ref[r_at(j)] == query[q_at(i)] else engine.OP_X)
                i += 1
                j += 1
            elif st == STATE_I:                     # '-' in the query: a ref base, SAM's D
                out.append(engine.OP_D)
                j += 1
            elif st == STATE_D:                     # '-' in the ref: a query base, SAM's I
                out.append(engine.OP_I)
                i += 1

    while ref_pos > 0 and query_pos > 0 and ((i > 0 and j > 0) or first_tile):          # :82
        rl, ql = min(ref_pos, tile_size), min(query_pos, tile_size)
        q = align(ref[ref_pos - rl:ref_pos], query[query_pos - ql:query_pos], scoring=scoring, reverse=False,
                  first=first_tile, early_terminate=early)
        tr = [ref_pos - rl, query_pos - ql, rl, ql, 0, int(first_tile), q[0], 0, 0]
        i = j = 0
        k, stop = 1, False
        if first_tile:                                                                    # :99-110
            tr[7], tr[8] = q[1], q[2]
            ref_pos, query_pos = ref_pos - rl + q[1], query_pos - ql + q[2]
            rev_ref_pos, rev_query_pos = ref_pos, query_pos
            first_tile_score = q[0]
            k = 3
            stop = q[0] < threshold
        if not stop:
            rp, qp = ref_pos, query_pos
            consume(q, k, left, lambda jj: rp - jj - 1, lambda ii: qp - ii - 1)
            ref_pos -= j
            query_pos -= i
        tiles.append(tuple(tr + [0 if stop else len(q) - k, i, j]))
        if stop:
            break
    ab, bb = ref_pos, query_pos                                                            # :136-141
    ref_pos, query_pos = rev_ref_pos, rev_query_pos
    i = j = tile_size
    while ref_pos < len(ref) and query_pos < len(query) and ((i > 0 and j > 0) or first_tile):   # :144
        rl = tile_size if ref_pos + tile_size < len(ref) else len(ref) - ref_pos
        ql = tile_size if query_pos + tile_size < len(query) else len(query) - query_pos
        q = align(ref[ref_pos:ref_pos + rl], query[query_pos:query_pos + ql], scoring=scoring, reverse=True,
                  first=first_tile, early_terminate=early)
        tr = [ref_pos, query_pos, rl, ql, 1, int(first_tile), q[0], 0, 0]
        i = j = 0
        k, stop = 1, False
        if first_tile:                                                                    # :162-171
            tr[7], tr[8] = q[1], q[2]
            ref_pos, query_pos = ref_pos + rl - q[1], query_pos + ql - q[2]
            first_tile_score = q[0]
            k = 3
            stop = q[0] < threshold
        if not stop:
            rp, qp = ref_pos, query_pos
            consume(q, k, right, lambda jj: rp + jj, lambda ii: qp + ii)
            ref_pos += j
            query_pos += i
        tiles.append(tuple(tr + [0 if stop else len(q) - k, i, j]))
        if stop:
            break
    cols = left[::-1] + right
    ops = columns_to_ops(cols)
    return dict(ab=ab, ae=ref_pos, bb=bb, be=query_pos, score=engine.rescore(ops, scoring),
                first_tile_score=first_tile_score, n_tiles=len(tiles), cols=cols, ops=ops, tiles=tiles,
                left_aligned=len(left) > 0)


def check_path(rec, ops, n_columns, ref, query, scoring, left_aligned=None):
    """the invariants every path must satisfy against its own record and the two reads (query: the strand the record's
    coordinates refer to).  The ops end at (ae, be).  They start at (ab, bb) whenever the left extension aligned anything;
    where it aligned nothing (its first tile under the threshold, or a hit at position 0) the right extension's first tile
    moved the start to its arg-max (gact.cpp:162-166) and ab / bb stay where the left one stopped (:136-137).  Returns
    whether the path spans [ab, ae) x [bb, be) exactly.  left_aligned (known to the model): that must then hold."""
    ops = np.asarray(ops, dtype=np.uint32)
    lens, codes = ops >> 4, ops & 15
    assert int(lens.sum()) == n_columns
    assert np.all(lens > 0)
    assert np.all(codes[1:] != codes[:-1]), "adjacent ops of one kind"
    r_used = int(lens[(codes == engine.OP_EQ) | (codes == engine.OP_X) | (codes == engine.OP_D)].sum())
    q_used = int(lens[(codes == engine.OP_EQ) | (codes == engine.OP_X) | (codes == engine.OP_I)].sum())
    exact = r_used == rec["ae"] - rec["ab"] and q_used == rec["be"] - rec["bb"]
    if left_aligned:
        assert exact, (r_used, q_used, rec)
    assert 0 <= r_used <= rec["ae"] - rec["ab"] and 0 <= q_used <= rec["be"] - rec["bb"], (r_used, q_used, rec)
    assert engine.rescore(ops, scoring) == rec["score"]
    # every = / X column against the bases it stands on (column by column, vectorised)
    cols = np.repeat(codes, lens.astype(np.int64))
    diag = (cols == engine.OP_EQ) | (cols == engine.OP_X)
    r_at = int(rec["ae"]) - r_used + np.cumsum(diag | (cols == engine.OP_D)) - 1
    q_at = int(rec["be"]) - q_used + np.cumsum(diag | (cols == engine.OP_I)) - 1
    ref, query = np.asarray(ref, dtype=np.uint8), np.asarray(query, dtype=np.uint8)
    same = ref[r_at[diag]] == query[q_at[diag]]
    assert np.array_equal(same, cols[diag] == engine.OP_EQ), "an =/X column disagrees with its bases"
    return exact
