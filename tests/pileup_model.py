"""The rule of gact_hip_pileup_begin / _add / _finish (include/gact_hip.h), restated in numpy one column at a time: every
record's alignment stacked on its target read, the counts of every position, the consensus byte and the per-read table.
No engine is involved: the CPU suite holds this model to literals worked out by hand (tests/test_pileup_model.py), the GPU
suite holds the device to this model (tests/test_gpu_pileup.py)."""
import re

import numpy as np

from gact_amd import engine

A, C, G, T, OTHER, DEL, INS, DEPTH = range(8)
_KIND = np.full(256, OTHER, dtype=np.int64)
for _k, _pair in enumerate((b"aA", b"cC", b"gG", b"tT")):
    for _b in _pair:
        _KIND[_b] = _k
_LETTER = b"ACGT-"
_CIGAR = re.compile(r"(\d+)([=XID])")


def columns(cigar_or_ops):
    """a CIGAR string or op words (len << 4 | op) -> the column letters, one per column"""
    if isinstance(cigar_or_ops, str):
        assert _CIGAR.sub("", cigar_or_ops) == "", cigar_or_ops
        return "".join(op * int(n) for n, op in _CIGAR.findall(cigar_or_ops))
    return "".join(engine._OP_CHARS[int(w) & 15] * (int(w) >> 4) for w in cigar_or_ops)


def call(n, own, min_depth):
    """the consensus byte of a position with the counts n[8] whose read has the byte `own` there"""
    if n[DEPTH] < min_depth:
        return own
    five = [int(n[k]) for k in (A, C, G, T, DEL)]
    best = max(five)
    if best == 0:
        return own
    mine = int(_KIND[own])
    if mine < 4 and five[mine] == best:
        return _LETTER[mine]
    return _LETTER[five.index(best)]


def pileup(reads, rc_reads, records, cigars_or_ops, window, min_depth):
    """reads: the sequences (uint8 arrays or bytes), ref and forward query alike; rc_reads: the reverse-complement strand's
    queries (rc_reads[i] for query_id i; only looked at for comp == 1 records); records: ref_id, query_id, ae, be, comp,
    emitted (engine.OVERLAP_DTYPE or dicts); cigars_or_ops[k]: record k's alignment, a CIGAR string or op words; window:
    (read_first, n_reads).  -> (counts uint32 [positions, 8], consensus uint8 [positions], engine.READ_PILEUP_DTYPE [n_reads]),
    the window's positions read after read"""
    first, n_reads = window
    lens = [len(reads[first + i]) for i in range(n_reads)]
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    counts = np.zeros((int(start[-1]), 8), dtype=np.uint32)
    table = np.zeros(n_reads, dtype=engine.READ_PILEUP_DTYPE)
    assert len(records) == len(cigars_or_ops)
    for rec, path in zip(records, cigars_or_ops):
        rid, qid = int(rec["ref_id"]), int(rec["query_id"])
        if not (first <= rid < first + n_reads) or not int(rec["emitted"]):
            continue
        cols = columns(path)
        if not cols:
            continue
        query = np.frombuffer(bytes(rc_reads[qid] if int(rec["comp"]) else reads[qid]), dtype=np.uint8)
        length = lens[rid - first]
        r = int(rec["ae"]) - sum(c != "I" for c in cols)
        q = int(rec["be"]) - sum(c != "D" for c in cols)
        assert 0 <= r and int(rec["ae"]) <= length and 0 <= q and int(rec["be"]) <= len(query), (rec, len(cols))
        mine = counts[start[rid - first]:start[rid - first + 1]]
        prev = None
        for c in cols:
            if c == "I":
                if prev != "I":
                    mine[min(r, length - 1), INS] += 1
                q += 1
            elif c == "D":
                mine[r, DEL] += 1
                mine[r, DEPTH] += 1
                r += 1
            else:
                mine[r, _KIND[query[q]]] += 1
                mine[r, DEPTH] += 1
                r += 1
                q += 1
            prev = c
        assert r == int(rec["ae"]) and q == int(rec["be"])
        table["n_alignments"][rid - first] += 1
    own = (np.concatenate([np.frombuffer(bytes(reads[first + i]), dtype=np.uint8) for i in range(n_reads)])
           if n_reads else np.zeros(0, dtype=np.uint8))
    consensus = consensus_of(counts, own, min_depth)
    depth, called = counts[:, DEPTH], counts[:, DEPTH] >= min_depth
    deleted = called & (consensus == ord("-"))
    changed = called & ~deleted & ((consensus | 0x20) != (own | 0x20))
    flagged = called & (2 * counts[:, INS].astype(np.int64) > depth)
    for i in range(n_reads):
        part = slice(int(start[i]), int(start[i + 1]))
        table["max_depth"][i] = int(depth[part].max()) if lens[i] else 0
        for name, mask in (("called", called), ("changed", changed), ("deleted", deleted), ("ins_flagged", flagged)):
            table[name][i] = int(mask[part].sum())
    return counts, consensus, table


def consensus_of(counts, own, min_depth):
    """call() at every position at once: counts [positions, 8], own uint8 [positions] -> uint8 [positions]"""
    five = counts[:, [A, C, G, T, DEL]].astype(np.int64)
    if len(five) == 0:
        return np.zeros(0, dtype=np.uint8)
    best = five.max(axis=1)
    pick = five.argmax(axis=1)                          # (the first of equal ones: the order A C G T DEL)
    mine = _KIND[own]
    own_tied = (mine < 4) & (five[np.arange(len(five)), np.minimum(mine, 3)] == best)
    pick = np.where(own_tied, mine, pick)
    made = np.frombuffer(_LETTER, dtype=np.uint8)[pick]
    return np.where((counts[:, DEPTH] < min_depth) | (best == 0), own, made).astype(np.uint8)
