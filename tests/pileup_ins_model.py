"""The rule of gact_hip_pileup_begin_ins / gact_hip_pileup_corrected (include/gact_hip.h), restated in numpy: the inserted
bases counted one column at a time into the slots in front of every position, the slot call, and the corrected reads spelled
from the emitted slots and the consensus.  The counts and the consensus byte are tests/pileup_model.py's, unchanged.  No engine
is involved: the CPU suite holds this model to literals worked out by hand and to the simulator's truth
(tests/test_pileup_ins_model.py), the GPU suite holds the device to this model (tests/test_gpu_pileup_ins.py)."""
import numpy as np

from gact_amd import engine
from pileup_model import _KIND, DEPTH, columns, pileup

MAX_INS_SLOTS = 4


def slot_counts(reads, rc_reads, records, cigars_or_ops, window, ins_slots):
    """-> (ins uint32 [positions, ins_slots, 4], runs_truncated): the j-th column of a run of 'I' in front of target position r
    adds 1 to ins[r, j, kind of its query byte] if j < ins_slots, r < len and the kind is A C G T; a run longer than
    ins_slots counts once in runs_truncated, wherever it stands"""
    first, n_reads = window
    lens = [len(reads[first + i]) for i in range(n_reads)]
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ins = np.zeros((int(start[-1]), ins_slots, 4), dtype=np.uint32)
    runs_truncated = 0
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
        mine = ins[start[rid - first]:start[rid - first + 1]]
        j = 0                                               # this column's index inside its run of 'I'
        for c in cols:
            if c == "I":
                kind = int(_KIND[query[q]])
                if j < ins_slots and r < length and kind < 4:
                    mine[r, j, kind] += 1
                if j == ins_slots:
                    runs_truncated += 1
                j += 1
                q += 1
            else:
                j = 0
                r += 1
                q += c != "D"
    return ins, runs_truncated


def slot_calls(counts, ins, min_depth):
    """-> (emitted bool [positions, K], byte uint8 [positions, K]): slot j of position p is emitted iff p is called, every slot
    below j at p is emitted and 2 * (the slot's four counts) > the depth at p; its byte is the largest count's, the first of
    equal ones in the order A C G T"""
    depth = counts[:, DEPTH].astype(np.int64)
    called = depth >= min_depth
    passes = 2 * ins.astype(np.int64).sum(axis=2) > depth[:, None]
    emitted = np.logical_and.accumulate(passes, axis=1) & called[:, None]
    byte = np.frombuffer(b"ACGT", dtype=np.uint8)[ins.argmax(axis=2)]
    return emitted, byte


def pileup_ins(reads, rc_reads, records, cigars_or_ops, window, min_depth, ins_slots):
    """the arguments of pileup_model.pileup and ins_slots -> (ins uint32 [positions, ins_slots, 4], table
    engine.READ_CORRECTED_DTYPE [n_reads], read_at int64 [n_reads + 1], seq bytes, runs_truncated): for every position in
    order its emitted slot bytes, then its consensus byte unless that is '-'"""
    assert 0 <= ins_slots <= MAX_INS_SLOTS
    first, n_reads = window
    counts, consensus, _ = pileup(reads, rc_reads, records, cigars_or_ops, window, min_depth)
    ins, runs_truncated = slot_counts(reads, rc_reads, records, cigars_or_ops, window, ins_slots)
    emitted, byte = slot_calls(counts, ins, min_depth)
    own = (np.concatenate([np.frombuffer(bytes(reads[first + i]), dtype=np.uint8) for i in range(n_reads)])
           if n_reads else np.zeros(0, dtype=np.uint8))
    kept = consensus != ord("-")
    called = counts[:, DEPTH] >= min_depth
    changed = called & kept & ((consensus | 0x20) != (own | 0x20))
    # a position's bytes: its slots, then its consensus byte -- row after row of [positions, K + 1] under the mask
    cells = np.concatenate([byte, consensus[:, None]], axis=1)
    mask = np.concatenate([emitted, kept[:, None]], axis=1)
    per_position = mask.sum(axis=1).astype(np.int64)
    start = np.concatenate([[0], np.cumsum([len(reads[first + i]) for i in range(n_reads)])]).astype(np.int64)
    table = np.zeros(n_reads, dtype=engine.READ_CORRECTED_DTYPE)
    read_at = np.zeros(n_reads + 1, dtype=np.int64)
    for i in range(n_reads):
        part = slice(int(start[i]), int(start[i + 1]))
        table["length"][i] = int(per_position[part].sum())
        table["inserted"][i] = int(emitted[part].sum())
        table["ins_sites"][i] = int(emitted[part].any(axis=1).sum()) if ins_slots else 0
        table["deleted"][i] = int((~kept[part]).sum())
        table["changed"][i] = int(changed[part].sum())
        read_at[i + 1] = read_at[i] + int(table["length"][i])
    return ins, table, read_at, cells[mask].tobytes(), runs_truncated
