"""The rule of gact_hip_pileup_variants and the line of gact_hip_format_vcf (include/gact_hip.h), restated in plain Python one
position at a time, from what the device has in front of it: the counts, the slot table, the sequences' own bytes and their
offsets.  No engine is involved: the CPU suite holds this model to literals worked out by hand (tests/test_variant_model.py),
the GPU suite holds the device to this model (tests/test_gpu_variants.py)."""
import numpy as np

from gact_amd import engine
from pileup_model import _KIND, DEL, DEPTH

DEFAULTS = dict(min_depth=8, min_alt=4, min_permille=250, hom_permille=750)
INS_KIND, DEL_KIND, SNV_KIND = 0, 1, 2
TRUNCATED = 4
_LETTERS = b"ACGT"


def check_params(min_depth, min_alt, min_permille, hom_permille):
    return min_depth >= 1 and min_alt >= 1 and 0 <= min_permille <= hom_permille <= 1000


def variants(counts, ins, own, offsets, seq_first=0, **params):
    """counts uint32 [positions, 8]; ins uint32 [positions, K, 4] or None (no slots); own uint8 [positions]; offsets [n + 1]:
    where the window's sequences begin in those arrays (offsets[0] == 0); seq_first: the first sequence's id.
    -> (records engine.VARIANT_DTYPE in the stated order, table engine.SEQ_VARIANTS_DTYPE [n])"""
    p = dict(DEFAULTS, **params)
    assert check_params(**p), p
    min_depth, min_alt, min_permille, hom_permille = (int(p[k]) for k in ("min_depth", "min_alt", "min_permille", "hom_permille"))
    K = 0 if ins is None else ins.shape[1]

    def qualifies(a, d):
        return a >= min_alt and 1000 * a >= min_permille * d

    def gt(a, d):
        return 2 if 1000 * a >= hom_permille * d else 1

    out = []
    n_seqs = len(offsets) - 1
    table = np.zeros(n_seqs, dtype=engine.SEQ_VARIANTS_DTYPE)
    for i in range(n_seqs):
        table["first"][i] = len(out)
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        run = None                                      # the open deletion run's record
        for x in range(hi - lo):
            n = [int(v) for v in counts[lo + x]]
            d = n[DEPTH]
            if d < min_depth:
                run = None
                continue
            table["examined"][i] += 1
            if K:
                s = [int(ins[lo + x, j].sum()) for j in range(K)]
                if qualifies(s[0], d):
                    length = 0
                    while length < K and qualifies(s[length], d):
                        length += 1
                    bases = 0
                    for j in range(length):
                        bases |= _LETTERS[int(np.argmax(ins[lo + x, j]))] << (8 * j)        # (argmax: the first of equal ones)
                    out.append((seq_first + i, x, INS_KIND, length, bases, s[0], d, gt(s[0], d) | (TRUNCATED if length == K else 0)))
                    table["n_ins"][i] += 1
            if qualifies(n[DEL], d):
                if run is None:
                    run = [seq_first + i, x, DEL_KIND, 0, 0, n[DEL], d, gt(n[DEL], d)]
                    out.append(run)
                    table["n_del"][i] += 1
                run[3] += 1
            else:
                run = None
            mine = int(_KIND[own[lo + x]])
            if mine < 4:
                for b in range(4):
                    if b != mine and qualifies(n[b], d):
                        out.append((seq_first + i, x, SNV_KIND, 1, _LETTERS[b], n[b], d, gt(n[b], d)))
                        table["n_snv"][i] += 1
    records = np.array([tuple(r) for r in out], dtype=engine.VARIANT_DTYPE) if out else np.zeros(0, dtype=engine.VARIANT_DTYPE)
    return records, table


def stats_of(table):
    """what gact_hip_last_variant_stats counts, from the table"""
    return {k: int(table[k].sum()) for k in ("examined", "n_ins", "n_del", "n_snv")}


def _ref(b):
    c = chr(int(b) & ~0x20)
    return c if c in "ACGT" else "N"


def format_vcf(v, name, seq):
    """the VCF line of one record on its sequence (bytes or uint8), "" for a deletion of the whole sequence"""
    seq = np.frombuffer(bytes(seq), dtype=np.uint8)
    pos, length, kind = int(v["pos"]), int(v["len"]), int(v["kind"])
    if kind == SNV_KIND:
        at, ref, alt = pos, _ref(seq[pos]), chr(int(v["bases"]) & 0xff)
    elif kind == DEL_KIND:
        if pos == 0 and length == len(seq):
            return ""
        if pos > 0:
            at, ref, alt = pos - 1, "".join(_ref(b) for b in seq[pos - 1:pos + length]), _ref(seq[pos - 1])
        else:
            at, ref, alt = 0, "".join(_ref(b) for b in seq[:length + 1]), _ref(seq[length])
    else:
        bases = "".join(chr((int(v["bases"]) >> (8 * j)) & 0xff) for j in range(length))
        at = pos - 1 if pos > 0 else 0
        ref = _ref(seq[at])
        alt = ref + bases if pos > 0 else bases + ref
    return "%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AD=%d\tGT\t%s\n" % (name, at + 1, ref, alt, int(v["depth"]), int(v["alt"]),
                                                             "1/1" if int(v["flags"]) & 3 == 2 else "0/1")
