"""ctypes binding of the C-ABI in include/gact_hip.h (libgact_hip.so).

Plumbing only: numpy arrays in, numpy arrays out.  Fails loudly when the HIP
library is missing or no device is present -- there is no CPU fallback.
"""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # darwin-gpu_amd/
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.path.join(_PKG, "libgact_hip.so")
# gact_engine.hip (the one translation unit, first) and every header under csrc/: none can be left out of the staleness check
SOURCES = sorted(glob.glob(os.path.join(_PKG, "csrc", "*.hip"))) + sorted(glob.glob(os.path.join(_PKG, "csrc", "*.hpp"))) + \
          [os.path.join(_ROOT, "include", "gact_hip.h")]

SET_REF, SET_QUERY, SET_QUERY_RC = 0, 1, 2
STATE_Z, STATE_D, STATE_I, STATE_M = 0, 1, 2, 3

TILE_DTYPE = np.dtype([("ref_id", "<i4"), ("query_id", "<i4"), ("ref_off", "<i4"), ("query_off", "<i4"),
                       ("ref_len", "<i4"), ("query_len", "<i4"),
                       ("reverse", "u1"), ("first", "u1"), ("query_set", "u1"), ("pad", "u1")])
TILE_RESULT_DTYPE = np.dtype([(n, "<i4") for n in
                              ("score", "max_i", "max_j", "ref_steps", "query_steps", "n_states")])
CAND_DTYPE = np.dtype([(n, "<i4") for n in ("ref_id", "query_id", "ref_pos", "query_pos")])
OVERLAP_DTYPE = np.dtype([(n, "<i4") for n in
                          ("ref_id", "query_id", "ab", "ae", "bb", "be", "score", "comp", "emitted",
                           "first_tile_score", "n_tiles", "reserved")] + [("cells", "<i8")])
assert TILE_DTYPE.itemsize == 28 and OVERLAP_DTYPE.itemsize == 56
PATH_DTYPE = np.dtype([("op_offset", "<i8"), ("n_ops", "<i4"), ("n_columns", "<i4")])
SUMMARY_DTYPE = np.dtype([(n, "<i4") for n in ("n_eq", "n_x", "ins_bases", "del_bases", "eq_runs", "x_runs", "ins_runs", "del_runs")])
assert SUMMARY_DTYPE.itemsize == 32
COVER_DTYPE = np.dtype([(n, "<i4") for n in ("n_intervals", "max_depth", "covered", "well_covered", "span_begin", "span_end")] +
                       [("depth_sum", "<i8")])
assert COVER_DTYPE.itemsize == 32
# the overlap graph (include/gact_hip.h gact_hip_overlap_graph): an arc u -> v of the bidirected graph, and the per-read table
GRAPH_ARC_DTYPE = np.dtype([(n, "<i4") for n in ("u", "v", "len", "ov_u", "ov_v", "record", "score", "flags")])
GRAPH_READ_DTYPE = np.dtype([(n, "<i4") for n in ("n_hits", "n_internal", "n_contains", "contained_by")] +
                            [("deg", "<i4", (2,)), ("kept", "<i4", (2,))])
assert GRAPH_ARC_DTYPE.itemsize == 32 and GRAPH_READ_DTYPE.itemsize == 32
GRAPH_NONE, GRAPH_SELF, GRAPH_DROPPED, GRAPH_INTERNAL, GRAPH_QUERY_CONTAINED, GRAPH_TARGET_CONTAINED, GRAPH_SHORT, \
    GRAPH_DOVETAIL = range(8)
# the unitigs of an overlap graph (include/gact_hip.h gact_hip_unitigs): a unitig, an entry of its layout, and where a read went
UNITIG_DTYPE = np.dtype([(n, "<i4") for n in ("first", "last", "n_reads", "circular")] +
                        [(n, "<i8") for n in ("layout_at", "seq_at", "length")])
UNITIG_ENTRY_DTYPE = np.dtype([("vertex", "<i4"), ("take", "<i4"), ("start", "<i8")])
UNITIG_PLACE_DTYPE = np.dtype([(n, "<i4") for n in ("unitig", "rank", "orient", "state")])
assert UNITIG_DTYPE.itemsize == 40 and UNITIG_ENTRY_DTYPE.itemsize == 16 and UNITIG_PLACE_DTYPE.itemsize == 16
UNITIG_PLACED, UNITIG_CONTAINED, UNITIG_EMPTY, UNITIG_TIP = range(4)
UNITIG_DEFAULT_TIP_READS = 3
# the bubbles of an overlap graph (include/gact_hip.h gact_hip_pop_bubbles): one record per bubble found
BUBBLE_DTYPE = np.dtype([(n, "<i4") for n in ("source", "sink", "n_vertices", "n_path", "n_removed", "state")] + [("path_len", "<i8")])
assert BUBBLE_DTYPE.itemsize == 32
BUBBLE_POPPED, BUBBLE_LOST = 0, 1
GRAPH_ARC_BUBBLE = 4
BUBBLE_DEFAULT_MAX_DIST = 50000
BUBBLE_MAX_VERTICES = 64
# the weak arcs and the cleaning rounds (include/gact_hip.h gact_hip_prune_overlaps, gact_hip_clean_graph): a step of the log, a read's state
GRAPH_ARC_TIP, GRAPH_ARC_SHORT = 8, 16
PRUNE_DEFAULT_RATIO_PERMILLE = 500
CLEAN_TIPS, CLEAN_BUBBLES, CLEAN_PRUNE = 0, 1, 2
CLEAN_KINDS = ("tips", "bubbles", "prune")
CLEAN_KEPT, CLEAN_BUBBLE = 0, 4                      # (states 1 .. 3 are UNITIG_CONTAINED, UNITIG_EMPTY, UNITIG_TIP)
CLEAN_STEP_DTYPE = np.dtype([(n, "<i4") for n in ("kind", "param", "reads_removed", "examined")] +
                            [(n, "<i8") for n in ("arcs_removed", "arcs_left")])
CLEAN_READ_DTYPE = np.dtype([("state", "<i4"), ("step", "<i4")])
assert CLEAN_STEP_DTYPE.itemsize == 32 and CLEAN_READ_DTYPE.itemsize == 8
# the placement of reads (include/gact_hip.h gact_hip_place_reads): one record per chosen record, one per read of the window
PLACE_DTYPE = np.dtype([(n, "<i4") for n in ("kind", "mapq", "parent", "rank")])
READ_PLACE_DTYPE = np.dtype([(n, "<i4") for n in ("n_records", "primary", "n_supplementary", "n_secondary", "n_extra", "score",
                                                  "second", "mapq")])
assert PLACE_DTYPE.itemsize == 16 and READ_PLACE_DTYPE.itemsize == 32
PLACE_NONE, PLACE_PRIMARY, PLACE_SUPPLEMENTARY, PLACE_SECONDARY, PLACE_EXTRA = range(5)
PLACE_MAX_PARENTS = 64
PLACE_DEFAULT_MASK_PERMILLE, PLACE_DEFAULT_MAPQ_CAP = 500, 60
# the kinds a position of a pileup counts (include/gact_hip.h GACT_PILEUP_*), and the per-read table of pileup_finish
PILEUP_A, PILEUP_C, PILEUP_G, PILEUP_T, PILEUP_OTHER, PILEUP_DEL, PILEUP_INS, PILEUP_DEPTH = range(8)
PILEUP_COL_DTYPE = np.dtype([("n", "<u4", (8,))])
READ_PILEUP_DTYPE = np.dtype([(n, "<i4") for n in ("n_alignments", "max_depth", "called", "changed", "deleted", "ins_flagged")] +
                             [("reserved", "<i4", (2,))])
assert PILEUP_COL_DTYPE.itemsize == 32 and READ_PILEUP_DTYPE.itemsize == 32
# the inserted bases in front of a position, per slot (gact_pileup_ins), and the per-read table of pileup_corrected
PILEUP_MAX_INS_SLOTS = 4
PILEUP_INS_DTYPE = np.dtype([("n", "<u4", (4,))])
READ_CORRECTED_DTYPE = np.dtype([(n, "<i4") for n in ("length", "inserted", "ins_sites", "deleted", "changed")] +
                                [("reserved", "<i4", (3,))])
assert PILEUP_INS_DTYPE.itemsize == 16 and READ_CORRECTED_DTYPE.itemsize == 32
# the variants of the pileup (include/gact_hip.h gact_hip_pileup_variants): one record per variant, one per sequence of the window
VARIANT_INS, VARIANT_DEL, VARIANT_SNV = range(3)
VARIANT_TRUNCATED = 4                                 # bit 2 of flags; the gt (1: 0/1, 2: 1/1) is flags & 3
VARIANT_CHUNK = 4096                                  # GACT_VARIANT_CHUNK: the positions one wave takes
VARIANT_DEFAULTS = dict(min_depth=8, min_alt=4, min_permille=250, hom_permille=750)       # GACT_VARIANT_DEFAULT_*
VARIANT_DTYPE = np.dtype([("seq", "<i4"), ("pos", "<i4"), ("kind", "<i4"), ("len", "<i4"), ("bases", "<u4"), ("alt", "<u4"),
                          ("depth", "<u4"), ("flags", "<i4")])
SEQ_VARIANTS_DTYPE = np.dtype([(n, "<i4") for n in ("examined", "n_ins", "n_del", "n_snv", "first")] + [("reserved", "<i4", (3,))])
assert VARIANT_DTYPE.itemsize == 32 and SEQ_VARIANTS_DTYPE.itemsize == 32

# alignment ops (include/gact_hip.h GACT_PATH_OP_*): BAM's CIGAR numbering; an op word is len << 4 | op
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
_OP_CHARS = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}


def cigar_string(ops):
    """op words (len << 4 | op) -> "153=1X2I..." """
    return "".join("%d%s" % (int(w) >> 4, _OP_CHARS[int(w) & 15]) for w in ops)


def summarise(ops):
    """op words -> one SUMMARY_DTYPE record: columns and ops of each kind (what gact_hip_candidates_summaries returns for the
    candidate whose ops these are, include/gact_hip.h gact_path_summary)"""
    s = np.zeros((), dtype=SUMMARY_DTYPE)
    cols = {OP_EQ: "n_eq", OP_X: "n_x", OP_I: "ins_bases", OP_D: "del_bases"}
    runs = {OP_EQ: "eq_runs", OP_X: "x_runs", OP_I: "ins_runs", OP_D: "del_runs"}
    for w in ops:
        n, op = int(w) >> 4, int(w) & 15
        s[cols[op]] += n
        s[runs[op]] += 1
    return s


def rescore(ops, scoring=(1, -1, -1, -1)):
    """the total score of gact.cpp:197-210 from op words: ONE `open` flag for both gap kinds, so an I run straight after a
    D run (or the other way round) goes on with the gap and is charged gap_extend"""
    match, mismatch, gap_open, gap_extend = scoring
    score, open_ = 0, True
    for w in ops:
        n, op = int(w) >> 4, int(w) & 15
        if op in (OP_I, OP_D):
            score += (gap_open if open_ else gap_extend) + (n - 1) * gap_extend
            open_ = False
        else:
            score += n * (match if op == OP_EQ else mismatch)
            open_ = True
    return score


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("tile_size", "tile_overlap", "match", "mismatch", "gap_open", "gap_extend",
                 "first_tile_score_threshold", "device_id", "n_slots", "max_blocks")]


class DeviceInfo(C.Structure):
    _fields_ = [("compute_units", C.c_int32), ("clock_mhz", C.c_int32), ("waves_per_cu", C.c_int32),
                ("wave_size", C.c_int32), ("hbm_bytes", C.c_int64), ("arch", C.c_char * 32)]


class RunStats(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("seed_ms", C.c_float), ("main_ms", C.c_float),
                ("packed16", C.c_int32), ("handed_off", C.c_int32), ("seed_packed16", C.c_int32),
                ("tagged_pointers", C.c_int32), ("linear_gap", C.c_int32), ("seed_cells", C.c_int64),
                ("raw_candidates", C.c_int32), ("band_redos", C.c_int32),
                ("merged_callers", C.c_int32), ("overlapped_seeding", C.c_int32),
                ("critical_lane", C.c_int32), ("role_waves", C.c_int32)]


class PathsStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("chunks", C.c_int32), ("column_bytes", C.c_int64), ("columns", C.c_int64),
                ("ops", C.c_int64)]


class SummariesStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("launches", C.c_int32), ("scratch_bytes", C.c_int64)]


class SelectStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("emitted", C.c_int32), ("selected", C.c_int32), ("table_slots", C.c_int64),
                ("scratch_bytes", C.c_int64)]


SELECT_EXACT, SELECT_PAIR = 0, 1
_SELECT_MODES = {"exact": SELECT_EXACT, "pair": SELECT_PAIR}


class CoverStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("reads", C.c_int32), ("intervals", C.c_int64), ("positions", C.c_int64),
                ("scratch_bytes", C.c_int64)]


class FilterParams(C.Structure):
    """the defaults are GACT_FILTER_DEFAULT_*"""
    _fields_ = [("min_identity_permille", C.c_int32), ("min_span", C.c_int32), ("max_drop_permille", C.c_int32)]


class FilterStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("reads", C.c_int32)] + \
               [(n, C.c_int64) for n in ("chosen", "counted", "kept", "not_emitted", "empty", "identity", "span", "relative",
                                         "scratch_bytes")]


# the filter of an overlap set (include/gact_hip.h gact_hip_filter_overlaps): one record per read of the window; why per record
FILTER_READ_DTYPE = np.dtype([(n, "<i4") for n in ("n_records", "n_passed", "n_kept", "best_permille")] +
                             [("eq_sum", "<i8"), ("col_sum", "<i8")])
assert FILTER_READ_DTYPE.itemsize == 32 and C.sizeof(FilterParams) == 12
FILTER_KEPT, FILTER_NOT_EMITTED, FILTER_EMPTY, FILTER_IDENTITY, FILTER_SPAN, FILTER_RELATIVE = range(6)
FILTER_DEFAULTS = {"min_identity": 650, "min_span": 0, "max_drop": 1000}


class PlaceParams(C.Structure):
    """the defaults are GACT_PLACE_DEFAULT_*"""
    _fields_ = [("mask_permille", C.c_int32), ("mapq_cap", C.c_int32)]


class PlaceStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("reads", C.c_int32), ("max_records", C.c_int32), ("reserved", C.c_int32),
                ("counted", C.c_int64), ("parents", C.c_int64), ("secondaries", C.c_int64), ("extras", C.c_int64),
                ("scratch_bytes", C.c_int64)]


class GraphParams(C.Structure):
    """the defaults are GACT_GRAPH_DEFAULT_*"""
    _fields_ = [(n, C.c_int32) for n in ("max_hang", "int_permille", "min_ovlp", "fuzz")]

    def __init__(self, max_hang=1000, int_permille=800, min_ovlp=1000, fuzz=1000):
        super().__init__(max_hang, int_permille, min_ovlp, fuzz)


class GraphStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("reads", C.c_int32), ("contained", C.c_int32), ("by_class", C.c_int64 * 8),
                ("proposed", C.c_int64), ("arcs", C.c_int64), ("transitive", C.c_int64), ("kept", C.c_int64),
                ("table_slots", C.c_int64), ("scratch_bytes", C.c_int64)]


class UnitigParams(C.Structure):
    """the default is GACT_UNITIG_DEFAULT_TIP_READS"""
    _fields_ = [("tip_reads", C.c_int32)]

    def __init__(self, tip_reads=UNITIG_DEFAULT_TIP_READS):
        super().__init__(tip_reads)


class UnitigStats(C.Structure):
    _fields_ = [("device_ms", C.c_float)] + \
               [(n, C.c_int32) for n in ("reads", "placed", "cut", "contained", "unitigs", "circular", "longest_reads", "rank_launches")] + \
               [(n, C.c_int64) for n in ("longest_bases", "e0_arcs", "e1_arcs", "joins", "links", "scratch_bytes")]


class BubbleParams(C.Structure):
    """the defaults are GACT_BUBBLE_DEFAULT_MAX_DIST and GACT_BUBBLE_MAX_VERTICES"""
    _fields_ = [("max_dist", C.c_int32), ("max_vertices", C.c_int32)]

    def __init__(self, max_dist=BUBBLE_DEFAULT_MAX_DIST, max_vertices=BUBBLE_MAX_VERTICES):
        super().__init__(max_dist, max_vertices)


class BubbleStats(C.Structure):
    _fields_ = [("device_ms", C.c_float)] + \
               [(n, C.c_int32) for n in ("reads", "sources", "found", "popped", "lost", "reads_removed")] + \
               [("working_arcs", C.c_int64), ("arcs_removed", C.c_int64), ("by_fail", C.c_int64 * 5), ("scratch_bytes", C.c_int64)]


class PruneParams(C.Structure):
    """the default is GACT_PRUNE_DEFAULT_RATIO_PERMILLE"""
    _fields_ = [("ratio_permille", C.c_int32)]

    def __init__(self, ratio_permille=PRUNE_DEFAULT_RATIO_PERMILLE):
        super().__init__(ratio_permille)


class PruneStats(C.Structure):
    _fields_ = [("device_ms", C.c_float)] + [(n, C.c_int32) for n in ("reads", "examined", "bared")] + \
               [(n, C.c_int64) for n in ("working_arcs", "weak", "arcs_removed", "scratch_bytes")]


class CleanParams(C.Structure):
    """the defaults are the ones gact_hip_clean_graph takes for NULL"""
    _fields_ = [(n, C.c_int32) for n in ("tip_reads", "max_dist", "max_vertices", "ratio_lo_permille", "ratio_hi_permille",
                                         "n_ratios", "max_passes")]

    def __init__(self, tip_reads=UNITIG_DEFAULT_TIP_READS, max_dist=BUBBLE_DEFAULT_MAX_DIST, max_vertices=BUBBLE_MAX_VERTICES,
                 ratio_lo_permille=500, ratio_hi_permille=700, n_ratios=3, max_passes=4):
        super().__init__(tip_reads, max_dist, max_vertices, ratio_lo_permille, ratio_hi_permille, n_ratios, max_passes)


class CleanStats(C.Structure):
    _fields_ = [("device_ms", C.c_float)] + [(n, C.c_int32) for n in ("reads", "steps", "passes", "reads_tip", "reads_bubble")] + \
               [("arcs_removed", C.c_int64 * 3), ("arcs_left", C.c_int64), ("scratch_bytes", C.c_int64)]


class PileupStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("adds", C.c_int32), ("chunks", C.c_int32), ("alignments", C.c_int64),
                ("columns", C.c_int64), ("positions", C.c_int64), ("scratch_bytes", C.c_int64)]


class PileupInsStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("ins_slots", C.c_int32), ("slot_adds", C.c_int64), ("runs_truncated", C.c_int64),
                ("emitted", C.c_int64), ("table_bytes", C.c_int64)]


class VariantParams(C.Structure):
    """the defaults are GACT_VARIANT_DEFAULT_*"""
    _fields_ = [(n, C.c_int32) for n in ("min_depth", "min_alt", "min_permille", "hom_permille")]


class VariantStats(C.Structure):
    _fields_ = [("device_ms", C.c_float), ("chunks", C.c_int32), ("n_ins", C.c_int64), ("n_del", C.c_int64), ("n_snv", C.c_int64),
                ("examined", C.c_int64), ("scratch_bytes", C.c_int64)]


COVER_REF, COVER_QUERY, COVER_BOTH = 1, 2, 3
_COVER_SIDES = {"ref": COVER_REF, "query": COVER_QUERY, "both": COVER_BOTH}


class DsoftParams(C.Structure):
    """params.cfg [DSOFT_params]; the defaults are the reference's"""
    _fields_ = [(n, C.c_int32) for n in ("seed_size", "bin_size", "window_size", "threshold", "num_seeds",
                                         "seed_occurence_multiple", "max_candidates")]

    def __init__(self, seed_size=14, bin_size=64, window_size=4, threshold=21, num_seeds=800,
                 seed_occurence_multiple=32, max_candidates=1000000):
        super().__init__(seed_size, bin_size, window_size, threshold, num_seeds, seed_occurence_multiple,
                         max_candidates)


class DsoftInfo(C.Structure):
    _fields_ = [("ref_length", C.c_int64), ("n_minimizers", C.c_int64), ("table_bytes", C.c_int64),
                ("pos_bytes", C.c_int64), ("max_occurrence", C.c_int32), ("n_bins", C.c_int32),
                ("build_ms", C.c_float)]


class GactHipError(RuntimeError):
    pass


def _ptr(a):
    return a.ctypes.data if a is not None else None


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -> darwin-gpu_amd/libgact_hip.so (in-tree)."""
    if not force and os.path.exists(LIB_PATH):
        newest = max(os.path.getmtime(s) for s in SOURCES)
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I" + os.path.join(_ROOT, "include"), "-o", LIB_PATH, SOURCES[0]]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


DRIVER_PATH = os.path.join(_PKG, "host", "darwin_hip")
DRIVER_SOURCES = [os.path.join(_PKG, "host", f) for f in
                  ("darwin_hip.cpp", "gact_shim.cpp", "dsoft.cpp", "gact.h", "align.h", "dsoft.h")]


def build_driver(force=False, verbose=False):
    """g++ -> darwin-gpu_amd/host/darwin_hip: the darwin.cpp-shaped driver + the gact.h/align.h shim"""
    build(force=force, verbose=verbose)
    if not force and os.path.exists(DRIVER_PATH):
        newest = max(os.path.getmtime(s) for s in DRIVER_SOURCES + [LIB_PATH])
        if os.path.getmtime(DRIVER_PATH) >= newest:
            return DRIVER_PATH
    cmd = ["g++", "-O2", "-std=c++14", "-pthread", "-I" + os.path.join(_ROOT, "include"),
           "-I" + os.path.join(_PKG, "host"), "-o", DRIVER_PATH, DRIVER_SOURCES[0], DRIVER_SOURCES[1], DRIVER_SOURCES[2],
           "-L" + _PKG, "-lgact_hip", "-Wl,-rpath," + _PKG]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return DRIVER_PATH


ASAN_DRIVER_PATH = DRIVER_PATH + "_asan"


def build_driver_asan(force=False, verbose=False):
    """the same host sources under AddressSanitizer + UndefinedBehaviorSanitizer (sanitizers run on
    the CPU build only; the CPU suite drives it through --dsoft-only, which never touches the GPU)"""
    build(verbose=verbose)
    if not force and os.path.exists(ASAN_DRIVER_PATH):
        newest = max(os.path.getmtime(s) for s in DRIVER_SOURCES + [LIB_PATH])
        if os.path.getmtime(ASAN_DRIVER_PATH) >= newest:
            return ASAN_DRIVER_PATH
    cmd = ["g++", "-O1", "-g", "-std=c++14", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(_ROOT, "include"), "-I" + os.path.join(_PKG, "host"),
           "-o", ASAN_DRIVER_PATH, DRIVER_SOURCES[0], DRIVER_SOURCES[1], DRIVER_SOURCES[2],
           "-L" + _PKG, "-lgact_hip", "-Wl,-rpath," + _PKG]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return ASAN_DRIVER_PATH


def driver_path():
    """the built driver; compiled here only if it does not exist yet (never re-built behind the back of
    concurrently running ranks -- __graft_entry__.build() is what refreshes stale binaries)"""
    if os.path.exists(DRIVER_PATH) and os.path.exists(LIB_PATH):
        return DRIVER_PATH
    return build_driver()


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    global LIB_PATH
    LIB_PATH = os.environ.get("GACT_HIP_LIB_PATH", LIB_PATH)        # A/B measurements of two builds in one GPU call
    if not os.path.exists(LIB_PATH):
        raise GactHipError("%s is missing: run __graft_entry__.build() (hipcc) first; "
                           "this engine has no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int32
    L.gact_hip_last_error.restype = C.c_char_p
    L.gact_hip_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.gact_hip_destroy.argtypes = [vp]
    L.gact_hip_destroy.restype = None
    L.gact_hip_get_device_info.argtypes = [vp, C.POINTER(DeviceInfo)]
    L.gact_hip_upload_seqs.argtypes = [vp, C.c_int, vp, vp, i32]
    L.gact_hip_align_tiles.argtypes = [vp, C.c_int, i32, vp, vp, vp, i32]
    L.gact_hip_align_tiles_inline.argtypes = [vp, C.c_int, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32]
    L.gact_hip_extend_candidates.argtypes = [vp, C.c_int, i32, vp, C.c_int, C.c_int, vp]
    L.gact_hip_candidates_upload.argtypes = [vp, C.c_int, i32, vp]
    L.gact_hip_candidates_run.argtypes = [vp, C.c_int, i32, C.c_int, C.c_int]
    L.gact_hip_candidates_run_range.argtypes = [vp, C.c_int, i32, i32, C.c_int, C.c_int]
    L.gact_hip_candidates_run_mixed.argtypes = [vp, C.c_int, i32, i32, i32, C.c_int]
    L.gact_hip_candidates_fetch.argtypes = [vp, C.c_int, i32, vp]
    L.gact_hip_sync.argtypes = [vp, C.c_int]
    L.gact_hip_last_kernel_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.gact_hip_last_run_stats.argtypes = [vp, C.c_int, C.POINTER(RunStats)]
    L.gact_hip_device_overlaps.argtypes = [vp, C.c_int]
    L.gact_hip_device_overlaps.restype = vp
    L.gact_hip_stream.argtypes = [vp, C.c_int]
    L.gact_hip_stream.restype = vp
    L.gact_hip_measure_valu_rate.argtypes = [vp, C.POINTER(C.c_double)]
    L.gact_hip_measure_valu_rate.restype = C.c_int
    L.gact_hip_scratch_fills.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gact_hip_scratch_fills.restype = C.c_int
    L.gact_hip_format_overlap.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, i32]
    L.gact_hip_dsoft_build.argtypes = [vp, C.POINTER(DsoftParams), C.POINTER(DsoftInfo)]
    L.gact_hip_dsoft_query.argtypes = [vp, C.c_int, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_float)]
    L.gact_hip_candidates_download.argtypes = [vp, C.c_int, i32, vp]
    L.gact_hip_derive_revcomp.argtypes = [vp]
    L.gact_hip_register_output.argtypes = [vp, C.c_int, vp, C.c_int64]
    L.gact_hip_unregister_output.argtypes = [vp, C.c_int]
    try:
        L.gact_hip_candidates_paths.argtypes = [vp, C.c_int, i32, vp, i32, C.c_int, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.gact_hip_candidates_paths.restype = C.c_int
        L.gact_hip_last_paths_stats.argtypes = [vp, C.c_int, C.POINTER(PathsStats)]
        L.gact_hip_last_paths_stats.restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_candidates_summaries.argtypes = [vp, C.c_int, i32, vp, i32, C.c_int, vp, vp]
        L.gact_hip_candidates_summaries.restype = C.c_int
        L.gact_hip_last_summaries_stats.argtypes = [vp, C.c_int, C.POINTER(SummariesStats)]
        L.gact_hip_last_summaries_stats.restype = C.c_int
        L.gact_hip_format_paf.argtypes = [vp, vp, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.c_char_p, i32]
        L.gact_hip_format_paf.restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_select_overlaps.argtypes = [vp, C.c_int, i32, vp, i32, vp, i32, C.POINTER(i32)]
        L.gact_hip_select_overlaps.restype = C.c_int
        L.gact_hip_last_select_stats.argtypes = [vp, C.c_int, C.POINTER(SelectStats)]
        L.gact_hip_last_select_stats.restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_read_coverage.argtypes = [vp, C.c_int, i32, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp]
        L.gact_hip_read_coverage.restype = C.c_int
        L.gact_hip_last_cover_stats.argtypes = [vp, C.c_int, C.POINTER(CoverStats)]
        L.gact_hip_last_cover_stats.restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_filter_overlaps.argtypes = [vp, C.c_int, i32, vp, i32, vp, vp, i32, i32, i32, C.POINTER(FilterParams), vp, vp, vp, i32,
                                               C.POINTER(i32), vp]
        L.gact_hip_filter_overlaps.restype = C.c_int
        L.gact_hip_last_filter_stats.argtypes = [vp, C.c_int, C.POINTER(FilterStats)]
        L.gact_hip_last_filter_stats.restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_place_reads.argtypes = [vp, C.c_int, i32, vp, i32, vp, vp, i32, i32, vp, C.POINTER(PlaceParams), vp, vp]
        L.gact_hip_place_reads.restype = C.c_int
        L.gact_hip_last_place_stats.argtypes = [vp, C.c_int, C.POINTER(PlaceStats)]
        L.gact_hip_last_place_stats.restype = C.c_int
        L.gact_hip_format_sam.argtypes = [vp, vp, i32, vp, C.c_char_p, vp, C.c_int64, C.c_char_p, C.c_char_p, C.c_int64]
        L.gact_hip_format_sam.restype = C.c_int64
        L.gact_hip_format_sam_unmapped.argtypes = [C.c_char_p, vp, C.c_int64, C.c_char_p, C.c_int64]
        L.gact_hip_format_sam_unmapped.restype = C.c_int64
    except AttributeError:
        pass
    try:
        L.gact_hip_overlap_graph.argtypes = [vp, C.c_int, i32, vp, i32, vp, vp, i32, vp, vp, C.POINTER(GraphParams), vp, vp, vp,
                                             C.c_int64, C.POINTER(C.c_int64)]
        L.gact_hip_overlap_graph.restype = C.c_int
        L.gact_hip_last_graph_stats.argtypes = [vp, C.c_int, C.POINTER(GraphStats)]
        L.gact_hip_last_graph_stats.restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_unitigs.argtypes = [vp, C.c_int, i32, vp, vp, vp, C.c_int64, vp, C.POINTER(UnitigParams), vp, C.POINTER(i32), vp, vp,
                                       vp, C.c_int64, C.POINTER(C.c_int64)]
        L.gact_hip_unitigs.restype = C.c_int
        L.gact_hip_last_unitig_stats.argtypes = [vp, C.c_int, C.POINTER(UnitigStats)]
        L.gact_hip_last_unitig_stats.restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_pop_bubbles.argtypes = [vp, C.c_int, i32, vp, vp, vp, C.c_int64, vp, vp, C.POINTER(BubbleParams), vp, C.c_int64,
                                           C.POINTER(C.c_int64), vp, vp]
        L.gact_hip_pop_bubbles.restype = C.c_int
        L.gact_hip_last_bubble_stats.argtypes = [vp, C.c_int, C.POINTER(BubbleStats)]
        L.gact_hip_last_bubble_stats.restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_prune_overlaps.argtypes = [vp, C.c_int, i32, vp, vp, vp, C.c_int64, vp, vp, C.POINTER(PruneParams), vp, vp]
        L.gact_hip_prune_overlaps.restype = C.c_int
        L.gact_hip_last_prune_stats.argtypes = [vp, C.c_int, C.POINTER(PruneStats)]
        L.gact_hip_last_prune_stats.restype = C.c_int
        L.gact_hip_clean_graph.argtypes = [vp, C.c_int, i32, vp, vp, vp, C.c_int64, vp, C.POINTER(CleanParams), vp, vp, vp, C.c_int64,
                                           C.POINTER(C.c_int64)]
        L.gact_hip_clean_graph.restype = C.c_int
        L.gact_hip_last_clean_stats.argtypes = [vp, C.c_int, C.POINTER(CleanStats)]
        L.gact_hip_last_clean_stats.restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_pileup_begin.argtypes = [vp, i32, i32]
        L.gact_hip_pileup_add.argtypes = [vp, C.c_int, i32, vp, i32, C.c_int]
        L.gact_hip_pileup_finish.argtypes = [vp, i32, vp, vp, vp]
        L.gact_hip_last_pileup_stats.argtypes = [vp, C.POINTER(PileupStats)]
        for name in ("pileup_begin", "pileup_add", "pileup_finish", "last_pileup_stats"):
            getattr(L, "gact_hip_" + name).restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_pileup_begin_ins.argtypes = [vp, i32, i32, i32]
        L.gact_hip_pileup_corrected.argtypes = [vp, i32, vp, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.gact_hip_last_pileup_ins_stats.argtypes = [vp, C.POINTER(PileupInsStats)]
        for name in ("pileup_begin_ins", "pileup_corrected", "last_pileup_ins_stats"):
            getattr(L, "gact_hip_" + name).restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_pileup_variants.argtypes = [vp, C.POINTER(VariantParams), vp, C.c_int64, C.POINTER(C.c_int64), vp]
        L.gact_hip_last_variant_stats.argtypes = [vp, C.POINTER(VariantStats)]
        L.gact_hip_format_vcf.argtypes = [vp, C.c_char_p, vp, C.c_int64, C.c_char_p, C.c_size_t]
        for name in ("pileup_variants", "last_variant_stats", "format_vcf"):
            getattr(L, "gact_hip_" + name).restype = C.c_int
    except AttributeError:
        pass
    try:                                    # (an older build loaded through GACT_HIP_LIB_PATH for an A/B run has none)
        L.gact_hip_comm_create.argtypes = [vp, i32, i32, C.c_char_p, i32, C.POINTER(vp)]
        L.gact_hip_comm_gather_lines.argtypes = [vp, C.c_int, i32, vp, vp, C.c_int64]
        L.gact_hip_comm_destroy.argtypes = [vp]
        for name in ("comm_create", "comm_gather_lines", "comm_destroy"):
            getattr(L, "gact_hip_" + name).restype = C.c_int
    except AttributeError:
        pass
    try:
        L.gact_hip_set_option.argtypes = [vp, C.c_char_p, i32]
        L.gact_hip_set_option.restype = C.c_int
    except AttributeError:
        pass
    for name in ("register_output", "unregister_output", "derive_revcomp", "dsoft_build", "dsoft_query", "candidates_download", "create", "get_device_info", "upload_seqs", "align_tiles", "align_tiles_inline",
                 "extend_candidates", "candidates_upload", "candidates_run", "candidates_run_range", "candidates_run_mixed",
                 "candidates_fetch", "sync", "last_kernel_ms", "last_run_stats", "format_overlap"):
        getattr(L, "gact_hip_" + name).restype = C.c_int
    _lib = L
    return L


EXPORTS = ("gact_hip_create", "gact_hip_destroy", "gact_hip_last_error", "gact_hip_get_device_info",
           "gact_hip_upload_seqs", "gact_hip_align_tiles", "gact_hip_align_tiles_inline",
           "gact_hip_extend_candidates", "gact_hip_candidates_upload", "gact_hip_candidates_run",
           "gact_hip_candidates_run_range", "gact_hip_candidates_run_mixed", "gact_hip_candidates_fetch", "gact_hip_sync",
           "gact_hip_last_kernel_ms", "gact_hip_last_run_stats", "gact_hip_device_overlaps", "gact_hip_stream",
           "gact_hip_measure_valu_rate", "gact_hip_format_overlap", "gact_hip_dsoft_build", "gact_hip_dsoft_query",
           "gact_hip_candidates_download", "gact_hip_derive_revcomp", "gact_hip_register_output",
           "gact_hip_unregister_output", "gact_hip_set_option", "gact_hip_prepare",
           "gact_hip_comm_create", "gact_hip_comm_gather_lines", "gact_hip_comm_destroy", "gact_hip_options_describe", "gact_hip_plan_describe",
           "gact_hip_candidates_paths", "gact_hip_last_paths_stats", "gact_hip_candidates_summaries",
           "gact_hip_last_summaries_stats", "gact_hip_format_paf", "gact_hip_select_overlaps", "gact_hip_last_select_stats",
           "gact_hip_read_coverage", "gact_hip_last_cover_stats", "gact_hip_overlap_graph", "gact_hip_last_graph_stats",
           "gact_hip_unitigs", "gact_hip_last_unitig_stats", "gact_hip_pop_bubbles", "gact_hip_last_bubble_stats",
           "gact_hip_prune_overlaps", "gact_hip_last_prune_stats", "gact_hip_clean_graph", "gact_hip_last_clean_stats",
           "gact_hip_pileup_begin", "gact_hip_pileup_add", "gact_hip_pileup_finish", "gact_hip_last_pileup_stats",
           "gact_hip_pileup_begin_ins", "gact_hip_pileup_corrected", "gact_hip_last_pileup_ins_stats",
           "gact_hip_place_reads", "gact_hip_last_place_stats", "gact_hip_format_sam", "gact_hip_format_sam_unmapped",
           "gact_hip_pileup_variants", "gact_hip_last_variant_stats", "gact_hip_format_vcf",
           "gact_hip_filter_overlaps", "gact_hip_last_filter_stats", "gact_hip_scratch_fills")


def plan(count, flags=0, compute_units=256, tile_size=320, tile_overlap=120, scoring=(1, -1, -1, -1), threshold=35):
    """the launch plan of gact_policy.hpp for one pass over `count` candidates (no device needed); flags: 1 raw bytes,
    2 the launch shares the machine, 4 role launch on, 8 cooperative launch always, 16 never"""
    import json
    lib = load()
    lib.gact_hip_plan_describe.restype = C.c_int64
    lib.gact_hip_plan_describe.argtypes = [C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int64]
    p = Params(tile_size, tile_overlap, scoring[0], scoring[1], scoring[2], scoring[3], threshold, 0, 1, 0)
    buf = C.create_string_buffer(1024)
    if lib.gact_hip_plan_describe(C.byref(p), compute_units, count, flags, buf, 1024) < 0:
        raise GactHipError(lib.gact_hip_last_error().decode())
    return json.loads(buf.value.decode())


def options_table():
    """[(name, environment variable or None, when, class, doc)] of every switch libgact_hip.so reads (no device needed)"""
    lib = load()
    lib.gact_hip_options_describe.restype = C.c_int64
    lib.gact_hip_options_describe.argtypes = [C.c_char_p, C.c_int64]
    n = lib.gact_hip_options_describe(None, 0)
    buf = C.create_string_buffer(int(n))
    lib.gact_hip_options_describe(buf, n)
    rows = []
    for line in buf.value.decode().splitlines():
        name, env, when, klass, doc = [x.strip() for x in line.split(" | ", 4)]
        rows.append((name, None if env == "-" else env, when, klass, doc))
    return rows


class Engine:
    """One gact_hip_engine.  Mirrors GPU_init .. GPU_close of the reference."""

    def __init__(self, tile_size=320, tile_overlap=120, scoring=(1, -1, -1, -1), threshold=35,
                 device_id=0, n_slots=1, max_blocks=0):
        self.L = load()
        self.p = Params(tile_size, tile_overlap, scoring[0], scoring[1], scoring[2], scoring[3],
                        threshold, device_id, n_slots, max_blocks)
        self.h = C.c_void_p()
        self._registered = {}
        self._n_cands = {}                            # slot -> candidates it holds (select_overlaps' default n)
        self._ref_offsets = np.zeros(1, dtype=np.int64)       # of SET_REF as uploaded (the pileup's window is made of its reads)
        self._pileup = None                           # (n_reads, positions) of the open pileup window
        self._check(self.L.gact_hip_create(C.byref(self.p), C.byref(self.h)))
        self.tile_size = tile_size
        self.tile_overlap = tile_overlap

    def _check(self, rc):
        if rc < 0:
            raise GactHipError("gact_hip error %d: %s" % (rc, self.L.gact_hip_last_error().decode()))
        return rc

    def close(self):
        if self.h:
            for slot in list(getattr(self, "_registered", {})):
                self.L.gact_hip_unregister_output(self.h, slot)
            self._registered = {}
            self.L.gact_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_info(self):
        info = DeviceInfo()
        self._check(self.L.gact_hip_get_device_info(self.h, C.byref(info)))
        return {"compute_units": info.compute_units, "clock_mhz": info.clock_mhz,
                "waves_per_cu": info.waves_per_cu, "wave_size": info.wave_size,
                "hbm_bytes": info.hbm_bytes, "arch": info.arch.decode()}

    def upload(self, which, concat, offsets):
        concat = np.ascontiguousarray(concat, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self._check(self.L.gact_hip_upload_seqs(self.h, which, concat.ctypes.data, offsets.ctypes.data,
                                                len(offsets) - 1))
        if which == SET_REF:
            self._ref_offsets = offsets.copy()

    def derive_revcomp(self):
        """SET_QUERY_RC := reverse complement of SET_QUERY, on the device (darwin.cpp:110-147)"""
        self._check(self.L.gact_hip_derive_revcomp(self.h))

    def upload_seqs(self, which, seqs):
        seqs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else
                np.asarray(s, dtype=np.uint8) for s in seqs]
        offs = np.zeros(len(seqs) + 1, dtype=np.int64)
        if seqs:
            offs[1:] = np.cumsum([len(s) for s in seqs])
        cat = np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)
        self.upload(which, cat, offs)

    def align_tiles(self, tiles, slot=0):
        tiles = np.ascontiguousarray(tiles, dtype=TILE_DTYPE)
        n = len(tiles)
        stride = 2 * self.tile_size
        res = np.zeros(n, dtype=TILE_RESULT_DTYPE)
        states = np.zeros((n, stride), dtype=np.uint8)
        self._check(self.L.gact_hip_align_tiles(self.h, slot, n, tiles.ctypes.data, res.ctypes.data,
                                                states.ctypes.data, stride))
        return res, states

    def align_tiles_inline(self, refs, queries, reverses, firsts, slot=0):
        n = len(refs)
        stride_seq = max([1] + [len(r) for r in refs] + [len(q) for q in queries])
        rb = np.zeros((n, stride_seq), dtype=np.uint8)
        qb = np.zeros((n, stride_seq), dtype=np.uint8)
        rl = np.zeros(n, dtype=np.int32)
        ql = np.zeros(n, dtype=np.int32)
        for t in range(n):
            r = np.frombuffer(refs[t], dtype=np.uint8) if isinstance(refs[t], (bytes, bytearray)) else refs[t]
            q = np.frombuffer(queries[t], dtype=np.uint8) if isinstance(queries[t], (bytes, bytearray)) else queries[t]
            rb[t, :len(r)] = r
            qb[t, :len(q)] = q
            rl[t], ql[t] = len(r), len(q)
        rv = np.ascontiguousarray(reverses, dtype=np.uint8)
        fs = np.ascontiguousarray(firsts, dtype=np.uint8)
        stride = 2 * self.tile_size
        res = np.zeros(n, dtype=TILE_RESULT_DTYPE)
        states = np.zeros((n, stride), dtype=np.uint8)
        self._check(self.L.gact_hip_align_tiles_inline(
            self.h, slot, n, rb.ctypes.data, qb.ctypes.data, stride_seq, rl.ctypes.data, ql.ctypes.data,
            rv.ctypes.data, fs.ctypes.data, res.ctypes.data, states.ctypes.data, stride))
        return res, states

    def extend(self, cands, complement=False, same_file=True, slot=0):
        cands = np.ascontiguousarray(cands, dtype=CAND_DTYPE)
        out = np.zeros(len(cands), dtype=OVERLAP_DTYPE)
        self._check(self.L.gact_hip_extend_candidates(self.h, slot, len(cands), cands.ctypes.data,
                                                      int(complement), int(same_file), out.ctypes.data))
        self._n_cands[slot] = len(cands)
        return out

    def candidates_upload(self, cands, slot=0):
        cands = np.ascontiguousarray(cands, dtype=CAND_DTYPE)
        self._check(self.L.gact_hip_candidates_upload(self.h, slot, len(cands), cands.ctypes.data))
        self._n_cands[slot] = len(cands)

    def candidates_run(self, n, complement=False, same_file=True, slot=0, first=0):
        self._check(self.L.gact_hip_candidates_run_range(self.h, slot, first, n, int(complement), int(same_file)))

    def candidates_run_mixed(self, n, rc_from, same_file=True, slot=0, first=0):
        """candidates [first, first+n) of the uploaded array; index >= rc_from => complement"""
        self._check(self.L.gact_hip_candidates_run_mixed(self.h, slot, first, n, rc_from, int(same_file)))

    def candidates_fetch(self, n, slot=0, out=None):
        """records of candidates [0, n); `out`: a caller-owned OVERLAP_DTYPE array to fill (no allocation)"""
        if out is None:
            out = np.empty(n, dtype=OVERLAP_DTYPE)
        assert out.dtype == OVERLAP_DTYPE and len(out) >= n and out.flags["C_CONTIGUOUS"]
        self._check(self.L.gact_hip_candidates_fetch(self.h, slot, n, out.ctypes.data))
        return out

    def candidates_paths(self, sel=None, n=None, rc_from=0x7fffffff, same_file=True, slot=0, ops_cap=None):
        """alignments of candidates `sel` of the slot's candidate array (sel None: the first n), index >= rc_from =>
        reverse-complement strand: (records OVERLAP_DTYPE, paths PATH_DTYPE, ops uint32), candidate k's ops at
        ops[paths[k]["op_offset"] : + paths[k]["n_ops"]] (include/gact_hip.h gact_hip_candidates_paths).  ops_cap: room
        for the first attempt; too little costs a second path run"""
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.int32)
            n = len(sel)
        n = int(n or 0)
        records = np.zeros(n, dtype=OVERLAP_DTYPE)
        paths = np.zeros(n, dtype=PATH_DTYPE)
        # (a guess that rarely needs the retry: 10 kb overlaps of reads with 15 % error have ~2,500 ops; the pages an
        #  unused tail would take are never touched)
        cap = int(ops_cap) if ops_cap is not None else 4096 * n + 1024
        needed = C.c_int64()
        for attempt in (0, 1):
            ops = np.empty(cap, dtype=np.uint32)
            rc = self.L.gact_hip_candidates_paths(self.h, slot, n, _ptr(sel), int(rc_from),
                                                  int(same_file), records.ctypes.data, paths.ctypes.data, ops.ctypes.data, cap,
                                                  C.byref(needed))
            if rc == -1 and attempt == 0 and needed.value > cap:
                cap = int(needed.value)              # too little room: once more with what the call said it needs
                continue
            self._check(rc)
            return records, paths, ops[:int(needed.value)]

    def _stats(self, fn, Struct, *args):
        """a last_*_stats entry's figures as a dict (an array field as a list)"""
        st = Struct()
        self._check(fn(self.h, *args, C.byref(st)))
        return {n: (list(getattr(st, n)) if isinstance(getattr(st, n), C.Array) else getattr(st, n)) for n, _ in Struct._fields_}

    def _records_arg(self, records, n, slot):
        """(records, n) of select_overlaps, read_coverage and overlap_graph: the caller's OVERLAP_DTYPE records (n None: all of
        them), else records [0, n) of the slot's device array (n None: as many as the slot holds candidates)"""
        if records is not None:
            records = np.ascontiguousarray(records, dtype=OVERLAP_DTYPE)
            n = len(records) if n is None else n
            assert n <= len(records)
        elif n is None:
            n = self._n_cands.get(slot, 0)
        return records, int(n)

    def last_paths_stats(self, slot=0):
        """the slot's last path run: device ms (HIP events around the whole call), chunks, most column bytes of one chunk,
        columns, ops"""
        return self._stats(self.L.gact_hip_last_paths_stats, PathsStats, slot)

    def candidates_summaries(self, sel=None, n=None, rc_from=0x7fffffff, same_file=True, slot=0):
        """the alignments of candidates_paths reduced on the device, same selection: (records OVERLAP_DTYPE, sums
        SUMMARY_DTYPE), sums[k] == summarise(candidate k's ops) (include/gact_hip.h gact_hip_candidates_summaries)"""
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.int32)
            n = len(sel)
        n = int(n or 0)
        records = np.zeros(n, dtype=OVERLAP_DTYPE)
        sums = np.zeros(n, dtype=SUMMARY_DTYPE)
        self._check(self.L.gact_hip_candidates_summaries(self.h, slot, n, _ptr(sel),
                                                         int(rc_from), int(same_file), records.ctypes.data, sums.ctypes.data))
        return records, sums

    def last_summaries_stats(self, slot=0):
        """the slot's last summary run: device ms (HIP events around the whole call), chain-kernel launches, device bytes
        the call holds for itself"""
        return self._stats(self.L.gact_hip_last_summaries_stats, SummariesStats, slot)

    def select_overlaps(self, n=None, records=None, mode="pair", slot=0):
        """every overlap once, chosen on the device: the ascending int32 indices of the records to keep, usable as `sel` of
        candidates_paths / candidates_summaries.  records None: records [0, n) of the slot's device array as its last run
        left them (n None: as many as the slot holds candidates); else the caller's OVERLAP_DTYPE records (n None: all of them).  mode "exact": the lowest index of every
        set of emitted records that print the same line; "pair": per (ref_id, query_id, comp) the record with the highest
        score, then the larger (ae - ab) + (be - bb), then the lower index (include/gact_hip.h gact_hip_select_overlaps)"""
        if isinstance(mode, str):
            if mode not in _SELECT_MODES:
                raise GactHipError("select_overlaps: unknown mode %r (\"exact\" or \"pair\")" % (mode,))
            mode = _SELECT_MODES[mode]
        records, n = self._records_arg(records, n, slot)
        sel = np.empty(max(n, 0), dtype=np.int32)
        n_sel = C.c_int32()
        self._check(self.L.gact_hip_select_overlaps(self.h, slot, n, _ptr(records),
                                                    mode, sel.ctypes.data, n, C.byref(n_sel)))
        return sel[:n_sel.value].copy()

    def last_select_stats(self, slot=0):
        """the slot's last selection: device ms (HIP events around the whole call), emitted records, selected records,
        table slots, device bytes the call holds for itself"""
        return self._stats(self.L.gact_hip_last_select_stats, SelectStats, slot)

    def read_coverage(self, read_lens, n=None, records=None, sel=None, sums=None, sides="both", min_depth=3, depth=False, slot=0):
        """per-read coverage of an overlap set, swept on the device: one COVER_DTYPE record per read of `read_lens` -- intervals
        counted, highest depth, positions covered, positions covered min_depth deep, the longest (leftmost) run of those, the
        sum of the depth -- or (cover, depth) with the int32 depth of every position, read after read, when `depth` is set.
        records None: records [0, n) of the slot's device array as its last run left them (n None: as many as the slot holds
        candidates); else the caller's OVERLAP_DTYPE records.  sel: the indices that count (select_overlaps' list), None: all;
        records that were not emitted never count.  sums: SUMMARY_DTYPE, one per chosen record: the begins become the
        alignment's, as the PAF lines have them.  sides "ref" / "query" / "both" or COVER_REF / COVER_QUERY / COVER_BOTH
        (include/gact_hip.h gact_hip_read_coverage)"""
        if isinstance(sides, str):
            if sides not in _COVER_SIDES:
                raise GactHipError("read_coverage: unknown sides %r (\"ref\", \"query\" or \"both\")" % (sides,))
            sides = _COVER_SIDES[sides]
        read_lens = np.ascontiguousarray(read_lens, dtype=np.int32)
        records, n = self._records_arg(records, n, slot)
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.int32)
        if sums is not None:
            sums = np.ascontiguousarray(sums, dtype=SUMMARY_DTYPE)
            assert len(sums) == (len(sel) if sel is not None else n)
        cover = np.zeros(len(read_lens), dtype=COVER_DTYPE)
        per_base = np.zeros(int(read_lens.astype(np.int64).clip(0).sum()), dtype=np.int32) if depth else None
        self._check(self.L.gact_hip_read_coverage(self.h, slot, n, _ptr(records), len(sel) if sel is not None else 0, _ptr(sel),
                                                  _ptr(sums), int(sides), int(min_depth), len(read_lens), _ptr(read_lens),
                                                  _ptr(cover), _ptr(per_base)))
        return (cover, per_base) if depth else cover

    def last_cover_stats(self, slot=0):
        """the slot's last coverage call: device ms (HIP events around the whole call), reads, intervals counted, positions,
        device bytes the call holds for itself"""
        return self._stats(self.L.gact_hip_last_cover_stats, CoverStats, slot)

    def filter_overlaps(self, sums, n=None, records=None, sel=None, min_identity=FILTER_DEFAULTS["min_identity"],
                        min_span=FILTER_DEFAULTS["min_span"], max_drop=FILTER_DEFAULTS["max_drop"], sides="both",
                        read_lens_or_n_reads=None, read_first=0, table=False, why=False, slot=0):
        """the overlap set filtered on the device by identity, span and each read's best: (sel2, sums2) -- the kept record
        indices, ascending in their position in the chosen list, and their summaries, to be passed on as `sel` and `sums` --
        followed by the FILTER_READ_DTYPE table of the window's reads when `table` is set and by the int32 reason of every
        chosen record (FILTER_*) when `why` is set.  sums (SUMMARY_DTYPE, one per chosen record) is required; records, n and
        sel as in read_coverage.  A record is dropped when it is not emitted, has no columns, has an identity under
        min_identity (permille of its columns), a shorter span under min_span, or, with max_drop < 1000, lies more than
        max_drop permille under the best passed record of a read it names on a requested side.  read_lens_or_n_reads: the
        reads of the window [read_first, read_first + n_reads), as their number or as anything with a length; None: no table,
        which max_drop == 1000 allows (include/gact_hip.h gact_hip_filter_overlaps)"""
        if isinstance(sides, str):
            if sides not in _COVER_SIDES:
                raise GactHipError("filter_overlaps: unknown sides %r (\"ref\", \"query\" or \"both\")" % (sides,))
            sides = _COVER_SIDES[sides]
        records, n = self._records_arg(records, n, slot)
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.int32)
        n_chosen = len(sel) if sel is not None else max(n, 0)
        if sums is not None:
            sums = np.ascontiguousarray(sums, dtype=SUMMARY_DTYPE)
            if len(sums) != n_chosen:
                raise GactHipError("filter_overlaps: %d summaries for %d chosen records" % (len(sums), n_chosen))
        if read_lens_or_n_reads is None:
            n_reads = 0
        elif isinstance(read_lens_or_n_reads, (int, np.integer)):
            n_reads = int(read_lens_or_n_reads)
        else:
            n_reads = len(read_lens_or_n_reads)
        params = FilterParams(int(min_identity), int(min_span), int(max_drop))
        reasons = np.zeros(n_chosen, dtype=np.int32) if why else None
        reads = np.zeros(max(n_reads, 0), dtype=FILTER_READ_DTYPE) if table else None
        n_kept = C.c_int32()
        kept_at = np.empty(n_chosen, dtype=np.int32)          # (room for every chosen record: the call never has to be repeated)
        kept_sel = np.empty(n_chosen, dtype=np.int32)
        self._check(self.L.gact_hip_filter_overlaps(self.h, slot, n, _ptr(records), len(sel) if sel is not None else 0, _ptr(sel),
                                                    _ptr(sums), int(sides), int(read_first), n_reads, C.byref(params), _ptr(reasons),
                                                    kept_at.ctypes.data, kept_sel.ctypes.data, n_chosen, C.byref(n_kept),
                                                    _ptr(reads)))
        out = (kept_sel[:n_kept.value].copy(), sums[kept_at[:n_kept.value]] if sums is not None else None)
        if table:
            out += (reads,)
        if why:
            out += (reasons,)
        return out

    def last_filter_stats(self, slot=0):
        """the slot's last filter call: device ms (HIP events around the whole call), reads of the window, chosen, counted and
        kept records, the dropped ones per reason, device bytes the call holds for itself"""
        return self._stats(self.L.gact_hip_last_filter_stats, FilterStats, slot)

    def place_reads(self, read_lens, read_first=0, n=None, records=None, sel=None, sums=None, mask_permille=PLACE_DEFAULT_MASK_PERMILLE,
                    mapq_cap=PLACE_DEFAULT_MAPQ_CAP, slot=0):
        """every read of the window [read_first, read_first + len(read_lens)) of the query set placed on the device: (place,
        reads) -- one PLACE_DTYPE record per chosen record (kind PLACE_*, mapq, parent, rank) and one READ_PLACE_DTYPE record
        per read (its counted records, the chosen index of its primary or -1, supplementaries, secondaries, extras, the
        primary's score, its best secondary's, its MAPQ).  records, n, sel and sums as in read_coverage; a read's counted
        records are ordered by score, span and index, a record that an earlier parent's query interval overlaps by
        mask_permille of the shorter one is that parent's secondary, the others are the primary and the supplementaries, and
        mapq = mapq_cap * (s1 - s2) / s1 -- a stated rule, not a calibrated model (include/gact_hip.h gact_hip_place_reads)"""
        read_lens = np.ascontiguousarray(read_lens, dtype=np.int32)
        records, n = self._records_arg(records, n, slot)
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.int32)
        n_chosen = len(sel) if sel is not None else max(n, 0)
        if sums is not None:
            sums = np.ascontiguousarray(sums, dtype=SUMMARY_DTYPE)
            assert len(sums) == n_chosen
        place = np.zeros(n_chosen, dtype=PLACE_DTYPE)
        place["parent"] = place["rank"] = -1
        reads = np.zeros(len(read_lens), dtype=READ_PLACE_DTYPE)
        reads["primary"] = -1
        params = PlaceParams(int(mask_permille), int(mapq_cap))
        self._check(self.L.gact_hip_place_reads(self.h, slot, n, _ptr(records), len(sel) if sel is not None else 0, _ptr(sel),
                                                _ptr(sums), int(read_first), len(read_lens), _ptr(read_lens), C.byref(params),
                                                _ptr(place), _ptr(reads)))
        return place, reads

    def last_place_stats(self, slot=0):
        """the slot's last placement: device ms (HIP events around the whole call), reads of the window, the most counted
        records on one read, counted records, parents, secondaries, extras, device bytes the call holds for itself"""
        return self._stats(self.L.gact_hip_last_place_stats, PlaceStats, slot)

    def overlap_graph(self, read_lens, n=None, records=None, sel=None, sums=None, clip=None, params=None, classes=False, slot=0):
        """the overlap graph of an overlap set, made on the device: (reads, arcs) -- one GRAPH_READ_DTYPE record per read of
        `read_lens` (hits, internal hits, reads it contains, the record that contains it or -1, out-degrees of its two vertices,
        all arcs and kept ones) and the GRAPH_ARC_DTYPE arcs ascending by (u, len, v), vertex 2 i = read i, 2 i + 1 its reverse
        complement, kept iff flags == 0 -- or (reads, arcs, classes) with one GRAPH_* class byte per chosen record.  records, n,
        sel and sums as in read_coverage.  clip: None, or (n_reads, 2) int32 [begin, end) of every read, read_coverage's
        span_begin / span_end.  params: None, a GraphParams, or a dict of max_hang, int_permille, min_ovlp, fuzz
        (include/gact_hip.h gact_hip_overlap_graph)"""
        read_lens = np.ascontiguousarray(read_lens, dtype=np.int32)
        records, n = self._records_arg(records, n, slot)
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.int32)
        n_chosen = len(sel) if sel is not None else max(n, 0)
        if sums is not None:
            sums = np.ascontiguousarray(sums, dtype=SUMMARY_DTYPE)
            assert len(sums) == n_chosen
        if clip is not None:
            clip = np.ascontiguousarray(clip, dtype=np.int32).reshape(-1)
            assert len(clip) == 2 * len(read_lens)
        if isinstance(params, dict):
            params = GraphParams(**params)
        reads = np.zeros(len(read_lens), dtype=GRAPH_READ_DTYPE)
        cls = np.zeros(n_chosen, dtype=np.uint8) if classes else None
        n_arcs = C.c_int64()
        cap = n_chosen                              # (room for 2 * n_chosen always suffices; most sets need less than half)
        for attempt in range(2):
            arcs = np.zeros(cap, dtype=GRAPH_ARC_DTYPE)
            rc = self.L.gact_hip_overlap_graph(self.h, slot, n, _ptr(records), len(sel) if sel is not None else 0, _ptr(sel), _ptr(sums),
                                               len(read_lens), _ptr(read_lens), _ptr(clip), C.byref(params) if params is not None else None,
                                               _ptr(reads), _ptr(cls), _ptr(arcs), cap, C.byref(n_arcs))
            if rc == 0 or attempt or n_arcs.value <= cap:
                break
            cap = n_arcs.value                      # (EINVAL with *n_arcs filled: once more with room for them)
        self._check(rc)
        arcs = arcs[:n_arcs.value].copy()
        return (reads, arcs, cls) if classes else (reads, arcs)

    def last_graph_stats(self, slot=0):
        """the slot's last overlap graph: device ms (HIP events around the whole call), reads, contained reads, chosen records
        per class (a list of 8), arcs proposed, arcs, transitive arcs, kept arcs, table slots, device bytes the call holds"""
        return self._stats(self.L.gact_hip_last_graph_stats, GraphStats, slot)

    def _graph_args(self, read_lens, reads, arcs, clip, skip=None):
        """the arrays of a call on an overlap graph, as the C-ABI takes them"""
        read_lens = np.ascontiguousarray(read_lens, dtype=np.int32)
        reads = np.ascontiguousarray(reads, dtype=GRAPH_READ_DTYPE)
        arcs = np.ascontiguousarray(arcs, dtype=GRAPH_ARC_DTYPE)
        n = len(read_lens)
        assert len(reads) == n
        if clip is not None:
            clip = np.ascontiguousarray(clip, dtype=np.int32).reshape(-1)
            assert len(clip) == 2 * n
        if skip is not None:
            skip = np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8)
            assert len(skip) == n
        return read_lens, reads, arcs, clip, skip, n

    def _with_room(self, cap, call):
        """call(cap) -> (rc, the count the call filled in, the array of cap records): made once, and where it came back EINVAL
        with a count beyond cap once more with room for that many; -> the array of the call that counts"""
        rc, need, out = call(cap)
        if rc != 0 and need > cap:
            rc, need, out = call(need)
        self._check(rc)
        return out

    def unitigs(self, read_lens, reads, arcs, clip=None, tip_reads=UNITIG_DEFAULT_TIP_READS, seq=False, slot=0):
        """the unitigs of an overlap graph, made on the device: (unitigs, layout, places) -- UNITIG_DTYPE records ascending by
        their first vertex, the UNITIG_ENTRY_DTYPE entries of their layouts one unitig after the other, and one
        UNITIG_PLACE_DTYPE record per read -- or (unitigs, layout, places, bases) with the unitigs' bases as bytes, spelled
        from the reads of SET_REF, when `seq` is set.  read_lens and clip as overlap_graph took them, reads and arcs as it
        returned them; tip_reads: dead ends of at most that many reads are cut, 0 cuts nothing
        (include/gact_hip.h gact_hip_unitigs)"""
        read_lens, reads, arcs, clip, _, n = self._graph_args(read_lens, reads, arcs, clip)
        params = UnitigParams(int(tip_reads))
        unitigs = np.zeros(n, dtype=UNITIG_DTYPE)
        layout = np.zeros(n, dtype=UNITIG_ENTRY_DTYPE)
        places = np.zeros(n, dtype=UNITIG_PLACE_DTYPE)
        n_unitigs, seq_len = C.c_int32(), C.c_int64()

        def call(cap):
            bases = np.zeros(cap, dtype=np.uint8) if seq else None
            rc = self.L.gact_hip_unitigs(self.h, slot, n, _ptr(read_lens), _ptr(clip), _ptr(reads), len(arcs), _ptr(arcs),
                                         C.byref(params), _ptr(unitigs), C.byref(n_unitigs), _ptr(layout), _ptr(places),
                                         _ptr(bases), cap, C.byref(seq_len))
            return rc, seq_len.value if seq else 0, bases

        # (most sets need far less than their reads' bases)
        bases = self._with_room(int(read_lens.astype(np.int64).sum()) // 2 if seq else 0, call)
        unitigs = unitigs[:n_unitigs.value].copy()
        layout = layout[:int(unitigs["n_reads"].sum())].copy()
        return (unitigs, layout, places, bases[:seq_len.value].tobytes()) if seq else (unitigs, layout, places)

    def last_unitig_stats(self, slot=0):
        """the slot's last unitig call: device ms (HIP events around the whole call), reads, reads placed, cut as tips and
        contained, unitigs, circular ones, the longest in reads and in bases, ranking launches, arcs with flags == 0, those
        left after the tip cut, joins and links among them, device bytes the call holds"""
        return self._stats(self.L.gact_hip_last_unitig_stats, UnitigStats, slot)

    def pop_bubbles(self, read_lens, reads, arcs, clip=None, skip=None, max_dist=BUBBLE_DEFAULT_MAX_DIST,
                    max_vertices=BUBBLE_MAX_VERTICES, slot=0):
        """the bubbles of an overlap graph, found and popped on the device: (bubbles, read_bubble, arc_flags) -- one
        BUBBLE_DTYPE record per bubble found, BUBBLE_POPPED or BUBBLE_LOST, ascending by source; per read the index of the
        bubble that removed it or -1; per arc its flags with GRAPH_ARC_BUBBLE set where a popped bubble removed it.
        read_lens, clip, reads and arcs as unitigs takes them; skip: None, or one value per read, != 0 takes the read's arcs
        out of the working set (the tips of an earlier unitigs call, places["state"] == UNITIG_TIP)
        (include/gact_hip.h gact_hip_pop_bubbles)"""
        read_lens, reads, arcs, clip, skip, n = self._graph_args(read_lens, reads, arcs, clip, skip)
        params = BubbleParams(int(max_dist), int(max_vertices))
        read_bubble = np.zeros(n, dtype=np.int32)
        arc_flags = np.zeros(len(arcs), dtype=np.int32)
        n_bubbles = C.c_int64()

        def call(cap):
            bubbles = np.zeros(cap, dtype=BUBBLE_DTYPE)
            rc = self.L.gact_hip_pop_bubbles(self.h, slot, n, _ptr(read_lens), _ptr(clip), _ptr(reads), len(arcs), _ptr(arcs),
                                             _ptr(skip), C.byref(params), _ptr(bubbles), cap, C.byref(n_bubbles),
                                             _ptr(read_bubble), _ptr(arc_flags))
            return rc, n_bubbles.value, bubbles

        bubbles = self._with_room(64, call)         # (a bubble per hundred reads is many)
        return bubbles[:n_bubbles.value].copy(), read_bubble, arc_flags

    def last_bubble_stats(self, slot=0):
        """the slot's last bubble call: device ms (HIP events around the whole call), reads, sources searched from, bubbles
        found, popped and lost, reads removed, arcs of the working set, arcs removed, the failed searches by their first
        failure (a list of 5: open, dead, twice, dist, many), device bytes the call holds"""
        return self._stats(self.L.gact_hip_last_bubble_stats, BubbleStats, slot)

    def prune_overlaps(self, read_lens, reads, arcs, clip=None, skip=None, ratio_permille=PRUNE_DEFAULT_RATIO_PERMILLE, best=False,
                       slot=0):
        """the weak arcs of an overlap graph, marked on the device: arc_flags -- per arc its flags with GRAPH_ARC_SHORT set where
        the arc's overlap, or its complement's, is below ratio_permille thousandths of the best one of its vertex -- or
        (arc_flags, vertex_best) with the best overlap of every examined vertex (0 elsewhere) when `best` is set.  read_lens,
        clip, reads, arcs and skip as pop_bubbles takes them (include/gact_hip.h gact_hip_prune_overlaps)"""
        read_lens, reads, arcs, clip, skip, n = self._graph_args(read_lens, reads, arcs, clip, skip)
        params = PruneParams(int(ratio_permille))
        arc_flags = np.zeros(len(arcs), dtype=np.int32)
        vertex_best = np.zeros(2 * n, dtype=np.int32) if best else None
        self._check(self.L.gact_hip_prune_overlaps(self.h, slot, n, _ptr(read_lens), _ptr(clip), _ptr(reads), len(arcs), _ptr(arcs),
                                                   _ptr(skip), C.byref(params), _ptr(arc_flags), _ptr(vertex_best)))
        return (arc_flags, vertex_best) if best else arc_flags

    def last_prune_stats(self, slot=0):
        """the slot's last prune call: device ms (HIP events around the whole call), reads, vertices examined, vertices that
        lost their last arc, arcs of the working set, weak arcs, arcs removed, device bytes the call holds"""
        return self._stats(self.L.gact_hip_last_prune_stats, PruneStats, slot)

    def clean_graph(self, read_lens, reads, arcs, clip=None, tip_reads=UNITIG_DEFAULT_TIP_READS, max_dist=BUBBLE_DEFAULT_MAX_DIST,
                    max_vertices=BUBBLE_MAX_VERTICES, ratios=(500, 700, 3), max_passes=4, slot=0):
        """the cleaning rounds of an overlap graph on the device -- tips and bubbles until a pass removes nothing, then the weak
        arcs at the ratios (lo, hi, n) in thousandths, settling again after every drop: (arc_flags, read_state, steps) -- per arc
        its flags with GRAPH_ARC_TIP, GRAPH_ARC_BUBBLE and GRAPH_ARC_SHORT set where a step removed it, one CLEAN_READ_DTYPE
        record per read, one CLEAN_STEP_DTYPE record per step made.  arc_flags written into arcs["flags"] is what unitigs takes
        (include/gact_hip.h gact_hip_clean_graph)"""
        read_lens, reads, arcs, clip, _, n = self._graph_args(read_lens, reads, arcs, clip)
        lo, hi, n_ratios = (int(v) for v in ratios)
        params = CleanParams(int(tip_reads), int(max_dist), int(max_vertices), lo, hi, n_ratios, int(max_passes))
        arc_flags = np.zeros(len(arcs), dtype=np.int32)
        read_state = np.zeros(n, dtype=CLEAN_READ_DTYPE)
        n_steps = C.c_int64()

        def call(cap):
            steps = np.zeros(cap, dtype=CLEAN_STEP_DTYPE)
            rc = self.L.gact_hip_clean_graph(self.h, slot, n, _ptr(read_lens), _ptr(clip), _ptr(reads), len(arcs), _ptr(arcs),
                                             C.byref(params), _ptr(arc_flags), _ptr(read_state), _ptr(steps), cap, C.byref(n_steps))
            return rc, n_steps.value, steps

        steps = self._with_room(16, call)           # (a graph that settles at once takes 2 + 3 steps)
        return arc_flags, read_state, steps[:n_steps.value].copy()

    def last_clean_stats(self, slot=0):
        """the slot's last clean call: device ms (HIP events around the whole call), reads, steps, passes, reads removed as tips
        and by bubbles, arcs removed by kind (a list of 3: tips, bubbles, prune), arcs left, device bytes the call holds"""
        return self._stats(self.L.gact_hip_last_clean_stats, CleanStats, slot)

    def pileup_begin(self, read_first=0, n_reads=None, ins_slots=0):
        """opens the pileup window: reads [read_first, read_first + n_reads) of SET_REF (n_reads None: to the set's end), counts
        zeroed; a second call starts over, and one that is refused leaves no window open, an earlier one's neither.
        ins_slots (0 .. PILEUP_MAX_INS_SLOTS): the inserted bases kept in front of every position, for pileup_corrected
        (include/gact_hip.h gact_hip_pileup_begin, gact_hip_pileup_begin_ins)"""
        n_all = len(self._ref_offsets) - 1
        if n_reads is None:
            n_reads = max(n_all - int(read_first), 0)
        self._pileup = None
        if int(ins_slots) == 0:
            self._check(self.L.gact_hip_pileup_begin(self.h, int(read_first), int(n_reads)))
        else:
            self._check(self.L.gact_hip_pileup_begin_ins(self.h, int(read_first), int(n_reads), int(ins_slots)))
        offs = self._ref_offsets
        self._pileup = (int(n_reads), int(offs[int(read_first) + int(n_reads)] - offs[int(read_first)]), int(ins_slots))

    def pileup_add(self, sel=None, n=None, rc_from=0x7fffffff, same_file=True, slot=0):
        """stacks the alignments of candidates `sel` of the slot's candidate array (sel None: the first n; index >= rc_from =>
        reverse-complement strand: the selection of candidates_paths) on their target reads inside the window, on the device;
        any number of calls, from several threads on different slots at once (gact_hip_pileup_add)"""
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.int32)
            n = len(sel)
        self._check(self.L.gact_hip_pileup_add(self.h, slot, int(n or 0), _ptr(sel),
                                               int(rc_from), int(same_file)))

    def pileup_finish(self, min_depth=3, counts=True, consensus=True):
        """-> (reads READ_PILEUP_DTYPE, counts uint32 [positions, 8] or None, consensus uint8 [positions] or None): the
        window's positions read after read, a position's counts indexed by PILEUP_*; the counts stay, so more pileup_add
        calls and another pileup_finish may follow (gact_hip_pileup_finish)"""
        if self._pileup is None:                      # (the sizes of the three arrays are the window's)
            raise GactHipError("gact_hip error -1: pileup_finish: no window is open (gact_hip_pileup_begin first)")
        n_reads, n_pos, _ = self._pileup
        reads = np.zeros(n_reads, dtype=READ_PILEUP_DTYPE)
        cnt = np.zeros((n_pos, 8), dtype=np.uint32) if counts else None
        cons = np.zeros(n_pos, dtype=np.uint8) if consensus else None
        self._check(self.L.gact_hip_pileup_finish(self.h, int(min_depth), _ptr(cnt), _ptr(cons), _ptr(reads)))
        return reads, cnt, cons

    def last_pileup_stats(self):
        """the pileup since pileup_begin: device ms of its adds and finishes (HIP events), adds, path-run chunks, alignments
        counted, their columns, the window's positions, device bytes the window holds"""
        return self._stats(self.L.gact_hip_last_pileup_stats, PileupStats)

    def pileup_corrected(self, min_depth=3, ins=False):
        """the corrected reads of the open window, spelled on the device: (reads READ_CORRECTED_DTYPE, read_at int64
        [n_reads + 1], seq bytes) -- read i is seq[read_at[i]:read_at[i + 1]]: for every position its emitted slots' bases,
        then its consensus byte unless that is '-' -- or, with `ins`, (reads, read_at, seq, ins uint32 [positions, ins_slots,
        4]), the slots' counts of A C G T; the counts stay (include/gact_hip.h gact_hip_pileup_corrected)"""
        if self._pileup is None:                      # (the sizes of the arrays are the window's)
            raise GactHipError("gact_hip error -1: pileup_corrected: no window is open (gact_hip_pileup_begin first)")
        n_reads, n_pos, slots = self._pileup
        reads = np.zeros(n_reads, dtype=READ_CORRECTED_DTYPE)
        read_at = np.zeros(n_reads + 1, dtype=np.int64)
        # (at least one word: a table asked of a window without slots is the library's to refuse, and it sees a pointer)
        table = np.zeros(max(n_pos * slots * 4, 1), dtype=np.uint32) if ins else None
        seq_len = C.c_int64()
        cap = n_pos + n_pos // 16                   # (positions * (ins_slots + 1) always suffices; few reads grow at all)
        for attempt in range(2):
            seq = np.zeros(max(cap, 1), dtype=np.uint8)
            rc = self.L.gact_hip_pileup_corrected(self.h, int(min_depth), table.ctypes.data if ins else None, _ptr(reads),
                                                  _ptr(read_at), seq.ctypes.data, cap, C.byref(seq_len))
            if rc == 0 or attempt or seq_len.value <= cap:
                break
            cap = seq_len.value                     # (EINVAL with *seq_len filled: once more with room for the bytes)
        self._check(rc)
        seq = seq[:seq_len.value].tobytes()
        return (reads, read_at, seq, table[:n_pos * slots * 4].reshape(n_pos, slots, 4)) if ins else (reads, read_at, seq)

    def last_pileup_ins_stats(self):
        """the slots since pileup_begin: device ms of the pileup_corrected calls (HIP events), ins_slots, adds to slots, runs
        longer than ins_slots, bases the last pileup_corrected put in, the table's bytes"""
        return self._stats(self.L.gact_hip_last_pileup_ins_stats, PileupInsStats)

    def pileup_variants(self, min_depth=VARIANT_DEFAULTS["min_depth"], min_alt=VARIANT_DEFAULTS["min_alt"],
                        min_permille=VARIANT_DEFAULTS["min_permille"], hom_permille=VARIANT_DEFAULTS["hom_permille"], table=False):
        """the variants of the open window, called from its counts on the device: VARIANT_DTYPE records ordered by seq, pos,
        kind (VARIANT_INS, _DEL, _SNV) and the SNV's base -- or, with `table`, (records, SEQ_VARIANTS_DTYPE [n_reads]).  A record
        exists where a >= min_alt reads and at least min_permille of the depth say so at a position of depth >= min_depth; its
        gt (flags & 3) is 2 from hom_permille of the depth on, else 1: thresholds of a stated rule, not likelihoods.  The counts
        stay (include/gact_hip.h gact_hip_pileup_variants)"""
        if self._pileup is None:                      # (the table's size is the window's)
            raise GactHipError("gact_hip error -1: pileup_variants: no window is open (gact_hip_pileup_begin first)")
        params = VariantParams(int(min_depth), int(min_alt), int(min_permille), int(hom_permille))
        seqs = np.zeros(self._pileup[0], dtype=SEQ_VARIANTS_DTYPE)
        n = C.c_int64(-1)
        cap = 1024                                  # (a guess; a window with more records says how many)
        for attempt in range(2):
            out = np.zeros(cap, dtype=VARIANT_DTYPE)
            rc = self.L.gact_hip_pileup_variants(self.h, C.byref(params), out.ctypes.data, cap, C.byref(n), _ptr(seqs))
            if rc == 0 or attempt or n.value <= cap:
                break
            cap = n.value                           # (EINVAL with *n_variants filled: once more with room for the records)
        self._check(rc)
        out = out[:n.value].copy()
        return (out, seqs) if table else out

    def last_variant_stats(self):
        """the last pileup_variants call: device ms (HIP events around the whole call), chunks, records per kind, examined
        positions, device bytes the pass holds"""
        return self._stats(self.L.gact_hip_last_variant_stats, VariantStats)

    def register_output(self, out, slot=0):
        """page-locks a caller-owned record array that will be fetched into repeatedly (opt-in; it must outlive the
        registration)"""
        assert out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        self._check(self.L.gact_hip_register_output(self.h, slot, out.ctypes.data, out.nbytes))
        self._registered[slot] = out               # (the array must not be collected while it is page-locked)

    def unregister_output(self, slot=0):
        self._check(self.L.gact_hip_unregister_output(self.h, slot))
        self._registered.pop(slot, None)

    def sync(self, slot=0):
        self._check(self.L.gact_hip_sync(self.h, slot))

    def prepare(self, expected_candidates=0):
        """arrays, second streams and empty launches ahead of the first job (include/gact_hip.h gact_hip_prepare)"""
        if hasattr(self.L, "gact_hip_prepare"):
            self.L.gact_hip_prepare.argtypes = [C.c_void_p, C.c_int32]
            self.L.gact_hip_prepare.restype = C.c_int
            self._check(self.L.gact_hip_prepare(self.h, int(expected_candidates)))

    def set_option(self, name, value):
        """scheduling switches of a live engine: "overlap_seed", "combine", "combine_window_us" (include/gact_hip.h)"""
        if hasattr(self.L, "gact_hip_set_option"):
            self._check(self.L.gact_hip_set_option(self.h, name.encode(), int(value)))

    # ---- D-SOFT on the device
    def dsoft_build(self, params=None):
        """minimizer index over the uploaded SET_REF (seed_pos_table.cpp:46-98)"""
        params = params or DsoftParams()
        info = DsoftInfo()
        self._check(self.L.gact_hip_dsoft_build(self.h, C.byref(params), C.byref(info)))
        return {n: getattr(info, n) for n, _ in DsoftInfo._fields_}

    def dsoft_query(self, first_query, n_queries, slot=0):
        """filters queries [first, first+n) of SET_QUERY / SET_QUERY_RC; the slot's device candidate array then
        holds the forward candidates followed by the reverse-complement ones.  Returns (n_forward, n_reverse, ms)."""
        nf, nr, ms = C.c_int32(), C.c_int32(), C.c_float()
        self._check(self.L.gact_hip_dsoft_query(self.h, slot, first_query, n_queries, C.byref(nf), C.byref(nr),
                                                C.byref(ms)))
        self._n_cands[slot] = nf.value + nr.value
        return nf.value, nr.value, float(ms.value)

    def candidates_download(self, n, slot=0):
        out = np.zeros(n, dtype=CAND_DTYPE)
        self._check(self.L.gact_hip_candidates_download(self.h, slot, n, out.ctypes.data))
        return out

    def last_kernel_ms(self, slot=0):
        ms = C.c_float()
        self._check(self.L.gact_hip_last_kernel_ms(self.h, slot, C.byref(ms)))
        return float(ms.value)

    def last_run_stats(self, slot=0):
        st = RunStats()
        self._check(self.L.gact_hip_last_run_stats(self.h, slot, C.byref(st)))
        if st.band_redos & (1 << 30):
            raise GactHipError("the role launch's watchdog fired: a DP wave went on without its walker's results (records are wrong)")
        return {"total_ms": st.total_ms, "seed_ms": st.seed_ms, "main_ms": st.main_ms,
                "packed16": bool(st.packed16), "layout": ("int32", "packed16-uniform", "packed16-split", "packed16-wide")[st.packed16],
                "seed_layout": "packed16" if st.seed_packed16 else "int32",
                "tagged_pointers": bool(st.tagged_pointers), "linear_gap": st.linear_gap in (1, 3), "lin_row_drift": st.linear_gap == 3, "affine_drift": st.linear_gap == 2,
                "handed_off": st.handed_off, "seed_cells": st.seed_cells, "raw_candidates": st.raw_candidates,
                "band_redos": st.band_redos, "merged_callers": st.merged_callers, "overlapped_seeding": bool(st.overlapped_seeding),
                "critical_lane": bool(st.critical_lane), "role_waves": st.role_waves == 1, "coop_walks": st.role_waves == 2}

    def measure_valu_rate(self):
        v = C.c_double()
        self._check(self.L.gact_hip_measure_valu_rate(self.h, C.byref(v)))
        return float(v.value)

    def scratch_fills(self):
        """(fills, bytes) of GACT_HIP_POISON_SCRATCH since the engine was made: how often a pass's scratch, a path buffer or a
        newly opened pileup window was filled with seeded garbage, and the bytes that covered; (0, 0) with the switch unset"""
        fills, nbytes = C.c_int64(), C.c_int64()
        self._check(self.L.gact_hip_scratch_fills(self.h, C.byref(fills), C.byref(nbytes)))
        return int(fills.value), int(nbytes.value)

    def device_overlaps_ptr(self, slot=0):
        return self.L.gact_hip_device_overlaps(self.h, slot)

    def format_overlap(self, rec, ref_name, query_name):
        rec = np.ascontiguousarray(rec, dtype=OVERLAP_DTYPE)
        buf = C.create_string_buffer(512)
        n = self._check(self.L.gact_hip_format_overlap(rec.ctypes.data, ref_name.encode(), query_name.encode(),
                                                       buf, 512))
        return buf.raw[:n].decode()


def format_paf(rec, summary, query_name, query_len, ref_name, ref_len, cap=1024):
    """one PAF line for a record and its summary (include/gact_hip.h gact_hip_format_paf; no engine, no device)"""
    L = load()
    rec = np.ascontiguousarray(rec, dtype=OVERLAP_DTYPE)
    summary = np.ascontiguousarray(summary, dtype=SUMMARY_DTYPE)
    buf = C.create_string_buffer(cap)
    n = L.gact_hip_format_paf(rec.ctypes.data, summary.ctypes.data, query_name.encode(), int(query_len), ref_name.encode(),
                              int(ref_len), buf, cap)
    if n < 0:
        raise GactHipError("gact_hip error %d: %s" % (n, L.gact_hip_last_error().decode()))
    return buf.raw[:min(n, cap - 1)].decode()


def _sam_line(call):
    """call(buf, cap) -> the line: once with a guessed room, once more with what the first call said it needs"""
    L = load()
    cap = 4096
    for _ in range(2):
        buf = C.create_string_buffer(cap)
        n = call(L, buf, cap)
        if n < 0:
            raise GactHipError("gact_hip error %d: %s" % (n, L.gact_hip_last_error().decode()))
        if n < cap:
            return buf.raw[:n].decode()
        cap = int(n) + 1


def _seq_bytes(seq):
    """a read as a contiguous uint8 array: str, bytes or an array of bytes"""
    if isinstance(seq, str):
        seq = seq.encode()
    if isinstance(seq, (bytes, bytearray)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.ascontiguousarray(seq, dtype=np.uint8)


def format_sam(rec, ops, place, query_name, query_seq, ref_name):
    """one SAM line for a record, its op words (candidates_paths) and its PLACE_DTYPE record; query_seq: the ORIGINAL read,
    bytes or uint8 (include/gact_hip.h gact_hip_format_sam; no engine, no device)"""
    rec = np.ascontiguousarray(rec, dtype=OVERLAP_DTYPE)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    place = np.ascontiguousarray(place, dtype=PLACE_DTYPE)
    seq = _seq_bytes(query_seq)
    return _sam_line(lambda L, buf, cap: L.gact_hip_format_sam(rec.ctypes.data, ops.ctypes.data, len(ops), place.ctypes.data,
                                                               query_name.encode(), seq.ctypes.data, len(seq), ref_name.encode(),
                                                               buf, cap))


def format_vcf(variant, seq_name, seq):
    """one VCF line for a VARIANT_DTYPE record and the sequence it lies on (bytes or uint8); "" for a deletion of the whole
    sequence (include/gact_hip.h gact_hip_format_vcf; no engine, no device)"""
    v = np.ascontiguousarray(variant, dtype=VARIANT_DTYPE)
    seq = _seq_bytes(seq)
    return _sam_line(lambda L, buf, cap: L.gact_hip_format_vcf(v.ctypes.data, seq_name.encode(), seq.ctypes.data, len(seq), buf, cap))


def format_sam_unmapped(query_name, query_seq):
    """the flag-4 SAM line of a read without a placement (include/gact_hip.h gact_hip_format_sam_unmapped)"""
    seq = _seq_bytes(query_seq)
    return _sam_line(lambda L, buf, cap: L.gact_hip_format_sam_unmapped(query_name.encode(), seq.ctypes.data, len(seq), buf, cap))


class Comm:
    """The C-ABI's own RCCL gather (include/gact_hip.h gact_hip_comm_*; csrc/gact_gather.hpp): what host/darwin_hip
    --rccl-gather and any C caller use where bench.py uses torch.distributed.  Collective calls: every rank makes them."""

    LINE_DTYPE = np.dtype([(n, "<i4") for n in ("ref_id", "query_id", "ab", "ae", "bb", "be", "score", "comp_emitted")])

    def __init__(self, eng, rank, world, id_path, timeout_s=120):
        self.eng, self.rank, self.world = eng, rank, world
        self.h = C.c_void_p()
        eng._check(eng.L.gact_hip_comm_create(eng.h, rank, world, id_path.encode(), int(timeout_s), C.byref(self.h)))

    def gather_lines(self, n, slot=0, room=None):
        """the first n records of `slot`, as 32-byte lines, to rank 0: (counts per rank, lines on rank 0 / None elsewhere)"""
        counts = np.zeros(self.world, dtype=np.int64)
        cap = int(room if room is not None else (n + 1) * self.world) if self.rank == 0 else 0
        lines = np.zeros(cap, dtype=self.LINE_DTYPE) if self.rank == 0 else None
        self.eng._check(self.eng.L.gact_hip_comm_gather_lines(self.h, slot, int(n), counts.ctypes.data,
                                                              lines.ctypes.data if lines is not None else None, cap))
        return counts, (lines[:int(counts.sum())] if lines is not None else None)

    def close(self):
        if self.h:
            self.eng.L.gact_hip_comm_destroy(self.h)
            self.h = C.c_void_p()


def queue_from_tile(result, states, first):
    """The std::queue<int> AlignWithBT would return (align.cpp:190-199), as a list."""
    n = int(result["n_states"])
    st = [int(x) for x in states[:n]]
    if first:
        return [int(result["score"]), int(result["max_i"]), int(result["max_j"])] + st
    return [int(result["score"])] + st
