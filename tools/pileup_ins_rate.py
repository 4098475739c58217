"""What the inserted bases of the pileup cost (gact_hip_pileup_begin_ins / gact_hip_pileup_corrected), on one GPU, in one
process, on the pair selection of a workload's candidates:
  (a0) one gact_hip_pileup_add into a window without slots -- the kernel a window has always run,
  (a0-other) the same through another build of the library (--other-lib PATH, e.g. the parent commit's), on an engine of its
       own in this process, so that the two alternate call by call,
  (aK) one gact_hip_pileup_add into a window with --ins-slots slots,
  (c0, cK) one gact_hip_pileup_corrected on either window, the bytes, read_at and the read table copied out, the slot table not
       (gact_hip_last_pileup_ins_stats).
Add times are gact_hip_last_pileup_stats' device_ms (HIP events around the add).  One warm-up round, then --reps rounds in which
the legs alternate.  The two builds' counts and consensus are compared byte for byte.  Prints one JSON line.
Usage: python tools/pileup_ins_rate.py [--workload ecoli10x] [--reps 5] [--ins-slots 2] [--other-lib PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "darwin-gpu_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ecoli10x")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-depth", type=int, default=3)
    ap.add_argument("--ins-slots", type=int, default=2)
    ap.add_argument("--other-lib", default=None)
    args = ap.parse_args()
    from gact_amd import engine, workload
    blk = workload.make_block(args.workload)
    cat, offs = blk.rs.concat()
    rcat, _ = blk.rs.concat(rc=True)
    cands = np.concatenate([blk.cf, blk.cr]).astype(engine.CAND_DTYPE)
    n, nf = len(cands), len(blk.cf)

    def engine_of(lib_path):
        if lib_path:                                # (the library is read once per load: load again for this engine)
            os.environ["GACT_HIP_LIB_PATH"] = lib_path
        else:
            os.environ.pop("GACT_HIP_LIB_PATH", None)
        engine._lib = None
        eng = engine.Engine()
        eng.upload(engine.SET_REF, cat, offs)
        eng.upload(engine.SET_QUERY, cat, offs)
        eng.upload(engine.SET_QUERY_RC, rcat, offs)
        eng.candidates_upload(cands)
        eng.candidates_run_mixed(n, nf)
        return eng

    default_lib = engine.LIB_PATH
    other = engine_of(os.path.abspath(args.other_lib)) if args.other_lib else None
    engine.LIB_PATH = default_lib
    eng = engine_of(None)
    sel = eng.select_overlaps(n=n, mode="pair")
    ms = {"a0_add": [], "a0_add_other": [], "aK_add": [], "c0_corrected": [], "cK_corrected": []}
    out = {}
    for rep in range(args.reps + 1):
        row = {}
        if other is not None:
            other.pileup_begin()
            other.pileup_add(sel=sel, rc_from=nf)
            row["a0_add_other"] = other.last_pileup_stats()["device_ms"]
        eng.pileup_begin()
        eng.pileup_add(sel=sel, rc_from=nf)
        row["a0_add"] = eng.last_pileup_stats()["device_ms"]
        plain = eng.pileup_corrected(min_depth=args.min_depth)
        row["c0_corrected"] = eng.last_pileup_ins_stats()["device_ms"]
        if other is not None and rep == 0:
            mine, theirs = eng.pileup_finish(min_depth=args.min_depth), other.pileup_finish(min_depth=args.min_depth)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(mine, theirs)), "the two builds' pileups differ"
        eng.pileup_begin(ins_slots=args.ins_slots)
        eng.pileup_add(sel=sel, rc_from=nf)
        row["aK_add"] = eng.last_pileup_stats()["device_ms"]
        st = eng.last_pileup_stats()
        slotted = eng.pileup_corrected(min_depth=args.min_depth)
        ist = eng.last_pileup_ins_stats()
        row["cK_corrected"] = ist["device_ms"]
        if rep:                                    # (the first round is the warm-up)
            for k, v in row.items():
                ms[k].append(v)
    out.update(workload=args.workload, reps=args.reps, min_depth=args.min_depth, ins_slots=args.ins_slots, candidates=n,
               selected=int(len(sel)), alignments=st["alignments"], columns=st["columns"], positions=st["positions"],
               scratch_bytes=st["scratch_bytes"], table_bytes=ist["table_bytes"], slot_adds=ist["slot_adds"],
               runs_truncated=ist["runs_truncated"], inserted=ist["emitted"], bases_without_slots=len(plain[2]),
               bases_with_slots=len(slotted[2]), deleted=int(slotted[0]["deleted"].sum()), changed=int(slotted[0]["changed"].sum()))
    for k, v in ms.items():
        if v:
            a = np.array(v)
            out[k] = {"ms": [round(float(x), 3) for x in a], "ms_median": float(np.median(a)), "ms_min": float(a.min()),
                      "ms_max": float(a.max())}
    eng.close()
    if other is not None:
        other.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
