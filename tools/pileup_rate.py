"""What the per-base pileup (gact_hip_pileup_begin / _add / _finish) costs beside the path run it replaces the host side of, on
one GPU, in one process, for one selection of a workload's candidates (--select emitted: every emitted record; pair: the pair
selection of gact_hip_select_overlaps):
  (p) gact_hip_candidates_paths over the selection: the CIGARs on the host (HIP events, gact_hip_last_paths_stats),
  (u) one gact_hip_pileup_add over the same selection plus one gact_hip_pileup_finish with the consensus and the read table
      copied out (gact_hip_last_pileup_stats: the add's and the finish's events together; the add's alone is reported too),
  (m) the host-side numpy model (tests/pileup_model.py) over the ops of the first --model-records records of the selection,
      once, wall clock, checked against a pileup of those records alone -- the thing the feature replaces; scaled by columns
      to the whole selection where it ran over a part.
Each device leg is warmed up once; the legs alternate --reps times.  Prints one JSON line.
The model is the test suite's: this tool puts tests/ on sys.path to import it, so it runs from a source tree that has tests/.
Usage: python tools/pileup_rate.py [--workload ecoli10x] [--select pair] [--reps 3] [--model-records 300]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "darwin-gpu_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ecoli10x")
    ap.add_argument("--select", default="pair", choices=["pair", "emitted"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-depth", type=int, default=3)
    ap.add_argument("--model-records", type=int, default=300)
    args = ap.parse_args()
    from gact_amd import engine, workload
    import pileup_model
    blk = workload.make_block(args.workload)
    cat, offs = blk.rs.concat()
    rcat, _ = blk.rs.concat(rc=True)
    eng = engine.Engine()
    eng.upload(engine.SET_REF, cat, offs)
    eng.upload(engine.SET_QUERY, cat, offs)
    eng.upload(engine.SET_QUERY_RC, rcat, offs)
    cands = np.concatenate([blk.cf, blk.cr]).astype(engine.CAND_DTYPE)
    n, nf = len(cands), len(blk.cf)
    eng.candidates_upload(cands)
    eng.candidates_run_mixed(n, nf)
    rec = eng.candidates_fetch(n)
    run_ms = eng.last_run_stats()["total_ms"]
    sel = eng.select_overlaps(n=n, mode="pair") if args.select == "pair" else np.flatnonzero(rec["emitted"]).astype(np.int32)
    ms = {"p_paths": [], "u_pileup_add_and_finish": [], "u_pileup_add": []}
    for rep in range(args.reps + 1):
        records, paths, ops = eng.candidates_paths(sel=sel, rc_from=nf, ops_cap=None if rep == 0 else len(ops))
        p_ms = eng.last_paths_stats()["device_ms"]
        eng.pileup_begin()
        eng.pileup_add(sel=sel, rc_from=nf)
        add_ms = eng.last_pileup_stats()["device_ms"]
        reads, _, cons = eng.pileup_finish(min_depth=args.min_depth, counts=False)
        st = eng.last_pileup_stats()
        if rep:                                    # (the first round is the warm-up)
            ms["p_paths"].append(p_ms)
            ms["u_pileup_add_and_finish"].append(st["device_ms"])
            ms["u_pileup_add"].append(add_ms)
    # the model over the first records of the selection, and the device's pileup of those alone
    m = min(args.model_records, len(sel)) if args.model_records > 0 else len(sel)
    rc_reads = {}

    class Rc:
        def __getitem__(self, i):
            if i not in rc_reads:
                rc_reads[i] = blk.rs.rc(i)
            return rc_reads[i]

    part_ops = [ops[paths[k]["op_offset"]:paths[k]["op_offset"] + paths[k]["n_ops"]] for k in range(m)]
    t0 = time.perf_counter()
    want = pileup_model.pileup(blk.rs.reads, Rc(), records[:m], part_ops, (0, len(blk.rs.reads)), args.min_depth)
    model_s = time.perf_counter() - t0
    eng.pileup_begin()
    eng.pileup_add(sel=sel[:m], rc_from=nf)
    got = eng.pileup_finish(min_depth=args.min_depth)
    part_columns = eng.last_pileup_stats()["columns"]
    eng.close()
    assert np.array_equal(got[1], want[0]) and got[2].tobytes() == want[1].tobytes() and got[0].tobytes() == want[2].tobytes()
    out = {"workload": args.workload, "select": args.select, "reps": args.reps, "min_depth": args.min_depth, "candidates": n,
           "selected": int(len(sel)), "normal_run_ms": run_ms, "alignments": st["alignments"], "columns": st["columns"],
           "positions": st["positions"], "chunks": st["chunks"], "scratch_bytes": st["scratch_bytes"], "ops": int(len(ops)),
           "max_depth": int(reads["max_depth"].max()), "called": int(reads["called"].sum()), "changed": int(reads["changed"].sum()),
           "deleted": int(reads["deleted"].sum()), "ins_flagged": int(reads["ins_flagged"].sum()),
           "model_records": m, "model_columns": part_columns, "model_wall_s": model_s,
           "model_wall_s_scaled_to_the_selection": model_s * st["columns"] / max(part_columns, 1)}
    for k, v in ms.items():
        a = np.array(v)
        out[k] = {"ms_median": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max())}
    out["add_over_paths"] = out["u_pileup_add"]["ms_median"] / out["p_paths"]["ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
