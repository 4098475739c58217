"""What the path run (gact_hip_candidates_paths) and the summary run (gact_hip_candidates_summaries) cost on ecoli10x, on one GPU:
  (a) the normal run over all candidates (default kernels; HIP events, gact_hip_last_run_stats),
  (b) the path run over every emitted candidate (HIP events around the whole call, gact_hip_last_paths_stats: chain
      kernel, compaction, copies, the host's scan between them), and (b') the same call without room for the ops (chain
      kernel, op count, records back: no op write, no op copy),
  (s) the summary run over the same selection (HIP events around the whole call, gact_hip_last_summaries_stats: chain
      kernel, records and summaries back), checked against the reduction of (b)'s ops,
  (c) the int32 chain kernel alone (GACT_HIP_FORCE_INT32, an engine of its own) over the same selection (HIP events).
Each leg is warmed up; (b), (b'), (s) and (c) alternate --reps times.  The column budget is the engine's
(GACT_HIP_PATH_BUDGET_MB, default 1024 MiB) and is printed with the chunks it made.  Prints ms and GCUPS (cells of the
selection's records) per leg, the spread, and (b) / (c), (b) / (a), (s) / (b) and (s) / (c).  Usage: python tools/path_rate.py [--workload ecoli10x] [--reps 5]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "darwin-gpu_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ecoli10x")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from gact_amd import engine, workload
    blk = workload.make_block(args.workload)
    rs = blk.rs
    cat, offs = rs.concat()
    rcat, _ = rs.concat(rc=True)

    def make(cands, env=None):
        if env:
            os.environ.update(env)
        try:
            eng = engine.Engine()
        finally:
            for k in (env or {}):
                os.environ.pop(k, None)
        eng.upload(engine.SET_REF, cat, offs)
        eng.upload(engine.SET_QUERY, cat, offs)
        eng.upload(engine.SET_QUERY_RC, rcat, offs)
        eng.candidates_upload(cands)
        return eng

    cands = np.concatenate([blk.cf, blk.cr]).astype(engine.CAND_DTYPE)
    n, nf = len(cands), len(blk.cf)
    eng = make(cands)
    normal_ms = []
    for rep in range(args.reps + 1):
        eng.candidates_run_mixed(n, nf)
        rec = eng.candidates_fetch(n)
        if rep:
            normal_ms.append(eng.last_run_stats()["total_ms"])
    all_cells = int(rec["cells"].sum())
    sel = np.flatnonzero(rec["emitted"]).astype(np.int32)
    sel_cells = int(rec["cells"][sel].sum())
    # (c)'s own list: the selection, forward strand first
    sub = cands[sel]
    sub_nf = int((sel < nf).sum())
    eng32 = make(sub, {"GACT_HIP_FORCE_INT32": "1"})
    eng.candidates_paths(sel=sel, rc_from=nf)                # warm-up
    eng.candidates_summaries(sel=sel, rc_from=nf)
    eng32.candidates_run_mixed(len(sub), sub_nf)
    eng32.candidates_fetch(len(sub))
    path_ms, int32_ms, noops_ms, sum_ms = [], [], [], []
    r_buf, p_buf, needed = np.zeros(len(sel), engine.OVERLAP_DTYPE), np.zeros(len(sel), engine.PATH_DTYPE), ctypes.c_int64()
    for _ in range(args.reps):
        prec, paths, ops = eng.candidates_paths(sel=sel, rc_from=nf)
        st = eng.last_paths_stats()
        path_ms.append(st["device_ms"])
        # (b') the same without the ops: chain kernel, op count, records and counts back -- no op write, no op copy
        eng.L.gact_hip_candidates_paths(eng.h, 0, len(sel), sel.ctypes.data, nf, 1, r_buf.ctypes.data, p_buf.ctypes.data,
                                        None, 0, ctypes.byref(needed))
        noops_ms.append(eng.last_paths_stats()["device_ms"])
        srec, sums = eng.candidates_summaries(sel=sel, rc_from=nf)
        sst = eng.last_summaries_stats()
        sum_ms.append(sst["device_ms"])
        eng32.candidates_run_mixed(len(sub), sub_nf)
        r32 = eng32.candidates_fetch(len(sub))
        int32_ms.append(eng32.last_run_stats()["total_ms"])
    assert prec.tobytes() == rec[sel].tobytes() and r32.tobytes() == rec[sel].tobytes()
    # the summaries against the reduction of the path run's ops (vectorised engine.summarise)
    assert srec.tobytes() == rec[sel].tobytes()
    owner = np.repeat(np.arange(len(sel)), paths["n_ops"])
    for op, cols, runs in ((engine.OP_EQ, "n_eq", "eq_runs"), (engine.OP_X, "n_x", "x_runs"), (engine.OP_I, "ins_bases", "ins_runs"),
                           (engine.OP_D, "del_bases", "del_runs")):
        mine = (ops & 15) == op
        assert np.array_equal(np.bincount(owner[mine], weights=(ops >> 4)[mine], minlength=len(sel)).astype(np.int64), sums[cols])
        assert np.array_equal(np.bincount(owner[mine], minlength=len(sel)), sums[runs])
    eng.close()
    eng32.close()

    def leg(ms, cells):
        a = np.array(ms)
        return {"ms_median": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max()),
                "gcups": cells / (float(np.median(a)) * 1e-3) / 1e9}

    out = {"workload": args.workload, "candidates": n, "emitted": int(len(sel)), "reps": args.reps,
           "a_normal_run": leg(normal_ms, all_cells), "b_path_run": leg(path_ms, sel_cells),
           "c_int32_run": leg(int32_ms, sel_cells), "b_without_ops": leg(noops_ms, sel_cells),
           "s_summary_run": leg(sum_ms, sel_cells), "summary_launches": sst["launches"], "summary_scratch_bytes": sst["scratch_bytes"],
           "budget_mb": int(os.environ.get("GACT_HIP_PATH_BUDGET_MB", "1024")), "chunks": st["chunks"], "ops": int(len(ops)),
           "columns": int(paths["n_columns"].sum())}
    out["b_over_c"] = out["b_path_run"]["ms_median"] / out["c_int32_run"]["ms_median"]
    out["b_over_a"] = out["b_path_run"]["ms_median"] / out["a_normal_run"]["ms_median"]
    out["s_over_b"] = out["s_summary_run"]["ms_median"] / out["b_path_run"]["ms_median"]
    out["s_over_c"] = out["s_summary_run"]["ms_median"] / out["c_int32_run"]["ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
