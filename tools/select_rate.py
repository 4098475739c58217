"""What the selection (gact_hip_select_overlaps) costs and yields on ecoli10x, on one GPU, in one process:
  (a) the normal run over all candidates (HIP events, gact_hip_last_run_stats),
  (x) / (p) the exact / pair selection over the run's device-resident records (HIP events around the whole call,
      gact_hip_last_select_stats), both checked against the model on the fetched records,
  (s) the summaries call over every emitted candidate and (t) over the pair selection (gact_hip_last_summaries_stats).
Each leg is warmed up; the legs alternate --reps times.  Prints one JSON line: medians with min and max, the counts, and the
ratios.  Usage: python tools/select_rate.py [--workload ecoli10x] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "darwin-gpu_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ecoli10x")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from gact_amd import engine, workload
    import select_model
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
    ms = {k: [] for k in ("a_normal_run", "x_select_exact", "p_select_pair", "s_summaries_emitted", "t_summaries_pair")}
    for rep in range(args.reps + 1):
        eng.candidates_run_mixed(n, nf)
        exact = eng.select_overlaps(n=n, mode="exact")
        x_ms = eng.last_select_stats()["device_ms"]
        pair = eng.select_overlaps(n=n, mode="pair")
        st = eng.last_select_stats()
        rec = eng.candidates_fetch(n)
        run_ms = eng.last_run_stats()["total_ms"]
        emitted = np.flatnonzero(rec["emitted"]).astype(np.int32)
        eng.candidates_summaries(sel=emitted, rc_from=nf)
        s_ms = eng.last_summaries_stats()["device_ms"]
        eng.candidates_summaries(sel=pair, rc_from=nf)
        t_ms = eng.last_summaries_stats()["device_ms"]
        if rep:                                    # (the first round is the warm-up)
            for k, v in zip(ms, (run_ms, x_ms, st["device_ms"], s_ms, t_ms)):
                ms[k].append(v)
    assert exact.tolist() == select_model.select(rec, "exact").tolist()
    assert pair.tolist() == select_model.select(rec, "pair").tolist()
    assert st["emitted"] == len(emitted) and st["selected"] == len(pair)
    eng.close()
    out = {"workload": args.workload, "reps": args.reps, "candidates": n, "emitted": int(len(emitted)), "exact": int(len(exact)),
           "pair": int(len(pair)), "table_slots": st["table_slots"], "scratch_bytes": st["scratch_bytes"]}
    for k, v in ms.items():
        a = np.array(v)
        out[k] = {"ms_median": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max())}
    med = lambda k: out[k]["ms_median"]
    out["p_over_a"] = med("p_select_pair") / med("a_normal_run")
    out["t_over_s"] = med("t_summaries_pair") / med("s_summaries_emitted")
    out["pair_over_emitted"] = len(pair) / max(1, len(emitted))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
