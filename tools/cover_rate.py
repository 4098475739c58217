"""What the per-read coverage (gact_hip_read_coverage) costs on ecoli10x, on one GPU, in one process:
  (a) the normal run over all candidates (HIP events, gact_hip_last_run_stats),
  (c) the coverage of every read over the run's device-resident records, both sides, min_depth 3 (HIP events around the whole
      call, gact_hip_last_cover_stats) and (d) the same with the per-base depth copied out,
  (p) the coverage over the pair selection of gact_hip_select_overlaps,
each checked against the model (tests/cover_model.py) on the fetched records.  Each leg is warmed up; the legs alternate --reps
times.  Prints one JSON line: medians with min and max, the read, interval and position counts, and the ratios to the run.
Usage: python tools/cover_rate.py [--workload ecoli10x] [--reps 5]"""
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
    ap.add_argument("--min-depth", type=int, default=3)
    args = ap.parse_args()
    from gact_amd import engine, workload
    import cover_model
    blk = workload.make_block(args.workload)
    cat, offs = blk.rs.concat()
    rcat, _ = blk.rs.concat(rc=True)
    lens = np.diff(offs).astype(np.int32)
    eng = engine.Engine()
    eng.upload(engine.SET_REF, cat, offs)
    eng.upload(engine.SET_QUERY, cat, offs)
    eng.upload(engine.SET_QUERY_RC, rcat, offs)
    cands = np.concatenate([blk.cf, blk.cr]).astype(engine.CAND_DTYPE)
    n, nf = len(cands), len(blk.cf)
    eng.candidates_upload(cands)
    ms = {k: [] for k in ("a_normal_run", "c_cover", "d_cover_with_depth", "p_cover_pair")}
    for rep in range(args.reps + 1):
        eng.candidates_run_mixed(n, nf)
        table = eng.read_coverage(lens, n=n, min_depth=args.min_depth)
        st = eng.last_cover_stats()
        table_d, depth = eng.read_coverage(lens, n=n, min_depth=args.min_depth, depth=True)
        st_d = eng.last_cover_stats()
        pair = eng.select_overlaps(n=n, mode="pair")
        table_p = eng.read_coverage(lens, n=n, sel=pair, min_depth=args.min_depth)
        st_p = eng.last_cover_stats()
        rec = eng.candidates_fetch(n)
        run_ms = eng.last_run_stats()["total_ms"]
        if rep:                                    # (the first round is the warm-up)
            for k, v in zip(ms, (run_ms, st["device_ms"], st_d["device_ms"], st_p["device_ms"])):
                ms[k].append(v)
        else:                                      # (the model once: the device's answer is the same on every round, see below)
            want, want_depth = cover_model.cover(rec, lens, min_depth=args.min_depth)
            want_p, _ = cover_model.cover(rec, lens, sel=pair, min_depth=args.min_depth)
        assert table.tobytes() == table_d.tobytes() == want.tobytes() and depth.tobytes() == want_depth.tobytes()
        assert table_p.tobytes() == want_p.tobytes()
        assert st["intervals"] == int(want["n_intervals"].sum()) and st_p["intervals"] == int(want_p["n_intervals"].sum())
    eng.close()
    span = want["span_end"] - want["span_begin"]
    out = {"workload": args.workload, "reps": args.reps, "min_depth": args.min_depth, "candidates": n,
           "emitted": int(rec["emitted"].sum()), "pair": int(len(pair)), "reads": st["reads"], "positions": st["positions"],
           "intervals": st["intervals"], "intervals_pair": st_p["intervals"], "scratch_bytes": st["scratch_bytes"],
           "scratch_bytes_with_depth": st_d["scratch_bytes"], "median_depth": float(np.median(depth)), "max_depth": int(want["max_depth"].max()),
           "reads_with_span": int((span > 0).sum()), "span_is_whole_read": int((span == lens).sum())}
    for k, v in ms.items():
        a = np.array(v)
        out[k] = {"ms_median": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max())}
    med = lambda k: out[k]["ms_median"]
    out["c_over_a"] = med("c_cover") / med("a_normal_run")
    out["d_over_a"] = med("d_cover_with_depth") / med("a_normal_run")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
