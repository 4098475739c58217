"""What the overlap graph (gact_hip_overlap_graph) costs on ecoli10x, on one GPU, in one process, beside the calls that feed it:
  (a) the normal run over all candidates (HIP events, gact_hip_last_run_stats),
  (s) the pair selection over the run's device-resident records (gact_hip_last_select_stats),
  (c) the coverage over that selection with its summaries, min_depth 3 (gact_hip_last_cover_stats),
  (g) the graph over the same selection and summaries, whole reads, and (k) the same clipped to the coverage's spans
      (HIP events around the whole call, gact_hip_last_graph_stats),
each graph checked against the model (tests/graph_model.py) on the fetched records.  Each leg is warmed up; the legs alternate
--reps times.  Prints one JSON line: medians with min and max, and the counts of both graphs.
Usage: python tools/graph_rate.py [--workload ecoli10x] [--reps 5]"""
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
    import graph_model
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
    ms = {k: [] for k in ("a_normal_run", "s_select_pair", "c_cover_pair", "g_graph", "k_graph_clipped")}
    for rep in range(args.reps + 1):
        eng.candidates_run_mixed(n, nf)
        pair = eng.select_overlaps(n=n, mode="pair")
        st_s = eng.last_select_stats()
        _, sums = eng.candidates_summaries(sel=pair, rc_from=nf)
        cover = eng.read_coverage(lens, n=n, sel=pair, sums=sums, min_depth=args.min_depth)
        st_c = eng.last_cover_stats()
        clip = np.stack([cover["span_begin"], cover["span_end"]], axis=1).astype(np.int32)
        got_g = eng.overlap_graph(lens, n=n, sel=pair, sums=sums, classes=True)
        st_g = eng.last_graph_stats()
        got_k = eng.overlap_graph(lens, n=n, sel=pair, sums=sums, clip=clip, classes=True)
        st_k = eng.last_graph_stats()
        rec = eng.candidates_fetch(n)
        run_ms = eng.last_run_stats()["total_ms"]
        if rep:                                    # (the first round is the warm-up)
            for k, v in zip(ms, (run_ms, st_s["device_ms"], st_c["device_ms"], st_g["device_ms"], st_k["device_ms"])):
                ms[k].append(v)
        else:                                      # (the model once: the device's answer is the same on every round, see below)
            want_g = graph_model.graph(rec, lens, sel=pair, sums=sums)
            want_k = graph_model.graph(rec, lens, sel=pair, sums=sums, clip=clip)
        for got, want in ((got_g, want_g), (got_k, want_k)):
            assert all(g.tobytes() == want[name].tobytes() for name, g in zip(("reads", "arcs", "classes"), got))
    eng.close()
    out = {"workload": args.workload, "reps": args.reps, "min_depth": args.min_depth, "candidates": n,
           "emitted": int(rec["emitted"].sum()), "pair": int(len(pair)), "reads": int(len(lens)),
           "max_out_degree": int(want_g["reads"]["deg"].max()), "max_out_degree_clipped": int(want_k["reads"]["deg"].max())}
    for name, st in (("graph", st_g), ("graph_clipped", st_k)):
        out[name] = {k: v for k, v in st.items() if k != "device_ms"}
    for k, v in ms.items():
        a = np.array(v)
        out[k] = {"ms_median": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
