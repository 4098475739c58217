"""What the unitigs (gact_hip_unitigs) cost on ecoli10x, on one GPU, in one process, behind the calls that feed them: the normal
run over all candidates, the pair selection, its summaries, the coverage (min_depth 3), the overlap graph clipped to the
coverage's spans -- the setup of tools/graph_rate.py -- and then
  (k) the graph call itself, the yardstick (HIP events around the whole call, gact_hip_last_graph_stats),
  (u) the unitigs without bases and (b) with bases, tip_reads 3 (HIP events around the whole call, gact_hip_last_unitig_stats),
each unitig result checked against the model (tests/unitig_model.py) on the graph the device returned, the model's wall clock
taken once.  One warm-up round, then --reps rounds.  Prints one JSON line: medians with min and max, the ranking launches, and
the counts (unitigs, circular, cut reads, the longest unitig, the N50 of the lengths).
Usage: python tools/unitig_rate.py [--workload ecoli10x] [--reps 5] [--tip-reads 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "darwin-gpu_amd"), os.path.join(ROOT, "tests")]


def n50(lengths):
    a = np.sort(np.asarray(lengths, dtype=np.int64))[::-1]
    return int(a[np.searchsorted(np.cumsum(a), (a.sum() + 1) // 2)]) if len(a) else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ecoli10x")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-depth", type=int, default=3)
    ap.add_argument("--tip-reads", type=int, default=3)
    args = ap.parse_args()
    from gact_amd import engine, workload
    import unitig_model
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
    ms = {k: [] for k in ("k_graph_clipped", "u_unitigs", "b_unitigs_bases")}
    for rep in range(args.reps + 1):
        eng.candidates_run_mixed(n, nf)
        pair = eng.select_overlaps(n=n, mode="pair")
        _, sums = eng.candidates_summaries(sel=pair, rc_from=nf)
        cover = eng.read_coverage(lens, n=n, sel=pair, sums=sums, min_depth=args.min_depth)
        clip = np.stack([cover["span_begin"], cover["span_end"]], axis=1).astype(np.int32)
        reads, arcs = eng.overlap_graph(lens, n=n, sel=pair, sums=sums, clip=clip)
        st_k = eng.last_graph_stats()
        got_u = eng.unitigs(lens, reads, arcs, clip=clip, tip_reads=args.tip_reads)
        st_u = eng.last_unitig_stats()
        got_b = eng.unitigs(lens, reads, arcs, clip=clip, tip_reads=args.tip_reads, seq=True)
        st_b = eng.last_unitig_stats()
        if rep:                                    # (the first round is the warm-up)
            for k, v in zip(ms, (st_k["device_ms"], st_u["device_ms"], st_b["device_ms"])):
                ms[k].append(v)
        else:                                      # (the model once: the device's answer is the same on every round, see below)
            t0 = time.perf_counter()
            want = unitig_model.unitigs(lens, reads, arcs, clip=clip, tip_reads=args.tip_reads, seqs=blk.rs.reads)
            model_s = time.perf_counter() - t0
        for got in (got_u, got_b):
            assert all(g.tobytes() == want[name].tobytes() for name, g in zip(("unitigs", "layout", "places"), got))
        assert got_b[3] == want["seq"].tobytes()
        assert all(st[k] == want["counts"][k] for st in (st_u, st_b) for k in unitig_model.COUNTS)
    eng.close()
    utg = want["unitigs"]
    out = {"workload": args.workload, "reps": args.reps, "min_depth": args.min_depth, "tip_reads": args.tip_reads, "candidates": n,
           "pair": int(len(pair)), "reads": int(len(lens)), "arcs": int(len(arcs)), "bases": int(len(want["seq"])),
           "n50": n50(utg["length"]), "model_seconds": round(model_s, 3),
           "unitigs": {k: v for k, v in st_b.items() if k != "device_ms"}}
    for k, v in ms.items():
        a = np.array(v)
        out[k] = {"ms_median": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
