"""What the bubble popping (gact_hip_pop_bubbles) costs on one GPU, in one process, next to the unitig call on the same graph:
  (r) tests/unitig_model.random_graph(3000, 1), the tips of a unitig call skipped;
  (e) the clipped graph of ecoli10x behind the calls that feed it -- the setup of tools/unitig_rate.py: the normal run over all
      candidates, the pair selection, its summaries, the coverage (min_depth 3), the overlap graph clipped to its spans.
On each: the unitig call without bases, tip_reads 3 (gact_hip_last_unitig_stats), the bubble call with those tips as skip
(gact_hip_last_bubble_stats), and the unitig call again over the cleaned arcs; HIP events around each whole call.  Every bubble
result is checked against the model (tests/bubble_model.py), whose wall clock is taken once.  One warm-up round, then --reps
rounds.  Prints one JSON line: medians with min and max, the bubble call's counts, the unitigs before and after.
Usage: python tools/bubble_rate.py [--workload ecoli10x] [--reps 5] [--max-dist 50000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "darwin-gpu_amd"), os.path.join(ROOT, "tests")]


def measure(eng, lens, reads, arcs, clip, reps, max_dist):
    import bubble_model
    import unitig_model
    ms = {"unitigs": [], "bubbles": [], "unitigs_cleaned": []}
    for rep in range(reps + 1):
        places = eng.unitigs(lens, reads, arcs, clip=clip, tip_reads=3)[2]
        st_u = eng.last_unitig_stats()
        skip = places["state"] == unitig_model.TIP
        got = eng.pop_bubbles(lens, reads, arcs, clip=clip, skip=skip, max_dist=max_dist)
        st_b = eng.last_bubble_stats()
        after = eng.unitigs(lens, reads, bubble_model.cleaned(arcs, got[2]), clip=clip, tip_reads=3)
        st_a = eng.last_unitig_stats()
        if rep:                                    # (the first round is the warm-up)
            for k, st in zip(ms, (st_u, st_b, st_a)):
                ms[k].append(st["device_ms"])
        else:
            t0 = time.perf_counter()
            want = bubble_model.pop_bubbles(lens, reads, arcs, clip=clip, skip=skip, max_dist=max_dist)
            model_s = time.perf_counter() - t0
            bubble_model.check(reads, arcs, want, skip=skip)
        assert all(g.tobytes() == want[name].tobytes() for name, g in zip(("bubbles", "read_bubble", "arc_flags"), got))
        assert all(st_b[k] == want["counts"][k] for k in bubble_model.COUNTS)
    out = {"reads": int(len(lens)), "arcs": int(len(arcs)), "model_seconds": round(model_s, 3),
           "bubbles": {k: v for k, v in st_b.items() if k != "device_ms"}, "unitigs_before": st_u["unitigs"],
           "unitigs_after": st_a["unitigs"], "longest_before": st_u["longest_bases"], "longest_after": st_a["longest_bases"]}
    for k, v in ms.items():
        a = np.array(v)
        out["ms_" + k] = {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="ecoli10x")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-depth", type=int, default=3)
    ap.add_argument("--max-dist", type=int, default=50000)
    args = ap.parse_args()
    from gact_amd import engine, workload
    import unitig_model
    eng = engine.Engine()
    out = {"reps": args.reps, "max_dist": args.max_dist}
    lens, reads, arcs, clip = unitig_model.random_graph(3000, 1)
    out["random3000_1"] = measure(eng, lens, reads, arcs, clip, args.reps, args.max_dist)
    blk = workload.make_block(args.workload)
    cat, offs = blk.rs.concat()
    rcat, _ = blk.rs.concat(rc=True)
    lens = np.diff(offs).astype(np.int32)
    eng.upload(engine.SET_REF, cat, offs)
    eng.upload(engine.SET_QUERY, cat, offs)
    eng.upload(engine.SET_QUERY_RC, rcat, offs)
    cands = np.concatenate([blk.cf, blk.cr]).astype(engine.CAND_DTYPE)
    n, nf = len(cands), len(blk.cf)
    eng.candidates_upload(cands)
    eng.candidates_run_mixed(n, nf)
    pair = eng.select_overlaps(n=n, mode="pair")
    _, sums = eng.candidates_summaries(sel=pair, rc_from=nf)
    cover = eng.read_coverage(lens, n=n, sel=pair, sums=sums, min_depth=args.min_depth)
    clip = np.stack([cover["span_begin"], cover["span_end"]], axis=1).astype(np.int32)
    reads, arcs = eng.overlap_graph(lens, n=n, sel=pair, sums=sums, clip=clip)
    out[args.workload] = measure(eng, lens, reads, arcs, clip.reshape(-1), args.reps, args.max_dist)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
