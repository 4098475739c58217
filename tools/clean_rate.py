"""What the weak-arc call (gact_hip_prune_overlaps) and the cleaning rounds (gact_hip_clean_graph) cost on one GPU, in one
process, next to the three calls of the driver's --bubbles path on the same graph.  The graphs are the clipped graphs of the
workloads behind the calls that feed them -- the setup of tools/bubble_rate.py: the normal run over all candidates, the pair
selection, its summaries, the coverage (min_depth 3), the overlap graph clipped to its spans.
  --part clean    one prune call at 500 per mille, one clean call with the defaults, and the unitig call over the cleaned arcs;
                  every result is checked against the model (tests/clean_model.py), whose wall clock is taken once
  --part bubbles  the unitig call without bases, tip_reads 3, the bubble call with those tips as skip, the unitig call over the
                  cleaned arcs, and the sum of the three: what the rounds are compared with.  It uses no entry of the rounds, so
                  GACT_HIP_LIB_PATH may name an older library
HIP events around each whole call (gact_hip_last_*_stats).  One warm-up round, then --reps rounds.  Prints one JSON line: medians
with min and max, the counts, the unitigs before and after.
Usage: python tools/clean_rate.py [--part clean|bubbles] [--workloads ecoli10x,ecoli10x_small] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "darwin-gpu_amd"), os.path.join(ROOT, "tests")]


def _spread(v):
    a = np.array(v)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def _layout(st):
    return {"unitigs": st["unitigs"], "longest_bases": st["longest_bases"], "placed": st["placed"]}


def measure_clean(eng, lens, reads, arcs, clip, reps):
    import clean_model
    ms = {"prune": [], "clean": [], "unitigs_cleaned": []}
    eng.unitigs(lens, reads, arcs, clip=clip, tip_reads=3)
    before = eng.last_unitig_stats()
    for rep in range(reps + 1):
        flags, best = eng.prune_overlaps(lens, reads, arcs, clip=clip, best=True)
        st_p = eng.last_prune_stats()
        got = eng.clean_graph(lens, reads, arcs, clip=clip)
        st_c = eng.last_clean_stats()
        eng.unitigs(lens, reads, clean_model.cleaned(arcs, got[0]), clip=clip, tip_reads=3)
        st_a = eng.last_unitig_stats()
        if rep:                                    # (the first round is the warm-up)
            for k, st in zip(ms, (st_p, st_c, st_a)):
                ms[k].append(st["device_ms"])
        else:
            want_p = clean_model.prune(lens, reads, arcs, clip=clip)
            t0 = time.perf_counter()
            want = clean_model.clean(lens, reads, arcs, clip=clip)
            model_s = time.perf_counter() - t0
            clean_model.check(reads, arcs, want["arc_flags"], want["steps"], want["read_state"])
        assert flags.tobytes() == want_p["arc_flags"].tobytes() and best.tobytes() == want_p["vertex_best"].tobytes()
        assert all(st_p[k] == want_p["counts"][k] for k in clean_model.PRUNE_COUNTS)
        assert all(g.tobytes() == want[name].tobytes() for name, g in zip(("arc_flags", "read_state", "steps"), got))
        assert all(st_c[k] == want["counts"][k] for k in clean_model.CLEAN_COUNTS)
    out = {"reads": int(len(lens)), "arcs": int(len(arcs)), "model_seconds": round(model_s, 3),
           "prune": {k: v for k, v in st_p.items() if k != "device_ms"}, "clean": {k: v for k, v in st_c.items() if k != "device_ms"},
           "steps": [[engine_kind(s["kind"])] + [int(s[k]) for k in ("param", "reads_removed", "examined", "arcs_removed", "arcs_left")]
                     for s in got[2]],
           "before": _layout(before), "after": _layout(st_a)}
    out.update(("ms_" + k, _spread(v)) for k, v in ms.items())
    return out


def engine_kind(kind):
    from gact_amd import engine
    return engine.CLEAN_KINDS[int(kind)]


def measure_bubbles(eng, lens, reads, arcs, clip, reps):
    import bubble_model
    import unitig_model
    ms = {"unitigs": [], "bubbles": [], "unitigs_cleaned": [], "sum": []}
    for rep in range(reps + 1):
        places = eng.unitigs(lens, reads, arcs, clip=clip, tip_reads=3)[2]
        st_u = eng.last_unitig_stats()
        got = eng.pop_bubbles(lens, reads, arcs, clip=clip, skip=places["state"] == unitig_model.TIP)
        st_b = eng.last_bubble_stats()
        eng.unitigs(lens, reads, bubble_model.cleaned(arcs, got[2]), clip=clip, tip_reads=3)
        st_a = eng.last_unitig_stats()
        if rep:
            three = [st["device_ms"] for st in (st_u, st_b, st_a)]
            for k, v in zip(ms, three + [sum(three)]):
                ms[k].append(v)
    out = {"reads": int(len(lens)), "arcs": int(len(arcs)), "before": _layout(st_u), "after": _layout(st_a)}
    out.update(("ms_" + k, _spread(v)) for k, v in ms.items())
    return out


def graph_of(eng, name, min_depth):
    from gact_amd import engine, workload
    blk = workload.make_block(name)
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
    cover = eng.read_coverage(lens, n=n, sel=pair, sums=sums, min_depth=min_depth)
    clip = np.stack([cover["span_begin"], cover["span_end"]], axis=1).astype(np.int32)
    reads, arcs = eng.overlap_graph(lens, n=n, sel=pair, sums=sums, clip=clip)
    return lens, reads, arcs, clip.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("clean", "bubbles"), default="clean")
    ap.add_argument("--workloads", default="ecoli10x,ecoli10x_small")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-depth", type=int, default=3)
    args = ap.parse_args()
    from gact_amd import engine
    out = {"part": args.part, "reps": args.reps}
    for name in args.workloads.split(","):
        eng = engine.Engine()
        lens, reads, arcs, clip = graph_of(eng, name, args.min_depth)
        out[name] = (measure_clean if args.part == "clean" else measure_bubbles)(eng, lens, reads, arcs, clip, args.reps)
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
