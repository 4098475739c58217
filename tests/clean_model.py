"""The weak-arc rule of gact_hip_prune_overlaps and the cleaning rounds of gact_hip_clean_graph in plain Python, restated from the
entries' comments in include/gact_hip.h, the checker of what those comments promise, the hand-made graphs and the generator of
graphs with repeats that tests/test_clean_model.py and tests/test_gpu_clean.py share.

  prune: W = the arcs with flags == 0 whose two reads are not named by skip; a vertex with two or more W arcs is examined, best =
  its largest ov_u; a W arc of an examined vertex is weak iff 1000 * ov_u < ratio_permille * best; an arc is removed iff it or
  its complement is weak.
  clean: over a flags array F -- T: the tip rule of unitig_model.unitigs, TIP reads removed, their arcs get the tip bit; B:
  bubble_model.pop_bubbles, its bits into F; settle = passes of T then B until one removes nothing (at most max_passes); then
  P(r_j) at the rising ratios, settling again after every one that removed an arc.
Both compose unitig_model and bubble_model unchanged.  Lists and loops, no cleverness."""
import numpy as np

from gact_amd import engine
import bubble_model
import graph_model
import unitig_model
from unitig_model import plain_reads, path_rows, shuffled_vertices, random_graph   # noqa: F401 (the tests' graphs)

BUBBLE_BIT, TIP_BIT, SHORT_BIT = 4, 8, 16
TIPS, BUBBLES, PRUNE = 0, 1, 2
KINDS = ("tips", "bubbles", "prune")
KEPT, CONTAINED, EMPTY, TIP, BUBBLE = 0, 1, 2, 3, 4
PRUNE_COUNTS = ("reads", "examined", "bared", "working_arcs", "weak", "arcs_removed")
CLEAN_COUNTS = ("reads", "steps", "passes", "reads_tip", "reads_bubble", "arcs_removed", "arcs_left")


def prune(read_lens, reads, arcs, clip=None, skip=None, ratio_permille=500):
    """-> dict(arc_flags int32 per arc, vertex_best int32 per vertex, counts: the integer fields of gact_prune_stats but
    scratch_bytes, weak: the indices of the weak arcs).  ValueError: what the entry refuses"""
    if not 0 <= ratio_permille <= 1000:
        raise ValueError("ratio_permille")
    n, rows, flags = bubble_model._checked(read_lens, reads, arcs, clip)
    nv = 2 * n
    sk = [0] * n if skip is None else [int(v) != 0 for v in skip]
    assert len(sk) == n
    ov = [int(v) for v in arcs["ov_u"].tolist()]
    in_w = [flags[k] == 0 and not sk[rows[k][0] >> 1] and not sk[rows[k][1] >> 1] for k in range(len(rows))]
    out = [[] for _ in range(nv)]
    for k in range(len(rows)):
        if in_w[k]:
            out[rows[k][0]].append(k)
    at = {}
    for k in range(len(rows)):
        if in_w[k]:
            at.setdefault((rows[k][0], rows[k][1]), k)
    best = [0] * nv
    weak = []
    examined = 0
    for x in range(nv):
        if len(out[x]) < 2:
            continue
        examined += 1
        best[x] = max(ov[k] for k in out[x])
        weak += [k for k in out[x] if 1000 * ov[k] < ratio_permille * best[x]]
    removed = [False] * len(rows)
    for k in weak:
        removed[k] = True
        removed[at[(rows[k][1] ^ 1, rows[k][0] ^ 1)]] = True
    bared = sum(1 for x in range(nv) if out[x] and all(removed[k] for k in out[x]))
    arc_flags = np.array([flags[k] | (SHORT_BIT if removed[k] else 0) for k in range(len(rows))], dtype=np.int32)
    counts = dict(reads=n, examined=examined, bared=bared, working_arcs=sum(in_w), weak=len(weak), arcs_removed=sum(removed))
    return dict(arc_flags=arc_flags, vertex_best=np.array(best, dtype=np.int32), counts=counts, weak=weak)


def ratios_of(lo, hi, n_ratios):
    return [lo if n_ratios == 1 else lo + (hi - lo) * j // (n_ratios - 1) for j in range(n_ratios)]


def _tip_chains(read_lens, reads, arcs, clip):
    """the linear chains the tip rule looks at, one per head vertex: the live vertices no join enters"""
    lens = [int(v) for v in read_lens]
    n = len(lens)
    cl = None if clip is None else [int(v) for v in np.asarray(clip).reshape(-1)]
    live = [int(reads["contained_by"][i]) < 0 and (lens[i] if cl is None else cl[2 * i + 1] - cl[2 * i]) > 0 for i in range(n)]
    rows = list(zip(arcs["u"].tolist(), arcs["v"].tolist(), arcs["len"].tolist()))
    e0 = [k for k in range(len(rows)) if arcs["flags"][k] == 0]
    _, _, prv, _, _ = unitig_model._joins(2 * n, rows, e0)
    return sum(1 for x in range(2 * n) if live[x >> 1] and prv[x] < 0)


def clean(read_lens, reads, arcs, clip=None, tip_reads=3, max_dist=50000, max_vertices=64, ratios=(500, 700, 3), max_passes=4):
    """-> dict(arc_flags int32 per arc, read_state CLEAN_READ_DTYPE, steps CLEAN_STEP_DTYPE, counts: the integer fields of
    gact_clean_stats but scratch_bytes (arcs_removed a list of 3)).  ValueError: what the entry refuses"""
    lo, hi, n_ratios = ratios
    if tip_reads < 1:
        raise ValueError("tip_reads")
    if not 1 <= max_dist <= 1 << 30:
        raise ValueError("max_dist")
    if not 3 <= max_vertices <= 64:
        raise ValueError("max_vertices")
    if not 0 <= lo <= hi <= 1000:
        raise ValueError("ratios")
    if not 0 <= n_ratios <= 16:
        raise ValueError("n_ratios")
    if not 1 <= max_passes <= 16:
        raise ValueError("max_passes")
    n, _, flags = bubble_model._checked(read_lens, reads, arcs, clip)
    work = arcs.copy()                                # (flags: F)
    first = unitig_model.unitigs(read_lens, reads, work, clip=clip, tip_reads=0)["places"]["state"].tolist()
    state = [{unitig_model.CONTAINED: CONTAINED, unitig_model.EMPTY: EMPTY}.get(s, KEPT) for s in first]
    step_of = [-1] * n
    steps = []
    totals = dict(passes=0, reads_tip=0, reads_bubble=0, arcs_removed=[0, 0, 0])
    touches = list(zip((arcs["u"] >> 1).tolist(), (arcs["v"] >> 1).tolist()))

    def log(kind, param, removed_reads, examined, new_flags):
        f = work["flags"]
        had = int((f == 0).sum())
        left = int((new_flags == 0).sum())
        for i in removed_reads:
            state[i], step_of[i] = (TIP if kind == TIPS else BUBBLE), len(steps)
        steps.append((kind, param, len(removed_reads), examined, had - left, left))
        totals["arcs_removed"][kind] += had - left
        work["flags"] = new_flags
        return had - left

    def tips():
        places = unitig_model.unitigs(read_lens, reads, work, clip=clip, tip_reads=tip_reads)["places"]
        cut = (places["state"] == unitig_model.TIP).tolist()
        f = work["flags"].copy()
        for k, (a, b) in enumerate(touches):
            if f[k] == 0 and (cut[a] or cut[b]):
                f[k] = TIP_BIT
        newly = [i for i in range(n) if cut[i] and state[i] == KEPT]
        totals["reads_tip"] += len(newly)
        return log(TIPS, tip_reads, newly, _tip_chains(read_lens, reads, work, clip), f)

    def bubbles():
        res = bubble_model.pop_bubbles(read_lens, reads, work, clip=clip, max_dist=max_dist, max_vertices=max_vertices)
        gone = np.flatnonzero(res["read_bubble"] >= 0).tolist()
        totals["reads_bubble"] += len(gone)
        return log(BUBBLES, max_dist, gone, res["counts"]["sources"], res["arc_flags"])

    def settle():
        for _ in range(max_passes):
            removed = tips() + bubbles()
            totals["passes"] += 1
            if removed == 0:
                break

    settle()
    for r in ratios_of(lo, hi, n_ratios):
        res = prune(read_lens, reads, work, clip=clip, ratio_permille=r)
        if log(PRUNE, r, [], res["counts"]["examined"], res["arc_flags"]):
            settle()
    read_state = np.zeros(n, dtype=engine.CLEAN_READ_DTYPE)
    read_state["state"], read_state["step"] = state, step_of
    counts = dict(reads=n, steps=len(steps), arcs_left=int((work["flags"] == 0).sum()), **totals)
    return dict(arc_flags=work["flags"].astype(np.int32), read_state=read_state,
                steps=np.array(steps, dtype=engine.CLEAN_STEP_DTYPE).reshape(-1), counts=counts)


def cleaned(arcs, arc_flags):
    """the arcs with arc_flags written into flags: what a following unitig call takes"""
    return bubble_model.cleaned(arcs, arc_flags)


def check(reads, arcs, arc_flags, steps=None, read_state=None):
    """what the header promises of a result of either entry: the arcs left are closed under complement; only the two new bits
    and the bubble bit are added, one to an arc, and only to arcs that had flags == 0; the log's arcs_left chain is consistent
    and its arcs_removed by kind are the arcs that carry the kind's bit; a removed read keeps no arc and names a step of its kind"""
    rows = list(zip(arcs["u"].tolist(), arcs["v"].tolist()))
    flags = arcs["flags"].tolist()
    af = np.asarray(arc_flags).tolist()
    assert len(af) == len(rows)
    for k in range(len(rows)):
        added = af[k] & ~flags[k]
        assert af[k] & flags[k] == flags[k] and added in (0, BUBBLE_BIT, TIP_BIT, SHORT_BIT), "arc %d: %d -> %d" % (k, flags[k], af[k])
        assert not (added and flags[k]), "arc %d had flags %d and got a bit" % (k, flags[k])
    left = set(rows[k] for k in range(len(rows)) if af[k] == 0)
    assert all((v ^ 1, u ^ 1) in left for u, v in left), "the arcs left are not closed under complement"
    if steps is None:
        return
    at = sum(1 for f in flags if f == 0)
    by_kind = [0, 0, 0]
    for s in steps:
        assert s["arcs_left"] == at - s["arcs_removed"] and s["arcs_removed"] >= 0 and s["kind"] in (TIPS, BUBBLES, PRUNE)
        at = int(s["arcs_left"])
        by_kind[int(s["kind"])] += int(s["arcs_removed"])
    assert at == len(left)
    added = [af[k] & ~flags[k] for k in range(len(rows))]
    assert by_kind == [added.count(TIP_BIT), added.count(BUBBLE_BIT), added.count(SHORT_BIT)]
    if read_state is None:
        return
    for i, (st, at_step) in enumerate(zip(read_state["state"].tolist(), read_state["step"].tolist())):
        if st in (TIP, BUBBLE):
            assert 0 <= at_step < len(steps) and steps["kind"][at_step] == (TIPS if st == TIP else BUBBLES)
            assert not any(u >> 1 == i or v >> 1 == i for u, v in left), "the removed read %d keeps an arc" % i
        else:
            assert st in (KEPT, CONTAINED, EMPTY) and at_step == -1
    assert int(steps["reads_removed"].sum()) == int(np.isin(read_state["state"], (TIP, BUBBLE)).sum())


# ---- hand-made graphs

def ov_arcs(rows):
    """[(u, v, len, ov_u, ov_v)] or [(u, v, len, ov_u, ov_v, flags)] -> GRAPH_ARC_DTYPE with every complement added (v^1 -> u^1,
    the same len and flags, ov_u and ov_v changing places: an arc's ov_v is its complement's ov_u), ascending by (u, len, v)"""
    full = {}
    for row in rows:
        u, v, ln, ou, ovv = row[:5]
        fl = row[5] if len(row) > 5 else 0
        full[(u, v)] = (ln, ou, ovv, fl)
    for (u, v), (ln, ou, ovv, fl) in list(full.items()):
        full.setdefault((v ^ 1, u ^ 1), (ln, ovv, ou, fl))
    order = sorted(full, key=lambda k: (k[0], full[k][0], k[1]))
    arcs = np.zeros(len(order), dtype=engine.GRAPH_ARC_DTYPE)
    for j, (u, v) in enumerate(order):
        ln, ou, ovv, fl = full[(u, v)]
        arcs[j] = (u, v, ln, ou, ovv, j, 50, fl)
    return arcs


HAND_MADE = ("false_fork", "threshold", "mirror_only", "single", "fan2", "fan63", "fan64", "fan65", "fan129", "flagged", "skipped",
             "big_ov", "no_arcs")
STRONG = 3000                                           # the overlap of an arc the case says nothing about


def hand_made(pattern, seed=20261101):
    """-> (read_lens int32, reads, arcs, clip None, info) of one of HAND_MADE, the same on every call.  Reads are 5000 long.
    The shapes are written over labels and the labels get read ids and strands at random.  Every branch leads into a path of
    four reads, so that no tip cut takes the case away.  info: skip (or None), x: the vertex the case is about, and weak: the
    (u, v) of the arcs that are weak at the default ratio"""
    rng = np.random.default_rng([seed, HAND_MADE.index(pattern)])
    rows, weak = [], []
    n_labels = [0]
    skip_labels = []

    def new(k=1):
        n_labels[0] += k
        return list(range(n_labels[0] - k, n_labels[0]))

    def path(labels, ln=800):
        rows.extend((u, v, l, STRONG, STRONG) for u, v, l in path_rows(labels, ln))

    def branch(x, ln, ov_u, ov_v=STRONG, flags=0, tail=4, is_weak=False):
        """an arc out of x into a new path of `tail` reads -> the path's first label"""
        labels = new(tail)
        rows.append((x, labels[0], ln, ov_u, ov_v, flags))
        path(labels)
        if is_weak:
            weak.append((x, labels[0]))
        return labels[0]

    x = None
    if pattern == "no_arcs":
        new(3)
    elif pattern == "single":
        path(new(9))
    else:
        left = new(5)
        path(left)
        x = left[-1]
        if pattern == "false_fork":
            # the backbone goes on through a strong arc; a weak one leads into a side path of six reads that never comes back
            branch(x, 1000, STRONG, tail=5)
            branch(x, 1100, 1000, tail=6, is_weak=True)
        elif pattern == "threshold":
            # best 2000: 1000 and 1400 are the equalities of 500 and 700 per mille, 999 and 1399 lie one below them
            for j, ov in enumerate((2000, 1400, 1399, 1000, 999)):
                branch(x, 1000 + j, ov, is_weak=ov == 999)
        elif pattern == "mirror_only":
            # x -> w is the best arc of x; w^1 sees it with 500 beside the 3000 of y -> w: weak there, so both go
            w = branch(x, 1000, 2000, ov_v=500)
            branch(x, 1100, 1500)
            y = new(5)
            path(y)
            rows.append((y[-1], w, 900, 3000, 3000))
            weak.append((~w, ~x))
        elif pattern.startswith("fan"):
            # the stretch of x in array order (len ascending): weak arcs at 0, 63, 64 and 128, the best arc last
            n = int(pattern[3:])
            for j in range(n):
                last = j == n - 1
                is_weak = j in (0, 63, 64, 128) and not last
                branch(x, 1000 + j, 4000 if last else 1000 if is_weak else STRONG, is_weak=is_weak)
        elif pattern in ("flagged", "skipped"):
            # W arcs of 2000, 1200 and 900 with arcs of 10^9 between them that are not of W: counted, they would make all three weak
            huge = 10 ** 9
            for j, ov in enumerate((2000, huge, 1200, huge, 900)):
                if ov == huge:
                    lab = branch(x, 1000 + j, huge, ov_v=huge, flags=1 if pattern == "flagged" else 0, tail=1)
                    skip_labels.append(lab)
                else:
                    branch(x, 1000 + j, ov, is_weak=ov == 900)
        elif pattern == "big_ov":
            # at 1000 per mille 2^31 - 2 is weak beside 2^31 - 1 and the tie stays: 1000 * ov_u needs 64 bits
            top = 2 ** 31 - 1
            branch(x, 1000, top)
            branch(x, 1001, top - 1)
            branch(x, 1002, top)
            branch(x, 1003, STRONG, is_weak=True)
        else:
            raise ValueError(pattern)
    n = n_labels[0]
    vertex_of = shuffled_vertices(rng, n)
    lab_vertex = lambda lab: vertex_of[lab] if lab >= 0 else vertex_of[~lab] ^ 1
    arcs = ov_arcs([(lab_vertex(r[0]), lab_vertex(r[1])) + tuple(r[2:]) for r in rows])
    skip = None
    if pattern == "skipped":
        skip = np.zeros(n, dtype=np.uint8)
        skip[[vertex_of[lab] >> 1 for lab in skip_labels]] = 1
    info = dict(skip=skip, x=None if x is None else vertex_of[x], weak=[(lab_vertex(u), lab_vertex(v)) for u, v in weak])
    return np.full(n, 5000, dtype=np.int32), plain_reads(n), arcs, None, info


# ---- graphs with repeats

def repeat_graph(n, seed, rep_len=1500, n_rep=6, loss=0.1):
    """-> (read_lens, reads, arcs, clip None, the set of record indices that exist only because of a repeat)"""
    rng = np.random.default_rng([20261101, n, seed])
    genome = 600 * n
    layout = graph_model._random_layout(rng, n, genome, 2000, 9000)
    lens = np.array([ln for _, ln, _ in layout], dtype=np.int32)
    order = sorted(range(n), key=lambda i: layout[i][0])
    rows = []
    for k, t in enumerate(order):
        for q in order[k + 1:]:
            if layout[q][0] >= layout[t][0] + layout[t][1]:
                break
            for a, b in ((t, q), (q, t)):
                row = graph_model.layout_row(layout, a, b)
                if row is not None and row[7] >= 300:
                    rows.append(row)
    n_true = len(rows)
    for _ in range(n_rep):
        p1, p2 = sorted(int(x) for x in rng.integers(0, genome - rep_len, 2))
        if p2 - p1 < 20000:
            continue
        c1 = [i for i in range(n) if layout[i][0] < p1 + rep_len and layout[i][0] + layout[i][1] > p1]
        c2 = [i for i in range(n) if layout[i][0] < p2 + rep_len and layout[i][0] + layout[i][1] > p2]
        for t in c1:
            for q in c2:
                for a, b, sh_a, sh_b in ((t, q, 0, p2 - p1), (q, t, p2 - p1, 0)):
                    (sa, la, da), (sb, lb, db) = layout[a], layout[b]
                    sa -= sh_a; sb -= sh_b                      # both in the first copy's frame
                    lo, hi = max(sa, sb, p1), min(sa + la, sb + lb, p1 + rep_len)
                    if hi - lo < 300:
                        continue
                    if da == 0: ab, ae, bb, be = lo - sa, hi - sa, lo - sb, hi - sb
                    else:       ab, ae, bb, be = sa + la - hi, sa + la - lo, sb + lb - hi, sb + lb - lo
                    rows.append((a, b, int(da != db), ab, ae, bb, be, hi - lo, 1))
    keep = np.flatnonzero(rng.random(len(rows)) < 1 - loss).tolist()
    rec = graph_model.records_of([rows[k] for k in keep])
    g = graph_model.graph(rec, lens, params=dict(max_hang=300, min_ovlp=600, fuzz=100))
    return lens, g["reads"], g["arcs"], None, set(j for j, k in enumerate(keep) if k >= n_true)
