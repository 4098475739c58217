"""The bubble popping of gact_hip_pop_bubbles in plain Python, restated from the entry's comment in include/gact_hip.h, the
checker of what that comment promises, and the hand-made graphs that tests/test_bubble_model.py and tests/test_gpu_bubbles.py
share.

  W = the arcs with flags == 0 whose two reads are not named by skip; out(x) = the W arcs out of x in array order, in(x) =
  |out(x^1)|.  One search per source s with |out(s)| >= 2: vertices are expanded from a LIFO stack, each only after all its
  in-arcs are crossed, every arc of the popped vertex in array order; the first failure -- open, dead, twice, dist, many -- is
  the search's.  It succeeds when one vertex is on the stack and none is waiting: that vertex is the sink.  owner[read] = the
  lowest source among the found bubbles whose interior holds the read; a bubble pops iff it owns all its interior reads.  A
  popped bubble keeps the path with the most arcs (then the fewest bases, then the lowest last arc) and removes the rest.
Dicts and loops, no cleverness."""
import numpy as np

from gact_amd import engine
from unitig_model import make_arcs, plain_reads, path_rows, shuffled_vertices, random_graph   # noqa: F401 (the tests' graphs)
import unitig_model

POPPED, LOST = 0, 1
BUBBLE_BIT = 4
FAILS = ("open", "dead", "twice", "dist", "many")
COUNTS = ("reads", "sources", "found", "popped", "lost", "reads_removed", "working_arcs", "arcs_removed", "by_fail")


def _checked(read_lens, reads, arcs, clip):
    """the refusals gact_hip_unitigs makes without bases -> (n, rows [(u, v, len)], flags)"""
    lens = [int(v) for v in read_lens]
    n = len(lens)
    nv = 2 * n
    if any(v < 0 for v in lens):
        raise ValueError("negative")
    cl = None if clip is None else [int(v) for v in np.asarray(clip).reshape(-1)]
    if cl is not None and not (len(cl) == nv and all(0 <= cl[2 * i] <= cl[2 * i + 1] <= lens[i] for i in range(n))):
        raise ValueError("clip")
    clipped = [lens[i] if cl is None else cl[2 * i + 1] - cl[2 * i] for i in range(n)]
    cby = [int(v) for v in reads["contained_by"]]
    assert len(cby) == n
    live = [cby[i] < 0 and clipped[i] > 0 for i in range(n)]
    rows = list(zip(arcs["u"].tolist(), arcs["v"].tolist(), arcs["len"].tolist()))
    flags = arcs["flags"].tolist()
    for k, (u, v, ln) in enumerate(rows):
        if not (0 <= u < nv and 0 <= v < nv) or u >> 1 == v >> 1 or ln < 1:
            raise ValueError("arc %d out of range" % k)
    for k in range(1, len(rows)):
        a, b = rows[k - 1], rows[k]
        if not (a[0], a[2], a[1]) < (b[0], b[2], b[1]):
            raise ValueError("arcs not ascending at %d" % k)
    e0 = set((rows[k][0], rows[k][1]) for k in range(len(rows)) if flags[k] == 0)
    for k, (u, v, ln) in enumerate(rows):
        if flags[k] == 0:
            if not (live[u >> 1] and live[v >> 1]):
                raise ValueError("arc %d names a read that is not live" % k)
            if (v ^ 1, u ^ 1) not in e0:
                raise ValueError("arc %d has no complement" % k)
    return n, rows, flags


def _search(s, out, rows, max_dist, max_vertices):
    """-> ("found", order of the seen vertices, their records, the sink) or (the failure's name,)"""
    rec = {s: [0, 0, 0, 0, -1]}                       # vertex -> [r, d, c, pd, pred]; dicts keep the order of seeing
    stack, pending = [s], 0
    while True:
        v = stack.pop()
        if not out[v]:
            return ("dead",)
        _, dv, cv, pdv, _ = rec[v]
        for k in out[v]:
            w, ln = rows[k][1], rows[k][2]
            if w == s or w == s ^ 1 or (w ^ 1) in rec:
                return ("twice",)
            d = dv + ln
            if d > max_dist:
                return ("dist",)
            if w not in rec:
                if len(rec) >= max_vertices:
                    return ("many",)
                rec[w] = [len(out[w ^ 1]), d, cv + 1, pdv + ln, k]
                pending += 1
            else:
                r = rec[w]
                r[1] = min(r[1], d)
                if (cv + 1, -(pdv + ln), -k) > (r[2], -r[3], -r[4]):
                    r[2], r[3], r[4] = cv + 1, pdv + ln, k
            rec[w][0] -= 1
            if rec[w][0] == 0:
                stack.append(w)
                pending -= 1
        if len(stack) == 1 and pending == 0:
            return ("found", list(rec), rec, stack[0])
        if not stack:
            return ("open",)


def pop_bubbles(read_lens, reads, arcs, clip=None, skip=None, max_dist=50000, max_vertices=64):
    """-> dict(bubbles BUBBLE_DTYPE ascending by source, read_bubble int32 per read, arc_flags int32 per arc, counts: the
    integer fields of gact_bubble_stats but scratch_bytes (by_fail a list of 5), detail: per bubble (seen vertices, the kept
    path s .. t, the removed reads) for the checker).  ValueError: what the entry refuses"""
    if not 1 <= max_dist <= 1 << 30:
        raise ValueError("max_dist")
    if not 3 <= max_vertices <= 64:
        raise ValueError("max_vertices")
    n, rows, flags = _checked(read_lens, reads, arcs, clip)
    nv = 2 * n
    sk = [0] * n if skip is None else [int(v) != 0 for v in skip]
    assert len(sk) == n
    in_w = [flags[k] == 0 and not sk[rows[k][0] >> 1] and not sk[rows[k][1] >> 1] for k in range(len(rows))]
    out = [[] for _ in range(nv)]
    for k, (u, v, ln) in enumerate(rows):
        if in_w[k]:
            out[u].append(k)
    at = {(rows[k][0], rows[k][1]): k for k in range(len(rows)) if in_w[k]}
    by_fail = [0] * 5
    found = []                                        # (s, t, seen, rec), ascending by s
    sources = 0
    for s in range(nv):
        if len(out[s]) < 2:
            continue
        sources += 1
        res = _search(s, out, rows, max_dist, max_vertices)
        if res[0] == "found":
            found.append((s, res[3], res[1], res[2]))
        else:
            by_fail[FAILS.index(res[0])] += 1
    owner = {}
    for s, t, seen, rec in found:
        for x in seen:
            if x != s and x != t:
                owner[x >> 1] = min(owner.get(x >> 1, s), s)
    bubbles = np.zeros(len(found), dtype=engine.BUBBLE_DTYPE)
    read_bubble = np.full(n, -1, dtype=np.int32)
    removed_arc = [False] * len(rows)
    gone = [False] * n
    detail = []
    for j, (s, t, seen, rec) in enumerate(found):
        path = [t]
        while path[-1] != s:
            path.append(rows[rec[path[-1]][4]][0])
        path.reverse()
        interior = [x for x in seen if x != s and x != t]
        removed = [x for x in interior if x not in path]
        popped = all(owner[x >> 1] == s for x in interior)
        assert interior
        bubbles[j] = (s, t, len(seen), len(path) - 2, len(removed), POPPED if popped else LOST, rec[t][3])
        detail.append((list(seen), path, [x >> 1 for x in removed] if popped else []))
        if not popped:
            continue
        for x in removed:
            gone[x >> 1] = True
            read_bubble[x >> 1] = j
        path_arcs = set(rec[x][4] for x in path[1:])
        for x in path[:-1]:
            for k in out[x]:
                if rows[k][1] in path and k not in path_arcs:
                    removed_arc[k] = True
                    removed_arc[at[(rows[k][1] ^ 1, x ^ 1)]] = True
    for k, (u, v, ln) in enumerate(rows):
        if in_w[k] and (gone[u >> 1] or gone[v >> 1]):
            removed_arc[k] = True
    arc_flags = np.array([flags[k] | (BUBBLE_BIT if removed_arc[k] else 0) for k in range(len(rows))], dtype=np.int32)
    n_popped = int((bubbles["state"] == POPPED).sum())
    counts = dict(reads=n, sources=sources, found=len(found), popped=n_popped, lost=len(found) - n_popped,
                  reads_removed=sum(gone), working_arcs=sum(in_w), arcs_removed=sum(removed_arc), by_fail=by_fail)
    return dict(bubbles=bubbles, read_bubble=read_bubble, arc_flags=arc_flags, counts=counts, detail=detail)


def cleaned(arcs, arc_flags):
    """the arcs with arc_flags written into flags: what a following unitig call takes"""
    a = arcs.copy()
    a["flags"] = arc_flags
    return a


def check(reads, arcs, result, skip=None):
    """what the header promises of a result: the arcs left are closed under complement; no read is removed by two bubbles
    and read_bubble names the one; after the pops a popped bubble's source has one W arc left, and every arc of its kept
    path is a join over what is left of W"""
    n = len(reads)
    rows = list(zip(arcs["u"].tolist(), arcs["v"].tolist()))
    flags = arcs["flags"].tolist()
    af = result["arc_flags"].tolist()
    assert len(af) == len(rows) and all(af[k] & ~BUBBLE_BIT == flags[k] for k in range(len(rows)))
    left = set(rows[k] for k in range(len(rows)) if af[k] == 0)
    assert all((v ^ 1, u ^ 1) in left for u, v in left), "the arcs left are not closed under complement"
    sk = [False] * n if skip is None else [int(v) != 0 for v in skip]
    w_left = [(u, v) for u, v in left if not sk[u >> 1] and not sk[v >> 1]]
    out = {}
    for u, v in w_left:
        out[u] = out.get(u, 0) + 1
    taken = {}
    b = result["bubbles"]
    assert (np.diff(b["source"]) > 0).all()
    for j, (seen, path, removed) in enumerate(result["detail"]):
        assert b["n_vertices"][j] == len(seen) and b["n_path"][j] == len(path) - 2 and b["n_path"][j] + b["n_removed"][j] == len(seen) - 2
        for i in removed:
            assert i not in taken, "read %d is removed by the bubbles %d and %d" % (i, taken[i], j)
            taken[i] = j
        if b["state"][j] != POPPED:
            assert not removed
            continue
        assert out.get(path[0], 0) == 1, "the source of bubble %d keeps %d arcs" % (j, out.get(path[0], 0))
        for u, v in zip(path, path[1:]):
            assert (u, v) in left and out.get(u, 0) == 1 and out.get(v ^ 1, 0) == 1, "arc %d -> %d of bubble %d is no join" % (u, v, j)
    rb = result["read_bubble"]
    assert rb.tolist() == [taken.get(i, -1) for i in range(n)]
    for i in taken:
        assert not any(u >> 1 == i or v >> 1 == i for u, v in w_left), "the removed read %d keeps an arc" % i


# ---- hand-made graphs

HAND_MADE = ("simple", "tie", "more_reads", "minus", "beads", "nested_in", "nested_out", "fan62", "fan63", "deep", "dead",
             "open_in", "open_out", "twice_cycle", "twice_inversion", "flagged", "long_lens")


def hand_made(pattern, seed=20261024):
    """-> (read_lens int32, reads, arcs, clip None, info) of one of HAND_MADE, the same on every call.  Reads are 5000 long
    (2^30 in long_lens).  The shapes are written over labels -- a backbone of four reads, the source its last, the branches,
    the sink, a backbone of four more -- and the labels get read ids and strands at random, but where the case is about the
    ids.  info: the vertices of some labels, by name"""
    rng = np.random.default_rng([seed, HAND_MADE.index(pattern)])
    rows, info = [], {}
    n_labels = [0]

    def new(k=1):
        n_labels[0] += k
        return list(range(n_labels[0] - k, n_labels[0]))

    def bubble(s, t, branches, ln=1000):
        """branches: lists of labels, each a path s -> ... -> t; arc lens ln + 100 * branch + position"""
        for j, br in enumerate(branches):
            p = [s] + br + [t]
            rows.extend((p[k], p[k + 1], ln + 100 * j + k) for k in range(len(p) - 1))

    left = new(4)
    rows += path_rows(left, 800)
    s = left[-1]
    read_len = 5000
    if pattern in ("simple", "flagged", "dead", "open_in", "open_out", "twice_cycle", "twice_inversion", "minus"):
        # s -> b (1000) -> t (1200) and s -> c (1100) -> t (1000): the same two arcs, c's path 100 bases shorter: b goes
        b, c, t = new(3)
        rows += [(s, b, 1000), (s, c, 1100), (b, t, 1200), (c, t, 1000)]
        if pattern == "flagged":
            rows[-4], rows[-2] = (s, b, 1000, 1), (b, t, 1200, 1)
        extra = []
        if pattern == "dead":
            extra = new(1)
            rows += [(b, extra[0], 700)]
        elif pattern == "open_in":
            extra = new(1)
            rows += [(extra[0], b, 700)]
        elif pattern == "open_out":
            extra = new(3)
            rows += [(b, extra[0], 700)] + path_rows(extra, 900)
        elif pattern == "twice_cycle":
            rows += [(b, s, 700)]
        elif pattern == "twice_inversion":
            rows += [(b, ~c, 700)]                      # (~label: the label's other strand)
        info.update(b=b, c=c, extra=extra)
    elif pattern == "tie":
        b, c, t = new(3)
        rows += [(s, b, 1000), (s, c, 1000), (b, t, 1200), (c, t, 1200)]
        info.update(b=b, c=c)
    elif pattern == "more_reads":
        b1, b2, c, t = new(4)
        rows += [(s, b1, 1000), (b1, b2, 1000), (b2, t, 1000), (s, c, 900), (c, t, 900), (s, t, 2500)]
        info.update(b=b1, b2=b2, c=c)
    elif pattern == "beads":
        b1, c1, m1, b2, c2, m2, b3, c3, t = new(9)
        bubble(s, m1, [[b1], [c1]])
        bubble(m1, m2, [[b2], [c2]])
        bubble(m2, t, [[b3], [c3]])
        info.update(m1=m1, m2=m2)
    elif pattern in ("nested_in", "nested_out"):
        x0, p, q, x1, y, t = new(6)
        rows += [(s, x0, 1000), (s, y, 1100), (x1, t, 1000), (y, t, 1100)]
        bubble(x0, x1, [[p], [q]])
        info.update(x0=x0, x1=x1, p=p, q=q, y=y)
    elif pattern in ("fan62", "fan63"):
        t = new(1)[0]
        bubble(s, t, [[b] for b in new(int(pattern[3:]))], ln=100)
    elif pattern == "deep":
        t = new(1)[0]
        bubble(s, t, [new(30), new(30)], ln=100)
    elif pattern == "long_lens":
        # path_len past 2^31 while no vertex is farther than max_dist = 2^30 from s: the kept path s -> b1 -> b2 -> b3 -> t has
        # three arcs near 2^30, and each of b2, b3 has a short arc from s as its least distance; c is the read that goes
        read_len = 1 << 30
        b1, b2, b3, c, t = new(5)
        big = 1 << 30
        rows += [(s, b1, 1), (s, b2, 2), (s, b3, 3), (s, c, 4), (b1, b2, big - 1), (b2, b3, big - 2), (b3, t, big - 3), (c, t, 5)]
        info.update(b=b1, b2=b2, b3=b3, c=c)
    else:
        raise ValueError(pattern)
    right = [t] + new(3)
    rows += path_rows(right, 800)
    n = n_labels[0]
    # the ids: at random, or the case's own
    if pattern == "tie":                                  # b below c: the arc b -> t is the lower one, and b reaches t second
        vertex_of = [2 * i for i in range(n)]
    elif pattern == "minus":                              # every label on its odd vertex, ids descending along the path: t^1 < s
        order = left + [info["b"], info["c"]] + right
        vertex_of = [0] * n
        for pos, lab in enumerate(order):
            vertex_of[lab] = 2 * (n - 1 - pos) + 1
    elif pattern in ("nested_in", "nested_out"):          # even vertices; read 0 is the inner source / the outer source
        first = info["x0"] if pattern == "nested_in" else s
        others = [lab for lab in range(n) if lab != first]
        vertex_of = [0] * n
        for lab, i in zip(others, (rng.permutation(n - 1) + 1).tolist()):
            vertex_of[lab] = 2 * i
    else:
        vertex_of = shuffled_vertices(rng, n)
    lab_vertex = lambda lab: vertex_of[lab] if lab >= 0 else vertex_of[~lab] ^ 1
    rows = [(lab_vertex(r[0]), lab_vertex(r[1])) + tuple(r[2:]) for r in rows]
    info = {k: ([vertex_of[x] for x in v] if isinstance(v, list) else vertex_of[v]) for k, v in info.items()}
    info.update(s=vertex_of[s], t=vertex_of[t])
    return np.full(n, read_len, dtype=np.int32), plain_reads(n), make_arcs(rows), None, info
