"""The unitigs of gact_hip_unitigs in plain Python and numpy, restated from the entry's comment in include/gact_hip.h, and the
hand-made graphs that tests/test_unitig_model.py and tests/test_gpu_unitigs.py share.

  live reads are the ones that are not contained and have a clipped length > 0; E0 = the arcs with flags == 0; an arc u -> v is a
  join iff out(u) == 1 and in(v) == 1; a chain is a maximal path of joins; a linear chain of at most tip_reads reads with no arc
  into its head or none out of its tail is a tip, cut in one simultaneous round; E1 = E0 without the arcs that touch a cut read;
  the chains of E1 are the unitigs, one per complement pair: the orientation with the smaller head, a cycle opened in front of
  the lowest vertex id of the cycle and its complement; numbered ascending by their first vertex.
Chains are walked one vertex at a time.  Lists and loops, no cleverness."""
import numpy as np

from gact_amd import engine

PLACED, CONTAINED, EMPTY, TIP = range(4)
COUNTS = ("reads", "placed", "cut", "contained", "unitigs", "circular", "longest_reads", "longest_bases", "e0_arcs", "e1_arcs",
          "joins", "links")
_COMP = {ord(a): ord(b) for a, b in zip("ACGTNacgtn", "TGCANtgcan")}
_COMP_TABLE = np.array([_COMP.get(b, ord("N")) for b in range(256)], dtype=np.uint8)


def oriented(read, cb, ce, s):
    """the clipped read [cb, ce) of a uint8 array as stored (s == 0) or reverse-complemented with revcomp_kernel's table"""
    piece = np.asarray(read, dtype=np.uint8)[cb:ce]
    return piece if s == 0 else _COMP_TABLE[piece[::-1]]


def _joins(nv, arcs, chosen):
    """over the arcs `chosen` (indices): (out, next, prev, join_len, number of joins)"""
    out, nxt, prv, jl = [0] * nv, [-1] * nv, [-1] * nv, [0] * nv
    for k in chosen:
        out[arcs[k][0]] += 1
    n_joins = 0
    for k in chosen:
        u, v, ln = arcs[k]
        if out[u] == 1 and out[v ^ 1] == 1:
            nxt[u], prv[v], jl[u] = v, u, ln
            n_joins += 1
    return out, nxt, prv, jl, n_joins


def _chains(vertices, nxt, prv):
    """-> (linear chains head first, cycles in some rotation) over `vertices`, each a list of vertices"""
    seen, linear, cycles = set(), [], []
    for x in vertices:
        if prv[x] < 0:
            chain = [x]
            while nxt[chain[-1]] >= 0:
                chain.append(nxt[chain[-1]])
            seen.update(chain)
            linear.append(chain)
    for x in vertices:
        if x not in seen:
            chain = [x]
            while nxt[chain[-1]] != x:
                chain.append(nxt[chain[-1]])
            seen.update(chain)
            cycles.append(chain)
    return linear, cycles


def unitigs(read_lens, reads, arcs, clip=None, tip_reads=3, seqs=None):
    """-> dict(unitigs UNITIG_DTYPE, layout UNITIG_ENTRY_DTYPE, places UNITIG_PLACE_DTYPE, seq: uint8 array or None, links:
    [(unitig of u, +|-, unitig of v, +|-, min(ov_u, ov_v))] in arc order, counts: the integer fields of gact_unitig_stats but
    rank_launches and scratch_bytes).  reads: GRAPH_READ_DTYPE (contained_by is read), arcs: GRAPH_ARC_DTYPE ascending by
    (u, len, v); seqs: None, or the reads as uint8 arrays.  ValueError: what the entry refuses"""
    lens = [int(v) for v in read_lens]
    n = len(lens)
    nv = 2 * n
    if tip_reads < 0:
        raise ValueError("tip_reads")
    if any(v < 0 for v in lens):
        raise ValueError("negative")
    cl = None if clip is None else [int(v) for v in np.asarray(clip).reshape(-1)]
    if cl is not None and not (len(cl) == nv and all(0 <= cl[2 * i] <= cl[2 * i + 1] <= lens[i] for i in range(n))):
        raise ValueError("clip")
    cb = [0 if cl is None else cl[2 * i] for i in range(n)]
    ce = [lens[i] if cl is None else cl[2 * i + 1] for i in range(n)]
    cby = [int(v) for v in reads["contained_by"]]
    assert len(cby) == n
    state = [CONTAINED if cby[i] >= 0 else EMPTY if ce[i] == cb[i] else PLACED for i in range(n)]
    live = [s == PLACED for s in state]
    rows = list(zip(arcs["u"].tolist(), arcs["v"].tolist(), arcs["len"].tolist()))
    flags = arcs["flags"].tolist()
    for k, (u, v, ln) in enumerate(rows):
        if not (0 <= u < nv and 0 <= v < nv) or u >> 1 == v >> 1 or ln < 1:
            raise ValueError("arc %d out of range" % k)
    for k in range(1, len(rows)):
        a, b = rows[k - 1], rows[k]
        if not (a[0], a[2], a[1]) < (b[0], b[2], b[1]):
            raise ValueError("arcs not ascending at %d" % k)
    e0 = [k for k in range(len(rows)) if flags[k] == 0]
    in_e0 = set((rows[k][0], rows[k][1]) for k in e0)
    for k in e0:
        u, v, ln = rows[k]
        if not (live[u >> 1] and live[v >> 1]):
            raise ValueError("arc %d names a read that is not live" % k)
        if (v ^ 1, u ^ 1) not in in_e0:
            raise ValueError("arc %d has no complement" % k)
        if seqs is not None and ln > ce[u >> 1] - cb[u >> 1]:
            raise ValueError("arc %d is longer than its read" % k)
    if seqs is not None and (len(seqs) != n or any(len(seqs[i]) != lens[i] for i in range(n))):
        raise ValueError("read set")
    live_vertices = [x for x in range(nv) if live[x >> 1]]
    # the tip cut: one round on E0
    out, nxt, prv, _, _ = _joins(nv, rows, e0)
    linear, _ = _chains(live_vertices, nxt, prv)
    for chain in linear:
        h, t = chain[0], chain[-1]
        if len(chain) <= tip_reads and (out[h ^ 1] == 0 or out[t] == 0):
            for x in chain:
                state[x >> 1] = TIP
    e1 = [k for k in e0 if state[rows[k][0] >> 1] == PLACED and state[rows[k][1] >> 1] == PLACED]
    out, nxt, prv, jl, n_joins = _joins(nv, rows, e1)
    linear, cycles = _chains([x for x in live_vertices if state[x >> 1] == PLACED], nxt, prv)
    emitted = []                                     # (vertices, circular, the last take)
    for chain in linear:
        if chain[0] < chain[-1] ^ 1:
            emitted.append((chain, 0, ce[chain[-1] >> 1] - cb[chain[-1] >> 1]))
    for chain in cycles:
        m = min(min(chain), min(x ^ 1 for x in chain))
        if m in chain:
            at = chain.index(m)
            chain = chain[at:] + chain[:at]
            emitted.append((chain, 1, jl[chain[-1]]))
    emitted.sort(key=lambda e: e[0][0])
    placed = sum(len(e[0]) for e in emitted)
    utg = np.zeros(len(emitted), dtype=engine.UNITIG_DTYPE)
    layout = np.zeros(placed, dtype=engine.UNITIG_ENTRY_DTYPE)
    places = np.zeros(n, dtype=engine.UNITIG_PLACE_DTYPE)
    places["unitig"], places["rank"], places["state"] = -1, -1, state
    closing = set()
    at, seq_at = 0, 0
    for j, (chain, circular, last_take) in enumerate(emitted):
        start = 0
        for r, x in enumerate(chain):
            take = jl[x] if r + 1 < len(chain) else last_take
            layout[at + r] = (x, take, start)
            places[x >> 1] = (j, r, x & 1, PLACED)
            start += take
        utg[j] = (chain[0], chain[-1], len(chain), circular, at, seq_at, start)
        if circular:
            closing.update([(chain[-1], chain[0]), (chain[0] ^ 1, chain[-1] ^ 1)])
        at += len(chain)
        seq_at += start
    links = []
    ov = list(zip(arcs["ov_u"].tolist(), arcs["ov_v"].tolist()))
    for k in e1:
        u, v, _ = rows[k]
        if nxt[u] == v and (u, v) not in closing:
            continue
        pu, pv = places[u >> 1], places[v >> 1]
        links.append((int(pu["unitig"]), "+" if pu["orient"] == (u & 1) else "-", int(pv["unitig"]),
                      "+" if pv["orient"] == (v & 1) else "-", min(ov[k])))
    seq = None
    if seqs is not None:
        seq = np.zeros(seq_at, dtype=np.uint8)
        for j in range(len(utg)):
            for e in layout[int(utg[j]["layout_at"]):int(utg[j]["layout_at"]) + int(utg[j]["n_reads"])]:
                x, take, to = int(e["vertex"]), int(e["take"]), int(utg[j]["seq_at"]) + int(e["start"])
                seq[to:to + take] = oriented(seqs[x >> 1], cb[x >> 1], ce[x >> 1], x & 1)[:take]
    counts = dict(reads=n, placed=placed, cut=state.count(TIP), contained=state.count(CONTAINED), unitigs=len(utg),
                  circular=int(utg["circular"].sum()), longest_reads=int(utg["n_reads"].max()) if len(utg) else 0,
                  longest_bases=int(utg["length"].max()) if len(utg) else 0, e0_arcs=len(e0), e1_arcs=len(e1), joins=n_joins,
                  links=len(links))
    return dict(unitigs=utg, layout=layout, places=places, seq=seq, links=links, counts=counts)


def vertex_lists(result):
    """the unitigs of a result as lists of vertices"""
    return [result["layout"]["vertex"][int(u["layout_at"]):int(u["layout_at"]) + int(u["n_reads"])].tolist() for u in result["unitigs"]]


# ---- hand-made graphs

def make_arcs(rows):
    """[(u, v, len)] or [(u, v, len, flags)] -> GRAPH_ARC_DTYPE with every complement added (same flags; len as given by
    `rows` where they name it too, else the same len), ascending by (u, len, v); ov_u = ov_v = 1000 + the lower vertex"""
    full = {}
    for row in rows:
        u, v, ln = row[:3]
        fl = row[3] if len(row) > 3 else 0
        full[(u, v)] = (ln, fl)
    for (u, v), (ln, fl) in list(full.items()):
        full.setdefault((v ^ 1, u ^ 1), (ln, fl))
    order = sorted(full, key=lambda k: (k[0], full[k][0], k[1]))
    arcs = np.zeros(len(order), dtype=engine.GRAPH_ARC_DTYPE)
    for j, (u, v) in enumerate(order):
        arcs[j] = (u, v, full[(u, v)][0], 1000 + min(u, v), 1000 + min(u, v), j, 50, full[(u, v)][1])
    return arcs


def plain_reads(n, contained=()):
    reads = np.zeros(n, dtype=engine.GRAPH_READ_DTYPE)
    reads["contained_by"] = -1
    for i in contained:
        reads["contained_by"][i] = 7
    return reads


def path_rows(vertices, ln=1000, closed=False):
    """the arcs of a path (closed: a cycle) through `vertices`, len ln + position so that no two are alike"""
    rows = [(vertices[k], vertices[k + 1], ln + k) for k in range(len(vertices) - 1)]
    if closed:
        rows.append((vertices[-1], vertices[0], ln + len(vertices) - 1))
    return rows


def shuffled_vertices(rng, n, first_id=0, minus=None):
    """n reads with ids first_id .. first_id + n - 1 in a random order along a path, each on a random strand (minus: True / False
    forces every strand)"""
    ids = rng.permutation(n) + first_id
    strands = rng.integers(0, 2, n) if minus is None else np.full(n, int(minus))
    return [int(2 * i + s) for i, s in zip(ids, strands)]


def random_graph(n, seed):
    """-> (read_lens, reads, arcs, clip) of graph_model.graph() over the exact overlaps of n reads of 2000 .. 9000 bases laid at
    random on both strands of a genome of 600 n bases (about nine deep), every read clipped a little and one clipped to
    nothing, a fifth of the overlaps lost.  Pairs are found in genome order, so 3000 reads cost no 9 million looks"""
    import graph_model
    rng = np.random.default_rng([20261022, n, seed])
    layout = graph_model._random_layout(rng, n, 600 * n, 2000, 9000)
    lens = np.array([ln for _, ln, _ in layout], dtype=np.int32)
    clip = np.array([(int(rng.integers(0, 200)), ln - int(rng.integers(0, 200))) for ln in lens.tolist()], dtype=np.int32)
    clip[rng.integers(0, n)] = (1000, 1000)
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
    # a fifth of the records lost and the ends moved a little, as an aligner leaves them: branches, dead ends, short chains
    rec = graph_model.records_of([rows[k] for k in np.flatnonzero(rng.random(len(rows)) < 0.8).tolist()])
    for name in ("ab", "bb"):
        rec[name] += rng.integers(0, 60, len(rec))
    for name in ("ae", "be"):
        rec[name] -= rng.integers(0, 60, len(rec))
    g = graph_model.graph(rec, lens, clip=clip.reshape(-1), params=dict(max_hang=300, min_ovlp=600, fuzz=100))
    return lens, g["reads"], g["arcs"], clip.reshape(-1)


HAND_MADE = ("chain1", "chain64", "chain65", "chain257", "chain5000", "minus64", "fork", "two_tips", "tip_lengths", "reverse_tip",
             "isolated", "no_arcs", "cycle2", "cycle3", "cycle300", "cycle_minus", "cycle_beside", "cycle_tip", "skipped",
             "tiling128", "tiling129")


def hand_made(pattern, seed=20261020):
    """-> (read_lens int32, reads, arcs, clip or None) of one of HAND_MADE, the same on every call.  Reads are 5000 long"""
    rng = np.random.default_rng([seed, HAND_MADE.index(pattern)])
    clip = None
    contained = ()
    if pattern.startswith("chain") or pattern == "minus64":
        n = int(pattern[5:]) if pattern.startswith("chain") else 64
        vs = shuffled_vertices(rng, n, minus=True if pattern == "minus64" else None)
        if pattern == "minus64":                         # the lowest read at the tail, so that the head of the complement is lower
            vs.remove(1)
            vs.append(1)
        rows = path_rows(vs)
    elif pattern == "fork":
        # a backbone of 10 reads with a dead end of 2 out of read 4: once it is cut the two halves (5 reads each: no tips at 3)
        # join through read 4
        n = 12
        rows = path_rows([2 * i for i in range(10)]) + [(8, 20, 900), (20, 22, 1000)]
    elif pattern == "two_tips":
        # a backbone of 5 reads, and two dead ends of one read out of its last one: both are cut
        n = 7
        rows = path_rows([0, 2, 4, 6, 8]) + [(8, 10, 900), (8, 12, 950)]
    elif pattern == "tip_lengths":
        # a backbone of 16 reads; out of read 3 a dead end of 3 reads, out of read 7 one of 4 reads, out of read 9 one of 1
        n = 24
        rows = path_rows([2 * i for i in range(16)]) + [(6, 32, 700)] + path_rows([32, 34, 36]) + [(14, 38, 700)] + \
            path_rows([38, 41, 42, 45]) + [(18, 46, 700)]
    elif pattern == "reverse_tip":
        # a dead end that runs INTO read 4 of a backbone of 8: it has no arc into its head
        n = 10
        rows = path_rows([2 * i for i in range(8)]) + [(16, 19, 800), (19, 8, 700)]
    elif pattern == "isolated":
        # a chain of 3 reads and one of 4, nothing else
        n = 7
        rows = path_rows([0, 3, 4]) + path_rows([6, 8, 11, 12])
    elif pattern == "no_arcs":
        n = 3
        rows = []
    elif pattern in ("cycle2", "cycle3", "cycle300"):
        n = int(pattern[5:])
        rows = path_rows(shuffled_vertices(rng, n), closed=True)
    elif pattern == "cycle_minus":
        # the stored orientation of the cycle holds read 0 on its minus strand: the emitted orientation is the complement
        n = 5
        rows = path_rows([1, 4, 7, 2, 8], closed=True)
    elif pattern == "cycle_beside":
        n = 40
        rows = path_rows(shuffled_vertices(rng, 12, 0)) + path_rows(shuffled_vertices(rng, 9, 12), closed=True) + \
            path_rows(shuffled_vertices(rng, 19, 21))
    elif pattern == "cycle_tip":
        # a cycle of 6 reads with a dead end of 2 out of one of them
        n = 8
        rows = path_rows([4, 2, 9, 6, 0, 11], closed=True) + [(9, 12, 600), (12, 15, 1000)]
    elif pattern == "skipped":
        # a chain of 6; read 6 is contained, read 7 has an empty clip, and two arcs carry flags != 0
        n = 8
        rows = path_rows([0, 3, 4, 7, 8, 10]) + [(0, 4, 2500, 1), (3, 7, 2600, 2)]
        contained = (6,)
        clip = np.array([(100, 4900)] * 7 + [(2000, 2000)], dtype=np.int32).reshape(-1)
    elif pattern in ("tiling128", "tiling129"):
        # reads in id order on random strands, joined in pieces of five; left over are reads 125 .. 127, a piece of three, and of
        # 129 reads the last one alone.  256 vertices are the last that one chunk of the scan holds; the last two of 258 are the
        # first behind its carry, and where no tip is cut read 128 is a unitig whose head is vertex 256
        n = int(pattern[6:])
        vs = [int(2 * i + s) for i, s in enumerate(rng.integers(0, 2, n))]
        rows = [row for a in range(0, 128, 5) for row in path_rows(vs[a:min(a + 5, 128)])]
    else:
        raise ValueError(pattern)
    return np.full(n, 5000, dtype=np.int32), plain_reads(n, contained), make_arcs(rows), clip
