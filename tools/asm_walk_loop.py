"""The traceback walk of the cooperative kernel (coop_walk_batch, gact_coop.hpp) in a device assembly listing
(hipcc -O3 -S --cuda-device-only): instructions per move and per refill, by the unit that issues them.  A sibling of
tools/asm_hot_loops.py.

python tools/asm_walk_loop.py file.s [--dump]

The walk is the innermost loop of extend_coop_kernel that holds v_bfe_u32 and ds_read_b32 and no v_pk_maximum3_f16; loops are
read off the compiler's block comments, since a loop's blocks need not be adjacent.  Two shapes are told apart by whether
that loop holds the refill's global_load_dwordx4:
  * it does not: the loop is ONE move, and the refill block is the loop around it without the move loop's blocks;
  * it does: the loop is a whole trip -- the block with the loads is the refill block, the others are straight-line moves
    and the trip's one exit test; the moves are counted by their LDS waits (a move that fetches has one wait for its
    reads; the trip's last move fetches nothing) and the figures are per move.
In the first shape the move loop has side paths, blocks that end in an unconditional branch (the trip's last move, the
way out); they are listed apart from the blocks every ordinary move runs.
SALU is every s_ instruction, s_waitcnt, s_nop and branches among them; those three are listed on their own as well.
--dump prints the loop's instructions as well."""
import re
import sys
from collections import Counter

KERNELS = (("extend_coop_kernel", "extend_coop_kernelINS_14SplitLayoutLinILi7ELi13EEELb0EE"),
           ("extend_coop_kernel (two sets)", "extend_coop_kernelINS_14SplitLayoutLinILi7ELi13EEELb1EE"),
           ("extend_coop_kernel<SplitLayoutLinRow>", "extend_coop_kernelINS_17SplitLayoutLinRowILi7ELi13EEELb0EE"),
           ("extend_coop_kernel<SplitLayoutLinRow> (two sets)", "extend_coop_kernelINS_17SplitLayoutLinRowILi7ELi13EEELb1EE"))


def is_inst(line):
    return re.match(r"^\s+(v_|s_|ds_|scratch_|buffer_|global_|flat_)", line) is not None


def loops_of(lines):
    """{header: (depth, [blocks])}, a block a list of line indices, from the compiler's own block comments: a block opens
    at a label or a `; %bb.N:` line and says which loop it is in ("in Loop: Header=BB1_2 Depth=3"; a header says
    "This [Inner] Loop Header: Depth=3" in the comment lines behind its label).  The blocks of a loop's child loops name
    the child, so a loop's blocks here are its own and not its children's; they need not be adjacent in the file."""
    loops, cur, k = {}, None, 0
    while k < len(lines):
        l = lines[k]
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", l)
        if m:
            cur = None
            note, j = l, k + 1
            while j < len(lines) and re.match(r"^\s+;", lines[j]) and "implicit-def" not in lines[j]:
                note += lines[j]
                j += 1
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
            d = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", note)
            if d and m.group(1):
                cur = m.group(1)
                loops.setdefault(cur, (int(d.group(1)), []))
            elif h:
                cur = h.group(1)
                loops.setdefault(cur, (int(h.group(2)), []))
            if cur is not None:
                loops[cur][1].append([])
        elif cur is not None and is_inst(l):
            loops[cur][1][-1].append(k)
        k += 1
    return loops


def tally(insts):
    c = Counter(insts)
    return {"all": len(insts),
            "VALU": sum(v for n, v in c.items() if n.startswith("v_")),
            "SALU": sum(v for n, v in c.items() if n.startswith("s_")),
            "LDS": sum(v for n, v in c.items() if n.startswith("ds_")),
            "global": sum(v for n, v in c.items() if n.startswith("global_")),
            "s_waitcnt": c.get("s_waitcnt", 0), "s_nop": c.get("s_nop", 0), "v_mad_u64_u32": c.get("v_mad_u64_u32", 0),
            "branch": sum(v for n, v in c.items() if n.startswith("s_branch") or n.startswith("s_cbranch")),
            "scratch": sum(v for n, v in c.items() if n.startswith("scratch_")),
            "lane spill": c.get("v_readlane_b32", 0) + c.get("v_writelane_b32", 0)}


COLS = ("all", "VALU", "SALU", "LDS", "global", "s_waitcnt", "s_nop", "v_mad_u64_u32", "branch", "scratch", "lane spill")


def row(name, t, per):
    print("  %-44s" % name + "".join(" %13s" % (("%.1f" % (t[k] / per)) if per != 1 else "%d" % t[k]) for k in COLS))


def describe(name, lines, dump):
    print(name)
    print("  code %d instructions" % sum(1 for l in lines if is_inst(l)))
    loops = loops_of(lines)

    def names(blocks):
        return [lines[k].split()[0] for blk in blocks for k in blk]

    def is_walk(blocks):
        c = Counter(names(blocks))
        return c.get("v_bfe_u32", 0) > 0 and (c.get("ds_read_b32", 0) > 0) and c.get("v_pk_maximum3_f16", 0) == 0

    def first(blocks):
        return min(k for blk in blocks for k in blk)

    def last(blocks):
        return max(k for blk in blocks for k in blk)

    # innermost: no deeper walk loop stands between this loop's first and last line
    walk = [(h, d, [blk for blk in blocks if blk]) for h, (d, blocks) in loops.items() if any(blocks) and is_walk(blocks)]
    walk = [w for w in walk if not any(o[1] > w[1] and first(w[2]) <= first(o[2]) <= last(w[2]) for o in walk)]
    if not walk:
        print("  no walk loop found")
        return
    print("  %-44s" % "" + "".join(" %13s" % k for k in COLS))
    for h, d, blocks in walk:
        shown = blocks
        if "global_load_dwordx4" not in names(blocks):
            # one move per trip round the loop.  A block that ends in an unconditional branch is a side path (the trip's last
            # move, which tests the band and fetches nothing; the way out): an ordinary move runs the others.
            side = [blk for blk in blocks if lines[blk[-1]].split()[0] == "s_branch"]
            main = [blk for blk in blocks if blk not in side]
            row("move loop %s: a move that fetches" % h, tally(names(main)), 1)
            row("move loop %s: side paths" % h, tally(names(side)), 1)
            for oh, (od, oblocks) in loops.items():
                oblocks = [blk for blk in oblocks if blk]
                if od == d - 1 and oblocks and first(oblocks) <= first(blocks) <= last(oblocks):
                    row("refill block %s (per 8 moves)" % oh, tally(names(oblocks)), 1)
                    shown = blocks + oblocks
        else:
            refill = [blk for blk in blocks if "global_load_dwordx4" in names([blk])]
            rest = [blk for blk in blocks if blk not in refill]
            moves = 1 + sum(1 for blk in rest for k in blk if lines[k].split()[0] == "s_waitcnt" and "lgkmcnt" in lines[k])
            row("trip loop %s: per move (%d moves)" % (h, moves), tally(names(rest)), moves)
            row("trip loop %s: the moves of a trip" % h, tally(names(rest)), 1)
            row("refill block %s (per %d moves)" % (h, moves), tally(names(refill)), 1)
        if dump:
            for k in sorted(k for blk in shown for k in blk):
                print("      | %7d %s" % (k, lines[k].rstrip()))


def main():
    dump = "--dump" in sys.argv
    path = [a for a in sys.argv[1:] if not a.startswith("--")][0]
    text = open(path).read().splitlines()
    starts = [(k, l.split(":")[0]) for k, l in enumerate(text) if re.match(r"^_Z\w+:", l)]
    for name, key in KERNELS:
        for n, (k, sym) in enumerate(starts):
            if key in sym:
                end = starts[n + 1][0] if n + 1 < len(starts) else len(text)
                describe(name, text[k:end], dump)
                break
        else:
            print("%s: not in this file" % name)


if __name__ == "__main__":
    main()
