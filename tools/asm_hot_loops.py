"""The DP loops of the three hot linear-gap kernels in a device assembly listing (hipcc -O3 -S --cuda-device-only):
VALU instructions per DP step, split into the recurrence and what surrounds it, beside each kernel's registers, spills,
scratch and LDS.  A sibling of tools/asm_loops.py (which lists every loop of a file).

python tools/asm_hot_loops.py file.s

A loop is an innermost backward branch whose body holds v_pk_maximum3_f16 (one per column slot and step).  The kind of
step follows from the instruction mix: v_bitop3_b32 marks a slot of the pointer phase, and the number of slots per step
tells the split pass's two-region steps (7 + 13 slots) from its one-region steps (13 or 7).  Recurrence instructions
per slot: 5 on plain scores in the row-drifted frame, 4 in the column-drifted frame of the split pass (gact_lin.hpp 2.: its
hand-overs are v_sub_u32_dpp, which is how a loop of that frame is told), 8 where pointers are made, 10 with the seed
launch's arg-max key.  Beside s_nop the scalar additions per step (the split pass moves its zero levels on the scalar unit)
and the lane-spill instructions (v_readlane_b32 / v_writelane_b32) inside the loop.  "all": every instruction per step, whatever
unit issues it -- a wave issues in order, so each takes a place in its stream.  The s_nop are reported in two parts: those that
stand directly behind a scalar addition ("nop<add": the hazard recogniser puts one behind an inline-asm statement) and the rest."""
import re
import sys
from collections import Counter

HOT = (("extend_coop_kernel", "extend_coop_kernelINS_14SplitLayoutLinILi7ELi13EEELb0EE"),
       ("extend_p16_kernel<SplitLayoutLin>", "extend_p16_kernelINS_14SplitLayoutLinILi7ELi13EEELb0ELb0EE"),
       ("seed_p16_kernel<20,false,1>", "seed_p16_kernelILi20ELb0ELi1EE"))
# (slots on plain scores, slots with pointers) per step -> name, for the split pass (7 + 13) and the uniform one (20)
KINDS = {(20, 0): "step", (7, 13): "step_tagged", (0, 13): "step_tagged_r2", (7, 0): "step_r1", (0, 20): "step_tagged (uniform)"}


def is_inst(line):
    return re.match(r"^\s+(v_|s_|ds_|scratch_|buffer_|global_|flat_)", line) is not None


def loops_of(lines):
    labels = {m.group(1): k for k, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    spans = []
    for k, l in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)      # (a loop may close with an unconditional s_branch)
        if m and labels.get(m.group(1), k + 1) <= k:
            spans.append((labels[m.group(1)], k, m.group(1)))
    inner = [s for s in spans if not any(o is not s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    return inner


def describe(name, lines, meta):
    print("%s" % name)
    print("  vgprs %s  vgpr spills %s  sgpr spills %s  scratch %s B  LDS %s B  code %d lines" % (
        meta.get("vgpr_count", "?"), meta.get("vgpr_spill_count", "?"), meta.get("sgpr_spill_count", "?"),
        meta.get("private_segment_fixed_size", "?"), meta.get("group_segment_fixed_size", "?"), sum(1 for l in lines if is_inst(l))))
    print("  %-24s %6s %8s %6s %11s %9s %5s %4s %6s %7s %6s %8s %10s" % ("loop", "steps", "all/step", "VALU", "VALU/step", "recurr.", "rest", "LDS", "s_nop", "nop<add", "s_add", "scratch", "lane spill"))
    for a, b, label in loops_of(lines):
        insts = [l.split()[0] for l in lines[a:b + 1] if is_inst(l)]
        c = Counter(insts)
        nop_add = sum(1 for p, q in zip(insts, insts[1:]) if q == "s_nop" and p.startswith("s_add"))
        n_max3 = c.get("v_pk_maximum3_f16", 0)
        if n_max3 == 0:
            continue
        valu = sum(v for n, v in c.items() if n.startswith("v_"))
        n_ptr = c.get("v_bitop3_b32", 0)
        kind, steps, rec = "?", 1, 0
        for (plain, ptr), kname in KINDS.items():
            per = plain + ptr
            if n_max3 % per == 0 and n_ptr == ptr * (n_max3 // per):
                amax = kname.endswith("(uniform)") and c.get("v_pk_mad_u16", 0) >= 2 * n_max3
                col_drift = c.get("v_sub_u32_dpp", 0) > 0
                kind, steps, rec = kname, n_max3 // per, plain * (4 if col_drift else 5) + ptr * (10 if amax else 8)
                break
        print("  %-24s %6d %8.1f %6d %11.1f %9d %5.1f %4.1f %6.1f %7.1f %6.1f %8d %10d" % (
            kind + " " + label, steps, len(insts) / steps, valu, valu / steps, rec, valu / steps - rec,
            sum(v for n, v in c.items() if n.startswith("ds_")) / steps, (c.get("s_nop", 0) - nop_add) / steps, nop_add / steps,
            sum(v for n, v in c.items() if n.startswith("s_add")) / steps,
            sum(v for n, v in c.items() if n.startswith("scratch_")),
            c.get("v_readlane_b32", 0) + c.get("v_writelane_b32", 0)))


def main():
    text = open(sys.argv[1]).read().splitlines()
    starts = [(k, l.split(":")[0]) for k, l in enumerate(text) if re.match(r"^_Z\w+:", l)]
    for name, key in HOT:
        for n, (k, sym) in enumerate(starts):
            if key in sym:
                end = starts[n + 1][0] if n + 1 < len(starts) else len(text)
                # (the record's fields come in alphabetical order around .name: gather both sides)
                meta = {}
                hit = [i for i, l in enumerate(text) if re.match(r"^\s+\.name:\s+%s\s*$" % re.escape(sym), l)]
                if hit:
                    i = hit[0]
                    lo = i
                    while lo > 0 and not text[lo].startswith("  - "):
                        lo -= 1
                    hi = i
                    while hi + 1 < len(text) and not text[hi + 1].startswith("  - ") and not text[hi + 1].startswith("amdhsa"):
                        hi += 1
                    for l in text[lo:hi + 1]:
                        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\d+)\s*$", l)
                        if m:
                            meta[m.group(1)] = m.group(2)
                describe(name, text[k:end], meta)
                break
        else:
            print("%s: not in this file" % name)


if __name__ == "__main__":
    main()
