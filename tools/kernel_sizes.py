"""Size of every kernel symbol in a device assembly listing of the engine: instructions, VGPRs, SGPRs, the two spill
counts, scratch bytes per lane and LDS bytes per block, one line per symbol, sorted by name.

python tools/kernel_sizes.py [-D flags ...]       compiles the listing first (build/engine.s, device side only)
python tools/kernel_sizes.py file.s               reads one made before:
                                                  hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -S --cuda-device-only
python tools/kernel_sizes.py parent.s change.s    the symbols that differ between two listings (gone, new, changed)

An instruction is an indented line between a kernel's label and its end label that is neither a directive nor a
comment; the other columns are the fields of the kernel's record in the listing's amdhsa.kernels metadata."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
HEAD = "%-90s %6s %5s %6s %5s %6s %8s %6s" % ("kernel", "insts", "vgpr", "spill", "sgpr", "spill", "scratch", "LDS")


def compile_listing(flags):
    out = os.path.join(ROOT, "build", "engine.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                           "--cuda-device-only"] + flags + ["-o", out, os.path.join(ROOT, "darwin-gpu_amd", "csrc", "gact_engine.hip")],
                          stderr=subprocess.DEVNULL)
    return out


def sizes(path):
    """{demangled kernel name: (instructions, vgprs, vgpr spills, sgprs, sgpr spills, scratch bytes, LDS bytes)}"""
    lines = open(path).read().splitlines()
    # the metadata records: "  - " opens one, its scalar fields sit at four spaces
    meta, rec = {}, None
    for l in lines:
        if l.startswith("  - "):
            rec = {}
            l = "    " + l[4:]
        m = re.match(r"^    \.(\w+):\s+(\S+)\s*$", l)
        if m and rec is not None:
            rec[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = rec
    count, sym = {}, None
    for l in lines:
        m = re.match(r"^(\w+):", l)
        if m and m.group(1) in meta:
            sym = m.group(1)
            count[sym] = 0
        elif l.startswith(".Lfunc_end"):
            sym = None
        elif sym and re.match(r"^\s+[A-Za-z_]", l):
            count[sym] += 1
    syms = sorted(count)
    names = subprocess.run(["c++filt"] + syms, capture_output=True, text=True, check=True).stdout.splitlines()
    short = [n.split("(")[0].replace("void ", "").replace("gact::", "") for n in names]
    return {n: (count[s],) + tuple(int(meta[s][f]) for f in FIELDS) for s, n in zip(syms, short)}


def row(name, v):
    return "%-90s %6d %5d %6d %5d %6d %8d %6d" % ((name[:90],) + v)


def main():
    files = [a for a in sys.argv[1:] if a.endswith(".s")]
    if not files:
        files = [compile_listing(sys.argv[1:])]
    tables = [sizes(f) for f in files[:2]]
    print(HEAD)
    if len(tables) == 1:
        for name in sorted(tables[0]):
            print(row(name, tables[0][name]))
        return
    a, b = tables
    same = 0
    for name in sorted(set(a) | set(b)):
        if a.get(name) == b.get(name):
            same += 1
            continue
        if name in a:
            print("- " + row(name, a[name]))
        if name in b:
            print("+ " + row(name, b[name]))
    print("%d symbols in %s, %d in %s, %d the same in every column" % (len(a), files[0], len(b), files[1], same))


if __name__ == "__main__":
    main()
