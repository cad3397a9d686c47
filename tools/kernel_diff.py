"""Per-kernel comparison of two builds' device assembly (no GPU needed):
   hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S FILE.hip -o DIR/FILE.s   for both builds, then
   python tools/kernel_diff.py PARENT_DIR NEW_DIR FILE.s [FILE.s ...]
Kernels are matched by demangled name with namespaces stripped.  Per kernel: code length, registers, scratch, static LDS and
occupancy as the assembler comments state them, and the instruction stream -- comments and directives dropped, labels and
symbol names normalised -- either identical or with the number of lines of the longer stream outside the longest common
subsequence and the opcode counts that differ."""
import collections
import difflib
import os
import re
import subprocess
import sys

FIELDS = ["codeLenInByte", "TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy"]
RESOURCES = ["NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy"]


def kernels(path):
    out = {}
    name, body = None, []
    lines = open(path).read().splitlines()
    for i, line in enumerate(lines):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            info = {}
            for l2 in lines[i:i + 80]:
                m2 = re.match(r"^; (\w+)\s*[:=] (\d+)", l2)
                if m2 and m2.group(1) in FIELDS and m2.group(1) not in info:
                    info[m2.group(1)] = int(m2.group(2))
            out[name] = (body, info)
            name = None
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") and not s.endswith(":"):
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        s = re.sub(r"_Z\w+", "SYM", s)
        body.append(s)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, r):
        d = re.sub(r"\(anonymous namespace\)::|pn::", "", d)
        d = re.sub(r"^void ", "", d)
        short[n] = re.sub(r"\(.*\)$", "", d)
    return short


def opcodes(body):
    return collections.Counter(l.split()[0] for l in body if not l.endswith(":"))


def main():
    pdir, ndir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    moved = 0
    for f in files:
        a, b = kernels(os.path.join(pdir, f)), kernels(os.path.join(ndir, f))
        da, db = demangle(list(a)), demangle(list(b))
        A, B = {da[k]: a[k] for k in a}, {db[k]: b[k] for k in b}
        print("%s  kernels: parent %d, new %d; missing %s; new %s" % (f, len(A), len(B), sorted(set(A) - set(B)), sorted(set(B) - set(A))))
        print("   %-34s %9s %5s %5s %5s %7s %7s %4s  %-9s stream (instr: differing lines / parent's; opcode counts new - parent)" %
              ("kernel", "codeLen", "SGPR", "VGPR", "AGPR", "scratch", "LDS", "occ", "resources"))
        same = 0
        for k in sorted(set(A) & set(B)):
            (ba, ia), (bb, ib) = A[k], B[k]
            res = "equal" if all(ia.get(x) == ib.get(x) for x in RESOURCES) else "MOVED"
            moved += res != "equal"
            if ba == bb:
                stream = "identical (%d)" % len(ba)
                same += 1
            else:
                sm = difflib.SequenceMatcher(None, ba, bb, autojunk=False)
                common = sum(blk.size for blk in sm.get_matching_blocks())
                oa, ob = opcodes(ba), opcodes(bb)
                d = {o: ob[o] - oa[o] for o in set(oa) | set(ob) if ob[o] != oa[o]}
                stream = "differs: %d / %d; %s" % (max(len(ba), len(bb)) - common, len(ba),
                                                   " ".join("%s %+d" % kv for kv in sorted(d.items())) or "opcode counts equal")
            cl = "%d" % ib.get("codeLenInByte", -1)
            if ib.get("codeLenInByte") != ia.get("codeLenInByte"):
                cl += "(%+d)" % (ib.get("codeLenInByte", 0) - ia.get("codeLenInByte", 0))
            print("   %-34s %9s %5d %5d %5d %7d %7d %4d  %-9s %s" % (k[:34], cl, ib.get("TotalNumSgprs", -1), ib.get("NumVgprs", -1),
                  ib.get("NumAgprs", -1), ib.get("ScratchSize", -1), ib.get("LDSByteSize", -1), ib.get("Occupancy", -1), res, stream))
            if res != "equal":
                print("      parent: " + " ".join("%s %s" % (x, ia.get(x)) for x in RESOURCES))
        print("   identical streams: %d of %d" % (same, len(set(A) & set(B))))
    print("kernels with a differing register / scratch / LDS / occupancy figure: %d" % moved)


if __name__ == "__main__":
    main()
