#!/usr/bin/env python
"""Which kernels did a change touch?  Compares the gfx950 assembly of two builds kernel by kernel (no GPU needed).

Compile the sources of both builds with the flags of waiwera_amd/build.py plus -save-temps; every translation unit
leaves a <name>-hip-amdgcn-amd-amdhsa-gfx950.s.  Then

    python tools/compare_kernel_asm.py --old OLD.s [OLD2.s ...] --new NEW.s [NEW2.s ...] [--diff]

For every kernel symbol (.amdhsa_kernel NAME) the instruction stream from the symbol's label to its end and the
.amdhsa_* descriptor block (registers, LDS, scratch) are compared after normalisation: the compiler's `;` comments are
dropped and the labels that carry the function's index in its file (.LBB12_3, .LJTI12_0) lose that index.  File-level
directives and the order of the kernels are ignored.  A kernel may move between translation units; it must not
appear in two of one build.  Exit status 0: same kernel names on both sides, none twice, all identical.
--diff prints a unified diff of every kernel that differs.
"""
import argparse
import difflib
import re
import subprocess
import sys

LABEL = re.compile(r"\.L([A-Za-z]+)\d+_(\d+)")
GETPC = re.compile(r"\.Lpost_getpc\d+")   # numbered through the file, in the order the functions are emitted


def norm(line):
    line = line.split(";", 1)[0].strip()
    return GETPC.sub(".Lpost_getpc", LABEL.sub(r".L\1_\2", line))


def kernels(path):
    """{symbol: (instruction lines, descriptor lines)} of one assembly file"""
    lines = open(path).read().split("\n")
    label = {}   # symbol -> line index of its label
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", l)
        if m:
            label.setdefault(m.group(1), i)
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        name = m.group(1)
        end = i
        while not lines[end].strip().startswith(".end_amdhsa_kernel"):
            end += 1
        desc = [norm(x) for x in lines[i + 1:end]]
        j = label[name] + 1
        body = []
        while j < i and not re.match(r"^\s*\.section\s", lines[j]) and not lines[j].startswith(".Lfunc_end"):
            body.append(norm(lines[j]))
            j += 1
        out[name] = ([x for x in body if x], [x for x in desc if x])
    return out


def collect(paths, side):
    allk, twice = {}, []
    for p in paths:
        k = kernels(p)
        print("%s %-60s %4d kernels" % (side, p[-60:], len(k)))
        for name, v in k.items():
            if name in allk:
                twice.append(name)
            allk[name] = v
    return allk, twice


def demangle(names):
    if not names:
        return []
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return [re.sub(r"\(.*", "", x).replace("void wai::", "") for x in r.stdout.split("\n")[:len(names)]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--diff", action="store_true")
    a = ap.parse_args()
    old, old2 = collect(a.old, "old")
    new, new2 = collect(a.new, "new")
    only_old = sorted(set(old) - set(new))
    only_new = sorted(set(new) - set(old))
    code, regs = [], []
    for name in sorted(set(old) & set(new)):
        if old[name][0] != new[name][0]:
            code.append(name)
        if old[name][1] != new[name][1]:
            regs.append(name)
    print("kernels: old %d, new %d, in both %d" % (len(old), len(new), len(set(old) & set(new))))
    for what, names in (("only in old", only_old), ("only in new", only_new), ("twice in old", old2), ("twice in new", new2),
                        ("instruction stream differs", code), ("descriptor differs", regs)):
        print("%-28s %d" % (what + ":", len(names)))
        for n in demangle(names):
            print("    " + n)
    if a.diff:
        for name in sorted(set(code) | set(regs)):
            print("==== " + demangle([name])[0])
            for k in (0, 1):
                sys.stdout.write("\n".join(difflib.unified_diff(old[name][k], new[name][k], "old", "new", lineterm="", n=2)) + "\n")
    ok = not (only_old or only_new or old2 or new2 or code or regs)
    print("identical: %d of %d" % (len(set(old) & set(new)) - len(set(code) | set(regs)), len(old)) + ("" if ok else "   FAILED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
