#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of the same translation unit, kernel by kernel.

  hipcc <the Makefile's flags> --cuda-device-only -S gemm.hip -o new.s      (and the same for the other commit)
  python scripts/isa_diff.py old.s new.s > table.txt

Per kernel symbol the instruction streams are compared with comments stripped and basic-block labels numbered in
order of appearance. Classes:
  A  the whole instruction stream is equal
  B  from the first instruction through the last v_mfma the streams are equal, as they stand ("B") or after ONE
     consistent one-to-one renaming of registers ("B*"); the same number of instructions in that span; equal resource
     figures (VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes, occupancy)
  C  anything else
A compile is not a run: the table says what the compiler made, not how fast it is. Exit status 1 if any kernel is C or
the two listings do not hold the same kernels.
"""
import re
import subprocess
import sys

FIGURES = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("sgpr", "TotalNumSgprs"), ("lds", "LDSByteSize"), ("scratch", "ScratchSize"), ("occ", "Occupancy"))
REG = re.compile(r"\b([vsa])(?:(\d+)|\[(\d+):(\d+)\])(?![\w\[])")
LABEL_DEF = re.compile(r"^(\.LBB\d+_\d+):")
LABEL_USE = re.compile(r"\.LBB\d+_\d+")


def kernels(path):
    """{symbol: (instruction lines, figures)} of the kernels (.amdhsa_kernel) in a listing"""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for name in names:
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:\n(.*?;\s*Occupancy:\s*\d+)" % re.escape(name), text, re.M | re.S)
        if not m:
            raise SystemExit("%s: no body for %s" % (path, name))
        labels, lines = {}, []
        for raw in m.group(1).splitlines():
            line = raw.split(";")[0].strip()
            if not line:
                continue
            d = LABEL_DEF.match(line)
            if d:
                labels.setdefault(d.group(1), "L%d" % len(labels))
                lines.append(labels[d.group(1)] + ":")
            elif not line.startswith("."):
                lines.append(" ".join(line.split()))
        # (a label used before its definition keeps the number of its definition: second pass)
        lines = [LABEL_USE.sub(lambda u: labels.get(u.group(0), u.group(0)), l) for l in lines]
        fig = {}
        for key, word in FIGURES:
            f = re.search(r";\s*%s:\s*(\d+)" % word, m.group(2))
            fig[key] = int(f.group(1)) if f else -1
        out[name] = (lines, fig)
    return out


def regs(line):
    found = []
    for m in REG.finditer(line):
        lo = int(m.group(2) if m.group(2) is not None else m.group(3))
        hi = int(m.group(2) if m.group(2) is not None else m.group(4))
        found.append((m.group(1), lo, hi))
    return found


def renamed_equal(a, b):
    """the two spans are equal under one bijection of registers"""
    if len(a) != len(b):
        return False
    fwd, back = {}, {}
    for x, y in zip(a, b):
        if REG.sub("R", x) != REG.sub("R", y):
            return False
        for (c1, lo1, hi1), (c2, lo2, hi2) in zip(regs(x), regs(y)):
            if c1 != c2 or hi1 - lo1 != hi2 - lo2:
                return False
            for k in range(hi1 - lo1 + 1):
                p, q = (c1, lo1 + k), (c2, lo2 + k)
                if fwd.setdefault(p, q) != q or back.setdefault(q, p) != p:
                    return False
    return True


def mfma_span(lines):
    last = max((i for i, l in enumerate(lines) if l.startswith("v_mfma")), default=-1)
    return lines[: last + 1]


def classify(old, new):
    (la, fa), (lb, fb) = old, new
    if la == lb:
        return "A"
    sa, sb = mfma_span(la), mfma_span(lb)
    if not sa or fa != fb or len(sa) != len(sb):
        return "C"
    if sa == sb:
        return "B"
    return "B*" if renamed_equal(sa, sb) else "C"


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, (o.replace("(anonymous namespace)::", "").replace("void ", "", 1) for o in out)))
    except Exception:
        return {n: n for n in names}


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pretty = demangle(sorted(set(old) | set(new)))
    counts, bad = {}, sorted(set(old) ^ set(new))
    fmt = lambda f: "%3d v %3d a %3d s %6d lds %4d scr occ %d" % tuple(f[k] for k, _ in FIGURES)
    print("# class | old figures | new figures | instructions old / new (through the last v_mfma: old / new) | kernel")
    for name in sorted(set(old) & set(new), key=lambda n: pretty[n]):
        c = classify(old[name], new[name])
        counts[c] = counts.get(c, 0) + 1
        ia = sum(not l.endswith(":") for l in old[name][0]), sum(not l.endswith(":") for l in new[name][0])
        im = sum(not l.endswith(":") for l in mfma_span(old[name][0])), sum(not l.endswith(":") for l in mfma_span(new[name][0]))
        print("%-2s | %s | %s | %5d / %5d (%5d / %5d) | %s" % (c, fmt(old[name][1]), fmt(new[name][1]), ia[0], ia[1], im[0], im[1], pretty[name]))
    for name in bad:
        print("?? only in %s: %s" % ("old" if name in old else "new", pretty[name]))
    print("# %d kernels: %s" % (len(set(old) & set(new)), ", ".join("%s %d" % kv for kv in sorted(counts.items()))))
    return 1 if bad or counts.get("C") else 0


if __name__ == "__main__":
    sys.exit(main())
