#!/usr/bin/env python3
"""Compare two rocprofv3 --kernel-trace runs of the same program dispatch by dispatch: route identity of two library builds.

  rocprofv3 --kernel-trace --stats -d DIR_A -- python -m pytest -m gpu tests/test_fused_paths.py ...     (one build)
  rocprofv3 --kernel-trace --stats -d DIR_B -- ...                                                        (the other)
  python scripts/trace_diff.py DIR_A DIR_B [ROWS]

Every *_kernel_trace.csv under a directory is read and all dispatches are put in start order; the two sequences are compared
row by row on (kernel name, grid x / y / z, workgroup x / y / z). A generated fused kernel carries a
digest of its whole signature in its name, so an equal name is an equal kernel. Prints the dispatch counts, the number of
differing rows and the first ROWS of them (default 10). Exit status 1 if any row differs or the counts do.
Meant for runs of ONE process that launches on one stream: with several processes in a directory their dispatches interleave by
timestamp, and that order is not the same from run to run.
"""
import csv
import glob
import sys

KEYS = ("Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z")


def dispatches(root):
    rows = []
    files = sorted(glob.glob(root + "/**/*_kernel_trace.csv", recursive=True))
    if not files:
        raise SystemExit("%s: no *_kernel_trace.csv" % root)
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    return [tuple(r[k] for k in KEYS) for r in rows]


def show(row):
    return "%s  grid %s x %s x %s  workgroup %s x %s x %s" % row


def main():
    a, b = dispatches(sys.argv[1]), dispatches(sys.argv[2])
    show_rows = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    differ = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
    print("dispatches: %s %d, %s %d" % (sys.argv[1], len(a), sys.argv[2], len(b)))
    print("differing dispatches: %d" % len(differ))
    for i in differ[:show_rows]:
        print("  #%d\n    %s\n    %s" % (i, show(a[i]), show(b[i])))
    if not differ:
        print("first difference: none")
    na, nb = set(r[0] for r in a), set(r[0] for r in b)
    print("distinct kernel names: %d, %d (%s)" % (len(na), len(nb), "the same set" if na == nb else "%d only in the first, %d only in the second" % (len(na - nb), len(nb - na))))
    return 1 if differ or len(a) != len(b) else 0


if __name__ == "__main__":
    sys.exit(main())
