#!/usr/bin/env python3
"""Compare two device-assembly listings of one translation unit, function by function.

    hipcc <Makefile FLAGS> <DEVFLAGS> --cuda-device-only -S unit.hip -o A.s      (at two commits)
    python scripts/kernel_text_diff.py A.s B.s

For two whole trees, `scripts/ab.py text PARENT_TREE CHANGE_TREE` makes the listings of every unit with each tree's own Makefile flags and
calls main() per unit.

A symbol is everything from its `name:` line to `.Lfunc_end` (a data symbol: to its `.size`); comments, debug / section directives and the
names of local labels are dropped, so two listings are "identical" when their instructions and operands are.
Exit status 1 when a function was added or differs (data symbols, `.type name,@object`, may: the per-unit
__hip_cuid_* is a hash of the source)."""
import re
import sys


def split(path):
    out, cur, data = {}, None, set()
    for line in open(path):
        t = re.match(r"^\s*\.type\s+(\w+),@object", line)
        if t:
            data.add(t.group(1))
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is None or line.lstrip().startswith(";") or re.match(r"^\s*\.(loc|file|ident|section|cfi)", line):
            continue
        elif line.startswith(".Lfunc_end") or re.match(r"\s*\.size\s", line):
            cur = None
        else:
            out[cur].append(re.sub(r"\.L\w+", "L", line.split(";")[0].rstrip()))
    return out, data


def main(path_a, path_b):
    (a, data_a), (b, data_b) = split(path_a), split(path_b)
    removed, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    same = [k for k in b if k in a and a[k] == b[k]]
    diff = [k for k in b if k in a and a[k] != b[k]]
    print(f"{path_a} -> {path_b}")
    for title, names in (("removed", removed), ("added", added), ("different", diff)):
        print(f"  {title}: {len(names)}")
        for k in names:
            print(f"    {k}" + (f"  ({len(a[k])} -> {len(b[k])} lines)" if title == "different" else "") + ("  [data]" if k in data_a | data_b else ""))
    print(f"  identical: {len(same)}")
    return 1 if [k for k in added + diff if k not in data_b] else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
