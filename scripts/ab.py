#!/usr/bin/env python3
"""Two builds against each other (the method is scripts/_ab.py; DESIGN 5, "Parent against change").  This process never opens the GPU.

    ab.py text PARENT_TREE CHANGE_TREE [--jobs J] [--make-arg K=V ...] [--units UNIT.hip ...]
        the device assembly of every unit of csrc/Makefile's SRCS, function by function; CPU only.  Exit 1 when a function differs or was
        added, or the trees' units differ; 2 when a unit does not compile.  A tree may carry a label, LABEL=TREE (an export's commit, say).
    ab.py outputs A B [--limit S]
        scripts/ab_outputs.py in each side, the saved arrays compared.  Exit 0 AGREE, 1 DISAGREE, 2 stopped.
    ab.py time --parent SIDE --change SIDE [--runs 3] --figure SPEC ... [--plan FILE]
        each figure in turns, parent first.  Exit 0 all within the bound, 1 any outside, 2 stopped.

A side is LABEL=TREE[:LIB].  A figure is 'NAME | higher|lower | KEY.PATH | LIMIT_S | command ...', its value read from the last JSON line
the command prints; --plan FILE holds one figure per line, # comments.  --out FILE also writes the report to FILE."""
import argparse
import os
import sys

import _ab


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    t, o, m = sub.add_parser("text"), sub.add_parser("outputs"), sub.add_parser("time")
    t.add_argument("parent"); t.add_argument("change")
    t.add_argument("--jobs", type=int, default=4, help="compilations at a time (default 4, 16 at most)")
    t.add_argument("--make-arg", action="append", default=[], metavar="K=V", help="passed to each tree's make")
    t.add_argument("--units", nargs="+", default=None, metavar="UNIT.hip", help="these units only")
    o.add_argument("a"); o.add_argument("b")
    o.add_argument("--limit", type=int, default=600, help="seconds per child (default 600)")
    m.add_argument("--parent", required=True); m.add_argument("--change", required=True)
    m.add_argument("--runs", type=int, default=3)
    m.add_argument("--figure", action="append", default=[], metavar="SPEC"); m.add_argument("--plan", default=None, metavar="FILE")
    for p in (t, o, m):
        p.add_argument("--out", default=None, metavar="FILE")
    a = ap.parse_args(argv)
    if a.mode == "text":
        status, lines = _ab.text_ab(_ab.side(a.parent, "parent"), _ab.side(a.change, "change"), a.jobs, a.make_arg, a.units)
    elif a.mode == "outputs":
        status, lines = _ab.outputs_ab(_ab.side(a.a), _ab.side(a.b), a.limit)
    else:
        figures = [_ab.figure(s) for s in a.figure] + (_ab.plan(a.plan) if a.plan else [])
        if not figures:
            ap.error("time needs a --figure or a --plan")
        sides = _ab.side(a.parent, "parent"), _ab.side(a.change, "change")
        head = ["# %s: %s, %s" % (s.label, os.path.relpath(s.tree), "R3D_LIB=" + os.path.relpath(s.lib) if s.lib else "its own library") for s in sides]
        head += ["# parent and change in turns, parent first, %d runs each, one figure after the other; the bound is DESIGN 5's (\"Parent against change\")" % a.runs, ""]
        status, lines = _ab.time_ab(sides[0], sides[1], figures, a.runs)
        lines = head + lines
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
