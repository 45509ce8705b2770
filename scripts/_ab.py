"""Two builds against each other, once ("Parent against change"): the device text of two trees function by function, the arrays
two builds compute, and figures timed in turns with one bound.  `scripts/ab.py` is the command line.  Plain functions; this module imports
without torch, numpy or the package, and the process that runs it never opens the GPU: whatever does runs in a child.

A side is LABEL=TREE[:LIB].  TREE holds the package and scripts/ (the working tree, or a `git archive` export of a commit); a child of the
side runs with cwd=TREE and TREE in front of PYTHONPATH, and with R3D_LIB=LIB where the side names one.  Nothing else of the environment is
set or unset.  Every child goes through start(): `timeout -k 10 LIMIT argv...`, one at a time, output captured, wall time recorded, the
outcome classified.  The first outcome that is not "ok" raises Stopped: no further child is started, nothing is retried, and the command
line writes the report it has, with the child that stopped it, and exits with status 2."""
import collections
import concurrent.futures
import contextlib
import glob
import io
import json
import math
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_text_diff  # noqa: E402  (beside this file)

Side = collections.namedtuple("Side", "label tree lib")
Child = collections.namedtuple("Child", "argv cwd lib limit status outcome stdout stderr wall_s")
Figure = collections.namedtuple("Figure", "name higher key limit command")
OUTCOMES = {124: "time limit", 137: "time limit", 134: "abort", -6: "abort", 139: "segmentation fault", -11: "segmentation fault"}


class Stopped(Exception):
    """A child ended in an outcome other than "ok"; args[0] is that Child."""


def side(text, label=None):
    """'LABEL=TREE[:LIB]' -> Side with absolute paths (the label may be left out where `label` gives one)."""
    head, eq, rest = text.partition("=")
    label, rest = (head, rest) if eq else (label or os.path.basename(os.path.abspath(text)), text)
    tree, _, lib = rest.partition(":")
    return Side(label, os.path.abspath(tree), os.path.abspath(lib) if lib else None)


def classify(status, text):
    """The outcome of a child from its exit status and its whole output.  A GPU fault counts whatever the status: HIP reports it and the
    program may go on."""
    if "illegal memory access" in text:
        return "gpu fault"
    return OUTCOMES.get(status, "failed" if status else "ok")


def run_child(argv, cwd, env, limit):
    """argv under `timeout -k 10 limit` -> (exit status, stdout, stderr, wall seconds)."""
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + list(argv), cwd=cwd, env=env, capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr, time.perf_counter() - t0


def start(s, argv, limit, run=run_child, value=None):
    """The one way a child is started: argv in the side's tree, under its own time limit.  `value`, where given, is value(stdout) -> what the
    caller wants from an "ok" child; a ValueError from it makes the child "failed".  Returns (Child, value); raises Stopped."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([s.tree] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
    if s.lib:
        env["R3D_LIB"] = s.lib
    status, out, err, wall = run(argv, s.tree, env, limit)
    child, got = Child(list(argv), s.tree, s.lib, limit, status, classify(status, out + err), out, err, wall), None
    if child.outcome == "ok" and value is not None:
        try:
            got = value(out)
        except ValueError as e:
            child = child._replace(outcome="failed", stderr=err + "\n%s\n" % e)
    print("ab: %s: %s: %s, %.1f s" % (s.label, " ".join(argv), child.outcome, wall), file=sys.stderr, flush=True)      # progress; the report is stdout
    if child.outcome != "ok":
        raise Stopped(child)
    return child, got


def stop_report(child):
    """The lines that name the child a run stopped at."""
    return ["STOPPED: %s (exit status %d after %.1f s); no further child was started, nothing was retried" % (child.outcome, child.status, child.wall_s),
            "  command: timeout -k 10 %d %s   (cwd %s%s)" % (child.limit, " ".join(shlex.quote(a) for a in child.argv), child.cwd, ", R3D_LIB=" + child.lib if child.lib else ""),
            "  the last 40 lines of its stderr:"] + ["    " + l for l in child.stderr.splitlines()[-40:]]


# ---- time: figures in turns, one bound

def figure(spec):
    """'NAME | higher|lower | KEY.PATH | LIMIT_S | command ...' -> Figure."""
    parts = [p.strip() for p in spec.split("|", 4)]
    if len(parts) != 5 or parts[1] not in ("higher", "lower") or not parts[4]:
        raise ValueError("a figure is 'NAME | higher|lower | KEY.PATH | LIMIT_S | command ...', got %r" % spec)
    return Figure(parts[0], parts[1] == "higher", parts[2], int(parts[3]), parts[4])


def plan(path):
    """The figures of a plan file: one spec per line, # starts a comment."""
    with open(path) as f:
        return [figure(l) for l in (l.split("#")[0].strip() for l in f) if l]


def key_path(stdout, path):
    """The number at the dotted `path` (list indices as integers) in the last line of stdout that parses as JSON; ValueError where there is
    no such line, no such key or no finite number there."""
    for line in reversed(stdout.splitlines()):
        try:
            node = json.loads(line)
        except ValueError:
            continue
        try:
            for k in path.split("."):
                node = node[int(k) if isinstance(node, list) else k]
        except (KeyError, IndexError, ValueError, TypeError):
            raise ValueError("no key %r in the last JSON line of stdout" % path)
        if isinstance(node, bool) or not isinstance(node, (int, float)) or not math.isfinite(node):
            raise ValueError("%r is %r, not a number" % (path, node))
        return node
    raise ValueError("no JSON line on stdout")


def verdict(parent_values, change_values, higher_is_better):
    """The rule, once: the medians of both sides; the parent's spread (max - min of its runs); the bound, the larger of that spread and 1 %
    of the parent's median; within the bound when the change's median is not worse than the parent's by more than the bound."""
    pm, cm = statistics.median(parent_values), statistics.median(change_values)
    spread, one = max(parent_values) - min(parent_values), 0.01 * abs(pm)
    bound = max(spread, one)
    return {"parent_median": pm, "change_median": cm, "spread": spread, "spread_pct": 100.0 * spread / abs(pm) if pm else math.inf,
            "bound": bound, "bound_is": "spread" if spread >= one else "1 %", "change_pct": 100.0 * (cm - pm) / abs(pm) if pm else math.inf,
            "within": ((pm - cm) if higher_is_better else (cm - pm)) <= bound}


def figure_block(fig, pv, cv, walls, v):
    """The report block of one figure, as the ab.txt files on record have it; numbers with the decimal places the runs came with (6 at most)."""
    places = max(len(("%.6f" % x).partition(".")[2].rstrip("0")) for x in pv + cv)
    n = lambda x: "%.*f" % (places, x)
    bound = "the spread is the bound" if v["bound_is"] == "spread" else "the 1 %% bound applies, %s" % n(v["bound"])
    return ["## %s: \"%s\", %s (%s is better)" % (fig.command, fig.key, fig.name, "higher" if fig.higher else "lower"),
            "parent  %s     median %s   spread %s (%.2f %%: %s)" % ("  ".join(map(n, pv)), n(v["parent_median"]), n(v["spread"]), v["spread_pct"], bound),
            "change  %s     median %s   = parent median %+.2f %%" % ("  ".join(map(n, cv)), n(v["change_median"]), v["change_pct"]),
            "verdict: %s" % ("within the bound" if v["within"] else "OUTSIDE the bound"),
            "wall time per child, s (limit %d): parent %s   change %s" % (fig.limit, "  ".join("%.1f" % w for w in walls[0]), "  ".join("%.1f" % w for w in walls[1])), ""]


def time_ab(parent, change, figures, runs=3, run=run_child):
    """Each figure: parent and change in turns, parent first, `runs` times each; one figure finished before the next begins.  A command
    that begins with a *.py runs under this interpreter.  -> (exit status, report lines): 0 all within the bound, 1 any outside, 2 stopped."""
    lines, status = [], 0
    try:
        for fig in figures:
            argv, values, walls = shlex.split(fig.command), ([], []), ([], [])
            argv = ([sys.executable] if argv[0].endswith(".py") else []) + argv
            for _ in range(runs):
                for i, s in enumerate((parent, change)):
                    child, x = start(s, argv, fig.limit, run, lambda out: key_path(out, fig.key))
                    values[i].append(x); walls[i].append(child.wall_s)
            v = verdict(values[0], values[1], fig.higher)
            lines += figure_block(fig, values[0], values[1], walls, v)
            status = max(status, 0 if v["within"] else 1)
    except Stopped as e:
        return 2, lines + stop_report(e.args[0])
    return status, lines


# ---- outputs: the arrays two builds compute

def compare_outputs(path_a, path_b):
    """Two files of scripts/ab_outputs.py, array by array -> (agree, report lines).  Two compilations may contract different mul + add
    pairs into fmas (fp-contract=fast around the SLP vectoriser), so arrays that are not bit-identical are held to a tight tolerance, not a
    digest: fp32 ray-kernel outputs within 1e-5, uint8 frames within one count in < 0.2 % of the bytes, the torso frame's fp32 image within
    3e-4 of its maximum -- a wrong operand in a quarter of the lanes (the packed-f32 op_sel erratum, DESIGN 4.1a, which these tolerances were
    set for) is off by the operand's magnitude."""
    import numpy as np
    a_all, b_all = dict(np.load(path_a)), dict(np.load(path_b))
    ok, lines = len(a_all) > 0 and set(a_all) == set(b_all), []
    for k in sorted(set(a_all) | set(b_all)):
        a, b = a_all.get(k), b_all.get(k)
        if a is None or b is None or a.shape != b.shape or a.dtype != b.dtype:
            ok = False
            lines.append("compare %-28s %s  BAD" % (k, "missing on one side" if a is None or b is None else "shape or dtype differs"))
            continue
        if a.tobytes() == b.tobytes():
            lines.append("compare %-28s %s %s: bit-identical" % (k, a.dtype, a.shape))
            continue
        if a.dtype == np.uint8:
            d = np.abs(a.astype(np.int32) - b.astype(np.int32)); frac = float((d > 0).mean())
            good = int(d.max()) <= 1 and frac < 2e-3
            lines.append("compare %-28s uint8: %d of %d bytes differ (%.2e), max %d  %s" % (k, int((d > 0).sum()), d.size, frac, int(d.max()), "ok" if good else "BAD"))
        else:
            fin = np.isfinite(a) & np.isfinite(b)
            e, top = (float(np.abs(a[fin] - b[fin]).max()), float(np.abs(a[fin]).max())) if fin.any() else (0.0, 0.0)
            # ray-kernel outputs: fp32 arithmetic, 1e-5 absolute; the torso frame's fp32 image went through nine f16mx convolutions whose fp8 roundings
            # flip with the last bit of their input: twice the tier's own error, 3e-4 of the largest value
            tol = 1e-5 if k.startswith("render_") else 3e-4 * top
            good = e <= tol and bool((np.isfinite(a) == np.isfinite(b)).all())
            lines.append("compare %-28s fp32 max |diff| %.2e (max |value| %.3g)  %s" % (k, e, top, "ok" if good else "BAD"))
        ok = ok and good
    return ok, lines + ["AGREE" if ok else "DISAGREE"]


def outputs_ab(a, b, limit=600, run=run_child):
    """scripts/ab_outputs.py -- the one beside this file, so that a side which is an older commit needs none of its own; the package and
    bench.py it imports are the side's, through PYTHONPATH -- as a child of each side, then the two files compared
    -> (exit status, report lines): 0 agree, 1 disagree, 2 stopped."""
    lines, script = [], os.path.join(os.path.dirname(os.path.abspath(__file__)), "ab_outputs.py")
    with tempfile.TemporaryDirectory() as tmp:
        files = [os.path.join(tmp, "%d.npz" % i) for i in range(2)]
        try:
            for s, f in zip((a, b), files):
                child, _ = start(s, [sys.executable, script, f], limit, run)
                lines += ["== %s: %s%s   (%.1f s, limit %d)" % (s.label, os.path.relpath(s.tree), ", R3D_LIB=" + os.path.relpath(s.lib) if s.lib else "", child.wall_s, limit)]
                lines += [l for l in child.stdout.splitlines() if l.startswith(("digest ", "time "))]
        except Stopped as e:
            return 2, lines + stop_report(e.args[0])
        ok, cmp_lines = compare_outputs(*files)
    return (0 if ok else 1), lines + ["== %s against %s" % (a.label, b.label)] + cmp_lines


# ---- text: the device assembly of two trees, unit by unit

def listings(tree, out_dir, jobs=4, make_args=(), units=None):
    """The device-assembly listing of every unit of the tree's csrc/Makefile (or of `units` among them) -> out_dir/<unit>.s, with the
    Makefile's own flags: the compile lines are the ones `make -n -B` prints and nothing here states a flag.  Returns those lines as make
    printed them; RuntimeError with the compiler's message where a unit does not compile."""
    csrc = os.path.join(tree, "real3dportrait_amd", "csrc")
    os.makedirs(out_dir, exist_ok=True)
    r = subprocess.run(["make", "-n", "-B", "-C", csrc, "OBJDIR=" + out_dir] + list(make_args), capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("make -n in %s failed:\n%s" % (csrc, r.stderr))
    printed, cmds = [], []
    for line in r.stdout.splitlines():
        argv = shlex.split(line) if "--cuda-device-only -S" in line else []
        unit = next((a for a in argv if a.endswith(".hip")), None)
        if unit and (not units or unit in units):
            argv[argv.index("-o") + 1] = os.path.join(out_dir, unit[:-4] + ".s")
            printed.append(line.strip()); cmds.append((unit, argv))
    if not cmds or (units and len(cmds) != len(set(units))):
        raise RuntimeError("%s: no compile line for %s" % (csrc, ", ".join(units) if units else "any unit"))
    with concurrent.futures.ThreadPoolExecutor(max(1, min(int(jobs), 16))) as pool:
        done = list(pool.map(lambda c: subprocess.run(c[1], cwd=csrc, capture_output=True, text=True), cmds))
    for (unit, _), d in zip(cmds, done):
        if d.returncode:
            raise RuntimeError("%s of %s does not compile:\n%s" % (unit, tree, d.stderr))
    return printed


def diff_listings(dir_a, dir_b, label_a, label_b):
    """Every <unit>.s of two directories through kernel_text_diff.main -> (exit status, report lines, (different, added, removed) functions
    over all units).  Status 1 when a unit's status is 1 or the two sets of units differ."""
    names = [sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "*.s"))) for d in (dir_a, dir_b)]
    status, lines, totals = 0, [], [0, 0, 0]
    if names[0] != names[1]:
        status = 1
        lines += ["the two trees do not have the same units: only in %s: %s; only in %s: %s" % (
            label_a, " ".join(sorted(set(names[0]) - set(names[1]))) or "-", label_b, " ".join(sorted(set(names[1]) - set(names[0]))) or "-"), ""]
    for name in sorted(set(names[0]) & set(names[1])):
        pa, pb = os.path.join(dir_a, name), os.path.join(dir_b, name)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            unit_status = kernel_text_diff.main(pa, pb)
        lines += out.getvalue().replace(pa, "%s/%s" % (label_a, name)).replace(pb, "%s/%s" % (label_b, name)).splitlines()
        lines += ["  exit status %d" % unit_status, ""]
        status = max(status, unit_status)
        (a, data_a), (b, data_b) = kernel_text_diff.split(pa), kernel_text_diff.split(pb)
        for i, n in enumerate(([k for k in b if k in a and a[k] != b[k] and k not in data_a | data_b], [k for k in set(b) - set(a) if k not in data_b],
                               [k for k in set(a) - set(b) if k not in data_a])):
            totals[i] += len(n)
    return status, lines, tuple(totals)


def text_ab(parent, change, jobs=4, make_args=(), units=None):
    """The device code of two trees, translation unit by translation unit -> (exit status, report lines): the established
    kernel_text_diff.txt.  A unit that does not compile is an error (status 2) with the compiler's message, not a difference."""
    with tempfile.TemporaryDirectory() as tmp:
        dirs = [os.path.join(tmp, "%d" % i) for i in range(2)]
        try:
            printed = [listings(s.tree, d, jobs, make_args, units) for s, d in zip((parent, change), dirs)]
        except RuntimeError as e:
            return 2, ["FAILED: %s" % e]
        status, lines, totals = diff_listings(dirs[0], dirs[1], parent.label, change.label)
    unit_of = lambda line: next(a for a in shlex.split(line) if a.endswith(".hip"))
    compile_lines = sorted({ls[0].split(" -o ")[0].replace(unit_of(ls[0]), "UNIT.hip") for ls in printed})          # two where the trees' flags differ
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(shlex.split(printed[1][0])[0])))
    head = ["Device code of %s (%s) against %s (%s), translation unit by translation unit (scripts/ab.py text -> scripts/kernel_text_diff.py), %d units of "
            "csrc/Makefile's SRCS." % (parent.label, os.path.relpath(parent.tree), change.label, os.path.relpath(change.tree), len(printed[0]))]
    head += ["Listings, the line of each tree's own `make -n -B`: " + l for l in compile_lines] + ["          both trees compiled on one machine; ROCm: %s" % rocm]
    head += ["A symbol is 'identical' when its instructions and operands are (comments, debug directives and local label names stripped).",
             "Result: %d functions different, %d added, %d removed over all units.  [data]: the per-unit __hip_cuid_* (a hash of the source and its path)." % totals, ""]
    return status, head + lines
