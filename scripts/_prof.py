"""The measuring method of the scripts/prof_<unit>.py files, once: three timers, the alternating-blocks runner, the two
summaries on record, the printed JSON line and the shared command-line arguments.  Plain functions; torch is imported inside the timers,
so this module imports on a machine without a GPU, and a timer called there fails at its first device call: nothing falls back.

    import _prof                                            (scripts/ is sys.path[0] of a script run from it)
    a = _prof.parser(__doc__, calls=20).parse_args()
    samples = _prof.alternate({"hip": _prof.route(hip, _prof.block_median, a.calls), ...}, a.blocks, warmup=3)
    _prof.emit({k: _prof.ms_spread(v) for k, v in samples.items()}, a.out, "prof_<unit>")
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def paths(tests=False):
    """Put the repository root (and tests/, for the scripts that time a reference kept there) in front of sys.path."""
    for p in ([os.path.join(ROOT, "tests")] if tests else []) + [ROOT]:
        sys.path.insert(0, p)


def parser(doc, calls, blocks=5):
    """The arguments every timing script has, --calls with the script's own default; the script adds its own and parses."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=calls, help="calls per block (default %(default)s)")
    ap.add_argument("--blocks", type=int, default=blocks, help="alternating blocks per route (default %(default)s)")
    ap.add_argument("--out", default=None, metavar="DIR", help="also write the JSON, indented, to DIR/<name>.json")
    return ap


# ---- timers: timer(fn, calls) -> ms per call.  All three are the "step or call time" row of the table in measuring-on-mi355x, section 4.

def block_median(fn, calls):
    """Device events around EVERY call: calls + 1 events, the median of the calls' intervals (that row's "device events", per call:
    one slow call does not move the figure)."""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for i in range(calls):
        fn()
        ev[i + 1].record()
    ev[-1].synchronize()
    return statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(calls))


def by_events(fn, calls):
    """Two device events around `calls` back-to-back calls, divided by calls (that row's "device events", the mean of a block)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def by_host_clock(fn, calls):
    """The host clock around `calls` back-to-back calls between two synchronises, divided by calls (that row's "host clock around work
    that ends in a device synchronise"): holds the host's share of a call, its copies and its own synchronisations as well."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


# ---- the alternating-blocks rule

def route(fn, timer, calls, warmup=None, blocks=None):
    """One side of a comparison: fn timed by timer(fn, calls).  warmup / blocks, where given, replace the run's (warmup=0: not warmed;
    blocks=k: sampled in the first k blocks only, for a route too slow to repeat)."""
    return {"fn": fn, "timer": timer, "calls": calls, "warmup": warmup, "blocks": blocks}


def routes(fns, timer, calls):
    """{name: fn} -> {name: route}, all with one timer and one `calls`."""
    return {k: route(fn, timer, calls) for k, fn in fns.items()}


def alternate(routes, blocks, warmup):
    """{name: route} -> {name: [one sample per block]}.  Every route is warmed first (one discarded sample of `warmup` calls by its own
    timer, which ends in a synchronise); then, block by block, every route gives one sample in the order of the dict, so that a drift
    of the machine falls on all routes alike."""
    for r in routes.values():
        n = warmup if r["warmup"] is None else r["warmup"]
        if n:
            r["timer"](r["fn"], n)
    samples = {k: [] for k in routes}
    for b in range(blocks):
        for k, r in routes.items():
            if r["blocks"] is None or b < r["blocks"]:
                samples[k].append(r["timer"](r["fn"], r["calls"]))
    return samples


# ---- the two summaries on record

def ms_spread(v, keep_blocks=False):
    """{"ms": the median of the block samples, "spread_ms": max - min[, "block_medians_ms": the samples]}, rounded to 4 places."""
    out = {"ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
    if keep_blocks:
        out["block_medians_ms"] = [round(x, 4) for x in v]
    return out


def median_min_max(v):
    """{"median", "min", "max"} of the block samples, unrounded."""
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def emit(result, out_dir, name):
    """Print the result as one JSON line; with out_dir, also write it indented to out_dir/name.json."""
    print(json.dumps(result))
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
