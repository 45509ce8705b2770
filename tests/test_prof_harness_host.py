"""scripts/_prof.py, the timing harness of the scripts/prof_<unit>.py files, driven on the host with a fake timer that
returns scripted numbers and records its calls: the order of the warm-up and of the alternating blocks, the per-route `calls`, warm-up
and block limit, the two summaries and the printed / written JSON.  No device and no torch timing: the harness imports torch inside
its three real timers only."""
import importlib.util
import json
import os
import statistics
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prof():
    before = set(sys.modules)
    spec = importlib.util.spec_from_file_location("_prof_under_test", os.path.join(ROOT, "scripts", "_prof.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "torch" in before or "torch" not in sys.modules, "importing the harness imported torch"
    return mod


class Log:
    """A fake timer per route: timer(fn, calls) appends (route, calls) to the shared log and returns the route's next scripted number."""

    def __init__(self):
        self.calls = []

    def timer(self, name, numbers):
        it = iter(numbers)

        def timer(fn, calls):
            assert fn() == name                     # the timer is handed its own route's function
            self.calls.append((name, calls))
            return next(it)
        return timer


def three_routes(prof, log):
    """a: 4 calls; b: 7 calls, its own warm-up of 1; c: 1 call, no warm-up, the first two blocks only.  The first scripted number of a
    and b is the warm-up's, which must not reach the samples."""
    return {"a": prof.route(lambda: "a", log.timer("a", [99.0, 1.0, 2.0, 3.0]), 4),
            "b": prof.route(lambda: "b", log.timer("b", [99.0, 10.0, 20.0, 30.0]), 7, warmup=1),
            "c": prof.route(lambda: "c", log.timer("c", [100.0, 200.0]), 1, warmup=0, blocks=2)}


def test_warm_up_comes_first_and_blocks_alternate_in_route_order(prof):
    log = Log()
    samples = prof.alternate(three_routes(prof, log), blocks=3, warmup=2)
    assert log.calls == [("a", 2), ("b", 1),                             # every warmed route before any sample; c is not warmed
                         ("a", 4), ("b", 7), ("c", 1),                   # block 0, in the order of the dict, each with its own calls
                         ("a", 4), ("b", 7), ("c", 1),                   # block 1
                         ("a", 4), ("b", 7)]                             # block 2: c was limited to two blocks
    assert samples == {"a": [1.0, 2.0, 3.0], "b": [10.0, 20.0, 30.0], "c": [100.0, 200.0]}
    assert list(samples) == ["a", "b", "c"]


def test_a_route_marked_no_warm_up_is_not_warmed(prof):
    log = Log()
    prof.alternate({"c": prof.route(lambda: "c", log.timer("c", [5.0]), 3, warmup=0)}, blocks=1, warmup=2)
    assert log.calls == [("c", 3)]
    log = Log()
    prof.alternate({"c": prof.route(lambda: "c", log.timer("c", [5.0]), 3)}, blocks=1, warmup=0)
    assert log.calls == [("c", 3)]


def test_a_route_limited_to_k_blocks_gets_k_samples(prof):
    for k in (0, 1, 4, 9):
        log = Log()
        r = {"full": prof.route(lambda: "full", log.timer("full", [0.0] + list(range(6))), 2),
             "few": prof.route(lambda: "few", log.timer("few", [0.0] + list(range(6))), 2, blocks=k)}
        samples = prof.alternate(r, blocks=6, warmup=1)
        assert len(samples["full"]) == 6 and len(samples["few"]) == min(k, 6)


def test_routes_gives_every_function_the_same_timer_and_calls(prof):
    log = Log()
    timer = lambda fn, calls: log.calls.append((fn(), calls)) or 1.5
    samples = prof.alternate(prof.routes({"x": lambda: "x", "y": lambda: "y"}, timer, 11), blocks=2, warmup=3)
    assert log.calls == [("x", 3), ("y", 3), ("x", 11), ("y", 11), ("x", 11), ("y", 11)]
    assert samples == {"x": [1.5, 1.5], "y": [1.5, 1.5]}


EVEN = [0.12344, 0.12356, 0.5, 0.1]          # four samples: the median is the mean of the two middle ones, 0.1235
ODD = [2.00004, 1.99996, 2.5]


def test_ms_spread_is_what_the_scripts_computed(prof):
    for v in (EVEN, ODD):
        want = {"ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
        assert prof.ms_spread(v) == want
        assert prof.ms_spread(v, keep_blocks=True) == dict(want, block_medians_ms=[round(x, 4) for x in v])
    assert prof.ms_spread(EVEN, keep_blocks=True) == {"ms": 0.1235, "spread_ms": 0.4, "block_medians_ms": [0.1234, 0.1236, 0.5, 0.1]}
    assert prof.ms_spread(ODD) == {"ms": 2.0, "spread_ms": 0.5}
    assert "block_medians_ms" not in prof.ms_spread(ODD)


def test_median_min_max_is_unrounded(prof):
    assert prof.median_min_max(EVEN) == {"median": (0.12344 + 0.12356) / 2, "min": 0.1, "max": 0.5}
    assert prof.median_min_max(ODD) == {"median": 2.00004, "min": 1.99996, "max": 2.5}


RESULT = {"metric": "m", "hip": {"a": {"ms": 0.1235, "spread_ms": 0.4}}, "equal": True, "counts": [1, 2, 3], "none": None}


def test_emit_prints_one_json_line_equal_to_the_file_it_writes(prof, tmp_path, capsys):
    out_dir = tmp_path / "new" / "dir"                    # made where missing
    prof.emit(RESULT, str(out_dir), "prof_unit")
    printed = capsys.readouterr().out
    assert printed.endswith("\n") and printed.count("\n") == 1
    assert [p.name for p in out_dir.iterdir()] == ["prof_unit.json"]
    text = (out_dir / "prof_unit.json").read_text()
    assert json.loads(printed) == json.loads(text) == RESULT
    assert text == json.dumps(RESULT, indent=1) + "\n"


def test_emit_without_out_dir_writes_nothing(prof, tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    prof.emit(RESULT, None, "prof_unit")
    assert json.loads(capsys.readouterr().out) == RESULT
    assert list(tmp_path.iterdir()) == []


def test_parser_has_the_shared_arguments_with_the_script_s_default(prof):
    ap = prof.parser("doc", calls=37)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args([])
    assert (a.calls, a.blocks, a.out, a.size) == (37, 5, None, 512)
    a = ap.parse_args(["--calls", "3", "--blocks", "2", "--out", "d"])
    assert (a.calls, a.blocks, a.out) == (3, 2, "d")
