"""scripts/_ab.py, the comparison of two builds ("Parent against change"), driven on the host.  Every child is a fake -- the
function that starts one is injected, returns a scripted (status, stdout, stderr, seconds) and records its call -- except in the one test
of the real time limit at the end.  The verdict is checked against the runs printed in profiles/clip_stage_checks/ab.txt."""
import importlib.util
import json
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ab():
    before = set(sys.modules)
    spec = importlib.util.spec_from_file_location("_ab_under_test", os.path.join(ROOT, "scripts", "_ab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "torch" in before or "torch" not in sys.modules, "importing the harness imported torch"
    return mod


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    monkeypatch.delenv("R3D_LIB", raising=False)
    monkeypatch.delenv("PYTHONPATH", raising=False)


class Fake:
    """run(argv, cwd, env, limit) of scripted children: the n-th call returns the n-th of `script`, each (status, stdout, stderr)."""

    def __init__(self, script):
        self.script, self.calls = iter(script), []

    def __call__(self, argv, cwd, env, limit):
        self.calls.append({"argv": list(argv), "cwd": cwd, "PYTHONPATH": env.get("PYTHONPATH"), "R3D_LIB": env.get("R3D_LIB"), "limit": limit})
        status, out, err = next(self.script)
        return status, out, err, 1.5


def ok(value, key="value"):
    return (0, "warming up\n" + json.dumps({key: value}) + "\n", "")


PARENT, CHANGE = "parent=/trees/parent:/libs/parent.so", "change=/trees/change"
FIGURES = ["frames/s | higher | value | 600 | bench.py --gpus 1 --steps 20 --warmup 5", "ms per call | lower | value | 90 | scripts/prof_x.py --calls 3"]


def test_a_side_is_label_tree_and_an_optional_library(ab):
    assert ab.side(PARENT) == ("parent", "/trees/parent", "/libs/parent.so")
    assert ab.side(CHANGE) == ("change", "/trees/change", None)
    assert ab.side("/trees/other", "change") == ("change", "/trees/other", None)
    assert ab.side("rel/tree") == ("tree", os.path.abspath("rel/tree"), None)


def test_figures_run_in_turns_parent_first_one_figure_after_the_other(ab):
    fake = Fake([ok(100.0 + i) for i in range(12)])
    status, lines = ab.time_ab(ab.side(PARENT), ab.side(CHANGE), [ab.figure(f) for f in FIGURES], runs=3, run=fake)
    assert status == 0
    assert [c["cwd"] for c in fake.calls] == ["/trees/parent", "/trees/change"] * 6
    assert [c["PYTHONPATH"] for c in fake.calls] == ["/trees/parent", "/trees/change"] * 6
    assert [c["R3D_LIB"] for c in fake.calls] == ["/libs/parent.so", None] * 6          # only where the side names one
    assert [c["limit"] for c in fake.calls] == [600] * 6 + [90] * 6
    assert [c["argv"] for c in fake.calls[:6]] == [[sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]] * 6
    assert [c["argv"] for c in fake.calls[6:]] == [[sys.executable, "scripts/prof_x.py", "--calls", "3"]] * 6
    assert [l for l in lines if l.startswith("parent ")][0].startswith("parent  100  102  104 ")          # the parent's runs are calls 0, 2, 4
    assert [l for l in lines if l.startswith("change ")][1].startswith("change  107  109  111 ")


def test_the_environment_is_passed_on_and_the_tree_leads_pythonpath(ab, monkeypatch):
    monkeypatch.setenv("PYTHONPATH", "/elsewhere")
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")
    seen = {}

    def run(argv, cwd, env, limit):
        seen.update(env)
        return 0, "", "", 0.1
    ab.start(ab.side(CHANGE), ["true"], 5, run)
    assert seen["PYTHONPATH"] == "/trees/change" + os.pathsep + "/elsewhere" and seen["GPU_MAX_HW_QUEUES"] == "4"
    assert {k: v for k, v in seen.items() if k != "PYTHONPATH"} == {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}


@pytest.mark.parametrize("status, stderr, outcome", [(124, "", "time limit"), (137, "", "time limit"), (134, "", "abort"), (-6, "", "abort"),
                                                      (139, "", "segmentation fault"), (-11, "", "segmentation fault"),
                                                      (0, "HIP error: an illegal memory access was encountered\n", "gpu fault"), (1, "Traceback\n", "failed")])
def test_the_first_outcome_that_is_not_ok_stops_the_run(ab, status, stderr, outcome):
    bad = (status, json.dumps({"value": 3.0}) + "\n", stderr + "".join("err %03d\n" % i for i in range(100)))
    fake = Fake([ok(1.0), ok(2.0), bad] + [ok(9.0)] * 9)
    rc, lines = ab.time_ab(ab.side(PARENT), ab.side(CHANGE), [ab.figure(f) for f in FIGURES], runs=3, run=fake)
    assert rc == 2 and len(fake.calls) == 3                                     # no fourth child
    text = "\n".join(lines)
    assert "STOPPED: %s (exit status %d " % (outcome, status) in text
    assert "command: timeout -k 10 600 %s bench.py --gpus 1 --steps 20 --warmup 5" % sys.executable in text and "cwd /trees/parent, R3D_LIB=/libs/parent.so" in text
    assert "err 059" not in text and "err 060" in text and "err 099" in text          # the last 40 lines of its stderr
    assert not [l for l in lines if l.startswith("verdict")]


def test_outputs_does_not_start_the_second_child_after_the_first_failed(ab):
    fake = Fake([(139, "", "Segmentation fault\n"), (0, "", "")])
    rc, lines = ab.outputs_ab(ab.side(PARENT), ab.side(CHANGE), limit=77, run=fake)
    assert rc == 2 and len(fake.calls) == 1 and fake.calls[0]["limit"] == 77
    assert fake.calls[0]["argv"][:2] == [sys.executable, os.path.join(ROOT, "scripts", "ab_outputs.py")]          # the harness's own, in the side's tree
    assert (fake.calls[0]["cwd"], fake.calls[0]["PYTHONPATH"]) == ("/trees/parent", "/trees/parent")
    assert "STOPPED: segmentation fault" in "\n".join(lines) and "AGREE" not in "\n".join(lines)


# profiles/clip_stage_checks/ab.txt: the runs, and what the record says of them
RECORD = [((1702.43, 1641.78, 1679.39), (1689.35, 1678.01, 1652.79), True, 1679.39, 1678.01, 60.65, "spread", "-0.08"),
          ((0.1748, 0.1739, 0.1733), (0.1752, 0.1755, 0.1733), False, 0.1739, 0.1752, 0.0015, "1 %", "+0.75")]


@pytest.mark.parametrize("parent, change, higher, pm, cm, spread, bound_is, pct", RECORD)
def test_verdict_reproduces_the_record(ab, parent, change, higher, pm, cm, spread, bound_is, pct):
    v = ab.verdict(list(parent), list(change), higher)
    assert (v["parent_median"], v["change_median"]) == (pm, cm)
    assert v["spread"] == pytest.approx(spread, abs=1e-9) and v["bound_is"] == bound_is and v["within"] is True
    assert "%+.2f" % v["change_pct"] == pct
    assert v["bound"] == pytest.approx(spread if bound_is == "spread" else 0.01 * pm, abs=1e-9)


def test_the_report_block_is_the_one_on_record(ab):
    parent, change = RECORD[1][0], RECORD[1][1]
    fig = ab.figure("ms per call, host clock | lower | hip.source_conditions.ms | 600 | scripts/prof_source_conditions.py")
    block = ab.figure_block(fig, list(parent), list(change), ([1.0] * 3, [2.0] * 3), ab.verdict(parent, change, False))
    assert block[:4] == ['## scripts/prof_source_conditions.py: "hip.source_conditions.ms", ms per call, host clock (lower is better)',
                         "parent  0.1748  0.1739  0.1733     median 0.1739   spread 0.0015 (0.86 %: the 1 % bound applies, 0.0017)",
                         "change  0.1752  0.1755  0.1733     median 0.1752   = parent median +0.75 %",
                         "verdict: within the bound"]
    parent, change = RECORD[0][0], RECORD[0][1]
    block = ab.figure_block(ab.figure(FIGURES[0]), list(parent), list(change), ([1.0] * 3, [2.0] * 3), ab.verdict(parent, change, True))
    assert block[1] == "parent  1702.43  1641.78  1679.39     median 1679.39   spread 60.65 (3.61 %: the spread is the bound)"
    assert block[2] == "change  1689.35  1678.01  1652.79     median 1678.01   = parent median -0.08 %"


def test_verdict_outside_the_bound_in_each_direction_and_equal_medians_within(ab):
    # higher is better: bound = max(spread 2, 1 % = 1) = 2; 97.9 is worse by 2.1, 98.0 by exactly the bound
    assert ab.verdict([100, 99, 101], [97.9, 97.9, 97.9], True)["within"] is False
    assert ab.verdict([100, 99, 101], [98.0, 98.0, 98.0], True)["within"] is True
    assert ab.verdict([100, 99, 101], [150, 150, 150], True)["within"] is True          # better is never outside
    # lower is better: spread 0.2 < 1 % = 1.0, so the 1 % bound applies
    v = ab.verdict([100.0, 99.9, 100.1], [101.1, 101.1, 101.1], False)
    assert v["within"] is False and v["bound_is"] == "1 %" and v["bound"] == pytest.approx(1.0)
    assert ab.verdict([100.0, 99.9, 100.1], [50, 50, 50], False)["within"] is True
    assert ab.verdict([5.0, 5.0, 5.0], [4.0, 5.0, 6.0], True)["within"] is True           # equal medians
    assert ab.verdict([5.0, 5.0, 5.0], [4.0, 5.0, 6.0], False)["within"] is True
    rc, lines = ab.time_ab(ab.side(PARENT), ab.side(CHANGE), [ab.figure(FIGURES[0])], runs=3,
                           run=Fake([ok(100), ok(97.9), ok(99), ok(97.9), ok(101), ok(97.9)]))
    assert rc == 1 and "verdict: OUTSIDE the bound" in lines


def test_key_path(ab):
    doc = {"value": 7, "hip": {"a": {"ms": 0.25}}, "repeats": {"fps": [10.0, 20.5, 30.0]}, "none": None, "flag": True, "text": "x"}
    out = "lib /x.so\n" + json.dumps({"value": 1}) + "\n" + json.dumps(doc) + "\nnot json {\n\n"
    assert ab.key_path(out, "value") == 7                                         # the LAST JSON line, non-JSON lines after it skipped
    assert ab.key_path(out, "hip.a.ms") == 0.25 and ab.key_path(out, "repeats.fps.1") == 20.5
    for missing in ("hip.b.ms", "repeats.fps.3", "repeats.fps.x", "value.more", "none", "flag", "text"):
        with pytest.raises(ValueError):
            ab.key_path(out, missing)
    with pytest.raises(ValueError):
        ab.key_path("no json here\n", "value")


def test_a_missing_value_counts_as_a_failed_child(ab):
    fake = Fake([ok(1.0), ok(1.0, key="other")] + [ok(1.0)] * 4)
    rc, lines = ab.time_ab(ab.side(PARENT), ab.side(CHANGE), [ab.figure(FIGURES[0])], runs=3, run=fake)
    assert rc == 2 and len(fake.calls) == 2
    assert "STOPPED: failed (exit status 0 " in "\n".join(lines) and "no key 'value'" in "\n".join(lines)


def test_plan_file_and_figure_syntax(ab, tmp_path):
    p = tmp_path / "plan"
    p.write_text("# two figures\n%s   # the flagship\n\n%s\n" % tuple(FIGURES))
    assert ab.plan(str(p)) == [ab.figure(f) for f in FIGURES]
    assert ab.figure(FIGURES[1]) == ("ms per call", False, "value", 90, "scripts/prof_x.py --calls 3")
    for bad in ("a | faster | k | 5 | cmd", "a | higher | k | 5", "a | higher | k | 5 | "):
        with pytest.raises(ValueError):
            ab.figure(bad)


def compare(ab, tmp_path, a, b):
    np.savez(tmp_path / "a.npz", **a); np.savez(tmp_path / "b.npz", **b)
    ok_, lines = ab.compare_outputs(str(tmp_path / "a.npz"), str(tmp_path / "b.npz"))
    assert lines[-1] == ("AGREE" if ok_ else "DISAGREE")
    return ok_, lines


def test_compare_outputs(ab, tmp_path):
    frame = (np.arange(4000) % 251).astype(np.uint8).reshape(40, 100)
    render = np.linspace(0.0, 1.0, 600, dtype=np.float32).reshape(20, 30)
    torso = np.linspace(-2.0, 2.0, 600, dtype=np.float32)
    base = {"head_frame_f16mx": frame, "render_R128_48+48_rgb": render, "torso_frame_f16mx": torso}

    def changed(key, index, delta):
        d = {k: v.copy() for k, v in base.items()}
        d[key].flat[index] += delta                  # (a NaN delta makes the element NaN)
        return d
    agree, lines = compare(ab, tmp_path, base, base)
    assert agree and len(lines) == 4 and all("bit-identical" in l for l in lines[:3])
    assert compare(ab, tmp_path, base, changed("head_frame_f16mx", 7, 1))[0]               # one byte of 4 000 off by one count
    assert not compare(ab, tmp_path, base, changed("head_frame_f16mx", 7, 2))[0]
    many = {k: v.copy() for k, v in base.items()}; many["head_frame_f16mx"][0, :8] += 1    # 8 of 4 000 bytes = 2e-3: not fewer than 2e-3
    assert not compare(ab, tmp_path, base, many)[0]
    assert compare(ab, tmp_path, base, changed("render_R128_48+48_rgb", 300, np.float32(9e-6)))[0]
    assert not compare(ab, tmp_path, base, changed("render_R128_48+48_rgb", 300, np.float32(2e-5)))[0]
    assert compare(ab, tmp_path, base, changed("torso_frame_f16mx", 300, np.float32(5e-4)))[0]      # 3e-4 of the largest value, 2.0, is 6e-4
    assert not compare(ab, tmp_path, base, changed("torso_frame_f16mx", 300, np.float32(7e-4)))[0]
    assert not compare(ab, tmp_path, base, changed("render_R128_48+48_rgb", 300, float("nan")))[0]  # a NaN on one side only
    assert not compare(ab, tmp_path, changed("torso_frame_f16mx", 5, float("nan")), base)[0]
    less = {k: v for k, v in base.items() if k != "torso_frame_f16mx"}
    for a, b in ((base, less), (less, base)):
        agree, lines = compare(ab, tmp_path, a, b)
        assert not agree and any("torso_frame_f16mx" in l and "missing on one side" in l for l in lines)
    assert not compare(ab, tmp_path, {}, {})[0]                                            # two empty files


LISTING = """\t.text
\t.globl\tkernel_a
\t.type\tkernel_a,@function
kernel_a:                               ; @kernel_a
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
.LBB0_1:
\tv_add_f32_e32 v0, v0, v1
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
.Lfunc_end0:
\t.size\tkernel_a, .Lfunc_end0-kernel_a
\t.type\t__hip_cuid_1111,@object
__hip_cuid_1111:
\t.byte\t0
\t.size\t__hip_cuid_1111, 1
"""


def test_text_on_hand_written_listings(ab, tmp_path):
    def trees(text_a, text_b, extra_b=None):
        a, b = tmp_path / "a", tmp_path / "b"
        for d in (a, b):
            shutil.rmtree(d, ignore_errors=True); d.mkdir()
        (a / "unit.s").write_text(text_a); (b / "unit.s").write_text(text_b)
        if extra_b:
            (b / extra_b).write_text(text_b)
        return ab.diff_listings(str(a), str(b), "parent", "change")
    status, lines, totals = trees(LISTING, LISTING.replace(".LBB0_1", ".LBB7_3").replace("__hip_cuid_1111", "__hip_cuid_2222"))
    assert status == 0 and totals == (0, 0, 0)                                   # a renamed local label, another __hip_cuid_* data symbol
    assert lines[0] == "parent/unit.s -> change/unit.s" and "  exit status 0" in lines and "    __hip_cuid_2222  [data]" in lines
    status, lines, totals = trees(LISTING, LISTING.replace("v_add_f32_e32 v0, v0, v1", "v_add_f32_e32 v0, v1, v1"))
    assert status == 1 and totals == (1, 0, 0) and "  exit status 1" in lines   # a changed instruction
    status, lines, totals = trees(LISTING, LISTING.replace("kernel_a", "kernel_b"))
    assert status == 1 and totals == (0, 1, 1)
    status, lines, totals = trees(LISTING, LISTING, extra_b="other.s")
    assert status == 1 and totals == (0, 0, 0) and "only in change: other.s" in lines[0]          # differing unit sets


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_text_through_the_compile_step_on_one_small_unit(ab):
    tree = ab.side(ROOT, "tree")
    status, lines = ab.text_ab(tree._replace(label="parent"), tree._replace(label="change"), jobs=2, units=["r3d_comm.hip"])
    text = "\n".join(lines)
    assert status == 0, text
    assert "Result: 0 functions different, 0 added, 0 removed over all units." in text
    assert "parent/r3d_comm.s -> change/r3d_comm.s" in lines and "--cuda-device-only -S UNIT.hip" in text
    status, lines = ab.text_ab(tree, tree, units=["no_such_unit.hip"])
    assert status == 2 and "no compile line for no_such_unit.hip" in lines[0]


def test_the_real_child_function_ends_a_child_at_its_limit(ab):
    status, out, err, wall = ab.run_child([sys.executable, "-c", "import time; time.sleep(5)"], None, dict(os.environ), 1)
    assert ab.classify(status, out + err) == "time limit" and status == 124 and wall < 4
