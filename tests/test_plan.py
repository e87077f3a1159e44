"""CPU: the image planner (aeon_amd/csrc/plan.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer.
`make -C aeon_amd/csrc sanitize_plan` builds tests/sanitize/callplan_driver.cpp, a stand-alone program over
plan.cpp: it plans each of its cases with fixed fake addresses, writes the call's job table into a zeroed
buffer and prints the table's hash, the sizes the device half allocates by and every launch's shape; a
layout rule of its own per case (sections and scratch regions in bounds, aligned, disjoint; scratch read
only after an earlier launch wrote it; taps inside the tap region; stats slots distinct; tiles covering
their windows); and every refusal's code and text.  tests/golden/plan_tables.json holds those lines as the
planner printed them when its code had been moved out of stage.cpp's run_batch verbatim, before it was
restructured: the tables must not change."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize", "callplan_driver")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_tables.json")


@pytest.fixture(scope="module")
def run():
    if not os.path.exists("/opt/rocm/llvm/bin/clang++"):
        pytest.skip("no clang with sanitizer runtimes")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize_plan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    return subprocess.run([DRIVER], capture_output=True, text=True, env=env, timeout=300)


def test_runs_clean(run):
    assert run.returncode == 0, run.stderr[-3000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


def test_layout_rule_holds_for_every_case(run):
    lines = run.stdout.splitlines()
    cases = [l.split()[1] for l in lines if l.startswith("case ")]
    rules = {l.split()[1]: l.split(" ", 2)[2] for l in lines if l.startswith("rule ")}
    assert len(cases) >= 17 and set(rules) == set(cases)
    for name in cases:
        assert rules[name] == "ok", (name, rules[name])


def test_every_refusal_refuses(run):
    refusals = [l for l in run.stdout.splitlines() if l.startswith("refuse ")]
    assert len(refusals) >= 24
    for l in refusals:
        assert " code=-1 text=" in l or " code=-3 text=" in l, l


def test_tables_equal_the_recorded_ones(run):
    golden = json.load(open(GOLDEN))["lines"]
    lines = run.stdout.splitlines()
    assert len(lines) == len(golden)
    for got, want in zip(lines, golden):
        assert got == want
