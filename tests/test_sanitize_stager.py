"""CPU: the stager (aeon_amd/csrc/stager.cpp) over a model device, under AddressSanitizer + UndefinedBehaviorSanitizer
and under ThreadSanitizer.  `make -C aeon_amd/csrc sanitize_stager tsan_stager` builds
tests/sanitize/stager_driver.cpp (a stand-alone program) with tests/sanitize/model_device.cpp, a HIP runtime whose
device memory is host memory and whose batch entries write a checksum of the bytes they read, so every output is
checked; each binary runs as a plain child process.  The scenarios: three flushed pageable windows (the third
reuses the first one's chunk and device outputs), six overlapped windows over two containers with eight staging
threads and a consumer's aeon_hip_stager_wait(NULL, buffer) (pageable and mapped buffers), a window dropped because
nobody waited for it, five zero-copy windows on one reused chunk, a two-chunk window (the (chunk << 48) | offset
rebasing) followed by a small one, a wait whose hipEventSynchronize fails (the `copying` count it left raised made
the window's last wait spin for ever), and a launch whose H2D fails.  The launch paths come from
aeon_hip_stager_last_launch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize")
SCENARIOS = ["pageable_flush", "overlap_wait_null[pageable]", "overlap_wait_null[mapped]", "dropped_window",
             "zero_copy_reuse", "two_chunks", "wait_sync_fails", "launch_copy_fails"]
# Seconds, ten times the whole run measured with the fixed stager (the margin is for a loaded machine):
# ASan + UBSan 0.6 s, ThreadSanitizer 1.7 s (most of it the two_chunks scenario's 70 MB window).  The driver arms
# alarm() with the same bound, so a scenario that spins ends by itself with a FAIL line.
LIMIT = {"sanitize_stager": 6, "tsan_stager": 17}
BINARY = {"sanitize_stager": "stager_driver_asan", "tsan_stager": "stager_driver_tsan"}


@pytest.fixture(scope="module", params=sorted(LIMIT))
def run(request):
    if not os.path.exists("/opt/rocm/llvm/bin/clang++"):
        pytest.skip("no clang with sanitizer runtimes")
    target = request.param
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), target])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87",
               TSAN_OPTIONS="halt_on_error=0:exitcode=88")
    limit = LIMIT[target]
    r = subprocess.run([os.path.join(BUILD, BINARY[target]), str(limit)], capture_output=True, text=True, env=env,
                       timeout=limit + 5)  # (the driver's own alarm fires first)
    return r, dict(line.split("\t", 1) for line in r.stdout.splitlines() if "\t" in line)


def test_every_scenario_ok(run):
    r, results = run
    assert list(results) == SCENARIOS, (r.stdout, r.stderr[-3000:])
    assert all(v == "ok" for v in results.values()), results
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])


def test_no_sanitizer_report(run):
    r, _ = run
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
