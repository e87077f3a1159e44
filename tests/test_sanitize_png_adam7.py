"""CPU: tests/sanitize/png_adam7_main.cpp, a program of its own under ASan + UBSan: the opt-in interlaced PNG
path's host half and its kernels' code over the interlaced fixtures, their truncations and single-byte mutations."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = np.load(os.path.join(ROOT, "tests", "golden", "png_fixtures.npz"))


def test_sanitizer_program(tmp_path):
    exe = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize", "png_adam7_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize_png_adam7"])
    paths = []
    for key in sorted(k for k in FX.files if k.endswith("_i.png")):
        (tmp_path / key).write_bytes(FX[key].tobytes())
        paths.append(str(tmp_path / key))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    r = subprocess.run([exe] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    files, runs, decoded, refused = [int(x) for x in re.findall(r"\d+", r.stdout.splitlines()[-1])]
    assert files == len(paths) == 15 and decoded > 3 * files and refused > decoded
