"""CPU: the MJPEG AVI demux of the video provider (aeon_amd/csrc/avi_host.cpp) and the JPEG header parser it
hands the frames to, under AddressSanitizer + UndefinedBehaviorSanitizer.  `make -C aeon_amd/csrc
sanitize_video` builds tests/sanitize/avi_driver.cpp (a stand-alone program); it runs as a child process over
aeon's bb8.avi, the synthetic files of tests/video_cases.py and a seeded corpus written here: bb8 cut at every
97th byte of its first 6 KB, 200 single-byte flips inside its hdrl list and its idx1 chunk, index offsets
pointing at and past the end of movi, and chunk sizes of 0xFFFFFFFF.  The run must end clean, every file with
the status the independent restatement (tests/video_ref.py) expects, and the product library must report the
same statuses."""
import os
import struct
import subprocess

import numpy as np
import pytest

import aeon_amd as A
from tests import video_cases as V
from tests import video_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize", "avi_driver")


def _corpus():
    files = {"bb8.avi": V.bb8()}
    bb8 = files["bb8.avi"]
    for k, (enc, n) in enumerate(zip(V.ENCODINGS, (1, 3, 4, 7))):
        files[f"synthetic_{enc}.avi"] = V.synthetic_avi(k, n, 23, 17, enc, empty=(2,) if enc == "444" else ())
    for cut in range(0, 6 * 1024, 97):
        files[f"trunc_{cut:05d}.avi"] = bb8[:cut]
    hdrl = bb8.index(b"hdrl")
    (hdrl_size,) = struct.unpack_from("<I", bb8, hdrl - 4)
    idx1 = bb8.rindex(b"idx1")
    spans = [(hdrl - 8, hdrl + hdrl_size), (idx1, len(bb8))]
    rng = np.random.default_rng(20240519)
    for k in range(200):
        lo, hi = spans[k % 2]
        pos = int(rng.integers(lo, hi))
        b = bytearray(bb8)
        b[pos] ^= 1 << int(rng.integers(0, 8))
        files[f"flip_{k:03d}_{pos:05d}.avi"] = bytes(b)
    frames = [V.encode(V.picture(i, 16, 16), "420") for i in range(3)]
    good = V.write_avi(frames, 16, 16)
    (movi_size,) = struct.unpack_from("<I", good, good.index(b"movi") - 4)
    for name, off in (("at_end", movi_size), ("past_end", movi_size + 4096), ("far", 0xFFFFFFF0)):
        files[f"offset_{name}.avi"] = V.write_avi(frames, 16, 16, index_offsets={1: off})
    for k in range(3):
        files[f"chunk_size_{k}.avi"] = V.write_avi(frames, 16, 16, chunk_sizes={k: 0xFFFFFFFF})
    movi_at = good.index(b"movi") - 4
    files["movi_size.avi"] = good[:movi_at] + struct.pack("<I", 0xFFFFFFFF) + good[movi_at + 4:]
    files["idx1_size.avi"] = good[:good.rindex(b"idx1") + 4] + struct.pack("<I", 0xFFFFFFFF) + good[good.rindex(b"idx1") + 8:]
    files["riff_size.avi"] = good[:4] + struct.pack("<I", 0xFFFFFFFF) + good[8:]
    files["empty.avi"] = b""
    return files


def _expected(data):
    """The status line's gist from the independent restatement: ("ok", sizes) or ("error",)."""
    try:
        frames, w, h = R.demux(data)
    except R.NotAvi:
        return ("error",)
    if frames[0][1] == 0:
        return ("error",)  # aeon has no frame to repeat yet: refused
    return ("ok", w, h, [n for _, n in frames])


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not os.path.exists("/opt/rocm/llvm/bin/clang++"):
        pytest.skip("no clang with sanitizer runtimes")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize_video"])
    d = tmp_path_factory.mktemp("video")
    files = _corpus()
    for k, v in files.items():
        (d / k).write_bytes(v)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([DRIVER] + [str(d / k) for k in sorted(files)], capture_output=True, text=True, env=env,
                       timeout=300)
    results = {}
    for line in r.stdout.splitlines():
        path, res = line.split("\t", 1)
        results[os.path.basename(path)] = res
    return r, results, files


def test_runs_clean(run):
    r, results, files = run
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert set(results) == set(files)
    assert sum(k.startswith("trunc_") for k in files) == 64 and sum(k.startswith("flip_") for k in files) == 200


def test_statuses_equal_the_reference(run):
    _, results, files = run
    kinds = set()
    for k, data in files.items():
        want, res = _expected(data), results[k]
        kinds.add(want[0])
        if want[0] == "error":
            assert res.startswith("error -1 "), (k, res)
        else:
            _, w, h, sizes = want
            head = f"ok {w}x{h} frames {len(sizes)} sizes {','.join(str(s) for s in sizes[:16])} jpeg "
            assert res.startswith(head), (k, res, head)
    assert kinds == {"ok", "error"}
    assert results["bb8.avi"] == "ok 80x60 frames 6 sizes 2944,0,2947,2957,2946,2947 jpeg 80x60x3 bad 0"
    assert results["synthetic_gray.avi"].endswith("jpeg 23x17x1 bad 0")
    assert results["offset_at_end.avi"].startswith("ok 16x16 frames 2 ")
    assert results["chunk_size_1.avi"] == "error -1 avi: the chunk of frame 1 runs past the datum"
    assert results["empty.avi"] == "error -1 avi: not a RIFF AVI file"


def test_product_library_reports_the_same(run):
    _, results, files = run
    for k, data in files.items():
        try:
            frames, w, h = A.avi_frames(data)
            got = f"ok {w}x{h} frames {len(frames)} sizes {','.join(str(n) for _, n in frames[:16])} jpeg "
            assert results[k].startswith(got), (k, results[k], got)
        except A.AeonHipError as e:
            assert results[k] == f"error {e.code} {str(e).split(': ', 1)[1]}", (k, results[k], str(e))
