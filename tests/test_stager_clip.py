"""CPU: the video half of the aeon-side drop-in without a device.

clip_info (aeon_clip_info) against tests/video_ref.py's demux and the oracle's JPEG header parser: the four encodings,
aeon's bb8.avi with its empty chunk, max_frames below, at and above the frame count, an avih size that is not the
frames'; its refusals with the demux's own code and text.

The stager's clip path (aeon_amd/csrc/stager.cpp + stager_clip.cpp with the demux and the JPEG header parser) over
the decoding model device and a model of the video call, under AddressSanitizer + UndefinedBehaviorSanitizer and under
ThreadSanitizer: `make -C aeon_amd/csrc sanitize_stager_clip tsan_stager_clip` builds
tests/sanitize/stager_clip_driver.cpp (a stand-alone program) with tests/sanitize/model_decode.cpp and
tests/sanitize/model_video.cpp; each binary runs as a plain child process.  The scenarios: both forms staged from
eight threads, two windows in flight and a third staged over an unwaited first, a hole in a batch, refused clips with
the idx staged again, the JPEG call and the video call failing once at launch (the window dropped, the next one
right), the consumer's wait by buffer alone, destroy with a window launched, a batch of more than 65,535 frames."""
import os
import subprocess

import pytest

import aeon_amd as A
import oracle as O
from tests import video_cases as V
from tests import video_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize")
EINVAL = -1


def _reference(data, max_frames):
    frames, _, _ = R.demux(data)
    off, n = frames[0]
    w, h, _ = O.jpeg_info(data[off:off + n])
    return min(len(frames), max_frames), w, h


@pytest.mark.parametrize("max_frames", [3, 6, 9])
@pytest.mark.parametrize("enc", V.ENCODINGS)
def test_clip_info_equals_the_demux_and_the_header(enc, max_frames):
    """Six frames of 48 x 40 (one an empty chunk) under an avih that claims 64 x 64: the size is the first frame's."""
    frames = [b"" if i == 2 else V.encode(V.picture(i, 48, 40), enc) for i in range(6)]
    data = V.write_avi(frames, 64, 64)
    assert R.demux(data)[1:] == (64, 64)
    got = A.clip_info(data, max_frames)
    assert got == _reference(data, max_frames) == (min(6, max_frames), 48, 40)


@pytest.mark.parametrize("max_frames", [1, 2, 6, 16])
def test_clip_info_bb8(max_frames):
    data = V.bb8()
    assert [n for _, n in R.demux(data)[0]] == V.BB8_SIZES
    assert A.clip_info(data, max_frames) == _reference(data, max_frames) == (min(6, max_frames), 80, 60)


def test_clip_info_refusals_are_the_demux_s():
    f = [V.encode(V.picture(i, 16, 16), "420") for i in range(3)]

    def both(data, max_frames, text):
        """The demux's error and clip_info's must be the same."""
        with pytest.raises(A.AeonHipError) as want:
            A.avi_frames(data, max_frames)
        with pytest.raises(A.AeonHipError) as got:
            A.clip_info(data, max_frames)
        assert (got.value.code, str(got.value)) == (want.value.code, str(want.value)) and want.value.code == EINVAL
        assert text in str(got.value), str(got.value)

    both(b"not an AVI file at all", 4, "not a RIFF AVI file")
    both(V.write_avi(f, 16, 16, flags=0), 4, "Not a valid AVI file type")  # the index flag cleared
    past = V.write_avi(f, 16, 16, chunk_sizes={1: 0xFFFFFFFF})
    both(past, 4, "runs past the datum")
    assert A.clip_info(past, 1) == (1, 16, 16)  # (frame 1 is not kept: its chunk header is not read)
    both(V.write_avi([b""] + f, 16, 16), 4, "the first frame is empty")
    # a first frame that is no JPEG file: the JPEG parser's refusal
    with pytest.raises(A.AeonHipError) as want:
        A.jpeg_info(b"junk" * 8)
    with pytest.raises(A.AeonHipError) as got:
        A.clip_info(V.write_avi([b"junk" * 8] + f, 16, 16), 4)
    assert (got.value.code, str(got.value)) == (want.value.code, str(want.value))
    with pytest.raises(A.AeonHipError, match="max_frames must be > 0"):
        A.clip_info(V.write_avi(f, 16, 16), 0)


# ---- the sanitizer programs ----
SCENARIOS = ["both_forms_8_threads", "two_windows_and_a_third", "hole_in_a_batch", "refused_clip_restaged", "batch_call_fails",
             "wait_by_buffer", "destroy_with_window_launched", "split_above_65535_frames"]
# Seconds: the whole run measured under one second in either build; the bound leaves a loaded machine room to start
# the process.  The driver arms alarm() with it, so a scenario that spins ends by itself with a FAIL line.
LIMIT = {"sanitize_stager_clip": 10, "tsan_stager_clip": 10}
BINARY = {"sanitize_stager_clip": "stager_clip_driver_asan", "tsan_stager_clip": "stager_clip_driver_tsan"}


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
