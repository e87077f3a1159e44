"""The PNG stage on the CPU: aeon_png_gpu_emulate runs the code the kernels png_inflate and png_unfilter compile
(png_inflate.hpp), lane after lane, so these tests cover the inflate state machine, the skewed row filters and
the conversion without a device; aeon_png_host_stage is the host half and its routing rule.  Every file the GPU
tests (tests/test_hip_png.py) send is checked here to be routed to the device, so none of them can pass there
by falling back to the host decoder.
"""
import os
import subprocess
import zlib

import numpy as np
import pytest

import aeon_amd as A
from oracle import png_oracle as PO
from tests import png_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX = np.load(os.path.join(HERE, "golden", "png_fixtures.npz"))
NAMES = sorted({k.rsplit(".", 1)[0] for k in FX.files})
MODES = [(A.PNG_BGR8, "bgr8"), (A.PNG_GRAY8, "gray8"), (A.PNG_ANYDEPTH, "any")]
EDEVICE = -4


def _interlaced(png):
    return png[28] == 1  # IHDR's last byte


def _check(name, png):
    for mode, _ in MODES:
        want = A.decode_png(png, mode)
        ora = PO.decode(png, mode)
        got = A.png_gpu_emulate(png, mode)
        assert ora.dtype == want.dtype and np.array_equal(ora, want), (name, mode, "host decoder vs oracle")
        assert got.dtype == want.dtype and np.array_equal(got, want), (name, mode, np.argwhere(got != want)[:3].tolist())


@pytest.mark.parametrize("name", [n for n in NAMES if not _interlaced(FX[n + ".png"].tobytes())])
def test_emulation_matches_fixture(name):
    png = FX[name + ".png"].tobytes()
    assert A.png_host_stage(png)[0]
    for mode, key in MODES:
        got = A.png_gpu_emulate(png, mode)
        assert got.dtype == FX[name + "." + key].dtype and np.array_equal(got, FX[name + "." + key]), (name, key)
    _check(name, png)


def test_routing_rule():
    n_inter = 0
    for name in NAMES:
        png = FX[name + ".png"].tobytes()
        for mode, _ in MODES:
            route, staged = A.png_host_stage(png, mode)
            assert route == (not _interlaced(png)), name
            assert staged > 0
        if _interlaced(png):
            n_inter += 1
            with pytest.raises(A.AeonHipError) as e:
                A.png_gpu_emulate(png)
            assert e.value.code == -3
    assert n_inter > 0
    # a row wider than the unfilter kernel's LDS budget stays on the host: 16 KiB with its filter byte
    from tests import png_writer as W
    wide = W.write(np.zeros((2, 16384), np.uint8), 0, 8)
    fits = W.write(np.zeros((2, 16383), np.uint8), 0, 8)
    assert not A.png_host_stage(wide)[0] and A.png_host_stage(fits)[0]
    assert np.array_equal(A.png_gpu_emulate(fits), A.decode_png(fits))


@pytest.mark.parametrize("group", ["filter_files", "band_files", "split_files"])
def test_emulation_matches_decoder_on_writer_files(group):
    files = getattr(PC, group)()
    assert len(files) > 3
    for name, png in files:
        assert A.png_host_stage(png)[0], name
        _check(name, png)


def test_emulation_inflate_edges():
    for name, png, stream, raw in PC.inflate_files():
        assert zlib.decompress(stream) == raw, name  # zlib accepts the hand-built stream
        assert A.png_host_stage(png)[0], name
        _check(name, png)


def test_emulation_refuses_corrupt_data():
    for name, png in PC.corrupt_files():
        for mode, _ in MODES:
            assert A.png_host_stage(png, mode)[0], name  # routed: the device is what refuses it
            with pytest.raises(A.AeonHipError) as e:
                A.png_gpu_emulate(png, mode)
            assert e.value.code == EDEVICE, (name, str(e.value))


def test_parse_time_refusals_match_the_decoder():
    png = FX["gray8_n.png"].tobytes()
    bad = [b"\x89PNX" + png[4:], png[:16] + bytes([png[16] ^ 1]) + png[17:], png[:60], png[:33] + png[-12:]]
    for b in bad:
        with pytest.raises(A.AeonHipError) as e0:
            A.decode_png(b)
        for fn in (A.png_host_stage, A.png_gpu_emulate):
            with pytest.raises(A.AeonHipError) as e1:
                fn(b)
            assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))
    # a zlib header inflate refuses: refused by the host half, as the decoder's inflate does
    from tests import png_writer as W
    raw = W.scanlines(np.zeros((3, 3), np.uint8), 0, 8)
    z = zlib.compress(raw)
    for hdr in (b"\x79\x01", b"\x88\x1c", b"\x78\x20", b"\x78\x02"):
        b = W.png_from_stream(3, 3, 0, 8, hdr + z[2:])
        with pytest.raises(A.AeonHipError) as e0:
            A.decode_png(b)
        with pytest.raises(A.AeonHipError) as e1:
            A.png_host_stage(b)
        assert (e1.value.code, str(e1.value)) == (e0.value.code, str(e0.value))


def test_sanitizer_program(tmp_path):
    """tests/sanitize/png_stage_main.cpp under ASan + UBSan: the host half and the kernels' code over the
    non-interlaced and two interlaced fixtures, their truncations and single-byte mutations."""
    exe = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize", "png_stage_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize_png"])
    paths = []
    for name in NAMES:
        png = FX[name + ".png"].tobytes()
        if _interlaced(png) and name not in ("c2_8_i", "pal4_i"):
            continue
        (tmp_path / (name + ".png")).write_bytes(png)
        paths.append(str(tmp_path / (name + ".png")))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    r = subprocess.run([exe] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    files, runs, decoded, refused = [int(x) for x in __import__("re").findall(r"\d+", r.stdout.splitlines()[-1])]
    assert files == len(paths) and decoded > 3 * files and refused > decoded  # mutations that still decode; most do not
