"""The pixmap stage on the CPU: aeon_pixmap_gpu_emulate runs the code the kernel pixmap_convert compiles
(pixmap_rows.hpp), lane after lane, so these tests cover the band split, the realignment of unaligned source rows
and every conversion without a device; aeon_pixmap_host_stage is the host half and its routing rule.  Every file
the GPU tests (tests/test_hip_pixmap.py) send as device-routed is checked here to be routed to the device.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import aeon_amd as A
from tests import pixmap_cases as PC
from tests import pixmap_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX = np.load(os.path.join(HERE, "golden", "pixmap_fixtures.npz"))
NAMES = sorted({k.rsplit(".", 1)[0] for k in FX.files})
MODES = [(A.DECODE_BGR8, "bgr8"), (A.DECODE_GRAY8, "gray8"), (A.DECODE_ANYDEPTH, "any")]
EUNSUPPORTED = -3


def test_emulation_matches_decoder_on_every_device_file():
    files = PC.device_files()
    assert len(files) > 200
    for name, f in files:
        for mode, _ in MODES:
            assert A.pixmap_host_stage(f, mode) == (True, len(f)), name
            want, got = A.decode_pixmap(f, mode), A.pixmap_gpu_emulate(f, mode)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, mode, np.argwhere(got != want)[:3].tolist())


def test_emulation_matches_fixtures():
    for name in NAMES:
        f = FX[name + ".file"].tobytes()
        for mode, key in MODES:
            if name + "." + key in FX.files:
                got = A.pixmap_gpu_emulate(f, mode)
                assert got.dtype == FX[name + "." + key].dtype and np.array_equal(got, FX[name + "." + key]), (name, key)


def test_routing_rule():
    """gpu_route == 1 exactly for binary PNM and uncompressed BMP; staged_bytes is the file for routed files, the
    pixels for the others."""
    for name, f in PC.device_files():
        assert f[:2] in (b"P4", b"P5", b"P6", b"BM"), name
    for name, f in PC.ascii_files():
        assert f[:2] in (b"P1", b"P2", b"P3"), name
        for mode, _ in MODES:
            px = A.decode_pixmap(f, mode)
            assert A.pixmap_host_stage(f, mode) == (False, px.nbytes), name
            with pytest.raises(A.AeonHipError) as e:
                A.pixmap_gpu_emulate(f, mode)
            assert e.value.code == EUNSUPPORTED, name


def test_emulation_writes_nothing_outside_a_row():
    """Strides that leave every row's start at another alignment, in a pre-filled buffer."""
    import ctypes
    for name, f in PC.device_files()[::7]:
        for mode, _ in MODES:
            want = A.decode_pixmap(f, mode)
            h, rowb = want.shape[0], want.nbytes // want.shape[0]
            for pad in (1, 2, 3, 5):
                buf = np.full(h * (rowb + pad) + 16, 0x5A, np.uint8)
                rc = A.lib().aeon_pixmap_gpu_emulate(f, len(f), mode, buf.ctypes.data + 16 - buf.ctypes.data % 16, rowb + pad)
                assert rc == 0, name
                o = 16 - buf.ctypes.data % 16
                rows = buf[o:o + h * (rowb + pad)].reshape(h, rowb + pad)
                assert np.all(rows[:, rowb:] == 0x5A) and np.all(buf[:o] == 0x5A), (name, mode, pad)
                assert np.array_equal(rows[:, :rowb].reshape(-1), want.view(np.uint8).reshape(-1)), (name, mode, pad)


def test_sanitizer_program(tmp_path):
    """tests/sanitize/pixmap_stage_main.cpp under ASan + UBSan: the decoder, the host half and the kernel's code over
    files of every kind, their truncations at every header byte and 64 single-byte mutations each."""
    exe = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize", "pixmap_stage_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize_pixmap"])
    rng = np.random.default_rng(3)
    pal = rng.integers(0, 256, (12, 3))
    files = {
        "p1.pbm": (W.pnm(1, rng.integers(0, 2, (3, 9)), digits_tight=True), "HHH"),
        "p2.pgm": (W.pnm(2, rng.integers(0, 300, (2, 5)), 300, comment=6), "HHH"),
        "p3.ppm": (W.pnm(3, rng.integers(0, 256, (2, 3, 3)), 255), "HHH"),
        "p4.pbm": (W.pnm(4, rng.integers(0, 2, (5, 13)), comment=9), "DDD"),
        "p5.pgm": (W.pnm(5, rng.integers(0, 256, (4, 7)), 255), "DDD"),
        "p5w.pgm": (W.pnm(5, rng.integers(0, 65536, (4, 7)), 65535, comment=3), "DDD"),
        "p6.ppm": (W.pnm(6, rng.integers(0, 256, (3, 5, 3)), 255, comment=4), "DDD"),
        "p6w.ppm": (W.pnm(6, rng.integers(0, 65536, (3, 5, 3)), 4095), "DDD"),
        "b1.bmp": (W.bmp(rng.integers(0, 2, (3, 11)), 1, pal[:2], gap=1), "DDD"),
        "b4.bmp": (W.bmp(rng.integers(0, 16, (3, 7)), 4, pal, header=108), "DDD"),
        "b8.bmp": (W.bmp(rng.integers(0, 256, (3, 6)), 8, rng.integers(0, 256, (256, 3)), header=12), "DDD"),
        "b24.bmp": (W.bmp(rng.integers(0, 256, (3, 5, 3)), 24, top_down=True, gap=2), "DDD"),
        "b32.bmp": (W.bmp(rng.integers(0, 256, (2, 3, 4)), 32, header=124), "DDD"),
        "rle.bmp": (W.bmp(rng.integers(0, 256, (2, 3)), 8, rng.integers(0, 256, (256, 3)), compression=1), "rrr"),
    }
    paths = []
    for name, (f, _) in files.items():
        (tmp_path / name).write_bytes(f)
        paths.append(str(tmp_path / name))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    r = subprocess.run([exe] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    outcome = dict(l.rsplit(": ", 1) for l in lines[:-1])
    for name, (f, want) in files.items():
        assert outcome[name] == want, (name, outcome[name])
        # cut anywhere inside the header: refused in every mode
        assert outcome[f"{name} cut at 1"] == "rrr" and outcome[f"{name} cut at 9"] == "rrr", name
        cuts = [k for k in outcome if k.startswith(name + " cut at ")]
        muts = [k for k in outcome if k.startswith(name + " mutation ")]
        assert len(cuts) >= 20 and len(muts) == 64, (name, len(cuts), len(muts))
        assert all(set(outcome[k]) <= set("DHr-") for k in cuts + muts)
    nfiles, runs, decoded, refused = [int(x) for x in re.findall(r"\d+", lines[-1])]
    assert nfiles == len(paths) and decoded > 3 * nfiles and refused > 3 * nfiles
