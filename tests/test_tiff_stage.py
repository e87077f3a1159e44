"""The TIFF stage on the CPU: aeon_tiff_gpu_emulate runs the code the kernels tiff_expand and tiff_convert compile
(tiff_strips.hpp, and png_inflate.hpp's inflate_file in its cut mode), lane after lane, so these tests cover the LZW
range table, the PackBits walk, the inflate of strips, the band split, the predictor's carried sums and every
conversion without a device; aeon_tiff_host_stage is the host half and its routing rule.  Every file the GPU tests
(tests/test_hip_tiff.py) send as device-routed is checked here to be routed to the device.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import aeon_amd as A
from tests import tiff_cases as TC
from tests import tiff_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX = np.load(os.path.join(HERE, "golden", "tiff_fixtures.npz"))
MODES = [A.DECODE_BGR8, A.DECODE_GRAY8, A.DECODE_ANYDEPTH]
EUNSUPPORTED, EDEVICE = -3, -4


def test_emulation_matches_decoder_on_every_device_file():
    files = TC.device_files()
    assert len(files) > 150
    for name, f in files:
        for mode in MODES:
            assert A.tiff_host_stage(f, mode) == (True, len(f)), name
            want, got = A.decode_tiff(f, mode), A.tiff_gpu_emulate(f, mode)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, mode, np.argwhere(got != want)[:3].tolist())


def test_emulation_matches_decoder_on_the_pillow_fixtures():
    n = 0
    for k in sorted(FX.files):
        if not k.endswith(".file") or "_RGBA_" in k:
            continue
        f = FX[k].tobytes()
        for mode in MODES:
            assert A.tiff_host_stage(f, mode)[0], k
            assert np.array_equal(A.tiff_gpu_emulate(f, mode), A.decode_tiff(f, mode)), (k, mode)
        n += 1
    assert n == 40


def test_routing_rule_at_its_boundaries():
    """An LZW / PackBits strip of 32,768 decoded bytes is the device's, one of 32,769 the host's; Deflate and
    uncompressed strips have no cap; the rule reads the header alone (RowsPerStrip x the row's bytes)."""
    g = np.zeros((198, 331), np.uint8)
    for comp, want in [("lzw", False), ("packbits", False), ("deflate", True), ("raw", True)]:
        f = W.write(g, 1, comp, rps=99)  # 32,769 bytes a strip
        assert A.tiff_host_stage(f)[0] is want and A.tiff_decoder_route(f) is want, comp
        if not want:
            assert A.tiff_host_stage(f) == (False, g.size * 3)
            with pytest.raises(A.AeonHipError) as e:
                A.tiff_gpu_emulate(f)
            assert e.value.code == EUNSUPPORTED
    g = np.zeros((128, 512), np.uint8)
    for comp in ("lzw", "packbits"):
        assert A.tiff_host_stage(W.write(g, 1, comp, rps=64))[0] is True    # 32,768
        assert A.tiff_host_stage(W.write(g, 1, comp, rps=65))[0] is False
        assert A.tiff_host_stage(W.write(g, 1, comp))[0] is False           # RowsPerStrip absent: one strip of 65,536
    for name, f in TC.host_files():
        for mode in MODES:
            assert A.tiff_host_stage(f, mode)[0] is False, name


def test_decoder_route_of_deflate_files_goes_by_the_strips_size():
    """The decoder's rule on top (kTiffDecoderDeflateMinRatio = 3, from the header alone): a Deflate file goes through
    the stage when its strips hold at most a third of its samples' bytes; the C entry keeps the plain rule."""
    rng = np.random.default_rng(8)
    noisy = rng.integers(0, 256, (64, 64)).astype(np.uint8)
    flat = (np.arange(64 * 64).reshape(64, 64) // 256).astype(np.uint8)
    for a, comp, want in [(noisy, "deflate", False), (flat, "deflate", True), (noisy, "adobe", False), (noisy, "lzw", True),
                          (noisy, "packbits", True), (noisy, "raw", True)]:
        f = W.write(a, 1, comp, rps=16)
        assert A.tiff_host_stage(f)[0] is True and A.tiff_decoder_route(f) is want, comp
    # at the boundary: strips of exactly a third (stored blocks: 4,096 samples in 1,365 + 1 bytes does not pass, 1,365 does)
    for nbytes, want in [(1365, True), (1366, False)]:
        f = W.write(flat, 1, "deflate", codec=lambda d: b"\x78\x01" + bytes(nbytes - 2))  # (the rule reads StripByteCounts, not the data)
        assert A.tiff_decoder_route(f) is want, nbytes


def test_emulation_writes_nothing_outside_a_row():
    """Strides that leave every row's start at another alignment, in a pre-filled buffer with guard bytes."""
    for name, f in TC.device_files()[::5]:
        for mode in MODES:
            want = A.decode_tiff(f, mode)
            h, rowb = want.shape[0], want.nbytes // want.shape[0]
            for pad in (1, 2, 3, 5):
                buf = np.full(h * (rowb + pad) + 32, 0x5A, np.uint8)
                o = 16 - buf.ctypes.data % 16
                rc = A.lib().aeon_tiff_gpu_emulate(f, len(f), mode, buf.ctypes.data + o, rowb + pad)
                assert rc == 0, name
                rows = buf[o:o + h * (rowb + pad)].reshape(h, rowb + pad)
                assert np.all(rows[:, rowb:] == 0x5A) and np.all(buf[:o] == 0x5A) and np.all(buf[o + rows.size:] == 0x5A), (name, mode, pad)
                assert np.array_equal(rows[:, :rowb].reshape(-1), want.view(np.uint8).reshape(-1)), (name, mode, pad)


def test_corrupt_strips_are_device_errors_in_the_emulation():
    for name, f in TC.corrupt_files():
        assert A.tiff_host_stage(f) == (True, len(f)), name
        with pytest.raises(A.AeonHipError) as e:
            A.tiff_gpu_emulate(f)
        assert e.value.code == EDEVICE, (name, str(e.value))


def test_sanitizer_program(tmp_path):
    """tests/sanitize/tiff_stage_main.cpp under ASan + UBSan: the decoder, the host half and the kernels' code over
    files of every compression and sample layout, their truncations at every header and IFD byte and 64 single-byte
    mutations each."""
    exe = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize", "tiff_stage_main")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize_tiff"])
    rng = np.random.default_rng(3)
    K = {k[0]: k for k in TC.KINDS}
    files = {
        "raw_rgb.tif": (TC.make(rng, K["rgb8"], 5, 9, "raw", rps=2, pad=3), "DDD"),
        "raw_gray16be.tif": (TC.make(rng, K["gray16"], 4, 7, "raw", big=True), "DDD"),
        "lzw_rgb_pred.tif": (TC.make(rng, K["rgb8"], 9, 40, "lzw", pred=2, rps=4), "DDD"),
        "lzw_gray16_pred_be.tif": (TC.make(rng, K["gray16"], 6, 33, "lzw", pred=2, big=True, rps=5, ifd_first=True), "DDD"),
        "lzw_pal.tif": (TC.make(rng, K["pal8"], 7, 21, "lzw", rps=3), "DDD"),
        "packbits_rgba.tif": (TC.make(rng, K["rgba8"], 6, 30, "packbits", rps=4, pad=1), "DDD"),
        "packbits_white.tif": (TC.make(rng, K["white8"], 3, 70, "packbits"), "DDD"),
        "deflate_rgb16_pred.tif": (TC.make(rng, K["rgb16"], 8, 25, "deflate", pred=2, rps=3, pad=2), "DDD"),
        "deflate_stored.tif": (W.write(TC.image(rng, 5, 30, 1, np.uint8), 1, "deflate", rps=2, codec=lambda d: W.deflate_stored(d, 40)), "DDD"),
        "deflate_fixed_cut.tif": (W.write(TC.image(rng, 5, 30, 1, np.uint8), 1, "deflate", rps=5, tail=b"\7" * 40, codec=W.deflate_fixed), "DDD"),
        "lzw_host.tif": (TC.make(rng, K["gray8"], 198, 331, "lzw", rps=99), "HHH"),
        "pillow_lzw.tif": (FX["tiff_lzw_RGB_1.file"].tobytes(), "DDD"),
        "pillow_deflate16.tif": (FX["tiff_adobe_deflate_I16_1.file"].tobytes(), "DDD"),
        "jpeg_in_tiff.tif": (W.write(np.zeros((3, 3), np.uint8), 1, 7), "rrr"),
    }
    paths = []
    for name, (f, _) in files.items():
        (tmp_path / name).write_bytes(f)
        paths.append(str(tmp_path / name))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    r = subprocess.run([exe] + paths, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    outcome = dict(l.rsplit(": ", 1) for l in lines[:-1])
    for name, (f, want) in files.items():
        assert outcome[name] == want, (name, outcome[name])
        assert outcome[f"{name} cut at 1"] == "rrr" and outcome[f"{name} cut at 7"] == "rrr", name
        cuts = [k for k in outcome if k.startswith(name + " cut at ")]
        muts = [k for k in outcome if k.startswith(name + " mutation ")]
        assert len(cuts) >= 20 and len(muts) == 64, (name, len(cuts), len(muts))
        assert all(set(outcome[k]) <= set("DHrc-") for k in cuts + muts)
    nfiles, runs, decoded, refused, corrupt = [int(x) for x in re.findall(r"\d+", lines[-1])]
    assert nfiles == len(paths) and decoded > 3 * nfiles and refused > 3 * nfiles and corrupt > 0
