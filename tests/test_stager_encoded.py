"""CPU: the encoded half of the aeon-side drop-in without a device.

encoded_info (aeon_encoded_info) against the per-format entries it stands for: one file of every format and of every
route of the decoder's routing rule, refusals and malformed headers with the parser's own code and message.

The stager's encoded path (aeon_amd/csrc/stager.cpp + stager_encoded.cpp) over a model device that decodes, under
AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer: `make -C aeon_amd/csrc
sanitize_stager_encoded tsan_stager_encoded` builds tests/sanitize/stager_encoded_driver.cpp (a stand-alone program)
with tests/sanitize/model_decode.cpp and the library's host decoders; each binary runs as a plain child process.
The scenarios: eight threads staging the encoded and decoded records of one window, three windows over two
containers, windows of files alone, a header error in mid-window with that idx staged again, every decode entry
failing once at launch (the window dropped, the next one right), a third window staged while the first was never
waited for.  The driver compares every slot and counts encoded files that a host-to-device copy carried as well."""
import os
import subprocess

import numpy as np
import pytest

import aeon_amd as A
from tests import stager_encoded_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize")
EINVAL, ERUNTIME, EUNSUPPORTED = -1, -2, -3
W, H = 131, 77


def _info(fmt, w, h, fcn, eb, route):
    return dict(format=fmt, width=w, height=h, file_channels=fcn, elem_bytes=eb, device_route=route)


IMAGE_FILES = ["jpeg420", "jpeg_gray", "jpeg_prog", "png_palette", "png_noise", "ppm_p6", "ppm_p3", "bmp_pal8", "tiff_lzw",
               "tiff_deflate_noise"]


@pytest.mark.parametrize("kind", IMAGE_FILES)
def test_encoded_info_equals_the_format_entries(kind):
    f = SC.image_file(kind, 11, W, H)
    got = A.encoded_info(f)
    if kind.startswith("jpeg"):
        w, h, n = A.jpeg_info(f)
        assert got == _info(A.FORMAT_JPEG, w, h, n, 1, True)
        assert n == (1 if kind == "jpeg_gray" else 3)
    elif kind.startswith("png"):
        w, h, depth, ctype = A.png_info(f)
        route = A.png_decoder_route(f)
        assert got == _info(A.FORMAT_PNG, w, h, {0: 1, 2: 3, 3: 3, 4: 2, 6: 4}[ctype], 1, route)
        assert route == (kind == "png_palette")  # flat indices go to the device, noise stays on the host
    elif kind.startswith(("ppm", "bmp")):
        w, h, depth, fcn, _ = A.pixmap_info(f)
        route = A.pixmap_host_stage(f)[0]
        assert got == _info(A.FORMAT_PIXMAP, w, h, fcn, 1, route)
        assert route == (kind != "ppm_p3")  # ASCII samples decode on the host
    else:
        w, h, fcn, eb = A.tiff_info(f)
        route = A.tiff_decoder_route(f)
        assert got == _info(A.FORMAT_TIFF, w, h, fcn, 1, route)
        assert route == (kind == "tiff_lzw")  # noisy Deflate strips decode on the host
    assert (got["width"], got["height"]) == (W, H)


def test_encoded_info_lzw_strip_above_32k_is_host_routed():
    f = SC.image_file("tiff_lzw_big", 5, 300, 200)  # one strip of 180 000 bytes
    assert A.encoded_info(f)["device_route"] is False and A.tiff_decoder_route(f) is False


@pytest.mark.parametrize("kind", SC.MASK_KINDS + ["pgm16"])
def test_encoded_info_masks(kind):
    """mask=True: ANYDEPTH; elem_bytes is 2 exactly where the host decoder gives uint16."""
    if kind == "pgm16":
        from tests import pixmap_writer as XW
        f = XW.pnm(5, A.synthetic_image(3, W, H, 1).astype(np.uint16) * 200, maxval=65535)
    else:
        f = SC.mask_file(kind, 13, W, H)
    got = A.encoded_info(f, mask=True)
    dec = SC.decode_mask(f)
    assert got["elem_bytes"] == dec.dtype.itemsize and dec.shape == (H, W)
    assert got["elem_bytes"] == (1 if kind == "png_palette" else 2)
    assert A.encoded_info(f, mask=False)["elem_bytes"] == 1  # images decode to 8 bits whatever the file holds


def test_refusals_and_malformed_headers_keep_the_stage_s_code_and_message():
    def both(fn, data, **kw):
        """The per-format entry's error and encoded_info's must be the same."""
        with pytest.raises(A.AeonHipError) as want:
            fn(data)
        with pytest.raises(A.AeonHipError) as got:
            A.encoded_info(data, **kw)
        assert (got.value.code, str(got.value)) == (want.value.code, str(want.value))
        return want.value

    jpg, png = SC.image_file("jpeg420", 1, W, H), SC.image_file("png_palette", 1, W, H)
    ppm, tif = SC.image_file("ppm_p6", 1, W, H), SC.image_file("tiff_lzw", 1, W, H)
    assert both(A.jpeg_info, jpg[:30]).code == EINVAL
    assert both(A.png_info, png[:20]).code == EINVAL
    assert both(A.pixmap_info, ppm[:4]).code == EINVAL
    from tests import tiff_writer as TW
    cut = TW.write(A.synthetic_image(4, 20, 10, 3), 2, ifd_first=True)[:40]  # the IFD starts at 8 and is cut short
    assert "TIFF:" in str(both(A.tiff_info, cut))
    # the TIFF sniff is strict, as the decoder's: a file whose IFD offset lies past its end is the JPEG parser's
    with pytest.raises(A.AeonHipError, match="JPEG: not a JPEG file") as e:
        A.encoded_info(tif[:12])
    assert e.value.code == EINVAL
    assert both(A.jpeg_info, b"not an image at all").code == EINVAL  # no sniff takes it: the JPEG parser's refusal
    twelve = bytearray(jpg)
    sof = twelve.index(b"\xff\xc0")
    twelve[sof + 4] = 12  # 12-bit samples
    assert both(A.jpeg_info, bytes(twelve)).code == EUNSUPPORTED
    from tests import pixmap_writer as XW
    rle = XW.bmp(A.synthetic_image(2, 16, 8, 1), 8, palette=np.zeros((256, 3), np.uint8), compression=1)
    assert both(A.pixmap_info, rle).code == EUNSUPPORTED
    with pytest.raises(A.AeonHipError, match="encoded pixel masks are decoded from PNG files only") as e:
        A.encoded_info(jpg, mask=True)
    assert e.value.code == ERUNTIME


# ---- the sanitizer programs ----
SCENARIOS = ["concurrent_mixed", "three_windows_two_containers", "encoded_only", "header_error_restage",
             "batch_call_fails", "third_window_unwaited"]
# Seconds: the whole run measured 0.12 s under ASan + UBSan and 0.17 s under ThreadSanitizer; the bound leaves a
# loaded machine room to start the process.  The driver arms alarm() with it, so a scenario that spins ends by
# itself with a FAIL line.
LIMIT = {"sanitize_stager_encoded": 5, "tsan_stager_encoded": 5}
BINARY = {"sanitize_stager_encoded": "stager_encoded_driver_asan", "tsan_stager_encoded": "stager_encoded_driver_tsan"}


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
