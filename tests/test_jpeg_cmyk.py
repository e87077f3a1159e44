"""CPU: CMYK, YCCK and Adobe-RGB JPEG files through the host half of the JPEG stage.

The header parser reports four components, the host entropy decoder and the GPU path's host stage
accept the files, tests/jpeg_cmyk_ref.py reproduces libjpeg-turbo's YCCK -> CMYK conversion, and what
libjpeg refuses stays refused.  The GPU entropy decoder's algorithm (jpeg_huff.hpp's phases, emulated
on the host by the stand-alone sanitizer driver) decodes every sequential fixture to the host decoder's
coefficients at each workgroup size.
"""
import os
import subprocess

import numpy as np
import pytest

import aeon_amd as A
from tests import jpeg_cmyk_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX = np.load(os.path.join(HERE, "golden", "jpeg_cmyk_fixtures.npz"))
NAMES = sorted(k[:-4] for k in FX.files if k.endswith(".jpg"))
FOUR = [n for n in NAMES if n != "rgb_adobe"]
DRIVER = os.path.join(ROOT, "aeon_amd", "csrc", "build_sanitize", "fuzz_driver")


def _jpg(name):
    return FX[name + ".jpg"].tobytes()


def test_fixture_set():
    assert len(NAMES) == 15 and "ycck_37x53" in NAMES and "prog_cmyk" in NAMES


@pytest.mark.parametrize("name", FOUR)
def test_jpeg_info_four_components(name):
    h, w = FX[name + ".gray"].shape
    assert A.jpeg_info(_jpg(name)) == (w, h, 4)


def test_jpeg_info_adobe_rgb():
    h, w = FX["rgb_adobe.gray"].shape
    assert A.jpeg_info(_jpg("rgb_adobe")) == (w, h, 3)


@pytest.mark.parametrize("name", NAMES)
def test_host_paths_accept(name):
    b = _jpg(name)
    h, w = FX[name + ".gray"].shape
    ncomp = 3 if name == "rgb_adobe" else 4
    ew, eh, en, n_blocks, n_values = A.jpeg_entropy_decode(b)[:5]
    assert (ew, eh, en) == (w, h, ncomp) and n_blocks > 0 and n_values > 0
    gpu_entropy, staged = A.jpeg_host_stage(b)
    assert bool(gpu_entropy) == (not name.startswith("prog_")) and staged > 0


def test_reference_reproduces_pillow_ycck():
    """The YCCK fixture is a CMYK file with its Adobe transform byte patched to 2: Pillow's decode of the
    unpatched file gives libjpeg's Y, Cb, Cr, K samples, its decode of the patched one libjpeg-turbo's
    ycck_cmyk_convert of them."""
    assert np.array_equal(R.ycck_to_cmyk(FX["ycck_37x53.ycck"]), FX["ycck_37x53.cmyk"])
    bgr, gray = R.decode(FX["ycck_37x53.cmyk"])
    assert np.array_equal(bgr, FX["ycck_37x53.bgr"]) and np.array_equal(gray, FX["ycck_37x53.gray"])


def test_reference_formula_corners():
    """K = 255 gives 255 - ((255 - c) * 255 >> 8) (the >> 8 in place of / 255: c itself at 255, else
    c + 1); K = 0 gives black whatever c, m, y are."""
    cmy = np.arange(256, dtype=np.uint8)
    px = np.stack([cmy, cmy[::-1], cmy, np.full(256, 255, np.uint8)], axis=-1)[None]
    want = np.minimum(cmy.astype(np.int32) + 1, 255).astype(np.uint8)
    assert np.array_equal(R.cmyk_to_bgr(px)[0], np.stack([want, want[::-1], want], axis=-1))
    px[..., 3] = 0
    assert not R.cmyk_to_bgr(px).any() and not R.cmyk_to_gray(px).any()
    assert np.array_equal(FX["cmyk_k0.bgr"], np.zeros_like(FX["cmyk_k0.bgr"]))
    assert FX["cmyk_k255.bgr"].any()


def _sof(b):
    i = b.index(b"\xff\xc0")
    return i, b[i + 9]


def test_two_components_still_refused():
    b = bytearray(np.load(os.path.join(HERE, "golden", "jpeg_fixtures.npz"))["s444_q90.jpg"].tobytes())
    i, ncomp = _sof(b)
    assert ncomp == 3
    b[i + 9] = 2
    for fn in (A.jpeg_info, A.jpeg_entropy_decode, A.jpeg_host_stage):
        with pytest.raises(A.AeonHipError, match="component"):
            fn(bytes(b))


def test_four_components_short_sof_refused():
    """A frame header that counts four components in a segment sized for three is refused, not read
    past its segment."""
    b = bytearray(np.load(os.path.join(HERE, "golden", "jpeg_fixtures.npz"))["s444_q90.jpg"].tobytes())
    i, _ = _sof(b)
    b[i + 9] = 4
    with pytest.raises(A.AeonHipError, match="bad frame header"):
        A.jpeg_info(bytes(b))


def test_four_component_mcu_of_twelve_blocks_refused():
    """2x2, 2x2, 2x1, 2x1: 12 blocks per MCU of the interleaved scan, past libjpeg's
    D_MAX_BLOCKS_IN_MCU (10); the header alone still parses."""
    b = bytearray(_jpg("cmyk_444_37x53"))
    i, ncomp = _sof(b)
    assert ncomp == 4
    for k, hv in enumerate((0x22, 0x22, 0x21, 0x21)):
        b[i + 11 + 3 * k] = hv
    b = bytes(b)
    assert A.jpeg_info(b)[2] == 4
    for fn in (A.jpeg_entropy_decode, A.jpeg_host_stage):
        with pytest.raises(A.AeonHipError, match="sampling factors too large"):
            fn(b)


def test_ten_block_mcu_accepted():
    """2x2, 1x1, 1x1, 2x2 is exactly 10 blocks per MCU: the header and the scan's shape are accepted (the
    entropy-coded data of the patched file no longer fits, so only the host stage's parse is asked)."""
    b = bytearray(_jpg("cmyk_444_37x53"))
    i, _ = _sof(b)
    for k, hv in enumerate((0x22, 0x11, 0x11, 0x22)):
        b[i + 11 + 3 * k] = hv
    gpu_entropy, _ = A.jpeg_host_stage(bytes(b))
    assert gpu_entropy


def _parse(stdout):
    results, gpu = {}, {}
    for line in stdout.splitlines():
        if line.startswith("gpu\t"):
            _, path, res = line.split("\t")
            gpu[os.path.basename(path)] = res
        else:
            path, res = line.split("\t", 1)
            results[os.path.basename(path)] = res
    return results, gpu


def test_gpu_entropy_emulation_matches_host_decoder(tmp_path):
    """The stand-alone driver (tests/sanitize/fuzz_driver.cpp under ASan + UBSan) on the fixtures: it
    runs jpeg_huff's phases on the host at 1,024, 512 and 256 lanes and reports "gpu ok <hash>" only when
    all three agree; that hash must be the host entropy decoder's.  The progressive file stays with the
    host decoder."""
    if not os.path.exists("/opt/rocm/llvm/bin/clang++"):
        pytest.skip("no clang with sanitizer runtimes")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize"])
    for k in NAMES:
        (tmp_path / (k + ".jpg")).write_bytes(_jpg(k))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([DRIVER] + [str(tmp_path / (k + ".jpg")) for k in NAMES], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    results, gpu = _parse(r.stdout)
    for k in NAMES:
        host, g = results[k + ".jpg"], gpu[k + ".jpg"]
        assert host.startswith("ok"), (k, host)
        if k.startswith("prog_"):
            assert g == "gpu host", (k, g)
        else:
            assert g.startswith("gpu ok") and host.split("hash ")[1] == g.split()[2], (k, host, g)
    # the long scans settle in more than one Jacobi round
    assert int(gpu["cmyk_long.jpg"].split("rounds ")[1]) >= 1
