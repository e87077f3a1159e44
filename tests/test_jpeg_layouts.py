"""CPU: the JPEG sampling layouts, tables and stream structures no encoder at hand produces.

tests/golden/jpeg_layout_fixtures.npz holds files written by tests/jpeg_writer.py (every layout of
make_jpeg_layout_fixtures.py's table) with Pillow's decode of each.  Here: the writer still produces the
committed bytes, the oracle's decode equals Pillow's to the pixel at both channel counts, the header
parser, the host entropy decoder and the GPU path's host stage accept every file, the GPU entropy
decoder's algorithm (jpeg_huff.hpp's phases, emulated on the host by the stand-alone sanitizer driver)
gives the host decoder's coefficients at each workgroup size, and what Pillow refuses is refused.
"""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import aeon_amd as A
import oracle
from tests import jpeg_writer as JW
from tests.test_jpeg_cmyk import DRIVER, _parse

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX = np.load(os.path.join(HERE, "golden", "jpeg_layout_fixtures.npz"))

NAMES = [
    # sampling layouts
    "y1x2_37x29", "y1x2_5x1", "y1x2_5x2", "y1x2_5x3", "y1x2_5x17", "y1x2_1x9", "y1x2_2x9", "y1x2_3x9",
    "y4x1", "y1x4", "y4x2", "y3x1", "mixed_c", "one_c_sub", "luma_sub", "gray_22", "gray_22_33x9",
    "w_thresh_h2v1_3", "w_thresh_h2v1_4", "w_thresh_h2v1_5", "w_thresh_h2v1_6",
    "w_thresh_h2v2_3", "w_thresh_h2v2_4", "w_thresh_h2v2_5", "w_thresh_h2v2_6", "cmyk_440",
    # tables
    "q16", "tab_ids_23", "tab_swapped", "tab_three", "huff_long", "huff_one_symbol",
    # coefficients
    "coef_extremes", "zz63", "all_ac",
    # streams
    "rst1_gray_529", "rst1_444_289", "rst_odd", "rst_single", "stuffed", "fill_bytes", "segments_shuffled",
]
REFUSED = ["frac_y3x1_c2x1"]  # Pillow (libjpeg) refuses these: fractional sampling ratios
HOST_ENTROPY = {"tab_three"}  # three Huffman table pairs: past the GPU decoder's two slots


def _jpg(name):
    return FX[name + ".jpg"].tobytes()


def _ncomp(name):
    return 4 if name == "cmyk_440" else 1 if name in ("gray_22", "gray_22_33x9", "coef_extremes", "rst1_gray_529") else 3


def test_fixture_set():
    assert sorted(k[:-4] for k in FX.files if k.endswith(".jpg")) == sorted(NAMES + REFUSED)
    assert sorted(k[:-4] for k in FX.files if k.endswith(".bgr")) == sorted(NAMES)
    assert sorted(k[:-5] for k in FX.files if k.endswith(".gray")) == sorted(NAMES)
    assert sorted(FX["refused"].tolist()) == sorted(REFUSED)
    for n in NAMES:
        assert FX[n + ".bgr"].shape == FX[n + ".gray"].shape + (3,), n


@pytest.fixture(scope="module")
def regenerated():
    spec = importlib.util.spec_from_file_location("make_jpeg_layout_fixtures",
                                                  os.path.join(HERE, "golden", "make_jpeg_layout_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    files, refused = mod.files()
    assert sorted(refused) == sorted(REFUSED)
    return files


@pytest.mark.parametrize("name", NAMES + REFUSED)
def test_writer_reproduces_committed_bytes(regenerated, name):
    assert regenerated[name] == _jpg(name)


def test_writer_refuses_invalid_files():
    """What would make a file invalid is an assertion in the writer, not a broken file."""
    q, dc, ac = {0: np.ones(64, np.int64)}, {0: JW.K3_DC_LUMA}, {0: JW.K3_AC_LUMA}
    one = [JW.Component(1)]

    def blocks(**at):
        a = np.zeros((1, 1, 64), np.int16)
        for k, v in at.items():
            a[0, 0, int(k[1:])] = v
        return [a]
    assert JW.write_jpeg(8, 8, one, blocks(n0=2047, n1=1023), q, dc, ac)
    with pytest.raises(AssertionError, match="category 11"):
        JW.write_jpeg(8, 8, one, blocks(n0=2048), q, dc, ac)
    with pytest.raises(AssertionError, match="category 10"):
        JW.write_jpeg(8, 8, one, blocks(n1=-1024), q, dc, ac)
    with pytest.raises(AssertionError, match="has no symbol"):
        JW.write_jpeg(8, 8, one, blocks(n1=1), q, dc, {0: JW.huffman_from_stats({0x00: 1})})
    comps = [JW.Component(1, 4, 2), JW.Component(2, 2, 1), JW.Component(3, 1, 1)]
    with pytest.raises(AssertionError, match="10 blocks per MCU"):
        JW.write_jpeg(8, 8, comps, [np.zeros((c.v, c.h, 64), np.int16) for c in comps], q, dc, ac)
    with pytest.raises(AssertionError, match="code space"):
        JW.huffman_codes([2] + [0] * 15, [0, 1])


def test_statistics_tables_fit_sixteen_bits():
    """Fibonacci frequencies ask for codes far longer than 16 bits: Adjust_BITS folds them back, the
    table keeps every symbol and stays a prefix code with the all-ones code free."""
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    counts, symbols = JW.huffman_from_stats({s: f for s, f in enumerate(fib)})
    assert sorted(symbols) == list(range(40)) and counts[15] > 0
    codes = JW.huffman_codes(counts, symbols)
    assert codes[39][1] < codes[0][1] == 16
    assert JW.huffman_from_stats({7: 5}) == ([1] + [0] * 15, [7])


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_pillow(name, channels):
    got, want = oracle.jpeg_decode(_jpg(name), channels), FX[name + (".bgr" if channels == 3 else ".gray")]
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (name, len(bad), [(c, got[tuple(c)], want[tuple(c)]) for c in bad[:3].tolist()])


def test_oracle_four_components_on_encoder_made_files():
    """The oracle's four-component path (cmyk_440 above is its only layout fixture) also equals the
    records of tests/golden/jpeg_cmyk_fixtures.npz: CMYK, YCCK, progressive, restart intervals."""
    from tests.test_jpeg_cmyk import FOUR, FX as CMYK
    for name in FOUR:
        for channels, key in ((3, ".bgr"), (1, ".gray")):
            assert np.array_equal(oracle.jpeg_decode(CMYK[name + ".jpg"].tobytes(), channels), CMYK[name + key]), (name, channels)


@pytest.mark.parametrize("name", NAMES)
def test_host_paths_accept(name):
    b = _jpg(name)
    h, w = FX[name + ".gray"].shape
    assert A.jpeg_info(b) == (w, h, _ncomp(name))
    ew, eh, en, n_blocks, n_values = A.jpeg_entropy_decode(b)[:5]
    assert (ew, eh, en) == (w, h, _ncomp(name)) and n_blocks > 0 and (n_values > 0 or name == "huff_one_symbol")
    gpu_entropy, staged = A.jpeg_host_stage(b)
    assert bool(gpu_entropy) == (name not in HOST_ENTROPY) and staged > 0


@pytest.mark.parametrize("name", REFUSED)
def test_refused_files_stay_refused(name):
    """A file libjpeg refuses is refused by every entry, with an error and not a decode or a crash."""
    b = _jpg(name)
    for fn in (A.jpeg_entropy_decode, A.jpeg_host_stage):
        with pytest.raises(A.AeonHipError, match="fractional sampling"):
            fn(b)
    for cn in (3, 1):
        with pytest.raises(RuntimeError, match="fractional sampling"):
            oracle.jpeg_decode(b, cn)


def test_gpu_entropy_emulation_matches_host_decoder(tmp_path):
    """The stand-alone driver (tests/sanitize/fuzz_driver.cpp under ASan + UBSan, a program of its own)
    on the new files, as tests/test_jpeg_cmyk.py runs it: jpeg_huff's phases on the host at 1,024, 512
    and 256 lanes, "gpu ok <hash>" only when all three agree, and that hash the host entropy
    decoder's.  The two restart-interval-1 files have more subsequences than lanes (the strided
    phases, one tiny segment per subsequence); tab_three stays with the host decoder."""
    if not os.path.exists("/opt/rocm/llvm/bin/clang++"):
        pytest.skip("no clang with sanitizer runtimes")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize"])
    for k in NAMES + REFUSED:
        (tmp_path / (k + ".jpg")).write_bytes(_jpg(k))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([DRIVER] + [str(tmp_path / (k + ".jpg")) for k in NAMES + REFUSED], capture_output=True,
                       text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    results, gpu = _parse(r.stdout)
    for k in NAMES:
        host, g = results[k + ".jpg"], gpu[k + ".jpg"]
        assert host.startswith("ok"), (k, host)
        if k in HOST_ENTROPY:
            assert g == "gpu host", (k, g)
        else:
            assert g.startswith("gpu ok") and host.split("hash ")[1] == g.split()[2], (k, host, g)
    for k in REFUSED:
        assert results[k + ".jpg"].startswith("error") and "fractional sampling" in results[k + ".jpg"], results[k + ".jpg"]
