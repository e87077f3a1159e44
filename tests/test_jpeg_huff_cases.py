"""CPU: the files of tests/jpeg_huff_cases.py are what the GPU tests take them for.

The stand-alone driver (tests/sanitize/fuzz_driver.cpp under ASan + UBSan, a program of its own) runs jpeg_huff's
phases on the host at 1,024, 512 and 256 lanes over every file: the host entropy decoder's coefficients each time.
Its --lanes line gives the Jacobi rounds and the subsequence layout per lane count, and the conditions that make
a file a test of its path are asserted on them here, so that tests/test_hip_jpeg_huff_paths.py cannot quietly test
less: never_sync files settle one subsequence per round, dense files take 50 rounds and more, a strided file has
more subsequences than lanes and a segment of more than half the lanes, the restart file has a segment that runs
from one chunk of the prefix scan into the next, the long-blocks file has subsequences that start no block.
"""
import os
import subprocess

import numpy as np
import pytest

import aeon_amd as A
from tests import jpeg_huff_cases as HC
from tests import jpeg_writer as JW
from tests.test_jpeg_cmyk import DRIVER, _parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in HC.cases()]


def _parse_lanes(text):
    """{lanes: dict(rounds, nsub, sub_bits, segs)} of a --lanes line's third field."""
    out = {}
    for part in text.split("; "):
        w = part.split()
        assert w[0] == "lanes" and w[2] == "rounds" and w[4] == "nsub" and w[6] == "sub_bits" and w[8] == "segs", part
        out[int(w[1])] = dict(rounds=int(w[3]), nsub=int(w[5]), sub_bits=int(w[7]), segs=[int(x) for x in w[9].split(",")])
    return out


@pytest.fixture(scope="module")
def driver_run(tmp_path_factory):
    if not os.path.exists("/opt/rocm/llvm/bin/clang++"):
        pytest.skip("no clang with sanitizer runtimes")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "aeon_amd", "csrc"), "sanitize"])
    d = tmp_path_factory.mktemp("huff_cases")
    for c in HC.cases():
        (d / (c.name + ".jpg")).write_bytes(c.data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([DRIVER, "--lanes"] + [str(d / (n + ".jpg")) for n in NAMES], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    results, gpu = _parse("\n".join(x for x in lines if not x.startswith("lanes\t")))
    lanes = {}
    for x in lines:
        if x.startswith("lanes\t"):
            _, path, res = x.split("\t")
            lanes[os.path.basename(path)[:-4]] = _parse_lanes(res)
    return results, gpu, lanes


def test_names_are_unique_and_every_family_is_there():
    assert len(set(NAMES)) == len(NAMES)
    assert {c.family for c in HC.cases()} == {"never_sync", "dense", "four", "sparse", "long"}
    for c in HC.cases():
        assert c.meant and set(c.meant) <= set(HC.LANES), c.name
    # per lane count a file meant for each path (the GPU test asserts the paths actually taken)
    for n in HC.LANES:
        assert {c.meant.get(n) for c in HC.cases()} >= {HC.STAGED, HC.UNSTAGED, HC.STRIDED}, n


@pytest.mark.parametrize("name", NAMES)
def test_emulation_gives_the_host_decoders_coefficients(driver_run, name):
    """"gpu ok" is printed only when 1,024, 512 and 256 lanes agree; the hash is the host decoder's."""
    results, gpu, lanes = driver_run
    host, g = results[name + ".jpg"], gpu[name + ".jpg"]
    assert host.startswith("ok"), (name, host)
    assert g.startswith("gpu ok") and host.split("hash ")[1] == g.split()[2], (name, host, g)
    assert sorted(lanes[name]) == sorted(HC.LANES)
    assert int(host.split("blocks ")[1].split()[0]) == HC.by_name()[name].blocks


@pytest.mark.parametrize("name", NAMES)
def test_layout_entry_agrees_with_the_driver(driver_run, name):
    """aeon_jpeg_huff_layout through the shipped library against the driver's own call of prepare_gpu."""
    data = HC.by_name()[name].data
    for n in HC.LANES:
        lay, drv = A.jpeg_huff_layout(data, n), driver_run[2][name][n]
        assert lay["gpu_entropy"] and A.jpeg_host_stage(data)[0]
        assert (lay["nsub"], lay["sub_bits"], lay["seg_nsub"]) == (drv["nsub"], drv["sub_bits"], drv["segs"]), (name, n)
        assert lay["nseg"] == len(lay["seg_nsub"]) and lay["seg_max"] == max(lay["seg_nsub"]) and sum(lay["seg_nsub"]) == lay["nsub"]
        assert HC.limits()["sub_min"] <= lay["sub_bits"] <= HC.limits()["sub_max"] and lay["sub_bits"] % 32 == 0
        assert lay["data_bytes"] % 4 == 0 and 0 < lay["data_bytes"] < len(data)
    with pytest.raises(A.AeonHipError):
        A.jpeg_huff_layout(data, 128)


def test_layout_entry_on_a_host_decoded_file():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_fixtures.npz"))
    prog = next(k for k in sorted(fx.files) if k.startswith("prog_") and k.endswith(".jpg"))
    lay = A.jpeg_huff_layout(fx[prog].tobytes(), 512)
    assert not lay["gpu_entropy"] and lay["nsub"] == 0 and lay["seg_nsub"] == []
    assert HC.limits()["default_lanes"] == 512


@pytest.mark.parametrize("name", NAMES)
def test_conditions_that_keep_the_files_honest(driver_run, name):
    c = HC.by_name()[name]
    for n, path in c.meant.items():
        d = driver_run[2][name][n]
        what = (name, n, path, d)
        if path == HC.STRIDED:
            assert d["nsub"] > n and max(d["segs"]) > n // 2, what
            assert d["sub_bits"] == HC.limits()["sub_max"], what
        else:
            assert d["nsub"] <= n, what
        if c.family == "never_sync":
            assert d["rounds"] >= max(d["segs"]) - 2, what
            assert d["sub_bits"] > HC.limits()["sub_min"], what  # (at sub_min the lead-in makes it nsub - 3)
        if c.family == "dense" and path != HC.STAGED:
            assert d["rounds"] >= 50, what
        if c.family == "long":
            assert d["sub_bits"] == HC.limits()["sub_min"] and c.blocks < d["nsub"] // 4, what


def test_never_sync_files_settle_one_subsequence_a_round_at_every_lane_count(driver_run):
    """Also where a file is not meant for a path: the rounds are the largest segment's subsequences less the
    starts that are exact before any round (the first, and those whose lead-in reaches back to it: two at sub_min)."""
    for c in HC.cases():
        if c.family == "never_sync":
            for n in HC.LANES:
                d = driver_run[2][c.name][n]
                assert max(d["segs"]) - 3 <= d["rounds"] <= max(d["segs"]) - 1, (c.name, n, d)


def test_never_sync_staged_file_fills_the_lanes(driver_run):
    """nsub close to the lane count on the staged path: within 5 % at 256 and at 512 lanes."""
    for n in (256, 512):
        d = driver_run[2][f"ns_staged{n}"][n]
        assert 0.95 * n <= d["nsub"] <= n, (n, d)


def test_restart_file_has_a_segment_across_two_scan_chunks(driver_run):
    """A segment whose first and last subsequence lie in different chunks of `lanes` subsequences (wg_scan's
    carry enters its DC predictors and block numbers), at each lane count where the file is strided; two to
    four segments, the long ones of a few hundred subsequences."""
    c = HC.by_name()["ns_restart"]
    for n, path in c.meant.items():
        if path != HC.STRIDED:
            continue
        segs, first, straddle = driver_run[2]["ns_restart"][n]["segs"], 0, []
        for s in segs:
            if first // n != (first + s - 1) // n and first % n:
                straddle.append((first, s))
            first += s
        assert straddle, (n, segs)
        assert 2 <= len(segs) <= 4 and sum(s >= 200 for s in segs) >= 2, (n, segs)


def test_sparse_file_block_counts_differ_fiftyfold_and_more():
    """Blocks started per subsequence, from the code lengths of the sparse half (DC code, difference bits, EOB):
    the sparse blocks fill four subsequences and more of 2,048 bits at 50 blocks and more each, while a dense
    block takes 1,000 bits and more, so a dense subsequence starts three at the most."""
    data, comps, coefs, row = HC.sparse_parts()
    lay = A.jpeg_huff_layout(data, 512)
    dcs = {0: JW.huffman_codes(*JW.K3_DC_LUMA), 1: JW.huffman_codes(*JW.K3_DC_CHROMA)}
    eob = {0: JW.huffman_codes(*JW.K3_AC_LUMA)[0][1], 1: JW.huffman_codes(*JW.K3_AC_CHROMA)[0][1]}
    sparse_bits = sparse_blocks = dense_blocks = 0
    for c, cf in zip(comps, coefs):
        dc = cf[:, :, 0].astype(np.int64).reshape(-1)  # 4:4:4: a component's scan order is its row-major order
        first = row * cf.shape[1]
        assert not cf[row:, :, 1:].any() and np.count_nonzero(cf[:row, :, 1:]) > 62 * first
        for d in np.diff(dc, prepend=0)[first:]:
            size = JW.category(d)
            sparse_bits += dcs[c.td][size][1] + size + eob[c.ta]
        sparse_blocks += len(dc) - first
        dense_blocks += first
    assert sparse_blocks + dense_blocks == HC.by_name()["sparse_444"].blocks and 2 * dense_blocks >= sparse_blocks
    dense_bits = lay["data_bytes"] * 8 - sparse_bits - 8 * 20  # (less the padding of the staged data)
    assert lay["nsub"] > 512 and lay["sub_bits"] == 2048
    assert sparse_bits >= 4 * 2048 and sparse_blocks / (sparse_bits / 2048 + 1) >= 50, (sparse_bits, sparse_blocks)
    assert dense_bits / dense_blocks >= 1000, (dense_bits, dense_blocks)
    assert dense_bits > HC.strided_above(512) * 8


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_decodes_every_file(name, channels):
    c = HC.by_name()[name]
    w, h, ncomp = A.jpeg_info(c.data)
    got = HC.reference(name, channels)
    assert got.dtype == np.uint8 and got.shape == ((h, w, 3) if channels == 3 else (h, w))
    assert ncomp == (4 if c.family == "four" else 1 if "gray" in name or c.family in ("never_sync", "long") else 3)
    assert got.min() < got.max(), name
    if ncomp == 1 and channels == 3:
        assert np.array_equal(got, np.repeat(HC.reference(name, 1)[:, :, None], 3, axis=2))
