"""GPU: jpeg_huff on each of its three paths -- staged lanes, unstaged lanes, strided -- at 256, 512 and 1,024 lanes,
with the files of tests/jpeg_huff_cases.py: files that never re-synchronise (one subsequence settles per Jacobi
round, up to a thousand rounds), dense files (50 to several hundred rounds), four-component files whose fourth
DC sum crosses the chunks of the prefix scan, sparse blocks among dense ones, blocks longer than six subsequences.

Per lane count the test first asserts, with the stage cap queried from the device, that the list holds files on
every path.  Every record is compared bit for bit with oracle.jpeg_decode (which also pins IDCT, upsampling and
colour) and with a context whose entropy decoding runs on the host (AEON_HIP_JPEG_HUFF=host: the same kernels
after it, so a difference is jpeg_huff's).  Rows are padded and the buffer pre-filled, so a store outside a record
shows.  tests/test_jpeg_huff_cases.py asserts, without a device, what makes each file a test of its path.
"""

import numpy as np
import pytest

import aeon_amd as A
from tests import jpeg_huff_cases as HC
from tests.test_hip_jpeg_layouts import OLD, _context, _sha

pytestmark = pytest.mark.gpu

CASES = HC.cases()
FILL = 0x5A


def _decode(ctx, files, channels):
    """One decode_jpeg_batch call: the records as arrays.  Rows are padded (stride > width), records are apart
    and the buffer is pre-filled: every byte outside the records' rows must keep the fill."""
    import torch
    descs, off = [], 0
    for i, b in enumerate(files):
        w, h, _ = A.jpeg_info(b)
        stride = w * channels + 5 + i % 3
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=stride, channels=channels))
        off += (stride * h + 15) // 16 * 16 + (2 if i % 2 else 0) * 16
    dst = torch.full((max(off, 16),), FILL, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_jpeg_batch(files, descs, dst.data_ptr(), stream)
    ctx.synchronize(stream)
    host = dst.cpu().numpy()
    out = []
    for d in descs:
        rows = host[d.offset:d.offset + d.stride * d.height].reshape(d.height, d.stride)
        a = np.ascontiguousarray(rows[:, :d.width * channels])
        out.append(a.reshape(d.height, d.width, 3) if channels == 3 else a)
        rows[:, :d.width * channels] = FILL
    assert np.all(host == FILL), ("bytes written outside the records", np.flatnonzero(host != FILL)[:3].tolist())
    return out


@pytest.fixture(scope="module")
def contexts():
    ctxs = {n: _context(AEON_HIP_JPEG_HUFF_LANES=str(n)) for n in HC.LANES}
    ctxs["host"] = _context(AEON_HIP_JPEG_HUFF="host")
    for n in HC.LANES:  # the flag took effect: the lane count is the context's, read when it was created
        assert ctxs[n].jpeg_huff_lanes() == n
    assert ctxs["host"].jpeg_huff_lanes() == HC.limits()["default_lanes"]
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope="module")
def caps(contexts):
    return {n: A.jpeg_huff_stage_cap(n) for n in HC.LANES}


@pytest.fixture(scope="module")
def host_records(contexts):
    """Every case through the host entropy decoder's context, once per channel count."""
    return {cn: _decode(contexts["host"], [c.data for c in CASES], cn) for cn in (3, 1)}


def _differences(got, want):
    bad = np.argwhere(got != want)
    return len(bad), [(c, int(got[tuple(c)]), int(want[tuple(c)])) for c in bad[:3].tolist()]


@pytest.mark.parametrize("lanes", HC.LANES)
def test_every_path_is_covered(caps, lanes):
    """With the cap jpeg_huff<lanes> has on this device: at least one staged, one unstaged-lanes and one strided
    file whose segments hold many subsequences; and every case is on the path it is meant for."""
    cap = caps[lanes]
    assert 0 < cap <= HC.limits()["stage_max"] and cap % 16 == 0, cap
    paths = {c.name: HC.path_of(c.data, lanes, cap) for c in CASES}
    for path in (HC.STAGED, HC.UNSTAGED, HC.STRIDED):
        assert [n for n, p in paths.items() if p == path], (lanes, cap, path, paths)
    multi = [c.name for c in CASES if paths[c.name] == HC.STRIDED and A.jpeg_huff_layout(c.data, lanes)["seg_max"] > lanes // 2]
    assert multi, (lanes, paths)
    for c in CASES:
        if lanes in c.meant:
            assert paths[c.name] == c.meant[lanes], (c.name, lanes, cap, A.jpeg_huff_layout(c.data, lanes))


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("lanes", HC.LANES)
def test_records_equal_the_oracle_and_the_host_entropy_decoder(contexts, caps, host_records, lanes, channels):
    res = _decode(contexts[lanes], [c.data for c in CASES], channels)
    failures = []
    for c, r, h in zip(CASES, res, host_records[channels]):
        want = HC.reference(c.name, channels)
        assert r.shape == want.shape == h.shape, c.name
        for ref, what in ((want, "oracle"), (h, "host entropy")):
            n, first = _differences(r, ref)
            if n:
                failures.append((c.name, HC.path_of(c.data, lanes, caps[lanes]), what, n, first))
    assert not failures, failures


def test_host_entropy_context_equals_the_oracle(host_records):
    """The second reference itself: the host decoder's records are the oracle's."""
    for cn in (3, 1):
        for c, h in zip(CASES, host_records[cn]):
            n, first = _differences(h, HC.reference(c.name, cn))
            assert n == 0, (c.name, cn, n, first)


# one call holding the three paths at each lane count, in an order that is not by size: a staged file, a strided
# one, the smallest, an unstaged one, the largest, ...
MIXED = ["ns_staged512", "dense_420_s512", "long_blocks", "dense_420_u256", "dense_444_s1024", "ns_staged256",
         "ns_strided256", "dense_cmyk_s256", "sparse_444", "dense_gray_s256", "ns_restart", "dense_cmyk_s512"]


@pytest.mark.parametrize("lanes", HC.LANES)
def test_mixed_call_twice(contexts, caps, lanes):
    """The size-class sort of the Huffman workgroups and the one dynamic LDS size of the launch (the largest file
    that fits the cap) with every path in the call; the second call equals the first."""
    by = HC.by_name()
    files = [by[n].data for n in MIXED]
    sizes = [len(f) for f in files]
    assert sizes != sorted(sizes) and sizes != sorted(sizes, reverse=True)
    assert {HC.path_of(f, lanes, caps[lanes]) for f in files} == {HC.STAGED, HC.UNSTAGED, HC.STRIDED}
    first = _decode(contexts[lanes], files, 3)
    for n, r in zip(MIXED, first):
        cnt, where = _differences(r, HC.reference(n, 3))
        assert cnt == 0, (n, HC.path_of(by[n].data, lanes, caps[lanes]), cnt, where)
    for n, a, b in zip(MIXED, first, _decode(contexts[lanes], files, 3)):
        assert np.array_equal(a, b), ("second call", n)


@pytest.mark.parametrize("lanes", HC.LANES)
def test_worst_case_is_still_an_answer(contexts, lanes):
    """After the files that take a round per subsequence the context goes on: the next batch is right."""
    ns = [c for c in CASES if c.family == "never_sync"]
    for c, r in zip(ns, _decode(contexts[lanes], [c.data for c in ns], 1)):
        cnt, where = _differences(r, HC.reference(c.name, 1))
        assert cnt == 0, (c.name, lanes, cnt, where)
    for cn, key in ((3, ".bgr"), (1, ".gray")):
        (r,) = _decode(contexts[lanes], [OLD["s420_q50.jpg"].tobytes()], cn)
        assert np.array_equal(_sha(r), OLD["s420_q50" + key]), (lanes, cn)
