"""GPU: RLE8 / RLE4 and 16-bit BMP files through the opt-in call (aeon_hip_decode_pixmap_packed_batch: bmp_rle_expand,
one wave per RLE file, then pixmap_convert) against the painted token lists and numpy shifts of
tests/bmp_packed_cases.py, bit for bit, in guard-filled, row-padded records.
"""
import numpy as np
import pytest

import aeon_amd as A
from tests import bmp_packed_cases as C
from tests import pixmap_writer as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def _decode(ctx, exp, sync=True):
    """One packed call over exp's files: the records and every guard byte around them checked against exp; with
    sync=False the call is only enqueued and the check is returned for after the synchronize."""
    import torch
    descs, off = [], 3
    for i, (_, f, m, want) in enumerate(exp):
        h, w, cn = want.shape[0], want.shape[1], want.shape[2] if want.ndim == 3 else 1
        descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=w * cn + 5 + i % 3, channels=cn, elem_bytes=1))
        off += descs[-1].stride * h + 7 + 2 * (i % 4)
    dst = torch.full((off + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.decode_pixmap_batch([e[1] for e in exp], [e[2] for e in exp], descs, dst.data_ptr(), stream, packed=True)

    def check(skip=()):
        host, end = dst.cpu().numpy(), 0
        for d, (name, _, m, want) in zip(descs, exp):
            rows = host[d.offset:d.offset + d.stride * d.height].reshape(d.height, d.stride)
            rowb = want[0].size
            assert np.all(host[end:d.offset] == 0x5A), (name, "bytes written between records")
            assert np.all(rows[:, rowb:] == 0x5A), (name, "bytes written past a row")
            if name not in skip:  # (a corrupt file's record is unspecified)
                assert np.array_equal(rows[:, :rowb].reshape(want.shape), want), (name, m)
            end = d.offset + d.stride * d.height
        assert np.all(host[end:] == 0x5A), "bytes written past the last record"

    if not sync:
        return check
    ctx.synchronize(stream)
    check()


def _plain():
    a = (np.arange(5 * 7 * 3) % 251).astype(np.uint8).reshape(5, 7, 3)
    return [("bmp24", W.bmp(a, 24), A.DECODE_BGR8, a), ("p5", W.pnm(5, a[:, :, 0], 255), A.DECODE_GRAY8, a[:, :, 0])]


def test_the_whole_table_and_two_plain_files_in_one_call(ctx):
    exp = C.good() + _plain()
    for name, f, _, _ in C.good():
        assert A.pixmap_packed_route(f), (name, "not routed to the device")
    for _ in range(2):  # the second staging set too
        _decode(ctx, exp)


@pytest.mark.parametrize("case", C.corrupt(), ids=lambda c: c[0])
def test_a_corrupt_file_sets_the_device_error_and_spares_the_others(ctx, case):
    import torch
    name, f = case
    w, h = A.pixmap_info(f, packed=True)[:2]
    good = C.good()[:12] + _plain()
    exp = good[:5] + [(name, f, A.DECODE_GRAY8, np.zeros((h, w), np.uint8))] + good[5:]
    check = _decode(ctx, exp, sync=False)
    with pytest.raises(A.AeonHipError) as e:
        ctx.synchronize(torch.cuda.current_stream().cuda_stream)
    assert e.value.code == A.AEON_HIP_EDEVICE and "BMP RLE" in str(e.value), str(e.value)
    check(skip=(name,))
    _decode(ctx, good)  # the context is usable, the next call decodes right
