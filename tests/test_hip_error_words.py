"""GPU: the per-stream device error words (context.hpp stream_error / release_stream_error, aeon_hip_synchronize and
aeon_hip_release_stream) with more than one stream.  An error word is a flag a kernel sets for input it refuses,
not a GPU fault: the only bad input here is tests/png_cases.py's "adler" file (24x16, a wrong Adler-32 trailer),
which the PNG stage decodes to the end and then refuses; the good files are filter_files()[3:6].

A context has 63 words besides the null stream's, so the tests that hand words back need more than 63 distinct
streams alive at once.  torch.cuda.Stream() deals from a pool of 32 handles, so those streams are made with
hipStreamCreateWithFlags on torch's own runtime and wrapped as torch.cuda.ExternalStream: torch streams as far as
torch's synchronize goes, each with a handle of its own."""
import ctypes
import os

import numpy as np
import pytest

import aeon_amd as A
from oracle import png_oracle as PO
from tests import png_cases as PC

pytestmark = pytest.mark.gpu

EDEVICE = -4
K_ERR_WORDS = 64  # aeon_hip_ctx::kErrWords


@pytest.fixture
def ctx():  # one per test: every word of its table is free
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files():
    name, bad = PC.corrupt_files()[0]
    assert name == "adler" and A.png_info(bad)[:2] == (24, 16)
    good = [png for _, png in PC.filter_files()[3:6]]
    for png in [bad] + good:
        assert A.png_host_stage(png, A.PNG_ANYDEPTH)[0], "not routed to the device"
    return bad, good, [PO.decode(png, PO.ANYDEPTH) for png in good]


class RawStreams:
    """n streams of their own (hipStreamCreateWithFlags, non-blocking) as torch ExternalStreams; destroyed by
    close()."""

    def __init__(self, n):
        import torch
        self.hip = ctypes.CDLL(os.path.join(torch.__path__[0], "lib", "libamdhip64.so"))
        self.hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
        self.hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        self.handles, self.streams = [], []
        for _ in range(n):
            h = ctypes.c_void_p()
            assert self.hip.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0  # hipStreamNonBlocking
            self.handles.append(h.value)
            self.streams.append(torch.cuda.ExternalStream(h.value))
        assert len(set(self.handles)) == n

    def close(self):
        self.streams = []
        for h in self.handles:
            self.hip.hipStreamDestroy(ctypes.c_void_p(h))
        self.handles = []


class Decode:
    """One decode_png_batch of `pngs` (ANYDEPTH) queued on `stream` (a raw handle); the output buffer was made
    and filled before anything was queued (prepare), so no other stream orders it."""

    def __init__(self, pngs):
        import torch
        self.pngs, self.descs, self.shapes, off = pngs, [], [], 0
        for b in pngs:
            w, h, d, c = A.png_info(b)
            eb = 2 if (d == 16 and c != 3) else 1
            self.descs.append(A.ImgDesc(offset=off, width=w, height=h, stride=w * eb, channels=1, elem_bytes=eb))
            self.shapes.append((h, w, eb))
            off += (w * eb * h + 15) // 16 * 16
        self.dst = torch.full((max(off, 16),), 0x5A, dtype=torch.uint8, device="cuda")

    def queue(self, ctx, stream):
        ctx.decode_png_batch(self.pngs, [A.PNG_ANYDEPTH] * len(self.pngs), self.descs, self.dst.data_ptr(), stream)

    def check(self, want):
        host = self.dst.cpu().numpy()
        for k, (d, (h, w, eb), ref) in enumerate(zip(self.descs, self.shapes, want)):
            a = host[d.offset:d.offset + w * eb * h]
            a = (a.view(np.uint16) if eb == 2 else a).reshape(h, w)
            assert a.dtype == ref.dtype and np.array_equal(a, ref.reshape(h, w)), k


def _raises_edevice(ctx, stream):
    with pytest.raises(A.AeonHipError) as e:
        ctx.synchronize(stream)
    assert e.value.code == EDEVICE and "PNG" in str(e.value), str(e.value)


@pytest.mark.parametrize("order", ["sync_good_first", "sync_bad_first"])
def test_error_stays_on_its_stream(ctx, files, order):
    import torch
    bad, good, want = files
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = sa.cuda_stream, sb.cuda_stream
    assert a != b
    da, db, da2 = Decode([bad]), Decode(good), Decode(good)
    torch.cuda.synchronize()
    da.queue(ctx, a)  # both queued before either is synchronized
    db.queue(ctx, b)
    if order == "sync_bad_first":
        _raises_edevice(ctx, a)
    ctx.synchronize(b)  # clean: A's bit is not B's
    db.check(want)
    if order == "sync_good_first":
        _raises_edevice(ctx, a)
    ctx.synchronize(a)  # reported exactly once
    ctx.synchronize(b)
    da2.queue(ctx, a)  # A decodes good files afterwards
    ctx.synchronize(a)
    da2.check(want)


def test_words_are_handed_back_by_release_stream(ctx, files):
    """70 streams, each used once, completed by torch and given up with aeon_hip_release_stream while it stays
    alive: with the words handed back, two fresh streams still get one each.  (When release kept them, streams 64
    to 70 and both fresh ones shared the null stream's word, and Y reported X's error.)"""
    import torch
    bad, good, want = files
    n = 70
    assert n > K_ERR_WORDS
    rs = RawStreams(n + 2)
    try:
        used = [Decode(good[:1]) for _ in range(n)]
        dx, dy = Decode([bad]), Decode(good)
        torch.cuda.synchronize()
        for d, h, s in zip(used, rs.handles, rs.streams):
            d.queue(ctx, h)
            s.synchronize()  # torch's own stream synchronize
            ctx.release_stream(h)
        for d in used:
            d.check(want[:1])
        (x, y), (sx, _) = rs.handles[n:], rs.streams[n:]
        dx.queue(ctx, x)
        dy.queue(ctx, y)
        sx.synchronize()  # X is complete (and its bit set) before Y's word is read
        ctx.synchronize(y)  # clean
        dy.check(want)
        _raises_edevice(ctx, x)
        ctx.synchronize(x)
    finally:
        torch.cuda.synchronize()
        rs.close()


def test_released_word_carries_no_old_bits(ctx, files):
    """A stream's refused file, never read: the stream is completed by torch and released.  63 fresh streams --
    every word of the table, the released one among them -- then decode good files and are synchronized through
    the ABI: none of them reports the old bit."""
    import torch
    bad, good, want = files
    rs = RawStreams(K_ERR_WORDS)
    try:
        dbad = Decode([bad])
        fresh = [Decode(good[:1]) for _ in range(K_ERR_WORDS - 1)]
        torch.cuda.synchronize()
        dbad.queue(ctx, rs.handles[0])
        rs.streams[0].synchronize()
        ctx.release_stream(rs.handles[0])  # without aeon_hip_synchronize
        for d, h in zip(fresh, rs.handles[1:]):  # all of them hold a word before the first is handed back
            d.queue(ctx, h)
        for d, h in zip(fresh, rs.handles[1:]):
            ctx.synchronize(h)
            d.check(want[:1])
    finally:
        torch.cuda.synchronize()
        rs.close()
