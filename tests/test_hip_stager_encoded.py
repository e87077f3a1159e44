"""GPU: the stager from encoded records (aeon_hip_stager_stage_encoded, stager_encoded.cpp): provide() hands over the
record's file, the window's launch decodes it on the device with the stage of its format -- or, where the decoder's
routing rule keeps a file off the device, the calling thread decodes it into the window's pinned staging -- and the
augment / mask launches read the decoded slots.  Every comparison is bit for bit against the reference decode
(oracle.jpeg_decode, the library's host decoders of the other formats) followed by the oracle's transform + load;
outputs go into buffers filled with 0xA5 with guard bytes past every item.  Which route a file takes is asked
(encoded_info), which path a window took is read back (last_launch / last_decode).
"""
import ctypes
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import aeon_amd as A
from aeon_amd import configs as C
from tests import helpers as H
from tests import stager_encoded_cases as SC
from tests.buffers import Buffer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, EDEVICE = -1, -4
BATCH, NBATCHES = 4, 2
OUT_W, OUT_H = 32, 24
GUARD = 64
FILL = 0xA5
SEED = 5
ETL = {"type": "image", "height": OUT_H, "width": OUT_W, "channels": 3, "output_type": "float", "channel_major": True,
       "bgr_to_rgb": True}
ITEM = 3 * OUT_H * OUT_W * 4
NAMES = A.FORMAT_NAMES


def _out():
    """float32 CHW, standardized, with GUARD bytes between the items."""
    return C.out_desc_for(ETL, C.C2_AUG, item_stride=ITEM + GUARD)


def _params():
    """C2 crop + flip draws for SIZES, the ones a Decoder with random_seed = SEED draws for the same records."""
    params = H.draw_params(C.C2_AUG, SC.SIZES, OUT_W, OUT_H, seed=SEED)
    assert any(p.flip for p in params) and any(p.crop_w < w for p, (w, _) in zip(params, SC.SIZES))
    return params


class Guarded(Buffer):
    """A batch buffer pre-filled with FILL, so that an item the stager did not write, or wrote past, shows."""

    def __init__(self, nbytes, where):
        super().__init__(nbytes + GUARD, where)  # (and GUARD bytes past the last item's stride)
        self.refill()

    def refill(self):
        if self.where == "device":
            import torch
            self.t.fill_(FILL)
            torch.cuda.synchronize()  # (the stager's streams do not wait for torch's)
        elif self.where == "pinned":
            ctypes.memset(self.ptr, FILL, self.n)
        else:
            self.a[:] = FILL

    def items(self, n, stride, nbytes):
        """The n items' bytes, after checking the guard bytes behind each.  A pageable batch is the exception the
        stager has always made: its wait copies the batch out of device memory in one piece, item strides whole, so
        there only the bytes past the batch are guarded."""
        flat = np.array(self.bytes()).reshape(-1)
        assert (flat[n * stride:] == FILL).all(), "bytes past the batch were written"
        raw = flat[:n * stride].reshape(n, stride)
        if self.where != "pageable":
            assert (raw[:, nbytes:] == FILL).all(), "guard bytes past an item were written"
        return raw[:, :nbytes]


def _reference(decoded, params, out, mask=False):
    return [r.reshape(-1).view(np.uint8) if r.dtype == np.uint8 else np.ascontiguousarray(r).reshape(-1).view(np.uint8)
            for r in H.oracle_records(list(decoded), params, out, mask=mask)]


def _assert_items(items, want, what):
    for i, w in enumerate(want):
        assert items[i].size == w.size and np.array_equal(items[i], w), (what, i, int((items[i] != w).sum()))


def _expected_counts(files, mask=False):
    dev, host = dict.fromkeys(NAMES, 0), dict.fromkeys(NAMES, 0)
    for f in files:
        info = A.encoded_info(f, mask)
        (dev if info["device_route"] else host)[NAMES[info["format"]]] += 1
    return dev, host


def _stage_window(st, bufs, files, params, order=None, threads=4):
    """provide() of every record from a pool: record i is idx i % BATCH of batch i // BATCH.  files[i]: bytes (encoded)
    or an array (decoded pixels)."""
    def one(i):
        f = files[i]
        stage = st.stage_encoded if isinstance(f, bytes) else st.stage
        stage(bufs[i // BATCH].ptr, i % BATCH, f, params[i])
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, order if order is not None else range(len(files))))


@pytest.fixture(scope="module")
def ctx():
    c = A.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def params():
    return _params()


def _window_reference(win, params, out):
    return _reference(SC.window_decoded(win), params, out)


def test_all_formats_in_one_window(ctx, params):
    """Eight records, one of every format, in 2 batches: each file on the route it is meant for, every record equal to
    decode + oracle, and last_decode reporting where each was decoded."""
    files = SC.window(0)
    for (kind, fmt, route), f in zip(SC.IMAGE_KINDS, files):
        info = A.encoded_info(f)
        assert (info["format"], info["device_route"]) == (fmt, route), (kind, info)
    assert not A.jpeg_host_stage(files[2])[0] and A.jpeg_host_stage(files[0])[0]  # progressive: the stage's host pool
    out = _out()
    st = A.Stager(ctx, out, BATCH)
    bufs = [Guarded(BATCH * out.item_stride, "pinned") for _ in range(NBATCHES)]
    try:
        _stage_window(st, bufs, files, params)
        for b in bufs:
            st.flush(b.ptr)
        want = _window_reference(0, params, out)
        for k, b in enumerate(bufs):
            _assert_items(b.items(BATCH, out.item_stride, ITEM), want[k * BATCH:(k + 1) * BATCH], ("batch", k))
        assert st.last_launch() == dict(launches=1, src_zero_copy=0, out_direct=1, chunks=1, records=8)
        assert st.last_decode() == dict(launches=1, device=dict(jpeg=3, png=1, pixmap=2, tiff=1),
                                        host=dict(jpeg=0, png=1, pixmap=0, tiff=0), pixels=0)
    finally:
        st.close()
        for b in bufs:
            b.free()


def test_same_records_other_front_doors(ctx, params):
    """The records of the window above through Decoder.decode (the project's own front door, which draws the same
    params from the same seed) and through Stager.stage of the decoded pixels: the same bytes as stage_encoded."""
    files, decoded = SC.window(0), SC.window_decoded(0)
    out = _out()
    got = {}
    for name, recs in (("encoded", files), ("pixels", decoded)):
        st = A.Stager(ctx, out, BATCH)
        bufs = [Guarded(BATCH * out.item_stride, "pageable") for _ in range(NBATCHES)]
        try:
            _stage_window(st, bufs, recs, params)
            for b in bufs:
                st.flush(b.ptr)
            got[name] = np.concatenate([b.items(BATCH, out.item_stride, ITEM) for b in bufs])
            assert st.last_decode()["pixels"] == (8 if name == "pixels" else 0)
        finally:
            st.close()
    d = A.Decoder(dict(batch_size=8, random_seed=SEED, etl=[ETL], augmentation=[C.C2_AUG]))
    (dec,) = d.decode([(f,) for f in files])
    d.close()
    got["decoder"] = np.ascontiguousarray(dec).reshape(8, -1).view(np.uint8)
    assert np.array_equal(got["encoded"], got["pixels"])
    assert np.array_equal(got["encoded"], got["decoder"])
    _assert_items(got["encoded"], _window_reference(0, params, out), "oracle")


def _mask16_reference(m, p, out):
    """saturate_cast<uchar> of the 16-bit NEAREST result (the mask path's uint8 load of a uint16 record)."""
    if m.dtype != np.uint16:
        return H.oracle_records([m], [p], out, mask=True)[0]
    lo = H.oracle_records([(m & 0xff).astype(np.uint8)], [p], out, mask=True)[0]
    hi = H.oracle_records([(m >> 8).astype(np.uint8)], [p], out, mask=True)[0]
    return np.minimum(hi.astype(np.uint32) * 256 + lo, 255).astype(np.uint8)


def test_mask_stager(ctx, params):
    """ANYDEPTH on a mask stager: a 16-bit PNG, a 16-bit gray TIFF and an 8-bit palette PNG staged encoded next to a
    decoded mask; a JPEG file is refused with the decoder's message, and its idx takes another record."""
    files = [SC.mask_file(kind, 40 + i, *SC.SIZES[i]) for i, kind in enumerate(SC.MASK_KINDS)]
    infos = [A.encoded_info(f, mask=True) for f in files]
    assert [i["elem_bytes"] for i in infos] == [2, 2, 1], infos
    decoded = [SC.decode_mask(f) for f in files]
    assert [d.dtype for d in decoded] == [np.uint16, np.uint16, np.uint8]
    plain = A.synthetic_image(77, *SC.SIZES[3], 1)
    item = OUT_W * OUT_H
    out = A.out_desc(channels=1, dtype="uint8", item_stride=item + GUARD)
    st = A.Stager(ctx, out, BATCH, A.STAGER_MASK)
    buf = Guarded(BATCH * out.item_stride, "pinned")
    try:
        with pytest.raises(A.AeonHipError, match="encoded pixel masks are decoded from PNG files only.*at idx 3"):
            st.stage_encoded(buf.ptr, 3, SC.window(0)[0], params[3])
        for i, f in enumerate(files):
            st.stage_encoded(buf.ptr, i, f, params[i])
        st.stage(buf.ptr, 3, plain, params[3])
        st.flush(buf.ptr)
        got = buf.items(BATCH, out.item_stride, item)
        for i, m in enumerate(decoded + [plain]):
            want = _mask16_reference(m, params[i], out)
            assert np.array_equal(got[i], want.reshape(-1)), i
        dev, host = _expected_counts(files, mask=True)
        assert st.last_decode() == dict(launches=1, device=dev, host=host, pixels=1)
        assert sum(dev.values()) > 0 and st.last_launch()["src_zero_copy"] == 0
    finally:
        st.close()
        buf.free()


def test_mixed_window_out_of_order(ctx, params):
    """One batch of 8 holding stage() and stage_encoded() records, two of the latter decoded by the calling thread
    (a noise PNG, an ASCII PPM), their idx staged out of order from 4 threads."""
    files = list(SC.window(1))
    files[5] = SC.image_file("ppm_p3", 1005, *SC.SIZES[5])
    assert [A.encoded_info(f)["device_route"] for f in (files[4], files[5])] == [False, False]
    decoded = [SC.decode_image(f) for f in files]
    recs = [decoded[i] if i in (1, 6) else files[i] for i in range(8)]  # two arrive decoded
    out = _out()
    st = A.Stager(ctx, out, 8)
    buf = Guarded(8 * out.item_stride, "pageable")
    order = list(range(8))
    random.Random(3).shuffle(order)
    assert order != sorted(order)
    try:
        def one(i):
            (st.stage_encoded if isinstance(recs[i], bytes) else st.stage)(buf.ptr, i, recs[i], params[i])
        with ThreadPoolExecutor(max_workers=4) as pool:
            list(pool.map(one, order))
        st.flush(buf.ptr)
        _assert_items(buf.items(8, out.item_stride, ITEM), _reference(decoded, params, out), "mixed")
        dev, host = _expected_counts([r for r in recs if isinstance(r, bytes)])
        assert st.last_decode() == dict(launches=1, device=dev, host=host, pixels=2)
        assert host == dict(jpeg=0, png=1, pixmap=1, tiff=0)
        assert st.last_launch() == dict(launches=1, src_zero_copy=0, out_direct=0, chunks=1, records=8)
    finally:
        st.close()


NWIN, PLAIN_WIN = 6, 3


@pytest.mark.parametrize("mode", ["flush", "overlap"])
@pytest.mark.parametrize("where", ["pinned", "pageable", "device"])
def test_output_kinds_and_window_reuse(ctx, params, where, mode):
    """Six windows with the same sizes and other pixels, so that a slot or a chunk reused shows a stale byte: flushed
    over one container, or overlapped over two (window k+1 staged and launched while window k runs).  Window
    PLAIN_WIN holds decoded records only and must report exactly what the stager reports without this feature."""
    out = _out()
    kind = A.STAGER_IMAGE | (A.STAGER_DEVICE_OUT if where == "device" else 0)
    st = A.Stager(ctx, out, BATCH, kind)
    ncont = 1 if mode == "flush" else 2
    conts = [[Guarded(BATCH * out.item_stride, where) for _ in range(NBATCHES)] for _ in range(ncont)]
    plain_info = dict(src_zero_copy=int(where == "pinned"), out_direct=int(where != "pageable"), chunks=1, records=8)
    coded_info = dict(plain_info, src_zero_copy=0)
    dev, host = _expected_counts(SC.window(0))

    def records(win):
        return SC.window_decoded(win) if win == PLAIN_WIN else SC.window(win)

    def launched(win):
        assert st.last_launch() == dict(plain_info if win == PLAIN_WIN else coded_info, launches=win + 1), win
        want = (dict(launches=win + 1, device=dict.fromkeys(NAMES, 0), host=dict.fromkeys(NAMES, 0), pixels=8)
                if win == PLAIN_WIN else dict(launches=win + 1, device=dev, host=host, pixels=0))
        assert st.last_decode() == want, win

    def check(win, bufs):
        want = _window_reference(win, params, out)
        for k, b in enumerate(bufs):
            _assert_items(b.items(BATCH, out.item_stride, ITEM), want[k * BATCH:(k + 1) * BATCH], (where, mode, win, k))
            b.refill()

    try:
        for win in range(NWIN):
            bufs = conts[win % ncont]
            _stage_window(st, bufs, records(win), params)
            if mode == "flush":
                for b in bufs:
                    st.flush(b.ptr)
                launched(win)
                check(win, bufs)
            else:
                for b in bufs:  # post_process: launch only
                    st.launch(b.ptr)
                launched(win)
                if win > 0:  # the consumer takes the window before
                    for b in conts[(win - 1) % 2]:
                        A.Stager.wait_buffer(b.ptr)
                    check(win - 1, conts[(win - 1) % 2])
        if mode == "overlap":
            for b in conts[(NWIN - 1) % 2]:
                st.wait(b.ptr)
            check(NWIN - 1, conts[(NWIN - 1) % 2])
    finally:
        st.close()
        for bufs in conts:
            for b in bufs:
                b.free()


def test_more_than_512_files(ctx):
    """520 JPEG files of 16 x 16 in one window (8 batches of 65): the launch splits them over two calls of the JPEG
    stage."""
    import oracle as O
    nb, bs, side = 8, 65, 16
    n = nb * bs
    files = [SC.image_file("jpeg420" if i % 3 else "jpeg_gray", 9000 + i, side, side) for i in range(n)]
    assert len(set(files)) > 500
    ps = [A.aug_params(crop_x=i % 5, crop_y=(i // 5) % 5, crop_w=12, crop_h=12, out_w=8, out_h=8, flip=i & 1) for i in range(n)]
    item = 3 * 8 * 8 * 4
    out = C.out_desc_for(dict(ETL, height=8, width=8), C.C2_AUG, item_stride=item + GUARD)
    st = A.Stager(ctx, out, bs)
    bufs = [Guarded(bs * out.item_stride, "pinned") for _ in range(nb)]
    try:
        def one(i):
            st.stage_encoded(bufs[i // bs].ptr, i % bs, files[i], ps[i])
        with ThreadPoolExecutor(max_workers=4) as pool:
            list(pool.map(one, range(n)))
        for b in bufs:
            st.flush(b.ptr)
        want = _reference([O.jpeg_decode(f, 3) for f in files], ps, out)
        for k, b in enumerate(bufs):
            _assert_items(b.items(bs, out.item_stride, item), want[k * bs:(k + 1) * bs], ("batch", k))
        assert st.last_decode() == dict(launches=1, device=dict(jpeg=n, png=0, pixmap=0, tiff=0),
                                        host=dict.fromkeys(NAMES, 0), pixels=0)
    finally:
        st.close()
        for b in bufs:
            b.free()


def test_errors_leave_the_stager_usable(ctx, params):
    """A truncated header is refused at stage time with the parser's code and message and the idx, and that idx is
    then staged again; a flipped scan byte of a GPU-decoded JPEG comes back from the window's last wait as a device
    error.  The window after each is bit-exact."""
    out = _out()
    st = A.Stager(ctx, out, BATCH)
    bufs = [Guarded(BATCH * out.item_stride, "pinned") for _ in range(NBATCHES)]
    try:
        # window 0: a header error in mid-window
        files = SC.window(2)
        for i in (0, 1):
            st.stage_encoded(bufs[0].ptr, i, files[i], params[i])
        with pytest.raises(A.AeonHipError, match="JPEG: truncated marker segment, at idx 2") as e:
            st.stage_encoded(bufs[0].ptr, 2, files[2][:30], params[2])
        assert e.value.code == EINVAL
        with pytest.raises(A.AeonHipError, match="PNG: .*, at idx 3") as e:
            st.stage_encoded(bufs[0].ptr, 3, files[3][:20], params[3])
        assert e.value.code == EINVAL
        _stage_window(st, bufs, files, params, order=range(2, 8))
        for b in bufs:
            st.flush(b.ptr)
        want = _window_reference(2, params, out)
        for k, b in enumerate(bufs):
            _assert_items(b.items(BATCH, out.item_stride, ITEM), want[k * BATCH:(k + 1) * BATCH], ("after header error", k))
            b.refill()
        # window 1: corrupt entropy-coded data (tests/golden/jpeg_corrupt.npz, the file test_jpeg.py reports)
        bad = np.load(os.path.join(HERE, "golden", "jpeg_corrupt.npz"))["s411_q85__flip10.jpg"].tobytes()
        w, h, _ = A.jpeg_info(bad)
        files = list(SC.window(3))
        _stage_window(st, bufs, files[:5] + files[6:], params[:5] + params[6:], order=None)  # 7 records: idx 0..3, 0..2
        st.stage_encoded(bufs[1].ptr, 3, bad, A.aug_params(crop_x=0, crop_y=0, crop_w=w, crop_h=h, out_w=OUT_W, out_h=OUT_H))
        st.flush(bufs[0].ptr)
        with pytest.raises(A.AeonHipError, match="JPEG entropy-coded data corrupt") as e:
            st.flush(bufs[1].ptr)  # the window's last wait
        assert e.value.code == EDEVICE
        for b in bufs:
            b.refill()
        # window 2
        _stage_window(st, bufs, SC.window(4), params)
        for b in bufs:
            st.flush(b.ptr)
        want = _window_reference(4, params, out)
        for k, b in enumerate(bufs):
            _assert_items(b.items(BATCH, out.item_stride, ITEM), want[k * BATCH:(k + 1) * BATCH], ("after device error", k))
        assert st.last_launch()["launches"] == 3
    finally:
        st.close()
        for b in bufs:
            b.free()
