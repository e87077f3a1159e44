"""GPU: the stager for provider::video (aeon_hip_stager_create_video, stager_clip.cpp): provide() hands over the
record's MJPEG AVI (stage_clip: the window's launch decodes the kept frames on the device) or its decoded frames
(stage_frames: pinned staging), and the window's launch makes one video call per batch.  The expected clip is always
tests/video_ref.py over the CPU oracle, byte for byte: the oracle restates the same integer arithmetic, so there is no
tolerance.  Every batch buffer is filled with 0xA5 and has an item stride of 3*D*H*W + 5, so the bytes between the
items and behind the batch are checked too; which path a window took is read back (last_launch / last_decode)."""
import ctypes
import functools
import io
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import aeon_amd as A
import oracle as O
from tests import helpers as H
from tests import video_cases as V
from tests import video_ref as R
from tests.buffers import Buffer

pytestmark = pytest.mark.gpu

EINVAL = -1
D, FW, FH = 5, 48, 40  # (the height is no multiple of the 4:2:0 MCU's 16 rows)
NB, BS = 2, 3
KEPT = (5, 2, 1)
AUG = {"type": "image", "scale": [0.5, 0.9], "flip_enable": True, "contrast": [0.7, 1.3]}
NAMES = A.FORMAT_NAMES
ZERO = dict.fromkeys(NAMES, 0)


class Filled(Buffer):
    """A batch buffer of n clips pre-filled with PREFILL, with 5 bytes between the items."""

    def __init__(self, n, item, where):
        self.n_items, self.item, self.stride = n, item, item + 5
        super().__init__(n * self.stride, where)
        self.refill()

    def refill(self):
        if self.where == "device":
            import torch
            self.t.fill_(V.PREFILL)
            torch.cuda.synchronize()  # (the stager's streams do not wait for torch's)
        elif self.where == "pinned":
            ctypes.memset(self.ptr, V.PREFILL, self.n)
        else:
            self.a[:] = V.PREFILL

    def clips(self, shape):
        raw = np.array(self.bytes()).reshape(self.n_items, self.stride)
        assert (raw[:, self.item:] == V.PREFILL).all(), "bytes between the items were written"
        return raw[:, :self.item].reshape((self.n_items,) + shape)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _avis(enc, win=0):
    """NB x BS clips keeping 5, 2 and 1 frames: the first clip of batch 0 has an empty chunk in the middle, the first
    of batch 1 holds 7 frames, of which D are kept."""
    avis = []
    for b in range(NB):
        for i, kept in enumerate(KEPT):
            nf = 7 if (b, i) == (1, 0) else kept
            avis.append(V.synthetic_avi(100 * win + 10 * b + i, nf, FW, FH, enc, empty=(2,) if (b, i) == (0, 0) else ()))
    return avis


@functools.lru_cache(maxsize=None)
def _frames(enc, win=0):
    return [R.decoded_frames(a, D) for a in _avis(enc, win)]


@functools.lru_cache(maxsize=None)
def _params(out_w, out_h, win=0):
    ps = H.draw_params(AUG, [(FW, FH)] * (NB * BS), out_w, out_h, seed=11 + 3 * win)  # (seeds that draw a flip)
    assert any(p.flip for p in ps) and any(p.crop_w < FW for p in ps) and any(p.contrast != 1.0 for p in ps)
    return ps


@functools.lru_cache(maxsize=None)
def _want(enc, out_w, out_h, win=0):
    """The reference, computed once per case and shared: (NB * BS, 3, D, out_h, out_w)."""
    want = np.stack([R.clip_of(f, p, D, out_w, out_h) for f, p in zip(_frames(enc, win), _params(out_w, out_h, win))])
    want.setflags(write=False)
    return want


def _as_staged(frames):
    """A clip's decoded frames as stage_frames takes them: a repeated frame is None."""
    return [None if d and f is frames[d - 1] else f for d, f in enumerate(frames)]


def _n_files(enc, win=0):
    return sum(sum(1 for f in _as_staged(fr) if f is not None) for fr in _frames(enc, win))


def _stage(st, bufs, records, params, order=None, threads=4):
    """provide() from a pool: record i is idx i % BS of batch i // BS; bytes go through stage_clip, a list of frames
    through stage_frames."""
    bs = bufs[0].n_items

    def one(i):
        r = records[i]
        (st.stage_clip if isinstance(r, bytes) else st.stage_frames)(bufs[i // bs].ptr, i % bs, r, params[i])
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, order if order is not None else range(len(records))))


def _run(ctx, records, params, out_w, out_h, where="pinned", bs=BS):
    """One window through a stager of its own; returns (clips, last_launch, last_decode)."""
    item = 3 * D * out_h * out_w
    st = A.Stager.video(ctx, D, out_w, out_h, item + 5, bs, device_out=where == "device")
    bufs = [Filled(bs, item, where) for _ in range(len(records) // bs)]
    try:
        order = list(range(len(records)))
        random.Random(3).shuffle(order)
        _stage(st, bufs, records, params, order)
        for b in bufs:
            st.flush(b.ptr)
        got = np.concatenate([b.clips((3, D, out_h, out_w)) for b in bufs])
        return got, st.last_launch(), st.last_decode()
    finally:
        st.close()
        for b in bufs:
            b.free()


def _assert_clips(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for i in range(len(want)):
        assert np.array_equal(got[i], want[i]), (what, i, np.argwhere(got[i] != want[i])[:4])


# ---- 1. the second form, every encoding --------------------------------------------------------------
@pytest.mark.parametrize("out_w,out_h", [(20, 16), (7, 5)])
@pytest.mark.parametrize("enc", V.ENCODINGS)
def test_clips_every_encoding(ctx, enc, out_w, out_h):
    """Two batches of 3 clips of 5, 2 and 1 kept frames (pad frames and clip_pad; at 7 x 5 a plane is 35 bytes and the
    pad regions start at odd addresses), one clip with an empty chunk, one cut at D; crop, flip and contrast."""
    avis, params = _avis(enc), _params(out_w, out_h)
    assert [A.clip_info(a, D) for a in avis] == [(k, FW, FH) for k in KEPT] * NB
    assert R.demux(avis[0])[0][2][1] == 0 and len(R.demux(avis[BS])[0]) == 7
    got, launch, decode = _run(ctx, avis, params, out_w, out_h)
    want = _want(enc, out_w, out_h)
    assert np.array_equal(want[0][:, 2], want[0][:, 1]) and want[0][:, 1].any() and not want[1][:, 2:].any()
    _assert_clips(got, want, enc)
    n_files = 2 * sum(KEPT) - 1
    assert n_files == _n_files(enc)
    assert decode == dict(launches=1, device=dict(ZERO, jpeg=n_files), host=ZERO, pixels=0)
    assert launch == dict(launches=1, src_zero_copy=0, out_direct=1, chunks=0, records=NB * BS)


# ---- 2. the first form, and the two mixed ------------------------------------------------------------
def test_frames_and_mixed(ctx):
    enc, out_w, out_h = "420", 20, 16
    params, want = _params(out_w, out_h), _want(enc, out_w, out_h)
    staged = [_as_staged(f) for f in _frames(enc)]
    assert staged[0][2] is None
    got, launch, decode = _run(ctx, staged, params, out_w, out_h)
    _assert_clips(got, want, "frames")
    assert decode == dict(launches=1, device=ZERO, host=ZERO, pixels=_n_files(enc))
    assert launch == dict(launches=1, src_zero_copy=1, out_direct=1, chunks=1, records=NB * BS)  # pinned buffers
    # one batch of 6 alternating the forms by idx, staged out of order from the pool (as _run stages)
    mixed = [_avis(enc)[i] if i % 2 else staged[i] for i in range(NB * BS)]
    got, launch, decode = _run(ctx, mixed, params, out_w, out_h, where="pageable", bs=NB * BS)
    _assert_clips(got, want, "mixed")
    n_pix = sum(sum(f is not None for f in staged[i]) for i in range(0, NB * BS, 2))
    assert n_pix > 0 and decode == dict(launches=1, device=dict(ZERO, jpeg=_n_files(enc) - n_pix), host=ZERO, pixels=n_pix)
    assert launch == dict(launches=1, src_zero_copy=0, out_direct=0, chunks=1, records=NB * BS)


# ---- 3. the same bytes as the other front door -------------------------------------------------------
def test_same_bytes_as_the_video_call(ctx):
    enc, out_w, out_h = "444", 20, 16
    params, frames = _params(out_w, out_h), _frames(enc)
    got, _, _ = _run(ctx, _avis(enc), params, out_w, out_h, where="device")
    item = 3 * D * out_h * out_w
    for b in range(NB):
        sl = slice(b * BS, (b + 1) * BS)
        buf = V.hip_video(ctx, frames[sl], KEPT, params[sl], D, out_w, out_h, item + 5)
        call = buf.reshape(BS, item + 5)
        assert (call[:, item:] == V.PREFILL).all()
        assert np.array_equal(call[:, :item].reshape(got[sl].shape), got[sl]), b
    _assert_clips(got, _want(enc, out_w, out_h), "oracle")


# ---- 4. output kinds and window reuse ----------------------------------------------------------------
NWIN = 3


@pytest.mark.parametrize("mode", ["flush", "overlap"])
@pytest.mark.parametrize("where", ["pinned", "pageable", "device"])
def test_output_kinds_and_window_reuse(ctx, where, mode):
    """Three windows of other clips through one stager: flushed over one container, or overlapped over two -- window
    k+1 staged and launched before window k is waited for, by buffer alone.  Windows alternate the forms."""
    enc, out_w, out_h = "420", 20, 16
    item = 3 * D * out_h * out_w
    st = A.Stager.video(ctx, D, out_w, out_h, item + 5, BS, device_out=where == "device")
    ncont = 1 if mode == "flush" else 2
    conts = [[Filled(BS, item, where) for _ in range(NB)] for _ in range(ncont)]

    def records(win):
        return [_as_staged(f) for f in _frames(enc, win)] if win == 1 else _avis(enc, win)

    def launched(win):
        info = dict(launches=win + 1, src_zero_copy=int(where == "pinned" and win == 1), out_direct=int(where != "pageable"),
                    chunks=int(win == 1), records=NB * BS)
        assert st.last_launch() == info, win
        n = _n_files(enc, win)
        assert st.last_decode() == dict(launches=win + 1, device=dict(ZERO, jpeg=0 if win == 1 else n), host=ZERO,
                                        pixels=n if win == 1 else 0), win

    def check(win, bufs):
        got = np.concatenate([b.clips((3, D, out_h, out_w)) for b in bufs])
        _assert_clips(got, _want(enc, out_w, out_h, win), (where, mode, win))
        for b in bufs:
            b.refill()

    try:
        for win in range(NWIN):
            bufs = conts[win % ncont]
            _stage(st, bufs, records(win), _params(out_w, out_h, win))
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
                A.Stager.wait_buffer(b.ptr)
            check(NWIN - 1, conts[(NWIN - 1) % 2])
    finally:
        st.close()
        for bufs in conts:
            for b in bufs:
                b.free()


# ---- 5. more frames than one JPEG call ---------------------------------------------------------------
def test_more_than_512_frames(ctx):
    """Two batches of 20 clips x 14 frames of 16 x 16: 560 JPEG files in one window, above the 512 of one JPEG call.
    One clip is a progressive re-encode, so the JPEG stage's host entropy path runs inside a clip."""
    from PIL import Image
    nb, bs, d, side, out = 2, 20, 14, 16, 12
    pics = [V.encode(V.picture(k, side, side), V.ENCODINGS[k % 4]) for k in range(24)]

    def progressive(f):
        buf = io.BytesIO()
        Image.open(io.BytesIO(f)).convert("RGB").save(buf, "JPEG", quality=90, progressive=True)
        return buf.getvalue()

    prog = [progressive(pics[k]) for k in range(d)]
    assert not A.jpeg_host_stage(prog[0])[0] and A.jpeg_host_stage(pics[0])[0]
    clips = [prog if i == 7 else [pics[(5 * i + 3 * k) % 24] for k in range(d)] for i in range(nb * bs)]
    avis = [V.write_avi(c, side, side) for c in clips]
    params = [A.aug_params(crop_x=i % 4, crop_y=(i // 4) % 4, crop_w=12, crop_h=12, out_w=out, out_h=out, flip=i & 1)
              for i in range(nb * bs)]
    item = 3 * d * out * out
    st = A.Stager.video(ctx, d, out, out, item + 5, bs)
    bufs = [Filled(bs, item, "pinned") for _ in range(nb)]
    try:
        _stage(st, bufs, avis, params)
        for b in bufs:
            st.flush(b.ptr)
        got = np.concatenate([b.clips((3, d, out, out)) for b in bufs])
        decoded = {f: O.jpeg_decode(f, 3) for f in set(pics) | set(prog)}  # the clips share their pictures
        for i, c in enumerate(clips):
            want = R.clip_of([decoded[f] for f in c], params[i], d, out, out)
            assert np.array_equal(got[i], want), i
        assert st.last_decode() == dict(launches=1, device=dict(ZERO, jpeg=nb * bs * d), host=ZERO, pixels=0)
        assert st.last_launch()["records"] == nb * bs
    finally:
        st.close()
        for b in bufs:
            b.free()


# ---- 6. aeon's own bb8.avi ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_frames", [4, 8])
def test_bb8(ctx, max_frames):
    """Six frames of 80 x 60, frame 1 an empty chunk: max_frames 4 cuts it, 8 appends two zero frames."""
    data = V.bb8()
    assert A.clip_info(data, max_frames) == (min(6, max_frames), 80, 60)
    params = H.draw_params({"type": "image", "flip_enable": True, "scale": [0.6, 1.0]}, [(80, 60)] * 2, 32, 24, seed=41)
    item = 3 * max_frames * 24 * 32
    st = A.Stager.video(ctx, max_frames, 32, 24, item + 5, 2)
    buf = Filled(2, item, "pageable")
    try:
        st.stage_clip(buf.ptr, 0, data, params[0])
        st.stage_frames(buf.ptr, 1, R.decoded_frames(data, max_frames), params[1])
        st.flush(buf.ptr)
        got = buf.clips((3, max_frames, 24, 32))
        for i in range(2):
            want = R.expected_clip(data, params[i], max_frames, 32, 24)
            assert np.array_equal(got[i], want), i
            assert np.array_equal(want[:, 1], want[:, 0]) and want[:, 0].any()  # the repeated frame
            if max_frames == 8:
                assert not want[:, 6:].any() and want[:, 5].any()
        kept = min(6, max_frames)
        assert st.last_decode() == dict(launches=1, device=dict(ZERO, jpeg=kept - 1), host=ZERO, pixels=kept)
    finally:
        st.close()
        buf.free()


# ---- 7. errors leave the stager usable ---------------------------------------------------------------
def test_errors_leave_the_stager_usable(ctx):
    enc, out_w, out_h = "restart", 20, 16
    avis, params, want = _avis(enc), _params(out_w, out_h), _want(enc, out_w, out_h)
    item = 3 * D * out_h * out_w
    st = A.Stager.video(ctx, D, out_w, out_h, item + 5, BS)
    bufs = [Filled(BS, item, "pinned") for _ in range(NB)]
    small, big = V.encode(V.picture(1, FW, FH), "420"), V.encode(V.picture(2, 64, 48), "420")
    frames = _frames(enc)[1]
    other = A.aug_params(crop_x=0, crop_y=0, crop_w=FW, crop_h=FH, out_w=out_w + 1, out_h=out_h)
    refused = [
        (lambda: st.stage_clip(bufs[0].ptr, 1, V.write_avi([small, small, big], FW, FH), params[1]),
         "video: frame 2 is 64x48, the first frame 48x40, at idx 1"),
        (lambda: st.stage_clip(bufs[0].ptr, 1, b"RIFX" + avis[1][4:], params[1]), "avi: not a RIFF AVI file, at idx 1"),
        (lambda: st.stage_clip(bufs[0].ptr, 1, b"", params[1]), "received encoded video with size 0, at idx 1"),
        (lambda: st.stage_frames(bufs[0].ptr, 1, [frames[0]] * (D + 1), params[1]), "n_frames 6 outside [1, max_frames 5], at idx 1"),
        (lambda: st.stage_clip(bufs[0].ptr, 1, avis[1], other), "params' output size 21x16 is not the stager's 20x16, at idx 1"),
        (lambda: st.stage_frames(bufs[0].ptr, 1, frames, other), "params' output size 21x16 is not the stager's 20x16, at idx 1"),
        (lambda: st.stage(bufs[0].ptr, 1, frames[0], params[1]), "aeon_hip_stager_stage on a video stager"),
        (lambda: st.stage_encoded(bufs[0].ptr, 1, small, params[1]), "aeon_hip_stager_stage_encoded on a video stager"),
    ]
    image = A.Stager(ctx, A.out_desc(dtype="uint8", item_stride=3 * out_h * out_w), BS)
    refused += [
        (lambda: image.stage_clip(bufs[0].ptr, 1, avis[1], params[1]), "aeon_hip_stager_stage_clip on an image stager"),
        (lambda: image.stage_frames(bufs[0].ptr, 1, frames, params[1]), "aeon_hip_stager_stage_frames on an image stager"),
    ]
    try:
        _stage(st, bufs, avis, params, order=[0, 2, 3, 4, 5])
        for call, message in refused:
            with pytest.raises(A.AeonHipError) as e:
                call()
            assert e.value.code == EINVAL and message in str(e.value) and str(e.value).endswith(", at idx 1"), str(e.value)
        st.stage_clip(bufs[0].ptr, 1, avis[1], params[1])  # the idx is staged again
        for b in bufs:
            st.flush(b.ptr)
        _assert_clips(np.concatenate([b.clips((3, D, out_h, out_w)) for b in bufs]), want, "after the refusals")
        assert st.last_launch()["launches"] == 1
        # a stager the video call could not serve is refused when it is made
        with pytest.raises(A.AeonHipError, match="video: a clip item above 2\\^31 - 1 bytes") as e:
            A.Stager.video(ctx, 65535, 256, 256, 1 << 40, BS)
        assert e.value.code == -3
        with pytest.raises(A.AeonHipError, match="item_stride") as e:
            A.Stager.video(ctx, D, out_w, out_h, item - 1, BS)
        assert e.value.code == EINVAL
    finally:
        st.close()
        image.close()
        for b in bufs:
            b.free()
