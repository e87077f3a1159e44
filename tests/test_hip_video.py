"""GPU: the video provider -- aeon_hip_video_batch (the image path's kernels over a clip's frames with the
clip's plane stride, and the clip_pad zero fill of aeon_amd/csrc/video_kernels.hip) and the video / label
providers of the decode stage -- against tests/video_ref.py over the CPU oracle, byte for byte: the oracle
restates the same integer arithmetic, so there is no tolerance.

Shapes are the smallest at which each piece can go wrong: output planes of 35, 60 and 256 bytes, so the pad
regions of a short clip start at odd, 4-aligned and 16-aligned addresses, with item strides that are no
multiple of anything; clips of 1, 2 and all frames; every route of the image path once (a clip's frames are
its records); aeon's own bb8.avi with its empty chunk; the documented (video, label) configuration at 16 x 12;
and one window with more frames (640) than one JPEG call takes (512)."""
import struct

import numpy as np
import pytest

import aeon_amd as A
import oracle as O
from tests import helpers as H
from tests import video_cases as V
from tests import video_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = A.Context(0)
    yield c
    c.close()


def _items(buf, n, item_stride, shape):
    nb = int(np.prod(shape))
    items = [buf[i * item_stride:i * item_stride + nb].reshape(shape) for i in range(n)]
    gaps = [buf[i * item_stride + nb:(i + 1) * item_stride] for i in range(n)]
    return items, gaps


# ---- 1. the video call on decoded frames ------------------------------------------------------------
@pytest.mark.parametrize("out_w,out_h", [(7, 5), (10, 6), (16, 16)])
def test_video_call_frames_pads_and_gaps(ctx, out_w, out_h):
    """n = 3 clips of D = 5 with 5, 2 and 1 frames of 23 x 17, crops and one flipped clip, item stride
    3*D*H*W + 5 in a buffer of 0xA5: kept frames equal the oracle, pad frames are zero, the 5 bytes after
    every item stay 0xA5.  Then all clips full: no pad launch, and no byte outside the frames changes."""
    D, n = 5, 3
    clips = [[A.synthetic_image(10 * i + d, 23, 17) for d in range(D)] for i in range(n)]
    params = [A.aug_params(crop_x=2, crop_y=1, crop_w=18, crop_h=14, out_w=out_w, out_h=out_h),
              A.aug_params(crop_x=0, crop_y=0, crop_w=23, crop_h=17, out_w=out_w, out_h=out_h, flip=1),
              A.aug_params(crop_x=5, crop_y=3, crop_w=12, crop_h=10, out_w=out_w, out_h=out_h)]
    stride = 3 * D * out_h * out_w + 5
    shape = (3, D, out_h, out_w)
    for counts in ((5, 2, 1), (5, 5, 5)):
        buf = V.hip_video(ctx, clips, counts, params, D, out_w, out_h, stride)
        items, gaps = _items(buf, n, stride, shape)
        for i in range(n):
            want = R.clip_of(clips[i][:counts[i]], params[i], D, out_w, out_h)
            assert not want[:, counts[i]:].any() and want[:, :counts[i]].any()
            assert np.array_equal(items[i], want), (counts, i, np.argwhere(items[i] != want)[:4])
            assert (gaps[i] == V.PREFILL).all(), (counts, i, gaps[i])


def test_video_call_refusals(ctx):
    import torch
    frames = [[A.synthetic_image(d, 23, 17) for d in range(2)]]
    p = [A.aug_params(crop_x=0, crop_y=0, crop_w=23, crop_h=17, out_w=8, out_h=8)]
    for kw, counts, message in ((dict(out_w=8, out_h=4), (2,), "differs from the frame size"),
                                (dict(out_w=8, out_h=8), (3,), "outside [0, max_frame_count]"),
                                (dict(out_w=8, out_h=8, stride=3 * 2 * 64 - 1), (2,), "does not fit item_stride")):
        with pytest.raises(A.AeonHipError) as e:
            V.hip_video(ctx, frames, counts, p, 2, kw["out_w"], kw["out_h"], kw.get("stride", 3 * 2 * 64))
        assert e.value.code == A.AEON_HIP_EINVAL and message in str(e.value), str(e.value)
    torch.cuda.synchronize()


# ---- 2. every route of the image path honours the plane stride -------------------------------------
PHOTO = {"type": "image", "scale": [0.5, 0.9], "contrast": [0.7, 1.3], "hue": [-20, 20], "lighting": [0.0, 0.1],
         "flip_enable": True}
ROUTES = {
    "contrast_hue_lighting": (PHOTO, {}),
    "contrast_two_launch": (PHOTO, {"AEON_HIP_RECORDS": "0"}),
    "planner": ({"type": "image", "scale": [0.5, 0.9], "flip_enable": True}, {"AEON_HIP_DIRECT": "0"}),
    "rotation": ({"type": "image", "scale": [0.5, 0.9], "angle": [30, 30]}, {}),
    "resize_short": ({"type": "image", "resize_short_size": 20, "crop_enable": True, "scale": [0.5, 0.9]}, {}),
    "cubic": ({"type": "image", "scale": [0.5, 0.9], "interpolation_method": "CUBIC"}, {}),
    "padding": ({"type": "image", "padding": 4, "crop_enable": False}, {}),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_honours_the_plane_stride(route, monkeypatch):
    """n = 2 clips of D = 3 frames of 32 x 24 -> 16 x 12 (one short, so the pad launch follows each route),
    equal to the per-frame oracle.  A context of its own per case: the route switches are read when it is
    made."""
    aug, env = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = A.Context(0)
    try:
        D, n, W, Ht = 3, 2, 16, 12
        clips = [[A.synthetic_image(50 + 10 * i + d, 32, 24) for d in range(D)] for i in range(n)]
        params = H.draw_params(aug, [(32, 24)] * n, W, Ht, seed=7)
        stride = 3 * D * Ht * W + 16
        buf = V.hip_video(c, clips, (3, 2), params, D, W, Ht, stride)
        items, gaps = _items(buf, n, stride, (3, D, Ht, W))
        for i, cnt in enumerate((3, 2)):
            want = R.clip_of(clips[i][:cnt], params[i], D, W, Ht)
            assert np.array_equal(items[i], want), (route, i, np.argwhere(items[i] != want)[:4])
            assert (gaps[i] == V.PREFILL).all()
    finally:
        c.close()


# ---- 3. bb8 through the decoder ---------------------------------------------------------------------
FRAME_AUG = {"type": "image", "flip_enable": True, "scale": [0.6, 1.0]}


@pytest.mark.parametrize("max_frames", [4, 8])
@pytest.mark.parametrize("frame_aug", [None, FRAME_AUG])
def test_bb8_through_the_decoder(max_frames, frame_aug):
    """aeon's bb8.avi (six frames of 80 x 60, frame 1 an empty chunk that repeats frame 0): max_frame_count 4
    cuts it, 8 appends two zero frames.  The param factory is built from augmentation[0]["frame"]
    (provider.cpp:483); the augmentation object itself needs its "type" (provider_factory.cpp:30-37)."""
    aug = {"type": "image"} if frame_aug is None else {"type": "image", "frame": frame_aug}
    etl = {"type": "video", "max_frame_count": max_frames, "frame": {"type": "image", "height": 24, "width": 32}}
    d = A.Decoder(dict(batch_size=2, random_seed=41, etl=[etl], augmentation=[aug]))
    f, states = A.ParamFactory(frame_aug or {"type": "image"}), A.seed_slots(41, 2)
    data = V.bb8()
    for window in range(2):
        params = [f.make_params(states[i:i + 1], 80, 60, 32, 24) for i in range(2)]
        (got,) = d.decode([(data,), (data,)])
        assert got.shape == (2, 3, max_frames, 24, 32) and got.dtype == np.uint8
        for i in range(2):
            want = R.expected_clip(data, params[i], max_frames, 32, 24)
            assert np.array_equal(got[i], want), (window, i)
            assert np.array_equal(want[:, 1], want[:, 0]) and want[:, 0].any()  # the repeated frame
            if max_frames == 8:
                assert not want[:, 6:].any() and want[:, 5].any()
    d.close()


# ---- 4. the documented (video, label) configuration, small ------------------------------------------
DOC_AUG = {"type": "image", "frame": FRAME_AUG}
DOC_VIDEO = {"type": "video", "max_frame_count": 4, "frame": {"type": "image", "height": 12, "width": 16}}
DOC_W, DOC_H, DOC_D = 16, 12, 4
LABELS = ["7", " 12", "-3", "0"]
LABEL_VALUES = [7, 12, -3, 0]


@pytest.fixture(scope="module")
def doc_window():
    """Four clips of 1, 3, 4 and 7 frames of 24 x 18, one per encoding (the 4:4:4 one with an empty chunk)."""
    return [V.synthetic_avi(20 + k, nf, 24, 18, enc, empty=(1,) if enc == "444" else ())
            for k, (enc, nf) in enumerate(zip(V.ENCODINGS, (1, 3, 4, 7)))]


def _doc_reference(avis, f, states):
    params = [f.make_params(states[i:i + 1], 24, 18, DOC_W, DOC_H) for i in range(len(avis))]
    return np.stack([R.expected_clip(a, p, DOC_D, DOC_W, DOC_H) for a, p in zip(avis, params)])


def test_documented_configuration_host_device_and_submit(doc_window):
    import torch
    cfg = dict(batch_size=4, random_seed=53, etl=[DOC_VIDEO, {"type": "label", "binary": False}], augmentation=[DOC_AUG])
    f, states = A.ParamFactory(FRAME_AUG), A.seed_slots(53, 4)
    wants = [_doc_reference(doc_window, f, states) for _ in range(2)]
    assert not np.array_equal(wants[0], wants[1])  # the engines moved on between the windows
    assert wants[0][1][:, 1].any() and not wants[0][1][:, 3:].any() and not wants[0][0][:, 1:].any()
    recs = list(zip(doc_window, LABELS))
    # host outputs, two decode calls
    d = A.Decoder(cfg)
    for k in range(2):
        out = d.decode_named(recs)
        assert np.array_equal(out["video"], wants[k]), k
        assert out["label"].dtype == np.int32 and out["label"].reshape(-1).tolist() == LABEL_VALUES
    d.close()
    # device outputs, the same two windows in flight through submit / wait
    d = A.Decoder(cfg)
    bufs = [[V.prefill(4 * o["item_bytes"]) for o in d.outputs] for _ in range(2)]
    enc = d.encoded(recs)
    d.submit(enc, [t.data_ptr() for t in bufs[0]], on_device=True)
    d.submit(enc, [t.data_ptr() for t in bufs[1]], on_device=True)
    d.wait()
    d.wait()
    for k in range(2):
        assert np.array_equal(bufs[k][0].cpu().numpy().reshape(wants[k].shape), wants[k]), k
        assert bufs[k][1].cpu().numpy().view(np.int32).tolist() == LABEL_VALUES
    d.close()
    torch.cuda.synchronize()


def test_documented_configuration_binary_labels_and_batch_major_false(doc_window):
    f, states = A.ParamFactory(FRAME_AUG), A.seed_slots(59, 4)
    want = _doc_reference(doc_window, f, states)
    blabels = [struct.pack("=i", v) for v in LABEL_VALUES]
    etl = [{"type": "label", "binary": True, "output_type": "int16_t"}, DOC_VIDEO]
    d = A.Decoder(dict(batch_size=4, random_seed=59, etl=etl, augmentation=[DOC_AUG]))
    out = d.decode_named(list(zip(blabels, doc_window)))
    assert np.array_equal(out["video"], want)
    assert out["label"].dtype == np.int16 and out["label"].reshape(-1).tolist() == LABEL_VALUES
    d.close()
    # batch_major=false: every output transposed per batch (dst[c * batch + r] = src[r * cols + c])
    d = A.Decoder(dict(batch_size=4, random_seed=59, batch_major=False, etl=etl, augmentation=[DOC_AUG]))
    out = d.decode_named(list(zip(blabels, doc_window)))
    assert np.array_equal(out["video"].reshape(-1), want.reshape(4, -1).T.reshape(-1))
    assert out["label"].reshape(-1).tolist() == LABEL_VALUES
    d.close()


# ---- 5. more frames than one JPEG call --------------------------------------------------------------
def test_more_frames_than_one_jpeg_call():
    """40 clips x 16 frames of 16 x 16: 640 JPEG files in one window, above the 512 of one JPEG call."""
    n, D = 40, 16
    pics = [V.encode(V.picture(k, 16, 16), V.ENCODINGS[k % 4]) for k in range(24)]
    avis = [V.write_avi([pics[(5 * i + 3 * d) % 24] for d in range(D)], 16, 16) for i in range(n)]
    etl = {"type": "video", "max_frame_count": D, "frame": {"type": "image", "height": 12, "width": 12}}
    d = A.Decoder(dict(batch_size=n, random_seed=61, etl=[etl], augmentation=[DOC_AUG]))
    f, states = A.ParamFactory(FRAME_AUG), A.seed_slots(61, n)
    params = [f.make_params(states[i:i + 1], 16, 16, 12, 12) for i in range(n)]
    (got,) = d.decode([(a,) for a in avis])
    decoded = {}  # JPEG file -> BGR frame: the clips share 24 pictures
    for i in range(n):
        files = [avis[i][o:o + s] for o, s in R.demux(avis[i])[0]]
        for b in files:
            if b not in decoded:
                decoded[b] = O.jpeg_decode(b, 3)
        want = R.clip_of([decoded[b] for b in files], params[i], D, 12, 12)
        assert np.array_equal(got[i], want), i
    assert len(decoded) == 24
    d.close()


# ---- 6. refusals leave the decoder usable -----------------------------------------------------------
def test_refusals_leave_the_decoder_usable(doc_window):
    cfg = dict(batch_size=4, random_seed=67, etl=[DOC_VIDEO, {"type": "label"}], augmentation=[DOC_AUG])
    d = A.Decoder(cfg)
    f, states = A.ParamFactory(FRAME_AUG), A.seed_slots(67, 4)
    good = list(zip(doc_window, LABELS))

    def good_window(what):
        want = _doc_reference(doc_window, f, states)
        out = d.decode_named(good)
        assert np.array_equal(out["video"], want), what
        assert out["label"].reshape(-1).tolist() == LABEL_VALUES, what

    good_window("first")
    small, big = V.encode(V.picture(1, 24, 18), "420"), V.encode(V.picture(2, 32, 24), "420")
    frames = [doc_window[2][o:o + s] for o, s in R.demux(doc_window[2])[0]]
    bad_windows = [
        ((V.write_avi([small, big, small], 24, 18), "1"), A.AEON_HIP_EINVAL, "frame 1 is 32x24, the first frame 24x18, at idx 2"),
        ((V.write_avi(frames, 24, 18, index=False), "1"), A.AEON_HIP_EINVAL, "Not a valid AVI file type, at idx 2"),
        ((b"", "1"), A.AEON_HIP_ERUNTIME, "received encoded video with size 0, at idx 2"),
        ((doc_window[2], "seven"), A.AEON_HIP_EINVAL, "at idx 2"),
        ((doc_window[2], "99999999999"), A.AEON_HIP_EINVAL, "out of range error, at idx 2"),
    ]
    for rec, code, message in bad_windows:
        bad = list(good)
        bad[2] = rec
        with pytest.raises(A.AeonHipError) as e:
            d.decode_named(bad)
        assert e.value.code == code and message in str(e.value), str(e.value)
        good_window(message)  # the failed window drew nothing: the engines are where the last good one left them
    d.close()
