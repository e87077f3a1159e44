"""CPU: the MJPEG AVI demux (aeon_avi_frames, aeon_amd/csrc/avi_host.cpp) against the independent
restatement in tests/video_ref.py, its refusals, and the video / label ETL configs of the decoder (no device:
the decoder's context is made by its first window)."""
import struct

import numpy as np
import pytest

import aeon_amd as A
import oracle as O
from tests import video_cases as V
from tests import video_ref as R


def _synthetic():
    return {enc: V.synthetic_avi(k, n, 23, 17, enc, empty=(2,) if enc == "444" else ())
            for k, (enc, n) in enumerate(zip(V.ENCODINGS, (1, 3, 4, 7)))}


def test_bb8_frames_equal_reference():
    """aeon's test/test_data/bb8.avi: six index entries, entry 1 an empty chunk, 80 x 60."""
    data = V.bb8()
    frames, w, h = A.avi_frames(data)
    assert (frames, w, h) == R.demux(data)
    assert [n for _, n in frames] == V.BB8_SIZES and (w, h) == (80, 60)
    for off, n in frames:
        assert n == 0 or data[off:off + 2] == b"\xff\xd8"  # every non-empty frame is a JPEG file
    assert A.avi_frames(data, cap=4)[0] == frames[:4]


def test_bb8_frames_decode_like_pillow():
    """The oracle's JPEG decoder (the GPU tests' reference for the frames) against Pillow on bb8's frames."""
    import io

    from PIL import Image
    data = V.bb8()
    for off, n in R.demux(data)[0]:
        if n:
            want = np.asarray(Image.open(io.BytesIO(data[off:off + n])).convert("RGB"))[..., ::-1]
            assert np.array_equal(O.jpeg_decode(data[off:off + n], 3), want)


@pytest.mark.parametrize("enc", V.ENCODINGS)
def test_synthetic_files_equal_reference(enc):
    data = _synthetic()[enc]
    frames, w, h = A.avi_frames(data)
    assert (frames, w, h) == R.demux(data) and (w, h) == (23, 17)
    assert len(frames) == dict(zip(V.ENCODINGS, (1, 3, 4, 7)))[enc]
    for off, n in frames:
        if n:
            assert A.jpeg_info(data[off:off + n])[:2] == (23, 17)
    if enc == "444":
        assert frames[2][1] == 0
    # the writer's options do not move the frames' bytes relative to each other
    plain = V.write_avi([data[o:o + n] for o, n in frames], 23, 17, junk=False)
    assert [n for _, n in A.avi_frames(plain)[0]] == [n for _, n in frames]


def _refused(data, message):
    with pytest.raises(A.AeonHipError) as e:
        A.avi_frames(data)
    assert e.value.code == A.AEON_HIP_EINVAL and message in str(e.value), str(e.value)
    with pytest.raises(R.NotAvi):
        R.demux(data)


def test_refusals():
    f = [V.encode(V.picture(i, 16, 16), "420") for i in range(3)]
    good = V.write_avi(f, 16, 16)
    assert len(A.avi_frames(good)[0]) == 3
    _refused(b"", "not a RIFF AVI file")
    _refused(b"RIFX" + good[4:], "not a RIFF AVI file")
    _refused(good[:8] + b"WAVE" + good[12:], "not a RIFF AVI file")
    _refused(V.write_avi(f, 16, 16, handler=b"H264"), "no MJPG video stream")
    _refused(V.write_avi(f, 16, 16, flags=0), "Not a valid AVI file type")
    _refused(V.write_avi(f, 16, 16, index=False), "Not a valid AVI file type")
    _refused(good[:60], "Not a valid AVI file type")
    # a frame chunk that runs past the datum: its header says so, or the file ends inside it
    _refused(V.write_avi(f, 16, 16, chunk_sizes={1: 0xFFFFFFFF}), "runs past the datum")
    cut = A.avi_frames(good)[0][2][0] + 5  # inside the last frame: idx1 is gone too
    _refused(good[:cut], "Not a valid AVI file type")
    with pytest.raises(A.AeonHipError) as e:  # (here the reference repeats nothing: aeon has no frame yet)
        A.avi_frames(V.write_avi([b""] + f, 16, 16))
    assert e.value.code == A.AEON_HIP_EINVAL and "first frame is empty" in str(e.value)


def test_index_entries_outside_movi_are_dropped():
    """parseIndex keeps an entry only while movi_start + dwChunkOffset < movi_end (avi.cpp:160-170)."""
    f = [V.encode(V.picture(i, 16, 16), "420") for i in range(3)]
    good = V.write_avi(f, 16, 16)
    movi = good.index(b"movi")
    (size,) = struct.unpack_from("<I", good, movi - 4)
    for off in (size, size + 1000, 0xFFFFFFF0):  # at and past movi_end
        data = V.write_avi(f, 16, 16, index_offsets={1: off})
        frames = A.avi_frames(data)[0]
        assert frames == R.demux(data)[0] and len(frames) == 2
    # only the kept frames' chunks are read: a bad chunk past max_frame_count is never looked at
    data = V.write_avi(f, 16, 16, chunk_sizes={2: 0xFFFFFFFF})
    assert len(A.avi_frames(data, cap=2)[0]) == 2
    with pytest.raises(A.AeonHipError):
        A.avi_frames(data)


# ---- ETL configs ---------------------------------------------------------------------------------
FRAME = {"type": "image", "height": 24, "width": 32}
VIDEO_ETL = {"type": "video", "max_frame_count": 5, "frame": FRAME}
LABEL_ETL = {"type": "label", "binary": False}
AUG = {"type": "image", "frame": {"type": "image", "flip_enable": True}}


def _decoder(etl, **extra):
    return A.Decoder(dict(batch_size=2, etl=etl, augmentation=[AUG], **extra))


def test_outputs_video_then_label():
    """video::config's shape {channels, max_frame_count, height, width} of frame.output_type
    (etl_video.hpp:55-57) and label's {1} of uint32_t (etl_label.hpp:40, 52), named through create_name."""
    d = _decoder([VIDEO_ETL, LABEL_ETL])
    assert d.n_inputs == 2
    assert [(o["name"], o["shape"], o["dtype"], o["item_bytes"]) for o in d.outputs] == [
        ("video", (3, 5, 24, 32), np.uint8, 3 * 5 * 24 * 32), ("label", (1,), np.int32, 4)]
    d = _decoder([dict(LABEL_ETL, name="y", output_type="int16_t"), dict(VIDEO_ETL, name="clip")])
    assert [(o["name"], o["shape"], o["item_bytes"]) for o in d.outputs] == [("y.label", (1,), 2),
                                                                            ("clip.video", (3, 5, 24, 32), 11520)]


@pytest.mark.parametrize("etl,code,message", [
    ({k: v for k, v in VIDEO_ETL.items() if k != "max_frame_count"}, A.AEON_HIP_EINVAL, "'max_frame_count' not set"),
    (dict(VIDEO_ETL, max_frames=3), A.AEON_HIP_EINVAL, "config element {max_frames} is not understood in video"),
    (dict(VIDEO_ETL, frame=dict(FRAME, channels=1)), A.AEON_HIP_EINVAL, "'channels' must be 3"),
    (dict(VIDEO_ETL, frame=dict(FRAME, output_type="float")), A.AEON_HIP_EUNSUPPORTED, "'output_type' must be uint8_t"),
    (dict(VIDEO_ETL, frame=dict(FRAME, hight=3)), A.AEON_HIP_EINVAL, "config element {hight} is not understood in image"),
    ({k: v for k, v in VIDEO_ETL.items() if k != "frame"}, A.AEON_HIP_ERUNTIME,
     "missing image config in json config: etl type 'video' without its 'frame' is outside the HIP image stage"),
    (dict(VIDEO_ETL, max_frame_count=0), A.AEON_HIP_EINVAL, "invalid max_frame_count"),
    (dict(LABEL_ETL, output_type="double"), A.AEON_HIP_EUNSUPPORTED, "8-byte 'output_type'"),
    (dict(LABEL_ETL, output_type="float16"), A.AEON_HIP_EINVAL, "'output_type' out of range"),
    (dict(LABEL_ETL, binry=True), A.AEON_HIP_EINVAL, "config element {binry} is not understood in label"),
])
def test_video_config_validation(etl, code, message):
    other = LABEL_ETL if etl.get("type") == "video" else VIDEO_ETL
    with pytest.raises(A.AeonHipError) as e:
        _decoder([etl, other])
    assert e.value.code == code and message in str(e.value), str(e.value)


def test_labels_alone_stay_outside_the_stage():
    """A config of label elements only has nothing for the device: refused, as before the providers existed;
    next to any device element the same label config is taken."""
    for etl in ([LABEL_ETL], [LABEL_ETL, dict(LABEL_ETL, name="b")]):
        with pytest.raises(A.AeonHipError) as e:
            _decoder(etl)
        assert e.value.code == A.AEON_HIP_ERUNTIME and "'label' on its own is outside the HIP image stage" in str(e.value)
    assert len(_decoder([LABEL_ETL, dict(FRAME)]).outputs) == 2
    assert len(_decoder([VIDEO_ETL, LABEL_ETL]).outputs) == 2


def test_record_elem_entries_refuse_video_configs():
    """aeon_decoder_decode / aeon_decoder_draw_params take aeon_record_elem, which has no byte size for
    an AVI datum or a label: AEON_HIP_EINVAL before anything runs."""
    img = np.zeros((24, 32, 3), np.uint8)
    for etl in ([VIDEO_ETL], [VIDEO_ETL, LABEL_ETL], [dict(FRAME), LABEL_ETL]):
        d = _decoder(etl)
        with pytest.raises(A.AeonHipError) as e:
            d.decode([tuple(img for _ in etl)])  # no bytes element: the aeon_record_elem entry
        assert e.value.code == A.AEON_HIP_EINVAL and "aeon_decoder_decode_encoded" in str(e.value)
        with pytest.raises(A.AeonHipError) as e:
            d.draw_params([(32, 24)])
        assert e.value.code == A.AEON_HIP_EINVAL
