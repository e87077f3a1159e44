"""Reference for the video provider's tests: an independent restatement of aeon's MJPEG AVI demux
(struct / numpy only, no call into the product library) and the expected clip over the CPU oracle.

demux(): MotionJpegCapture::parseRiff (aeon src/cap_mjpeg_decoder.cpp:190-227) over AviMjpegStream
(src/avi.cpp:145-379): every RIFF AVI / AVIX list; hdrl -> avih (index flag 0x10, dwStreams, dwWidth /
dwHeight), one strl per stream, the first vids/MJPG stream giving the chunk id NNdc; an optional INFO list,
an optional JUNK; movi; idx1 at movi_start + movi_size; the frames are the idx1 entries of that id whose
movi_start + dwChunkOffset lies below movi_end, read through the chunk header at that position.  Sizes as
written, no even-padding.

expected_clip(): video::transformer + loader (src/etl_video.cpp:49-107): every kept frame decoded to BGR
and through transform_single_image with the one params set, an empty chunk repeating the previous frame
(cap_mjpeg_decoder.cpp:138-141), zero frames appended, stacked channel x frame x height x width."""
import struct

import numpy as np

import oracle as O
from tests import helpers as H


class NotAvi(ValueError):
    pass


class _In:
    """aeon's istream over the datum: a read past the end fails, and the failure sticks."""

    def __init__(self, data):
        self.d, self.pos, self.ok = data, 0, True

    def read(self, fmt):
        n = struct.calcsize(fmt)
        if not self.ok or self.pos + n > len(self.d):
            self.ok = False
            return None
        v = struct.unpack_from(fmt, self.d, self.pos)
        self.pos += n
        return v

    def seek(self, pos):
        if self.ok:
            self.pos = pos


def _rest(size):
    return (size - 4) & 0xFFFFFFFF  # RiffList::m_size counts the list type already read (uint32 arithmetic)


def _parse_list(s, frames):
    """One AVI / AVIX list; returns (width, height) of its main header, or None."""
    v = s.read("<4sI4s")
    if v is None or v[0] != b"LIST" or v[2] != b"hdrl":
        return None
    next_list = s.pos + _rest(v[1])
    v = s.read("<4sI")
    if v is None or v[0] != b"avih":
        return None
    next_strl = s.pos + v[1]
    avih = s.read("<14I")
    if avih is None:
        return None
    has_index, streams, width, height = bool(avih[3] & 0x10), avih[6], avih[8], avih[9]
    stream_id, found = None, False
    for i in range(min(streams, 256)):
        s.seek(next_strl)
        v = s.read("<4sI4s")
        if v is None or v[0] != b"LIST" or v[2] != b"strl":
            break
        next_strl = s.pos + _rest(v[1])
        found = False
        v = s.read("<4sI")
        if v is None or v[0] != b"strh":
            continue
        strh = s.read("<4s4s48x")
        if strh is None or strh[0] != b"vids" or strh[1] != b"MJPG":
            continue
        found = True
        if stream_id is None:
            stream_id = bytes([i // 10 + 48, i % 10 + 48]) + b"dc"
    if not found:
        return None
    s.seek(next_list)
    v = s.read("<4sI4s")
    if v is not None and v[0] == b"LIST" and v[2] == b"INFO":
        s.seek(s.pos + _rest(v[1]))
        v = s.read("<4sI4s")
    if v is not None and v[0] == b"JUNK":
        s.seek(s.pos + _rest(v[1]))
        v = s.read("<4sI4s")
    if v is None or v[0] != b"LIST" or v[2] != b"movi":
        return None
    movi_start = s.pos - 4
    movi_end = movi_start + v[1]
    if not has_index:
        return None
    s.seek(movi_start + 4 + _rest(v[1]))
    v = s.read("<4sI")
    if v is None or v[0] != b"idx1":
        return None
    end = s.pos + v[1]
    while s.ok and s.pos < end:
        e = s.read("<4sIII")
        if e is None:
            break
        if e[0] == stream_id and movi_start + e[2] < movi_end:
            frames.append(movi_start + e[2])
    return width, height


def demux(data):
    """(frames, width, height): frames = [(offset, size)] of the chunks' data.  NotAvi when aeon finds no
    frame ("Not a valid AVI file type") or a frame's chunk does not lie inside the datum."""
    data = bytes(data)
    s, positions, size = _In(data), [], None
    while s.ok:
        v = s.read("<4sI4s")
        if v is None or v[0] != b"RIFF" or v[2] not in (b"AVI ", b"AVIX"):
            break
        next_riff = s.pos + _rest(v[1])
        got = _parse_list(s, positions)
        if got is not None and positions:
            size = got
        s.seek(next_riff)
    if not positions:
        raise NotAvi("Not a valid AVI file type")
    frames = []
    for p in positions:
        if p + 8 > len(data):
            raise NotAvi("frame chunk past the datum")
        (n,) = struct.unpack_from("<I", data, p + 4)
        if p + 8 + n > len(data):
            raise NotAvi("frame chunk past the datum")
        frames.append((p + 8, n))
    return frames, size[0], size[1]


def decoded_frames(data, max_frames):
    """The first min(count, max_frames) frames as BGR arrays, an empty chunk repeating the previous frame."""
    frames, _, _ = demux(data)
    out = []
    for off, n in frames[:max_frames]:
        out.append(O.jpeg_decode(data[off:off + n], 3) if n else out[-1])
    return out


def clip_of(frames, params, max_frames, out_w, out_h):
    """video::transformer + loader over decoded BGR frames: uint8 (3, max_frames, out_h, out_w)."""
    q = H.to_oracle_params(params)
    clip = np.zeros((3, max_frames, out_h, out_w), np.uint8)
    for d, f in enumerate(frames[:max_frames]):
        clip[:, d] = O.transform_image(f, q).transpose(2, 0, 1)
    return clip


def expected_clip(data, params, max_frames, out_w, out_h):
    return clip_of(decoded_frames(data, max_frames), params, max_frames, out_w, out_h)
