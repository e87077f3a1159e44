"""What the video provider's tests share: a small MJPEG AVI writer, synthetic clips over Pillow-encoded
frames in the encodings the JPEG stage distinguishes (4:2:0, 4:4:4, grayscale, a restart interval), the
0xA5 prefill of an output buffer, and the video call over already decoded frames."""
import io
import os
import struct

import numpy as np

import aeon_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BB8 = os.path.join(ROOT, "tests", "golden", "video", "bb8.avi")
BB8_SIZES = [2944, 0, 2947, 2957, 2946, 2947]  # aeon's test/test_data/bb8.avi: 80x60, entry 1 an empty chunk
PREFILL = 0xA5
ENCODINGS = ("420", "444", "gray", "restart")


def bb8():
    return open(BB8, "rb").read()


def _chunk(cc, payload):
    return cc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _list(kind, payload):
    return b"LIST" + struct.pack("<I", 4 + len(payload)) + kind + payload


def write_avi(frames, width, height, flags=0x10, handler=b"MJPG", index=True, junk=True, index_offsets=None,
              chunk_sizes=None):
    """An AVI file over `frames` (JPEG files as bytes; b"" = an empty chunk): hdrl / avih with `flags`, one
    strl (vids / `handler`), an optional JUNK, movi with 00dc chunks, idx1 with offsets relative to the movi
    fourcc.  index_offsets / chunk_sizes: {frame: value} overrides of an index entry's offset / a chunk
    header's size (for the refusal tests)."""
    n = len(frames)
    avih = struct.pack("<14I", 40000, 0, 0, flags, n, 0, 1, 0, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4s10I4h", b"vids", handler, 0, 0, 0, 1, 25, 0, n, 0, 0, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    movi, entries = b"", []
    for i, f in enumerate(frames):
        off = 4 + len(movi)  # from the movi fourcc
        c = _chunk(b"00dc", f)
        if chunk_sizes and i in chunk_sizes:
            c = c[:4] + struct.pack("<I", chunk_sizes[i]) + c[8:]
        movi += c
        entries.append((b"00dc", 0x10, (index_offsets or {}).get(i, off), len(f)))
    body = hdrl + (_chunk(b"JUNK", b"\0" * 12) if junk else b"") + _list(b"movi", movi)
    if index:
        body += _chunk(b"idx1", b"".join(struct.pack("<4sIII", *e) for e in entries))
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"AVI " + body


def picture(index, w, h):
    """A smooth colour picture with some texture, HWC uint8 RGB (what a camera frame looks like to a JPEG
    encoder: noise alone would not exercise the DC prediction or end-of-block runs)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    rng = np.random.default_rng(1000 + index)
    base = np.stack([127 + 120 * np.sin((x + 3 * index) / (5 + index % 3)), 127 + 120 * np.cos((y - index) / 7),
                     (x * y + 31 * index) % 255], -1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(img, encoding, quality=88):
    """One Pillow-encoded JPEG file of an RGB picture in one of ENCODINGS."""
    from PIL import Image
    buf = io.BytesIO()
    if encoding == "gray":
        Image.fromarray(img[..., 1], "L").save(buf, "JPEG", quality=quality)
    else:
        kw = dict(subsampling=0 if encoding == "444" else 2)
        if encoding == "restart":
            kw["restart_marker_blocks"] = 2
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def synthetic_avi(seed, n_frames, w, h, encoding, empty=()):
    """An AVI of n_frames frames of w x h in `encoding`; frames listed in `empty` are empty chunks."""
    frames = [b"" if i in empty else encode(picture(97 * seed + i, w, h), encoding) for i in range(n_frames)]
    return write_avi(frames, w, h)


def prefill(nbytes):
    """A device buffer of nbytes, every byte PREFILL: what a call does not write stays visible."""
    import torch
    return torch.full((nbytes,), PREFILL, dtype=torch.uint8, device="cuda")


def hip_video(ctx, clips, counts, params, max_frames, out_w, out_h, item_stride, dst=None):
    """aeon_hip_video_batch over decoded frames: clips[i] = the BGR frames of clip i (counts[i] of them are
    read).  Returns the whole output buffer (prefilled with PREFILL unless `dst` is given) as numpy bytes."""
    import torch
    n = len(clips)
    images = [f for c in clips for f in c]
    arena, flat = A.pack_images(images)
    descs = (A.ImgDesc * (n * max_frames))()
    k = 0
    for i, c in enumerate(clips):
        for d, _ in enumerate(c):
            descs[i * max_frames + d] = flat[k]
            k += 1
    src = torch.from_numpy(arena).to("cuda")
    if dst is None:
        dst = prefill(n * item_stride)
    stream = torch.cuda.current_stream().cuda_stream
    ctx.video_batch(counts, descs, src.data_ptr(), params, max_frames, out_w, out_h, dst.data_ptr(), item_stride, stream)
    ctx.synchronize(stream)
    return dst.cpu().numpy()
